// Python bindings for the ddlbench_amd CDNA4 kernels (gfx950).
// Compiled by hipcc via torch.utils.cpp_extension (PYTORCH_ROCM_ARCH=gfx950);
// HIP-native throughout — no CUDA names, no hipify.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <algorithm>
#include <stdexcept>
#include <unordered_map>
#include <vector>

#include "launchers.h"

using namespace ddlb;

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_gpu_contig(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the HIP device");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

bool is_bf16(const torch::Tensor& t) {
  return t.scalar_type() == at::kBFloat16;
}

template <typename T>
T* dptr(const torch::Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}

// Calls fn with a value-initialised element of x's dtype as a type tag:
// __hip_bfloat16 for bf16 tensors, float otherwise.
template <typename F>
auto dispatch_f32_bf16(bool bf16, F&& fn) {
  return bf16 ? fn(__hip_bfloat16{}) : fn(float{});
}
template <typename F>
auto dispatch_f32_bf16(const torch::Tensor& x, F&& fn) {
  return dispatch_f32_bf16(is_bf16(x), fn);
}

// Per-device cached workspace on `like`'s device: at least min_numel
// elements of dtype, (re)allocated at max(min_numel, grow_floor) when
// missing or too small. Contents are uninitialised unless `zeroed`.
using WsCache = std::unordered_map<int, torch::Tensor>;
torch::Tensor cached_ws(WsCache& cache, const torch::Tensor& like,
                        at::ScalarType dtype, int64_t min_numel,
                        int64_t grow_floor = 0, bool zeroed = false) {
  torch::Tensor& t = cache[(int)like.get_device()];
  if (!t.defined() || t.numel() < min_numel) {
    const int64_t cap = std::max(min_numel, grow_floor);
    const auto opt = like.options().dtype(dtype);
    t = zeroed ? torch::zeros({cap}, opt) : torch::empty({cap}, opt);
  }
  return t;
}

// 16-element zero page for the conv kernels' padding redirect (a fresh
// torch::zeros per call cost ~160 fill launches per training step).
torch::Tensor zero_page(const torch::Tensor& like) {
  static WsCache zp;
  return cached_ws(zp, like, at::kBFloat16, 16, 0, /*zeroed=*/true);
}

// BN reduce + finalize workspaces, sized by the bn_plan the launchers
// walk.
// sums: [S][2][C] partial slabs, fp32 or double by plan. Reduce-style
// kernels write plain per-block stores and the finalize kernel sums over
// S — no cross-block atomics (a C=64 layer at S~1500 slices serialized
// ~1500 f64 atomics per channel address), and no zeroing (every slab slot
// is written every call).
// part / tickets: the finalize kernel's second-level partials and its
// per-channel-chunk ticket words. The tickets are zeroed once, at
// allocation; each launch leaves them at zero.
struct BnWorkspace {
  torch::Tensor sums, part, tickets;
};
BnWorkspace bn_workspace(const torch::Tensor& x, const BnPlan& plan) {
  static WsCache ws_sums, ws_part, ws_tickets;
  BnWorkspace w;
  w.sums = cached_ws(ws_sums, x, at::kDouble, (plan.slab_bytes + 7) / 8,
                     1 << 18);
  w.part = cached_ws(ws_part, x, at::kDouble,
                     std::max<int64_t>(plan.part_doubles, 1), 1 << 16);
  w.tickets = cached_ws(ws_tickets, x, at::kInt, plan.cchunks, 1 << 10,
                        /*zeroed=*/true);
  return w;
}

const char* bn_name(BnReduce k) {
  return k == BnReduce::nchw ? "nchw"
         : k == BnReduce::nhwc_scalar ? "nhwc_scalar" : "nhwc_vec";
}
const char* bn_name(BnElt k) {
  return k == BnElt::fixed_channel ? "fixed_channel"
         : k == BnElt::vec ? "vec" : "scalar";
}
const char* bn_name(BnGate g) {
  return g == BnGate::none ? "none" : g == BnGate::y ? "y" : "mask";
}

bool bn_layout_ok(const torch::Tensor& t, bool nhwc) {
  return nhwc ? t.is_contiguous(at::MemoryFormat::ChannelsLast)
              : t.is_contiguous();
}

// is_cuda + bf16 + channels_last, the operand contract of the conv and
// pool bindings; `op` prefixes the dtype message
void check_conv_operand(const torch::Tensor& t, const char* name,
                        const char* op = "conv_igemm") {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16, op,
              ": bf16 HIP tensors only");
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), name,
              " must be channels_last");
}

int conv_out_size(int64_t H, int64_t pad, int64_t R, int64_t stride) {
  return (int)((H + 2 * pad - R) / stride + 1);
}

// geometry contract of the conv_igemm bindings and plan queries; checked
// first, so a violation raises before any size is derived or launched on
void check_conv_geometry(const char* op, int64_t N, int64_t H, int64_t W,
                         int64_t R, int64_t S, int64_t stride,
                         int64_t pad) {
  TORCH_CHECK(stride >= 1, op, ": stride must be >= 1");
  TORCH_CHECK(pad >= 0, op, ": pad must be >= 0");
  TORCH_CHECK(R >= 1 && S >= 1, op, ": kernel dims must be >= 1");
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1, op, ": empty input");
  TORCH_CHECK(H + 2 * pad >= R && W + 2 * pad >= S, op,
              ": kernel larger than the padded input");
}

// dy's (N, OH, OW) against the forward conv's geometry
void check_conv_dy(const char* op, const torch::Tensor& dy, int64_t N,
                   int64_t H, int64_t W, int64_t R, int64_t S,
                   int64_t stride, int64_t pad) {
  TORCH_CHECK(dy.size(0) == N, op, ": dy batch does not match x");
  TORCH_CHECK(dy.size(2) == conv_out_size(H, pad, R, stride) &&
                  dy.size(3) == conv_out_size(W, pad, S, stride),
              op, ": dy spatial dims do not match (H,W,R,S,stride,pad)");
}

torch::Tensor empty_nhwc(const torch::Tensor& like, int64_t N, int64_t C,
                         int64_t H, int64_t W) {
  return torch::empty({N, C, H, W}, like.options().memory_format(
                                        at::MemoryFormat::ChannelsLast));
}

}  // namespace

// ---- fused SGD --------------------------------------------------------
void fused_sgd(torch::Tensor ptr_params, torch::Tensor ptr_grads,
               torch::Tensor ptr_moms, torch::Tensor prefix, int64_t total,
               double lr, double momentum, double weight_decay,
               bool first_step, bool bf16) {
  check_gpu_contig(ptr_params, "ptr_params");
  dispatch_f32_bf16(bf16, [&](auto tag) {
    launch_fused_sgd<decltype(tag)>(
        dptr<uintptr_t>(ptr_params), dptr<uintptr_t>(ptr_grads),
        dptr<uintptr_t>(ptr_moms), dptr<int64_t>(prefix),
        (int)ptr_params.numel(), total, (float)lr, (float)momentum,
        (float)weight_decay, first_step, cur_stream());
  });
}

void fused_adam(torch::Tensor ptr_params, torch::Tensor ptr_grads,
                torch::Tensor ptr_ms, torch::Tensor ptr_vs,
                torch::Tensor prefix, int64_t total, double lr,
                double beta1, double beta2, double eps,
                double weight_decay, double bc1, double bc2,
                bool decoupled_wd, bool bf16) {
  check_gpu_contig(ptr_params, "ptr_params");
  dispatch_f32_bf16(bf16, [&](auto tag) {
    launch_fused_adam<decltype(tag)>(
        dptr<uintptr_t>(ptr_params), dptr<uintptr_t>(ptr_grads),
        dptr<uintptr_t>(ptr_ms), dptr<uintptr_t>(ptr_vs),
        dptr<int64_t>(prefix), (int)ptr_params.numel(), total, (float)lr,
        (float)beta1, (float)beta2, (float)eps, (float)weight_decay,
        (float)bc1, (float)bc2, decoupled_wd, cur_stream());
  });
}

// ---- fused BN + act (+residual) ---------------------------------------
std::vector<torch::Tensor> bn_act_fwd(
    torch::Tensor x, c10::optional<torch::Tensor> res, torch::Tensor gamma,
    torch::Tensor beta, c10::optional<torch::Tensor> running_mean,
    c10::optional<torch::Tensor> running_var, bool training, double momentum,
    double eps, int64_t act, bool nhwc) {
  TORCH_CHECK(x.is_cuda(), "x must be on the HIP device");
  TORCH_CHECK(x.dim() == 4, "x must be 4-D");
  TORCH_CHECK(bn_layout_ok(x, nhwc), "x layout mismatch");
  const int64_t N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  const BnPlan plan = bn_plan(N, C, HW, nhwc, (int)x.element_size(),
                              (int)act, training, /*masked=*/0);
  auto s = cur_stream();
  auto fopt = x.options().dtype(at::kFloat);
  torch::Tensor mean = torch::empty({C}, fopt);
  torch::Tensor invstd = torch::empty({C}, fopt);
  if (training) {
    const BnWorkspace ws = bn_workspace(x, plan);
    dispatch_f32_bf16(x, [&](auto tag) {
      using T = decltype(tag);
      launch_bn_stats<T>(plan, dptr<T>(x), ws.sums.data_ptr(), s);
    });
    launch_bn_finalize(
        plan, ws.sums.data_ptr(), dptr<double>(ws.part),
        dptr<unsigned>(ws.tickets), dptr<float>(mean), dptr<float>(invstd),
        running_mean ? dptr<float>(*running_mean) : nullptr,
        running_var ? dptr<float>(*running_var) : nullptr, (float)eps,
        (float)momentum, s);
  } else {
    TORCH_CHECK(running_mean && running_var,
                "eval mode needs running stats");
    mean.copy_(*running_mean);
    invstd.copy_((running_var->to(at::kFloat) + eps).rsqrt());
  }
  torch::Tensor y = torch::empty_like(x);
  // 1-bit activation mask for the backward (bf16 NHWC training path):
  // bit (i & 7) of byte i/8 gates element i's activation gradient.
  torch::Tensor msk;
  if (plan.writes_mask)
    msk = torch::empty({x.numel() / 8}, x.options().dtype(at::kByte));
  dispatch_f32_bf16(x, [&](auto tag) {
    using T = decltype(tag);
    launch_bn_apply<T>(
        plan, dptr<T>(x), res ? dptr<T>(*res) : nullptr, dptr<T>(y),
        dptr<float>(mean), dptr<float>(invstd), dptr<float>(gamma),
        dptr<float>(beta),
        msk.defined() ? msk.data_ptr<unsigned char>() : nullptr, s);
  });
  if (msk.defined()) return {y, mean, invstd, msk};
  return {y, mean, invstd};
}

// gate: a foreign 1-bit mask for an act == 0 layer whose dy is the shortcut
// gradient of a residual join, handed over ungated: the join's ReLU mask
// (numel/8 bytes, the fused apply's bit order). dy' = dy * bit is formed in
// fp32 inside the masked reduce and dx kernels, which take the act code
// from the gate, not from the layer, so the results equal those on a
// materialised bf16(dy * bit) bit for bit.
std::vector<torch::Tensor> bn_act_bwd(torch::Tensor dy,
                                      c10::optional<torch::Tensor> y_opt,
                                      torch::Tensor x, torch::Tensor mean,
                                      torch::Tensor invstd,
                                      torch::Tensor gamma, int64_t act,
                                      bool training, bool need_dres,
                                      bool nhwc,
                                      c10::optional<torch::Tensor> msk,
                                      c10::optional<torch::Tensor> gate) {
  TORCH_CHECK(dy.is_cuda(), "dy must be on the HIP device");
  if (gate) {
    TORCH_CHECK(act == 0 && !msk && !need_dres,
                "bn_act_bwd: a foreign gate is for an act == 0 layer with "
                "no mask and no residual of its own");
    TORCH_CHECK(is_bf16(x) && nhwc,
                "bn_act_bwd: a foreign gate needs bf16 NHWC tensors");
    TORCH_CHECK(gate->is_cuda() && gate->device() == dy.device() &&
                    gate->scalar_type() == at::kByte &&
                    gate->is_contiguous(),
                "bn_act_bwd: the gate must be a contiguous uint8 tensor on "
                "dy's device");
    // the masked ReLU-gated kernels read nothing of the act but the bits
    msk = gate;
    act = 1;
  }
  TORCH_CHECK(y_opt || msk,
              "bn_act_bwd needs y or the 1-bit activation mask");
  TORCH_CHECK(dy.sizes() == x.sizes(), "dy and x differ in size");
  TORCH_CHECK(dy.scalar_type() == x.scalar_type(),
              "dy and x differ in dtype");
  TORCH_CHECK(bn_layout_ok(dy, nhwc), "dy layout mismatch");
  const int64_t N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  TORCH_CHECK(!msk || msk->numel() == x.numel() / 8,
              "the activation mask must hold numel/8 bytes");
  // the fp32 kernels read y and never the mask
  TORCH_CHECK(is_bf16(x) || y_opt, "fp32 backward needs y");
  const BnPlan plan = bn_plan(N, C, HW, nhwc, (int)x.element_size(),
                              (int)act, training,
                              msk.has_value() && is_bf16(x));
  TORCH_CHECK(y_opt || (plan.reduce_gate != BnGate::y &&
                        plan.dx_gate != BnGate::y),
              "bn_act_bwd: no masked kernel for this shape, y is needed");
  TORCH_CHECK(!gate || (plan.reduce_gate == BnGate::mask &&
                        plan.dx_gate == BnGate::mask &&
                        plan.dx == BnElt::fixed_channel),
              "bn_act_bwd: no masked kernel for this shape, the foreign "
              "gate cannot be applied");
  auto s = cur_stream();
  auto fopt = x.options().dtype(at::kFloat);
  const BnWorkspace ws = bn_workspace(x, plan);
  torch::Tensor dgamma = torch::empty({C}, fopt);
  torch::Tensor dbeta = torch::empty({C}, fopt);
  torch::Tensor k = torch::empty({3, C}, fopt);
  torch::Tensor dx = torch::empty_like(x);
  torch::Tensor dres =
      need_dres ? torch::empty_like(x) : torch::Tensor();
  const unsigned char* mp =
      msk && is_bf16(x) ? msk->data_ptr<unsigned char>() : nullptr;
  dispatch_f32_bf16(x, [&](auto tag) {
    using T = decltype(tag);
    const T* yp = y_opt ? dptr<T>(*y_opt) : nullptr;
    launch_bn_bwd_reduce<T>(plan, dptr<T>(dy), yp, dptr<T>(x),
                            dptr<float>(mean), dptr<float>(invstd),
                            ws.sums.data_ptr(), mp, s);
    launch_bn_bwd_finalize(plan, ws.sums.data_ptr(), dptr<double>(ws.part),
                           dptr<unsigned>(ws.tickets), dptr<float>(gamma),
                           dptr<float>(invstd), dptr<float>(dgamma),
                           dptr<float>(dbeta), dptr<float>(k), training, s);
    launch_bn_bwd_dx<T>(plan, dptr<T>(dy), yp, dptr<T>(x), dptr<float>(mean),
                        dptr<float>(invstd), dptr<float>(k), dptr<T>(dx),
                        need_dres ? dptr<T>(dres) : nullptr, mp, s);
  });
  if (need_dres) return {dx, dgamma, dbeta, dres};
  return {dx, dgamma, dbeta};
}

py::dict bn_plan_py(int64_t N, int64_t C, int64_t HW, bool nhwc,
                    int64_t elsize, int64_t act, bool training,
                    bool masked) {
  TORCH_CHECK(N >= 1 && C >= 1 && HW >= 1, "bn_plan: empty input");
  TORCH_CHECK(elsize == 2 || elsize == 4, "bn_plan: elsize is 2 or 4");
  const BnPlan p = bn_plan(N, C, HW, nhwc, (int)elsize, (int)act, training,
                           masked);
  py::dict d;
  d["reduce"] = bn_name(p.reduce);
  d["cblocks"] = p.reduce_grid.x;
  d["S"] = p.reduce_grid.y;
  d["slab"] = p.slab_f32 ? "f32" : "f64";
  d["slab_bytes"] = p.slab_bytes;
  d["reduce_gate"] = bn_name(p.reduce_gate);
  d["cchunks"] = p.cchunks;
  d["Y"] = p.Y;
  d["part_doubles"] = p.part_doubles;
  d["apply"] = bn_name(p.apply);
  d["apply_grid"] = py::make_tuple(p.apply_grid.x, p.apply_grid.y);
  d["writes_mask"] = p.writes_mask != 0;
  d["dx"] = bn_name(p.dx);
  d["dx_grid"] = py::make_tuple(p.dx_grid.x, p.dx_grid.y);
  d["dx_gate"] = bn_name(p.dx_gate);
  return d;
}

// ---- cross entropy ----------------------------------------------------
std::vector<torch::Tensor> ce_fwd(torch::Tensor logits,
                                  torch::Tensor target) {
  check_gpu_contig(logits, "logits");
  const int64_t B = logits.size(0), K = logits.size(1);
  auto s = cur_stream();
  auto fopt = logits.options().dtype(at::kFloat);
  torch::Tensor lse = torch::empty({B}, fopt);
  torch::Tensor loss_sum = torch::zeros({1}, fopt);
  dispatch_f32_bf16(logits, [&](auto tag) {
    using T = decltype(tag);
    launch_ce_fwd<T>(dptr<T>(logits), dptr<int64_t>(target),
                     dptr<float>(lse), dptr<float>(loss_sum), B, K, s);
  });
  return {loss_sum, lse};
}

torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor target,
                     torch::Tensor lse, torch::Tensor gscale) {
  const int64_t B = logits.size(0), K = logits.size(1);
  auto s = cur_stream();
  torch::Tensor dx = torch::empty_like(logits);
  dispatch_f32_bf16(logits, [&](auto tag) {
    using T = decltype(tag);
    launch_ce_bwd<T>(dptr<T>(logits), dptr<int64_t>(target),
                     dptr<float>(lse), dptr<float>(gscale), dptr<T>(dx), B,
                     K, s);
  });
  return dx;
}

// ---- label-smoothed cross entropy with an ignore index -----------------
void check_ls_ce(const torch::Tensor& logits, const torch::Tensor& target) {
  check_gpu_contig(logits, "logits");
  check_gpu_contig(target, "target");
  TORCH_CHECK(logits.dim() == 2, "ls_ce: logits must be (R, K)");
  TORCH_CHECK(logits.scalar_type() == at::kFloat || is_bf16(logits),
              "ls_ce: logits must be fp32 or bf16");
  TORCH_CHECK(target.scalar_type() == at::kLong,
              "ls_ce: target must be int64");
  TORCH_CHECK(target.device() == logits.device(),
              "ls_ce: target must be on the logits' device");
  TORCH_CHECK(target.dim() == 1 && target.size(0) == logits.size(0),
              "ls_ce: target must be (R,)");
  TORCH_CHECK(logits.size(1) >= 1 && logits.size(1) < (1LL << 30),
              "ls_ce: K must be in [1, 2^30)");
  TORCH_CHECK(logits.size(0) < (1LL << 31), "ls_ce: too many rows");
}

// -> {loss (0-dim fp32), lse[R], n_valid (0-dim int64)}
std::vector<torch::Tensor> ls_ce_fwd(torch::Tensor logits,
                                     torch::Tensor target, double smoothing,
                                     int64_t ignore_index, bool mean) {
  check_ls_ce(logits, target);
  const int64_t R = logits.size(0), K = logits.size(1);
  auto s = cur_stream();
  auto fopt = logits.options().dtype(at::kFloat);
  // row 0: lse (returned), row 1: per-row losses (every slot written)
  torch::Tensor rows = torch::empty({2, R}, fopt);
  torch::Tensor loss = torch::empty({}, fopt);
  torch::Tensor n_valid = torch::empty({}, fopt.dtype(at::kLong));
  dispatch_f32_bf16(logits, [&](auto tag) {
    using T = decltype(tag);
    launch_ls_ce_fwd<T>(dptr<T>(logits), dptr<int64_t>(target),
                        dptr<float>(rows) + R, dptr<float>(rows),
                        dptr<float>(loss), dptr<int64_t>(n_valid), R, K,
                        (float)smoothing, ignore_index, mean, s);
  });
  return {loss, rows[0], n_valid};
}

torch::Tensor ls_ce_bwd(torch::Tensor logits, torch::Tensor target,
                        torch::Tensor lse, torch::Tensor n_valid,
                        torch::Tensor grad_out, double smoothing,
                        int64_t ignore_index, bool mean) {
  check_ls_ce(logits, target);
  check_gpu_contig(lse, "lse");
  check_gpu_contig(n_valid, "n_valid");
  check_gpu_contig(grad_out, "grad_out");
  const int64_t R = logits.size(0), K = logits.size(1);
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == R,
              "ls_ce_bwd: lse must be fp32 (R,)");
  TORCH_CHECK(n_valid.scalar_type() == at::kLong && n_valid.numel() == 1,
              "ls_ce_bwd: n_valid must be one int64");
  TORCH_CHECK(grad_out.scalar_type() == at::kFloat && grad_out.numel() == 1,
              "ls_ce_bwd: grad_out must be one fp32");
  TORCH_CHECK(lse.device() == logits.device() &&
                  n_valid.device() == logits.device() &&
                  grad_out.device() == logits.device(),
              "ls_ce_bwd: all tensors must be on the logits' device");
  auto s = cur_stream();
  torch::Tensor dx = torch::empty_like(logits);
  dispatch_f32_bf16(logits, [&](auto tag) {
    using T = decltype(tag);
    launch_ls_ce_bwd<T>(dptr<T>(logits), dptr<int64_t>(target),
                        dptr<float>(lse), dptr<int64_t>(n_valid),
                        dptr<float>(grad_out), dptr<T>(dx), R, K,
                        (float)smoothing, ignore_index, mean, s);
  });
  return dx;
}

// ---- fused Bahdanau attention score ------------------------------------
// Returns the mask's data pointer (nullptr without a mask).
const uint8_t* check_attn_score(const torch::Tensor& q,
                                const torch::Tensor& k,
                                const torch::Tensor& bias,
                                const torch::Tensor& vn,
                                const c10::optional<torch::Tensor>& mask) {
  check_gpu_contig(q, "q");
  check_gpu_contig(k, "k");
  check_gpu_contig(bias, "bias");
  check_gpu_contig(vn, "vn");
  TORCH_CHECK(q.scalar_type() == at::kFloat || is_bf16(q),
              "attn_score: q must be fp32 or bf16");
  TORCH_CHECK(k.scalar_type() == q.scalar_type() &&
                  bias.scalar_type() == q.scalar_type() &&
                  vn.scalar_type() == q.scalar_type(),
              "attn_score: q, k, bias and vn must share one dtype");
  TORCH_CHECK(k.device() == q.device() && bias.device() == q.device() &&
                  vn.device() == q.device(),
              "attn_score: all tensors must be on q's device");
  TORCH_CHECK(q.dim() == 3, "attn_score: q must be (B, Tq, H)");
  TORCH_CHECK(k.dim() == 3 && k.size(0) == q.size(0) &&
                  k.size(2) == q.size(2),
              "attn_score: k must be (B, Tk, H) with q's B and H");
  const int64_t B = q.size(0), H = q.size(2);
  TORCH_CHECK(H >= 1, "attn_score: H must be at least 1");
  TORCH_CHECK(bias.dim() == 1 && bias.size(0) == H,
              "attn_score: bias must be (H,) with q's H");
  TORCH_CHECK(vn.dim() == 1 && vn.size(0) == H,
              "attn_score: vn must be (H,) with q's H");
  TORCH_CHECK(B * ((H + 63) / 64) < (1LL << 31),
              "attn_score: B * ceil(H / 64) must be below 2^31");
  if (!mask.has_value()) return nullptr;
  const torch::Tensor& m = *mask;
  check_gpu_contig(m, "mask");
  TORCH_CHECK(m.scalar_type() == at::kBool || m.scalar_type() == at::kByte,
              "attn_score: mask must be bool or uint8");
  TORCH_CHECK(m.device() == q.device(),
              "attn_score: mask must be on q's device");
  TORCH_CHECK(m.dim() == 2 && m.size(0) == B && m.size(1) == k.size(1),
              "attn_score: mask must be (B, Tk)");
  return reinterpret_cast<const uint8_t*>(m.data_ptr());
}

torch::Tensor attn_score_fwd(torch::Tensor q, torch::Tensor k,
                             torch::Tensor bias, torch::Tensor vn,
                             c10::optional<torch::Tensor> mask) {
  const uint8_t* mp = check_attn_score(q, k, bias, vn, mask);
  const int64_t B = q.size(0), Tq = q.size(1), Tk = k.size(1), H = q.size(2);
  torch::Tensor out = torch::empty({B, Tq, Tk}, q.options());
  auto s = cur_stream();
  dispatch_f32_bf16(q, [&](auto tag) {
    using T = decltype(tag);
    launch_attn_score_fwd<T>(dptr<T>(q), dptr<T>(k), dptr<T>(bias),
                             dptr<T>(vn), mp, dptr<T>(out), B, Tq, Tk, H, s);
  });
  return out;
}

// -> {dq, dk, dbias, dvn}; need_q covers dq, dbias and dvn (one sweep makes
// all three), need_k covers dk. What is not needed comes back undefined.
std::vector<torch::Tensor> attn_score_bwd(torch::Tensor ds, torch::Tensor q,
                                          torch::Tensor k, torch::Tensor bias,
                                          torch::Tensor vn,
                                          c10::optional<torch::Tensor> mask,
                                          bool need_q, bool need_k) {
  const uint8_t* mp = check_attn_score(q, k, bias, vn, mask);
  check_gpu_contig(ds, "ds");
  const int64_t B = q.size(0), Tq = q.size(1), Tk = k.size(1), H = q.size(2);
  TORCH_CHECK(ds.scalar_type() == q.scalar_type() &&
                  ds.device() == q.device(),
              "attn_score_bwd: ds must have q's dtype and device");
  TORCH_CHECK(ds.dim() == 3 && ds.size(0) == B && ds.size(1) == Tq &&
                  ds.size(2) == Tk,
              "attn_score_bwd: ds must be (B, Tq, Tk)");
  torch::Tensor dq, dk, dbias, dvn, slab;
  if (need_q) {
    dq = torch::empty_like(q);
    dbias = torch::empty_like(bias);
    dvn = torch::empty_like(vn);
    slab = torch::empty({2, B, H}, q.options().dtype(at::kFloat));
    if (B == 0 || Tq == 0 || Tk == 0) {  // the kernels do not run
      dq.zero_();
      dbias.zero_();
      dvn.zero_();
    }
  }
  if (need_k) {
    dk = torch::empty_like(k);
    if (B == 0 || Tq == 0 || Tk == 0) dk.zero_();
  }
  auto s = cur_stream();
  dispatch_f32_bf16(q, [&](auto tag) {
    using T = decltype(tag);
    auto p = [](const torch::Tensor& t) {
      return t.defined() ? dptr<T>(t) : nullptr;
    };
    launch_attn_score_bwd<T>(
        dptr<T>(ds), dptr<T>(q), dptr<T>(k), dptr<T>(bias), dptr<T>(vn), mp,
        p(dq), p(dk), p(dbias), p(dvn),
        slab.defined() ? dptr<float>(slab) : nullptr, B, Tq, Tk, H, need_q,
        need_k, s);
  });
  return {dq, dk, dbias, dvn};
}

// ---- LSTM recurrence ----------------------------------------------------
// Shape, dtype, device and alignment of one tensor the step kernels read or
// write; bf16 rows are fetched as 16-byte fragments.
void check_lstm(const torch::Tensor& t, const char* name,
                at::ScalarType dtype, at::IntArrayRef shape,
                const torch::Tensor& like) {
  check_gpu_contig(t, name);
  TORCH_CHECK(t.scalar_type() == dtype, "lstm: ", name, " must be ",
              dtype == at::kFloat ? "fp32" : "bf16");
  TORCH_CHECK(t.device() == like.device(), "lstm: ", name,
              " must be on the first tensor's device");
  TORCH_CHECK(t.sizes() == shape, "lstm: ", name, " has shape ", t.sizes(),
              ", expected ", shape);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0,
              "lstm: ", name, " must be 16-byte aligned");
}

void check_lstm_dims(int64_t T, int64_t B, int64_t H) {
  TORCH_CHECK(T >= 1 && B >= 1, "lstm: T and B must be at least 1");
  TORCH_CHECK(H >= 8 && H % 8 == 0, "lstm: H must be a multiple of 8");
  TORCH_CHECK(((H + 15) / 16) * ((B + 15) / 16) < (1LL << 31),
              "lstm: ceil(H/16) * ceil(B/16) must be below 2^31");
}

// xproj (T, B, 4H) bf16, w_hh (4H, H) bf16, bias (4H) fp32, h0 (B, H) bf16,
// c0 (B, H) fp32 -> {y (T, B, H) bf16, cs (T, B, H) fp32, gates (T, B, 4H)
// bf16}; gates comes back undefined unless save_gates.
std::vector<torch::Tensor> lstm_fwd(torch::Tensor xproj, torch::Tensor w_hh,
                                    torch::Tensor bias,
                                    c10::optional<torch::Tensor> h0,
                                    c10::optional<torch::Tensor> c0,
                                    bool save_gates) {
  TORCH_CHECK(xproj.dim() == 3 && w_hh.dim() == 2,
              "lstm: xproj must be (T, B, 4H) and w_hh (4H, H)");
  const int64_t T = xproj.size(0), B = xproj.size(1), H = w_hh.size(1);
  check_lstm_dims(T, B, H);
  check_lstm(xproj, "xproj", at::kBFloat16, {T, B, 4 * H}, xproj);
  check_lstm(w_hh, "w_hh", at::kBFloat16, {4 * H, H}, xproj);
  check_lstm(bias, "bias", at::kFloat, {4 * H}, xproj);
  if (h0.has_value()) check_lstm(*h0, "h0", at::kBFloat16, {B, H}, xproj);
  if (c0.has_value()) check_lstm(*c0, "c0", at::kFloat, {B, H}, xproj);

  torch::Tensor y = torch::empty({T, B, H}, xproj.options());
  torch::Tensor cs =
      torch::empty({T, B, H}, xproj.options().dtype(at::kFloat));
  torch::Tensor gates;
  if (save_gates) gates = torch::empty({T, B, 4 * H}, xproj.options());

  using bf16 = __hip_bfloat16;
  const bf16* xp = dptr<bf16>(xproj);
  bf16* yp = dptr<bf16>(y);
  bf16* gp = save_gates ? dptr<bf16>(gates) : nullptr;
  float* cp = dptr<float>(cs);
  const bf16* h_prev = h0.has_value() ? dptr<bf16>(*h0) : nullptr;
  const float* c_prev = c0.has_value() ? dptr<float>(*c0) : nullptr;
  auto s = cur_stream();
  for (int64_t t = 0; t < T; ++t) {
    bf16* y_t = yp + t * B * H;
    float* c_t = cp + t * B * H;
    launch_lstm_step_fwd(h_prev, dptr<bf16>(w_hh), xp + t * B * 4 * H,
                         dptr<float>(bias), c_prev, y_t, c_t,
                         gp ? gp + t * B * 4 * H : nullptr, B, H, s);
    h_prev = y_t;
    c_prev = c_t;
  }
  return {y, cs, gates};
}

// dy (T, B, H) bf16, dh_T (B, H) bf16, dc_T (B, H) fp32, w_hh (4H, H) bf16,
// gates / cs as lstm_fwd returned them, c0 as given to it
// -> {dgates (T, B, 4H) bf16, dc0 (B, H) fp32}. W_hh is transposed once
// here, outside the loop, so the backward product reads K-contiguous rows.
std::vector<torch::Tensor> lstm_bwd(torch::Tensor dy,
                                    c10::optional<torch::Tensor> dh_T,
                                    c10::optional<torch::Tensor> dc_T,
                                    torch::Tensor w_hh, torch::Tensor gates,
                                    torch::Tensor cs,
                                    c10::optional<torch::Tensor> c0) {
  TORCH_CHECK(dy.dim() == 3, "lstm: dy must be (T, B, H)");
  const int64_t T = dy.size(0), B = dy.size(1), H = dy.size(2);
  check_lstm_dims(T, B, H);
  check_lstm(dy, "dy", at::kBFloat16, {T, B, H}, dy);
  check_lstm(w_hh, "w_hh", at::kBFloat16, {4 * H, H}, dy);
  torch::Tensor w_hh_t = w_hh.t().contiguous();
  check_lstm(gates, "gates", at::kBFloat16, {T, B, 4 * H}, dy);
  check_lstm(cs, "cs", at::kFloat, {T, B, H}, dy);
  if (dh_T.has_value()) check_lstm(*dh_T, "dh_T", at::kBFloat16, {B, H}, dy);
  if (dc_T.has_value()) check_lstm(*dc_T, "dc_T", at::kFloat, {B, H}, dy);
  if (c0.has_value()) check_lstm(*c0, "c0", at::kFloat, {B, H}, dy);

  torch::Tensor dgates = torch::empty({T, B, 4 * H}, dy.options());
  // dc ping-pong: step t writes half t & 1, so dc0 ends in half 0
  torch::Tensor dc = torch::empty({2, B, H}, cs.options());

  using bf16 = __hip_bfloat16;
  bf16* dgp = dptr<bf16>(dgates);
  float* dcp = dptr<float>(dc);
  const float* csp = dptr<float>(cs);
  auto s = cur_stream();
  for (int64_t t = T - 1; t >= 0; --t) {
    const bool last = t == T - 1;
    const float* c_prev = t > 0 ? csp + (t - 1) * B * H
                          : c0.has_value() ? dptr<float>(*c0) : nullptr;
    const float* dc_in =
        !last ? dcp + ((t + 1) & 1) * B * H
        : dc_T.has_value() ? dptr<float>(*dc_T) : nullptr;
    launch_lstm_step_bwd(
        last ? nullptr : dgp + (t + 1) * B * 4 * H, dptr<bf16>(w_hh_t),
        dptr<bf16>(dy) + t * B * H,
        last && dh_T.has_value() ? dptr<bf16>(*dh_T) : nullptr,
        dptr<bf16>(gates) + t * B * 4 * H, csp + t * B * H, c_prev, dc_in,
        dgp + t * B * 4 * H, dcp + (t & 1) * B * H, B, H, s);
  }
  return {dgates, dc.select(0, 0)};
}

// ---- MFMA implicit-GEMM conv (NHWC bf16) ------------------------------
// x: (N,C,H,W) logical, channels_last memory; w: (K,C,R,S) logical,
// channels_last memory (= (K,R,S,C) image). Returns channels_last y.
torch::Tensor conv_igemm_fwd(torch::Tensor x, torch::Tensor w,
                             int64_t stride, int64_t pad) {
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4, "conv_igemm: 4-D tensors only");
  check_conv_operand(x, "x", "conv_igemm");
  check_conv_operand(w, "w", "conv_igemm");
  TORCH_CHECK(w.device() == x.device(), "conv_igemm: w must be on x's device");
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int K = w.size(0), R = w.size(2), S = w.size(3);
  TORCH_CHECK(w.size(1) == C, "conv_igemm: weight C does not match x");
  TORCH_CHECK(C % 8 == 0, "conv_igemm fwd needs C % 8 == 0");
  TORCH_CHECK(K >= 1, "conv_igemm: empty weight");
  check_conv_geometry("conv_igemm", N, H, W, R, S, stride, pad);
  const int OH = conv_out_size(H, pad, R, stride);
  const int OW = conv_out_size(W, pad, S, stride);
  auto y = empty_nhwc(x, N, K, OH, OW);
  launch_conv_igemm(x.data_ptr(), w.data_ptr(), y.data_ptr(),
                    zero_page(x).data_ptr(), N, H, W, C, K, OH, OW, R, S,
                    (int)stride, (int)pad, /*dgrad=*/0, /*add=*/nullptr,
                    /*gate=*/nullptr, cur_stream());
  return y;
}

// dy: (N,K,OH,OW) channels_last; w_perm: (C,R,S,K) plain-contiguous
// memory (the autograd bridge permutes the weight once per backward
// call). Returns a freshly allocated channels_last dx.
// add: optional (N,C,H,W) channels_last bf16 tensor — the other gradient
// meeting dx at a residual join. It is only read; the result equals
// dgrad(dy) + add bit for bit (the accumulator is rounded to bf16, then
// one bf16 add). The kernels' epilogues do the add wherever every dx
// element is written exactly once; the one case that relies on a
// pre-zeroed dx (stride 2 with R==1 or S==1) adds after the launch.
// gate: optional, with add only: numel/8 bytes holding one bit per element
// of add in its channels_last memory order (bit i&7 of byte i/8, the mask
// the fused BN apply writes; C % 8 == 0). The addend is then
// bf16(float(add) * bit): what the BN backward at a residual join stores
// as its shortcut gradient, formed here from its dy and mask instead.
torch::Tensor conv_igemm_dgrad(torch::Tensor dy, torch::Tensor w_perm,
                               int64_t N, int64_t C, int64_t H, int64_t W,
                               int64_t stride, int64_t pad,
                               c10::optional<torch::Tensor> add,
                               c10::optional<torch::Tensor> gate) {
  TORCH_CHECK(dy.dim() == 4 && w_perm.dim() == 4,
              "conv_igemm: 4-D tensors only");
  check_conv_operand(dy, "dy", "conv_igemm");
  TORCH_CHECK(w_perm.is_cuda() && w_perm.scalar_type() == at::kBFloat16 &&
                  w_perm.device() == dy.device(),
              "conv_igemm: w_perm must be a bf16 tensor on dy's device");
  TORCH_CHECK(w_perm.is_contiguous(), "w_perm must be contiguous");
  if (add) {
    check_conv_operand(*add, "add", "conv_igemm");
    TORCH_CHECK(add->dim() == 4 && add->size(0) == N &&
                    add->size(1) == C && add->size(2) == H &&
                    add->size(3) == W,
                "add must have dx's shape (N,C,H,W)");
    TORCH_CHECK(add->device() == dy.device(),
                "add must be on dy's device");
  }
  if (gate) {
    TORCH_CHECK(add.has_value(), "conv_igemm: gate is legal only with add");
    TORCH_CHECK(C % 8 == 0, "conv_igemm: gate needs C % 8 == 0");
    TORCH_CHECK(gate->is_cuda() && gate->device() == dy.device() &&
                    gate->scalar_type() == at::kByte &&
                    gate->is_contiguous(),
                "conv_igemm: gate must be a contiguous uint8 tensor on dy's "
                "device");
    TORCH_CHECK(gate->numel() == N * C * H * W / 8,
                "conv_igemm: gate must hold dx.numel()/8 bytes");
  }
  const int K = dy.size(1), OH = dy.size(2), OW = dy.size(3);
  const int R = w_perm.size(1), S = w_perm.size(2);
  TORCH_CHECK(K % 8 == 0, "conv_igemm dgrad needs K % 8 == 0");
  TORCH_CHECK(C >= 1 && w_perm.size(0) == C && w_perm.size(3) == K,
              "conv_igemm: w_perm must be (C,R,S,K) for dx's C and dy's K");
  check_conv_geometry("conv_igemm", N, H, W, R, S, stride, pad);
  check_conv_dy("conv_igemm", dy, N, H, W, R, S, stride, pad);
  // stride-2 parity classes with R==1 or S==1 have pixel classes no tap
  // reaches — those dx entries must be zeros, so zero-init in that case
  // (zero_() after empty: torch::zeros does not honour the
  // channels_last memory_format request)
  auto dx = empty_nhwc(dy, N, C, H, W);
  const bool sparse = stride == 2 && (R == 1 || S == 1);
  if (sparse) dx.zero_();
  launch_conv_igemm(dy.data_ptr(), w_perm.data_ptr(), dx.data_ptr(),
                    zero_page(dy).data_ptr(), (int)N, (int)H, (int)W,
                    (int)C, K, OH, OW, R, S, (int)stride, (int)pad,
                    /*dgrad=*/1, add && !sparse ? add->data_ptr() : nullptr,
                    gate && !sparse ? gate->data_ptr() : nullptr,
                    cur_stream());
  if (add && sparse) {
    if (gate) {
      // no in-kernel add on this path: materialise the gated addend
      auto gated = torch::empty_like(*add);
      launch_gate_addend(add->data_ptr(), gate->data_ptr(),
                         gated.data_ptr(), add->numel() / 8, cur_stream());
      dx.add_(gated);
    } else {
      dx.add_(*add);
    }
  }
  return dx;
}

// x: (N,C,H,W) channels_last; dy: (N,K,OH,OW) channels_last.
// out_bf16 = false: fp32 dw in (K, R*S*C) memory = logical (K,C,R,S)
// channels_last after the python-side permute. out_bf16 = true: a bf16
// tensor of logical shape (K,C,R,S) with channels_last strides (the same
// (K,R,S,C) memory), each element the round-to-nearest-even bf16 of its
// fp32 sum, written by the kernels themselves.
static torch::Tensor conv_wgrad_impl(const torch::Tensor& x,
                                     const torch::Tensor& dy, int64_t R,
                                     int64_t S, int64_t stride, int64_t pad,
                                     bool out_bf16) {
  TORCH_CHECK(x.dim() == 4 && dy.dim() == 4, "conv_wgrad: 4-D tensors only");
  check_conv_operand(x, "x", "conv_wgrad");
  check_conv_operand(dy, "dy", "conv_wgrad");
  TORCH_CHECK(dy.device() == x.device(),
              "conv_wgrad: dy must be on x's device");
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int K = dy.size(1), OH = dy.size(2), OW = dy.size(3);
  TORCH_CHECK(C % 8 == 0 && K % 8 == 0,
              "conv_wgrad needs C %% 8 == 0 and K %% 8 == 0");
  TORCH_CHECK(K >= 1, "conv_wgrad: empty dy");
  check_conv_geometry("conv_wgrad", N, H, W, R, S, stride, pad);
  check_conv_dy("conv_wgrad", dy, N, H, W, R, S, stride, pad);
  // strides (R*S*C, 1, S*C, C): channels_last also where K, R or S is 1
  auto dw = out_bf16
                ? torch::empty({K, R, S, C}, x.options()).permute({0, 3, 1, 2})
                : torch::empty({K, R * S * C}, x.options().dtype(at::kFloat));
  // split-P partial-slab workspace: a fixed 8M floats (32 MB), the
  // launcher caps its split to fit
  static WsCache wgws;
  auto part = cached_ws(wgws, x, at::kFloat, kConvWgradPartCap);
  launch_conv_wgrad(x.data_ptr(), dy.data_ptr(),
                    out_bf16 ? nullptr : dw.data_ptr<float>(),
                    part.data_ptr<float>(), (long)part.numel(),
                    zero_page(x).data_ptr(), N, H, W, C, K, OH, OW, (int)R,
                    (int)S, (int)stride, (int)pad, cur_stream(),
                    out_bf16 ? dw.data_ptr() : nullptr);
  return dw;
}

torch::Tensor conv_igemm_wgrad(torch::Tensor x, torch::Tensor dy,
                               int64_t R, int64_t S, int64_t stride,
                               int64_t pad) {
  return conv_wgrad_impl(x, dy, R, S, stride, pad, /*out_bf16=*/false);
}

torch::Tensor conv_igemm_wgrad_bf16(torch::Tensor x, torch::Tensor dy,
                                    int64_t R, int64_t S, int64_t stride,
                                    int64_t pad) {
  return conv_wgrad_impl(x, dy, R, S, stride, pad, /*out_bf16=*/true);
}

// weight: bf16 logical (K,C,R,S), channels_last ((K,R,S,C) memory) or
// plain contiguous. Returns the contiguous (C,R,S,K) tensor the dgrad
// kernels read — a pure copy, equal to weight.permute(1,2,3,0).contiguous().
torch::Tensor conv_weight_dgrad_layout(torch::Tensor weight) {
  TORCH_CHECK(weight.is_cuda() && weight.scalar_type() == at::kBFloat16,
              "conv_weight_dgrad_layout: bf16 HIP tensors only");
  TORCH_CHECK(weight.dim() == 4,
              "conv_weight_dgrad_layout: weight must be 4-D (K,C,R,S)");
  const int64_t K = weight.size(0), C = weight.size(1);
  const int64_t R = weight.size(2), S = weight.size(3);
  TORCH_CHECK(K >= 8 && C >= 8 && K % 8 == 0 && C % 8 == 0 && R >= 1 &&
                  S >= 1,
              "conv_weight_dgrad_layout needs K % 8 == 0 and C % 8 == 0");
  const bool cl = weight.is_contiguous(at::MemoryFormat::ChannelsLast);
  TORCH_CHECK(cl || weight.is_contiguous(),
              "conv_weight_dgrad_layout: weight must be channels_last or "
              "contiguous");
  auto out = torch::empty({C, R, S, K}, weight.options().memory_format(
                                            at::MemoryFormat::Contiguous));
  const int64_t RS = R * S;
  if (cl)  // in[k][rs][c] -> out[c][rs][k], batch rs
    launch_weight_transpose(weight.data_ptr(), out.data_ptr(), RS, K, C,
                            RS * C, C, RS * K, K, cur_stream());
  else     // in[k][c*rs] -> out[c*rs][k]: one plain 2-D transpose
    launch_weight_transpose(weight.data_ptr(), out.data_ptr(), 1, K, C * RS,
                            C * RS, 0, K, 0, cur_stream());
  return out;
}

// ---- dispatch plans ---------------------------------------------------
// The launchers' own host decisions for a shape (no device needed): the
// functions below call exactly what launch_conv_igemm / launch_conv_wgrad
// call, so a test can assert which kernel variant a shape reaches.
// One dict per launch (up to four parity classes for stride-2 dgrad);
// honours DDLB_CONV_V2 like the launcher.
py::list conv_igemm_plan_py(int64_t N, int64_t C, int64_t H, int64_t W,
                            int64_t K, int64_t R, int64_t S, int64_t stride,
                            int64_t pad, bool dgrad) {
  check_conv_geometry("conv_igemm_plan", N, H, W, R, S, stride, pad);
  const ConvIgemmPlan plan = conv_igemm_plan(
      (int)N, (int)H, (int)W, (int)C, (int)K,
      conv_out_size(H, pad, R, stride), conv_out_size(W, pad, S, stride),
      (int)R, (int)S, (int)stride, (int)pad, dgrad ? 1 : 0);
  py::list out;
  for (int i = 0; i < plan.n; ++i) {
    const ConvIgemmLaunch& e = plan.e[i];
    py::dict d;
    d["structure"] = e.v2 ? "v2" : "v1";
    d["mode"] = e.mode;
    d["BM"] = e.bm;
    d["BN"] = e.bn;
    d["LIN"] = e.lin != 0;
    d["M"] = e.M;
    d["Nd"] = e.Nd;
    d["Kd"] = e.Kd;
    d["cls"] = py::make_tuple(e.cls_a, e.cls_b);
    d["taps"] = py::make_tuple(e.nr, e.ns);
    out.append(d);
  }
  return out;
}

py::dict conv_wgrad_plan_py(int64_t N, int64_t C, int64_t H, int64_t W,
                            int64_t K, int64_t R, int64_t S, int64_t stride,
                            int64_t pad) {
  check_conv_geometry("conv_wgrad_plan", N, H, W, R, S, stride, pad);
  const ConvWgradPlan pl = conv_wgrad_plan(
      (int)N, (int)C, (int)K, conv_out_size(H, pad, R, stride),
      conv_out_size(W, pad, S, stride), (int)R, (int)S, (int)stride,
      (int)pad, kConvWgradPartCap);
  py::dict d;
  d["TK"] = pl.tk;
  d["TR"] = pl.tr;
  d["ring"] = pl.ring;
  d["r1"] = pl.r1 != 0;
  d["split"] = pl.split;
  d["p_per"] = pl.p_per;
  d["steps"] = pl.steps;
  d["tail"] = pl.tail;
  d["psb"] = pl.psb;
  return d;
}

// ---- stem conv (C < 8, NHWC bf16) -------------------------------------
// Shape limits of csrc/conv_stem.hip; a violation raises before any
// launch.
static void check_stem_shape(int64_t C, int64_t K, int64_t R, int64_t S,
                             int64_t stride, int64_t pad) {
  TORCH_CHECK(C >= 1 && C <= 4, "conv_stem needs 1 <= C <= 4");
  TORCH_CHECK(R == S && (R == 3 || R == 5 || R == 7),
              "conv_stem needs a square 3x3, 5x5 or 7x7 kernel");
  TORCH_CHECK(stride == 1 || stride == 2, "conv_stem needs stride 1 or 2");
  TORCH_CHECK(pad >= 0 && pad <= R / 2, "conv_stem needs 0 <= pad <= R/2");
  TORCH_CHECK(K % 8 == 0 && K >= 8 && K <= 128,
              "conv_stem needs K % 8 == 0 and K <= 128");
}

// x: (N,C,H,W) channels_last; w: (K,C,R,R) channels_last (= (K, R*R*C)
// row-major memory). Returns channels_last y.
torch::Tensor conv_stem_fwd(torch::Tensor x, torch::Tensor w,
                            int64_t stride, int64_t pad) {
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4, "conv_stem: 4-D tensors only");
  check_conv_operand(x, "x", "conv_stem");
  check_conv_operand(w, "w", "conv_stem");
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int K = w.size(0), R = w.size(2), S = w.size(3);
  TORCH_CHECK(w.size(1) == C, "conv_stem: weight C mismatch");
  check_stem_shape(C, K, R, S, stride, pad);
  const int OH = conv_out_size(H, pad, R, stride);
  const int OW = conv_out_size(W, pad, S, stride);
  TORCH_CHECK(N >= 1 && H + 2 * pad >= R && W + 2 * pad >= S,
              "conv_stem: empty output");
  auto y = empty_nhwc(x, N, K, OH, OW);
  launch_conv_stem_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), N, H, W, C,
                       K, OH, OW, R, (int)stride, (int)pad, cur_stream());
  return y;
}

// x: (N,C,H,W) channels_last; dy: (N,K,OH,OW) channels_last. Returns fp32
// dw in (K, R*S*C) memory — the conv_igemm_wgrad convention.
torch::Tensor conv_stem_wgrad(torch::Tensor x, torch::Tensor dy, int64_t R,
                              int64_t S, int64_t stride, int64_t pad) {
  TORCH_CHECK(x.dim() == 4 && dy.dim() == 4, "conv_stem: 4-D tensors only");
  check_conv_operand(x, "x", "conv_stem");
  check_conv_operand(dy, "dy", "conv_stem");
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int K = dy.size(1), OH = dy.size(2), OW = dy.size(3);
  check_stem_shape(C, K, R, S, stride, pad);
  TORCH_CHECK(N >= 1 && dy.size(0) == N && OH >= 1 && OW >= 1 &&
                  OH == conv_out_size(H, pad, R, stride) &&
                  OW == conv_out_size(W, pad, S, stride),
              "conv_stem: dy shape does not match x");
  const int64_t total = (int64_t)K * R * S * C;
  auto dw = torch::empty({K, R * S * C}, x.options().dtype(at::kFloat));
  // per-block partial slabs, grown to need; every slab element the
  // combine reads is written by the same call
  static WsCache stws;
  auto part = cached_ws(stws, x, at::kFloat,
                        total * conv_stem_wgrad_chunks(N, OH, OW, K));
  launch_conv_stem_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr<float>(),
                         part.data_ptr<float>(), N, H, W, C, K, OH, OW,
                         (int)R, (int)stride, (int)pad, cur_stream());
  return dw;
}

// ---- NHWC max-pool ----------------------------------------------------
std::vector<torch::Tensor> maxpool_fwd(torch::Tensor x, int64_t k,
                                       int64_t stride, int64_t pad) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16,
              "maxpool: bf16 HIP tensors only");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "maxpool: x must be channels_last");
  const int64_t N = x.size(0), C = x.size(1);
  const int H = (int)x.size(2), W = (int)x.size(3);
  TORCH_CHECK(C % 8 == 0, "maxpool needs C %% 8 == 0");
  const int OH = (H + 2 * (int)pad - (int)k) / (int)stride + 1;
  const int OW = (W + 2 * (int)pad - (int)k) / (int)stride + 1;
  auto y = torch::empty({N, C, OH, OW},
                        x.options().memory_format(
                            at::MemoryFormat::ChannelsLast));
  auto idx = torch::empty({N * OH * OW * C},
                          x.options().dtype(at::kByte));
  launch_maxpool_fwd(x.data_ptr(), y.data_ptr(),
                     idx.data_ptr<unsigned char>(), N, C, H, W, OH, OW,
                     (int)k, (int)stride, (int)pad, cur_stream());
  return {y, idx};
}

torch::Tensor maxpool_bwd(torch::Tensor dy, torch::Tensor idx,
                          int64_t H, int64_t W, int64_t k,
                          int64_t stride, int64_t pad) {
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16,
              "maxpool: bf16 HIP tensors only");
  TORCH_CHECK(dy.is_contiguous(at::MemoryFormat::ChannelsLast),
              "maxpool: dy must be channels_last");
  const int64_t N = dy.size(0), C = dy.size(1);
  const int OH = (int)dy.size(2), OW = (int)dy.size(3);
  auto dx = torch::empty({N, C, H, W},
                         dy.options().memory_format(
                             at::MemoryFormat::ChannelsLast));
  launch_maxpool_bwd(dy.data_ptr(), idx.data_ptr<unsigned char>(),
                     dx.data_ptr(), N, C, (int)H, (int)W, OH, OW,
                     (int)k, (int)stride, (int)pad, cur_stream());
  return dx;
}

// ---- depthwise 3x3 ----------------------------------------------------
torch::Tensor dw3x3_fwd(torch::Tensor x, torch::Tensor w, int64_t stride,
                        bool nhwc) {
  TORCH_CHECK(x.is_cuda(), "x must be on the HIP device");
  check_gpu_contig(w, "w");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t OH = (H + 2 - 3) / stride + 1, OW = (W + 2 - 3) / stride + 1;
  auto s = cur_stream();
  torch::Tensor y = nhwc
      ? torch::empty({N, C, OH, OW}, x.options().memory_format(
            at::MemoryFormat::ChannelsLast))
      : torch::empty({N, C, OH, OW}, x.options());
  dispatch_f32_bf16(x, [&](auto tag) {
    using T = decltype(tag);
    launch_dw3x3_fwd<T>(dptr<T>(x), dptr<float>(w), dptr<T>(y), N, C, H, W,
                        OH, OW, (int)stride, nhwc, s);
  });
  return y;
}

std::vector<torch::Tensor> dw3x3_bwd(torch::Tensor x, torch::Tensor w,
                                     torch::Tensor dy, int64_t stride,
                                     bool need_dx, bool need_dw,
                                     bool nhwc) {
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t OH = dy.size(2), OW = dy.size(3);
  auto s = cur_stream();
  torch::Tensor dx, dwt;
  if (need_dx) {
    dx = torch::empty_like(x);
    dispatch_f32_bf16(x, [&](auto tag) {
      using T = decltype(tag);
      launch_dw3x3_bwd_dx<T>(dptr<T>(dy), dptr<float>(w), dptr<T>(dx), N, C,
                             H, W, OH, OW, (int)stride, nhwc, s);
    });
  }
  if (need_dw) {
    torch::Tensor acc = torch::zeros({C * 9}, x.options().dtype(at::kDouble));
    dispatch_f32_bf16(x, [&](auto tag) {
      using T = decltype(tag);
      launch_dw3x3_bwd_dw<T>(dptr<T>(x), dptr<T>(dy), dptr<double>(acc), N,
                             C, H, W, OH, OW, (int)stride, nhwc, s);
    });
    dwt = acc.to(at::kFloat).view({C, 1, 3, 3});
  }
  return {dx, dwt};
}

// ---- sequence utils (GNMT) --------------------------------------------
torch::Tensor revert_varlen(torch::Tensor x, torch::Tensor lengths) {
  check_gpu_contig(x, "x");
  TORCH_CHECK(x.dim() == 3, "x must be (T, B, F)");
  TORCH_CHECK(lengths.scalar_type() == at::kLong, "lengths must be int64");
  const int64_t T = x.size(0), B = x.size(1), F = x.size(2);
  auto out = torch::empty_like(x);
  auto s = cur_stream();
  dispatch_f32_bf16(x, [&](auto tag) {
    using E = decltype(tag);
    launch_revert_varlen<E>(dptr<E>(x), dptr<E>(out),
                            dptr<int64_t>(lengths), T, B, F, s);
  });
  return out;
}

torch::Tensor varlen_mask(torch::Tensor lengths, int64_t T) {
  TORCH_CHECK(lengths.is_cuda(), "lengths must be on the HIP device");
  const int64_t B = lengths.size(0);
  auto mask = torch::empty({T, B}, lengths.options().dtype(at::kByte));
  launch_varlen_mask(dptr<int64_t>(lengths), dptr<uint8_t>(mask), T, B,
                     cur_stream());
  return mask;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "ddlbench_amd gfx950 HIP kernels";
  m.def("fused_sgd", &fused_sgd, "fused multi-tensor SGD step");
  m.def("fused_adam", &fused_adam, "fused multi-tensor Adam/AdamW step");
  m.def("bn_act_fwd", &bn_act_fwd, "fused BN+act(+res) forward");
  m.def("bn_act_bwd", &bn_act_bwd, "fused BN+act(+res) backward",
        py::arg("dy"), py::arg("y"), py::arg("x"), py::arg("mean"),
        py::arg("invstd"), py::arg("gamma"), py::arg("act"),
        py::arg("training"), py::arg("need_dres"), py::arg("nhwc"),
        py::arg("msk"), py::arg("gate") = py::none());
  m.def("bn_plan", &bn_plan_py,
        "the dispatch plan the BN+act launchers walk (no device needed)",
        py::arg("N"), py::arg("C"), py::arg("HW"), py::arg("nhwc"),
        py::arg("elsize"), py::arg("act"), py::arg("training"),
        py::arg("masked"));
  m.def("maxpool_fwd", &maxpool_fwd, "NHWC bf16 max-pool forward");
  m.def("maxpool_bwd", &maxpool_bwd, "NHWC bf16 max-pool backward");
  m.def("conv_igemm_fwd", &conv_igemm_fwd,
        "NHWC bf16 MFMA implicit-GEMM conv forward");
  m.def("conv_igemm_dgrad", &conv_igemm_dgrad,
        "NHWC bf16 MFMA implicit-GEMM conv data-grad (+ optional addend)",
        py::arg("dy"), py::arg("w_perm"), py::arg("N"), py::arg("C"),
        py::arg("H"), py::arg("W"), py::arg("stride"), py::arg("pad"),
        py::arg("add") = py::none(), py::arg("gate") = py::none());
  m.def("conv_igemm_wgrad", &conv_igemm_wgrad,
        "NHWC bf16 MFMA implicit-GEMM conv weight-grad (fp32 out)");
  m.def("conv_igemm_wgrad_bf16", &conv_igemm_wgrad_bf16,
        "MFMA weight-grad straight to bf16 (K,C,R,S) channels_last",
        py::arg("x"), py::arg("dy"), py::arg("R"), py::arg("S"),
        py::arg("stride"), py::arg("pad"));
  m.def("conv_weight_dgrad_layout", &conv_weight_dgrad_layout,
        "bf16 weight (K,C,R,S) -> contiguous (C,R,S,K) for the dgrad kernels",
        py::arg("weight"));
  m.def("conv_igemm_plan", &conv_igemm_plan_py,
        "launches conv_igemm_fwd/dgrad make for a shape (host only)",
        py::arg("N"), py::arg("C"), py::arg("H"), py::arg("W"),
        py::arg("K"), py::arg("R"), py::arg("S"), py::arg("stride"),
        py::arg("pad"), py::arg("dgrad"));
  m.def("conv_wgrad_plan", &conv_wgrad_plan_py,
        "tile/split/steps conv_igemm_wgrad uses for a shape (host only)",
        py::arg("N"), py::arg("C"), py::arg("H"), py::arg("W"),
        py::arg("K"), py::arg("R"), py::arg("S"), py::arg("stride"),
        py::arg("pad"));
  m.def("conv_stem_fwd", &conv_stem_fwd,
        "NHWC bf16 MFMA stem conv (C < 8) forward");
  m.def("conv_stem_wgrad", &conv_stem_wgrad,
        "NHWC bf16 MFMA stem conv (C < 8) weight-grad (fp32 out)");
  m.def("ce_fwd", &ce_fwd, "cross-entropy forward");
  m.def("ce_bwd", &ce_bwd, "cross-entropy backward");
  m.def("ls_ce_fwd", &ls_ce_fwd,
        "label-smoothed cross-entropy forward (ignore index)");
  m.def("ls_ce_bwd", &ls_ce_bwd, "label-smoothed cross-entropy backward");
  m.def("attn_score_fwd", &attn_score_fwd,
        "fused Bahdanau attention score forward (B,Tq,Tk)", py::arg("q"),
        py::arg("k"), py::arg("bias"), py::arg("vn"),
        py::arg("mask") = py::none());
  m.def("attn_score_bwd", &attn_score_bwd,
        "fused Bahdanau attention score backward -> dq, dk, dbias, dvn",
        py::arg("ds"), py::arg("q"), py::arg("k"), py::arg("bias"),
        py::arg("vn"), py::arg("mask") = py::none(),
        py::arg("need_q") = true, py::arg("need_k") = true);
  m.def("lstm_fwd", &lstm_fwd,
        "LSTM recurrence forward: one native kernel per time step");
  m.def("lstm_bwd", &lstm_bwd,
        "LSTM recurrence backward: one native kernel per time step");
  m.def("revert_varlen", &revert_varlen,
        "reverse each batch element's valid time prefix (T,B,F)");
  m.def("varlen_mask", &varlen_mask, "valid-timestep mask (T,B) uint8");
  m.def("dw3x3_fwd", &dw3x3_fwd, "depthwise 3x3 forward");
  m.def("dw3x3_bwd", &dw3x3_bwd, "depthwise 3x3 backward");
}
