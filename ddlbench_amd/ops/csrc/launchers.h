// Host entry points of the kernel files, declared once. bindings.hip
// calls them; every .hip that defines one includes this header and
// defines it under its qualified name (ddlb::launch_x), so a definition
// whose signature drifts from the declaration does not compile.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddlb {

// ---- fused_sgd.hip ----------------------------------------------------
template <typename T>
void launch_fused_sgd(uintptr_t* params, uintptr_t* grads, uintptr_t* moms,
                      const int64_t* prefix, int n_tensors, int64_t total,
                      float lr, float momentum, float wd, int first_step,
                      hipStream_t stream);
template <typename T>
void launch_fused_adam(uintptr_t* params, uintptr_t* grads, uintptr_t* ms,
                       uintptr_t* vs, const int64_t* prefix, int n_tensors,
                       int64_t total, float lr, float beta1, float beta2,
                       float eps, float wd, float bc1, float bc2,
                       int decoupled, hipStream_t stream);

// ---- bn_act.hip -------------------------------------------------------
// Every dispatch decision of one BN+act layer, taken once by bn_plan (pure
// host code, no device call) and walked by the launchers below.
enum class BnReduce { nchw, nhwc_scalar, nhwc_vec };
enum class BnElt { fixed_channel, vec, scalar };  // apply and dx kernels
enum class BnGate { none, y, mask };  // where backward reads the act gate
struct BnGrid { int64_t x, y; };
struct BnPlan {
  int64_t N, C, HW;
  int nhwc, act;
  // stats and backward reduce: grid = (cblocks, S); each block writes one
  // row of the [S][2][C] partial slabs — fp32 from the 8-wide bf16 kernels,
  // whose partials are fp32, double from the others
  BnReduce reduce;
  BnGrid reduce_grid;
  int slab_f32;
  int64_t slab_bytes;
  BnGate reduce_gate;
  // finalize: grid = (cchunks, Y); when Y > 1 it hands double partials
  // through part[part_doubles] and one ticket word per channel chunk (zero
  // before the first launch; the kernel leaves them zero)
  int64_t cchunks, Y, part_doubles;
  // forward apply; the fixed-channel bf16 NHWC training apply also writes
  // the 1-bit activation mask (numel/8 bytes)
  BnElt apply;
  BnGrid apply_grid;
  int writes_mask;
  // backward dx
  BnElt dx;
  BnGrid dx_grid;
  BnGate dx_gate;
};
// masked: the caller holds the forward's mask (honoured where a masked
// kernel exists: act != 0, bf16 NHWC, C % 8 == 0; otherwise the gate is y)
BnPlan bn_plan(int64_t N, int64_t C, int64_t HW, int nhwc, int elsize,
               int act, int training, int masked);
// sums: the slab workspace (void*: its element type follows the plan)
template <typename T>
void launch_bn_stats(const BnPlan&, const T* x, void* sums, hipStream_t);
void launch_bn_finalize(const BnPlan&, const void* sums, double* part,
                        unsigned* tickets, float* mean, float* invstd,
                        float* running_mean, float* running_var, float eps,
                        float momentum, hipStream_t);
template <typename T>
void launch_bn_apply(const BnPlan&, const T* x, const T* res, T* y,
                     const float* mean, const float* invstd,
                     const float* gamma, const float* beta,
                     unsigned char* msk, hipStream_t);
template <typename T>
void launch_bn_bwd_reduce(const BnPlan&, const T* dy, const T* y, const T* x,
                          const float* mean, const float* invstd, void* sums,
                          const unsigned char* msk, hipStream_t);
void launch_bn_bwd_finalize(const BnPlan&, const void* sums, double* part,
                            unsigned* tickets, const float* gamma,
                            const float* invstd, float* dgamma, float* dbeta,
                            float* k, int training, hipStream_t);
template <typename T>
void launch_bn_bwd_dx(const BnPlan&, const T* dy, const T* y, const T* x,
                      const float* mean, const float* invstd, const float* k,
                      T* dx, T* dres, const unsigned char* msk, hipStream_t);

// ---- cross_entropy.hip ------------------------------------------------
template <typename T>
void launch_ce_fwd(const T*, const int64_t*, float*, float*, int64_t,
                   int64_t, hipStream_t);
template <typename T>
void launch_ce_bwd(const T*, const int64_t*, const float*, const float*, T*,
                   int64_t, int64_t, hipStream_t);
// Label-smoothed CE with an ignore index. Forward writes loss_r[R] and
// lse[R] per row, then loss[0] (mean over non-ignored rows, count clamped
// to 1, or the plain sum) and n_valid[0]; backward forms its scale from
// grad_out[0] and n_valid[0] on the device. K < 2^30.
template <typename T>
void launch_ls_ce_fwd(const T* logits, const int64_t* target, float* loss_r,
                      float* lse, float* loss, int64_t* n_valid, int64_t R,
                      int64_t K, float smoothing, int64_t ignore_index,
                      int mean, hipStream_t);
template <typename T>
void launch_ls_ce_bwd(const T* logits, const int64_t* target,
                      const float* lse, const int64_t* n_valid,
                      const float* grad_out, T* dx, int64_t R, int64_t K,
                      float smoothing, int64_t ignore_index, int mean,
                      hipStream_t);

// ---- attn_score.hip ---------------------------------------------------
// scores[b,i,j] = sum_h vn[h] * tanh(q[b,i,h] + k[b,j,h] + bias[h]) for
// q (B,Tq,H), k (B,Tk,H); mask (B,Tk), 1 = valid key, nullptr = none. A
// masked key scores -65504 and is never read. B * ceil(H / 64) < 2^31.
template <typename T>
void launch_attn_score_fwd(const T* q, const T* k, const T* bias,
                           const T* vn, const uint8_t* mask, T* scores,
                           int64_t B, int64_t Tq, int64_t Tk, int64_t H,
                           hipStream_t);
// need_q: dq, dbias and dvn are written (slab: 2*B*H floats of workspace);
// need_k: dk is written. Pointers of a part that is not needed stay unused.
template <typename T>
void launch_attn_score_bwd(const T* ds, const T* q, const T* k,
                           const T* bias, const T* vn, const uint8_t* mask,
                           T* dq, T* dk, T* dbias, T* dvn, float* slab,
                           int64_t B, int64_t Tq, int64_t Tk, int64_t H,
                           int need_q, int need_k, hipStream_t);

// ---- conv_mfma.hip: forward (dgrad=0) or data-grad (dgrad=1); the dims
// are always those of the forward conv. add (dgrad only, nullptr = none)
// is a read-only bf16 tensor of dx's geometry summed into dx in the
// epilogue; stride-2 with R==1 or S==1 does not take one (throws). gate
// (with add only, Cin % 8 == 0, nullptr = none) holds one bit per element
// of add, bit i&7 of byte i/8: the epilogue then adds bf16(add * bit) ---
void launch_conv_igemm(const void* a, const void* b, void* out,
                       const void* zero, int N, int H, int W, int Cin,
                       int K, int OH, int OW, int R, int S, int stride,
                       int pad, int dgrad, const void* add,
                       const void* gate, hipStream_t stream);
// out = bf16(add * bit) over n8 8-element chunks, materialised: for the
// dgrad passes whose add runs outside the kernel
void launch_gate_addend(const void* add, const void* gate, void* out,
                        long n8, hipStream_t stream);

// The launches launch_conv_igemm makes for a shape, as pure host data:
// the launcher walks this plan, and the bindings expose it so tests can
// assert which kernel variant a shape reaches.
struct ConvIgemmLaunch {
  int v2;      // 1 = deep-pipeline structure (conv_mfma2.hip), 0 = 128-tile
  int mode;    // 0 FPROP, 1 DGRAD gather, 2 DGRAD stride-2 parity class
  int bm, bn;  // block tile
  int lin;     // v2 only: plain row-major A operand (1x1 stride-1 pad-0)
  long M, Nd, Kd;                            // GEMM dims of this launch
  int cls_a, cls_b, r0, s0, nr, ns, nh, nw;  // mode 2 only, else 0
};
struct ConvIgemmPlan {
  int n;                 // launches: 1, or up to 4 parity classes
  ConvIgemmLaunch e[4];
};
// reads DDLB_CONV_V2 at call time, as the launcher always has
ConvIgemmPlan conv_igemm_plan(int N, int H, int W, int Cin, int K, int OH,
                              int OW, int R, int S, int stride, int pad,
                              int dgrad);

// ---- conv_wgrad.hip: part_ws holds part_cap floats of slab workspace ---
// floats of split-P slab workspace the binding hands launch_conv_wgrad
constexpr long kConvWgradPartCap = 8L << 20;
// launch_conv_wgrad's host decisions for a shape
struct ConvWgradPlan {
  int tk, tr;    // dw tile (k rows x rsc columns)
  int ring;      // LDS ring depth: 2 for the 128x128 tile, else 3
  int r1;        // 1x1 stride-1 pad-0: linear B operand, no carry chain
  long nk, nr;   // tiles along k and rsc
  long split;    // p-chunks per tile (grid = nk*nr*split)
  long p_per;    // pixels per chunk (the last chunk may hold fewer)
  long steps;    // 64-pixel steps of a full chunk
  long tail;     // pixels in a full chunk's last step (64 = not ragged)
  long psb;      // combine rows: 0 no combine (split == 1), 1 plain
                 // stores, > 1 memset + atomicAdd
};
ConvWgradPlan conv_wgrad_plan(int N, int C, int K, int OH, int OW, int R,
                              int S, int stride, int pad, long part_cap);
// dw_bf16 == nullptr: fp32 dw in (K, R*S*C) memory. Otherwise dw is
// unused and the result goes to dw_bf16 in the same layout, each element
// the round-to-nearest-even bf16 of its fp32 sum: from the kernel's
// epilogue (split == 1) or from a combine that adds every element's
// slabs in slab order (no memset, no atomics).
void launch_conv_wgrad(const void* x, const void* dy, float* dw,
                       float* part_ws, long part_cap, const void* zero,
                       int N, int H, int W, int C, int K, int OH, int OW,
                       int R, int S, int stride, int pad,
                       hipStream_t stream, void* dw_bf16 = nullptr);

// ---- conv_weight_layout.hip: bf16 batched transpose -------------------
// in[b][m][n] (row stride in_rs, batch stride in_bs) ->
// out[b][n][m] (row stride out_rs, batch stride out_bs); M % 8 == 0,
// Nn % 8 == 0, every stride a multiple of 8 elements.
void launch_weight_transpose(const void* in, void* out, long B, long M,
                             long Nn, long in_rs, long in_bs, long out_rs,
                             long out_bs, hipStream_t stream);

// ---- conv_stem.hip ----------------------------------------------------
void launch_conv_stem_fwd(const void* x, const void* w, void* y, int N,
                          int H, int W, int C, int K, int OH, int OW, int R,
                          int stride, int pad, hipStream_t stream);
void launch_conv_stem_wgrad(const void* x, const void* dy, float* dw,
                            float* part, int N, int H, int W, int C, int K,
                            int OH, int OW, int R, int stride, int pad,
                            hipStream_t stream);
int conv_stem_wgrad_chunks(int N, int OH, int OW, int K);

// ---- maxpool.hip ------------------------------------------------------
void launch_maxpool_fwd(const void*, void*, unsigned char*, int64_t,
                        int64_t, int, int, int, int, int, int, int,
                        hipStream_t);
void launch_maxpool_bwd(const void*, const unsigned char*, void*,
                        int64_t, int64_t, int, int, int, int, int, int,
                        int, hipStream_t);

// ---- seq_utils.hip ----------------------------------------------------
template <typename T>
void launch_revert_varlen(const T*, T*, const int64_t*, int64_t, int64_t,
                          int64_t, hipStream_t);
void launch_varlen_mask(const int64_t*, uint8_t*, int64_t, int64_t,
                        hipStream_t);

// ---- lstm.hip ---------------------------------------------------------
// One time step each; bf16 tensors travel as void*. H % 8 == 0, every bf16
// base 16-byte aligned, ceil(H/16) * ceil(B/16) below 2^31. Null h_prev /
// c_prev / dg_next / dh_add / dc_in mean zeros; null gates is not written.
void launch_lstm_step_fwd(const void* h_prev, const void* w,
                          const void* xproj, const float* bias,
                          const float* c_prev, void* y, float* cs,
                          void* gates, int64_t B, int64_t H,
                          hipStream_t stream);
void launch_lstm_step_bwd(const void* dg_next, const void* wt,
                          const void* dy, const void* dh_add,
                          const void* gates, const float* cs,
                          const float* c_prev, const float* dc_in, void* dg,
                          float* dc_out, int64_t B, int64_t H,
                          hipStream_t stream);

// ---- depthwise_conv.hip -----------------------------------------------
template <typename T>
void launch_dw3x3_fwd(const T*, const float*, T*, int64_t, int64_t, int64_t,
                      int64_t, int64_t, int64_t, int, int, hipStream_t);
template <typename T>
void launch_dw3x3_bwd_dx(const T*, const float*, T*, int64_t, int64_t,
                         int64_t, int64_t, int64_t, int64_t, int, int,
                         hipStream_t);
template <typename T>
void launch_dw3x3_bwd_dw(const T*, const T*, double*, int64_t, int64_t,
                         int64_t, int64_t, int64_t, int64_t, int, int,
                         hipStream_t);

}  // namespace ddlb
