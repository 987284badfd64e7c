// LSTM recurrence for gfx950: one kernel launch per time step, forward and
// backward. bf16 operands, fp32 accumulation and fp32 cell state.
//
//   gates_t = xproj[t] + h_{t-1} W_hh^T + bias        (gate rows i, f, g, o)
//   c_t = s(f) c_{t-1} + s(i) tanh(g),   h_t = s(o) tanh(c_t)
//
// Tiling, both directions: a block owns 16 hidden units x 16 batch rows and
// runs four waves. The recurrent product's K axis (H forward, 4H backward)
// is dealt to the waves in 32-wide steps, wave w taking steps w, w+4, ...;
// every wave keeps all of the block's accumulators (four gate tiles
// forward, one dh tile backward) on v_mfma_f32_16x16x32_bf16. The four
// partial tiles meet in LDS and are added in wave order, so a cell's sum
// has one fixed order and its four gate pre-activations sit in one block,
// where thread (b, j) finishes the cell. Both MFMA operands are rows with K
// contiguous (h / dgates rows, W_hh rows forward, rows of the once-per-call
// transpose W_hh^T backward), so a lane's fragment is one 16-byte load and
// each operand byte goes to exactly one lane of the block: there is nothing
// for an LDS stage to share.
//
// Blocks are numbered unit-slice major and passed through xcd_remap, so an
// XCD owns a contiguous eighth of the hidden units and finds its slice of
// W_hh in its own L2 on every step.
//
// No atomics, no cross-block communication: step t+1 sees step t's stores
// because it is a later kernel on the same stream.
//
// sigma and tanh come from the hardware exp2 and reciprocal,
//   s(x) = 1 / (1 + 2^(-x log2 e)),  tanh x = 1 - 2 / (2^(2 x log2 e) + 1);
// both saturate through inf -> 0 with no inf/inf.

#include "mfma_common.h"
#include "launchers.h"
#include <stdexcept>
#include <string>

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kTile = 16;    // units and batch rows per block
constexpr int kCells = kTile * kTile;

DEV float sigmoid_f(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-x * kLog2e));
}
DEV float tanh_f(float x) {
  return 1.f - 2.f * __builtin_amdgcn_rcpf(
                         __builtin_amdgcn_exp2f(x * (2.f * kLog2e)) + 1.f);
}
DEV float bf(const __hip_bfloat16* p) { return __bfloat162float(*p); }

// 8 bf16 at p when ok, else zeros; p must be 16-byte aligned when ok
DEV bf16x8 frag(const __hip_bfloat16* p, bool ok) {
  bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return ok ? *reinterpret_cast<const bf16x8*>(p) : z;
}

// block -> (unit slice, batch tile): slice-major logical order, XCD-remapped
DEV void tile_origin(int n_bt, int64_t& j0, int64_t& b0) {
  const int block = xcd_remap(blockIdx.x, gridDim.x);
  j0 = (int64_t)(block / n_bt) * kTile;
  b0 = (int64_t)(block % n_bt) * kTile;
}

}  // namespace

// h_prev / c_prev null: zeros (the product is skipped outright).
// gates null: not written (nothing will run backward).
__global__ __launch_bounds__(256) void lstm_step_fwd_kernel(
    const __hip_bfloat16* __restrict__ h_prev,
    const __hip_bfloat16* __restrict__ w,      // (4H, H)
    const __hip_bfloat16* __restrict__ xproj,  // (B, 4H)
    const float* __restrict__ bias,            // (4H)
    const float* __restrict__ c_prev, __hip_bfloat16* __restrict__ y,
    float* __restrict__ cs, __hip_bfloat16* __restrict__ gates, int64_t B,
    int64_t H, int n_bt) {
  __shared__ float red[4][4][kCells];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int r = lane & 15, kq = lane >> 4;
  int64_t j0, b0;
  tile_origin(n_bt, j0, b0);

  f32x4 acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (h_prev) {
    const bool arow = b0 + r < B, wrow = j0 + r < H;
    const __hip_bfloat16* ap = h_prev + (b0 + r) * H;
    const __hip_bfloat16* wp = w + (j0 + r) * H;
    // the trip count is wave-uniform (an MFMA needs all 64 lanes); a lane
    // whose 8-wide fragment starts at or past H feeds zeros. H % 8 == 0: a
    // fragment starting below H ends at or below H
    for (int64_t k0 = (int64_t)wave * 32; k0 < H; k0 += 128) {
      const int64_t k = k0 + kq * 8;
      const bool kin = k < H;
      const bf16x8 a = frag(ap + k, arow && kin);
#pragma unroll
      for (int g = 0; g < 4; ++g)
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a, frag(wp + g * H * H + k, wrow && kin), acc[g], 0, 0, 0);
    }
  }
  // accumulator element i of a lane is (row 4 kq + i, col r) of the tile
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      red[wave][g][(kq * 4 + i) * kTile + r] = acc[g][i];
  __syncthreads();

  const int64_t b = b0 + tid / kTile, j = j0 + tid % kTile;
  if (b >= B || j >= H) return;
  float pre[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float hw = ((red[0][g][tid] + red[1][g][tid]) + red[2][g][tid]) +
                     red[3][g][tid];
    pre[g] = hw + bf(xproj + b * 4 * H + g * H + j) + bias[g * H + j];
  }
  const float gi = sigmoid_f(pre[0]), gf = sigmoid_f(pre[1]),
              gg = tanh_f(pre[2]), go = sigmoid_f(pre[3]);
  const float cp = c_prev ? c_prev[b * H + j] : 0.f;
  const float c = gf * cp + gi * gg;
  cs[b * H + j] = c;
  y[b * H + j] = __float2bfloat16(go * tanh_f(c));
  if (gates) {
    __hip_bfloat16* gp = gates + b * 4 * H + j;
    gp[0] = __float2bfloat16(gi);
    gp[H] = __float2bfloat16(gf);
    gp[2 * H] = __float2bfloat16(gg);
    gp[3 * H] = __float2bfloat16(go);
  }
}

// dh = dy + dh_add + dg_next W_hh; dg_next / dh_add / dc_in / c_prev null:
// zeros.
__global__ __launch_bounds__(256) void lstm_step_bwd_kernel(
    const __hip_bfloat16* __restrict__ dg_next,  // (B, 4H), step t+1
    const __hip_bfloat16* __restrict__ wt,       // (H, 4H) = W_hh^T
    const __hip_bfloat16* __restrict__ dy,       // (B, H)
    const __hip_bfloat16* __restrict__ dh_add,   // (B, H)
    const __hip_bfloat16* __restrict__ gates,    // (B, 4H), step t
    const float* __restrict__ cs, const float* __restrict__ c_prev,
    const float* __restrict__ dc_in, __hip_bfloat16* __restrict__ dg,
    float* __restrict__ dc_out, int64_t B, int64_t H, int n_bt) {
  __shared__ float red[4][kCells];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int r = lane & 15, kq = lane >> 4;
  int64_t j0, b0;
  tile_origin(n_bt, j0, b0);

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (dg_next) {
    const bool arow = b0 + r < B, wrow = j0 + r < H;
    const __hip_bfloat16* ap = dg_next + (b0 + r) * 4 * H;
    const __hip_bfloat16* wp = wt + (j0 + r) * 4 * H;
    // 4H % 32 == 0: every K step is whole, the trip count wave-uniform
    for (int64_t k0 = (int64_t)wave * 32; k0 < 4 * H; k0 += 128) {
      const int64_t k = k0 + kq * 8;
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          frag(ap + k, arow), frag(wp + k, wrow), acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wave][(kq * 4 + i) * kTile + r] = acc[i];
  __syncthreads();

  const int64_t b = b0 + tid / kTile, j = j0 + tid % kTile;
  if (b >= B || j >= H) return;
  const int64_t cell = b * H + j;
  float dh = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  dh += bf(dy + cell);
  if (dh_add) dh += bf(dh_add + cell);
  const __hip_bfloat16* gp = gates + b * 4 * H + j;
  const float gi = bf(gp), gf = bf(gp + H), gg = bf(gp + 2 * H),
              go = bf(gp + 3 * H);
  const float tc = tanh_f(cs[cell]);
  const float cp = c_prev ? c_prev[cell] : 0.f;
  const float dc = (dc_in ? dc_in[cell] : 0.f) + dh * go * (1.f - tc * tc);
  __hip_bfloat16* dp = dg + b * 4 * H + j;
  dp[0] = __float2bfloat16(dc * gg * gi * (1.f - gi));
  dp[H] = __float2bfloat16(dc * cp * gf * (1.f - gf));
  dp[2 * H] = __float2bfloat16(dc * gi * (1.f - gg * gg));
  dp[3 * H] = __float2bfloat16(dh * tc * go * (1.f - go));
  dc_out[cell] = dc * gf;
}

namespace {

// blocks of one step, or 0 when there is nothing to do
int64_t lstm_tiles(int64_t B, int64_t H, int* n_bt) {
  *n_bt = (int)((B + kTile - 1) / kTile);
  return ((H + kTile - 1) / kTile) * *n_bt;
}

}  // namespace

void ddlb::launch_lstm_step_fwd(const void* h_prev, const void* w,
                                const void* xproj, const float* bias,
                                const float* c_prev, void* y, float* cs,
                                void* gates, int64_t B, int64_t H,
                                hipStream_t stream) {
  int n_bt;
  const int64_t nwg = lstm_tiles(B, H, &n_bt);
  if (nwg == 0) return;
  using bf16 = __hip_bfloat16;
  hipLaunchKernelGGL(lstm_step_fwd_kernel, dim3((uint32_t)nwg), dim3(256), 0,
                     stream, (const bf16*)h_prev, (const bf16*)w,
                     (const bf16*)xproj, bias, c_prev, (bf16*)y, cs,
                     (bf16*)gates, B, H, n_bt);
  HIP_CHECK_LAST();
}

void ddlb::launch_lstm_step_bwd(const void* dg_next, const void* wt,
                                const void* dy, const void* dh_add,
                                const void* gates, const float* cs,
                                const float* c_prev, const float* dc_in,
                                void* dg, float* dc_out, int64_t B, int64_t H,
                                hipStream_t stream) {
  int n_bt;
  const int64_t nwg = lstm_tiles(B, H, &n_bt);
  if (nwg == 0) return;
  using bf16 = __hip_bfloat16;
  hipLaunchKernelGGL(lstm_step_bwd_kernel, dim3((uint32_t)nwg), dim3(256), 0,
                     stream, (const bf16*)dg_next, (const bf16*)wt,
                     (const bf16*)dy, (const bf16*)dh_add, (const bf16*)gates,
                     cs, c_prev, dc_in, (bf16*)dg, dc_out, B, H, n_bt);
  HIP_CHECK_LAST();
}
