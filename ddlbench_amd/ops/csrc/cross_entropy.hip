// Fused softmax cross-entropy (mean reduction) for gfx950.
//
// Replaces F.cross_entropy in the benchmark loss path
// (/root/reference/benchmark/mnist/mnist_pytorch.py uses F.cross_entropy;
// the gpipe scripts use F.nll_loss on log-softmax output). Small-vocab
// rows (CNN classifiers, K <= 2048) use one wave per row; large-vocab
// rows (GNMT K = 32320) use one 256-thread block per row with 16-byte
// vector loads. Backward is one vectorized elementwise kernel — no
// materialized softmax tensor. GNMT's own loss (label smoothing, PAD
// ignored, mean over tokens) is the ls_ce_* family at the end of the file.

#include "common.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <string>

typedef __attribute__((ext_vector_type(8))) short short8v;

namespace {

DEV float bf16_at(const short8v& v, int j) {
  __hip_bfloat16 h;
  unsigned short u = (unsigned short)v[j];
  __builtin_memcpy(&h, &u, 2);
  return __bfloat162float(h);
}

}  // namespace

// ---- small K: one wave per row ---------------------------------------
template <typename T>
__global__ void ce_fwd_wave_kernel(const T* __restrict__ logits,
                                   const int64_t* __restrict__ target,
                                   float* __restrict__ lse,
                                   float* __restrict__ loss_sum,
                                   int64_t B, int64_t K) {
  const int64_t b = blockIdx.x;
  if (b >= B) return;
  const T* row = logits + b * K;
  const int lane = threadIdx.x;
  float m = -INFINITY;
  for (int64_t k = lane; k < K; k += WAVE) m = fmaxf(m, to_f32(row[k]));
  m = wave_reduce_max(m);
  m = __shfl(m, 0, WAVE);
  float s = 0.f;
  for (int64_t k = lane; k < K; k += WAVE) s += __expf(to_f32(row[k]) - m);
  s = wave_reduce_sum(s);
  if (lane == 0) {
    const float l = m + __logf(s);
    lse[b] = l;
    atomicAdd(loss_sum, l - to_f32(row[target[b]]));
  }
}

// ---- large K: one 256-thread block per row, bf16x8 vector loads ------
template <typename T, bool VEC>
__global__ void ce_fwd_block_kernel(const T* __restrict__ logits,
                                    const int64_t* __restrict__ target,
                                    float* __restrict__ lse,
                                    float* __restrict__ loss_sum,
                                    int64_t B, int64_t K) {
  __shared__ float tmp[8];
  const int64_t b = blockIdx.x;
  if (b >= B) return;
  const T* row = logits + b * K;
  const int tid = threadIdx.x;
  float m = -INFINITY;
  if (VEC) {
    const short8v* rv = reinterpret_cast<const short8v*>(row);
    for (int64_t k8 = tid; k8 < K / 8; k8 += blockDim.x) {
      short8v v = rv[k8];
#pragma unroll
      for (int j = 0; j < 8; ++j) m = fmaxf(m, bf16_at(v, j));
    }
  } else {
    for (int64_t k = tid; k < K; k += blockDim.x)
      m = fmaxf(m, to_f32(row[k]));
  }
  auto maxop = [](float v) { return wave_reduce_max(v); };
  m = block_reduce(m, tmp, maxop, -INFINITY);
  if (tid == 0) tmp[0] = m;
  __syncthreads();
  m = tmp[0];
  __syncthreads();
  float s = 0.f;
  if (VEC) {
    const short8v* rv = reinterpret_cast<const short8v*>(row);
    for (int64_t k8 = tid; k8 < K / 8; k8 += blockDim.x) {
      short8v v = rv[k8];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += __expf(bf16_at(v, j) - m);
    }
  } else {
    for (int64_t k = tid; k < K; k += blockDim.x)
      s += __expf(to_f32(row[k]) - m);
  }
  auto sumop = [](float v) { return wave_reduce_sum(v); };
  s = block_reduce(s, tmp, sumop, 0.f);
  if (tid == 0) {
    const float l = m + __logf(s);
    lse[b] = l;
    atomicAdd(loss_sum, l - to_f32(row[target[b]]));
  }
}

// dx = (softmax - onehot) * gscale   (gscale = dloss / B for mean)
template <typename T>
__global__ void ce_bwd_kernel(const T* __restrict__ logits,
                              const int64_t* __restrict__ target,
                              const float* __restrict__ lse,
                              const float* __restrict__ gscale,
                              T* __restrict__ dx, int64_t B, int64_t K) {
  const int64_t total = B * K;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const int64_t b = i / K, k = i - b * K;
    float p = __expf(to_f32(logits[i]) - lse[b]);
    if (k == target[b]) p -= 1.f;
    dx[i] = from_f32<T>(p * gscale[0]);
  }
}

template <typename T>
void ddlb::launch_ce_fwd(const T* logits, const int64_t* target, float* lse,
                         float* loss_sum, int64_t B, int64_t K,
                         hipStream_t stream) {
  if (K >= 4096) {
    const bool vec = (K % 8 == 0) && sizeof(T) == 2;
    if (vec)
      hipLaunchKernelGGL((ce_fwd_block_kernel<T, true>),
                         dim3((uint32_t)B), dim3(256), 0, stream, logits,
                         target, lse, loss_sum, B, K);
    else
      hipLaunchKernelGGL((ce_fwd_block_kernel<T, false>),
                         dim3((uint32_t)B), dim3(256), 0, stream, logits,
                         target, lse, loss_sum, B, K);
  } else {
    hipLaunchKernelGGL((ce_fwd_wave_kernel<T>), dim3((uint32_t)B),
                       dim3(WAVE), 0, stream, logits, target, lse,
                       loss_sum, B, K);
  }
  HIP_CHECK_LAST();
}

template <typename T>
void ddlb::launch_ce_bwd(const T* logits, const int64_t* target,
                         const float* lse, const float* gscale, T* dx,
                         int64_t B, int64_t K, hipStream_t stream) {
  const int block = 256;
  int64_t want = (B * K + block - 1) / block;
  const int grid = (int)i64min(want > 0 ? want : 1, 256 * 8);
  hipLaunchKernelGGL((ce_bwd_kernel<T>), dim3(grid), dim3(block), 0, stream,
                     logits, target, lse, gscale, dx, B, K);
  HIP_CHECK_LAST();
}

// ======================================================================
// Label-smoothed cross-entropy with an ignore index (the GNMT loss).
//
// Per row r (logits x, width K, target t, smoothing e):
//   lse    = m + log sum exp(x - m)
//   loss_r = (1-e)*(lse - x[t]) + e*(lse - sum(x)/K)      t != ignore
//   dx_k   = (softmax_k - (1-e)*[k == t] - e/K) * scale   t != ignore
// One block per row: NW waves (1 below K = 4096, 4 from there on). Forward
// sweeps the row once, each thread keeping a running max, a sum of exps
// rescaled to that max, the plain sum and x[t]; backward reads the row once
// and writes dx once. Ignored rows are never read. A target outside [0, K)
// that is not the ignore index never becomes an address: its loss, lse and
// dx row are NaN. Row losses go to loss_r[] with plain stores and one block
// adds them in a fixed order, so the same input gives the same bits.
namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int uint4v;

// Largest finite negative: the running max starts here, not at -inf, so
// a thread that has seen nothing (or only -inf) never forms inf - inf.
constexpr float kLsNegMax = -3.402823466e+38f;

// element j (0..7) of eight packed bf16
DEV float bf16x8_at(const uint4v& v, int j) {
  const unsigned w = v[j >> 1];
  return __uint_as_float((j & 1) ? (w & 0xffff0000u) : (w << 16));
}

DEV unsigned pack_bf16x2(float lo, float hi) {
  const __hip_bfloat16 a = __float2bfloat16(lo), b = __float2bfloat16(hi);
  unsigned short ua, ub;
  __builtin_memcpy(&ua, &a, 2);
  __builtin_memcpy(&ub, &b, 2);
  return (unsigned)ua | ((unsigned)ub << 16);
}

// Sum or max over the block's NW waves, returned to every thread, always
// combined in the same order.
template <int NW, bool MAX>
DEV float ls_block_all(float v, float* tmp) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off, WAVE);
    v = MAX ? fmaxf(v, o) : v + o;
  }
  if (NW == 1) return v;
  __syncthreads();  // tmp may still be read from the previous call
  if ((threadIdx.x & (WAVE - 1)) == 0) tmp[threadIdx.x / WAVE] = v;
  __syncthreads();
  v = tmp[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) v = MAX ? fmaxf(v, tmp[w]) : v + tmp[w];
  return v;
}

struct LsRowAcc {
  float m = kLsNegMax, s = 0.f, sx = 0.f;
  DEV void rescale(float vmax) {
    const float nm = fmaxf(m, vmax);
    s *= __expf(m - nm);
    m = nm;
  }
  DEV void add(float x) {
    s += __expf(x - m);
    sx += x;
  }
  DEV void add8(const uint4v& v) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = bf16x8_at(v, j);
    float vmax = f[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) vmax = fmaxf(vmax, f[j]);
    rescale(vmax);
#pragma unroll
    for (int j = 0; j < 8; ++j) add(f[j]);
  }
};

}  // namespace

template <typename T, bool VEC, int NW>
__global__ __launch_bounds__(NW * WAVE) void ls_ce_fwd_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ target,
    float* __restrict__ loss_r, float* __restrict__ lse, int K,
    float smoothing, int64_t ignore_index) {
  constexpr int NT = NW * WAVE;
  __shared__ float tmp[NW];
  __shared__ float xt_sh;
  const int64_t r = blockIdx.x;
  const int64_t t64 = target[r];
  // block-uniform exits, taken before the row is touched
  if (t64 == ignore_index || t64 < 0 || t64 >= K) {
    if (threadIdx.x == 0) {
      const float v = (t64 == ignore_index) ? 0.f : __builtin_nanf("");
      loss_r[r] = v;
      lse[r] = v;
    }
    return;
  }
  const int t = (int)t64;
  const int tid = threadIdx.x;
  const T* row = logits + r * K;
  LsRowAcc a;
  if (VEC) {
    const uint4v* rv = reinterpret_cast<const uint4v*>(row);
    const int nv = K >> 3, tv = t >> 3;
    // x[t] is picked out of the sweep's own load of its vector
    auto take = [&](const uint4v& v, int k8) {
      a.add8(v);
      if (k8 == tv) {
        float xt = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j == (t & 7)) xt = bf16x8_at(v, j);
        xt_sh = xt;
      }
    };
    int k8 = tid;
    // four independent 16 B loads in flight per lane
    for (; k8 + 3 * NT < nv; k8 += 4 * NT) {
      const uint4v v0 = rv[k8], v1 = rv[k8 + NT], v2 = rv[k8 + 2 * NT],
                   v3 = rv[k8 + 3 * NT];
      take(v0, k8);
      take(v1, k8 + NT);
      take(v2, k8 + 2 * NT);
      take(v3, k8 + 3 * NT);
    }
    for (; k8 < nv; k8 += NT) take(rv[k8], k8);
  } else {
    for (int k = tid; k < K; k += NT) {
      const float x = to_f32(row[k]);
      a.rescale(x);
      a.add(x);
      if (k == t) xt_sh = x;
    }
  }
  const float m = ls_block_all<NW, true>(a.m, tmp);
  const float s = ls_block_all<NW, false>(a.s * expf(a.m - m), tmp);
  const float sx = ls_block_all<NW, false>(a.sx, tmp);
  __syncthreads();  // xt_sh
  if (tid == 0) {
    const float l = m + logf(s);
    lse[r] = l;
    loss_r[r] = (1.f - smoothing) * (l - xt_sh) +
                smoothing * (l - sx / (float)K);
  }
}

// One block: loss_sum and n_valid in a fixed order, then the final scalar.
// out[0] = loss (mean: loss_sum / max(n_valid, 1)), n_valid_out[0] = count.
__global__ __launch_bounds__(256) void ls_ce_finish_kernel(
    const float* __restrict__ loss_r, const int64_t* __restrict__ target,
    float* __restrict__ out, int64_t* __restrict__ n_valid_out, int64_t R,
    int64_t ignore_index, int mean) {
  __shared__ float tmp[4];
  __shared__ long long cnt_sh[4];
  float s = 0.f;
  long long cnt = 0;
  for (int64_t r = threadIdx.x; r < R; r += 256) {
    s += loss_r[r];
    cnt += target[r] != ignore_index;
  }
  s = ls_block_all<4, false>(s, tmp);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) cnt_sh[threadIdx.x / WAVE] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long total = cnt_sh[0] + cnt_sh[1] + cnt_sh[2] + cnt_sh[3];
    n_valid_out[0] = total;
    out[0] = mean ? s / (float)(total > 1 ? total : 1) : s;
  }
}

template <typename T, bool VEC, int NW>
__global__ __launch_bounds__(NW * WAVE) void ls_ce_bwd_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ target,
    const float* __restrict__ lse, const int64_t* __restrict__ n_valid,
    const float* __restrict__ grad_out, T* __restrict__ dx, int K,
    float smoothing, int64_t ignore_index, int mean) {
  constexpr int NT = NW * WAVE;
  const int64_t r = blockIdx.x;
  const int64_t t64 = target[r];
  const int tid = threadIdx.x;
  T* drow = dx + r * K;
  if (t64 == ignore_index || t64 < 0 || t64 >= K) {
    // zeros for an ignored row, NaN for a bad target; the logits stay unread
    const float fill = (t64 == ignore_index) ? 0.f : __builtin_nanf("");
    if (VEC) {
      const unsigned w = pack_bf16x2(fill, fill);
      const uint4v v = {w, w, w, w};
      uint4v* dv = reinterpret_cast<uint4v*>(drow);
      for (int k8 = tid; k8 < (K >> 3); k8 += NT) dv[k8] = v;
    } else {
      const T v = from_f32<T>(fill);
      for (int k = tid; k < K; k += NT) drow[k] = v;
    }
    return;
  }
  const int t = (int)t64;
  const T* row = logits + r * K;
  const float l = lse[r];
  float scale = grad_out[0];
  if (mean) {
    const int64_t nvld = n_valid[0];
    scale /= (float)(nvld > 1 ? nvld : 1);
  }
  const float uni = smoothing / (float)K, hit = 1.f - smoothing;
  if (VEC) {
    const uint4v* rv = reinterpret_cast<const uint4v*>(row);
    uint4v* dv = reinterpret_cast<uint4v*>(drow);
    const int nv = K >> 3, tv = t >> 3;
    auto grad8 = [&](const uint4v& v, int k8) {
      float g[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = __expf(bf16x8_at(v, j) - l) - uni;
      if (k8 == tv) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j == (t & 7)) g[j] -= hit;
      }
      uint4v o;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = pack_bf16x2(g[2 * j] * scale, g[2 * j + 1] * scale);
      return o;
    };
    int k8 = tid;
    for (; k8 + 3 * NT < nv; k8 += 4 * NT) {
      const uint4v v0 = rv[k8], v1 = rv[k8 + NT], v2 = rv[k8 + 2 * NT],
                   v3 = rv[k8 + 3 * NT];
      dv[k8] = grad8(v0, k8);
      dv[k8 + NT] = grad8(v1, k8 + NT);
      dv[k8 + 2 * NT] = grad8(v2, k8 + 2 * NT);
      dv[k8 + 3 * NT] = grad8(v3, k8 + 3 * NT);
    }
    for (; k8 < nv; k8 += NT) dv[k8] = grad8(rv[k8], k8);
  } else {
    for (int k = tid; k < K; k += NT) {
      float g = __expf(to_f32(row[k]) - l) - uni;
      if (k == t) g -= hit;
      drow[k] = from_f32<T>(g * scale);
    }
  }
}

namespace {

// 16 B per-lane accesses: 2-byte elements, K % 8 == 0 (every row then starts
// 16 B aligned) and 16 B aligned bases
template <typename T>
bool ls_ce_vec_ok(const T* a, const T* b, int64_t K) {
  return sizeof(T) == 2 && K % 8 == 0 &&
         (reinterpret_cast<uintptr_t>(a) & 15) == 0 &&
         (reinterpret_cast<uintptr_t>(b) & 15) == 0;
}

}  // namespace

template <typename T>
void ddlb::launch_ls_ce_fwd(const T* logits, const int64_t* target,
                            float* loss_r, float* lse, float* loss,
                            int64_t* n_valid, int64_t R, int64_t K,
                            float smoothing, int64_t ignore_index, int mean,
                            hipStream_t stream) {
  if (R > 0) {
    const bool vec = ls_ce_vec_ok(logits, logits, K);
    const bool wide = K >= 4096;
    const dim3 grid((uint32_t)R);
#define LS_FWD(V, NW)                                                      \
  hipLaunchKernelGGL((ls_ce_fwd_kernel<T, V, NW>), grid, dim3(NW * WAVE),  \
                     0, stream, logits, target, loss_r, lse, (int)K,       \
                     smoothing, ignore_index)
    if constexpr (sizeof(T) == 2) {
      if (vec && wide) LS_FWD(true, 4);
      else if (vec) LS_FWD(true, 1);
    }
    if (!vec && wide) LS_FWD(false, 4);
    else if (!vec) LS_FWD(false, 1);
#undef LS_FWD
    HIP_CHECK_LAST();
  }
  hipLaunchKernelGGL(ls_ce_finish_kernel, dim3(1), dim3(256), 0, stream,
                     loss_r, target, loss, n_valid, R, ignore_index, mean);
  HIP_CHECK_LAST();
}

template <typename T>
void ddlb::launch_ls_ce_bwd(const T* logits, const int64_t* target,
                            const float* lse, const int64_t* n_valid,
                            const float* grad_out, T* dx, int64_t R,
                            int64_t K, float smoothing, int64_t ignore_index,
                            int mean, hipStream_t stream) {
  if (R == 0) return;
  const bool vec = ls_ce_vec_ok(logits, dx, K);
  const bool wide = K >= 4096;
  const dim3 grid((uint32_t)R);
#define LS_BWD(V, NW)                                                      \
  hipLaunchKernelGGL((ls_ce_bwd_kernel<T, V, NW>), grid, dim3(NW * WAVE),  \
                     0, stream, logits, target, lse, n_valid, grad_out, dx, \
                     (int)K, smoothing, ignore_index, mean)
  if constexpr (sizeof(T) == 2) {
    if (vec && wide) LS_BWD(true, 4);
    else if (vec) LS_BWD(true, 1);
  }
  if (!vec && wide) LS_BWD(false, 4);
  else if (!vec) LS_BWD(false, 1);
#undef LS_BWD
  HIP_CHECK_LAST();
}

#define INSTANTIATE(T)                                                     \
  template void ddlb::launch_ls_ce_fwd<T>(                                 \
      const T*, const int64_t*, float*, float*, float*, int64_t*, int64_t, \
      int64_t, float, int64_t, int, hipStream_t);                          \
  template void ddlb::launch_ls_ce_bwd<T>(                                 \
      const T*, const int64_t*, const float*, const int64_t*,              \
      const float*, T*, int64_t, int64_t, float, int64_t, int,             \
      hipStream_t);                                                        \
  template void ddlb::launch_ce_fwd<T>(                                  \
      const T*, const int64_t*, float*, float*, int64_t, int64_t,          \
      hipStream_t);                                                        \
  template void ddlb::launch_ce_bwd<T>(                                    \
      const T*, const int64_t*, const float*, const float*, T*, int64_t,   \
      int64_t, hipStream_t);
INSTANTIATE(float)
INSTANTIATE(__hip_bfloat16)
#undef INSTANTIATE
