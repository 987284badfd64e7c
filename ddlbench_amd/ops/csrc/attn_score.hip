// Fused Bahdanau (additive) attention score for gfx950, forward and backward.
//
//   scores[b,i,j] = sum_h vn[h] * tanh(q[b,i,h] + k[b,j,h] + bias[h])
//
// The eager composition builds the (B, Tq, Tk, H) tanh tensor; these kernels
// never do. All arithmetic is fp32, results are rounded once into the input
// dtype. A key with mask[b,j] == 0 scores exactly kMaskedScore, costs no
// tanh, and its k row is never read, forward or backward.
//
// tanh comes from the hardware exp2 and reciprocal:
//   e = 2^(x * 2 log2 e),  r = 1 / (e + 1),  tanh x = 1 - 2 r,
//   1 - tanh^2 x = 4 r (1 - r)
// x -> +inf gives e = inf, r = 0; x -> -inf gives e = 0, r = 1: both forms
// saturate with no inf/inf, and the derivative has no cancellation.
//
// Forward: lane-per-h. A wave owns a TI x 4 tile of (i, j) and sweeps H in
// chunks of 64 * V elements, V per lane from one 16 B load (8 bf16 / 4 fp32;
// V = 1 when H is no multiple of V or a base is not 16 B aligned). Each
// loaded q or k vector feeds TI * 4 * V / (TI + 4) tanh, so loads are noise
// beside the 16 independent accumulation chains; a 6-step xor butterfly
// closes each chain. TI = 1 serves Tq < 4 (the decode step).
//
// Backward recomputes tanh and needs no cross-lane sum at all: a block owns
// (b, 64 columns of h), a lane one column. Its waves first take the q rows
// in turn, sweeping every valid key (dq, and this block's share of dbias
// and dvn), then take the keys in turn, sweeping every q row (dk). ds[b,i,j]
// is the same for the whole wave. The four waves' dbias / dvn shares are
// added in wave order into one (b, h) fp32 slab entry each, and a second
// kernel adds the B slabs in batch order: no atomics, same bits every run.

#include "common.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <string>

namespace {

constexpr float kMaskedScore = -65504.0f;
constexpr float kTwoLog2e = 2.8853900817779268f;
constexpr int kTJ = 4;       // keys per forward wave tile
constexpr int kBwdCols = WAVE;  // h columns per backward block

typedef __attribute__((ext_vector_type(4))) unsigned int uint4v;
typedef __attribute__((ext_vector_type(4))) float float4v;

// r = 1 / (exp(2x) + 1)
DEV float tanh_r(float x) {
  return __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(x * kTwoLog2e) + 1.f);
}

template <typename T, int V> struct VecLoad;
template <typename T> struct VecLoad<T, 1> {
  static DEV void load(const T* p, float (&f)[1]) { f[0] = to_f32(*p); }
};
template <> struct VecLoad<float, 4> {
  static DEV void load(const float* p, float (&f)[4]) {
    const float4v v = *reinterpret_cast<const float4v*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = v[e];
  }
};
template <> struct VecLoad<__hip_bfloat16, 8> {
  static DEV void load(const __hip_bfloat16* p, float (&f)[8]) {
    const uint4v v = *reinterpret_cast<const uint4v*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f[2 * e] = __uint_as_float(v[e] << 16);
      f[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u);
    }
  }
};

DEV int wave_id() {
  return __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
}

}  // namespace

// grid-stride over wave tiles; tile -> (b, i tile, j tile), j fastest so a
// block's four waves share their q rows
template <typename T, int V, int TI>
__global__ __launch_bounds__(256) void attn_score_fwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k,
    const T* __restrict__ bias, const T* __restrict__ vn,
    const uint8_t* __restrict__ mask, T* __restrict__ out, int64_t Tq,
    int64_t Tk, int64_t H, int64_t n_it, int64_t n_jt, int64_t n_tiles) {
  const int lane = threadIdx.x & (WAVE - 1);
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave_id(); tile < n_tiles;
       tile += (int64_t)gridDim.x * 4) {
    const int64_t jt = tile % n_jt, it = (tile / n_jt) % n_it,
                  b = tile / (n_jt * n_it);
    const int64_t i0 = it * TI, j0 = jt * kTJ;
    bool inside[kTJ], valid[kTJ], any = false;
#pragma unroll
    for (int jj = 0; jj < kTJ; ++jj) {
      inside[jj] = j0 + jj < Tk;
      valid[jj] = inside[jj] && (!mask || mask[b * Tk + j0 + jj] != 0);
      any = any || valid[jj];
    }
    // rows past Tq repeat the last one: computed, never stored
    const T* qrow[TI];
#pragma unroll
    for (int ii = 0; ii < TI; ++ii)
      qrow[ii] = q + (b * Tq + i64min(i0 + ii, Tq - 1)) * H;
    const T* krow = k + (b * Tk + j0) * H;

    float acc[TI][kTJ];
#pragma unroll
    for (int ii = 0; ii < TI; ++ii)
#pragma unroll
      for (int jj = 0; jj < kTJ; ++jj) acc[ii][jj] = 0.f;

    if (any) {
      for (int64_t h = (int64_t)lane * V; h < H; h += WAVE * V) {
        float vnv[V], bv[V], qv[TI][V];
        VecLoad<T, V>::load(vn + h, vnv);
        VecLoad<T, V>::load(bias + h, bv);
#pragma unroll
        for (int ii = 0; ii < TI; ++ii) {
          VecLoad<T, V>::load(qrow[ii] + h, qv[ii]);
#pragma unroll
          for (int e = 0; e < V; ++e) qv[ii][e] += bv[e];
        }
#pragma unroll
        for (int jj = 0; jj < kTJ; ++jj) {
          if (!valid[jj]) continue;  // wave-uniform
          float kv[V];
          VecLoad<T, V>::load(krow + jj * H + h, kv);
#pragma unroll
          for (int ii = 0; ii < TI; ++ii)
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const float r = tanh_r(qv[ii][e] + kv[e]);
              acc[ii][jj] += vnv[e] * (1.f - 2.f * r);
            }
        }
      }
    }
#pragma unroll
    for (int ii = 0; ii < TI; ++ii)
#pragma unroll
      for (int jj = 0; jj < kTJ; ++jj) {
        float v = acc[ii][jj];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
        if (lane == 0 && i0 + ii < Tq && inside[jj])
          out[(b * Tq + i0 + ii) * Tk + j0 + jj] =
              from_f32<T>(valid[jj] ? v : kMaskedScore);
      }
  }
}

// block = (b, 64 h columns); slab: [2][B][H] fp32, dbias shares then dvn
template <typename T>
__global__ __launch_bounds__(256) void attn_score_bwd_kernel(
    const T* __restrict__ ds, const T* __restrict__ q,
    const T* __restrict__ k, const T* __restrict__ bias,
    const T* __restrict__ vn, const uint8_t* __restrict__ mask,
    T* __restrict__ dq, T* __restrict__ dk, float* __restrict__ slab,
    int64_t B, int64_t Tq, int64_t Tk, int64_t H, int64_t n_ht, int need_q,
    int need_k) {
  __shared__ float share[2][4][WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = wave_id();
  const int64_t b = blockIdx.x / n_ht;
  const int64_t h = (blockIdx.x % n_ht) * kBwdCols + lane;
  const bool act = h < H;  // idle lanes run on zeros and store nothing
  const float vnh = act ? to_f32(vn[h]) : 0.f;
  const float bh = act ? to_f32(bias[h]) : 0.f;
  const uint8_t* mrow = mask ? mask + b * Tk : nullptr;
  const T* dsb = ds + b * Tq * Tk;

  if (need_q) {
    float dbias_acc = 0.f, dvn_acc = 0.f;
    for (int64_t i = wave; i < Tq; i += 4) {
      const int64_t row = (b * Tq + i) * H + h;
      const float qb = act ? to_f32(q[row]) + bh : 0.f;
      float g = 0.f;
      for (int64_t j = 0; j < Tk; ++j) {
        if (mrow && mrow[j] == 0) continue;  // wave-uniform
        const float d = to_f32(dsb[i * Tk + j]);
        const float kv = act ? to_f32(k[(b * Tk + j) * H + h]) : 0.f;
        const float r = tanh_r(qb + kv);
        g += d * (4.f * r * (1.f - r));
        dvn_acc += d * (1.f - 2.f * r);
      }
      g *= vnh;
      dbias_acc += g;
      if (act) dq[row] = from_f32<T>(g);
    }
    share[0][wave][lane] = dbias_acc;
    share[1][wave][lane] = dvn_acc;
    __syncthreads();
    if (wave < 2 && act) {
      const float* s = &share[wave][0][lane];
      slab[(wave * B + b) * H + h] =
          ((s[0] + s[WAVE]) + s[2 * WAVE]) + s[3 * WAVE];
    }
  }
  if (need_k) {
    for (int64_t j = wave; j < Tk; j += 4) {
      const int64_t row = (b * Tk + j) * H + h;
      if (mrow && mrow[j] == 0) {  // wave-uniform; k stays unread
        if (act) dk[row] = from_f32<T>(0.f);
        continue;
      }
      const float kb = act ? to_f32(k[row]) + bh : 0.f;
      float g = 0.f;
      for (int64_t i = 0; i < Tq; ++i) {
        const float d = to_f32(dsb[i * Tk + j]);
        const float qv = act ? to_f32(q[(b * Tq + i) * H + h]) : 0.f;
        const float r = tanh_r(qv + kb);
        g += d * (4.f * r * (1.f - r));
      }
      if (act) dk[row] = from_f32<T>(g * vnh);
    }
  }
}

// dbias[h], dvn[h] = the B slab entries added in batch order
template <typename T>
__global__ __launch_bounds__(256) void attn_score_bwd_combine_kernel(
    const float* __restrict__ slab, T* __restrict__ dbias,
    T* __restrict__ dvn, int64_t B, int64_t H) {
  const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (h >= H) return;
  float sb = 0.f, sv = 0.f;
  for (int64_t b = 0; b < B; ++b) {
    sb += slab[b * H + h];
    sv += slab[(B + b) * H + h];
  }
  dbias[h] = from_f32<T>(sb);
  dvn[h] = from_f32<T>(sv);
}

namespace {

bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace

template <typename T>
void ddlb::launch_attn_score_fwd(const T* q, const T* k, const T* bias,
                                 const T* vn, const uint8_t* mask, T* out,
                                 int64_t B, int64_t Tq, int64_t Tk,
                                 int64_t H, hipStream_t stream) {
  if (B == 0 || Tq == 0 || Tk == 0) return;
  constexpr int VW = 16 / sizeof(T);
  const bool vec = H % VW == 0 && aligned16(q) && aligned16(k) &&
                   aligned16(bias) && aligned16(vn);
  const bool one = Tq < 4;
  const int64_t n_it = one ? Tq : (Tq + 3) / 4, n_jt = (Tk + kTJ - 1) / kTJ;
  const int64_t n_tiles = B * n_it * n_jt;
  const dim3 grid((uint32_t)i64min((n_tiles + 3) / 4, 1 << 20));
#define ATTN_FWD(V, TI)                                                     \
  hipLaunchKernelGGL((attn_score_fwd_kernel<T, V, TI>), grid, dim3(256), 0, \
                     stream, q, k, bias, vn, mask, out, Tq, Tk, H, n_it,    \
                     n_jt, n_tiles)
  if (vec && one) ATTN_FWD(VW, 1);
  else if (vec) ATTN_FWD(VW, 4);
  else if (one) ATTN_FWD(1, 1);
  else ATTN_FWD(1, 4);
#undef ATTN_FWD
  HIP_CHECK_LAST();
}

template <typename T>
void ddlb::launch_attn_score_bwd(const T* ds, const T* q, const T* k,
                                 const T* bias, const T* vn,
                                 const uint8_t* mask, T* dq, T* dk,
                                 T* dbias, T* dvn, float* slab, int64_t B,
                                 int64_t Tq, int64_t Tk, int64_t H,
                                 int need_q, int need_k,
                                 hipStream_t stream) {
  if (B == 0 || Tq == 0 || Tk == 0 || !(need_q || need_k)) return;
  const int64_t n_ht = (H + kBwdCols - 1) / kBwdCols;
  hipLaunchKernelGGL((attn_score_bwd_kernel<T>), dim3((uint32_t)(B * n_ht)),
                     dim3(256), 0, stream, ds, q, k, bias, vn, mask, dq, dk,
                     slab, B, Tq, Tk, H, n_ht, need_q, need_k);
  HIP_CHECK_LAST();
  if (need_q) {
    hipLaunchKernelGGL((attn_score_bwd_combine_kernel<T>),
                       dim3((uint32_t)((H + 255) / 256)), dim3(256), 0,
                       stream, slab, dbias, dvn, B, H);
    HIP_CHECK_LAST();
  }
}

#define INSTANTIATE(T)                                                      \
  template void ddlb::launch_attn_score_fwd<T>(                             \
      const T*, const T*, const T*, const T*, const uint8_t*, T*, int64_t,  \
      int64_t, int64_t, int64_t, hipStream_t);                              \
  template void ddlb::launch_attn_score_bwd<T>(                             \
      const T*, const T*, const T*, const T*, const T*, const uint8_t*, T*, \
      T*, T*, T*, float*, int64_t, int64_t, int64_t, int64_t, int, int,     \
      hipStream_t);
INSTANTIATE(float)
INSTANTIATE(__hip_bfloat16)
#undef INSTANTIATE
