// Fused BatchNorm2d + activation (+ residual add) for gfx950.
//
// Replaces the reference's unfused BatchNorm2d -> ReLU (-> add) chains
// (SURVEY.md §2.6 "Key model ops") with single-pass kernels:
//   forward train:  stats reduce -> finalize -> apply(normalize+act[+add])
//   forward eval:   apply only (running stats)
//   backward:       masked-dy reduce -> finalize -> dx elementwise
// BN is HBM-bandwidth-bound on MI355X (≈8 TB/s HBM3E): fusing the
// activation and the residual add into the normalize pass removes one to
// two full tensor round-trips per block vs eager PyTorch.
//
// dtype: x/y/dy in T ∈ {float, bf16}; gamma/beta/stats always fp32.
// Activation codes: 0 = identity, 1 = relu, 2 = relu6.
//
// Which kernel a shape reaches is decided once, by ddlb::bn_plan at the
// end of this file; the launchers only switch on the plan they are given.

#include "common.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <string>
#include <type_traits>

using ddlb::BnElt;
using ddlb::BnGate;
using ddlb::BnGrid;
using ddlb::BnPlan;
using ddlb::BnReduce;

namespace {

using bf16 = __hip_bfloat16;

template <int ACT> DEV float act_fwd(float v) {
  if (ACT == 1) return fmaxf(v, 0.f);
  if (ACT == 2) return fminf(fmaxf(v, 0.f), 6.f);
  return v;
}

// activation backward mask from the *output* y
template <int ACT> DEV float act_mask(float y) {
  if (ACT == 1) return y > 0.f ? 1.f : 0.f;
  if (ACT == 2) return (y > 0.f && y < 6.f) ? 1.f : 0.f;
  return 1.f;
}

// ---- W-wide lane IO: W = 1 (one element) or 8 (one 16 B / 32 B vector) --
// NHWC: 8 consecutive elements are 8 consecutive channels (C % 8 == 0);
// NCHW: 8 consecutive elements share one channel when HW % 8 == 0.
typedef __attribute__((ext_vector_type(8))) short short8v;
typedef __attribute__((ext_vector_type(8))) float float8v;

template <typename T> struct vec8;
template <> struct vec8<float> { using type = float8v; };
template <> struct vec8<bf16> { using type = short8v; };

DEV float elt_f32(const short8v& v, int j) {
  bf16 h;
  unsigned short u = (unsigned short)v[j];
  __builtin_memcpy(&h, &u, 2);
  return __bfloat162float(h);
}
DEV float elt_f32(const float8v& v, int j) { return v[j]; }

DEV void set_elt(short8v& v, int j, float f) {
  bf16 h = __float2bfloat16(f);
  unsigned short u;
  __builtin_memcpy(&u, &h, 2);
  v[j] = (short)u;
}
DEV void set_elt(float8v& v, int j, float f) { v[j] = f; }

// W consecutive elements of one tensor, kept as loaded (bf16 stays packed)
// and converted lane by lane where the arithmetic uses them.
template <typename T, int W> struct Lanes;
template <typename T> struct Lanes<T, 1> {
  T v;
  DEV void load(const T* __restrict__ p, int64_t vi) { v = p[vi]; }
  DEV void store(T* __restrict__ p, int64_t vi) const { p[vi] = v; }
  DEV float get(int) const { return to_f32(v); }
  DEV void set(int, float f) { v = from_f32<T>(f); }
};
template <typename T> struct Lanes<T, 8> {
  using V = typename vec8<T>::type;
  V v;
  DEV void load(const T* __restrict__ p, int64_t vi) {
    v = reinterpret_cast<const V*>(p)[vi];
  }
  DEV void store(T* __restrict__ p, int64_t vi) const {
    reinterpret_cast<V*>(p)[vi] = v;
  }
  DEV float get(int j) const { return elt_f32(v, j); }
  DEV void set(int j, float f) { set_elt(v, j, f); }
};

// Activation-gradient gate of elements vi*W ..: from the 1-bit mask the
// forward apply wrote (one byte per 8 channels; y is never read) or from
// the output y. bit = the lane's bit in its mask byte.
template <typename T, int W, int ACT, bool MASKED>
struct Gate {
  Lanes<T, W> vy;
  unsigned mb;
  DEV void load(const T* __restrict__ y,
                const unsigned char* __restrict__ msk, int64_t vi) {
    if constexpr (MASKED) mb = msk[W == 8 ? vi : vi >> 3];
    else if constexpr (ACT != 0) vy.load(y, vi);
  }
  DEV float get(int j, int bit) const {
    if constexpr (MASKED) return (float)((mb >> bit) & 1u);
    else if constexpr (ACT != 0) return act_mask<ACT>(vy.get(j));
    else return 1.f;
  }
};

// ---- the two per-element terms of a reduction ---------------------------
// Every reduce kernel sums p and p*q per channel: (x, x) for the batch
// statistics, (dy', xhat) for the backward, dy' = dy * gate.
template <typename T, int W>
struct StatsTerms {
  const T* x;
  struct Lane {};
  DEV Lane bind(int64_t) const { return {}; }
  DEV void load(const Lane&, int64_t vi, float (&p)[W], float (&q)[W]) const {
    Lanes<T, W> vx;
    vx.load(x, vi);
#pragma unroll
    for (int j = 0; j < W; ++j) p[j] = q[j] = vx.get(j);
  }
};

template <typename T, int W, int ACT, bool MASKED>
struct BwdTerms {
  const T* dy;
  const T* y;
  const T* x;
  const float* mean;
  const float* invstd;
  const unsigned char* msk;
  struct Lane { float mu[W], is[W]; int bit0; };
  DEV Lane bind(int64_t c0) const {
    Lane l;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      l.mu[j] = mean[c0 + j];
      l.is[j] = invstd[c0 + j];
    }
    l.bit0 = W == 8 ? 0 : (int)(c0 & 7);
    return l;
  }
  DEV void load(const Lane& l, int64_t vi, float (&p)[W],
                float (&q)[W]) const {
    Lanes<T, W> vdy, vx;
    Gate<T, W, ACT, MASKED> gate;
    vdy.load(dy, vi);
    vx.load(x, vi);
    gate.load(y, msk, vi);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      p[j] = vdy.get(j) * gate.get(j, l.bit0 + j);
      q[j] = (vx.get(j) - l.mu[j]) * l.is[j];
    }
  }
};

// double accumulators (N*HW can exceed 1e7 elements per channel) ...
DEV void accum(double& s, double& ss, float p, float q) {
  s += p;
  ss += fma((double)p, (double)q, 0.0);
}
// ... and fp32 ones for the 8-wide bf16 kernels: a thread's row slice is
// at most a few hundred values that never were wider than fp32
DEV void accum(float& s, float& ss, float p, float q) {
  s += p;
  ss = fmaf(p, q, ss);
}

// ---- reduce, NCHW -------------------------------------------------------
// grid = (C, S): block (c, s) covers slice s of channel c's N*HW space and
// writes its two sums to slab s of sums[S][2][C].
template <typename Terms>
__global__ void bn_reduce_nchw_kernel(Terms terms, double* __restrict__ sums,
                                      int64_t N, int64_t C, int64_t HW) {
  __shared__ double tmp[8];
  const int64_t c = blockIdx.x;
  const auto lane = terms.bind(c);
  const int64_t total = N * HW;
  const int64_t per = (total + gridDim.y - 1) / gridDim.y;
  const int64_t begin = (int64_t)blockIdx.y * per;
  const int64_t end = i64min(begin + per, total);
  double s = 0.0, ss = 0.0;
  for (int64_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
    const int64_t n = i / HW, r = i - n * HW;
    float p[1], q[1];
    terms.load(lane, (n * C + c) * HW + r, p, q);
    accum(s, ss, p[0], q[0]);
  }
  auto op = [](double v) { return wave_reduce_sum(v); };
  s = block_reduce(s, tmp, op, 0.0);
  __syncthreads();
  ss = block_reduce(ss, tmp, op, 0.0);
  if (threadIdx.x == 0) {
    sums[((int64_t)blockIdx.y * 2 + 0) * C + c] = s;
    sums[((int64_t)blockIdx.y * 2 + 1) * C + c] = ss;
  }
}

// ---- reduce, NHWC (channels-last) ---------------------------------------
// rows = N*H*W; element (row, c) at row*C + c. Block = CG channel lanes of
// W channels each x (256/CG) row-groups; grid = (lane blocks, S row
// slices). Every wave reads consecutive channels of one row (coalesced);
// per-thread partials of type AT combine across row-groups in LDS, in
// row-group order, and land in slab blockIdx.y of sums[S][2][C] with plain
// stores. W = 8: one 16 B bf16 vector per lane, fp32 partials and slabs.
// W = 1: double partials and slabs. UNROLL4 is the scalar statistics
// kernel's summation order: four rows are added to each other first and
// then to the running sum.
template <int W, typename AT, bool UNROLL4, typename Terms>
__global__ void bn_reduce_nhwc_kernel(Terms terms, AT* __restrict__ sums,
                                      int64_t rows, int64_t C, int CG) {
  static_assert(!UNROLL4 || W == 1, "the 4-row order is a scalar one");
  __shared__ AT tmp[2][256][W];
  const int ci = threadIdx.x % CG;
  const int rj = threadIdx.x / CG;
  const int RG = blockDim.x / CG;
  const int64_t c0 = ((int64_t)blockIdx.x * CG + ci) * W;
  const bool active = (c0 < C) && (rj < RG);
  const int64_t per = (rows + gridDim.y - 1) / gridDim.y;
  const int64_t begin = (int64_t)blockIdx.y * per;
  const int64_t end = i64min(begin + per, rows);
  AT s[W] = {}, ss[W] = {};
  if (active) {
    const auto lane = terms.bind(c0);
    int64_t r = begin + rj;
    const int64_t step = RG;
    if constexpr (UNROLL4) {
      for (; r + 3 * step < end; r += 4 * step) {
        float p0[1], p1[1], p2[1], p3[1], q0[1], q1[1], q2[1], q3[1];
        terms.load(lane, (r + 0 * step) * C + c0, p0, q0);
        terms.load(lane, (r + 1 * step) * C + c0, p1, q1);
        terms.load(lane, (r + 2 * step) * C + c0, p2, q2);
        terms.load(lane, (r + 3 * step) * C + c0, p3, q3);
        s[0] += (double)p0[0] + p1[0] + p2[0] + p3[0];
        ss[0] += fma((double)p0[0], q0[0], fma((double)p1[0], q1[0],
                     fma((double)p2[0], q2[0], (double)p3[0] * q3[0])));
      }
    }
    for (; r < end; r += step) {
      float p[W], q[W];
      terms.load(lane, (r * C + c0) / W, p, q);
#pragma unroll
      for (int j = 0; j < W; ++j) accum(s[j], ss[j], p[j], q[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < W; ++j) {
    tmp[0][threadIdx.x][j] = s[j];
    tmp[1][threadIdx.x][j] = ss[j];
  }
  __syncthreads();
  if (rj == 0 && c0 < C) {
    for (int g = 1; g < RG; ++g)
#pragma unroll
      for (int j = 0; j < W; ++j) {
        s[j] += tmp[0][g * CG + ci][j];
        ss[j] += tmp[1][g * CG + ci][j];
      }
#pragma unroll
    for (int j = 0; j < W; ++j) {
      sums[((int64_t)blockIdx.y * 2 + 0) * C + c0 + j] = s[j];
      sums[((int64_t)blockIdx.y * 2 + 1) * C + c0 + j] = ss[j];
    }
  }
}

}  // namespace

// ---- finalize: slabs -> per-channel results, one launch ----------------
// sums = per-(row-slice) partial slabs [S][2][C] written with plain
// stores by the reduce kernels (a C=64 layer at S~1500 slices would
// otherwise serialize ~1500 f64 atomics per channel address). ST is the
// slab element: float from the bf16 vec reduces, double from the scalar
// and fp32 ones.
//
// Geometry: block = BN_FIN_CH channels (threadIdx.x: adjacent threads
// read adjacent channels of one slab row) x BN_FIN_TY slab rows; grid =
// (channel chunks, Y slab chunks), so the block count follows the slab
// bytes, not C. Every sum runs in an order fixed by indices:
//   1. thread (tx, ty) adds rows r0+ty, r0+ty+TY, ... of its chunk in
//      double, the TY partials combine in LDS in ty order;
//   2. Y > 1: the block stores its double partial to part[chunk][y][2][CH]
//      and draws a ticket on its channel chunk (stores, vmcnt(0) in
//      every wave, barrier, agent-scope release, wait, relaxed agent
//      fetch_add). The block that draws the last ticket acquires, sums
//      the Y partials the same way (y = ty, ty+TY, ... then ty order),
//      resets the ticket and writes the results. No block waits on
//      another; the ticket words live in a zero-initialised workspace.
#define BN_FIN_CH 32
#define BN_FIN_TY 8
#define BN_FIN_ROWS 32   // slab rows per block (before the Y cap)
#define BN_FIN_YMAX 64   // Y * 2 * CH doubles = 32 KB per channel chunk

struct BnFinParams {
  const void* sums;      // [S][2][C] of ST
  double* part;          // [cchunks][Y][2][BN_FIN_CH]
  unsigned* tickets;     // [cchunks], zero between launches
  int64_t C, S;
  int rows_per;          // slab rows per block
  double count;
  // forward
  float* mean; float* invstd; float* running_mean; float* running_var;
  float eps, momentum;
  // backward
  const float* gamma; const float* invstd_in;
  float* dgamma; float* dbeta; float* k;  // k = [3][C]
  int training;
};

template <typename ST, bool BWD>
__global__ __launch_bounds__(BN_FIN_CH * BN_FIN_TY)
void bn_finalize_kernel(BnFinParams q) {
  __shared__ double sh[2][BN_FIN_TY][BN_FIN_CH];
  __shared__ int is_last;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int t = ty * BN_FIN_CH + tx;
  const int Y = gridDim.y;
  const int64_t c = (int64_t)blockIdx.x * BN_FIN_CH + tx;
  const ST* sums = static_cast<const ST*>(q.sums);

  // level 1: this block's slab rows
  double a0 = 0.0, a1 = 0.0;
  if (c < q.C) {
    const int64_t r0 = (int64_t)blockIdx.y * q.rows_per;
    const int64_t r1 = i64min(r0 + q.rows_per, q.S);
    int64_t r = r0 + ty;
    for (; r + 3 * BN_FIN_TY < r1; r += 4 * BN_FIN_TY) {
      ST v0[4], v1[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v0[j] = sums[((r + j * BN_FIN_TY) * 2 + 0) * q.C + c];
        v1[j] = sums[((r + j * BN_FIN_TY) * 2 + 1) * q.C + c];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a0 += (double)v0[j];
        a1 += (double)v1[j];
      }
    }
    for (; r < r1; r += BN_FIN_TY) {
      a0 += (double)sums[(r * 2 + 0) * q.C + c];
      a1 += (double)sums[(r * 2 + 1) * q.C + c];
    }
  }
  sh[0][ty][tx] = a0;
  sh[1][ty][tx] = a1;
  __syncthreads();
  // threads 0..2*CH-1: (which, channel) = (t / CH, t % CH)
  double v = 0.0;
  if (t < 2 * BN_FIN_CH) {
#pragma unroll
    for (int j = 0; j < BN_FIN_TY; ++j) v += sh[ty][j][tx];
  }

  if (Y > 1) {
    double* part = q.part + (int64_t)blockIdx.x * Y * 2 * BN_FIN_CH;
    if (t < 2 * BN_FIN_CH) part[(int64_t)blockIdx.y * 2 * BN_FIN_CH + t] = v;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned ticket = __hip_atomic_fetch_add(
          &q.tickets[blockIdx.x], 1u, __ATOMIC_RELAXED,
          __HIP_MEMORY_SCOPE_AGENT);
      const int last = ticket == (unsigned)(Y - 1);
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // every arrival is in: the next launch finds the word at zero
        __hip_atomic_store(&q.tickets[blockIdx.x], 0u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      is_last = last;
    }
    __syncthreads();
    if (!is_last) return;
    // level 2: the Y partials of this channel chunk, in index order
    a0 = 0.0;
    a1 = 0.0;
    for (int y = ty; y < Y; y += BN_FIN_TY) {
      a0 += part[(int64_t)(y * 2 + 0) * BN_FIN_CH + tx];
      a1 += part[(int64_t)(y * 2 + 1) * BN_FIN_CH + tx];
    }
    sh[0][ty][tx] = a0;
    sh[1][ty][tx] = a1;
    __syncthreads();
    v = 0.0;
    if (t < 2 * BN_FIN_CH) {
#pragma unroll
      for (int j = 0; j < BN_FIN_TY; ++j) v += sh[ty][j][tx];
    }
  }

  // hand the second sum over to the thread that owns the channel
  __syncthreads();
  if (t < 2 * BN_FIN_CH) sh[ty][0][tx] = v;
  __syncthreads();
  if (t >= BN_FIN_CH || c >= q.C) return;
  const double s0 = sh[0][0][tx], s1 = sh[1][0][tx];
  if (!BWD) {
    // s0 = sum x, s1 = sum x^2
    const double m = s0 / q.count;
    double var = s1 / q.count - m * m;
    var = var < 0.0 ? 0.0 : var;
    q.mean[c] = (float)m;
    q.invstd[c] = (float)rsqrt(var + (double)q.eps);
    if (q.running_mean != nullptr) {
      const double unbiased =
          q.count > 1.0 ? var * q.count / (q.count - 1.0) : var;
      q.running_mean[c] = (1.f - q.momentum) * q.running_mean[c] +
                          q.momentum * (float)m;
      q.running_var[c] = (1.f - q.momentum) * q.running_var[c] +
                         q.momentum * (float)unbiased;
    }
  } else {
    // s0 = sum dy', s1 = sum dy' * xhat
    q.dgamma[c] = (float)s1;
    q.dbeta[c] = (float)s0;
    q.k[c] = q.gamma[c] * q.invstd_in[c];                        // k1
    q.k[q.C + c] = q.training ? (float)(s0 / q.count) : 0.f;     // k2
    q.k[2 * q.C + c] = q.training ? (float)(s1 / q.count) : 0.f; // k3
  }
}

namespace {

// ---- apply / dx, grid-stride --------------------------------------------
// y = act(gamma*(x-mean)*invstd + beta [+ res]);
// dx = k1 * (dy' - k2 - xhat*k3), optionally dres = dy'.
// Thread i handles elements i*W ..; LANE_CH: lane j has channel
// (i*W) % C + j (NHWC vectors), otherwise all W share (i*W / cdiv) % C.
template <typename T, int W, int ACT, bool ADD, bool LANE_CH>
__global__ void bn_apply_kernel(const T* __restrict__ x,
                                const T* __restrict__ res,
                                T* __restrict__ y,
                                const float* __restrict__ mean,
                                const float* __restrict__ invstd,
                                const float* __restrict__ gamma,
                                const float* __restrict__ beta,
                                int64_t C, int64_t cdiv, int64_t totalW) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < totalW; i += stride) {
    const int64_t e0 = i * W;
    const int64_t cb = LANE_CH ? e0 % C : (e0 / cdiv) % C;
    Lanes<T, W> vx, vr, vy;
    vx.load(x, i);
    if (ADD) vr.load(res, i);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int64_t c = LANE_CH ? cb + j : cb;
      float v = (vx.get(j) - mean[c]) * invstd[c] * gamma[c] + beta[c];
      if (ADD) v += vr.get(j);
      vy.set(j, act_fwd<ACT>(v));
    }
    vy.store(y, i);
  }
}

template <typename T, int W, int ACT, bool ADD, bool LANE_CH>
__global__ void bn_bwd_dx_kernel(const T* __restrict__ dy,
                                 const T* __restrict__ y,
                                 const T* __restrict__ x,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ invstd,
                                 const float* __restrict__ k,
                                 T* __restrict__ dx, T* __restrict__ dres,
                                 int64_t C, int64_t cdiv, int64_t totalW) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < totalW; i += stride) {
    const int64_t e0 = i * W;
    Lanes<T, W> vdy, vx, vdx, vdr;
    Gate<T, W, ACT, false> gate;
    vdy.load(dy, i);
    gate.load(y, nullptr, i);
    vx.load(x, i);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int64_t c = LANE_CH ? (e0 % C + j) : ((e0 / cdiv) % C);
      const float g = vdy.get(j) * gate.get(j, j);
      const float xhat = (vx.get(j) - mean[c]) * invstd[c];
      vdx.set(j, k[c] * (g - k[C + c] - xhat * k[2 * C + c]));
      if (ADD) vdr.set(j, g);
    }
    vdx.store(dx, i);
    if (ADD) vdr.store(dres, i);
  }
}

// ---- NHWC bf16 apply / dx, fixed-channel geometry -------------------------
// Same (CG8 x RG) block shape as the reductions: each thread owns 8
// channels and walks rows, so per-channel params load ONCE per thread
// instead of once per element (the grid-stride variant is issue-bound
// on the 32 extra scalar loads per 48 B of traffic).
template <int ACT, bool ADD>
__global__ void bn_apply_fixed_kernel(const bf16* __restrict__ x,
                                      const bf16* __restrict__ res,
                                      bf16* __restrict__ y,
                                      const float* __restrict__ mean,
                                      const float* __restrict__ invstd,
                                      const float* __restrict__ gamma,
                                      const float* __restrict__ beta,
                                      unsigned char* __restrict__ msk,
                                      int64_t rows, int64_t C, int CG8) {
  const int ci = threadIdx.x % CG8;
  const int rj = threadIdx.x / CG8;
  const int RG = blockDim.x / CG8;
  const int64_t c0 = ((int64_t)blockIdx.x * CG8 + ci) * 8;
  if (c0 >= C || rj >= RG) return;
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = invstd[c0 + j] * gamma[c0 + j];
    sh[j] = beta[c0 + j] - mean[c0 + j] * sc[j];
  }
  const int64_t per = (rows + gridDim.y - 1) / gridDim.y;
  const int64_t begin = (int64_t)blockIdx.y * per;
  const int64_t end = i64min(begin + per, rows);
  for (int64_t r = begin + rj; r < end; r += RG) {
    const int64_t i8 = (r * C + c0) / 8;
    Lanes<bf16, 8> vx, vr, vy;
    vx.load(x, i8);
    if (ADD) vr.load(res, i8);
    unsigned mbits = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = fmaf(vx.get(j), sc[j], sh[j]);
      if (ADD) v += vr.get(j);
      if (ACT != 0 && act_mask<ACT>(v) > 0.f) mbits |= 1u << j;
      vy.set(j, act_fwd<ACT>(v));
    }
    vy.store(y, i8);
    // 1-bit activation mask: backward re-reads this byte instead of y
    if (ACT != 0 && msk != nullptr) msk[i8] = (unsigned char)mbits;
  }
}

template <int ACT, bool ADD, bool MASKED>
__global__ void bn_bwd_dx_fixed_kernel(const bf16* __restrict__ dy,
                                       const bf16* __restrict__ y,
                                       const bf16* __restrict__ x,
                                       const float* __restrict__ mean,
                                       const float* __restrict__ invstd,
                                       const float* __restrict__ k,
                                       bf16* __restrict__ dx,
                                       bf16* __restrict__ dres,
                                       const unsigned char* __restrict__ msk,
                                       int64_t rows, int64_t C, int CG8) {
  const int ci = threadIdx.x % CG8;
  const int rj = threadIdx.x / CG8;
  const int RG = blockDim.x / CG8;
  const int64_t c0 = ((int64_t)blockIdx.x * CG8 + ci) * 8;
  if (c0 >= C || rj >= RG) return;
  float k1[8], k2[8], k3[8], mu[8], is[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    k1[j] = k[c0 + j];
    k2[j] = k[C + c0 + j];
    k3[j] = k[2 * C + c0 + j];
    mu[j] = mean[c0 + j];
    is[j] = invstd[c0 + j];
  }
  const int64_t per = (rows + gridDim.y - 1) / gridDim.y;
  const int64_t begin = (int64_t)blockIdx.y * per;
  const int64_t end = i64min(begin + per, rows);
  for (int64_t r = begin + rj; r < end; r += RG) {
    const int64_t i8 = (r * C + c0) / 8;
    Lanes<bf16, 8> vdy, vx, vdx, vdr;
    Gate<bf16, 8, ACT, MASKED> gate;
    vdy.load(dy, i8);
    vx.load(x, i8);
    gate.load(y, msk, i8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float g = vdy.get(j) * gate.get(j, j);
      const float xhat = (vx.get(j) - mu[j]) * is[j];
      vdx.set(j, k1[j] * (g - k2[j] - xhat * k3[j]));
      if (ADD) vdr.set(j, g);
    }
    vdx.store(dx, i8);
    if (ADD) vdr.store(dres, i8);
  }
}

// ---- dispatch plan --------------------------------------------------------
// The tuning constants of the whole family; re-tuning one is an edit here,
// measured with benchmark/bn_probe.py against the previous build.
constexpr int BN_BLOCK = 256;             // threads per block, all kernels
constexpr int64_t BN_LANES = 64;          // channel lanes per NHWC block
// 8-wide bf16 reduces up to this C (the probe shows them ahead there)
constexpr int64_t BN_VEC_REDUCE_MAX_C = 512;
// the fixed-channel apply/dx starve below this many rows (too few blocks)
constexpr int64_t BN_FIXED_MIN_ROWS = 32768;
// rows/16 (not /512): a block still covers >=16 rows per row-group, and
// the old cap starved the small-HW layers (C2048@7x7 ran 196 blocks on a
// 256-CU chip)
constexpr int64_t BN_ROWS_PER_SLICE = 16;
constexpr int64_t BN_MAX_BLOCKS = 2048;   // reduce / fixed-channel grids
constexpr int64_t BN_ELT_MAX_BLOCKS = 256 * 8;  // grid-stride grids

// (lane blocks, row slices) of the NHWC kernels whose threads own channels
BnGrid row_grid(int64_t rows, int64_t lanes) {
  const int64_t cg = i64min(lanes, BN_LANES);
  BnGrid g;
  g.x = (lanes + cg - 1) / cg;
  g.y = i64min(i64max(rows / BN_ROWS_PER_SLICE, 1),
               i64max(BN_MAX_BLOCKS / g.x, 1));
  return g;
}

BnGrid elementwise_grid(int64_t total) {
  const int64_t want = (total + BN_BLOCK - 1) / BN_BLOCK;
  return {i64min(want > 0 ? want : 1, BN_ELT_MAX_BLOCKS), 1};
}

template <typename F> void dispatch_act(int act, F&& f) {
  if (act == 0) f(std::integral_constant<int, 0>{});
  else if (act == 1) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 2>{});
}
template <typename F> void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

dim3 dim3_of(const BnGrid& g) {
  return dim3((unsigned)g.x, (unsigned)g.y);
}

}  // namespace

BnPlan ddlb::bn_plan(int64_t N, int64_t C, int64_t HW, int nhwc, int elsize,
                     int act, int training, int masked) {
  BnPlan p = {};
  p.N = N; p.C = C; p.HW = HW; p.nhwc = nhwc; p.act = act;
  const int64_t rows = N * HW, total = rows * C;
  // the 16 B-per-lane NHWC kernels: bf16, whole 8-channel groups
  const bool nhwc8 = nhwc && elsize == 2 && C % 8 == 0;
  // the mask exists only where the fixed-channel apply wrote it
  const bool use_mask = masked && act != 0 && nhwc8;
  const BnGate gate = act == 0 ? BnGate::none
                      : use_mask ? BnGate::mask : BnGate::y;

  // stats and backward reduce
  if (!nhwc) {
    p.reduce = BnReduce::nchw;
    p.reduce_grid.x = C;
    p.reduce_grid.y = i64max(
        i64min((rows + BN_BLOCK - 1) / BN_BLOCK,
               i64max(BN_MAX_BLOCKS / C, 1)), 1);
    p.reduce_gate = act == 0 ? BnGate::none : BnGate::y;
  } else {
    const bool vec = nhwc8 && C <= BN_VEC_REDUCE_MAX_C;
    p.reduce = vec ? BnReduce::nhwc_vec : BnReduce::nhwc_scalar;
    p.reduce_grid = row_grid(rows, vec ? C / 8 : C);
    p.reduce_gate = gate;
  }
  p.slab_f32 = p.reduce == BnReduce::nhwc_vec;
  p.slab_bytes = p.reduce_grid.y * 2 * C * (p.slab_f32 ? 4 : 8);

  // finalize grid along the slabs: BN_FIN_ROWS rows per block, at most
  // BN_FIN_YMAX blocks per channel chunk
  const int64_t S = p.reduce_grid.y;
  p.cchunks = (C + BN_FIN_CH - 1) / BN_FIN_CH;
  p.Y = i64min((S + BN_FIN_ROWS - 1) / BN_FIN_ROWS, BN_FIN_YMAX);
  p.part_doubles = p.Y > 1 ? p.cchunks * p.Y * 2 * BN_FIN_CH : 0;

  // apply and dx
  const bool vec8ok = total % 8 == 0 && (nhwc ? C % 8 == 0 : HW % 8 == 0);
  const BnElt stride_kind = vec8ok ? BnElt::vec : BnElt::scalar;
  const BnGrid stride_grid = elementwise_grid(vec8ok ? total / 8 : total);
  p.writes_mask = training && act != 0 && nhwc8;
  const bool apply_fixed =
      nhwc8 && (rows >= BN_FIXED_MIN_ROWS || p.writes_mask);
  p.apply = apply_fixed ? BnElt::fixed_channel : stride_kind;
  p.apply_grid = apply_fixed ? row_grid(rows, C / 8) : stride_grid;
  const bool dx_fixed = nhwc8 && (rows >= BN_FIXED_MIN_ROWS || use_mask);
  p.dx = dx_fixed ? BnElt::fixed_channel : stride_kind;
  p.dx_grid = dx_fixed ? row_grid(rows, C / 8) : stride_grid;
  // only the fixed-channel dx can take its gate from the mask
  p.dx_gate = gate;
  return p;
}

// ---- launchers: each walks the plan it is given ----------------------------
template <typename T>
void ddlb::launch_bn_stats(const BnPlan& p, const T* x, void* sums,
                     hipStream_t stream) {
  const dim3 grid = dim3_of(p.reduce_grid), block(BN_BLOCK);
  const int64_t rows = p.N * p.HW;
  switch (p.reduce) {
    case BnReduce::nchw:
      hipLaunchKernelGGL((bn_reduce_nchw_kernel<StatsTerms<T, 1>>), grid,
                         block, 0, stream, StatsTerms<T, 1>{x},
                         (double*)sums, p.N, p.C, p.HW);
      break;
    case BnReduce::nhwc_scalar:
      hipLaunchKernelGGL(
          (bn_reduce_nhwc_kernel<1, double, true, StatsTerms<T, 1>>), grid,
          block, 0, stream, StatsTerms<T, 1>{x}, (double*)sums, rows, p.C,
          (int)i64min(p.C, BN_LANES));
      break;
    case BnReduce::nhwc_vec:
      if constexpr (sizeof(T) == 2)
        hipLaunchKernelGGL(
            (bn_reduce_nhwc_kernel<8, float, false, StatsTerms<T, 8>>), grid,
            block, 0, stream, StatsTerms<T, 8>{x}, (float*)sums, rows, p.C,
            (int)i64min(p.C / 8, BN_LANES));
      else
        throw std::logic_error("bn_plan: 8-wide reduce on a 4-byte dtype");
      break;
  }
  HIP_CHECK_LAST();
}

template <typename T>
void ddlb::launch_bn_bwd_reduce(const BnPlan& p, const T* dy, const T* y,
                          const T* x, const float* mean, const float* invstd,
                          void* sums, const unsigned char* msk,
                          hipStream_t stream) {
  const dim3 grid = dim3_of(p.reduce_grid), block(BN_BLOCK);
  const int64_t rows = p.N * p.HW;
  dispatch_act(p.act, [&](auto A) {
    dispatch_bool(p.reduce_gate == BnGate::mask, [&](auto M) {
      constexpr int ACT = decltype(A)::value;
      constexpr bool MASKED = decltype(M)::value && ACT != 0;
      switch (p.reduce) {
        case BnReduce::nchw: {
          using Terms = BwdTerms<T, 1, ACT, false>;
          hipLaunchKernelGGL((bn_reduce_nchw_kernel<Terms>), grid, block, 0,
                             stream, Terms{dy, y, x, mean, invstd, nullptr},
                             (double*)sums, p.N, p.C, p.HW);
          break;
        }
        case BnReduce::nhwc_scalar: {
          using Terms = BwdTerms<T, 1, ACT, MASKED>;
          hipLaunchKernelGGL(
              (bn_reduce_nhwc_kernel<1, double, false, Terms>), grid, block,
              0, stream, Terms{dy, y, x, mean, invstd, msk}, (double*)sums,
              rows, p.C, (int)i64min(p.C, BN_LANES));
          break;
        }
        case BnReduce::nhwc_vec:
          if constexpr (sizeof(T) == 2) {
            using Terms = BwdTerms<T, 8, ACT, MASKED>;
            hipLaunchKernelGGL(
                (bn_reduce_nhwc_kernel<8, float, false, Terms>), grid, block,
                0, stream, Terms{dy, y, x, mean, invstd, msk}, (float*)sums,
                rows, p.C, (int)i64min(p.C / 8, BN_LANES));
          } else {
            throw std::logic_error(
                "bn_plan: 8-wide reduce on a 4-byte dtype");
          }
          break;
      }
    });
  });
  HIP_CHECK_LAST();
}

// one launch for either direction; q carries the direction's pointers
template <bool BWD>
static void bn_finalize_launch(const BnPlan& p, BnFinParams q,
                               const void* sums, double* part,
                               unsigned* tickets, hipStream_t stream) {
  q.sums = sums; q.part = part; q.tickets = tickets;
  q.C = p.C; q.S = p.reduce_grid.y; q.count = (double)(p.N * p.HW);
  q.rows_per = (int)((q.S + p.Y - 1) / p.Y);
  const dim3 grid((unsigned)p.cchunks, (unsigned)p.Y);
  const dim3 block(BN_FIN_CH, BN_FIN_TY);
  if (p.slab_f32)
    hipLaunchKernelGGL((bn_finalize_kernel<float, BWD>), grid, block, 0,
                       stream, q);
  else
    hipLaunchKernelGGL((bn_finalize_kernel<double, BWD>), grid, block, 0,
                       stream, q);
  HIP_CHECK_LAST();
}

void ddlb::launch_bn_finalize(const BnPlan& p, const void* sums, double* part,
                        unsigned* tickets, float* mean, float* invstd,
                        float* rm, float* rv, float eps, float momentum,
                        hipStream_t stream) {
  BnFinParams q = {};
  q.mean = mean; q.invstd = invstd;
  q.running_mean = rm; q.running_var = rv;
  q.eps = eps; q.momentum = momentum;
  bn_finalize_launch<false>(p, q, sums, part, tickets, stream);
}

void ddlb::launch_bn_bwd_finalize(const BnPlan& p, const void* sums,
                                  double* part, unsigned* tickets,
                                  const float* gamma, const float* invstd,
                                  float* dgamma, float* dbeta, float* k,
                                  int training, hipStream_t stream) {
  BnFinParams q = {};
  q.gamma = gamma; q.invstd_in = invstd;
  q.dgamma = dgamma; q.dbeta = dbeta; q.k = k;
  q.training = training;
  bn_finalize_launch<true>(p, q, sums, part, tickets, stream);
}

template <typename T>
void ddlb::launch_bn_apply(const BnPlan& p, const T* x, const T* res, T* y,
                     const float* mean, const float* invstd,
                     const float* gamma, const float* beta,
                     unsigned char* msk, hipStream_t stream) {
  const dim3 grid = dim3_of(p.apply_grid), block(BN_BLOCK);
  const int64_t rows = p.N * p.HW, total = rows * p.C;
  const int64_t cdiv = p.nhwc ? 1 : p.HW;
  dispatch_act(p.act, [&](auto A) {
    dispatch_bool(res != nullptr, [&](auto R) {
      constexpr int ACT = decltype(A)::value;
      constexpr bool ADD = decltype(R)::value;
      switch (p.apply) {
        case BnElt::fixed_channel:
          if constexpr (sizeof(T) == 2)
            hipLaunchKernelGGL((bn_apply_fixed_kernel<ACT, ADD>), grid,
                               block, 0, stream, x, res, y, mean, invstd,
                               gamma, beta, p.writes_mask ? msk : nullptr,
                               rows, p.C, (int)i64min(p.C / 8, BN_LANES));
          else
            throw std::logic_error(
                "bn_plan: fixed-channel apply on a 4-byte dtype");
          break;
        case BnElt::vec:
          dispatch_bool(p.nhwc != 0, [&](auto L) {
            hipLaunchKernelGGL(
                (bn_apply_kernel<T, 8, ACT, ADD, decltype(L)::value>), grid,
                block, 0, stream, x, res, y, mean, invstd, gamma, beta, p.C,
                cdiv, total / 8);
          });
          break;
        case BnElt::scalar:
          hipLaunchKernelGGL((bn_apply_kernel<T, 1, ACT, ADD, false>), grid,
                             block, 0, stream, x, res, y, mean, invstd,
                             gamma, beta, p.C, cdiv, total);
          break;
      }
    });
  });
  HIP_CHECK_LAST();
}

template <typename T>
void ddlb::launch_bn_bwd_dx(const BnPlan& p, const T* dy, const T* y,
                            const T* x, const float* mean,
                            const float* invstd, const float* k, T* dx,
                            T* dres, const unsigned char* msk,
                            hipStream_t stream) {
  const dim3 grid = dim3_of(p.dx_grid), block(BN_BLOCK);
  const int64_t rows = p.N * p.HW, total = rows * p.C;
  const int64_t cdiv = p.nhwc ? 1 : p.HW;
  dispatch_act(p.act, [&](auto A) {
    dispatch_bool(dres != nullptr, [&](auto R) {
      constexpr int ACT = decltype(A)::value;
      constexpr bool ADD = decltype(R)::value;
      switch (p.dx) {
        case BnElt::fixed_channel:
          if constexpr (sizeof(T) == 2)
            dispatch_bool(p.dx_gate == BnGate::mask, [&](auto M) {
              constexpr bool MASKED = decltype(M)::value && ACT != 0;
              hipLaunchKernelGGL(
                  (bn_bwd_dx_fixed_kernel<ACT, ADD, MASKED>), grid, block, 0,
                  stream, dy, y, x, mean, invstd, k, dx, dres, msk, rows,
                  p.C, (int)i64min(p.C / 8, BN_LANES));
            });
          else
            throw std::logic_error(
                "bn_plan: fixed-channel dx on a 4-byte dtype");
          break;
        case BnElt::vec:
          dispatch_bool(p.nhwc != 0, [&](auto L) {
            hipLaunchKernelGGL(
                (bn_bwd_dx_kernel<T, 8, ACT, ADD, decltype(L)::value>), grid,
                block, 0, stream, dy, y, x, mean, invstd, k, dx, dres, p.C,
                cdiv, total / 8);
          });
          break;
        case BnElt::scalar:
          hipLaunchKernelGGL((bn_bwd_dx_kernel<T, 1, ACT, ADD, false>), grid,
                             block, 0, stream, dy, y, x, mean, invstd, k, dx,
                             dres, p.C, cdiv, total);
          break;
      }
    });
  });
  HIP_CHECK_LAST();
}

#define INSTANTIATE(T)                                                        \
  template void ddlb::launch_bn_stats<T>(const BnPlan&, const T*, void*,      \
                                   hipStream_t);                              \
  template void ddlb::launch_bn_apply<T>(                                     \
      const BnPlan&, const T*, const T*, T*, const float*, const float*,      \
      const float*, const float*, unsigned char*, hipStream_t);               \
  template void ddlb::launch_bn_bwd_reduce<T>(                                \
      const BnPlan&, const T*, const T*, const T*, const float*,              \
      const float*, void*, const unsigned char*, hipStream_t);                \
  template void ddlb::launch_bn_bwd_dx<T>(                                    \
      const BnPlan&, const T*, const T*, const T*, const float*,              \
      const float*, const float*, T*, T*, const unsigned char*, hipStream_t);

INSTANTIATE(float)
INSTANTIATE(__hip_bfloat16)
#undef INSTANTIATE
