// Fused attention softmax + context for gfx950, forward and backward.
//
//   attn[b,i,j] = softmax over valid j of scores[b,i,j]
//   ctx[b,i,h]  = sum_j attn[b,i,j] * values[b,j,h]
//
// scores (B,Tq,Tk) and attn are dense; values is (B,Tk,H) read through its
// batch and key strides (h stride 1), and so is the incoming dctx. A key with
// mask[b,j] == 0 has attn == 0 exactly; its score, its values row and its
// dattn entries are never read, and its dscores and dvalues are exactly 0.
// A row with no valid key gives attn = 0 and ctx = 0.
//
// Forward, one launch: a 256-thread block owns (b, 16 q rows).
//   Phase 1. Each wave takes 4 rows, lanes over j in chunks of 64. Max and
//   sum are fp32 xor butterflies over valid keys, the exponential is the
//   hardware exp2. Each probability is rounded once to the output dtype and
//   goes to global attn and to the LDS tile P[16][Tk padded to 32, + 8].
//   Phase 2, bf16. ctx = P V on v_mfma_f32_16x16x32_bf16. The block sweeps H
//   in passes of 256 columns, 64 (four 16-column tiles) per wave, and loops
//   over K = Tk in steps of 32. The A fragment is one 16 B read of P. The B
//   fragment wants j contiguous while memory has h contiguous, so each wave
//   stages its 32 x 64 piece of values through LDS with a transposing store
//   (16 B global loads, eight 2 B LDS stores into image[col][32 j + 8]) and
//   reads fragments back as 16 B rows. Rows of masked keys are stored as
//   zeros without being loaded; a K step whose 32 keys are all masked is
//   skipped. fp32 accumulation, one rounding into ctx.
//   Phase 2, fp32 and the one-row tile. Tq < 16 (the decode step) takes a
//   one-row tile, so no MFMA row is padding; it and every fp32 call run
//   phase 2 on the VALU: a thread owns column h, reads values[j][h]
//   coalesced and P[i][j] as an LDS broadcast.
//
// Backward, dscores: same block tiling. g = dctx V^T + dattn with K = h:
// both operands have h contiguous, so bf16 fragments are 16 B global loads;
// the waves take the 16-key tiles in turn and leave dP in fp32 in LDS
// (never rounded). Then, per row, ds = P (g - sum_j' P g), rounded once.
//
// Backward, dvalues: a block owns (b, 16 keys, 256 columns) and loops over
// the q rows in steps of 32: dV = P^T dctx. K = i is the strided index of
// both operands; P^T and dctx go through the same transposing stage. A block
// whose keys are all masked writes zeros and reads nothing.
//
// Operands that are not 16 B aligned (base, strides or H % 8) take scalar
// loads in the same tiling. No atomics: every sum has one fixed order.

#include "mfma_common.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace {

using bf16 = __hip_bfloat16;

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kTI = 16;           // q rows (keys, in dvalues) per block
constexpr int kKS = 32;           // MFMA K step
constexpr int kPitch = kKS + 8;   // halfwords per row of a transposed image
constexpr int kWaveCols = 64;     // columns per wave per pass
constexpr int kBlockCols = 4 * kWaveCols;

DEV bool key_valid(const uint8_t* mrow, int64_t j, int64_t Tk) {
  return j < Tk && (!mrow || mrow[j] != 0);
}

DEV float xor_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}
DEV float xor_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, WAVE));
  return v;
}

DEV bf16x8 zero8() { return bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; }
DEV f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// halfwords row[k .. k+7] when ok, zeros past H or when !ok
template <bool VEC>
DEV bf16x8 load8(const short* row, int64_t k, int64_t H, bool ok) {
  bf16x8 v = zero8();
  if constexpr (VEC) {
    if (ok && k < H) v = *reinterpret_cast<const bf16x8*>(row + k);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (ok && k + e < H) v[e] = row[k + e];
  }
  return v;
}

// One wave stages rows 0..31 x columns c0..c0+63 of a row-major bf16 matrix
// (row pitch `pitch`, H columns) as img[col][row]. Bit r of `rows` says
// whether row r may be read; every other element is stored as zero.
template <bool VEC>
DEV void stage_t(const short* src, int64_t pitch, int64_t c0, int64_t H,
                 uint32_t rows, short* img, int lane) {
  if constexpr (VEC) {
    const int c8 = lane & 7, jr = lane >> 3;
    const int64_t h = c0 + c8 * 8;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int jl = pass * 8 + jr;
      bf16x8 v = zero8();
      if (((rows >> jl) & 1u) && h < H)
        v = *reinterpret_cast<const bf16x8*>(src + jl * pitch + h);
#pragma unroll
      for (int e = 0; e < 8; ++e) img[(c8 * 8 + e) * kPitch + jl] = v[e];
    }
  } else {
    const int64_t h = c0 + lane;
    for (int jl = 0; jl < kKS; ++jl) {
      short x = 0;
      if (((rows >> jl) & 1u) && h < H) x = src[jl * pitch + h];
      img[lane * kPitch + jl] = x;
    }
  }
}

// acc[t] += A(16 x 32, rows of a) * img tile t, for a wave's four tiles
DEV void mfma4(const short* a, const short* img, int r, int kq,
               f32x4 (&acc)[4]) {
  const bf16x8 af = *reinterpret_cast<const bf16x8*>(a + kq * 8);
#pragma unroll
  for (int t = 0; t < 4; ++t)
    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        af,
        *reinterpret_cast<const bf16x8*>(img + (t * 16 + r) * kPitch + kq * 8),
        acc[t], 0, 0, 0);
}

}  // namespace

// block = (b, TI q rows). LDS: P[TI][ld] of T, then (MFMA) four wave images.
template <typename T, int TI, bool MFMA, bool VEC>
__global__ __launch_bounds__(256) void attn_ctx_fwd_kernel(
    const T* __restrict__ scores, const T* __restrict__ values,
    const uint8_t* __restrict__ mask, T* __restrict__ attn,
    T* __restrict__ ctx, int64_t Tq, int64_t Tk, int64_t H, int64_t vsb,
    int64_t vsj, int64_t n_it, int ld) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* P = reinterpret_cast<T*>(smem);
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int64_t b = blockIdx.x / n_it, i0 = (blockIdx.x % n_it) * TI;
  const uint8_t* mrow = mask ? mask + b * Tk : nullptr;
  const int64_t kp = MFMA ? (Tk + kKS - 1) / kKS * kKS : Tk;

  constexpr int RPW = TI == kTI ? 4 : 1;  // rows per wave
  if (TI == kTI || wave == 0) {
    for (int rr = 0; rr < RPW; ++rr) {
      const int ii = wave * RPW + rr;
      const int64_t i = i0 + ii;
      T* prow = P + ii * ld;
      if (i >= Tq) {  // a padding row of the MFMA tile
        for (int64_t j = lane; j < kp; j += WAVE) prow[j] = from_f32<T>(0.f);
        continue;
      }
      const T* srow = scores + (b * Tq + i) * Tk;
      float m = -INFINITY;
      for (int64_t j = lane; j < Tk; j += WAVE)
        if (key_valid(mrow, j, Tk)) m = fmaxf(m, to_f32(srow[j]));
      m = xor_max(m);
      float sum = 0.f;
      for (int64_t j = lane; j < Tk; j += WAVE)
        if (key_valid(mrow, j, Tk))
          sum += __builtin_amdgcn_exp2f((to_f32(srow[j]) - m) * kLog2e);
      sum = xor_sum(sum);
      const float inv = sum > 0.f ? 1.f / sum : 0.f;
      T* arow = attn + (b * Tq + i) * Tk;
      for (int64_t j = lane; j < kp; j += WAVE) {
        T p = from_f32<T>(0.f);
        if (key_valid(mrow, j, Tk))
          p = from_f32<T>(
              __builtin_amdgcn_exp2f((to_f32(srow[j]) - m) * kLog2e) * inv);
        prow[j] = p;
        if (j < Tk) arow[j] = p;
      }
    }
  }
  __syncthreads();

  if constexpr (!MFMA) {
    const T* vb = values + b * vsb;
    for (int64_t h = tid; h < H; h += 256) {
      float acc[TI];
#pragma unroll
      for (int ii = 0; ii < TI; ++ii) acc[ii] = 0.f;
      for (int64_t j = 0; j < Tk; ++j) {
        if (mrow && mrow[j] == 0) continue;  // block-uniform
        const float v = to_f32(vb[j * vsj + h]);
#pragma unroll
        for (int ii = 0; ii < TI; ++ii) acc[ii] += to_f32(P[ii * ld + j]) * v;
      }
#pragma unroll
      for (int ii = 0; ii < TI; ++ii)
        if (i0 + ii < Tq)
          ctx[(b * Tq + i0 + ii) * H + h] = from_f32<T>(acc[ii]);
    }
  } else {
    const short* Ps = reinterpret_cast<const short*>(smem);
    short* img = reinterpret_cast<short*>(smem) + kTI * ld +
                 wave * kWaveCols * kPitch;
    const short* vb = reinterpret_cast<const short*>(values) + b * vsb;
    const int r = lane & 15, kq = lane >> 4;
    const int nks = (int)(kp / kKS);
    for (int64_t h0 = 0; h0 < H; h0 += kBlockCols) {
      const int64_t c0 = h0 + wave * kWaveCols;
      f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
      for (int ks = 0; ks < nks; ++ks) {
        // the same bits in every wave: the branch is block-uniform
        const uint32_t rows = (uint32_t)__ballot(
            lane < kKS && key_valid(mrow, (int64_t)ks * kKS + lane, Tk));
        if (rows == 0) continue;
        __syncthreads();
        stage_t<VEC>(vb + (int64_t)ks * kKS * vsj, vsj, c0, H, rows, img,
                     lane);
        __syncthreads();
        mfma4(Ps + r * ld + ks * kKS, img, r, kq, acc);
      }
      // accumulator element e of a lane is (row 4 kq + e, col r) of a tile
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t i = i0 + kq * 4 + e, h = c0 + t * 16 + r;
          if (i < Tq && h < H)
            ctx[(b * Tq + i) * H + h] = from_f32<T>(acc[t][e]);
        }
    }
  }
}

// block = (b, TI q rows). LDS: G[TI][ldg] fp32, g without the dattn term.
template <typename T, int TI, bool MFMA, bool VEC>
__global__ __launch_bounds__(256) void attn_ctx_bwd_ds_kernel(
    const T* __restrict__ dctx, const T* __restrict__ dattn,
    const T* __restrict__ attn, const T* __restrict__ values,
    const uint8_t* __restrict__ mask, T* __restrict__ ds, int64_t Tq,
    int64_t Tk, int64_t H, int64_t vsb, int64_t vsj, int64_t dsb,
    int64_t dsi, int64_t n_it, int ldg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* G = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int64_t b = blockIdx.x / n_it, i0 = (blockIdx.x % n_it) * TI;
  const uint8_t* mrow = mask ? mask + b * Tk : nullptr;

  if constexpr (MFMA) {
    const int r = lane & 15, kq = lane >> 4;
    const bool ok_i = i0 + r < Tq;
    const short* drow =
        reinterpret_cast<const short*>(dctx) + b * dsb + (i0 + r) * dsi;
    for (int64_t j0 = (int64_t)wave * 16; j0 < Tk; j0 += 64) {
      const bool ok_j = key_valid(mrow, j0 + r, Tk);
      if (__ballot(ok_j) == 0) continue;  // a masked tile: G stays unread
      const short* vrow =
          reinterpret_cast<const short*>(values) + b * vsb + (j0 + r) * vsj;
      f32x4 acc = zero4();
      for (int64_t k0 = 0; k0 < H; k0 += kKS) {
        const int64_t k = k0 + kq * 8;
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            load8<VEC>(drow, k, H, ok_i), load8<VEC>(vrow, k, H, ok_j), acc,
            0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) G[(kq * 4 + e) * ldg + j0 + r] = acc[e];
    }
  } else {
    // a wave per (i, j): lanes over h, one butterfly
    for (int64_t idx = wave; idx < TI * Tk; idx += 4) {
      const int ii = (int)(idx / Tk);
      const int64_t j = idx % Tk, i = i0 + ii;
      if (i >= Tq || (mrow && mrow[j] == 0)) continue;
      const T* drow = dctx + b * dsb + i * dsi;
      const T* vrow = values + b * vsb + j * vsj;
      float s = 0.f;
      for (int64_t h = lane; h < H; h += WAVE)
        s += to_f32(drow[h]) * to_f32(vrow[h]);
      s = xor_sum(s);
      if (lane == 0) G[ii * ldg + j] = s;
    }
  }
  __syncthreads();

  constexpr int RPW = TI == kTI ? 4 : 1;
  if (TI != kTI && wave != 0) return;
  for (int rr = 0; rr < RPW; ++rr) {
    const int ii = wave * RPW + rr;
    const int64_t i = i0 + ii;
    if (i >= Tq) continue;
    const int64_t row = (b * Tq + i) * Tk;
    float dot = 0.f;
    for (int64_t j = lane; j < Tk; j += WAVE)
      if (key_valid(mrow, j, Tk)) {
        float g = G[ii * ldg + j];
        if (dattn) g += to_f32(dattn[row + j]);
        dot += to_f32(attn[row + j]) * g;
      }
    dot = xor_sum(dot);
    for (int64_t j = lane; j < Tk; j += WAVE) {
      float d = 0.f;
      if (key_valid(mrow, j, Tk)) {
        float g = G[ii * ldg + j];
        if (dattn) g += to_f32(dattn[row + j]);
        d = to_f32(attn[row + j]) * (g - dot);
      }
      ds[row + j] = from_f32<T>(d);
    }
  }
}

// block = (b, 16 keys, 256 columns); dv is dense (B, Tk, H)
template <typename T, bool MFMA, bool VEC>
__global__ __launch_bounds__(256) void attn_ctx_bwd_dv_kernel(
    const T* __restrict__ dctx, const T* __restrict__ attn,
    const uint8_t* __restrict__ mask, T* __restrict__ dv, int64_t Tq,
    int64_t Tk, int64_t H, int64_t dsb, int64_t dsi, int64_t n_jt,
    int64_t n_hc) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int64_t hc = blockIdx.x % n_hc, jt = (blockIdx.x / n_hc) % n_jt,
                b = blockIdx.x / (n_hc * n_jt);
  const int64_t j0 = jt * kTI, h0 = hc * kBlockCols;
  const uint8_t* mrow = mask ? mask + b * Tk : nullptr;

  if (__ballot(key_valid(mrow, j0 + (lane & 15), Tk)) == 0) {
    for (int idx = tid; idx < kTI * kBlockCols; idx += 256) {
      const int64_t j = j0 + idx / kBlockCols, h = h0 + idx % kBlockCols;
      if (j < Tk && h < H) dv[(b * Tk + j) * H + h] = from_f32<T>(0.f);
    }
    return;
  }

  if constexpr (!MFMA) {
    const int64_t h = h0 + tid;
    if (h >= H) return;
    float acc[kTI];
#pragma unroll
    for (int jj = 0; jj < kTI; ++jj) acc[jj] = 0.f;
    for (int64_t i = 0; i < Tq; ++i) {
      const float d = to_f32(dctx[b * dsb + i * dsi + h]);
      const T* arow = attn + (b * Tq + i) * Tk;
#pragma unroll
      for (int jj = 0; jj < kTI; ++jj)
        if (j0 + jj < Tk) acc[jj] += to_f32(arow[j0 + jj]) * d;
    }
#pragma unroll
    for (int jj = 0; jj < kTI; ++jj)
      if (j0 + jj < Tk)
        dv[(b * Tk + j0 + jj) * H + h] =
            from_f32<T>(key_valid(mrow, j0 + jj, Tk) ? acc[jj] : 0.f);
  } else {
    __shared__ __attribute__((aligned(16))) short Pt[kTI * kPitch];
    __shared__ __attribute__((aligned(16))) short Dt[4 * kWaveCols * kPitch];
    short* img = Dt + wave * kWaveCols * kPitch;
    const short* as = reinterpret_cast<const short*>(attn) + b * Tq * Tk;
    const short* dsrc = reinterpret_cast<const short*>(dctx) + b * dsb;
    const int r = lane & 15, kq = lane >> 4;
    const int64_t c0 = h0 + wave * kWaveCols;
    f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
    for (int64_t i0 = 0; i0 < Tq; i0 += kKS) {
      __syncthreads();
      // P^T: thread -> (key tid % 16, q rows tid / 16 and tid / 16 + 16)
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int il = tid / 16 + pass * 16, jl = tid % 16;
        const int64_t i = i0 + il, j = j0 + jl;
        Pt[jl * kPitch + il] = (i < Tq && j < Tk) ? as[i * Tk + j] : (short)0;
      }
      const int64_t left = Tq - i0;
      const uint32_t rows = left >= kKS ? 0xffffffffu : (1u << left) - 1u;
      stage_t<VEC>(dsrc + i0 * dsi, dsi, c0, H, rows, img, lane);
      __syncthreads();
      mfma4(Pt + r * kPitch, img, r, kq, acc);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t j = j0 + kq * 4 + e, h = c0 + t * 16 + r;
        if (j < Tk && h < H)
          dv[(b * Tk + j) * H + h] =
              from_f32<T>(key_valid(mrow, j, Tk) ? acc[t][e] : 0.f);
      }
  }
}

namespace {

bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// 16 B fragment loads: H, both strides and the base in 8-halfword units
template <typename T>
bool vec_ok(const T* p, int64_t H, int64_t s0, int64_t s1) {
  return H % 8 == 0 && s0 % 8 == 0 && s1 % 8 == 0 && aligned16(p);
}

void check_tk(int64_t Tk) {
  if (Tk > ddlb::kAttnCtxMaxTk)
    throw std::runtime_error(
        "attn_ctx: Tk = " + std::to_string(Tk) + " is over the cap of " +
        std::to_string(ddlb::kAttnCtxMaxTk) +
        " keys (the 16-row probability tile must fit in 64 KiB of LDS)");
}

}  // namespace

template <typename T>
void ddlb::launch_attn_ctx_fwd(const T* scores, const T* values,
                               const uint8_t* mask, T* attn, T* ctx,
                               int64_t B, int64_t Tq, int64_t Tk, int64_t H,
                               int64_t vsb, int64_t vsj, hipStream_t stream) {
  if (B == 0 || Tq == 0 || Tk == 0 || H == 0) return;
  check_tk(Tk);
  const bool one = Tq < kTI;
  const int64_t n_it = one ? Tq : (Tq + kTI - 1) / kTI;
  const dim3 grid((uint32_t)(B * n_it));
#define ATTN_CTX_FWD(TI, MFMA, VEC, LD, LDS)                                 \
  hipLaunchKernelGGL((attn_ctx_fwd_kernel<T, TI, MFMA, VEC>), grid,          \
                     dim3(256), (LDS), stream, scores, values, mask, attn,   \
                     ctx, Tq, Tk, H, vsb, vsj, n_it, (int)(LD))
  if (one) {
    ATTN_CTX_FWD(1, false, false, Tk, Tk * sizeof(T));
  } else if constexpr (std::is_same<T, __hip_bfloat16>::value) {
    const int64_t ld = (Tk + kKS - 1) / kKS * kKS + 8;
    const size_t lds = (kTI * ld + 4 * kWaveCols * kPitch) * sizeof(short);
    if (vec_ok(values, H, vsb, vsj)) ATTN_CTX_FWD(kTI, true, true, ld, lds);
    else ATTN_CTX_FWD(kTI, true, false, ld, lds);
  } else {
    ATTN_CTX_FWD(kTI, false, false, Tk, kTI * Tk * sizeof(T));
  }
#undef ATTN_CTX_FWD
  HIP_CHECK_LAST();
}

template <typename T>
void ddlb::launch_attn_ctx_bwd(const T* dctx, const T* dattn, const T* attn,
                               const T* values, const uint8_t* mask,
                               T* dscores, T* dvalues, int64_t B, int64_t Tq,
                               int64_t Tk, int64_t H, int64_t vsb,
                               int64_t vsj, int64_t dsb, int64_t dsi,
                               hipStream_t stream) {
  if (B == 0 || Tq == 0 || Tk == 0 || H == 0) return;
  check_tk(Tk);
  constexpr bool is_bf16 = std::is_same<T, __hip_bfloat16>::value;
  const bool dvec = vec_ok(dctx, H, dsb, dsi);
  if (dscores) {
    const bool one = Tq < kTI;
    const int64_t n_it = one ? Tq : (Tq + kTI - 1) / kTI;
    const int64_t ldg = (Tk + 15) / 16 * 16;
    const dim3 grid((uint32_t)(B * n_it));
#define ATTN_CTX_DS(TI, MFMA, VEC)                                           \
  hipLaunchKernelGGL((attn_ctx_bwd_ds_kernel<T, TI, MFMA, VEC>), grid,       \
                     dim3(256), (TI) * ldg * sizeof(float), stream, dctx,    \
                     dattn, attn, values, mask, dscores, Tq, Tk, H, vsb,     \
                     vsj, dsb, dsi, n_it, (int)ldg)
    if (one) {
      ATTN_CTX_DS(1, false, false);
    } else if constexpr (is_bf16) {
      if (dvec && vec_ok(values, H, vsb, vsj)) ATTN_CTX_DS(kTI, true, true);
      else ATTN_CTX_DS(kTI, true, false);
    } else {
      ATTN_CTX_DS(kTI, false, false);
    }
#undef ATTN_CTX_DS
    HIP_CHECK_LAST();
  }
  if (dvalues) {
    const int64_t n_jt = (Tk + kTI - 1) / kTI;
    const int64_t n_hc = (H + kBlockCols - 1) / kBlockCols;
    const dim3 grid((uint32_t)(B * n_jt * n_hc));
#define ATTN_CTX_DV(MFMA, VEC)                                               \
  hipLaunchKernelGGL((attn_ctx_bwd_dv_kernel<T, MFMA, VEC>), grid,           \
                     dim3(256), 0, stream, dctx, attn, mask, dvalues, Tq,    \
                     Tk, H, dsb, dsi, n_jt, n_hc)
    if constexpr (is_bf16) {
      if (dvec) ATTN_CTX_DV(true, true);
      else ATTN_CTX_DV(true, false);
    } else {
      ATTN_CTX_DV(false, false);
    }
#undef ATTN_CTX_DV
    HIP_CHECK_LAST();
  }
}

#define INSTANTIATE(T)                                                       \
  template void ddlb::launch_attn_ctx_fwd<T>(                                \
      const T*, const T*, const uint8_t*, T*, T*, int64_t, int64_t, int64_t, \
      int64_t, int64_t, int64_t, hipStream_t);                               \
  template void ddlb::launch_attn_ctx_bwd<T>(                                \
      const T*, const T*, const T*, const T*, const uint8_t*, T*, T*,        \
      int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,         \
      int64_t, hipStream_t);
INSTANTIATE(float)
INSTANTIATE(__hip_bfloat16)
#undef INSTANTIATE
