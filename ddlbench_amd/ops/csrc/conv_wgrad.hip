// NHWC bf16 convolution weight-grad on MFMA (gfx950) — completes the
// native conv triple (fprop/dgrad in conv_mfma*.hip).
//
//   dw[k][r,s,c] = sum_{n,oh,ow} dy[n,oh,ow,k] * x[n, oh*st+r-p, ow*st+s-p, c]
//
// GEMM view: C[k][rsc] = A[k][p] * B[p][rsc], reduction over output
// pixels p. Both operands are p-major in memory (transposed from the
// MFMA fragment layout), so tiles stage into a ds_read_b64_tr_b16 image
// and fragments come out of the HARDWARE TRANSPOSE READ — one b64-class
// LDS instruction per 4 fragment elements instead of per-element
// scalar gathers.
//
// Structure:
//   * TKt x TRt dw tile (64 or 128 per side, by shape), BP=64 pixels
//     per step, 256 or 512 threads.
//   * tr image per operand: 4 column groups x [two p-parity
//     sub-images] x [p/8][4][16] halfword blocks; glds stages it with
//     lane-linear 16-B chunks whose SOURCE index is decoded per slot
//     (cdna_hip_programming.md T10: lane l of a 16-lane group reads
//     column l&15 of a [4][16] block at lane-linear 8-B addresses).
//   * 3-buffer LDS ring, staging 2 steps ahead, counted s_waitcnt
//     vmcnt(GA+GB) per step, raw s_barrier (never __syncthreads with
//     glds in flight). The 128x128 tile runs a 2-buffer ring instead
//     and overlaps through its co-resident second block.
//   * split-P partial slabs [split][K][RSC] fp32 + a combine kernel —
//     no per-tile global atomics (a C64K64R1 layer would serialize
//     ~2048 atomic adds per dw element).
//   * bf16 output (the weight's dtype, same (K, R*S*C) memory): the
//     epilogue rounds the accumulator when split == 1, otherwise an
//     ordered combine adds each element's slabs in slab order and rounds
//     once — no memset, no atomics, the same bits every call.
//
// Constraints: bf16, K % 8 == 0, C % 8 == 0.

#include "mfma_common.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <string>

using bf16 = __hip_bfloat16;
typedef __attribute__((address_space(3))) const short* lds_cptr;

#define WG_BKP 64     // p rows per step

struct WgradParams {
  const bf16* x;      // (N,H,W,C) memory
  const bf16* dy;     // (N,OH,OW,K) memory
  float* dw;          // (K, R*S*C) fp32 output
  bf16* dwb;          // non-null: bf16 output instead of dw
  float* part;        // [split][K][RSC] fp32 partial slabs (split>1)
  const bf16* zero;
  int N, H, W, C, K, OH, OW, R, S, stride, pad;
  long P;             // N*OH*OW
  long RSC;
  int split_p;        // p-chunks per (k,rsc) tile
};

namespace {

// tr image geometry (per operand, per buffer): 4 column groups g of 16,
// each a pair of p-parity sub-images of [BP/8][4][16] halfword blocks:
//   half(p, ch) = g*BP*16 + ((p>>2)&1)*BP*8 + (p>>3)*64 + (p&3)*16
//                 + (ch&15)
// A 16-B staging chunk d in [0, 512) covers (p, ch0=8*h8):
DEV void wg_decode_chunk(int d, int& p, int& ch) {
  const int g = d >> 7;
  const int r = d & 127;
  const int phalf = r >> 6;
  const int r2 = r & 63;
  p = (r2 >> 3) * 8 + phalf * 4 + ((r2 >> 1) & 3);
  ch = g * 16 + (r2 & 1) * 8;
}

DEV bf16x8 wg_tr_frag(const short* img, int group, int ks, int lane) {
  // fragment (m/n-col = lane&15, p = ks*32 + (lane>>4)*8 + e):
  // two tr reads (p parity halves) at lane-linear 8-B addresses
  bf16x4 lo, hi;
  lds_cptr base = (lds_cptr)(img + group * (WG_BKP * 16) + ks * 4 * 64 +
                             lane * 4);
  asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
               "ds_read_b64_tr_b16 %1, %2 offset:%3"
               : "=&v"(lo), "=&v"(hi)
               : "v"(base), "i"(WG_BKP * 8 * 2));
  bf16x8 f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[e] = lo[e];
    f[4 + e] = hi[e];
  }
  return f;
}

// TKt x TRt dw tile, WR x WC waves. The 128x128 tile halves both
// operands' cross-tile re-staging (the 64x64 tile is staging-BW-bound:
// A re-reads x nr, B x nk).
// R1: 1x1 stride-1 pad-0 conv — B (im2col x) degenerates to the plain
// row-major tensor; skip the per-step carry chain and bounds tests
template <int TKt, int TRt, int WR, int WC, int TPB, bool R1, bool RING2>
__global__ __launch_bounds__(TPB, RING2 ? 4 : 2)
void conv_wgrad2_kernel(WgradParams q) {
  constexpr int NBUF = RING2 ? 2 : 3;
  constexpr int GA = TKt * 8 / TPB;  // A glds chunks per thread per step
  constexpr int GB = TRt * 8 / TPB;  // B
  constexpr int MFS = TKt / WR / 16; // A fragments per wave
  constexpr int NFS = TRt / WC / 16; // B fragments per wave
  static_assert(WR * WC == TPB / 64, "wave count");
  static_assert(GA >= 1 && GB >= 1, "tile vs threads");
  // 3-buffer ring: [buf][A TKtx64 | B TRtx64] bf16
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* lds = reinterpret_cast<short*>(smem);
  auto aimg = [&](int buf) { return lds + buf * WG_BKP * (TKt + TRt); };
  auto bimg = [&](int buf) { return aimg(buf) + WG_BKP * TKt; };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;

  const int nk = (q.K + TKt - 1) / TKt;
  const int nr = (int)((q.RSC + TRt - 1) / TRt);
  const long block = blockIdx.x;
  const long kb = (block % nk) * TKt;
  const long rb = ((block / nk) % nr) * TRt;
  const int ps_idx = (int)(block / ((long)nk * nr));
  const long p_per = (q.P + q.split_p - 1) / q.split_p;
  const long p_begin = ps_idx * p_per;
  const long p_end = i64min(p_begin + p_per, q.P);
  const int nsteps = (int)((p_end - p_begin + WG_BKP - 1) / WG_BKP);

  // ---- staging slots: GA/GB chunks per thread per operand --------------
  // A (dy): source advances linearly by BP*K per step.
  // B (x im2col): fixed (r,s,c0) per slot; (n,oh,ow) advances by BP
  // rows per step with carries.
  int a_p[GA], a_ch[GA];
  const bf16* a_src[GA];
  bool a_chok[GA];
  long a_pabs[GA];
  int bp_[GB], b_r[GB], b_s[GB], b_c0[GB];
  int b_n[GB], b_ohw[GB];  // (oh << 16) | ow
  bool b_rscok[GB];
  long b_pabs[GB];
  const bf16* b_lin[GB];  // R1: linear source pointers
#pragma unroll
  for (int j = 0; j < GA; ++j) {
    const int d = j * TPB + tid;
    wg_decode_chunk(d, a_p[j], a_ch[j]);
    a_chok[j] = kb + a_ch[j] < q.K;
    a_src[j] = q.dy + (p_begin + a_p[j]) * q.K + kb + a_ch[j];
    a_pabs[j] = p_begin + a_p[j];
  }
#pragma unroll
  for (int j = 0; j < GB; ++j) {
    const int d = j * TPB + tid;
    int bch;
    wg_decode_chunk(d, bp_[j], bch);
    const long rsc = rb + bch;
    b_rscok[j] = rsc < q.RSC;
    const long rr = b_rscok[j] ? rsc : 0;
    b_c0[j] = (int)(rr % q.C);
    const int rs = (int)(rr / q.C);
    b_r[j] = rs / q.S;
    b_s[j] = rs - b_r[j] * q.S;
    // decompose pixel p_begin + p once
    const long pp = p_begin + bp_[j];
    const int ohw = q.OH * q.OW;
    const long ppc = pp < q.P ? pp : 0;
    b_n[j] = (int)(ppc / ohw);
    const int rem = (int)(ppc - (long)b_n[j] * ohw);
    const int oh0 = rem / q.OW;
    b_ohw[j] = (oh0 << 16) | (rem - oh0 * q.OW);
    b_pabs[j] = pp;
    if (R1) b_lin[j] = q.x + (p_begin + bp_[j]) * q.C + b_c0[j];
  }

  auto stage = [&](int buf, int t) {
    short* la = aimg(buf);
    short* lb = bimg(buf);
    const long plim = p_end;
#pragma unroll
    for (int j = 0; j < GA; ++j) {
      const int d = j * TPB + tid;
      const bf16* src =
          (a_chok[j] && a_pabs[j] + (long)t * WG_BKP < plim)
              ? a_src[j] + (long)t * WG_BKP * q.K
              : q.zero;
      glds16(src, la + d * 8);
    }
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      const int d = j * TPB + tid;
      // advance (n,oh,ow) to step t lazily: ow' = ow + t*BP with carry
      // would need history; instead recompute from the running state —
      // the stage calls are strictly t = 0,1,2,... so the running state
      // IS step t's state; advance after use.
      const bf16* src = q.zero;
      if (R1) {
        if (b_rscok[j] && b_pabs[j] + (long)t * WG_BKP < plim)
          src = b_lin[j] + (long)t * WG_BKP * q.C;
      } else if (b_rscok[j] && b_pabs[j] + (long)t * WG_BKP < plim) {
        const int ih = (b_ohw[j] >> 16) * q.stride + b_r[j] - q.pad;
        const int iw = (b_ohw[j] & 0xffff) * q.stride + b_s[j] - q.pad;
        if (ih >= 0 && ih < q.H && iw >= 0 && iw < q.W)
          src = q.x + (((long)b_n[j] * q.H + ih) * q.W + iw) * q.C +
                b_c0[j];
      }
      glds16(src, lb + d * 8);
      if (!R1) {
        // advance the pixel coords by BP rows (carry chain)
        int oh = b_ohw[j] >> 16, ow = (b_ohw[j] & 0xffff) + WG_BKP;
        while (ow >= q.OW) {
          ow -= q.OW;
          if (++oh == q.OH) {
            oh = 0;
            ++b_n[j];
          }
        }
        b_ohw[j] = (oh << 16) | ow;
      }
    }
  };

  const int wk = wid / WC;
  const int wc = wid % WC;
  f32x4 acc[MFS][NFS];
#pragma unroll
  for (int i = 0; i < MFS; ++i)
#pragma unroll
    for (int j = 0; j < NFS; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // ---- prologue: stage steps 0 and 1 -----------------------------------
  stage(0, 0);
  if (!RING2 && nsteps > 1) {
    stage(1, 1);
    wait_vmcnt<GA + GB>();  // step 0 landed, step 1 in flight
  } else {
    wait_vmcnt<0>();
  }
  __builtin_amdgcn_s_barrier();

  for (int t = 0; t < nsteps; ++t) {
    const short* la = aimg(t % NBUF);
    const short* lb = bimg(t % NBUF);
    // fragments via hardware transpose read; process the two 32-p
    // halves (ks) back to back
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[MFS], bf_[NFS];
#pragma unroll
      for (int nf = 0; nf < NFS; ++nf)
        bf_[nf] = wg_tr_frag(lb, wc * NFS + nf, ks, lane);
#pragma unroll
      for (int mf = 0; mf < MFS; ++mf)
        af[mf] = wg_tr_frag(la, wk * MFS + mf, ks, lane);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);  // keep MFMAs behind the wait
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mf = 0; mf < MFS; ++mf)
#pragma unroll
        for (int nf = 0; nf < NFS; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mf], bf_[nf], acc[mf][nf], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    if (RING2) {
      // 2-buffer ring: stage t+1 after this step's MFMAs, drain, swap.
      // Overlap comes from the co-resident second block, not from
      // loads spanning barriers.
      if (t + 1 < nsteps) stage((t + 1) % 2, t + 1);
      wait_vmcnt<0>();
    } else if (t + 2 < nsteps) {
      stage((t + 2) % 3, t + 2);
      wait_vmcnt<GA + GB>();
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
  }

  // ---- write the tile: partial slab (split>1) or dw directly ----------
  float* out = (q.split_p > 1)
                   ? q.part + (long)ps_idx * q.K * q.RSC
                   : q.dw;
#pragma unroll
  for (int mf = 0; mf < MFS; ++mf) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const long k = kb + (wk * MFS + mf) * 16 + (lane >> 4) * 4 + reg;
      if (k >= q.K) continue;
#pragma unroll
      for (int nf = 0; nf < NFS; ++nf) {
        const long rsc = rb + (wc * NFS + nf) * 16 + (lane & 15);
        if (rsc >= q.RSC) continue;
        if (q.split_p == 1 && q.dwb != nullptr)
          q.dwb[k * q.RSC + rsc] = __float2bfloat16(acc[mf][nf][reg]);
        else
          out[k * q.RSC + rsc] = acc[mf][nf][reg];
      }
    }
  }
}

// Ordered combine: element i's slabs are added in slab order. Thread
// (tx, ty) owns V consecutive elements and slabs [64*ty, 64*ty + 64),
// summed from 0.f upwards exactly as wgrad_combine_kernel sums a 64-slab
// chunk; blockDim.y > 1 (split > 64) then adds the chunk sums in ty
// order through LDS, so a small dw with many slabs still spreads over
// blockDim.y times the threads. The result is rounded once to OutT.
template <typename OutT, int V, int TX, int TY>
__global__ void wgrad_combine_ordered_kernel(const float* __restrict__ part,
                                             OutT* __restrict__ dw,
                                             long total, long stride_elems,
                                             int split) {
  __shared__ float sh[TY][TX][V];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const long i = ((long)blockIdx.x * TX + tx) * V;
  const int ps0 = ty * 64;
  const int ps1 = min(ps0 + 64, split);
  float s[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s[j] = 0.f;
  if (i < total) {
#pragma unroll 4
    for (int ps = ps0; ps < ps1; ++ps) {
      const float* src = part + ps * stride_elems + i;
      if constexpr (V == 4) {
        typedef __attribute__((ext_vector_type(4))) float float4x;
        const float4x v = *reinterpret_cast<const float4x*>(src);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += v[j];
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) s[j] += src[j];
      }
    }
  }
  if (TY > 1 && blockDim.y > 1) {
#pragma unroll
    for (int j = 0; j < V; ++j) sh[ty][tx][j] = s[j];
    __syncthreads();
    if (ty != 0) return;
    for (int g = 1; g < (int)blockDim.y; ++g)
#pragma unroll
      for (int j = 0; j < V; ++j) s[j] += sh[g][tx][j];
  }
  if (i >= total) return;
#pragma unroll
  for (int j = 0; j < V; ++j) dw[i + j] = from_f32<OutT>(s[j]);
}

// 2D combine: blockIdx.y covers 64-slab chunks (atomics per element are
// <= ceil(split/64)-way) so small dw tensors still parallelize
__global__ void wgrad_combine_kernel(const float* __restrict__ part,
                                     float* __restrict__ dw, long total,
                                     long stride_elems, int split) {
  const int ps0 = blockIdx.y * 64;
  const int ps1 = min(ps0 + 64, split);
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long gstride = (long)gridDim.x * blockDim.x;
  for (long i = i0; i < total; i += gstride) {
    float s = 0.f;
    for (int ps = ps0; ps < ps1; ++ps) s += part[ps * stride_elems + i];
    if (gridDim.y > 1)
      atomicAdd(&dw[i], s);
    else
      dw[i] = s;
  }
}

// R1 is a property of the conv, the tile a property of the dw shape
template <int TKt, int TRt, int WR, int WC, int TPB, bool RING2>
void wg_launch(const WgradParams& q, bool r1, unsigned grid, size_t lds,
               hipStream_t stream) {
  if (r1)
    hipLaunchKernelGGL(
        (conv_wgrad2_kernel<TKt, TRt, WR, WC, TPB, true, RING2>),
        dim3(grid), dim3(TPB), lds, stream, q);
  else
    hipLaunchKernelGGL(
        (conv_wgrad2_kernel<TKt, TRt, WR, WC, TPB, false, RING2>),
        dim3(grid), dim3(TPB), lds, stream, q);
}

}  // namespace

ddlb::ConvWgradPlan ddlb::conv_wgrad_plan(int N, int C, int K, int OH,
                                          int OW, int R, int S, int stride,
                                          int pad, long part_cap) {
  ConvWgradPlan pl;
  const long P = (long)N * OH * OW;
  const long RSC = (long)R * S * C;
  // tile by shape: square 128 where possible (least re-staging),
  // rectangular when only one dim allows it
  const bool bigK = K >= 128, bigR = RSC >= 128;
  pl.tk = bigK ? 128 : 64;
  pl.tr = bigR ? 128 : 64;
  pl.nk = (K + pl.tk - 1) / pl.tk;
  pl.nr = (RSC + pl.tr - 1) / pl.tr;
  long split = 2048 / i64max(pl.nk * pl.nr, 1);
  split = i64max(i64min(split, (P + WG_BKP - 1) / WG_BKP), 1);
  split = i64min(split, 256);  // combine traffic cap
  if (split > 1)
    split = i64min(split, part_cap / i64max((long)K * RSC, 1));
  split = i64max(split, 1);
  pl.split = split;
  // square tile: 512 threads on a 2-buffer ring (64 KiB, 2 blocks/CU);
  // smaller tiles: 256 threads on the 3-buffer ring
  pl.ring = (bigK && bigR) ? 2 : 3;
  pl.r1 = (R == 1 && S == 1 && stride == 1 && pad == 0);
  // the kernel's chunking: chunk i covers [i*p_per, min((i+1)*p_per, P))
  pl.p_per = (P + split - 1) / split;
  pl.steps = (pl.p_per + WG_BKP - 1) / WG_BKP;
  pl.tail = pl.p_per - (pl.steps - 1) * WG_BKP;
  pl.psb = split > 1 ? (split + 63) / 64 : 0;
  return pl;
}

void ddlb::launch_conv_wgrad(const void* x, const void* dy, float* dw,
                             float* part_ws, long part_cap, const void* zero,
                             int N, int H, int W, int C, int K, int OH, int OW,
                             int R, int S, int stride, int pad,
                             hipStream_t stream, void* dw_bf16) {
  WgradParams q;
  q.x = (const bf16*)x;
  q.dy = (const bf16*)dy;
  q.dw = dw;
  q.dwb = (bf16*)dw_bf16;
  q.part = part_ws;
  q.zero = (const bf16*)zero;
  q.N = N; q.H = H; q.W = W; q.C = C; q.K = K; q.OH = OH; q.OW = OW;
  q.R = R; q.S = S; q.stride = stride; q.pad = pad;
  q.P = (long)N * OH * OW;
  q.RSC = (long)R * S * C;

  const ConvWgradPlan pl = conv_wgrad_plan(N, C, K, OH, OW, R, S, stride,
                                           pad, part_cap);
  q.split_p = (int)pl.split;
  const size_t lds = pl.ring * WG_BKP * (pl.tk + pl.tr) * sizeof(bf16);
  const bool r1 = pl.r1 != 0;
  const unsigned grid = (unsigned)(pl.nk * pl.nr * q.split_p);
  if (pl.tk == 128 && pl.tr == 128)
    wg_launch<128, 128, 2, 4, 512, true>(q, r1, grid, lds, stream);
  else if (pl.tr == 128)
    wg_launch<64, 128, 1, 4, 256, false>(q, r1, grid, lds, stream);
  else if (pl.tk == 128)
    wg_launch<128, 64, 4, 1, 256, false>(q, r1, grid, lds, stream);
  else
    wg_launch<64, 64, 1, 4, 256, false>(q, r1, grid, lds, stream);
  if (q.split_p > 1 && q.dwb != nullptr) {
    // total % 8 == 0 (C % 8 == 0); psb <= 4 (split <= 256)
    const long total = q.K * q.RSC;
    if (pl.psb > 4)
      throw std::runtime_error("conv_wgrad: ordered combine needs split <= 256");
    if (pl.psb <= 1) {
      const unsigned blocks = (unsigned)((total / 4 + 255) / 256);
      hipLaunchKernelGGL((wgrad_combine_ordered_kernel<bf16, 4, 256, 1>),
                         dim3(blocks), dim3(256, 1), 0, stream, part_ws,
                         q.dwb, total, total, q.split_p);
    } else {
      const unsigned blocks = (unsigned)((total + 31) / 32);
      hipLaunchKernelGGL((wgrad_combine_ordered_kernel<bf16, 1, 32, 4>),
                         dim3(blocks), dim3(32, (unsigned)pl.psb), 0, stream,
                         part_ws, q.dwb, total, total, q.split_p);
    }
  } else if (q.split_p > 1) {
    const long total = q.K * q.RSC;
    const int blocks = (int)i64min((total + 255) / 256, 2048);
    const int psb = (int)pl.psb;
    // multi-chunk combine accumulates with atomics -> dw must be 0
    // (dw arrives as torch::empty; the single-chunk combine writes)
    if (psb > 1)
      hipMemsetAsync(dw, 0, total * sizeof(float), stream);
    hipLaunchKernelGGL(wgrad_combine_kernel, dim3(blocks, psb),
                       dim3(256), 0,
                       stream, part_ws, dw, total, total, q.split_p);
  }
  HIP_CHECK_LAST();
}
