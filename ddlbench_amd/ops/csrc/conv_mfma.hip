// NHWC implicit-GEMM convolution on MFMA matrix cores (gfx950, bf16).
//
// The conv/GEMM core the reference gets from cuDNN (SURVEY.md §2.11
// "MI355X plan implication"), hand-written for CDNA4:
//   y[n,oh,ow,k] = sum_{r,s,c} x[n, oh*st+r-p, ow*st+s-p, c] * w[k,r,s,c]
// viewed as GEMM  C[M=N*OH*OW][Nd=K] = A[M][Kd=R*S*C] * B[Nd][Kd]^T
// with A materialized implicitly (im2col addressing in the staging
// stage) and B = the conv weight read directly in its channels-last
// (K,R,S,C) memory image — no host-side im2col, no weight transform for
// forward.
//
// One kernel template serves forward (FPROP) and data-grad (DGRAD —
// A = scatter-gathered dy with transposed-conv addressing, B = the
// weight permuted to (C,R,S,K) memory once per backward).
//
// Structure = the documented CDNA4 GEMM recipe (cdna_hip_programming.md
// §5): 128x128 block tile, BK=64, 4 waves each owning a 64x64 sub-tile
// of 16x16x32 bf16 MFMA fragments, double-buffered LDS filled by
// 16-byte global_load_lds (lane-linear dest; XOR bank swizzle applied on
// the SOURCE chunk index and re-applied on the ds_read side — rule 21),
// out-of-bounds/padding chunks redirected to a zero page so every lane
// always issues its DMA.
//
// Constraints (dispatcher falls back for the rest): bf16, groups=1,
// dilation=1, C %8 == 0 (FPROP) / K %8 == 0 (DGRAD) so no 16-B chunk
// crosses an (r,s) boundary.

#include "conv_igemm.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <stdlib.h>
#include <string>

using bf16 = conv_bf16;

#define BM 128
#define BN 128
#define BK 64
#define THREADS 256

// ---- chunk -> global address generators -------------------------------
// A-chunk: logical (row=m in [0,BM), cg in [0,8)) of the current K-step.
// Returns the 16-byte-aligned source for elements kk0+cg*8 .. +7.

// MODE: 0 = FPROP, 1 = DGRAD (any stride, gather with validity tests),
//       2 = DGRAD stride-2 parity class (all taps valid by construction)
//
// The A operand's row -> pixel decomposition is loop-invariant (the
// GEMM row never changes across K-steps), so it is computed once per
// staging slot (conv_a_row_coords) and only the (r, s, c/k) part runs
// per step (a_step_addr).
template <int MODE>
DEV const bf16* a_step_addr(const ConvParams& p, const ConvRowCoords& rc,
                            long kkg) {
  if (!rc.valid) return p.zero;
  if (MODE == 0) {
    const int c0 = (int)(kkg % p.Cin);
    const int rs = (int)(kkg / p.Cin);
    const int r = rs / p.S, s = rs - (rs / p.S) * p.S;
    const int ih = rc.y * p.stride + r - p.pad;
    const int iw = rc.x * p.stride + s - p.pad;
    if (ih < 0 || ih >= p.H || iw < 0 || iw >= p.W) return p.zero;
    return p.a + (((long)rc.n * p.H + ih) * p.W + iw) * p.Cin + c0;
  } else if (MODE == 1) {
    const int k0 = (int)(kkg % p.K);
    const int rs = (int)(kkg / p.K);
    const int r = rs / p.S, s = rs - (rs / p.S) * p.S;
    const int tih = rc.y + p.pad - r;
    const int tiw = rc.x + p.pad - s;
    if (tih < 0 || tiw < 0 || (tih % p.stride) || (tiw % p.stride))
      return p.zero;
    const int oh = tih / p.stride, ow = tiw / p.stride;
    if (oh >= p.OH || ow >= p.OW) return p.zero;
    return p.a + (((long)rc.n * p.OH + oh) * p.OW + ow) * p.K + k0;
  } else {
    const int k0 = (int)(kkg % p.K);
    const int rs = (int)(kkg / p.K);
    const int ri = rs / p.ns, si = rs - (rs / p.ns) * p.ns;
    const int r = p.r0 + 2 * ri, s = p.s0 + 2 * si;
    const int oh = (rc.y + p.pad - r) >> 1;
    const int ow = (rc.x + p.pad - s) >> 1;
    if (oh < 0 || ow < 0 || oh >= p.OH || ow >= p.OW) return p.zero;
    return p.a + (((long)rc.n * p.OH + oh) * p.OW + ow) * p.K + k0;
  }
}

template <int MODE>
DEV const bf16* b_chunk_addr(const ConvParams& p, long row, long kkg) {
  if (row >= p.Nd || kkg >= p.Kd) return p.zero;
  if (MODE != 2) return p.b + row * p.Kd + kkg;
  // class subset of the (C,R,S,K) weight image
  const int k0 = (int)(kkg % p.K);
  const int rs = (int)(kkg / p.K);
  const int ri = rs / p.ns, si = rs - (rs / p.ns) * p.ns;
  const int r = p.r0 + 2 * ri, s = p.s0 + 2 * si;
  return p.b + (row * p.R + r) * (long)p.S * p.K + (long)s * p.K + k0;
}

// ---- the kernel -------------------------------------------------------
// LDS: A[2][128][64] + B[2][128][64] bf16 = 64 KiB. Lane-linear glds
// image: slot ca in [0,1024) holds logical (row = ca>>3, cg' = ca&7)
// where the DATA stored is logical cg = cg' ^ (row & 7). ds_read applies
// the same XOR.

// Tile geometry is templated so small output-channel counts get a
// narrow N tile instead of half-empty MFMA work: 4 waves arranged
// (WR x WC) each owning a (BM_/WR x BN_/WC) sub-tile.
// ADD: dgrad epilogue adds p.add (same rounding order as the deep-pipeline
// kernel: round the accumulator to bf16, then one bf16 add).
// GATE (with ADD): the addend is p.add gated by the 1-bit mask p.gate.
template <int MODE, int BM_, int BN_, int WR, int WC, bool ADD,
          bool GATE = false>
__global__ __launch_bounds__(THREADS, 2)
void conv_igemm_kernel(ConvParams p) {
  constexpr int WM = BM_ / WR;        // wave tile M
  constexpr int WN = BN_ / WC;        // wave tile N
  constexpr int MF = WM / 16;         // M fragments per wave
  constexpr int NF = WN / 16;         // N fragments per wave
  constexpr int CA = BM_ * BK / 8 / THREADS;  // A chunks per thread
  constexpr int CB = BN_ * BK / 8 / THREADS;  // B chunks per thread
  static_assert(ADD || !GATE, "the gate applies to the addend");
  static_assert(WR * WC == 4, "4 waves");
  static_assert(CA >= 1 && CB >= 1, "tile vs thread count");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* lds = reinterpret_cast<bf16*>(smem);
  auto lds_tile = [&](int buf, int ab) {
    return lds + buf * (BM_ + BN_) * BK + (ab ? BM_ * BK : 0);
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;

  const int nbn = (int)((p.Nd + BN_ - 1) / BN_);
  const int block = xcd_remap(blockIdx.x, gridDim.x);
  const long bm = (long)(block / nbn) * BM_;
  const long bn = (long)(block % nbn) * BN_;

  const int nsteps = (int)((p.Kd + BK - 1) / BK);

  // ---- staging slots: slot ca -> (row = ca>>3, stored cg = ca&7),
  // holding source logical cg = (ca&7) ^ (row&7)
  int a_cg[CA], b_row[CB], b_cg[CB];
  ConvRowCoords a_rc[CA];
#pragma unroll
  for (int l = 0; l < CA; ++l) {
    const int ca = l * THREADS + tid;
    const int arow = ca >> 3;
    a_cg[l] = (ca & 7) ^ (arow & 7);
    a_rc[l] = conv_a_row_coords<MODE>(p, bm + arow);
  }
#pragma unroll
  for (int l = 0; l < CB; ++l) {
    const int ca = l * THREADS + tid;
    b_row[l] = ca >> 3;
    b_cg[l] = (ca & 7) ^ (b_row[l] & 7);
  }

  auto stage = [&](int buf, int step) {
    const long kk0 = (long)step * BK;
    bf16* la = lds_tile(buf, 0);
    bf16* lb = lds_tile(buf, 1);
#pragma unroll
    for (int l = 0; l < CA; ++l) {
      const long kkga = kk0 + a_cg[l] * 8;
      const bf16* src = a_step_addr<MODE>(p, a_rc[l],
                                          kkga < p.Kd ? kkga : 0);
      if (kkga >= p.Kd) src = p.zero;
      glds16(src, la + (l * THREADS + tid) * 8);
    }
#pragma unroll
    for (int l = 0; l < CB; ++l) {
      const bf16* src = b_chunk_addr<MODE>(p, bn + b_row[l],
                                           kk0 + b_cg[l] * 8);
      glds16(src, lb + (l * THREADS + tid) * 8);
    }
  };

  // ---- fragment read offsets (XOR re-applied) -----------------------
  const int fr = lane & 15;         // row-in-frag
  const int fk = lane >> 4;         // k-subgroup
  const int wm = (wid / WC) * WM;   // wave M offset
  const int wn = (wid % WC) * WN;   // wave N offset

  auto frag_ptr = [&](bf16* tile, int row, int ks) -> const bf16x8* {
    const int cg = (ks * 4 + fk) ^ (row & 7);
    return reinterpret_cast<const bf16x8*>(tile + row * BK + cg * 8);
  };

  f32x4 acc[MF][NF];
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j)
      acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  wait_vmcnt<0>();
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < nsteps; ++t) {
    if (t + 1 < nsteps) stage(cur ^ 1, t + 1);
    bf16* la = lds_tile(cur, 0);
    bf16* lb = lds_tile(cur, 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[MF], bfr[NF];
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
        af[mf] = *frag_ptr(la, wm + mf * 16 + fr, ks);
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        bfr[nf] = *frag_ptr(lb, wn + nf * 16 + fr, ks);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mf], bfr[nf], acc[mf][nf], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    wait_vmcnt<0>();
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: D[row=(lane>>4)*4+reg][col=lane&15] per fragment ---
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const long row = bm + wm + mf * 16 + fk * 4 + reg;
      if (row >= p.M) continue;
      // class row -> scattered dx pixel
      const long out_row = (MODE == 2) ? conv_class_dx_row(p, row) : row;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        const long col = bn + wn + nf * 16 + fr;
        if (col < p.Nd) {
          const long o = out_row * p.Nd + col;
          bf16 v = from_f32<bf16>(acc[mf][nf][reg]);
          if (GATE)
            v = from_f32<bf16>(
                to_f32(v) +
                to_f32(p.add[o]) * (float)((p.gate[o >> 3] >> (o & 7)) & 1));
          else if (ADD)
            v = from_f32<bf16>(to_f32(v) + to_f32(p.add[o]));
          p.out[o] = v;
        }
      }
    }
  }
}

// ---- launchers --------------------------------------------------------
namespace {

// fills one plan entry from the prepared params: the deep-pipeline
// structure (conv_mfma2.hip) first, else the 128-tile structure with a
// narrow N tile for small output-channel counts
void plan_entry(const ConvParams& p, int mode, bool use_v2,
                ddlb::ConvIgemmLaunch& e) {
  e.mode = mode;
  e.M = p.M; e.Nd = p.Nd; e.Kd = p.Kd;
  e.cls_a = e.cls_b = e.r0 = e.s0 = e.nr = e.ns = e.nh = e.nw = 0;
  if (mode == 2) {
    e.cls_a = p.cls_a; e.cls_b = p.cls_b; e.r0 = p.r0; e.s0 = p.s0;
    e.nr = p.nr; e.ns = p.ns; e.nh = p.nh; e.nw = p.nw;
  }
  bool lin = false;
  e.v2 = use_v2 && conv_igemm_v2_select(p, mode, e.bm, e.bn, lin);
  e.lin = lin;
  if (e.v2) return;
  if (p.Nd <= 64 && p.M >= 256) { e.bm = 256; e.bn = 64; }
  else if (p.Nd <= 64) { e.bm = 128; e.bn = 64; }
  else { e.bm = 128; e.bn = 128; }
}

// the dims every pass shares; M/Nd/Kd are those of the whole pass
// (stride-2 dgrad overrides M and Kd per parity class)
void fill_dims(ConvParams& p, int N, int H, int W, int Cin, int K, int OH,
               int OW, int R, int S, int stride, int pad, int dgrad) {
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.K = K; p.OH = OH; p.OW = OW;
  p.R = R; p.S = S; p.stride = stride; p.pad = pad;
  if (!dgrad) {
    p.M = (long)N * OH * OW;
    p.Nd = K;
    p.Kd = (long)R * S * Cin;
  } else {
    p.M = (long)N * H * W;
    p.Nd = Cin;
    p.Kd = (long)R * S * K;
  }
}

}  // namespace

ddlb::ConvIgemmPlan ddlb::conv_igemm_plan(int N, int H, int W, int Cin,
                                          int K, int OH, int OW, int R,
                                          int S, int stride, int pad,
                                          int dgrad) {
  ConvParams p{};
  fill_dims(p, N, H, W, Cin, K, OH, OW, R, S, stride, pad, dgrad);
  // deep-pipeline structure (conv_mfma2.hip) first; DDLB_CONV_V2=0
  // forces the 128-tile structure (re-read per call so benchmarks can
  // A/B the two structures in one process)
  const char* v2e = getenv("DDLB_CONV_V2");
  const bool use_v2 = !(v2e && v2e[0] == '0');

  ConvIgemmPlan plan;
  plan.n = 0;
  if (!dgrad) {
    plan_entry(p, 0, use_v2, plan.e[plan.n++]);
  } else if (stride == 2 && K % 8 == 0) {
    // four parity classes, each a dense reduction over its valid taps
    for (int a_ = 0; a_ < 2; ++a_) {
      for (int b_ = 0; b_ < 2; ++b_) {
        p.cls_a = a_;
        p.cls_b = b_;
        // r valid iff (ih + pad - r) even  ->  r ≡ (a_ + pad) (mod 2)
        p.r0 = (a_ + pad) & 1;
        p.s0 = (b_ + pad) & 1;
        p.nr = (R - p.r0 + 1) / 2;
        p.ns = (S - p.s0 + 1) / 2;
        p.nh = (H - a_ + 1) / 2;
        p.nw = (W - b_ + 1) / 2;
        if (p.nr <= 0 || p.ns <= 0 || p.nh <= 0 || p.nw <= 0) continue;
        p.M = (long)N * p.nh * p.nw;
        p.Kd = (long)p.nr * p.ns * K;
        plan_entry(p, 2, use_v2, plan.e[plan.n++]);
      }
    }
  } else {
    plan_entry(p, 1, use_v2, plan.e[plan.n++]);
  }
  return plan;
}

void ddlb::launch_conv_igemm(const void* a, const void* b, void* out,
                             const void* zero, int N, int H, int W, int Cin,
                             int K, int OH, int OW, int R, int S, int stride,
                             int pad, int dgrad, const void* add,
                             const void* gate, hipStream_t stream) {
  // the addend needs every dx element written exactly once: FPROP has
  // no addend, and stride-2 classes with R==1 or S==1 leave pixels to
  // the caller's zero fill (the binding adds after the launch there)
  if (add && (!dgrad || (stride == 2 && K % 8 == 0 && (R == 1 || S == 1))))
    throw std::invalid_argument(
        "launch_conv_igemm: addend unsupported for this pass");
  if (gate && (!add || Cin % 8 != 0))
    throw std::invalid_argument(
        "launch_conv_igemm: the gate needs an addend and C % 8 == 0");
  ConvParams p;
  p.a = (const bf16*)a;
  p.b = (const bf16*)b;
  p.out = (bf16*)out;
  p.zero = (const bf16*)zero;
  p.add = (const bf16*)add;
  p.gate = (const unsigned char*)gate;
  fill_dims(p, N, H, W, Cin, K, OH, OW, R, S, stride, pad, dgrad);

#define LAUNCH(MODE, BM_, BN_, WR, WC)                                      \
  do {                                                                      \
    const long nbm = (p.M + (BM_) - 1) / (BM_);                             \
    const long nbn = (p.Nd + (BN_) - 1) / (BN_);                            \
    const size_t lds_bytes = 2 * ((BM_) + (BN_)) * BK * sizeof(bf16);       \
    if ((MODE) != 0 && p.add && p.gate)                                     \
      hipLaunchKernelGGL(                                                   \
          (conv_igemm_kernel<MODE, BM_, BN_, WR, WC, (MODE) != 0,           \
                             (MODE) != 0>),                                 \
          dim3((unsigned)(nbm * nbn)), dim3(THREADS), lds_bytes, stream,    \
          p);                                                               \
    else if ((MODE) != 0 && p.add)                                          \
      hipLaunchKernelGGL(                                                   \
          (conv_igemm_kernel<MODE, BM_, BN_, WR, WC, (MODE) != 0>),         \
          dim3((unsigned)(nbm * nbn)), dim3(THREADS), lds_bytes, stream,    \
          p);                                                               \
    else                                                                    \
      hipLaunchKernelGGL(                                                   \
          (conv_igemm_kernel<MODE, BM_, BN_, WR, WC, false>),               \
          dim3((unsigned)(nbm * nbn)), dim3(THREADS), lds_bytes, stream,    \
          p);                                                               \
  } while (0)
#define LAUNCH_TILED(MODE)                                                  \
  do {                                                                      \
    if (e.bm == 256) LAUNCH(MODE, 256, 64, 4, 1);                           \
    else if (e.bn == 64) LAUNCH(MODE, 128, 64, 4, 1);                       \
    else LAUNCH(MODE, 128, 128, 2, 2);                                      \
  } while (0)

  const ConvIgemmPlan plan = conv_igemm_plan(N, H, W, Cin, K, OH, OW, R, S,
                                             stride, pad, dgrad);
  for (int i = 0; i < plan.n; ++i) {
    const ConvIgemmLaunch& e = plan.e[i];
    p.M = e.M;
    p.Kd = e.Kd;
    p.cls_a = e.cls_a; p.cls_b = e.cls_b; p.r0 = e.r0; p.s0 = e.s0;
    p.nr = e.nr; p.ns = e.ns; p.nh = e.nh; p.nw = e.nw;
    if (e.v2) launch_conv_igemm_v2(p, e.mode, e.bm, e.lin != 0, stream);
    else if (e.mode == 0) LAUNCH_TILED(0);
    else if (e.mode == 1) LAUNCH_TILED(1);
    else LAUNCH_TILED(2);
  }
#undef LAUNCH_TILED
#undef LAUNCH
  HIP_CHECK_LAST();
}

// ---- gated addend, materialised ---------------------------------------
// out = bf16(float(add) * g) over n8 8-element chunks, g the chunk's mask
// byte: the fallback for dgrad passes with no in-kernel add (the sparse
// stride-2 case, where the binding adds after the launch).
namespace {
typedef __attribute__((ext_vector_type(8))) unsigned short gate_u16x8;

__global__ void gate_addend_kernel(const bf16* __restrict__ add,
                                   const unsigned char* __restrict__ gate,
                                   bf16* __restrict__ out, long n8) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += stride) {
    gate_u16x8 v = reinterpret_cast<const gate_u16x8*>(add)[i];
    const unsigned g = gate[i];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      // the product is v, a signed zero or a NaN: its low 16 bits are 0
      v[j] = (unsigned short)(__float_as_uint(
                                  __uint_as_float((unsigned)v[j] << 16) *
                                  (float)((g >> j) & 1u)) >> 16);
    reinterpret_cast<gate_u16x8*>(out)[i] = v;
  }
}
}  // namespace

void ddlb::launch_gate_addend(const void* add, const void* gate, void* out,
                              long n8, hipStream_t stream) {
  if (n8 <= 0) return;
  const long want = (n8 + THREADS - 1) / THREADS;
  const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
  hipLaunchKernelGGL(gate_addend_kernel, dim3(blocks), dim3(THREADS), 0,
                     stream, (const bf16*)add, (const unsigned char*)gate,
                     (bf16*)out, n8);
  HIP_CHECK_LAST();
}
