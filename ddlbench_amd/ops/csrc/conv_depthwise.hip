// NHWC bf16 depthwise convolution (groups == C in == C out) for gfx950:
// forward, data-grad and weight-grad for square K in {3, 5, 7}, pad K/2,
// stride 1 or 2, C % 4 == 0 (NASNet's 5x5 / 7x7 separable convs).
//
// K*K taps per output make the op FMA- and LDS-bound as well as
// byte-bound, so every direction stages its operands in LDS once per tile
// and each thread reuses what it reads from LDS across several outputs
// (forward, data-grad) or several taps (weight-grad). There is no matrix
// instruction here: a channel's row convolution as a banded Toeplitz GEMM
// would use at most K/32 of an MFMA and needs a channel-major LDS image.
//
// Common to all kernels. A block owns a chunk of 32 channels (one 64-byte
// segment per pixel) and walks spatial tiles grid-stride with that chunk
// fixed. V channels (8: 16-byte accesses, C % 8 == 0; else 4: 8-byte) form
// a thread's channel vector; adjacent lanes hold adjacent channel vectors
// of one pixel, then adjacent pixels. Tiles are staged as bf16
// [row][col][32 ch + 8] with zeros outside the image and past C: the
// compute loops carry no border tests. The 80-byte pixel pitch keeps every
// vector 16-byte aligned and spreads the lanes' pixels over the banks.
//
// forward / stride-1 data-grad (dwk_fwd_kernel):
//   tile = TH x 16 outputs (TH = 8, 4 at stride 2), halo
//   ((TH-1)S+K) x (15S+K) pixels. The chunk's weights sit in LDS as fp32
//   [K*K][32], read straight from the (C,1,K,K) weight, tap-reversed for
//   the data-grad of a stride-1 conv (the same conv run on dy). A thread
//   owns one channel vector and 4 consecutive outputs of one row: per kh it
//   takes that weight row (K*V floats) into registers and walks the 3S+K
//   input columns once, feeding each loaded vector to every accumulator it
//   contributes to: K(3S+K)/4 LDS reads per output instead of K*K.
//
// stride-2 data-grad (dwk_dgrad2_kernel):
//   dx splits into its four (ih%2, iw%2) parity classes; in the plane
//   coordinates (ih/2, iw/2) each class is a stride-1 correlation of dy
//   with the taps of matching parity, ceil(K/2) or floor(K/2) per axis,
//   all chosen at compile time. A block stages the dy halo of an 8 x 16
//   plane tile (16 x 32 dx pixels); a thread owns 2 plane columns of a
//   plane row, i.e. 2 x 4 dx pixels, and does the two row classes in turn,
//   the two column classes together from one walk over the dy row. dx is
//   written completely, pixels no tap reaches as zeros.
//
// weight-grad (dwk_wgrad_kernel + dwk_combine_kernel):
//   a block stages a dy tile and the matching x halo. A thread owns one
//   channel vector and one kernel row kh (K*V fp32 accumulators, kept over
//   all of the block's tiles) and sweeps output pixels along rows; the x
//   values form a K-wide register window that shifts by S per output, so a
//   step costs S x reads, one dy read and K*V FMAs. The threads that split
//   the tile's rows add their partials through LDS in row order; the block
//   writes one fp32 slab [C chunk][K*K]. The combine adds the slabs of an
//   element in a fixed order (8 interleaved groups ascending, then the 8
//   group sums ascending) and rounds once to bf16. No memset, no atomics,
//   no fp64: the same inputs give the same bits.

#include "common.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <string>
#include <type_traits>

// The compiler keeps to plain v_fma_f32 in this file: the packed fp32 forms
// (v_pk_fma_f32 and kin) are switched off for every device function here.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int DW_CC = 32;            // channels per block
constexpr int DW_PITCH = DW_CC + 8;  // halves per LDS pixel
constexpr int DW_TW = 16;            // tile width
constexpr int DW_R = 4;              // fwd: outputs per thread along a row
constexpr int DW_MAX_BLOCKS = 1024;  // blocks per launch, every direction
constexpr int DW_U = 4;              // staging loads in flight per thread

struct DwParams {
  const unsigned short* in;  // staged halo tensor: x (fwd, wgrad), dy (dgrad)
  const unsigned short* w;   // (C,1,K,K) = [C][K*K]
  unsigned short* out;       // y (fwd) or dx (dgrad)
  const unsigned short* dy;  // wgrad
  float* part;               // wgrad slabs [slot][C][K*K]
  int N, C;
  int IH, IW;                // size of `in`
  int OH, OW;                // size of the tiled tensor: out, or wgrad's dy
  int tiles_h, tiles_w, nct, slots;
  long nsp;                  // spatial tiles = N*tiles_h*tiles_w
};

// V bf16 channels, loaded and stored as one 8- or 16-byte access
template <int V> struct BfVec;
template <> struct BfVec<8> {
  uint4 d;
  DEV unsigned get(int i) const {
    return i == 0 ? d.x : i == 1 ? d.y : i == 2 ? d.z : d.w;
  }
  DEV void set(int i, unsigned v) {
    if (i == 0) d.x = v; else if (i == 1) d.y = v;
    else if (i == 2) d.z = v; else d.w = v;
  }
};
template <> struct BfVec<4> {
  uint2 d;
  DEV unsigned get(int i) const { return i == 0 ? d.x : d.y; }
  DEV void set(int i, unsigned v) { if (i == 0) d.x = v; else d.y = v; }
};

DEV float bf2f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

DEV unsigned f2bf(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

template <int V> DEV void unpack(const BfVec<V>& b, float (&f)[V]) {
#pragma unroll
  for (int i = 0; i < V / 2; ++i) {
    f[2 * i] = __uint_as_float(b.get(i) << 16);
    f[2 * i + 1] = __uint_as_float(b.get(i) & 0xffff0000u);
  }
}

template <int V> DEV BfVec<V> pack(const float (&f)[V]) {
  BfVec<V> b;
#pragma unroll
  for (int i = 0; i < V / 2; ++i)
    b.set(i, f2bf(f[2 * i]) | (f2bf(f[2 * i + 1]) << 16));
  return b;
}

template <int V> DEV BfVec<V> lds_vec(const unsigned short* p) {
  return *reinterpret_cast<const BfVec<V>*>(p);
}

// PH x PW pixels of image n of `in` (IH x IW x C) from (vh0, vw0), channels
// cb .. cb+31, into lds[pixel][DW_PITCH]; zeros outside the image and
// past C. All NT threads of the block call it.
template <int V, int PH, int PW, int NT>
DEV void stage_patch(unsigned short* lds, const unsigned short* in, int n,
                     int IH, int IW, int C, int vh0, int vw0, int cb,
                     int tid) {
  constexpr int NV = DW_CC / V;
  constexpr int NLOAD = PH * PW * NV;
  for (int b0 = 0; b0 < NLOAD; b0 += DW_U * NT) {
    BfVec<V> v[DW_U];
#pragma unroll
    for (int u = 0; u < DW_U; ++u) {
      const int idx = b0 + u * NT + tid;
      const int pix = idx / NV, cv = idx - pix * NV;
      const int ph = pix / PW, pw = pix - ph * PW;
      const int ih = vh0 + ph, iw = vw0 + pw, c = cb + cv * V;
      v[u] = BfVec<V>{};
      if (idx < NLOAD && ih >= 0 && ih < IH && iw >= 0 && iw < IW && c < C)
        v[u] = *reinterpret_cast<const BfVec<V>*>(
            in + (((long)n * IH + ih) * IW + iw) * C + c);
    }
#pragma unroll
    for (int u = 0; u < DW_U; ++u) {
      const int idx = b0 + u * NT + tid;
      const int pix = idx / NV, cv = idx - pix * NV;
      if (idx < NLOAD)
        *reinterpret_cast<BfVec<V>*>(lds + pix * DW_PITCH + cv * V) = v[u];
    }
  }
}

// the chunk's weights as fp32 wl[tap][32], tap-reversed when FLIP; zeros
// past C
template <int K, bool FLIP, int NT>
DEV void stage_weights(float* wl, const unsigned short* w, int C, int cb,
                       int tid) {
  constexpr int KK = K * K;
  for (int i = tid; i < KK * DW_CC; i += NT) {
    const int cl = i / KK, t = i - cl * KK;
    const int c = cb + cl;
    wl[(FLIP ? KK - 1 - t : t) * DW_CC + cl] =
        c < C ? bf2f(w[(long)c * KK + t]) : 0.f;
  }
}

// weight row kh of this thread's channel vector, LDS -> registers
template <int K, int V>
DEV void load_wrow(const float* wl, int kh, int cv, float (&wr)[K][V]) {
#pragma unroll
  for (int kw = 0; kw < K; ++kw)
#pragma unroll
    for (int e = 0; e < V; e += 4) {
      const float4 f = *reinterpret_cast<const float4*>(
          wl + (kh * K + kw) * DW_CC + cv * V + e);
      wr[kw][e] = f.x; wr[kw][e + 1] = f.y;
      wr[kw][e + 2] = f.z; wr[kw][e + 3] = f.w;
    }
}

struct TileCoord {
  int n, h0, w0;
};

DEV TileCoord tile_coord(const DwParams& q, long sp, int th, int tw) {
  TileCoord t;
  const int twb = (int)(sp % q.tiles_w);
  const long r = sp / q.tiles_w;
  t.n = (int)(r / q.tiles_h);
  t.h0 = (int)(r - (long)t.n * q.tiles_h) * th;
  t.w0 = twb * tw;
  return t;
}

// ---------------------------------------------------------------------
// forward (FLIP = false) and the data-grad of a stride-1 conv (FLIP = true,
// S = 1, q.in = dy)
template <int S> struct FwdGeom {
  static constexpr int TH = S == 1 ? 8 : 4;
};

template <int K, int S, int V, bool FLIP>
__global__ __launch_bounds__((DW_CC / V) * (DW_TW / DW_R) * FwdGeom<S>::TH)
void dwk_fwd_kernel(DwParams q) {
  constexpr int TH = FwdGeom<S>::TH;
  constexpr int PH = (TH - 1) * S + K, PW = (DW_TW - 1) * S + K;
  constexpr int NV = DW_CC / V, RUNS = DW_TW / DW_R;
  constexpr int NT = NV * RUNS * TH;
  constexpr int NJ = (DW_R - 1) * S + K;  // input columns of a run
  __shared__ __attribute__((aligned(16)))
      unsigned short patch[PH * PW * DW_PITCH];
  __shared__ __attribute__((aligned(16))) float wl[K * K * DW_CC];

  const int tid = threadIdx.x;
  const int cv = tid % NV, run = (tid / NV) % RUNS, row = tid / (NV * RUNS);
  const int ct = blockIdx.x % q.nct, slot = blockIdx.x / q.nct;
  const int cb = ct * DW_CC;
  const bool active = cb + cv * V < q.C;

  stage_weights<K, FLIP, NT>(wl, q.w, q.C, cb, tid);

  for (long sp = slot; sp < q.nsp; sp += q.slots) {
    const TileCoord tc = tile_coord(q, sp, TH, DW_TW);
    __syncthreads();  // the previous tile's reads are done
    stage_patch<V, PH, PW, NT>(patch, q.in, tc.n, q.IH, q.IW, q.C,
                               tc.h0 * S - K / 2, tc.w0 * S - K / 2, cb, tid);
    __syncthreads();
    if (!active) continue;

    float acc[DW_R][V];
#pragma unroll
    for (int r = 0; r < DW_R; ++r)
#pragma unroll
      for (int e = 0; e < V; ++e) acc[r][e] = 0.f;
    const unsigned short* p0 =
        patch + (row * S * PW + run * DW_R * S) * DW_PITCH + cv * V;
    // one kernel row at a time: the weight row and the NJ loaded vectors
    // of a row are all that is live besides the accumulators
#pragma unroll 1
    for (int kh = 0; kh < K; ++kh) {
      float wr[K][V];
      load_wrow<K, V>(wl, kh, cv, wr);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float xv[V];
        unpack<V>(lds_vec<V>(p0 + (kh * PW + j) * DW_PITCH), xv);
#pragma unroll
        for (int r = 0; r < DW_R; ++r) {
          const int kw = j - r * S;
          if (kw >= 0 && kw < K) {
#pragma unroll
            for (int e = 0; e < V; ++e)
              acc[r][e] = fmaf(xv[e], wr[kw][e], acc[r][e]);
          }
        }
      }
    }
    const int oh = tc.h0 + row;
#pragma unroll
    for (int r = 0; r < DW_R; ++r) {
      const int ow = tc.w0 + run * DW_R + r;
      if (oh < q.OH && ow < q.OW)
        *reinterpret_cast<BfVec<V>*>(
            q.out + (((long)tc.n * q.OH + oh) * q.OW + ow) * q.C + cb +
            cv * V) = pack<V>(acc[r]);
    }
  }
}

// ---------------------------------------------------------------------
// data-grad of a stride-2 conv. dx pixel ih = 2a + ph takes the taps
// kh = k0 + 2m (k0 = (ph + pad) % 2, m < nk) from dy row a + d - m.
template <int K> struct S2Geom {
  static constexpr int P = K / 2;
  static constexpr int k0(int ph) { return (ph + P) & 1; }
  static constexpr int d(int ph) { return (ph + P - k0(ph)) / 2; }
  static constexpr int nk(int ph) { return (K - k0(ph) + 1) / 2; }
  static constexpr int lo(int ph) { return d(ph) - nk(ph) + 1; }
  static constexpr int LO = lo(0) < lo(1) ? lo(0) : lo(1);
  static constexpr int HI = d(0) > d(1) ? d(0) : d(1);
};

constexpr int D2_TH = 8, D2_TW = 16;  // plane tile: 16 x 32 dx pixels
constexpr int D2_NT = 256;

template <int K, int V>
__global__ __launch_bounds__(D2_NT)
void dwk_dgrad2_kernel(DwParams q) {
  using G = S2Geom<K>;
  constexpr int LO = G::LO, HI = G::HI;
  constexpr int PH = D2_TH + HI - LO, PW = D2_TW + HI - LO;
  constexpr int NV = DW_CC / V, RUNS = D2_TW / 2;
  constexpr int TROWS = D2_NT / (NV * RUNS), RPT = D2_TH / TROWS;
  static_assert(TROWS * RPT == D2_TH, "rows split evenly");
  __shared__ __attribute__((aligned(16)))
      unsigned short patch[PH * PW * DW_PITCH];
  __shared__ __attribute__((aligned(16))) float wl[K * K * DW_CC];

  const int tid = threadIdx.x;
  const int cv = tid % NV, run = (tid / NV) % RUNS, tr = tid / (NV * RUNS);
  const int ct = blockIdx.x % q.nct, slot = blockIdx.x / q.nct;
  const int cb = ct * DW_CC;
  const bool active = cb + cv * V < q.C;

  stage_weights<K, false, D2_NT>(wl, q.w, q.C, cb, tid);

  for (long sp = slot; sp < q.nsp; sp += q.slots) {
    const TileCoord tc = tile_coord(q, sp, D2_TH, D2_TW);
    __syncthreads();
    stage_patch<V, PH, PW, D2_NT>(patch, q.in, tc.n, q.IH, q.IW, q.C,
                                  tc.h0 + LO, tc.w0 + LO, cb, tid);
    __syncthreads();
    if (!active) continue;

#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int al = tr + TROWS * i;
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        float acc[2][2][V];  // [pw][plane column]
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int e = 0; e < V; ++e) acc[a >> 1][a & 1][e] = 0.f;
#pragma unroll 1
        for (int m = 0; m < G::nk(ph); ++m) {
          float wr[K][V];
          load_wrow<K, V>(wl, G::k0(ph) + 2 * m, cv, wr);
          const unsigned short* p0 =
              patch + ((al + G::d(ph) - m - LO) * PW + run * 2) * DW_PITCH +
              cv * V;
#pragma unroll
          for (int c = LO; c <= 1 + HI; ++c) {
            float gv[V];
            unpack<V>(lds_vec<V>(p0 + (c - LO) * DW_PITCH), gv);
#pragma unroll
            for (int pw = 0; pw < 2; ++pw)
#pragma unroll
              for (int r = 0; r < 2; ++r) {
                const int nn = r + G::d(pw) - c;
                if (nn >= 0 && nn < G::nk(pw)) {
                  const int kw = G::k0(pw) + 2 * nn;
#pragma unroll
                  for (int e = 0; e < V; ++e)
                    acc[pw][r][e] = fmaf(gv[e], wr[kw][e], acc[pw][r][e]);
                }
              }
          }
        }
        const int ih = 2 * (tc.h0 + al) + ph;
#pragma unroll
        for (int pw = 0; pw < 2; ++pw)
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const int iw = 2 * (tc.w0 + run * 2 + r) + pw;
            if (ih < q.OH && iw < q.OW)
              *reinterpret_cast<BfVec<V>*>(
                  q.out + (((long)tc.n * q.OH + ih) * q.OW + iw) * q.C + cb +
                  cv * V) = pack<V>(acc[pw][r]);
          }
      }
    }
  }
}

// ---------------------------------------------------------------------
// weight-grad. q.in = x (N,IH,IW,C), q.dy = dy (N,OH,OW,C).
template <int S, int V> struct WgGeom {
  static constexpr int TH = S == 1 ? 8 : 4;
  static constexpr int NV = DW_CC / V;
  static constexpr int TROWS = TH < 32 / NV ? TH : 32 / NV;
  static constexpr int RPT = TH / TROWS;
};

template <int K, int S, int V>
__global__ __launch_bounds__(((DW_CC / V) * K * WgGeom<S, V>::TROWS))
void dwk_wgrad_kernel(DwParams q) {
  using G = WgGeom<S, V>;
  constexpr int TH = G::TH, NV = G::NV, TROWS = G::TROWS, RPT = G::RPT;
  constexpr int PH = (TH - 1) * S + K, PW = (DW_TW - 1) * S + K;
  constexpr int NT = NV * K * TROWS;
  constexpr int KK = K * K;
  static_assert(TROWS * RPT == TH, "rows split evenly");
  __shared__ __attribute__((aligned(16)))
      unsigned short xs[PH * PW * DW_PITCH];
  __shared__ __attribute__((aligned(16)))
      unsigned short dys[TH * DW_TW * DW_PITCH];
  __shared__ float red[DW_CC * KK];

  const int tid = threadIdx.x;
  const int cv = tid % NV, kh = (tid / NV) % K, tr = tid / (NV * K);
  const int ct = blockIdx.x % q.nct, slot = blockIdx.x / q.nct;
  const int cb = ct * DW_CC;
  const bool active = cb + cv * V < q.C;

  float acc[K][V];
#pragma unroll
  for (int kw = 0; kw < K; ++kw)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[kw][e] = 0.f;

  for (long sp = slot; sp < q.nsp; sp += q.slots) {
    const TileCoord tc = tile_coord(q, sp, TH, DW_TW);
    __syncthreads();
    stage_patch<V, PH, PW, NT>(xs, q.in, tc.n, q.IH, q.IW, q.C,
                               tc.h0 * S - K / 2, tc.w0 * S - K / 2, cb, tid);
    stage_patch<V, TH, DW_TW, NT>(dys, q.dy, tc.n, q.OH, q.OW, q.C, tc.h0,
                                  tc.w0, cb, tid);
    __syncthreads();
    if (!active) continue;

#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int ol = tr + TROWS * i;
      const unsigned short* xr = xs + (ol * S + kh) * PW * DW_PITCH + cv * V;
      const unsigned short* dr = dys + ol * DW_TW * DW_PITCH + cv * V;
      // win[kw] = x column ow*S + kw of this row; shifts by S per output
      float win[K][V];
#pragma unroll
      for (int j = 0; j < K - S; ++j)
        unpack<V>(lds_vec<V>(xr + j * DW_PITCH), win[j + S]);
#pragma unroll
      for (int ow = 0; ow < DW_TW; ++ow) {
#pragma unroll
        for (int j = 0; j < K - S; ++j)
#pragma unroll
          for (int e = 0; e < V; ++e) win[j][e] = win[j + S][e];
#pragma unroll
        for (int s = 0; s < S; ++s)
          unpack<V>(lds_vec<V>(xr + (ow * S + K - S + s) * DW_PITCH),
                    win[K - S + s]);
        float g[V];
        unpack<V>(lds_vec<V>(dr + ow * DW_PITCH), g);
#pragma unroll
        for (int kw = 0; kw < K; ++kw)
#pragma unroll
          for (int e = 0; e < V; ++e)
            acc[kw][e] = fmaf(g[e], win[kw][e], acc[kw][e]);
      }
    }
  }

  // the row threads of one (channel vector, kh) add up in row order
  for (int r = 1; r < TROWS; ++r) {
    __syncthreads();
    if (active && tr == r) {
#pragma unroll
      for (int kw = 0; kw < K; ++kw)
#pragma unroll
        for (int e = 0; e < V; ++e)
          red[(cv * V + e) * KK + kh * K + kw] = acc[kw][e];
    }
    __syncthreads();
    if (active && tr == 0) {
#pragma unroll
      for (int kw = 0; kw < K; ++kw)
#pragma unroll
        for (int e = 0; e < V; ++e)
          acc[kw][e] += red[(cv * V + e) * KK + kh * K + kw];
    }
  }
  if (active && tr == 0) {
    float* out = q.part + ((long)slot * q.C + cb + cv * V) * KK + kh * K;
#pragma unroll
    for (int kw = 0; kw < K; ++kw)
#pragma unroll
      for (int e = 0; e < V; ++e) out[e * KK + kw] = acc[kw][e];
  }
}

// dw[i] (bf16, i over [C][K*K]) = the sum of part[slot][i] in a fixed
// order: 8 slab groups x 32 elements per block, each thread adds its
// group's slabs ascending, then the 8 group sums are added ascending and
// rounded once.
__global__ __launch_bounds__(256)
void dwk_combine_kernel(const float* __restrict__ part,
                        unsigned short* __restrict__ dw, int total,
                        int slots) {
  __shared__ float red[8][32];
  const int e = threadIdx.x & 31;
  const int grp = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + e;
  float s = 0.f;
  if (i < total)
    for (int sl = grp; sl < slots; sl += 8) s += part[(long)sl * total + i];
  red[grp][e] = s;
  __syncthreads();
  if (grp == 0 && i < total) {
    float r = red[0][e];
#pragma unroll
    for (int k = 1; k < 8; ++k) r += red[k][e];
    dw[i] = (unsigned short)f2bf(r);
  }
}

// ---------------------------------------------------------------------
int cdiv(int a, int b) { return (a + b - 1) / b; }

void fill(ddlb::DwkTiling& t, int N, int rows, int cols, int th, int nct) {
  t.th = th;
  t.tw = DW_TW;
  t.tiles_h = cdiv(rows, th);
  t.tiles_w = cdiv(cols, DW_TW);
  t.tiles = (long)N * t.tiles_h * t.tiles_w;
  t.slots = (int)i64max(i64min(t.tiles, DW_MAX_BLOCKS / nct), 1);
}

DwParams params(const ddlb::DwkPlan& pl, const ddlb::DwkTiling& t, int N,
                int C) {
  DwParams q = {};
  q.N = N;
  q.C = C;
  q.tiles_h = t.tiles_h;
  q.tiles_w = t.tiles_w;
  q.nct = pl.nct;
  q.slots = t.slots;
  q.nsp = t.tiles;
  return q;
}

template <int I> using IC = std::integral_constant<int, I>;

// f(IC<K>, IC<S>, IC<V>) for the runtime (K, S, V) of a checked plan
template <typename F> void dwk_switch(int K, int S, int V, F&& f) {
  auto on_v = [&](auto k, auto s) {
    if (V == 8) f(k, s, IC<8>{}); else f(k, s, IC<4>{});
  };
  auto on_s = [&](auto k) {
    if (S == 1) on_v(k, IC<1>{}); else on_v(k, IC<2>{});
  };
  if (K == 3) on_s(IC<3>{});
  else if (K == 5) on_s(IC<5>{});
  else on_s(IC<7>{});
}

}  // namespace

ddlb::DwkPlan ddlb::dwk_plan(int N, int C, int H, int W, int K, int stride) {
  if ((K != 3 && K != 5 && K != 7) || (stride != 1 && stride != 2) ||
      C < 4 || C % 4 || N < 1 || H < 1 || W < 1)
    throw std::runtime_error("conv_depthwise: unsupported problem");
  DwkPlan pl = {};
  pl.V = C % 8 == 0 ? 8 : 4;
  pl.cc = DW_CC;
  pl.nct = cdiv(C, DW_CC);
  pl.OH = (H + 2 * (K / 2) - K) / stride + 1;
  pl.OW = (W + 2 * (K / 2) - K) / stride + 1;
  fill(pl.fwd, N, pl.OH, pl.OW, stride == 1 ? 8 : 4, pl.nct);
  if (stride == 1)
    fill(pl.dgrad, N, H, W, 8, pl.nct);
  else  // tiles of the (ih/2, iw/2) parity planes
    fill(pl.dgrad, N, cdiv(H, 2), cdiv(W, 2), D2_TH, pl.nct);
  fill(pl.wgrad, N, pl.OH, pl.OW, stride == 1 ? 8 : 4, pl.nct);
  pl.part_floats = (long)pl.wgrad.slots * C * K * K;
  return pl;
}

void ddlb::launch_conv_depthwise_fwd(const DwkPlan& pl, const void* x,
                                     const void* w, void* y, int N, int C,
                                     int H, int W, int K, int stride,
                                     hipStream_t stream) {
  DwParams q = params(pl, pl.fwd, N, C);
  q.in = (const unsigned short*)x;
  q.w = (const unsigned short*)w;
  q.out = (unsigned short*)y;
  q.IH = H; q.IW = W; q.OH = pl.OH; q.OW = pl.OW;
  const dim3 grid(q.slots * q.nct);
  dwk_switch(K, stride, pl.V, [&](auto k, auto s, auto v) {
    constexpr int Kc = decltype(k)::value, Sc = decltype(s)::value;
    constexpr int Vc = decltype(v)::value;
    constexpr int NT = (DW_CC / Vc) * (DW_TW / DW_R) * FwdGeom<Sc>::TH;
    hipLaunchKernelGGL((dwk_fwd_kernel<Kc, Sc, Vc, false>), grid, dim3(NT), 0,
                       stream, q);
  });
  HIP_CHECK_LAST();
}

void ddlb::launch_conv_depthwise_dgrad(const DwkPlan& pl, const void* dy,
                                       const void* w, void* dx, int N, int C,
                                       int H, int W, int K, int stride,
                                       hipStream_t stream) {
  DwParams q = params(pl, pl.dgrad, N, C);
  q.in = (const unsigned short*)dy;
  q.w = (const unsigned short*)w;
  q.out = (unsigned short*)dx;
  q.IH = pl.OH; q.IW = pl.OW; q.OH = H; q.OW = W;
  const dim3 grid(q.slots * q.nct);
  dwk_switch(K, stride, pl.V, [&](auto k, auto s, auto v) {
    constexpr int Kc = decltype(k)::value, Sc = decltype(s)::value;
    constexpr int Vc = decltype(v)::value;
    if constexpr (Sc == 1) {
      constexpr int NT = (DW_CC / Vc) * (DW_TW / DW_R) * FwdGeom<1>::TH;
      hipLaunchKernelGGL((dwk_fwd_kernel<Kc, 1, Vc, true>), grid, dim3(NT), 0,
                         stream, q);
    } else {
      hipLaunchKernelGGL((dwk_dgrad2_kernel<Kc, Vc>), grid, dim3(D2_NT), 0,
                         stream, q);
    }
  });
  HIP_CHECK_LAST();
}

void ddlb::launch_conv_depthwise_wgrad(const DwkPlan& pl, const void* x,
                                       const void* dy, void* dw, float* part,
                                       int N, int C, int H, int W, int K,
                                       int stride, hipStream_t stream) {
  DwParams q = params(pl, pl.wgrad, N, C);
  q.in = (const unsigned short*)x;
  q.dy = (const unsigned short*)dy;
  q.part = part;
  q.IH = H; q.IW = W; q.OH = pl.OH; q.OW = pl.OW;
  const dim3 grid(q.slots * q.nct);
  dwk_switch(K, stride, pl.V, [&](auto k, auto s, auto v) {
    constexpr int Kc = decltype(k)::value, Sc = decltype(s)::value;
    constexpr int Vc = decltype(v)::value;
    constexpr int NT = (DW_CC / Vc) * Kc * WgGeom<Sc, Vc>::TROWS;
    hipLaunchKernelGGL((dwk_wgrad_kernel<Kc, Sc, Vc>), grid, dim3(NT), 0,
                       stream, q);
  });
  HIP_CHECK_LAST();
  const int total = C * K * K;
  hipLaunchKernelGGL(dwk_combine_kernel, dim3(cdiv(total, 32)), dim3(256), 0,
                     stream, part, (unsigned short*)dw, total, q.slots);
  HIP_CHECK_LAST();
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
