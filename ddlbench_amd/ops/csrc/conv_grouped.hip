// NHWC bf16 grouped 3x3 convolution on MFMA (gfx950): forward, data-grad
// and weight-grad for groups > 1 with Cg = C/groups in {4, 8, 16, 32} and
// as many output as input channels (ResNeXt's conv2).
//
// These layers are bandwidth-bound (9*Cg MACs per output element), so the
// design reads each activation tensor once with 16-byte accesses and
// spends MFMA lanes freely.
//
// Slab formulation. 16 consecutive channels hold 16/Cg whole groups
// (Cg <= 16); restricted to them the conv is a dense 16->16 conv whose
// (tap, 16, 16) weight is block-diagonal. One wave owns one slab. The MFMA
// k index runs over (tap, channel in slab): one 16x16x32 instruction covers
// taps (2t, 2t+1) x 16 channels, 9 taps take 5 MFMAs, the 10th tap's weight
// and activation fragments are zero. Cg = 32: the slab's 16 output channels
// reduce over their group's 32 channels, one MFMA per tap, nothing padded.
// The weight fragments (MFMA A operand: rows = output channels) are
// gathered once per block straight from the (K,3,3,Cg) weight and live in
// registers; data-grad gathers them tap-flipped and in/out-transposed
// within the group, so there is no layout kernel.
//
// fwd / dgrad (one kernel, gconv_kernel):
//   * A block loops over tiles of TH x 16 output pixels (grid-stride) with
//     its 64-channel span fixed: every pixel is a 128-byte global access.
//   * The tile's input patch, halo included, goes to LDS once per tile as
//     [row][col][64 ch + 8], zero-filled outside the image: fragments have
//     no border logic. A lane's activation fragment is one 16-byte LDS
//     read at (pixel + tap, slab*16 + 8*(j%2)). The 144-byte pixel pitch
//     keeps the 16 pixels of a fragment row on distinct 16-byte bank
//     groups; at stride 2 the patch columns are stored de-interleaved by
//     parity so that the pixels two apart are neighbours again.
//   * dgrad is the stride-1 loop over dy with pad 2-pad and flipped taps;
//     for a stride-2 conv dy is written into the patch dilated (zeros
//     between samples). Rows or columns of dx no tap reaches come out as
//     zeros like any other border.
//   * Epilogue: each lane holds 4 consecutive channels of one pixel; 8-byte
//     LDS writes into a [pixel][64 ch + 8] tile, then 16 B/lane stores.
//
// wgrad (gconv_wgrad_kernel + gconv_combine_kernel):
//   dw[tap][k][c] = sum_p dy[p][k] * x[p*stride + tap][c] per slab: pixels
//   are the MFMA k index, so both operands are transposed while staging
//   ([channel][pixel] in LDS, 2-byte writes, rows skewed by 16 B per 8
//   channels so the 8 channel octets of a wave write distinct banks).
//   dy fragments are aligned 16-byte reads. The x fragment of tap (r, s)
//   is the 8-pixel window starting s pixels into an aligned 16-pixel read,
//   cut out with funnel shifts: one pair of reads serves the three s taps
//   of a row (stride 2: even/odd columns are stored apart, s = 0, 1 are
//   aligned and s = 2 is the even window shifted by one). Accumulators: 9
//   taps x f32x4 (x2 for Cg = 32) per wave, kept over the block's tiles.
//   Every block writes one fp32 partial slab; the combine sums them in a
//   fixed order, picks the diagonal blocks and writes bf16 dw in the
//   weight's (K,3,3,Cg) memory. No atomics: the same bits every call.
//
// Limits (checked in bindings.hip): C == K, C % 16 == 0 (32 for Cg = 32),
// 3x3, stride 1 or 2, pad 0 or 1.

#include "mfma_common.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <string>

namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_TW = 16;          // tile width: one MFMA pixel block
constexpr int GC_CT = 64;          // channels per block, one slab per wave
constexpr int GC_PITCH = GC_CT + 8;  // halves per LDS pixel (fwd/dgrad)
constexpr int GC_MAX_BLOCKS = 1536;  // persistent blocks of fwd/dgrad
constexpr int GW_MAX_BLOCKS = 512;   // wgrad blocks = partial slabs * nct

struct GcParams {
  const unsigned short* in;   // staged tensor: x (fwd) or dy (dgrad)
  const unsigned short* w;    // (K,3,3,Cg)
  unsigned short* out;        // y (fwd) or dx (dgrad), (N,OH,OW,C)
  float* part;                // wgrad: [chunks][C/16][9][16][16*NCT]
  const unsigned short* dy;   // wgrad
  int N, C, Cg;
  int IH, IW;                 // stored size of `in`
  int OH, OW;                 // tiled (output) size
  // fwd/dgrad: output (o) tap (t) reads virtual input o*OS - padv + t; the
  // virtual input is `in` dilated by dil (1 or 2)
  int dil, padv;
  int tiles_h, tiles_w, nct;
  long nsp;                   // spatial tiles = N*tiles_h*tiles_w
  int chunks;                 // blocks per channel tile
};

DEV unsigned short f2bf(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

DEV bf16x8 as_frag(uint4 v) { return __builtin_bit_cast(bf16x8, v); }

struct TileCoord {
  int n, oh0, ow0;
};

template <int TH> DEV TileCoord tile_coord(const GcParams& q, long sp) {
  TileCoord t;
  const int twb = (int)(sp % q.tiles_w);
  const long r = sp / q.tiles_w;
  t.n = (int)(r / q.tiles_h);
  t.oh0 = (int)(r - (long)t.n * q.tiles_h) * TH;
  t.ow0 = twb * GC_TW;
  return t;
}

// 16-byte load of 8 channels of virtual input pixel (vh, vw), zero outside
// the image, between the samples of a dilated input and past the channels
DEV uint4 load_in(const GcParams& q, int n, int vh, int vw, int c, bool cok) {
  bool ok = cok && vh >= 0 && vw >= 0;
  int ih = vh, iw = vw;
  if (q.dil == 2) {
    ok = ok && !((vh | vw) & 1);
    ih = vh >> 1;
    iw = vw >> 1;
  }
  ok = ok && ih < q.IH && iw < q.IW;
  uint4 v = {0u, 0u, 0u, 0u};
  if (ok)
    v = *reinterpret_cast<const uint4*>(
        q.in + (((long)n * q.IH + ih) * q.IW + iw) * q.C + c);
  return v;
}

// ---------------------------------------------------------------------
// forward (DGRAD = false, OS = conv stride) and data-grad (DGRAD = true,
// OS = 1, q.dil = conv stride)
template <int TH, int OS, bool DGRAD, bool CG32>
__global__ __launch_bounds__(GC_THREADS, 2)
void gconv_kernel(GcParams q) {
  constexpr int NT = CG32 ? 9 : 5;             // MFMAs per pixel block
  constexpr int PH = (TH - 1) * OS + 3;        // patch rows
  constexpr int PW = (GC_TW - 1) * OS + 3;     // patch columns
  constexpr int HALFW = (PW + 1) / 2;          // OS == 2: even columns
  constexpr int PWP = OS == 2 ? 2 * HALFW : PW;
  constexpr int NLOAD = PH * PW * 8;           // 16-byte chunks of a patch
  constexpr int U = 5;                         // loads in flight per thread
  __shared__ __attribute__((aligned(16)))
      unsigned short patch[PH * PWP * GC_PITCH];
  __shared__ __attribute__((aligned(16)))
      unsigned short ot[TH * GC_TW * GC_PITCH];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int g = lane >> 4, l15 = lane & 15;
  const int ct = blockIdx.x % q.nct;
  const int chunk = blockIdx.x / q.nct;
  const int cb = ct * GC_CT;
  const int ccnt = min(q.C - cb, GC_CT);
  const bool active = wid * 16 < ccnt;

  // weight fragments: row = this lane's output channel co, k index
  // 8*g + j = (tap, input channel) of MFMA t
  bf16x8 wf[NT];
  int boff[NT];
  {
    const int co = cb + wid * 16 + l15;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int tap = CG32 ? t : 2 * t + (g >> 1);
      const int tapc = min(tap, 8);
      if (!DGRAD) {
        // the 8 input channels of a fragment are contiguous in w's row co:
        // one 16-byte load (Cg = 4: the 8 bytes of co's own group)
        const int ci0 = cb + wid * 16 + 8 * (g & 1);
        const unsigned short* row = q.w + ((long)co * 9 + tapc) * q.Cg;
        uint4 v = {0u, 0u, 0u, 0u};
        if (CG32) {
          if (active) v = *reinterpret_cast<const uint4*>(row + 8 * g);
        } else if (active && tap < 9 &&
                   ci0 / max(q.Cg, 8) == co / max(q.Cg, 8)) {
          if (q.Cg == 4) {
            const uint2 h = *reinterpret_cast<const uint2*>(row);
            if (co & 4) { v.z = h.x; v.w = h.y; } else { v.x = h.x; v.y = h.y; }
          } else {
            v = *reinterpret_cast<const uint4*>(row + ci0 % q.Cg);
          }
        }
        wf[t] = as_frag(v);
      } else {
        // transposed within the group: 2-byte gathers, coalesced over co
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          unsigned short v = 0;
          if (active) {
            if (CG32) {
              const int gb = co & ~31, kk = 8 * g + j;
              v = q.w[((long)(gb + kk) * 9 + (8 - tap)) * 32 + (co - gb)];
            } else {
              const int ci = cb + wid * 16 + 8 * (g & 1) + j;
              if (tap < 9 && ci / q.Cg == co / q.Cg)
                v = q.w[((long)ci * 9 + (8 - tap)) * q.Cg + co % q.Cg];
            }
          }
          wf[t][j] = (short)v;
        }
      }
      // this lane's activation fragment of MFMA t, relative to the patch
      // row of its pixel block: pixel column l15, tap (r, s)
      const int r = tapc / 3, s = tapc - 3 * r;
      const int pw = l15 * OS + s;
      const int col = OS == 2 ? (pw & 1) * HALFW + (pw >> 1) : pw;
      const int ch = CG32 ? ((wid * 16) & ~31) + 8 * g : wid * 16 + 8 * (g & 1);
      boff[t] = (r * PWP + col) * GC_PITCH + ch;
    }
  }

  for (long sp = chunk; sp < q.nsp; sp += q.chunks) {
    const TileCoord tc = tile_coord<TH>(q, sp);
    const int vh0 = tc.oh0 * OS - q.padv, vw0 = tc.ow0 * OS - q.padv;
    // patch -> LDS, U loads in flight per thread
#pragma unroll
    for (int b0 = 0; b0 < NLOAD; b0 += U * GC_THREADS) {
      uint4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = b0 + u * GC_THREADS + tid;
        const int pix = idx >> 3, c8 = idx & 7;
        const int ph = pix / PW, pw = pix - ph * PW;
        v[u] = load_in(q, tc.n, vh0 + ph, vw0 + pw, cb + c8 * 8,
                       idx < NLOAD && c8 * 8 < ccnt);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = b0 + u * GC_THREADS + tid;
        const int pix = idx >> 3, c8 = idx & 7;
        const int ph = pix / PW, pw = pix - ph * PW;
        const int col = OS == 2 ? (pw & 1) * HALFW + (pw >> 1) : pw;
        if (idx < NLOAD)
          *reinterpret_cast<uint4*>(
              &patch[(ph * PWP + col) * GC_PITCH + c8 * 8]) = v[u];
      }
    }
    __syncthreads();

    if (active) {
#pragma unroll
      for (int m = 0; m < TH; ++m) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const unsigned short* prow = patch + m * OS * PWP * GC_PITCH;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          bf16x8 xf = *reinterpret_cast<const bf16x8*>(prow + boff[t]);
          // the 10th tap: zero on both sides, so no 0 * inf
          if (!CG32 && t == NT - 1 && g >= 2) xf = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t], xf, acc, 0, 0,
                                                        0);
        }
        // D: row = channel 4*g + reg, col = pixel l15
        uint2 v;
        v.x = (unsigned)f2bf(acc[0]) | ((unsigned)f2bf(acc[1]) << 16);
        v.y = (unsigned)f2bf(acc[2]) | ((unsigned)f2bf(acc[3]) << 16);
        *reinterpret_cast<uint2*>(
            &ot[(m * GC_TW + l15) * GC_PITCH + wid * 16 + 4 * g]) = v;
      }
    }
    __syncthreads();

    // 16 B/lane stores: 8 lanes cover one pixel's 64 channels
#pragma unroll
    for (int it = 0; it < TH * GC_TW * 8 / GC_THREADS; ++it) {
      const int idx = it * GC_THREADS + tid;
      const int p = idx >> 3, c8 = idx & 7;
      const int oh = tc.oh0 + (p >> 4), ow = tc.ow0 + (p & 15);
      if (oh < q.OH && ow < q.OW && c8 * 8 < ccnt) {
        const uint4 v =
            *reinterpret_cast<const uint4*>(&ot[p * GC_PITCH + c8 * 8]);
        *reinterpret_cast<uint4*>(
            q.out + (((long)tc.n * q.OH + oh) * q.OW + ow) * q.C + cb +
            c8 * 8) = v;
      }
    }
    // the next tile's patch writes are ordered behind this tile's fragment
    // reads by the barrier above; its epilogue writes behind these reads by
    // the barrier after its patch load
  }
}

// ---------------------------------------------------------------------
// weight-grad. q.in = x (N,IH,IW,C), q.dy = dy (N,OH,OW,C), q.padv = pad.
template <int ST> struct GwGeom {
  static constexpr int TH = ST == 2 ? 4 : 8;
  static constexpr int PH = (TH - 1) * ST + 3;
  static constexpr int PW = (GC_TW - 1) * ST + 3;
  static constexpr int PARW = 24;   // even-column block of a stride-2 row
  // LDS row of one channel's patch row: every 16-pixel aligned read of a
  // window stays inside it
  static constexpr int RP = ST == 2 ? PARW + 16 : 24;
  // channel pitch: an odd number of 16-byte units
  static constexpr int CP = PH * RP + (((PH * RP / 8) & 1) ? 0 : 8);
  static constexpr int DP = TH * GC_TW + 8;
};

// elements j+1 .. j+8 of the 16 halves (lo, hi)
DEV bf16x8 window1(uint4 lo, uint4 hi) {
  uint4 r;
  r.x = (lo.x >> 16) | (lo.y << 16);
  r.y = (lo.y >> 16) | (lo.z << 16);
  r.z = (lo.z >> 16) | (lo.w << 16);
  r.w = (lo.w >> 16) | (hi.x << 16);
  return as_frag(r);
}

template <int ST, int NCT>
__global__ __launch_bounds__(GC_THREADS, 2)
void gconv_wgrad_kernel(GcParams q) {
  using G = GwGeom<ST>;
  constexpr int TH = G::TH, PH = G::PH, PW = G::PW, RP = G::RP;
  constexpr int CP = G::CP, DP = G::DP;
  constexpr int NLOAD = PH * PW * 8;
  constexpr int U = 5;
  __shared__ __attribute__((aligned(16)))
      unsigned short xT[GC_CT * CP + GC_CT];   // [channel][row][col]
  __shared__ __attribute__((aligned(16)))
      unsigned short dyT[GC_CT * DP + GC_CT];  // [channel][pixel]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int g = lane >> 4, l15 = lane & 15;
  const int ct = blockIdx.x % q.nct;
  const int chunk = blockIdx.x / q.nct;
  const int cb = ct * GC_CT;
  const int ccnt = min(q.C - cb, GC_CT);
  const bool active = wid * 16 < ccnt;

  // channel ch of the tile starts at ch*pitch + 8*(ch/8)
  const int kl = wid * 16 + l15;
  const unsigned short* afrag = dyT + kl * DP + (kl >> 3) * 8 + 8 * g;
  const unsigned short* bfrag[NCT];
#pragma unroll
  for (int nt = 0; nt < NCT; ++nt) {
    const int cl = (NCT == 2 ? ((wid * 16) & ~31) + nt * 16 : wid * 16) + l15;
    // MFMA k index 8*g + j of step ks: tile row 2*ks + g/2, col 8*(g%2) + j
    bfrag[nt] = xT + cl * CP + (cl >> 3) * 8 + (g >> 1) * ST * RP + 8 * (g & 1);
  }

  f32x4 acc[9][NCT];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int nt = 0; nt < NCT; ++nt) acc[t][nt] = {0.f, 0.f, 0.f, 0.f};

  for (long sp = chunk; sp < q.nsp; sp += q.chunks) {
    const TileCoord tc = tile_coord<TH>(q, sp);
    const int vh0 = tc.oh0 * ST - q.padv, vw0 = tc.ow0 * ST - q.padv;
    // x patch -> LDS transposed; outside the image it is zeros
#pragma unroll
    for (int b0 = 0; b0 < NLOAD; b0 += U * GC_THREADS) {
      uint4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = b0 + u * GC_THREADS + tid;
        const int pix = idx >> 3, c8 = idx & 7;
        const int ph = pix / PW, pw = pix - ph * PW;
        v[u] = load_in(q, tc.n, vh0 + ph, vw0 + pw, cb + c8 * 8,
                       idx < NLOAD && c8 * 8 < ccnt);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = b0 + u * GC_THREADS + tid;
        const int pix = idx >> 3, c8 = idx & 7;
        const int ph = pix / PW, pw = pix - ph * PW;
        const int col = ST == 2 ? (pw & 1) * G::PARW + (pw >> 1) : pw;
        if (idx < NLOAD) {
          unsigned short* d = &xT[c8 * 8 * CP + c8 * 8 + ph * RP + col];
          const unsigned e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            d[(2 * i) * CP] = (unsigned short)(e[i] & 0xffffu);
            d[(2 * i + 1) * CP] = (unsigned short)(e[i] >> 16);
          }
        }
      }
    }
    // dy tile -> LDS transposed; pixels outside dy are zeros
#pragma unroll
    for (int it = 0; it < TH * GC_TW * 8 / GC_THREADS; ++it) {
      const int idx = it * GC_THREADS + tid;
      const int p = idx >> 3, c8 = idx & 7;
      const int oh = tc.oh0 + (p >> 4), ow = tc.ow0 + (p & 15);
      uint4 v = {0u, 0u, 0u, 0u};
      if (oh < q.OH && ow < q.OW && c8 * 8 < ccnt)
        v = *reinterpret_cast<const uint4*>(
            q.dy + (((long)tc.n * q.OH + oh) * q.OW + ow) * q.C + cb + c8 * 8);
      unsigned short* d = &dyT[c8 * 8 * DP + c8 * 8 + p];
      const unsigned e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        d[(2 * i) * DP] = (unsigned short)(e[i] & 0xffffu);
        d[(2 * i + 1) * DP] = (unsigned short)(e[i] >> 16);
      }
    }
    __syncthreads();

    if (active) {
#pragma unroll
      for (int ks = 0; ks < TH / 2; ++ks) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(afrag + ks * 32);
#pragma unroll
        for (int nt = 0; nt < NCT; ++nt) {
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const unsigned short* rp = bfrag[nt] + (2 * ks * ST + r) * RP;
            const uint4 lo = *reinterpret_cast<const uint4*>(rp);
            const uint4 hi = *reinterpret_cast<const uint4*>(rp + 8);
            bf16x8 xf[3];
            xf[0] = as_frag(lo);
            if (ST == 2) {
              xf[1] = *reinterpret_cast<const bf16x8*>(rp + G::PARW);
              xf[2] = window1(lo, hi);
            } else {
              xf[1] = window1(lo, hi);
              xf[2] = as_frag(uint4{lo.y, lo.z, lo.w, hi.x});
            }
#pragma unroll
            for (int s = 0; s < 3; ++s)
              acc[r * 3 + s][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  af, xf[s], acc[r * 3 + s][nt], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }

  // partial slab [chunk][slab][tap][k 16][c 16*NCT]: D row = k 4*g + reg,
  // col = c l15
  if (active) {
    constexpr int NC = 16 * NCT;
    float* out = q.part +
                 (((long)chunk * (q.C / 16) + cb / 16 + wid) * 9) * 16 * NC;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int nt = 0; nt < NCT; ++nt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          out[(t * 16 + 4 * g + reg) * NC + nt * 16 + l15] = acc[t][nt][reg];
  }
}

// dw[k][tap][c] (bf16, the weight's channels_last memory) = the sum of the
// partial slabs' diagonal-block element in a fixed order: 8 slab groups x
// 32 elements per block, each thread sums its group's slabs ascending,
// then the 8 group sums are added ascending and rounded once.
__global__ __launch_bounds__(256)
void gconv_combine_kernel(const float* __restrict__ part,
                          unsigned short* __restrict__ dw, int total, int C,
                          int Cg, int chunks) {
  __shared__ float red[8][32];
  const int e = threadIdx.x & 31;
  const int grp = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + e;
  float s = 0.f;
  if (i < total) {
    const int c = i % Cg;
    const int tap = (i / Cg) % 9;
    const int k = i / (9 * Cg);
    const int kl = k & 15;
    const int nc = Cg == 32 ? 32 : 16;
    const int col = Cg == 32 ? c : kl / Cg * Cg + c;
    const long slab = (long)(C / 16) * 9 * 16 * nc;
    const long off = (((long)(k >> 4) * 9 + tap) * 16 + kl) * nc + col;
    for (int ch = grp; ch < chunks; ch += 8) s += part[ch * slab + off];
  }
  red[grp][e] = s;
  __syncthreads();
  if (grp == 0 && i < total) {
    float r = red[0][e];
#pragma unroll
    for (int k = 1; k < 8; ++k) r += red[k][e];
    dw[i] = f2bf(r);
  }
}

void fill_tiles(GcParams& q, int th, int max_blocks) {
  q.tiles_h = (q.OH + th - 1) / th;
  q.tiles_w = (q.OW + GC_TW - 1) / GC_TW;
  q.nct = (q.C + GC_CT - 1) / GC_CT;
  q.nsp = (long)q.N * q.tiles_h * q.tiles_w;
  q.chunks = (int)i64max(i64min(q.nsp, max_blocks / q.nct), 1);
}

template <int TH, int OS, bool DGRAD>
void launch_gconv(const GcParams& q, hipStream_t stream) {
  const dim3 grid(q.chunks * q.nct), block(GC_THREADS);
  if (q.Cg == 32)
    hipLaunchKernelGGL((gconv_kernel<TH, OS, DGRAD, true>), grid, block, 0,
                       stream, q);
  else
    hipLaunchKernelGGL((gconv_kernel<TH, OS, DGRAD, false>), grid, block, 0,
                       stream, q);
  HIP_CHECK_LAST();
}

void check_problem(int C, int Cg, int stride, int pad) {
  const bool cg_ok = Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32;
  if (!cg_ok || C % Cg || C % (Cg == 32 ? 32 : 16) || C == Cg ||
      (stride != 1 && stride != 2) || (pad != 0 && pad != 1))
    throw std::runtime_error("conv_grouped: unsupported problem");
}

}  // namespace

void ddlb::launch_conv_grouped_fwd(const void* x, const void* w, void* y,
                                   int N, int H, int W, int C, int Cg, int OH,
                                   int OW, int stride, int pad,
                                   hipStream_t stream) {
  check_problem(C, Cg, stride, pad);
  GcParams q = {};
  q.in = (const unsigned short*)x;
  q.w = (const unsigned short*)w;
  q.out = (unsigned short*)y;
  q.N = N; q.C = C; q.Cg = Cg; q.IH = H; q.IW = W; q.OH = OH; q.OW = OW;
  q.dil = 1; q.padv = pad;
  if (stride == 1) {
    fill_tiles(q, 8, GC_MAX_BLOCKS);
    launch_gconv<8, 1, false>(q, stream);
  } else {
    // the stride-2 patch is ~4x the tile: 4 rows keep 2+ blocks per CU
    fill_tiles(q, 4, GC_MAX_BLOCKS);
    launch_gconv<4, 2, false>(q, stream);
  }
}

void ddlb::launch_conv_grouped_dgrad(const void* dy, const void* w, void* dx,
                                     int N, int H, int W, int C, int Cg,
                                     int OH, int OW, int stride, int pad,
                                     hipStream_t stream) {
  check_problem(C, Cg, stride, pad);
  GcParams q = {};
  q.in = (const unsigned short*)dy;
  q.w = (const unsigned short*)w;
  q.out = (unsigned short*)dx;
  q.N = N; q.C = C; q.Cg = Cg; q.IH = OH; q.IW = OW; q.OH = H; q.OW = W;
  q.dil = stride; q.padv = 2 - pad;
  fill_tiles(q, 8, GC_MAX_BLOCKS);
  launch_gconv<8, 1, true>(q, stream);
}

long ddlb::conv_grouped_wgrad_part_floats(int N, int C, int Cg, int OH,
                                          int OW, int stride) {
  GcParams q = {};
  q.N = N; q.C = C; q.OH = OH; q.OW = OW;
  fill_tiles(q, stride == 2 ? GwGeom<2>::TH : GwGeom<1>::TH, GW_MAX_BLOCKS);
  return (long)q.chunks * (C / 16) * 9 * 16 * (Cg == 32 ? 32 : 16);
}

void ddlb::launch_conv_grouped_wgrad(const void* x, const void* dy, void* dw,
                                     float* part, int N, int H, int W, int C,
                                     int Cg, int OH, int OW, int stride,
                                     int pad, hipStream_t stream) {
  check_problem(C, Cg, stride, pad);
  GcParams q = {};
  q.in = (const unsigned short*)x;
  q.dy = (const unsigned short*)dy;
  q.part = part;
  q.N = N; q.C = C; q.Cg = Cg; q.IH = H; q.IW = W; q.OH = OH; q.OW = OW;
  q.dil = 1; q.padv = pad;
  fill_tiles(q, stride == 2 ? GwGeom<2>::TH : GwGeom<1>::TH, GW_MAX_BLOCKS);
  const dim3 grid(q.chunks * q.nct), block(GC_THREADS);
  if (stride == 1 && Cg == 32)
    hipLaunchKernelGGL((gconv_wgrad_kernel<1, 2>), grid, block, 0, stream, q);
  else if (stride == 1)
    hipLaunchKernelGGL((gconv_wgrad_kernel<1, 1>), grid, block, 0, stream, q);
  else if (Cg == 32)
    hipLaunchKernelGGL((gconv_wgrad_kernel<2, 2>), grid, block, 0, stream, q);
  else
    hipLaunchKernelGGL((gconv_wgrad_kernel<2, 1>), grid, block, 0, stream, q);
  HIP_CHECK_LAST();
  const int total = C * 9 * Cg;
  hipLaunchKernelGGL(gconv_combine_kernel, dim3((total + 31) / 32), dim3(256),
                     0, stream, part, (unsigned short*)dw, total, C, Cg,
                     q.chunks);
  HIP_CHECK_LAST();
}
