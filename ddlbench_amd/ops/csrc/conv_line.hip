// 1-D ("line") convolution on MFMA for gfx950: the (1,T) and (T,1) convs
// of Inception's factorised 7x7 blocks. bf16 NHWC, fp32 accumulation on
// v_mfma_f32_16x16x32_bf16, stride 1, padding T/2 along the filter and 0
// across it, T in {3, 7}, C % 32 == 0, K % 32 == 0.
//
// A *line* is the run of pixels the filter slides along: an image row
// (n,h) for (1,T) — length L = W, pixel pitch 1 — or an image column (n,w)
// for (T,1) — length L = H, pixel pitch W. Both are one kernel: pixel
// (line, pos) is  (line / lpi) * img + (line % lpi) * lstep + pos * pp.
//
// forward / data-grad (conv_line_kernel):
//   256 threads, 4 waves. A tile is BL whole lines (BL*L <= 128 GEMM rows,
//   a wave owns 32 of them) times 64 output channels. Per 32-channel chunk
//   the block stages each of its lines ONCE into LDS as L + T - 1 pixel
//   slots of 64 B; the T/2 slots at either end of a line are zeros, written
//   to LDS once per block and never loaded. Tap t of GEMM row (line, pos)
//   is slot line*(L+T-1) + pos + t, so the T MFMA passes over a chunk only
//   differ by an address offset: no validity test, no zero page, and the
//   activation is read from global memory once per chunk instead of T
//   times. The weight chunk is staged as T tiles of [64][32].
//   The 16-byte piece c of a slot (or weight row) s sits at position
//   c ^ sigma((s >> 2) & 3) (conv_mfma2.hip's ds_read_b128 swizzle, on the
//   absolute slot index); the per-(row, tap) read offsets are computed once
//   per block. Chunks are double-buffered: the next chunk's global loads
//   are issued into registers before the current chunk's T passes and
//   written to the other buffer after them, one barrier per chunk.
//   The tile leaves through an LDS image as 16-byte stores; the (T,1)
//   orientation walks the image position-major, so every position is a run
//   of BL consecutive pixels. Blocks walk tiles grid-stride in XCD order.
//   The data-grad is the same kernel on dy and the (C,T,K) weight image
//   with the taps reversed.
//
// weight-grad (conv_line_wgrad_kernel + conv_line_combine_kernel):
//   dW[k,t,c] = sum_j dyS[j,k] * xS[j + t - T/2, c] over slot indices j of
//   the same zero-haloed slot scheme (both operands), so a tap is again an
//   offset of the reduction index. A block owns a 64(K) x 64(C) tile of dW
//   for all T taps (T*4 accumulator fragments per wave) and a slice of the
//   lines, which it walks in steps of up to 128 slots. Both operands are
//   read transposed with ds_read_b64_tr_b16 from images of [4 slots][16
//   channels] blocks. The transposed read takes 4 aligned slots, so x is
//   kept in min(T,4) copies shifted by 0..3 slots: tap t reads copy t & 3
//   at block offset t >> 2. Each block writes one fp32 slab; the combine
//   adds an element's slabs in slab order and rounds once to bf16 in the
//   weight's (K,T,C) memory. No atomics, no memset, same bits every call.

#include "mfma_common.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <string>

// plain v_fma_f32 / v_add_f32 only in this file
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

constexpr int CL_THREADS = 256;
constexpr int CL_BM = 128;        // GEMM rows per tile, at most
constexpr int CL_BN = 64;         // output channels per tile
constexpr int CL_MAX_BL = 32;     // lines per tile, at most
constexpr int CL_MAX_GRID = 512;  // 2 blocks per CU
constexpr int CL_WG_TILE = 64;    // weight-grad: K and C extent of a tile
constexpr int CL_WG_SLOTS = 128;  // weight-grad: slots per step, at most
constexpr int CL_WG_BLOCKS = 256; // weight-grad: one block per CU
constexpr int CL_WG_SLABS = 64;

DEV int sigma4(int x) { return (0x1320 >> (x * 4)) & 0xF; }

// pixel addressing shared by the three directions
struct LineGeom {
  int nlines, L;
  int lpi;    // lines per image
  int lstep;  // pixels between neighbouring lines of an image
  int pp;     // pixels between neighbouring positions of a line
  long img;   // pixels per image
};

DEV long line_pixel(const LineGeom& g, int line, int pos) {
  const int n = line / g.lpi;
  return (long)n * g.img + (long)(line - n * g.lpi) * g.lstep +
         (long)pos * g.pp;
}

struct LineParams {
  const unsigned short* a;  // x (fwd) or dy (dgrad): [pixel][Cred]
  const unsigned short* b;  // weight image [Nd][T][Cred]
  unsigned short* out;      // y or dx: [pixel][Nd]
  LineGeom g;
  int Cred, Nd;
  int BL;        // lines per tile
  int nnt;       // column tiles
  long tiles;
  int flip;      // dgrad: tap t reads weight tap T-1-t
  int pos_major; // (T,1): store positions outermost
};

template <int T>
__global__ __launch_bounds__(CL_THREADS, 2)
void conv_line_kernel(LineParams p) {
  constexpr int HALO = T / 2;
  constexpr int BTILE = CL_BN * 32;  // halfwords of one tap's weight tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* lds = reinterpret_cast<short*>(smem);
  const int L = p.g.L;
  const int LS = L + T - 1;        // slots per line
  const int SA = p.BL * LS;        // slots per A buffer
  const int rows = p.BL * L;       // GEMM rows of a full tile
  short* abase = lds;                    // 2 buffers of SA slots
  short* bbase = lds + 2 * SA * 32;      // 2 buffers of T weight tiles

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int fr = lane & 15;
  const int fk = lane >> 4;

  // halo slots are zero for the whole life of the block: staging only
  // ever writes the L real slots of a line
  for (int i = tid; i < 2 * SA * 4; i += CL_THREADS)
    reinterpret_cast<u16x8*>(abase)[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};

  // ---- staging geometry, the same for every tile ------------------------
  // A: 16-byte piece i = tid + 256 j of the tile: GEMM row i >> 2
  int a_line[2], a_pos[2], a_dst[2], a_cg[2];
  bool a_rowok[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = tid + CL_THREADS * j;
    const int r = i >> 2;
    a_rowok[j] = r < rows;
    const int rr = a_rowok[j] ? r : 0;
    a_line[j] = rr / L;
    a_pos[j] = rr - a_line[j] * L;
    const int s = a_line[j] * LS + HALO + a_pos[j];
    a_dst[j] = s * 32 + (i & 3) * 8;
    a_cg[j] = (i & 3) ^ sigma4((s >> 2) & 3);
  }
  // B: weight row tid >> 2 of every tap
  const int b_n = tid >> 2;
  const int b_cg = (tid & 3) ^ sigma4((b_n >> 2) & 3);
  const int b_dst = b_n * 32 + (tid & 3) * 8;

  // ---- fragment read offsets (halfwords) --------------------------------
  int aoff[2][T];
#pragma unroll
  for (int mf = 0; mf < 2; ++mf) {
    const int r = wid * 32 + mf * 16 + fr;
    const int rr = r < rows ? r : 0;  // padding rows read row 0: in bounds
    const int line = rr / L;
    const int rs = line * LS + (rr - line * L);
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int s = rs + t;
      aoff[mf][t] = s * 32 + ((fk ^ sigma4((s >> 2) & 3)) * 8);
    }
  }
  const int boff = fr * 32 + ((fk ^ sigma4((fr >> 2) & 3)) * 8);

  const int nchunks = p.Cred / 32;
  __syncthreads();

  for (long tile = xcd_remap(blockIdx.x, gridDim.x); tile < p.tiles;
       tile += gridDim.x) {
    const int mt = (int)(tile / p.nnt);
    const int bn = (int)(tile - (long)mt * p.nnt) * CL_BN;
    const int line0 = mt * p.BL;
    // 16-column fragments of this tile that exist (Nd % 32 == 0)
    const int nfv = min(4, (p.Nd - bn) / 16);

    const unsigned short* a_src[2];
    bool a_ok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gl = line0 + a_line[j];
      a_ok[j] = a_rowok[j] && gl < p.g.nlines;
      a_src[j] = p.a + (a_ok[j] ? line_pixel(p.g, gl, a_pos[j]) * p.Cred +
                                      a_cg[j] * 8
                                : 0);
    }
    const bool b_ok = bn + b_n < p.Nd;
    const unsigned short* b_src =
        p.b + (b_ok ? (long)(bn + b_n) * T * p.Cred + b_cg * 8 : 0);

    u16x8 ra[2], rb[T];
    auto load = [&](int c) {
      const int c0 = c * 32;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        ra[j] = a_ok[j] ? *reinterpret_cast<const u16x8*>(a_src[j] + c0)
                        : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int tap = p.flip ? T - 1 - t : t;
        rb[t] = b_ok ? *reinterpret_cast<const u16x8*>(
                           b_src + (long)tap * p.Cred + c0)
                     : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    };
    auto write = [&](int buf) {
      short* la = abase + buf * SA * 32;
      short* lb = bbase + buf * T * BTILE;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (a_rowok[j]) *reinterpret_cast<u16x8*>(la + a_dst[j]) = ra[j];
#pragma unroll
      for (int t = 0; t < T; ++t)
        *reinterpret_cast<u16x8*>(lb + t * BTILE + b_dst) = rb[t];
    };

    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    load(0);
    write(0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
      if (c + 1 < nchunks) load(c + 1);
      const short* la = abase + (c & 1) * SA * 32;
      const short* lb = bbase + (c & 1) * T * BTILE + boff;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        bf16x8 af[2], bfr[4];
#pragma unroll
        for (int mf = 0; mf < 2; ++mf)
          af[mf] = *reinterpret_cast<const bf16x8*>(la + aoff[mf][t]);
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
          bfr[nf] = *reinterpret_cast<const bf16x8*>(lb + t * BTILE +
                                                     nf * 16 * 32);
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
          if (nf < nfv) {
#pragma unroll
            for (int mf = 0; mf < 2; ++mf)
              acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  af[mf], bfr[nf], acc[mf][nf], 0, 0, 0);
          }
      }
      if (c + 1 < nchunks) write((c + 1) & 1);
      __syncthreads();
    }

    // ---- epilogue: [128][64] bf16 image in the weight buffers ------------
    static_assert(CL_BM * CL_BN <= 2 * 3 * BTILE, "image fits the B region");
    unsigned short* img = reinterpret_cast<unsigned short*>(bbase);
#pragma unroll
    for (int mf = 0; mf < 2; ++mf)
#pragma unroll
      for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          img[(wid * 32 + mf * 16 + fk * 4 + reg) * CL_BN + nf * 16 + fr] =
              __bfloat16_as_ushort(__float2bfloat16(acc[mf][nf][reg]));
    __syncthreads();
#pragma unroll
    for (int it = 0; it < CL_BM * CL_BN / 8 / CL_THREADS; ++it) {
      const int idx = it * CL_THREADS + tid;
      const int ro = idx >> 3;
      const int ck = idx & 7;
      if (ro >= rows) continue;
      int line, pos;
      if (p.pos_major) {
        pos = ro / p.BL;
        line = ro - pos * p.BL;
      } else {
        line = ro / L;
        pos = ro - line * L;
      }
      const int gl = line0 + line;
      if (gl >= p.g.nlines || bn + ck * 8 >= p.Nd) continue;
      *reinterpret_cast<u16x8*>(p.out + line_pixel(p.g, gl, pos) * p.Nd +
                                bn + ck * 8) =
          *reinterpret_cast<const u16x8*>(img + (line * L + pos) * CL_BN +
                                          ck * 8);
    }
    __syncthreads();  // the image is the next tile's weight buffer
  }
}

// ---- weight-grad -------------------------------------------------------
struct LineWgradParams {
  const unsigned short* x;   // [pixel][C]
  const unsigned short* dy;  // [pixel][K]
  float* part;               // [slabs][K][T][C]
  LineGeom g;
  int C, K;
  int BLW;    // lines per step
  int SP;     // slots per step, padded to a multiple of 32
  int nct;    // C tiles
  int ntp;    // K tiles * C tiles
  int steps;  // ceil(nlines / BLW)
  int steps_per;  // steps per slab
};

// transposed fragment: column lane & 15 of the 16-channel group at grp,
// slots 4 blk .. 4 blk + 7 (two [4][16] blocks)
DEV bf16x8 line_tr_frag(const short* grp, int blk, int lane) {
  typedef __attribute__((address_space(3))) bf16x4* lds_b64;
  const short* base = grp + blk * 64 + (lane & 15) * 4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_b64)base);
  const bf16x4 hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_b64)(base + 64));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int T>
__global__ __launch_bounds__(CL_THREADS, 1)
void conv_line_wgrad_kernel(LineWgradParams q) {
  constexpr int HALO = T / 2;
  constexpr int NB = T < 4 ? T : 4;  // shifted x copies
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* lds = reinterpret_cast<short*>(smem);
  const int L = q.g.L;
  const int LS = L + T - 1;
  const int NQ = q.SP / 4 + 2;   // [4][16] blocks per channel group
  const int GRP = NQ * 64;       // halfwords of one channel group
  short* dyimg = lds;            // [4 groups][NQ][4][16]
  short* ximg = lds + 4 * GRP;   // [NB copies][4 groups][NQ][4][16]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int fk = lane >> 4;
  const int wk = wid >> 1, wc = wid & 1;

  const int tp = blockIdx.x % q.ntp;
  const int slab = blockIdx.x / q.ntp;
  const int kb = (tp / q.nct) * CL_WG_TILE;
  const int cb = (tp % q.nct) * CL_WG_TILE;
  const int s_begin = slab * q.steps_per;
  const int s_end = min(q.steps, s_begin + q.steps_per);

  // every slot staging does not write stays zero: halos and padding
  for (int i = tid; i < (4 + 4 * NB) * GRP / 8; i += CL_THREADS)
    reinterpret_cast<u16x8*>(lds)[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};

  // staging geometry: piece i = tid + 256 j is 8 channels of pixel i >> 3
  int s_line[4], s_pos[4], s_slot[4];
  bool s_rowok[4];
  const int c8 = tid & 7;
  const int sub = (c8 >> 1) * GRP + (c8 & 1) * 8;  // group + half row
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (tid + CL_THREADS * j) >> 3;
    s_rowok[j] = r < q.BLW * L;
    const int rr = s_rowok[j] ? r : 0;
    s_line[j] = rr / L;
    s_pos[j] = rr - s_line[j] * L;
    s_slot[j] = s_line[j] * LS + HALO + s_pos[j];
  }
  const bool k_ok = kb + c8 * 8 < q.K;
  const bool c_ok = cb + c8 * 8 < q.C;

  u16x8 rdy[4], rx[4];
  auto load = [&](int s) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gl = s * q.BLW + s_line[j];
      rdy[j] = rx[j] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (s_rowok[j] && gl < q.g.nlines) {
        const long px = line_pixel(q.g, gl, s_pos[j]);
        if (k_ok)
          rdy[j] = *reinterpret_cast<const u16x8*>(q.dy + px * q.K + kb +
                                                   c8 * 8);
        if (c_ok)
          rx[j] = *reinterpret_cast<const u16x8*>(q.x + px * q.C + cb +
                                                  c8 * 8);
      }
    }
  };
  // a line past the end is written as zeros: the slots belong to the sum
  auto write = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!s_rowok[j]) continue;
      const int sl = s_slot[j];
      *reinterpret_cast<u16x8*>(dyimg + sub + (sl >> 2) * 64 +
                                (sl & 3) * 16) = rdy[j];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        // copy b holds slot j at position j - b + HALO (>= 0: j >= HALO)
        const int i2 = sl - b + HALO;
        *reinterpret_cast<u16x8*>(ximg + b * 4 * GRP + sub + (i2 >> 2) * 64 +
                                  (i2 & 3) * 16) = rx[j];
      }
    }
  };

  f32x4 acc[T][2][2];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = {0.f, 0.f, 0.f, 0.f};

  if (s_begin < s_end) load(s_begin);
  for (int s = s_begin; s < s_end; ++s) {
    __syncthreads();  // the previous step's reads (or the zero fill) done
    write();
    __syncthreads();
    if (s + 1 < s_end) load(s + 1);
    for (int ks = 0; ks < q.SP / 32; ++ks) {
      const int blk = ks * 8 + fk * 2;
      bf16x8 af[2], bfr[T][2];
#pragma unroll
      for (int mf = 0; mf < 2; ++mf)
        af[mf] = line_tr_frag(dyimg + (wk * 2 + mf) * GRP, blk, lane);
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int nf = 0; nf < 2; ++nf)
          bfr[t][nf] = line_tr_frag(
              ximg + ((t & 3) * 4 + wc * 2 + nf) * GRP, blk + (t >> 2), lane);
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int mf = 0; mf < 2; ++mf)
#pragma unroll
          for (int nf = 0; nf < 2; ++nf)
            acc[t][mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[mf], bfr[t][nf], acc[t][mf][nf], 0, 0, 0);
    }
  }

  // one slab per block; a block without steps writes zeros
  float* out = q.part + (long)slab * q.K * T * q.C;
#pragma unroll
  for (int mf = 0; mf < 2; ++mf)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int k = kb + (wk * 2 + mf) * 16 + fk * 4 + reg;
      if (k >= q.K) continue;
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        const int c = cb + (wc * 2 + nf) * 16 + (lane & 15);
        if (c >= q.C) continue;
#pragma unroll
        for (int t = 0; t < T; ++t)
          out[((long)k * T + t) * q.C + c] = acc[t][mf][nf][reg];
      }
    }
}

// dw[i] = bf16(part[0][i] + part[1][i] + ...), slabs ascending; 4 elements
// per thread (total % 4 == 0)
__global__ __launch_bounds__(256)
void conv_line_combine_kernel(const float* __restrict__ part,
                              unsigned short* __restrict__ dw, long total,
                              int slabs) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= total) return;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int ps = 0; ps < slabs; ++ps) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(part + ps * total + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += v[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    dw[i + j] = __bfloat16_as_ushort(__float2bfloat16(s[j]));
}

LineGeom line_geom(int N, int H, int W, int orient_h) {
  LineGeom g;
  g.img = (long)H * W;
  if (orient_h) {  // (T,1): a line is a column (n,w)
    g.nlines = N * W; g.L = H; g.lpi = W; g.lstep = 1; g.pp = W;
  } else {         // (1,T): a line is a row (n,h)
    g.nlines = N * H; g.L = W; g.lpi = H; g.lstep = W; g.pp = 1;
  }
  return g;
}

size_t line_lds_bytes(const ddlb::LinePlan& pl, int T) {
  return (size_t)(2 * pl.BL * (pl.L + T - 1) * 32 + 2 * T * CL_BN * 32) * 2;
}

void launch_line(const ddlb::LinePlan& pl, const ddlb::LineTiling& tl,
                 const void* a, const void* b, void* out, int N, int H, int W,
                 int Cred, int Nd, int orient_h, int T, int flip,
                 hipStream_t stream) {
  LineParams p;
  p.a = (const unsigned short*)a;
  p.b = (const unsigned short*)b;
  p.out = (unsigned short*)out;
  p.g = line_geom(N, H, W, orient_h);
  p.Cred = Cred; p.Nd = Nd; p.BL = pl.BL; p.nnt = tl.ntn;
  p.tiles = tl.tiles; p.flip = flip; p.pos_major = orient_h;
  const size_t lds = line_lds_bytes(pl, T);
  if (T == 7)
    hipLaunchKernelGGL(conv_line_kernel<7>, dim3(tl.slots),
                       dim3(CL_THREADS), lds, stream, p);
  else
    hipLaunchKernelGGL(conv_line_kernel<3>, dim3(tl.slots),
                       dim3(CL_THREADS), lds, stream, p);
  HIP_CHECK_LAST();
}

}  // namespace

ddlb::LinePlan ddlb::line_plan(int N, int C, int K, int H, int W,
                               int orient_h, int T) {
  if (T != 3 && T != 7)
    throw std::runtime_error("conv_line needs a filter of 3 or 7 taps");
  if (C < 32 || K < 32 || C % 32 || K % 32)
    throw std::runtime_error("conv_line needs C % 32 == 0 and K % 32 == 0");
  const long nlines = (long)N * (orient_h ? W : H);
  const int L = orient_h ? H : W;
  if (N < 1 || L < 1 || L > 64 || nlines < 1 || nlines >= (1L << 31))
    throw std::runtime_error("conv_line needs 1 <= line length <= 64");
  LinePlan pl;
  pl.L = L;
  pl.nlines = nlines;
  pl.BL = (int)i64max(1, i64min(CL_MAX_BL, CL_BM / L));
  auto tiling = [&](int nd) {
    LineTiling t;
    t.ntm = (int)((nlines + pl.BL - 1) / pl.BL);
    t.ntn = (nd + CL_BN - 1) / CL_BN;
    t.tiles = (long)t.ntm * t.ntn;
    // a block walks at least two tiles where there are two, so the halo
    // fill and the offset tables are paid once for both
    t.slots = (int)i64max(1, i64min(CL_MAX_GRID, (t.tiles + 1) / 2));
    return t;
  };
  pl.fwd = tiling(K);
  pl.dgrad = tiling(C);
  // weight-grad: whole lines per step, at most CL_WG_SLOTS slots
  const int LS = L + T - 1;
  pl.BLW = (int)i64max(1, CL_WG_SLOTS / LS);
  pl.SP = (pl.BLW * LS + 31) / 32 * 32;
  pl.wgrad.ntm = (K + CL_WG_TILE - 1) / CL_WG_TILE;
  pl.wgrad.ntn = (C + CL_WG_TILE - 1) / CL_WG_TILE;
  pl.wgrad.tiles = (nlines + pl.BLW - 1) / pl.BLW;  // steps
  const int ntp = pl.wgrad.ntm * pl.wgrad.ntn;
  long slabs = i64min(CL_WG_SLABS, i64max(1, CL_WG_BLOCKS / ntp));
  slabs = i64min(slabs, pl.wgrad.tiles);
  pl.steps_per = (int)((pl.wgrad.tiles + slabs - 1) / slabs);
  // no empty slab: the last one starts inside the steps
  slabs = (pl.wgrad.tiles + pl.steps_per - 1) / pl.steps_per;
  pl.wgrad.slots = (int)slabs;
  pl.part_floats = slabs * K * T * C;
  return pl;
}

void ddlb::launch_conv_line_fwd(const LinePlan& pl, const void* x,
                                const void* w, void* y, int N, int C, int K,
                                int H, int W, int orient_h, int T,
                                hipStream_t stream) {
  launch_line(pl, pl.fwd, x, w, y, N, H, W, C, K, orient_h, T, 0, stream);
}

void ddlb::launch_conv_line_dgrad(const LinePlan& pl, const void* dy,
                                  const void* w_crsk, void* dx, int N, int C,
                                  int K, int H, int W, int orient_h, int T,
                                  hipStream_t stream) {
  launch_line(pl, pl.dgrad, dy, w_crsk, dx, N, H, W, K, C, orient_h, T, 1,
              stream);
}

void ddlb::launch_conv_line_wgrad(const LinePlan& pl, const void* x,
                                  const void* dy, void* dw, float* part,
                                  int N, int C, int K, int H, int W,
                                  int orient_h, int T, hipStream_t stream) {
  LineWgradParams q;
  q.x = (const unsigned short*)x;
  q.dy = (const unsigned short*)dy;
  q.part = part;
  q.g = line_geom(N, H, W, orient_h);
  q.C = C; q.K = K; q.BLW = pl.BLW; q.SP = pl.SP;
  q.nct = pl.wgrad.ntn;
  q.ntp = pl.wgrad.ntm * pl.wgrad.ntn;
  q.steps = (int)pl.wgrad.tiles;
  q.steps_per = pl.steps_per;
  const int nb = T < 4 ? T : 4;
  const size_t lds = (size_t)(4 + 4 * nb) * (pl.SP / 4 + 2) * 64 * 2;
  const unsigned grid = (unsigned)(q.ntp * pl.wgrad.slots);
  if (T == 7)
    hipLaunchKernelGGL(conv_line_wgrad_kernel<7>, dim3(grid),
                       dim3(CL_THREADS), lds, stream, q);
  else
    hipLaunchKernelGGL(conv_line_wgrad_kernel<3>, dim3(grid),
                       dim3(CL_THREADS), lds, stream, q);
  const long total = (long)K * T * C;
  hipLaunchKernelGGL(conv_line_combine_kernel,
                     dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0,
                     stream, part, (unsigned short*)dw, total,
                     pl.wgrad.slots);
  HIP_CHECK_LAST();
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
