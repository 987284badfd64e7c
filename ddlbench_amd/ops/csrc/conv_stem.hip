// NHWC bf16 stem convolution (C < 8 inputs) on MFMA (gfx950): forward and
// weight-grad. The conv_igemm*/conv_wgrad* kernels stage 16-byte
// (8-channel) tap vectors, which a C=3 pixel (6 bytes, 2-byte aligned
// rows when W is odd) cannot feed — this file is the small-C path.
//
//   fwd :  y[p][k]   = sum_kd im2col(x)[p][kd] * w[k][kd]
//   wgrad: dw[k][kd] = sum_p  dy[p][k] * im2col(x)[p][kd]
// with kd = (r, s, c) row-major, Kd = R*R*C <= 196 — exactly the weight's
// channels_last memory, so no pack kernel and no host-side pad.
//
// Shared structure:
//   * A block owns a tile of 8 output rows x 16 output columns (128
//     pixels) and loops over tiles (grid-stride) with the K tile fixed, so
//     weights (fwd) / accumulators (wgrad) live for the whole block.
//   * The input patch — ((8-1)*stride + R) rows of ((16-1)*stride + R)*C
//     contiguous bf16 — is copied to LDS once per tile with aligned dword
//     loads. The LDS image keeps the 2-byte parity of the global address
//     (row pitch parity == (W*C) parity), so an aligned global pair is an
//     aligned LDS pair; edge pairs fall back to one 2-byte load. Everything
//     outside the image is zero-filled here, so fragments need no border
//     logic.
//   * im2col fragments are gathered from the patch with per-lane offsets
//     off(kd) = r*pitch + s*C + c computed once per block.
//   * fwd: the weights are the MFMA A operand (rows = output channels), so
//     each lane ends up with 4 consecutive channels of one pixel: packed
//     8-byte LDS writes into a [pixel][channel] tile, then 16 B/lane global
//     stores (LDS-transpose epilogue as in conv_mfma2.hip).
//   * wgrad: dy is transposed while staging ([k][p] in LDS) so its
//     fragments are 16-byte LDS reads; P is the MFMA k dimension. Each
//     block writes one fp32 partial slab; stem_combine_kernel sums slabs in
//     a fixed order. No global atomics: results are bit-identical from call
//     to call.
//
// Limits (checked in bindings.hip): C in 1..4, square R in {3,5,7},
// stride in {1,2}, 0 <= pad <= R/2, K % 8 == 0, K <= 128.

#include "mfma_common.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <string>

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_TH = 8;          // output rows per tile
constexpr int ST_TW = 16;         // output cols per tile (one MFMA block)
constexpr int ST_TP = ST_TH * ST_TW;
constexpr int ST_KT = 64;         // output channels per block
constexpr int ST_MAXKS = 7;       // ceil(196 / 32)
constexpr int ST_MAXKDP = ST_MAXKS * 32;
constexpr int ST_WPITCH_MAX = ST_MAXKDP + 8;
// patch: 21 rows x ((15*2+7)*4 + 5) elements + parity shift, rounded up
constexpr int ST_PATCH = 3328;
constexpr int ST_OPITCH = ST_KT + 8;   // fwd epilogue tile pitch (halves)
constexpr int ST_DPITCH = ST_TP + 8;   // wgrad dy^T pitch (halves)

struct StemParams {
  const unsigned short* x;   // (N,H,W,C)
  const unsigned short* w;   // (K, Kd)            fwd
  unsigned short* y;         // (N,OH,OW,K)        fwd
  const unsigned short* dy;  // (N,OH,OW,K)        wgrad
  float* part;               // [chunks][K][Kd]    wgrad
  int N, H, W, C, K, OH, OW, R, stride, pad;
  int Kd, nks, SC;           // R*R*C, ceil(Kd/32), R*C
  int Lrow, pitch, PH, PPR;  // patch row length / pitch / rows / pairs
  int tiles_h, tiles_w, nkt;
  long nsp;                  // spatial tiles = N*tiles_h*tiles_w
  int chunks;                // blocks per K tile
};

DEV unsigned short f2bf(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

struct TileCoord {
  int n, oh0, ow0;
};

DEV TileCoord tile_coord(const StemParams& q, long sp) {
  TileCoord t;
  const int twb = (int)(sp % q.tiles_w);
  const long r = sp / q.tiles_w;
  t.n = (int)(r / q.tiles_h);
  t.oh0 = (int)(r - (long)t.n * q.tiles_h) * ST_TH;
  t.ow0 = twb * ST_TW;
  return t;
}

// Copy the tile's input patch to LDS, zero-filling outside the image.
// Returns the parity shift sh: patch element (pr, e) is at
// sh + pr*pitch + e.
DEV int load_patch(const StemParams& q, const TileCoord& t,
                   unsigned short* patch, int tid) {
  const int ih0 = t.oh0 * q.stride - q.pad;
  const int iw0 = t.ow0 * q.stride - q.pad;
  const long WC = (long)q.W * q.C;
  // element (2-byte) address of x, so parity follows the real pointer
  const long xa = (long)(reinterpret_cast<uintptr_t>(q.x) >> 1);
  const long a00 = xa + ((long)t.n * q.H + ih0) * WC + (long)iw0 * q.C;
  const int sh = (int)(a00 & 1);
  const int total = q.PH * q.PPR;
  for (int idx = tid; idx < total; idx += ST_THREADS) {
    const int pr = idx / q.PPR;
    const int i = idx - pr * q.PPR;
    const int ih = ih0 + pr;
    const int l0 = sh + pr * q.pitch;        // LDS element of e = 0
    const int le = (l0 & ~1) + 2 * i;        // this pair's LDS element
    if (le >= l0 + q.Lrow) continue;
    const long row_lo = xa + ((long)t.n * q.H + ih) * WC;
    const long row_hi = row_lo + WC;
    const long ae = row_lo + (long)iw0 * q.C + (le - l0);  // even
    const bool rowok = ih >= 0 && ih < q.H;
    const bool v0 = rowok && ae >= row_lo && ae < row_hi;
    const bool v1 = rowok && ae + 1 >= row_lo && ae + 1 < row_hi;
    unsigned val = 0;
    if (v0 && v1)
      val = *reinterpret_cast<const unsigned*>((uintptr_t)ae << 1);
    else if (v0)
      val = *reinterpret_cast<const unsigned short*>((uintptr_t)ae << 1);
    else if (v1)
      val = (unsigned)*reinterpret_cast<const unsigned short*>(
                (uintptr_t)(ae + 1) << 1) << 16;
    reinterpret_cast<unsigned*>(patch)[le >> 1] = val;
  }
  return sh;
}

// patch offset of reduction index kd (clamped to tap 0 past Kd; the
// matching weight column / dw column is zero / never stored)
DEV int kd_offset(const StemParams& q, int kd) {
  if (kd >= q.Kd) return 0;
  const int r = kd / q.SC;
  return r * q.pitch + (kd - r * q.SC);
}

// ---------------------------------------------------------------------
// forward
__global__ __launch_bounds__(ST_THREADS, 2)
void conv_stem_fwd_kernel(StemParams q) {
  __shared__ __attribute__((aligned(16))) unsigned short patch[ST_PATCH];
  __shared__ __attribute__((aligned(16)))
      unsigned short wl[ST_KT * ST_WPITCH_MAX];
  __shared__ __attribute__((aligned(16)))
      unsigned short ot[ST_TP * ST_OPITCH];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int kt = blockIdx.x % q.nkt;
  const int chunk = blockIdx.x / q.nkt;
  const int k0 = kt * ST_KT;
  const int kcnt = min(q.K - k0, ST_KT);
  const int nnb = (kcnt + 15) >> 4;
  const int kdp = q.nks * 32;
  const int wp = kdp + 8;

  // weights -> LDS once per block, zero-filling the Kd tail and k >= K
  for (int k = wid; k < nnb * 16; k += ST_THREADS / 64) {
    const bool kok = k < kcnt;
    const unsigned short* src = q.w + (long)(k0 + k) * q.Kd;
    for (int kd = lane; kd < kdp; kd += 64)
      wl[k * wp + kd] = (kok && kd < q.Kd) ? src[kd] : (unsigned short)0;
  }

  // per-lane gather offsets: fragment element j of k-step ks is
  // kd = ks*32 + 8*(lane>>4) + j
  int aoff[ST_MAXKS][8];
#pragma unroll
  for (int ks = 0; ks < ST_MAXKS; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      aoff[ks][j] = kd_offset(q, ks * 32 + 8 * (lane >> 4) + j);
  // elements of the last k-step past Kd are masked to zero
  bf16x8 tailmask;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    tailmask[j] =
        ((q.nks - 1) * 32 + 8 * (lane >> 4) + j < q.Kd) ? (short)-1 : (short)0;

  const int sC = q.stride * q.C;
  // this wave's two output rows of the tile, this lane's pixel column
  const int pbase0 = (2 * wid) * q.stride * q.pitch + (lane & 15) * sC;
  const int pbase1 = pbase0 + q.stride * q.pitch;

  for (long sp = chunk; sp < q.nsp; sp += q.chunks) {
    const TileCoord t = tile_coord(q, sp);
    const int sh = load_patch(q, t, patch, tid);
    __syncthreads();

    f32x4 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[m][nb] = {0.f, 0.f, 0.f, 0.f};

    const unsigned short* pa = patch + sh + pbase0;
    const unsigned short* pb = patch + sh + pbase1;
#pragma unroll
    for (int ks = 0; ks < ST_MAXKS; ++ks) {
      if (ks < q.nks) {
        bf16x8 x0, x1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          x0[j] = (short)pa[aoff[ks][j]];
          x1[j] = (short)pb[aoff[ks][j]];
        }
        if (ks == q.nks - 1) {
          x0 &= tailmask;
          x1 &= tailmask;
        }
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          if (nb < nnb) {
            const bf16x8 wf = *reinterpret_cast<const bf16x8*>(
                &wl[(nb * 16 + (lane & 15)) * wp + ks * 32 +
                    (lane >> 4) * 8]);
            acc[0][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf, x0, acc[0][nb], 0, 0, 0);
            acc[1][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf, x1, acc[1][nb], 0, 0, 0);
          }
        }
      }
    }

    // D: row = channel nb*16 + (lane>>4)*4 + reg, col = pixel lane&15
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int p = (2 * wid + m) * ST_TW + (lane & 15);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        if (nb < nnb) {
          uint2 v;
          v.x = (unsigned)f2bf(acc[m][nb][0]) |
                ((unsigned)f2bf(acc[m][nb][1]) << 16);
          v.y = (unsigned)f2bf(acc[m][nb][2]) |
                ((unsigned)f2bf(acc[m][nb][3]) << 16);
          *reinterpret_cast<uint2*>(
              &ot[p * ST_OPITCH + nb * 16 + (lane >> 4) * 4]) = v;
        }
      }
    }
    __syncthreads();

    // 16 B/lane stores: 8 lanes cover one pixel's 64 channels
#pragma unroll
    for (int it = 0; it < ST_TP * 8 / ST_THREADS; ++it) {
      const int idx = it * ST_THREADS + tid;
      const int p = idx >> 3, c8 = idx & 7;
      const int oh = t.oh0 + (p >> 4), ow = t.ow0 + (p & 15);
      if (oh < q.OH && ow < q.OW && c8 * 8 < kcnt) {
        const uint4 v =
            *reinterpret_cast<const uint4*>(&ot[p * ST_OPITCH + c8 * 8]);
        unsigned short* dst =
            q.y + (((long)t.n * q.OH + oh) * q.OW + ow) * q.K + k0 + c8 * 8;
        *reinterpret_cast<uint4*>(dst) = v;
      }
    }
    // the next tile's patch writes are ordered behind this tile's gathers
    // by the barrier above; its epilogue writes behind these reads by the
    // barrier after its patch load
  }
}

// ---------------------------------------------------------------------
// weight-grad
__global__ __launch_bounds__(ST_THREADS, 2)
void conv_stem_wgrad_kernel(StemParams q) {
  __shared__ __attribute__((aligned(16))) unsigned short patch[ST_PATCH];
  __shared__ __attribute__((aligned(16)))
      unsigned short dyt[ST_KT * ST_DPITCH];   // [k][pixel]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int kt = blockIdx.x % q.nkt;
  const int chunk = blockIdx.x / q.nkt;
  const int k0 = kt * ST_KT;
  const int kcnt = min(q.K - k0, ST_KT);
  const int nnb = (kcnt + 15) >> 4;
  const int ncb = (q.Kd + 15) >> 4;     // 16-wide kd column blocks

  // this wave's column blocks cb = wid + 4*i; lane's kd = cb*16 + lane&15
  int boff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    boff[i] = kd_offset(q, (wid + 4 * i) * 16 + (lane & 15));

  const int sC = q.stride * q.C;
  // MFMA k index 8*(lane>>4)+j of step ks is tile pixel
  // (row 2*ks + (lane>>5), col 8*((lane>>4)&1) + j)
  const int pix0 = (lane >> 5) * q.stride * q.pitch + 8 * ((lane >> 4) & 1) * sC;

  f32x4 acc[4][4];   // [k block][col block i]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[a][i] = {0.f, 0.f, 0.f, 0.f};

  for (long sp = chunk; sp < q.nsp; sp += q.chunks) {
    const TileCoord t = tile_coord(q, sp);
    const int sh = load_patch(q, t, patch, tid);
    // dy tile -> LDS transposed; invalid pixels / channels are zeros
#pragma unroll
    for (int it = 0; it < ST_TP * 8 / ST_THREADS; ++it) {
      const int idx = it * ST_THREADS + tid;
      const int p = idx >> 3, c8 = idx & 7;
      const int oh = t.oh0 + (p >> 4), ow = t.ow0 + (p & 15);
      uint4 v = {0u, 0u, 0u, 0u};
      if (oh < q.OH && ow < q.OW && c8 * 8 < kcnt)
        v = *reinterpret_cast<const uint4*>(
            q.dy + (((long)t.n * q.OH + oh) * q.OW + ow) * q.K + k0 + c8 * 8);
      unsigned short* d = &dyt[(c8 * 8) * ST_DPITCH + p];
      d[0 * ST_DPITCH] = (unsigned short)(v.x & 0xffffu);
      d[1 * ST_DPITCH] = (unsigned short)(v.x >> 16);
      d[2 * ST_DPITCH] = (unsigned short)(v.y & 0xffffu);
      d[3 * ST_DPITCH] = (unsigned short)(v.y >> 16);
      d[4 * ST_DPITCH] = (unsigned short)(v.z & 0xffffu);
      d[5 * ST_DPITCH] = (unsigned short)(v.z >> 16);
      d[6 * ST_DPITCH] = (unsigned short)(v.w & 0xffffu);
      d[7 * ST_DPITCH] = (unsigned short)(v.w >> 16);
    }
    __syncthreads();

#pragma unroll
    for (int ks = 0; ks < ST_TP / 32; ++ks) {
      const unsigned short* pp =
          patch + sh + pix0 + (2 * ks) * q.stride * q.pitch;
      bf16x8 bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (wid + 4 * i < ncb) {
#pragma unroll
          for (int j = 0; j < 8; ++j) bf[i][j] = (short)pp[j * sC + boff[i]];
        }
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (a < nnb) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(
              &dyt[(a * 16 + (lane & 15)) * ST_DPITCH + ks * 32 +
                   (lane >> 4) * 8]);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (wid + 4 * i < ncb)
              acc[a][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  af, bf[i], acc[a][i], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // partial slab [chunk][K][Kd]: row = k, col = kd
  float* out = q.part + (long)chunk * q.K * q.Kd;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int k = a * 16 + (lane >> 4) * 4 + reg;
      if (k >= kcnt) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kd = (wid + 4 * i) * 16 + (lane & 15);
        if (kd < q.Kd) out[(long)(k0 + k) * q.Kd + kd] = acc[a][i][reg];
      }
    }
  }
}

// dw[i] = sum over slabs in a fixed order: 8 slab groups x 32 elements per
// block, each thread sums its group's slabs ascending, then the 8 group
// sums are added ascending.
__global__ __launch_bounds__(256)
void stem_combine_kernel(const float* __restrict__ part,
                         float* __restrict__ dw, int total, int chunks) {
  __shared__ float red[8][32];
  const int e = threadIdx.x & 31;
  const int g = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + e;
  float s = 0.f;
  if (i < total)
    for (int c = g; c < chunks; c += 8) s += part[(long)c * total + i];
  red[g][e] = s;
  __syncthreads();
  if (g == 0 && i < total) {
    float r = red[0][e];
#pragma unroll
    for (int k = 1; k < 8; ++k) r += red[k][e];
    dw[i] = r;
  }
}

void fill_geometry(StemParams& q, long max_blocks) {
  q.Kd = q.R * q.R * q.C;
  q.nks = (q.Kd + 31) / 32;
  q.SC = q.R * q.C;
  q.Lrow = ((ST_TW - 1) * q.stride + q.R) * q.C;
  // pitch parity == (W*C) parity keeps LDS and global pair alignment in
  // step from row to row; +4 keeps rows' covering pairs disjoint
  q.pitch = q.Lrow + 4 + ((q.Lrow + q.W * q.C) & 1);
  q.PH = (ST_TH - 1) * q.stride + q.R;
  q.PPR = (q.Lrow + 1) / 2 + 1;
  if (q.Kd > ST_MAXKDP || q.PH * q.pitch + 2 > ST_PATCH)
    throw std::runtime_error("conv_stem: shape exceeds the LDS patch");
  q.tiles_h = (q.OH + ST_TH - 1) / ST_TH;
  q.tiles_w = (q.OW + ST_TW - 1) / ST_TW;
  q.nkt = (q.K + ST_KT - 1) / ST_KT;
  q.nsp = (long)q.N * q.tiles_h * q.tiles_w;
  q.chunks = (int)i64max(i64min(q.nsp, max_blocks / q.nkt), 1);
}

}  // namespace

// blocks per K tile the wgrad launch will use (= partial slabs)
int ddlb::conv_stem_wgrad_chunks(int N, int OH, int OW, int K) {
  const long nsp = (long)N * ((OH + ST_TH - 1) / ST_TH) *
                   ((OW + ST_TW - 1) / ST_TW);
  const int nkt = (K + ST_KT - 1) / ST_KT;
  return (int)i64max(i64min(nsp, 512 / nkt), 1);
}

void ddlb::launch_conv_stem_fwd(const void* x, const void* w, void* y, int N,
                                int H, int W, int C, int K, int OH, int OW,
                                int R, int stride, int pad,
                                hipStream_t stream) {
  StemParams q = {};
  q.x = (const unsigned short*)x;
  q.w = (const unsigned short*)w;
  q.y = (unsigned short*)y;
  q.N = N; q.H = H; q.W = W; q.C = C; q.K = K; q.OH = OH; q.OW = OW;
  q.R = R; q.stride = stride; q.pad = pad;
  fill_geometry(q, 512);
  hipLaunchKernelGGL(conv_stem_fwd_kernel, dim3(q.chunks * q.nkt),
                     dim3(ST_THREADS), 0, stream, q);
  HIP_CHECK_LAST();
}

void ddlb::launch_conv_stem_wgrad(const void* x, const void* dy, float* dw,
                                  float* part, int N, int H, int W, int C,
                                  int K, int OH, int OW, int R, int stride,
                                  int pad, hipStream_t stream) {
  StemParams q = {};
  q.x = (const unsigned short*)x;
  q.dy = (const unsigned short*)dy;
  q.part = part;
  q.N = N; q.H = H; q.W = W; q.C = C; q.K = K; q.OH = OH; q.OW = OW;
  q.R = R; q.stride = stride; q.pad = pad;
  fill_geometry(q, 512);
  hipLaunchKernelGGL(conv_stem_wgrad_kernel, dim3(q.chunks * q.nkt),
                     dim3(ST_THREADS), 0, stream, q);
  const int total = K * q.Kd;
  hipLaunchKernelGGL(stem_combine_kernel, dim3((total + 31) / 32), dim3(256),
                     0, stream, part, dw, total, q.chunks);
  HIP_CHECK_LAST();
}
