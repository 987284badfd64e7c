// NHWC bf16 average pooling, forward + backward (gfx950).
//
// Windowed pool, (k, stride, pad) in {(3,1,1), (3,2,1), (2,2,0)}, PyTorch's
// defaults (count_include_pad, no ceil_mode): the divisor is the constant
// k*k and padding adds zeros. Global pool: adaptive_avg_pool2d(x, 1).
// bf16 in and out, fp32 accumulation, one rounding. Channels travel in
// vectors of V = 8 (16 B) when C % 8 == 0, else of V = 4 (8 B). No atomics,
// no memset, no workspace; every sum has one fixed order.
//
// Windowed forward (avgpool_win_kernel). The k x k box sum is separable: a
// thread owns one channel vector of one output column, walks down its strip
// of output rows and keeps the horizontal k-tap sums of the last k input
// rows in an fp32 register ring, so each input row's horizontal sum is
// formed once and feeds every output row it belongs to (three at stride 1).
// Threads run channel-fastest, then along W: one tap of a wave is one
// contiguous NHWC segment of an input row. Horizontal neighbours overlap by
// k - 1 pixels; that overlap is left to L1 (the k tap loads of a wave cover
// the same segment shifted by one pixel, issued back to back), so the row
// walk has no barrier and no LDS and the loads of several rows stay in
// flight. A tile is th output rows x tw output columns x one channel chunk
// of one image; blocks take tiles grid-stride in an XCD-contiguous order,
// W tiles then H tiles innermost, so tiles that share a halo share an L2.
//
// Windowed backward. (3,1,1) is self-adjoint (same divisor everywhere, dx
// has dy's extent): dx is the forward kernel applied to dy. Stride 2 is the
// gather form (avgpool_s2_bwd_kernel), one pass over dx on the same tiling:
// an input pixel sums the dy of the at most 2 x 2 windows that cover it —
// again separably, the horizontal sum of a dy row is formed once per thread
// and reused for the up to three dx rows it feeds — and every dx element is
// written exactly once (0 where no window covers it).
//
// Global forward: lanes run over channel vectors; gap_split_kernel also
// splits the pixel axis over the threads of a block (interleaved, so a
// wave still reads contiguous segments) and combines the partials through
// LDS in slice order; gap_flat_kernel gives every (image, channel vector)
// one thread. global_avgpool_plan chooses. Global backward is one write
// pass with dy hoisted per thread.

#include "common.h"
#include "launchers.h"
#include "mfma_common.h"
#include <stdexcept>
#include <string>

namespace {

template <int V> struct ChanVec;
template <> struct ChanVec<8> {
  typedef __attribute__((ext_vector_type(8))) short T;
};
template <> struct ChanVec<4> {
  typedef __attribute__((ext_vector_type(4))) short T;
};

DEV float bf2f(short v) {
  return __uint_as_float(((unsigned)(unsigned short)v) << 16);
}

DEV short f2bf(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  unsigned short u;
  __builtin_memcpy(&u, &h, 2);
  return (short)u;
}

template <int V> DEV void zero(float (&a)[V]) {
#pragma unroll
  for (int j = 0; j < V; ++j) a[j] = 0.f;
}

// a += the V bf16 channels at p
template <int V> DEV void add_vec(float (&a)[V], const short* p) {
  const typename ChanVec<V>::T v =
      *reinterpret_cast<const typename ChanVec<V>::T*>(p);
#pragma unroll
  for (int j = 0; j < V; ++j) a[j] += bf2f(v[j]);
}

// *p = bf16(a * scale), one rounding
template <int V> DEV void store_vec(short* p, const float (&a)[V],
                                    float scale) {
  typename ChanVec<V>::T v;
#pragma unroll
  for (int j = 0; j < V; ++j) v[j] = f2bf(a[j] * scale);
  *reinterpret_cast<typename ChanVec<V>::T*>(p) = v;
}

// Device image of an AvgWinPlan: rh x rw is the tensor the kernel reads,
// wh x ww the one it writes and tiles.
struct WinParams {
  int C, CV, rh, rw, wh, ww;
  int cvb, nct, tw, th, tiles_w, tiles_h;
  int tiles;
  float scale;
};

// One tile's thread coordinates; false for a thread with nothing to write.
struct WinThread {
  long n;
  int cv, col, row0, row1;
};
DEV bool win_thread(const WinParams& p, int tile, WinThread& t) {
  const int ct = tile % p.nct;
  tile /= p.nct;
  const int twi = tile % p.tiles_w;
  tile /= p.tiles_w;
  const int thi = tile % p.tiles_h;
  t.n = tile / p.tiles_h;
  const int cvl = threadIdx.x % p.cvb, cl = threadIdx.x / p.cvb;
  t.cv = ct * p.cvb + cvl;
  t.col = twi * p.tw + cl;
  t.row0 = thi * p.th;
  t.row1 = min(t.row0 + p.th, p.wh);
  return cl < p.tw && t.cv < p.CV && t.col < p.ww;
}

template <int V, int K, int S>
__global__ __launch_bounds__(256) void avgpool_win_kernel(
    const short* __restrict__ x, short* __restrict__ y, const WinParams p) {
  constexpr int P = K == 3 ? 1 : 0;
  for (int tile = xcd_remap(blockIdx.x, gridDim.x); tile < p.tiles;
       tile += gridDim.x) {
    WinThread t;
    if (!win_thread(p, tile, t)) continue;
    const int iw0 = t.col * S - P;
    const short* xc = x + t.n * p.rh * p.rw * p.C + (long)t.cv * V;
    short* yc = y + (t.n * p.wh * p.ww + t.col) * p.C + (long)t.cv * V;
    // horizontal K-tap sum of input row ih, left to right; zeros outside
    auto hrow = [&](int ih, float (&r)[V]) {
      zero<V>(r);
      if (ih < 0 || ih >= p.rh) return;
      const short* row = xc + (long)ih * p.rw * p.C;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int iw = iw0 + k;
        if (iw >= 0 && iw < p.rw) add_vec<V>(r, row + (long)iw * p.C);
      }
    };
    // ring[j] is window row j of the current output row; K - S of them
    // carry over to the next output row
    float ring[K][V];
#pragma unroll
    for (int j = 0; j < K - S; ++j) hrow(t.row0 * S - P + j, ring[j + S]);
    for (int oh = t.row0; oh < t.row1; ++oh) {
#pragma unroll
      for (int j = 0; j < K - S; ++j)
#pragma unroll
        for (int v = 0; v < V; ++v) ring[j][v] = ring[j + S][v];
#pragma unroll
      for (int j = K - S; j < K; ++j) hrow(oh * S - P + j, ring[j]);
      float acc[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        acc[v] = ring[0][v];
#pragma unroll
        for (int j = 1; j < K; ++j) acc[v] += ring[j][v];
      }
      store_vec<V>(yc + (long)oh * p.ww * p.C, acc, p.scale);
    }
  }
}

// Stride-2 backward, gather form: the thread owns dx column iw and walks dx
// rows; dy is rh x rw, dx wh x ww. Window o covers pixel i when
// o*2 - P <= i <= o*2 - P + K - 1.
template <int V, int K>
__global__ __launch_bounds__(256) void avgpool_s2_bwd_kernel(
    const short* __restrict__ dy, short* __restrict__ dx,
    const WinParams p) {
  constexpr int S = 2, P = K == 3 ? 1 : 0;
  for (int tile = xcd_remap(blockIdx.x, gridDim.x); tile < p.tiles;
       tile += gridDim.x) {
    WinThread t;
    if (!win_thread(p, tile, t)) continue;
    const int ow_lo = (t.col + P - K + S) / S;
    const int ow_hi = min(p.rw - 1, (t.col + P) / S);
    const short* dyc = dy + t.n * p.rh * p.rw * p.C + (long)t.cv * V;
    short* dxc = dx + (t.n * p.wh * p.ww + t.col) * p.C + (long)t.cv * V;
    // sum of dy row oh over the windows that cover column iw
    auto grow = [&](int oh, float (&g)[V]) {
      zero<V>(g);
      const short* row = dyc + (long)oh * p.rw * p.C;
      for (int ow = ow_lo; ow <= ow_hi; ++ow)
        add_vec<V>(g, row + (long)ow * p.C);
    };
    float g[V];
    int have = -1;  // the dy row g holds
    for (int ih = t.row0; ih < t.row1; ++ih) {
      const int oh_lo = (ih + P - K + S) / S;
      const int oh_hi = min(p.rh - 1, (ih + P) / S);
      float acc[V];
      zero<V>(acc);
      if (oh_lo <= oh_hi) {
        if (have != oh_lo) grow(oh_lo, g);
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = g[v];
        have = oh_lo;
        if (oh_hi > oh_lo) {
          grow(oh_hi, g);
          have = oh_hi;
#pragma unroll
          for (int v = 0; v < V; ++v) acc[v] += g[v];
        }
      }
      store_vec<V>(dxc + (long)ih * p.ww * p.C, acc, p.scale);
    }
  }
}

// ---- global pool --------------------------------------------------------
struct GapParams {
  long N;
  int C, CV, HW;
  int cvb, nct, psplit;
  long items;  // split / backward: N * nct blocks of work; flat: N * CV
  float scale;
};

// A block item is one channel chunk of one image; thread (cvl, ps) sums
// pixels ps, ps + psplit, ... of its channel vector; slice 0 then adds the
// partials in slice order.
template <int V>
__global__ __launch_bounds__(256) void gap_split_kernel(
    const short* __restrict__ x, short* __restrict__ y, const GapParams p) {
  __shared__ float part[256 * V];
  const int cvl = threadIdx.x % p.cvb, ps = threadIdx.x / p.cvb;
  for (long item = blockIdx.x; item < p.items; item += gridDim.x) {
    const long n = item / p.nct;
    const int cv = (int)(item % p.nct) * p.cvb + cvl;
    const bool live = ps < p.psplit && cv < p.CV;
    float acc[V];
    zero<V>(acc);
    if (live) {
      const short* xc = x + n * p.HW * p.C + (long)cv * V;
      for (int px = ps; px < p.HW; px += p.psplit)
        add_vec<V>(acc, xc + (long)px * p.C);
#pragma unroll
      for (int v = 0; v < V; ++v) part[threadIdx.x * V + v] = acc[v];
    }
    __syncthreads();
    if (live && ps == 0) {
      for (int s = 1; s < p.psplit; ++s)
#pragma unroll
        for (int v = 0; v < V; ++v)
          acc[v] += part[(s * p.cvb + cvl) * V + v];
      store_vec<V>(y + n * p.C + (long)cv * V, acc, p.scale);
    }
    __syncthreads();
  }
}

// One thread per (image, channel vector), pixels in order.
template <int V>
__global__ __launch_bounds__(256) void gap_flat_kernel(
    const short* __restrict__ x, short* __restrict__ y, const GapParams p) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < p.items;
       i += (long)gridDim.x * blockDim.x) {
    const long n = i / p.CV;
    const int cv = (int)(i % p.CV);
    const short* xc = x + n * p.HW * p.C + (long)cv * V;
    float acc[V];
    zero<V>(acc);
    for (int px = 0; px < p.HW; ++px) add_vec<V>(acc, xc + (long)px * p.C);
    store_vec<V>(y + n * p.C + (long)cv * V, acc, p.scale);
  }
}

// dx[n, px, c] = dy[n, c] / HW: the dy vector is scaled and rounded once
// per thread, then stored to pixels ps, ps + psplit, ...
template <int V>
__global__ __launch_bounds__(256) void gap_bwd_kernel(
    const short* __restrict__ dy, short* __restrict__ dx,
    const GapParams p) {
  const int cvl = threadIdx.x % p.cvb, ps = threadIdx.x / p.cvb;
  if (ps >= p.psplit) return;
  for (long item = blockIdx.x; item < p.items; item += gridDim.x) {
    const long n = item / p.nct;
    const int cv = (int)(item % p.nct) * p.cvb + cvl;
    if (cv >= p.CV) continue;
    float g[V];
    zero<V>(g);
    add_vec<V>(g, dy + n * p.C + (long)cv * V);
    typename ChanVec<V>::T out;
#pragma unroll
    for (int v = 0; v < V; ++v) out[v] = f2bf(g[v] * p.scale);
    short* dxc = dx + n * p.HW * p.C + (long)cv * V;
    for (int px = ps; px < p.HW; px += p.psplit)
      *reinterpret_cast<typename ChanVec<V>::T*>(dxc + (long)px * p.C) = out;
  }
}

constexpr int kThreads = 256;
// windowed tiling
constexpr int kWinMaxTw = 64;        // output columns per tile
constexpr int kWinMinTh = 8;         // rows per tile: halo rows <= 2 in 8
constexpr long kWinTargetTiles = 2048;  // 256 CUs x 8 resident blocks
constexpr int kWinMinRows = 16;      // rows a block walks before it retires
constexpr int kMaxBlocks = 2048;
// global pool
constexpr int kGapMaxCvb = 32;       // 32 lanes x 16 B: 512-B row segments
constexpr int kGapSplitPixels = 64;  // split the pixel axis from here on
constexpr int kGapMinSplitPixels = 16;  // ... or from here on when
constexpr long kGapFillVectors = 32768;  // N * C / V leaves the CUs idle

int chan_vec(int C) {
  if (C % 8 == 0) return 8;
  if (C % 4 == 0) return 4;
  throw std::runtime_error("avgpool needs C % 4 == 0");
}

WinParams win_params(const ddlb::AvgWinPlan& pl, int C, int rh, int rw,
                     int wh, int ww, float scale) {
  WinParams p;
  p.C = C;
  p.CV = C / pl.V;
  p.rh = rh;
  p.rw = rw;
  p.wh = wh;
  p.ww = ww;
  p.cvb = pl.cvb;
  p.nct = pl.nct;
  p.tw = pl.tw;
  p.th = pl.th;
  p.tiles_w = pl.tiles_w;
  p.tiles_h = pl.tiles_h;
  p.tiles = (int)pl.tiles;
  p.scale = scale;
  return p;
}

template <int V>
void launch_win(const ddlb::AvgWinPlan& pl, const WinParams& p, int k,
                int stride, bool gather, const short* in, short* out,
                hipStream_t stream) {
  const dim3 grid(pl.blocks), block(kThreads);
  if (gather && k == 3)
    hipLaunchKernelGGL((avgpool_s2_bwd_kernel<V, 3>), grid, block, 0, stream,
                       in, out, p);
  else if (gather)
    hipLaunchKernelGGL((avgpool_s2_bwd_kernel<V, 2>), grid, block, 0, stream,
                       in, out, p);
  else if (k == 3 && stride == 1)
    hipLaunchKernelGGL((avgpool_win_kernel<V, 3, 1>), grid, block, 0, stream,
                       in, out, p);
  else if (k == 3)
    hipLaunchKernelGGL((avgpool_win_kernel<V, 3, 2>), grid, block, 0, stream,
                       in, out, p);
  else
    hipLaunchKernelGGL((avgpool_win_kernel<V, 2, 2>), grid, block, 0, stream,
                       in, out, p);
  HIP_CHECK_LAST();
}

void check_window(int k, int stride, int pad) {
  if (!((k == 3 && stride == 1 && pad == 1) ||
        (k == 3 && stride == 2 && pad == 1) ||
        (k == 2 && stride == 2 && pad == 0)))
    throw std::runtime_error(
        "avgpool supports (k, stride, pad) in {(3,1,1), (3,2,1), (2,2,0)}");
}

GapParams gap_params(const ddlb::GapPlan& pl, long N, int C, int HW) {
  GapParams p;
  p.N = N;
  p.C = C;
  p.CV = C / pl.V;
  p.HW = HW;
  p.cvb = pl.cvb;
  p.nct = pl.nct;
  p.psplit = pl.psplit;
  p.items = pl.split ? N * pl.nct : N * p.CV;
  p.scale = 1.0f / (float)HW;
  return p;
}

}  // namespace

ddlb::AvgWinPlan ddlb::avgpool_win_plan(int N, int C, int WH, int WW) {
  AvgWinPlan pl;
  pl.V = chan_vec(C);
  const int CV = C / pl.V;
  pl.cvb = CV < kThreads ? CV : kThreads;
  pl.nct = (CV + pl.cvb - 1) / pl.cvb;
  pl.tw = kThreads / pl.cvb;
  if (pl.tw > kWinMaxTw) pl.tw = kWinMaxTw;
  if (pl.tw > WW) pl.tw = WW;
  pl.tiles_w = (WW + pl.tw - 1) / pl.tw;
  // whole columns first (no halo rows read twice); halve the strip while
  // the grid would leave CUs idle
  pl.th = WH;
  auto tiles = [&](int th) {
    return (long)N * ((WH + th - 1) / th) * pl.tiles_w * pl.nct;
  };
  while (tiles(pl.th) < kWinTargetTiles && (pl.th + 1) / 2 >= kWinMinTh)
    pl.th = (pl.th + 1) / 2;
  pl.tiles_h = (WH + pl.th - 1) / pl.th;
  pl.tiles = tiles(pl.th);
  if (pl.tiles >= (1L << 31) || (long)N * WH * WW * C >= (1L << 40))
    throw std::runtime_error("avgpool: problem too large");
  const int per = pl.th >= kWinMinRows ? 1 : kWinMinRows / pl.th;
  const long blocks = (pl.tiles + per - 1) / per;
  pl.blocks = (int)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
  return pl;
}

void ddlb::launch_avgpool_fwd(const void* x, void* y, int N, int C, int H,
                              int W, int k, int stride, int pad,
                              hipStream_t stream) {
  check_window(k, stride, pad);
  const int OH = (H + 2 * pad - k) / stride + 1;
  const int OW = (W + 2 * pad - k) / stride + 1;
  const AvgWinPlan pl = avgpool_win_plan(N, C, OH, OW);
  const WinParams p = win_params(pl, C, H, W, OH, OW, 1.0f / (float)(k * k));
  if (pl.V == 8)
    launch_win<8>(pl, p, k, stride, false, (const short*)x, (short*)y,
                  stream);
  else
    launch_win<4>(pl, p, k, stride, false, (const short*)x, (short*)y,
                  stream);
}

void ddlb::launch_avgpool_bwd(const void* dy, void* dx, int N, int C, int H,
                              int W, int k, int stride, int pad,
                              hipStream_t stream) {
  check_window(k, stride, pad);
  // (3,1,1) is self-adjoint: one divisor for every window and dx of dy's
  // extent, so dx is the forward pool of dy
  if (stride == 1) {
    launch_avgpool_fwd(dy, dx, N, C, H, W, k, stride, pad, stream);
    return;
  }
  const int OH = (H + 2 * pad - k) / stride + 1;
  const int OW = (W + 2 * pad - k) / stride + 1;
  const AvgWinPlan pl = avgpool_win_plan(N, C, H, W);
  const WinParams p = win_params(pl, C, OH, OW, H, W, 1.0f / (float)(k * k));
  if (pl.V == 8)
    launch_win<8>(pl, p, k, stride, true, (const short*)dy, (short*)dx,
                  stream);
  else
    launch_win<4>(pl, p, k, stride, true, (const short*)dy, (short*)dx,
                  stream);
}

ddlb::GapPlan ddlb::global_avgpool_plan(long N, int C, int HW) {
  GapPlan pl;
  pl.V = chan_vec(C);
  const int CV = C / pl.V;
  if (N * (long)HW * C >= (1L << 40))
    throw std::runtime_error("avgpool: problem too large");
  pl.cvb = CV < kGapMaxCvb ? CV : kGapMaxCvb;
  pl.nct = (CV + pl.cvb - 1) / pl.cvb;
  pl.psplit = kThreads / pl.cvb;
  if (pl.psplit > HW) pl.psplit = HW;
  pl.split = HW >= kGapSplitPixels ||
             (N * CV < kGapFillVectors && HW >= kGapMinSplitPixels);
  const long split_items = N * pl.nct;
  const long fwd = pl.split ? split_items : (N * CV + kThreads - 1) / kThreads;
  pl.fwd_blocks = (int)(fwd < kMaxBlocks ? fwd : kMaxBlocks);
  // the backward always runs on the (channel chunk, pixel slice) layout
  pl.bwd_blocks = (int)(split_items < 4 * kMaxBlocks ? split_items
                                                     : 4 * kMaxBlocks);
  return pl;
}

void ddlb::launch_global_avgpool_fwd(const void* x, void* y, long N, int C,
                                     int HW, hipStream_t stream) {
  const GapPlan pl = global_avgpool_plan(N, C, HW);
  const GapParams p = gap_params(pl, N, C, HW);
  const dim3 grid(pl.fwd_blocks), block(kThreads);
  const short* in = (const short*)x;
  short* out = (short*)y;
  if (pl.split && pl.V == 8)
    hipLaunchKernelGGL(gap_split_kernel<8>, grid, block, 0, stream, in, out,
                       p);
  else if (pl.split)
    hipLaunchKernelGGL(gap_split_kernel<4>, grid, block, 0, stream, in, out,
                       p);
  else if (pl.V == 8)
    hipLaunchKernelGGL(gap_flat_kernel<8>, grid, block, 0, stream, in, out,
                       p);
  else
    hipLaunchKernelGGL(gap_flat_kernel<4>, grid, block, 0, stream, in, out,
                       p);
  HIP_CHECK_LAST();
}

void ddlb::launch_global_avgpool_bwd(const void* dy, void* dx, long N, int C,
                                     int HW, hipStream_t stream) {
  GapPlan pl = global_avgpool_plan(N, C, HW);
  pl.split = 1;  // items = N * nct
  const GapParams p = gap_params(pl, N, C, HW);
  const dim3 grid(pl.bwd_blocks), block(kThreads);
  if (pl.V == 8)
    hipLaunchKernelGGL(gap_bwd_kernel<8>, grid, block, 0, stream,
                       (const short*)dy, (short*)dx, p);
  else
    hipLaunchKernelGGL(gap_bwd_kernel<4>, grid, block, 0, stream,
                       (const short*)dy, (short*)dx, p);
  HIP_CHECK_LAST();
}
