// bf16 Linear on MFMA (gfx950): y = x W^T + b and both gradients, fp32
// accumulation on v_mfma_f32_16x16x32_bf16.
//
// x (M, K), W (N, K), y / dy (M, N), all row-major. Every direction is one
// GEMM  C[i][j] = sum_r A(i, r) * B(j, r)  over an (I, J) output and a
// reduction of length R; what differs is how each operand lies in memory:
//
//            C      I  J  R   A(i, r)        B(j, r)
//   fwd   y  (NT)   M  N  K   x[i][r]  row   W[j][r]  row
//   dgrad dx (NN)   M  K  N   dy[i][r] row   W[r][j]  tr
//   wgrad dW (TN)   N  K  M   dy[r][i] tr    x[r][j]  tr
//
//   * "row": the reduction axis is contiguous, so a lane's MFMA fragment
//     is one 16-byte chunk. A 64-deep step is two k-halves of [T][32]
//     bf16; the chunk at (row, slot s) holds logical chunk
//     s ^ sigma((row >> 2) & 3), sigma = [0,2,3,1] (the swizzle
//     conv_mfma2.hip documents): glds writes lane-linear, the XOR goes on
//     the SOURCE chunk index and is re-applied on the ds_read_b128.
//   * "tr": the operand is reduction-major (transposed from the fragment
//     layout). It is staged as a ds_read_b64_tr_b16 image, T/16 column
//     groups x two r-parity sub-images of [64/8][4][16] halfwords, and
//     fragments come out of the hardware transpose read (the image
//     conv_wgrad.hip uses, re-stated here). W is read in place by the
//     data-grad: no transposed copy exists anywhere.
//   * Both kinds are T*8 16-byte glds chunks per step, so one staging
//     loop, one ring and one vmcnt count serve all three kernels.
//   * Tiles: 128x128 (512 threads, waves 2x4, 2-buffer ring, 64 KiB, two
//     blocks per CU overlap each other) and 64x64 (256 threads, waves 2x2,
//     3-buffer ring staged two steps ahead, 48 KiB). Counted s_waitcnt
//     vmcnt and raw s_barrier: never __syncthreads with glds in flight.
//   * fwd / dgrad: no split, bias added in the fp32 accumulator, one
//     rounding to bf16, the same bits on every call.
//   * wgrad: the m range is cut into `split` slabs when the (N, K) tile
//     grid cannot fill the CUs; each slab writes an fp32 partial and an
//     ordered combine adds them in slab order and rounds once. No atomics,
//     no memset. db rides along: the blocks of the first K-tile column sum
//     the dy image they have staged anyway (4 threads per column, 16 rows
//     each per step) into a [split][N] slab the same combine reduces.
//
// Edges: an out-of-range chunk (output-tile tail or reduction tail) is
// redirected to a zero page, so it contributes exactly 0 and no load
// leaves the tensors; tail accumulators are never stored. K % 8 == 0 and
// N % 8 == 0 keep every chunk whole and aligned; M is arbitrary. Offsets
// are 32-bit: the launchers refuse operands of 2^31 elements or more.

#include "mfma_common.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <string>

using bf16 = __hip_bfloat16;
typedef __attribute__((address_space(3))) const short* lds_cptr;

#define LIN_BK 64  // reduction depth of one step

struct LinParams {
  const bf16* a;
  const bf16* b;
  const bf16* zero;   // 16-byte zero page
  bf16* out;          // (I, J) bf16, written when split == 1
  float* part;        // [split][I][J] fp32 slabs (split > 1)
  const void* bias;   // fwd: [J] bf16 or fp32, nullptr = none
  void* db;           // wgrad, split == 1: [I] in the bias dtype
  float* dbpart;      // wgrad, split > 1: [split][I]
  int bias_f32;       // dtype of bias / db
  int want_db;
  int I, J, R;
  int split, r_per;   // wgrad: slabs and reduction rows per slab
};

namespace {

// sigma = [0,2,3,1]: stored slot s holds logical chunk s ^ sigma(rb)
DEV int sigma4(int x) { return (0x1320 >> (x * 4)) & 0xF; }

// tr image (per operand, per buffer): column group g of 16, r-parity
// half, then [r/8][4][16] halfword blocks:
//   half(r, c) = (c >> 4) * 1024 + ((r >> 2) & 1) * 512 + (r >> 3) * 64
//                + (r & 3) * 16 + (c & 15)
// The 16-byte staging chunk d covers (r, c0 .. c0 + 7):
DEV void tr_decode_chunk(int d, int& r, int& c0) {
  const int g = d >> 7;
  const int q = d & 127;
  const int q2 = q & 63;
  r = (q2 >> 3) * 8 + (q >> 6) * 4 + ((q2 >> 1) & 3);
  c0 = g * 16 + (q2 & 1) * 8;
}

DEV int tr_half(int r, int c) {
  return (c >> 4) * (LIN_BK * 16) + ((r >> 2) & 1) * (LIN_BK * 8) +
         (r >> 3) * 64 + (r & 3) * 16 + (c & 15);
}

// fragment (column = lane & 15 of group, r = ks*32 + (lane >> 4)*8 + e):
// two transpose reads (the r-parity halves) at lane-linear 8-B addresses
DEV bf16x8 tr_frag(const short* img, int group, int ks, int lane) {
  bf16x4 lo, hi;
  lds_cptr base = (lds_cptr)(img + group * (LIN_BK * 16) + ks * 4 * 64 +
                             lane * 4);
  asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
               "ds_read_b64_tr_b16 %1, %2 offset:%3"
               : "=&v"(lo), "=&v"(hi)
               : "v"(base), "i"(LIN_BK * 8 * 2));
  bf16x8 f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[e] = lo[e];
    f[4 + e] = hi[e];
  }
  return f;
}

DEV float bf16_bits_to_f32(short v) {
  return __uint_as_float((unsigned)(unsigned short)v << 16);
}

// One operand's staging state: G chunks per thread per step. `t0` is the
// tile's first row/column, E the operand's extent along it, ld its leading
// dimension, [r_begin, r_end) the reduction range of this block.
template <int T, int TPB, bool TR>
struct Stager {
  static constexpr int G = T * 8 / TPB;
  static_assert(G >= 1 && G * TPB == T * 8, "tile vs threads");
  unsigned off[G];  // element offset of the chunk at step 0
  int r0[G];        // its reduction index at step 0
  bool ok[G];       // its row/column lies inside the operand

  DEV void init(int tid, int t0, int E, int ld, int r_begin) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int d = j * TPB + tid;
      if (TR) {
        int r, c0;
        tr_decode_chunk(d, r, c0);
        r0[j] = r_begin + r;
        ok[j] = t0 + c0 < E;
        off[j] = (unsigned)r0[j] * (unsigned)ld + (unsigned)(t0 + c0);
      } else {
        const int kh = d / (T * 4);
        const int ca = d % (T * 4);
        const int row = ca >> 2;
        const int cg = (ca & 3) ^ sigma4((ca >> 4) & 3);
        r0[j] = r_begin + kh * 32 + cg * 8;
        ok[j] = t0 + row < E;
        off[j] = (unsigned)(t0 + row) * (unsigned)ld + (unsigned)r0[j];
      }
    }
  }

  DEV void stage(const bf16* base, const bf16* zero, short* img, int tid,
                 int t, int ld, int r_end) const {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const unsigned adv = TR ? (unsigned)(t * LIN_BK) * (unsigned)ld
                              : (unsigned)(t * LIN_BK);
      const bf16* src = (ok[j] && r0[j] + t * LIN_BK < r_end)
                            ? base + (off[j] + adv)
                            : zero;
      glds16(src, img + (j * TPB + tid) * 8);
    }
  }
};

// T x T tile, WR x WC waves, NBUF-deep LDS ring. DB: sum the A image's
// columns (wgrad's dy) in the blocks of the first J tile.
template <int T, int TPB, int WR, int WC, int NBUF, bool A_TR, bool B_TR,
          bool DB>
DEV void linear_gemm(const LinParams& q) {
  constexpr int G = T * 8 / TPB;   // glds chunks per thread, operand, step
  constexpr int MFS = T / WR / 16; // A fragments per wave
  constexpr int NFS = T / WC / 16; // B fragments per wave
  static_assert(WR * WC == TPB / 64, "wave count");
  static_assert(NBUF == 2 || NBUF == 3, "ring depth");
  static_assert(!DB || TPB == 4 * T, "db: four threads per column");
  // ring: [buf][A T x 64 | B T x 64] bf16
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* lds = reinterpret_cast<short*>(smem);
  auto aimg = [&](int buf) { return lds + buf * LIN_BK * 2 * T; };
  auto bimg = [&](int buf) { return aimg(buf) + LIN_BK * T; };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int fr = lane & 15;
  const int fk = lane >> 4;

  const int ni = (q.I + T - 1) / T;
  const int nj = (q.J + T - 1) / T;
  const int block = xcd_remap(blockIdx.x, gridDim.x);
  const int jb = (block % nj) * T;
  const int ib = ((block / nj) % ni) * T;
  const int slab = block / (ni * nj);
  const int r_begin = slab * q.r_per;
  const int r_end = min(r_begin + q.r_per, q.R);
  const int nsteps = max((r_end - r_begin + LIN_BK - 1) / LIN_BK, 0);

  // leading dimensions: reduction-contiguous operands are (E, R),
  // reduction-major ones (R, E)
  const int lda = A_TR ? q.I : q.R;
  const int ldb = B_TR ? q.J : q.R;
  Stager<T, TPB, A_TR> sa;
  Stager<T, TPB, B_TR> sb;
  sa.init(tid, ib, q.I, lda, r_begin);
  sb.init(tid, jb, q.J, ldb, r_begin);
  auto stage = [&](int buf, int t) {
    sa.stage(q.a, q.zero, aimg(buf), tid, t, lda, r_end);
    sb.stage(q.b, q.zero, bimg(buf), tid, t, ldb, r_end);
  };

  const int wr = wid / WC;
  const int wc = wid % WC;
  // reduction-contiguous fragment: row fr of the 16, chunk fk un-swizzled
  const int fchunk = (fk ^ sigma4((fr >> 2) & 3)) * 8;
  auto frag = [&](const short* img, bool tr, int f, int ks) {
    if (tr) return tr_frag(img, f, ks, lane);
    return *reinterpret_cast<const bf16x8*>(img + ks * T * 32 +
                                            (f * 16 + fr) * 32 + fchunk);
  };

  f32x4 acc[MFS][NFS];
#pragma unroll
  for (int i = 0; i < MFS; ++i)
#pragma unroll
    for (int j = 0; j < NFS; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const bool do_db = DB && q.want_db && jb == 0;  // block-uniform
  const int dbc = tid % T;  // db: this thread's column and row quarter
  const int dbq = tid / T;
  float dbacc = 0.f;

  // ---- prologue ---------------------------------------------------------
  stage(0, 0);
  if (NBUF == 3 && nsteps > 1) {
    stage(1, 1);
    wait_vmcnt<2 * G>();  // step 0 landed, step 1 in flight
  } else {
    wait_vmcnt<0>();
  }
  __builtin_amdgcn_s_barrier();

  for (int t = 0; t < nsteps; ++t) {
    const short* la = aimg(t % NBUF);
    const short* lb = bimg(t % NBUF);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[MFS], bfr[NFS];
#pragma unroll
      for (int nf = 0; nf < NFS; ++nf)
        bfr[nf] = frag(lb, B_TR, wc * NFS + nf, ks);
#pragma unroll
      for (int mf = 0; mf < MFS; ++mf)
        af[mf] = frag(la, A_TR, wr * MFS + mf, ks);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);  // keep MFMAs behind the wait
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mf = 0; mf < MFS; ++mf)
#pragma unroll
        for (int nf = 0; nf < NFS; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mf], bfr[nf], acc[mf][nf], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    if (do_db) {
      // rows past r_end were staged from the zero page: they add 0
#pragma unroll
      for (int e = 0; e < 16; ++e)
        dbacc += bf16_bits_to_f32(la[tr_half(dbq * 16 + e, dbc)]);
    }
    if (NBUF == 2) {
      // stage t+1 behind this step's MFMAs, drain, swap: the overlap
      // comes from the co-resident second block
      if (t + 1 < nsteps) stage((t + 1) % 2, t + 1);
      wait_vmcnt<0>();
    } else if (t + 2 < nsteps) {
      stage((t + 2) % 3, t + 2);
      wait_vmcnt<2 * G>();
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
  }

  // ---- epilogue: bias in fp32, one rounding; or the fp32 slab -----------
  float* slab_out = q.part + (unsigned)slab * ((unsigned)q.I * (unsigned)q.J);
#pragma unroll
  for (int nf = 0; nf < NFS; ++nf) {
    const int col = jb + (wc * NFS + nf) * 16 + fr;
    if (col >= q.J) continue;
    float bv = 0.f;
    if (q.bias != nullptr)
      bv = q.bias_f32 ? ((const float*)q.bias)[col]
                      : to_f32(((const bf16*)q.bias)[col]);
#pragma unroll
    for (int mf = 0; mf < MFS; ++mf) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = ib + (wr * MFS + mf) * 16 + fk * 4 + reg;
        if (row >= q.I) continue;
        const unsigned o = (unsigned)row * (unsigned)q.J + (unsigned)col;
        if (q.split > 1)
          slab_out[o] = acc[mf][nf][reg];
        else
          q.out[o] = __float2bfloat16(acc[mf][nf][reg] + bv);
      }
    }
  }

  if (DB) {
    if (!do_db) return;
    // the loop's last barrier released the ring: reuse it for the four
    // quarter sums of each column, added in quarter order
    float* red = reinterpret_cast<float*>(smem);
    red[dbq * T + dbc] = dbacc;
    __syncthreads();
    const int n = ib + tid;
    if (tid >= T || n >= q.I) return;
    const float s = ((red[tid] + red[T + tid]) + red[2 * T + tid]) +
                    red[3 * T + tid];
    if (q.split > 1)
      q.dbpart[slab * q.I + n] = s;
    else if (q.bias_f32)
      ((float*)q.db)[n] = s;
    else
      ((bf16*)q.db)[n] = __float2bfloat16(s);
  }
}

// 128 tile: 512 threads on a 2-buffer ring; 64 tile: 256 threads on a
// 3-buffer ring
#define LIN_TILE_ARGS(T) T, (T == 128 ? 512 : 256), 2, (T == 128 ? 4 : 2), \
                         (T == 128 ? 2 : 3)

template <int T>
__global__ __launch_bounds__(T == 128 ? 512 : 256, T == 128 ? 4 : 2)
void linear_fwd_kernel(LinParams q) {
  linear_gemm<LIN_TILE_ARGS(T), false, false, false>(q);
}

template <int T>
__global__ __launch_bounds__(T == 128 ? 512 : 256, T == 128 ? 4 : 2)
void linear_dgrad_kernel(LinParams q) {
  linear_gemm<LIN_TILE_ARGS(T), false, true, false>(q);
}

template <int T>
__global__ __launch_bounds__(T == 128 ? 512 : 256, T == 128 ? 4 : 2)
void linear_wgrad_kernel(LinParams q) {
  linear_gemm<LIN_TILE_ARGS(T), true, true, true>(q);
}

// Ordered combine: dW element i = bf16(sum over slabs, in slab order);
// the threads past the dW vectors reduce the db slab the same way.
__global__ void linear_wgrad_combine_kernel(const float* __restrict__ part,
                                            bf16* __restrict__ dw, int total,
                                            const float* __restrict__ dbpart,
                                            void* __restrict__ db,
                                            int db_f32, int I, int split) {
  typedef __attribute__((ext_vector_type(4))) float float4x;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int nvec = total / 4;  // total % 8 == 0
  if (i < nvec) {
    float4x s = {0.f, 0.f, 0.f, 0.f};
    for (int ps = 0; ps < split; ++ps)
      s += *reinterpret_cast<const float4x*>(part + (size_t)ps * total +
                                             (size_t)i * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) dw[(size_t)i * 4 + j] = __float2bfloat16(s[j]);
    return;
  }
  const int n = i - nvec;
  if (db == nullptr || n >= I) return;
  float s = 0.f;
  for (int ps = 0; ps < split; ++ps) s += dbpart[ps * I + n];
  if (db_f32)
    ((float*)db)[n] = s;
  else
    ((bf16*)db)[n] = __float2bfloat16(s);
}

constexpr int kCUs = 256;  // MI355X

void check_extent(const char* what, long a, long b) {
  if (a * b >= (1L << 31))
    throw std::runtime_error(
        std::string("linear: ") + what +
        " has 2^31 elements or more (kernel offsets are 32-bit)");
}

ddlb::LinearDirPlan dir_plan(long I, long J, long R, bool wgrad) {
  ddlb::LinearDirPlan d;
  const long g128 = ((I + 127) / 128) * ((J + 127) / 128);
  // the 128 tile re-stages least, but only pays once its grid fills the
  // CUs; the weight-grad can split its reduction instead, so it takes the
  // big tile whenever both sides hold one
  const bool big = I >= 128 && J >= 128 && (wgrad || g128 >= kCUs);
  d.tile = big ? 128 : 64;
  d.ni = (I + d.tile - 1) / d.tile;
  d.nj = (J + d.tile - 1) / d.tile;
  d.split = 1;
  d.r_per = R;
  if (wgrad && d.ni * d.nj < kCUs) {
    // aim at two blocks per CU; never more slabs than 64-row steps, than
    // the combine's serial loop should walk (64), or than fit the
    // workspace cap (one slab is I*J dW floats plus I db floats)
    long split = (2 * kCUs + d.ni * d.nj - 1) / (d.ni * d.nj);
    split = i64min(split, (R + LIN_BK - 1) / LIN_BK);
    split = i64min(split, 64);
    split = i64min(split, ddlb::kLinearWgradPartCap / (I * J + I));
    split = i64max(split, 1);
    d.r_per = (R + split - 1) / split;
    d.split = (R + d.r_per - 1) / d.r_per;  // no empty slab
  }
  d.steps = (d.r_per + LIN_BK - 1) / LIN_BK;
  return d;
}

}  // namespace

ddlb::LinearPlan ddlb::linear_plan(long M, long N, long K) {
  if (M < 1 || N < 8 || K < 8 || N % 8 != 0 || K % 8 != 0)
    throw std::runtime_error(
        "linear: needs M >= 1 and N, K positive multiples of 8");
  check_extent("x", M, K);
  check_extent("w", N, K);
  check_extent("y", M, N);
  LinearPlan pl;
  pl.fwd = dir_plan(M, N, K, false);
  pl.dgrad = dir_plan(M, K, N, false);
  pl.wgrad = dir_plan(N, K, M, true);
  pl.part_floats = pl.wgrad.split > 1 ? pl.wgrad.split * (N * K + N) : 0;
  return pl;
}

namespace {

LinParams base_params(const ddlb::LinearDirPlan& d, const void* a,
                      const void* b, const void* zero, void* out, long I,
                      long J, long R) {
  LinParams q = {};
  q.a = (const bf16*)a;
  q.b = (const bf16*)b;
  q.zero = (const bf16*)zero;
  q.out = (bf16*)out;
  q.I = (int)I;
  q.J = (int)J;
  q.R = (int)R;
  q.split = (int)d.split;
  q.r_per = (int)d.r_per;
  return q;
}

unsigned grid_of(const ddlb::LinearDirPlan& d) {
  return (unsigned)(d.ni * d.nj * d.split);
}

size_t lds_of(int tile) {
  return (size_t)(tile == 128 ? 2 : 3) * LIN_BK * 2 * tile * sizeof(bf16);
}

}  // namespace

void ddlb::launch_linear_fwd(const LinearPlan& pl, const void* x,
                             const void* w, const void* bias, int bias_f32,
                             void* y, const void* zero, long M, long N,
                             long K, hipStream_t stream) {
  LinParams q = base_params(pl.fwd, x, w, zero, y, M, N, K);
  q.bias = bias;
  q.bias_f32 = bias_f32;
  if (pl.fwd.tile == 128)
    hipLaunchKernelGGL(linear_fwd_kernel<128>, dim3(grid_of(pl.fwd)),
                       dim3(512), lds_of(128), stream, q);
  else
    hipLaunchKernelGGL(linear_fwd_kernel<64>, dim3(grid_of(pl.fwd)),
                       dim3(256), lds_of(64), stream, q);
  HIP_CHECK_LAST();
}

void ddlb::launch_linear_dgrad(const LinearPlan& pl, const void* dy,
                               const void* w, void* dx, const void* zero,
                               long M, long N, long K, hipStream_t stream) {
  const LinParams q = base_params(pl.dgrad, dy, w, zero, dx, M, K, N);
  if (pl.dgrad.tile == 128)
    hipLaunchKernelGGL(linear_dgrad_kernel<128>, dim3(grid_of(pl.dgrad)),
                       dim3(512), lds_of(128), stream, q);
  else
    hipLaunchKernelGGL(linear_dgrad_kernel<64>, dim3(grid_of(pl.dgrad)),
                       dim3(256), lds_of(64), stream, q);
  HIP_CHECK_LAST();
}

void ddlb::launch_linear_wgrad(const LinearPlan& pl, const void* dy,
                               const void* x, void* dw, void* db, int db_f32,
                               float* part, const void* zero, long M, long N,
                               long K, hipStream_t stream) {
  LinParams q = base_params(pl.wgrad, dy, x, zero, dw, N, K, M);
  q.want_db = db != nullptr;
  q.db = db;
  q.bias_f32 = db_f32;
  if (q.split > 1) {
    if (part == nullptr)
      throw std::runtime_error("linear_wgrad: split > 1 needs a workspace");
    q.part = part;
    q.dbpart = part + pl.wgrad.split * N * K;
  }
  if (pl.wgrad.tile == 128)
    hipLaunchKernelGGL(linear_wgrad_kernel<128>, dim3(grid_of(pl.wgrad)),
                       dim3(512), lds_of(128), stream, q);
  else
    hipLaunchKernelGGL(linear_wgrad_kernel<64>, dim3(grid_of(pl.wgrad)),
                       dim3(256), lds_of(64), stream, q);
  if (q.split > 1) {
    const int total = (int)(N * K);
    const unsigned blocks = (unsigned)((total / 4 + N + 255) / 256);
    hipLaunchKernelGGL(linear_wgrad_combine_kernel, dim3(blocks), dim3(256),
                       0, stream, q.part, (bf16*)dw, total, q.dbpart, db,
                       db_f32, (int)N, q.split);
  }
  HIP_CHECK_LAST();
}
