// Weight layout for the data-grad kernels (gfx950): bf16 (K,R,S,C)
// memory -> contiguous (C,R,S,K), the dgrad B tile's layout. A batched
// K x C transpose with R*S as the batch — weight-sized bytes, so the only
// job is to move them in full 16-B accesses on both sides instead of a
// generic strided copy.
//
// 64x64 tile per block, 256 threads. Each thread loads two 16-B chunks
// (8 columns of one row), scatters them transposed into LDS, and stores
// two 16-B chunks of the transposed tile. The LDS row pitch of 66
// halfwords (33 words) spreads the transposed 2-byte writes over the
// banks; rows stay 4-B aligned, so the read side uses four b32 reads
// per chunk.

#include "common.h"
#include "launchers.h"
#include <stdint.h>
#include <stdexcept>
#include <string>

namespace {

#define WL_TILE 64
#define WL_PITCH 66

typedef __attribute__((ext_vector_type(8))) unsigned short ushort8x;
typedef __attribute__((ext_vector_type(4))) unsigned uint4x;

// in[b][m][n] -> out[b][n][m]; M, Nn multiples of 8, so a 16-B chunk is
// either wholly inside or wholly outside the matrix
__global__ __launch_bounds__(256)
void weight_transpose_kernel(const unsigned short* __restrict__ in,
                             unsigned short* __restrict__ out, long M,
                             long Nn, long in_rs, long in_bs, long out_rs,
                             long out_bs) {
  __shared__ __attribute__((aligned(16)))
      unsigned short tile[WL_TILE * WL_PITCH];  // [n][m]
  const int t = threadIdx.x;
  const long n0 = (long)blockIdx.x * WL_TILE;
  const long m0 = (long)blockIdx.y * WL_TILE;
  in += (long)blockIdx.z * in_bs;
  out += (long)blockIdx.z * out_bs;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = (t >> 3) + 32 * i;  // tile row
    const int n = (t & 7) * 8;        // first of 8 tile columns
    if (m0 + m < M && n0 + n < Nn) {
      const ushort8x v = *reinterpret_cast<const ushort8x*>(
          in + (m0 + m) * in_rs + n0 + n);
#pragma unroll
      for (int j = 0; j < 8; ++j) tile[(n + j) * WL_PITCH + m] = v[j];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = (t >> 3) + 32 * i;  // output row within the tile
    const int m = (t & 7) * 8;        // first of 8 output columns
    if (n0 + n < Nn && m0 + m < M) {
      const unsigned* src =
          reinterpret_cast<const unsigned*>(tile + n * WL_PITCH + m);
      uint4x v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = src[j];
      *reinterpret_cast<uint4x*>(out + (n0 + n) * out_rs + m0 + m) = v;
    }
  }
}

}  // namespace

void ddlb::launch_weight_transpose(const void* in, void* out, long B, long M,
                                   long Nn, long in_rs, long in_bs,
                                   long out_rs, long out_bs,
                                   hipStream_t stream) {
  if (M % 8 || Nn % 8 || in_rs % 8 || in_bs % 8 || out_rs % 8 || out_bs % 8)
    throw std::runtime_error(
        "weight_transpose: dims and strides must be multiples of 8");
  if (B < 1 || B > 65535 || (M + WL_TILE - 1) / WL_TILE > 65535)
    throw std::runtime_error("weight_transpose: grid out of range");
  const dim3 grid((unsigned)((Nn + WL_TILE - 1) / WL_TILE),
                  (unsigned)((M + WL_TILE - 1) / WL_TILE), (unsigned)B);
  hipLaunchKernelGGL(weight_transpose_kernel, grid, dim3(256), 0, stream,
                     (const unsigned short*)in, (unsigned short*)out, M, Nn,
                     in_rs, in_bs, out_rs, out_bs);
  HIP_CHECK_LAST();
}
