// Multi-scale Fourier embedding of coordinates and input functions (the original GNOT code's
// horiz_fourier_dim; no reference counterpart in the replicated model.py, which takes raw inputs).
// For an order n >= 1, W = 4 n + 3 and f_k = 2^(k - n), k = 0 .. 2 n, channel c of a row (value v) becomes the
// W consecutive columns c W .. c W + W - 1
//     [ v, cos(f_0 v) .. cos(f_2n v), sin(f_0 v) .. sin(f_2n v) ]
//   fourier_embed     : src [R, C] -> dst [R, ld], pad columns C W .. ld - 1 written as zeros (the engine's
//                       input staging: gnot_forward's "x" / "fn{i}" rows in front of concat_theta)
//   fourier_embed_bwd : dv [R, C] from the gradient of the embedded row (the sum of up to two sources, as
//                       d x_in[:, :in] + d x_gate in gnot_input_grads) and the embedded row itself, whose cos /
//                       sin columns are the derivatives' factors: no trigonometry in the backward
//     dv = g_0 + sum_k f_k (cos(f_k v) g_sin,k - sin(f_k v) g_cos,k),   g_0 first, then k = 0 .. 2 n
// f_k v is an exact fp32 product (a power of two); sinf / cosf are the full-range routines (the hardware
// fast path reduces its argument in fp32 revolutions and misses by 1e-4 at 1000 rad).
#include <algorithm>

#include "gnot_common.h"
#include "gnot_kernels.h"

namespace gnot {

// 2^e as a float, e in [-8, 8]
__device__ __forceinline__ float pow2f(int e) { return __int_as_float((127 + e) << 23); }

__global__ void __launch_bounds__(256) fourier_embed_kernel(const float* __restrict__ src, long lds, int C, int n,
                                                            float* __restrict__ dst, long ld, long rows) {
  const int W = 4 * n + 3, CW = C * W, nf = 2 * n + 1;
  const long total = rows * ld;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / ld;
    const int col = (int)(i - r * ld);
    float out = 0.f;                               // pad columns are zero
    if (col < CW) {
      const int c = col / W, j = col - c * W;
      const float v = src[r * lds + c];
      if (j == 0) out = v;                         // the raw value, bit for bit
      else if (j <= nf) out = cosf(pow2f(j - 1 - n) * v);
      else out = sinf(pow2f(j - 1 - nf - n) * v);
    }
    dst[i] = out;
  }
}

__global__ void __launch_bounds__(256) fourier_embed_bwd_kernel(const float* __restrict__ emb, long ld,
                                                                const float* __restrict__ ga, long ldga,
                                                                const float* __restrict__ gb, long ldgb, int C,
                                                                int n, float* __restrict__ dv, long rows) {
  const int W = 4 * n + 3, nf = 2 * n + 1;
  const long total = rows * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / C;
    const int c0 = (int)(i - r * C) * W;
    const float* e = emb + r * ld + c0;
    const float* a = ga + r * ldga + c0;
    const float* b = gb ? gb + r * ldgb + c0 : nullptr;
    float acc = b ? a[0] + b[0] : a[0];
    for (int k = 0; k < nf; ++k) {
      const float gc = b ? a[1 + k] + b[1 + k] : a[1 + k];
      const float gs = b ? a[1 + nf + k] + b[1 + nf + k] : a[1 + nf + k];
      acc += pow2f(k - n) * (e[1 + k] * gs - e[1 + nf + k] * gc);
    }
    dv[i] = acc;
  }
}

hipError_t launch_fourier_embed(const float* src, long lds, int C, int n, float* dst, long ld, long rows,
                                hipStream_t s) {
  const long total = rows * ld;
  if (total <= 0) return hipSuccess;
  // 32-bit column indices in the kernel
  if (n < 1 || n > 8 || C < 1 || lds < C || ld < (long)C * (4 * n + 3) || ld >= (1L << 31)) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)std::min<long>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(fourier_embed_kernel, dim3(grid), dim3(256), 0, s, src, lds, C, n, dst, ld, rows);
  return hipGetLastError();
}

hipError_t launch_fourier_embed_bwd(const float* emb, long ld, const float* ga, long ldga, const float* gb, long ldgb,
                                    int C, int n, float* dv, long rows, hipStream_t s) {
  const long total = rows * C;
  if (total <= 0) return hipSuccess;
  const long CW = (long)C * (4 * n + 3);
  if (n < 1 || n > 8 || C < 1 || CW >= (1L << 31) || ld < CW || ldga < CW || (gb && ldgb < CW))
    return hipErrorInvalidValue;
  const unsigned grid = (unsigned)std::min<long>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(fourier_embed_bwd_kernel, dim3(grid), dim3(256), 0, s, emb, ld, ga, ldga, gb, ldgb, C, n, dv,
                     rows);
  return hipGetLastError();
}

}  // namespace gnot
