// Per-channel statistics of a dataset array that lives in device memory, for unit-Gaussian normalisation (the
// original GNOT code's UnitTransformer, (x - mean) / (std + 1e-8), over packed rows; no counterpart in the
// replicated main.py, which trains on raw values):
//
//   stats = {mean[C], std[C], rstd[C]} of src [rows, C]; std unbiased (divisor rows - 1, torch.std),
//   rstd = 1 / (std + eps); a constant channel (rows == 1, or std <= 1e-6 |mean|) gets std = 0, rstd = 1.
//
// The variance is never taken as E[x^2] - E[x]^2 of raw values (at mean 1e4, std 1 that loses every digit).
// Two fixed-order stages, no atomics -- the number of partials depends on rows alone:
//   stage 1  workgroup k owns rows [k kStatRows, (k + 1) kStatRows) and, per channel, makes two passes over
//            them (the second one hits the cache): m_k = pivot + sum (x - pivot) / n_k with the slice's first
//            row as pivot, then s_k = sum (x - m_k) and q_k = sum (x - m_k)^2.  m_k is a rounded fp32 value,
//            s_k what it misses: the slice's exact mean is m_k + s_k / n_k.
//   stage 2  one workgroup per channel merges the slices about M, exactly as algebra (Chan et al. with the
//            residual kept): M = P + sum_k (n_k (m_k - P) + s_k) / rows, P = m_0, and
//            sum (x - M)^2 = sum_k (q_k + (m_k - M) (2 s_k + n_k (m_k - M))).
// Every difference above is taken between nearby fp32 values, so the sums carry errors relative to the
// channel's spread, not to its offset.  A one-off pass per dataset (Normalizer.fit), not a per-step kernel.
#include "gnot_common.h"
#include "gnot_kernels.h"

namespace gnot {

constexpr long kStatRows = 4096;   // rows per stage-1 workgroup: 16 per thread and channel
constexpr int kStatPart = 3;       // floats per (slice, channel): {m_k, s_k, q_k}

long channel_stats_slices(long rows) { return rows < 1 ? 0 : (rows + kStatRows - 1) / kStatRows; }

// partial[k][c] = {m_k, s_k, q_k} of channel c over slice k = blockIdx.x
__global__ void __launch_bounds__(256) channel_stats_partial_kernel(const float* __restrict__ src, long rows, int C,
                                                                    float* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ float red[256];
  const long r0 = (long)blockIdx.x * kStatRows;
  const long r1 = min(rows, r0 + kStatRows);
  const float n = (float)(r1 - r0);
  for (int c = 0; c < C; ++c) {
    const float pivot = src[r0 * C + c];
    float a = 0.f;
    for (long r = r0 + threadIdx.x; r < r1; r += 256) a += src[r * C + c] - pivot;
    const float m = pivot + block_sum(a, red) / n;
    float s = 0.f, q = 0.f;
    for (long r = r0 + threadIdx.x; r < r1; r += 256) {
      const float d = src[r * C + c] - m;
      s += d;
      q = fmaf(d, d, q);
    }
    s = block_sum(s, red);
    q = block_sum(q, red);
    if (threadIdx.x == 0) {
      float* P = partial + ((long)blockIdx.x * C + c) * kStatPart;
      P[0] = m;
      P[1] = s;
      P[2] = q;
    }
  }
}

// channel c = blockIdx.x: the slices in index order, strided over the threads, then the tree
__global__ void __launch_bounds__(256) channel_stats_finish_kernel(const float* __restrict__ partial, long rows,
                                                                   long nslice, int C, float eps,
                                                                   float* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ float red[256];
  const int c = blockIdx.x;
  const float* Pc = partial + (long)c * kStatPart;
  const long ld = (long)C * kStatPart;
  const float pivot = Pc[0];
  float a = 0.f;
  for (long k = threadIdx.x; k < nslice; k += 256) {
    const float n = (float)min(kStatRows, rows - k * kStatRows);
    a += n * (Pc[k * ld] - pivot) + Pc[k * ld + 1];
  }
  const float mean = pivot + block_sum(a, red) / (float)rows;
  float q = 0.f;
  for (long k = threadIdx.x; k < nslice; k += 256) {
    const float n = (float)min(kStatRows, rows - k * kStatRows);
    const float d = Pc[k * ld] - mean;
    q += Pc[k * ld + 2] + d * (2.0f * Pc[k * ld + 1] + n * d);
  }
  q = block_sum(q, red);
  if (threadIdx.x == 0) {
    float sd = rows > 1 ? sqrtf(fmaxf(q, 0.f) / (float)(rows - 1)) : 0.f;
    const bool constant = rows == 1 || sd <= 1e-6f * fabsf(mean);
    if (constant) sd = 0.f;
    stats[c] = mean;
    stats[C + c] = sd;
    stats[2 * C + c] = constant ? 1.0f : 1.0f / (sd + eps);
  }
}

// work: channel_stats_slices(rows) * 3 * C floats; rows >= 1, C >= 1
hipError_t launch_channel_stats(const float* src, long rows, int C, float eps, float* work, float* stats,
                                hipStream_t s) {
  const long nslice = channel_stats_slices(rows);
  hipLaunchKernelGGL(channel_stats_partial_kernel, dim3((unsigned)nslice), dim3(256), 0, s, src, rows, C, work);
  hipLaunchKernelGGL(channel_stats_finish_kernel, dim3((unsigned)C), dim3(256), 0, s, (const float*)work, rows, nslice,
                     C, eps, stats);
  return hipGetLastError();
}

}  // namespace gnot
