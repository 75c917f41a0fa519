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

// ---------------------------------------------------------------- the same statistics with a weight per row
// gnot_channel_stats_weighted: w [rows] >= 0 (quadrature weights, a mask), V1 = sum w, V2 = sum w^2,
//   mean = sum w x / V1,   var = sum w (x - mean)^2 / (V1 - V2 / V1)
// -- the reliability-weights estimator, whose divisor is rows - 1 at w == 1.  The scheme is the one above with w
// inside every sum and the sums of w where the row counts stood:
//   stage 1  slice k: V1_k, V2_k once, and per channel m_k = pivot + sum w (x - pivot) / V1_k, s_k = sum w (x - m_k),
//            q_k = sum w (x - m_k)^2; the pivot is the slice's first row with w > 0.  A slice without one stores
//            V1_k = 0 and is skipped in stage 2.
//   stage 2  M = P + sum_k (V1_k (m_k - P) + s_k) / V1 with P the m_k of the first slice that has one, and
//            sum w (x - M)^2 = sum_k (q_k + (m_k - M) (2 s_k + V1_k (m_k - M))).
// A row with w == 0 (anything not > 0) is skipped before its values are loaded: a NaN under a mask is never read.
// At w == 1 every expression is the unweighted kernel's on the same operands.  V1 - V2 / V1 <= 0 (one weighted
// row) is a constant channel; no weighted row at all gives mean = 0 / 0.
// work: per slice {V1_k, V2_k} and kStatPart floats per channel.
constexpr int kStatHead = 2;

// the least x over the workgroup's 256 threads, to every thread (block_sum's tree)
__device__ __forceinline__ float block_min(float x, float* red) {
  red[threadIdx.x] = x;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const float m = red[0];
  __syncthreads();
  return m;
}

__global__ void __launch_bounds__(256) channel_stats_weighted_partial_kernel(const float* __restrict__ src,
                                                                             const float* __restrict__ w, long rows,
                                                                             int C, float* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ float red[256];
  const long r0 = (long)blockIdx.x * kStatRows;
  const long r1 = min(rows, r0 + kStatRows);
  float* P = partial + (long)blockIdx.x * (kStatHead + (long)C * kStatPart);
  // the slice's first weighted row (its index in the slice, exact in fp32) and the sums of w
  float first = (float)kStatRows, v1 = 0.f, v2 = 0.f;
  for (long r = r0 + threadIdx.x; r < r1; r += 256) {
    const float wr = w[r];
    if (!(wr > 0.f)) continue;
    first = fminf(first, (float)(r - r0));
    v1 += wr;
    v2 = fmaf(wr, wr, v2);
  }
  first = block_min(first, red);
  v1 = block_sum(v1, red);
  v2 = block_sum(v2, red);
  if (threadIdx.x == 0) {
    P[0] = first < (float)kStatRows ? v1 : 0.f;
    P[1] = first < (float)kStatRows ? v2 : 0.f;
  }
  if (!(first < (float)kStatRows)) {      // no weighted row (uniform over the workgroup): nothing of src is read
    for (int i = threadIdx.x; i < C * kStatPart; i += 256) P[kStatHead + i] = 0.f;
    return;
  }
  const long rp = r0 + (long)first;
  for (int c = 0; c < C; ++c) {
    const float pivot = src[rp * C + c];
    float a = 0.f;
    for (long r = r0 + threadIdx.x; r < r1; r += 256) {
      const float wr = w[r];
      if (!(wr > 0.f)) continue;
      a += wr * (src[r * C + c] - pivot);
    }
    const float m = pivot + block_sum(a, red) / v1;
    float s = 0.f, q = 0.f;
    for (long r = r0 + threadIdx.x; r < r1; r += 256) {
      const float wr = w[r];
      if (!(wr > 0.f)) continue;
      const float d = src[r * C + c] - m;
      const float wd = wr * d;
      s += wd;
      q = fmaf(wd, d, q);
    }
    s = block_sum(s, red);
    q = block_sum(q, red);
    if (threadIdx.x == 0) {
      float* Pc = P + kStatHead + c * kStatPart;
      Pc[0] = m;
      Pc[1] = s;
      Pc[2] = q;
    }
  }
}

__global__ void __launch_bounds__(256) channel_stats_weighted_finish_kernel(const float* __restrict__ partial,
                                                                            long nslice, int C, float eps,
                                                                            float* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ float red[256];
  const int c = blockIdx.x;
  const long ld = kStatHead + (long)C * kStatPart;
  const float* Pc = partial + kStatHead + (long)c * kStatPart;
  // the first slice with a weighted row (nslice < 2^19: exact in fp32), V1 and V2
  float first = (float)nslice, v1 = 0.f, v2 = 0.f;
  for (long k = threadIdx.x; k < nslice; k += 256) {
    const float n = partial[k * ld];
    if (!(n > 0.f)) continue;
    first = fminf(first, (float)k);
    v1 += n;
    v2 += partial[k * ld + 1];
  }
  first = block_min(first, red);
  v1 = block_sum(v1, red);
  v2 = block_sum(v2, red);
  const float pivot = first < (float)nslice ? Pc[(long)first * ld] : 0.f;
  float a = 0.f;
  for (long k = threadIdx.x; k < nslice; k += 256) {
    const float n = partial[k * ld];
    if (!(n > 0.f)) continue;
    a += n * (Pc[k * ld] - pivot) + Pc[k * ld + 1];
  }
  const float mean = pivot + block_sum(a, red) / v1;
  float q = 0.f;
  for (long k = threadIdx.x; k < nslice; k += 256) {
    const float n = partial[k * ld];
    if (!(n > 0.f)) continue;
    const float d = Pc[k * ld] - mean;
    q += Pc[k * ld + 2] + d * (2.0f * Pc[k * ld + 1] + n * d);
  }
  q = block_sum(q, red);
  if (threadIdx.x == 0) {
    const float dof = v1 - v2 / v1;      // rows - 1 at w == 1
    float sd = dof > 0.f ? sqrtf(fmaxf(q, 0.f) / dof) : 0.f;
    const bool constant = !(dof > 0.f) || sd <= 1e-6f * fabsf(mean);
    if (constant) sd = 0.f;
    stats[c] = mean;
    stats[C + c] = sd;
    stats[2 * C + c] = constant ? 1.0f : 1.0f / (sd + eps);
  }
}

// work: channel_stats_slices(rows) * (2 + 3 * C) floats; rows >= 1, C >= 1
hipError_t launch_channel_stats_weighted(const float* src, const float* w, long rows, int C, float eps, float* work,
                                         float* stats, hipStream_t s) {
  const long nslice = channel_stats_slices(rows);
  hipLaunchKernelGGL(channel_stats_weighted_partial_kernel, dim3((unsigned)nslice), dim3(256), 0, s, src, w, rows, C,
                     work);
  hipLaunchKernelGGL(channel_stats_weighted_finish_kernel, dim3((unsigned)C), dim3(256), 0, s, (const float*)work,
                     nslice, C, eps, stats);
  return hipGetLastError();
}

}  // namespace gnot
