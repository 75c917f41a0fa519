// Batch assembly on the device: rows of a dataset that lives in device memory are copied into a packed batch,
// every segment (one mesh) either whole and in its own order or as the first k values of a keyed permutation
// of its n rows -- a uniform subsample without replacement that is a pure function of (key, n), so a resumed
// run redraws it bit for bit with no device random state (no reference counterpart: main.py:57-58 batches on
// the host through a DataLoader).
//
//   table  one row of kGatherCols int64 per segment b: {src_row0, n, dst_row0, k, key_lo, key_hi}
//   dst[dst_row0 + j] = src[src_row0 + sigma_b(j)], 0 <= j < k;  sigma_b = identity if k == n, else pi
//   (gnot_gather_rows_affine: the same rows, every value normalised with its channel's statistics, stats.hip)
//
// pi(j; n, key) is a cycle-walking Feistel permutation of [0, n), all arithmetic uint32:
//   bits = bit_length(n - 1), h = (bits + 1) / 2, mask = 2^h - 1   (the domain 2^(2h) is below 4 n)
//   rk_r = fmix32(key_lo ^ (r * 0x9E3779B9)) + key_hi, r = 0..5    (fmix32: murmur3's finalizer)
//   E(x): L = x >> h, R = x & mask; six times (L, R) = (R, L ^ (fmix32(R ^ rk_r) & mask)); (L << h) | R
//   pi(j) = the first of E(j), E(E(j)), ... below n -- E is a bijection of the domain, so the walk from a
//   j < n returns into [0, n) and pi is a bijection of it.  Six rounds: four leave a measurable bias.
#include "gnot_common.h"
#include "gnot_kernels.h"

namespace gnot {

constexpr int kFeistelRounds = 6;

__device__ __forceinline__ unsigned fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// the segment b of destination row r: dst_row0[b] <= r < dst_row0[b] + k[b] (train.hip's sample_of_row over the
// table's dst_row0 column; segments without rows are never the answer)
__device__ __forceinline__ int segment_of_row(const long* __restrict__ table, int B, long r) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[(long)mid * kGatherCols + 2] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// one thread per destination row; `rows` = sum of k.  Stats is empty -- gather_rows_kernel<>, the plain copy, with
// the argument list and so the code it had before there was anything else -- or one const float*, the stats
// block {mean[C], std[C], rstd[C]}: every value is then written normalised, (s - mean[c]) * rstd[c], the
// difference and the product each rounded to fp32 -- the bits of the plain gather followed by torch's
// (g - mean) * rstd
template <typename... Stats>
__global__ void __launch_bounds__(256) gather_rows_kernel(const float* __restrict__ src, int C,
                                                          const long* __restrict__ table, int B,
                                                          float* __restrict__ dst, long rows, Stats... stats_arg) {
  static_assert(sizeof...(Stats) <= 1, "at most one stats block");
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
    const long* T = table + (long)segment_of_row(table, B, r) * kGatherCols;
    const long n = T[1], k = T[3];
    unsigned x = (unsigned)(r - T[2]);                       // j < k <= n < 2^31
    if (k != n) {                                            // n >= 2 here (k < n and a row to write: k >= 1)
      const unsigned key_lo = (unsigned)T[4], key_hi = (unsigned)T[5];
      const int h = (32 - __clz((unsigned)(n - 1)) + 1) >> 1;      // 1 .. 16
      const unsigned mask = (1u << h) - 1u;
      unsigned rk[kFeistelRounds];
#pragma unroll
      for (int i = 0; i < kFeistelRounds; ++i) rk[i] = fmix32(key_lo ^ ((unsigned)i * 0x9E3779B9u)) + key_hi;
      do {
        unsigned L = x >> h, R = x & mask;
#pragma unroll
        for (int i = 0; i < kFeistelRounds; ++i) {
          const unsigned t = L ^ (fmix32(R ^ rk[i]) & mask);
          L = R;
          R = t;
        }
        x = (L << h) | R;
      } while (x >= (unsigned)n);
    }
    const float* s = src + (T[0] + (long)x) * C;
    float* d = dst + r * C;
    if constexpr (sizeof...(Stats) == 1) {
      const float* __restrict__ stats = (stats_arg, ...);
      for (int c = 0; c < C; ++c) d[c] = __fmul_rn(__fsub_rn(s[c], stats[c]), stats[2 * C + c]);
    } else {
      for (int c = 0; c < C; ++c) d[c] = s[c];
    }
  }
}

// rows >= 1; stats == nullptr: the plain copy
hipError_t launch_gather_rows(const float* src, int C, const long* table, int B, const float* stats, float* dst,
                              long rows, hipStream_t s) {
  const unsigned grid = (unsigned)std::min<long>((rows + 255) / 256, 8192);
  if (stats)
    hipLaunchKernelGGL(gather_rows_kernel<const float*>, dim3(grid), dim3(256), 0, s, src, C, table, B, dst, rows,
                       stats);
  else
    hipLaunchKernelGGL(gather_rows_kernel<>, dim3(grid), dim3(256), 0, s, src, C, table, B, dst, rows);
  return hipGetLastError();
}

}  // namespace gnot
