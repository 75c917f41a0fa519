// Keyed dropout on the rows an attention call hands to its soft-MoE experts (gnot_plan_set_dropout; the original
// GNOT code's resid_drop1 / resid_drop2, which the replicated model.py dropped).  One in-place HBM row pass:
//   x[r, c] = u(r, c) >= T ? x[r, c] * scale : +0.0f        for c < C; columns C .. ld - 1 are left as they are
// a select, never x * 0: a dropped Inf / NaN becomes +0.  No mask is stored: u is a pure function of the key,
//   (u_0 .. u_3) of the quad q = c / 4 = Philox4x32-10(counter = (n, b, site << 8 | q, step), key = (seed_lo, seed_hi))
// with b the row's sample, n its point index WITHIN THE WHOLE sample (glo[b] + r - off[b]: a point-sharded rank
// keys its rows as the unsharded run does), site the call site and (seed_lo, seed_hi, step) read from DEVICE
// memory when the kernel runs -- a captured graph drops a fresh mask on every replay, and the backward is this
// same kernel on the gradient rows with the forward's key.
// One wave64 per row, four rows per workgroup, lane l owning the quads l, l + 64, .. (every wave instruction
// moves 1 KiB contiguous), 16-byte loads and stores, no LDS, no atomics.  The sample of a row is found by a
// wave-uniform binary search over the offsets (the largest b with off[b] <= r: empty samples own no row).
#include "gnot_common.h"
#include "gnot_kernels.h"

namespace gnot {

constexpr int kDropRows = 4;   // rows (waves) per workgroup

// the standard Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by the Weyl constants between them
GNOT_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                            uint32_t (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

template <int NV>
__global__ void __launch_bounds__(WAVE * kDropRows) dropout_rows_kernel(float* x, long ld, long rows, int C,
                                                                        const long* __restrict__ off,
                                                                        const long* __restrict__ glo, int B,
                                                                        const uint32_t* __restrict__ key, uint32_t site,
                                                                        uint32_t T, float scale) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long r = (long)blockIdx.x * kDropRows + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= rows) return;                       // whole waves leave
  int b = 0, hi = B;                           // off[b] <= r < off[hi] throughout (off[0] = 0, off[B] = rows)
  while (hi - b > 1) {
    const int mid = (b + hi) >> 1;
    if (off[mid] <= r) b = mid; else hi = mid;
  }
  const uint32_t n = (uint32_t)(r - off[b] + glo[b]);
  const uint32_t k0 = key[0], k1 = key[1], step = key[2];
  float* row = x + r * ld;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int q = lane + WAVE * k, c = 4 * q;
    if (c >= C) continue;                      // (the float4 that holds column C - 1 lies below the pitch)
    float4 v = *reinterpret_cast<const float4*>(row + c);
    uint32_t u[4];
    philox4x32_10(n, (uint32_t)b, (site << 8) | (uint32_t)q, step, k0, k1, u);
    v.x = u[0] >= T ? v.x * scale : 0.f;
    if (c + 1 < C) v.y = u[1] >= T ? v.y * scale : 0.f;
    if (c + 2 < C) v.z = u[2] >= T ? v.z * scale : 0.f;
    if (c + 3 < C) v.w = u[3] >= T ? v.w * scale : 0.f;
    *reinterpret_cast<float4*>(row + c) = v;
  }
}

// rows in [1, 2^31), C in [1, 1024], the pitch a multiple of 4 that is at least C, 16-byte aligned rows: the
// entries of engine.cpp check them; here only what keeps the launch in bounds.  T = 0: nothing to drop, no launch
hipError_t launch_dropout_rows(float* x, long ld, long rows, int C, const long* off, const long* glo, int B,
                               const uint32_t* key, uint32_t site, uint32_t T, float scale, hipStream_t s) {
  if (rows <= 0 || T == 0) return hipSuccess;
  if (rows >= (1L << 31) || C < 1 || C > 1024 || ld < C || ld % 4 != 0 || ld >= (1L << 31) || B < 1 || !x || !off ||
      !glo || !key || site >= (1u << 24))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((rows + kDropRows - 1) / kDropRows)), block(WAVE * kDropRows);
  const int nv = (C + 255) / 256;              // quads per lane
#define GNOT_DROP(NV) \
  hipLaunchKernelGGL(dropout_rows_kernel<NV>, grid, block, 0, s, x, ld, rows, C, off, glo, B, key, site, T, scale)
  if (nv == 1) GNOT_DROP(1);
  else if (nv == 2) GNOT_DROP(2);
  else if (nv == 3) GNOT_DROP(3);
  else GNOT_DROP(4);
#undef GNOT_DROP
  return hipGetLastError();
}

}  // namespace gnot
