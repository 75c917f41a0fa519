// Parameter-free LayerNorm over the C real features of a row (the pre-norm of the attention inputs,
// gnot_plan_set_pre_norm; the original GNOT code's ln1 .. ln5 without gamma / beta, which fold into the Linear
// behind; no counterpart in the replicated model.py).  Two HBM-bound row passes:
//   layer_norm     : y[r, :C] = (x[r, :C] - mean) * rstd, rstd = 1 / sqrtf(var + eps), var the biased variance
//                    as the sum of (x - mean)^2 over the registers (never E[x^2] - mean^2); columns C .. ldy - 1
//                    written as exact zeros (the engine's padded widths); input columns C .. ldx - 1 masked, not
//                    assumed zero; rstd[r] kept when asked for
//   layer_norm_bwd : dx = rstd * (dy - mean_C(dy) - y * mean_C(dy * y)) from the saved y and rstd (no statistics
//                    recomputed), stored (pad columns C .. lddx - 1 as zeros) or added onto dx with one rounded
//                    add per element (pad columns untouched); dx may alias dy
// One wave64 per row, four rows per workgroup: the row lives in registers (NV float4 per lane, lane l holding
// float4 l, l + 64, ..: every wave instruction moves 1 KiB contiguous), one pass over memory, no LDS, no atomics.
// Every row sum is the lane's own partial (its float4 in order, x + y + z + w each) followed by an xor butterfly
// over the 64 lanes: one fixed order, the same on every lane, whatever grid or workgroup the row runs in.
// The mean is kept as two floats, mean = hi + lo with hi = sum(x) / C rounded and lo = sum(x - hi) / C, and
// x - mean is (x - hi) - lo: a row with a large common offset loses nothing to the rounding of hi (x - hi is
// exact there, and lo is small), so y and rstd carry the rounding of the deviations, not of the offset; and a
// constant row gives exact zeros (x - hi is then the same multiple of one ulp on every lane, its sums and the
// division by C are exact, and lo equals it).
#include "gnot_common.h"
#include "gnot_kernels.h"

namespace gnot {

constexpr int kNormRows = 4;   // rows (waves) per workgroup

GNOT_DEV float wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) v += shfl_xor(v, m);
  return v;
}

// the lane's float4 k of a row with C real columns; columns from C on read as zeros (the float4 that holds
// column C - 1 lies below the row pitch, a multiple of 4)
template <int NV>
GNOT_DEV void load_row(const float* __restrict__ row, int C, int lane, float4 (&v)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * (lane + WAVE * k);
    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) {
      v[k] = *reinterpret_cast<const float4*>(row + c);
      if (c + 1 >= C) v[k].y = 0.f;
      if (c + 2 >= C) v[k].z = 0.f;
      if (c + 3 >= C) v[k].w = 0.f;
    }
  }
}

template <int NV>
GNOT_DEV float row_sum(const float4 (&v)[NV]) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
  return wave_sum(s);
}

template <int NV>
__global__ void __launch_bounds__(WAVE * kNormRows) layer_norm_kernel(const float* __restrict__ x, long ldx,
                                                                      long rows, int C, float eps,
                                                                      float* __restrict__ y, long ldy,
                                                                      float* __restrict__ rstd_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long r = (long)blockIdx.x * kNormRows + (threadIdx.x >> 6);
  if (r >= rows) return;                       // whole waves leave: no lane of a live wave is missing
  float4 v[NV];
  load_row<NV>(x + r * ldx, C, lane, v);
  const float fc = (float)C;
  // the mean as two floats: hi the rounded row mean, lo the mean of the exact differences x - hi
  const float hi = row_sum<NV>(v) / fc;
  float4 d[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * (lane + WAVE * k);
    d[k].x = c < C ? v[k].x - hi : 0.f;
    d[k].y = c + 1 < C ? v[k].y - hi : 0.f;
    d[k].z = c + 2 < C ? v[k].z - hi : 0.f;
    d[k].w = c + 3 < C ? v[k].w - hi : 0.f;
  }
  const float lo = row_sum<NV>(d) / fc;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * (lane + WAVE * k);
    d[k].x = c < C ? d[k].x - lo : 0.f;
    d[k].y = c + 1 < C ? d[k].y - lo : 0.f;
    d[k].z = c + 2 < C ? d[k].z - lo : 0.f;
    d[k].w = c + 3 < C ? d[k].w - lo : 0.f;
  }
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) q += (d[k].x * d[k].x + d[k].y * d[k].y) + (d[k].z * d[k].z + d[k].w * d[k].w);
  const float var = wave_sum(q) / fc;
  const float rstd = 1.0f / sqrtf(var + eps);
  float* yr = y + r * ldy;
  const int ld4 = (int)(ldy >> 2);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c4 = lane + WAVE * k;
    if (c4 < ld4)                              // pad columns: d is zero there
      *reinterpret_cast<float4*>(yr + 4 * c4) = make_float4(d[k].x * rstd, d[k].y * rstd, d[k].z * rstd, d[k].w * rstd);
  }
  for (int c4 = lane + WAVE * NV; c4 < ld4; c4 += WAVE)
    *reinterpret_cast<float4*>(yr + 4 * c4) = make_float4(0.f, 0.f, 0.f, 0.f);
  if (rstd_out && lane == 0) rstd_out[r] = rstd;
}

template <int NV>
__global__ void __launch_bounds__(WAVE * kNormRows) layer_norm_bwd_kernel(const float* __restrict__ y, long ldy,
                                                                          const float* __restrict__ rstd,
                                                                          const float* dy, long lddy, long rows, int C,
                                                                          float* dx, long lddx, int accumulate) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long r = (long)blockIdx.x * kNormRows + (threadIdx.x >> 6);
  if (r >= rows) return;
  float4 yv[NV], g[NV];
  load_row<NV>(y + r * ldy, C, lane, yv);
  load_row<NV>(dy + r * lddy, C, lane, g);     // the whole row is in registers before any of it is written
  const float rs = rstd[r];
  float4 gy[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) gy[k] = make_float4(g[k].x * yv[k].x, g[k].y * yv[k].y, g[k].z * yv[k].z, g[k].w * yv[k].w);
  const float fc = (float)C;
  const float m1 = row_sum<NV>(g) / fc;        // mean_C(dy)
  const float m2 = row_sum<NV>(gy) / fc;       // mean_C(dy * y)
  float* dr = dx + r * lddx;
  const int ld4 = (int)(lddx >> 2);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c4 = lane + WAVE * k, c = 4 * c4;
    if (c4 >= ld4 || (accumulate && c >= C)) continue;
    float4 o;                                  // (mul_rn: the add of the accumulating form below stays one rounded add)
    o.x = c < C ? mul_rn(rs, (g[k].x - m1) - yv[k].x * m2) : 0.f;
    o.y = c + 1 < C ? mul_rn(rs, (g[k].y - m1) - yv[k].y * m2) : 0.f;
    o.z = c + 2 < C ? mul_rn(rs, (g[k].z - m1) - yv[k].z * m2) : 0.f;
    o.w = c + 3 < C ? mul_rn(rs, (g[k].w - m1) - yv[k].w * m2) : 0.f;
    float4* p = reinterpret_cast<float4*>(dr + c);
    if (accumulate) {
      const float4 old = *p;                   // (adding the zero of a pad column leaves it as it is)
      o = make_float4(old.x + o.x, old.y + o.y, old.z + o.z, old.w + o.w);
    }
    *p = o;
  }
  if (!accumulate)
    for (int c4 = lane + WAVE * NV; c4 < ld4; c4 += WAVE)
      *reinterpret_cast<float4*>(dr + 4 * c4) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// rows in [1, 2^31), C in [1, 1024], every pitch a multiple of 4 that is at least C and below 2^31, 16-byte
// aligned pointers: the entries of engine.cpp check them; here only what keeps the launch in bounds
static bool norm_shape_ok(long rows, int C, long lda, long ldb) {
  return rows < (1L << 31) && C >= 1 && C <= 1024 && lda >= C && ldb >= C && lda % 4 == 0 && ldb % 4 == 0 &&
         lda < (1L << 31) && ldb < (1L << 31);
}

hipError_t launch_layer_norm(const float* x, long ldx, long rows, int C, float eps, float* y, long ldy, float* rstd,
                             hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!norm_shape_ok(rows, C, ldx, ldy)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((rows + kNormRows - 1) / kNormRows)), block(WAVE * kNormRows);
  const int nv = (C + 255) / 256;              // float4 per lane
#define GNOT_LN(NV) hipLaunchKernelGGL(layer_norm_kernel<NV>, grid, block, 0, s, x, ldx, rows, C, eps, y, ldy, rstd)
  if (nv == 1) GNOT_LN(1);
  else if (nv == 2) GNOT_LN(2);
  else if (nv == 3) GNOT_LN(3);
  else GNOT_LN(4);
#undef GNOT_LN
  return hipGetLastError();
}

hipError_t launch_layer_norm_bwd(const float* y, long ldy, const float* rstd, const float* dy, long lddy, long rows,
                                 int C, float* dx, long lddx, int accumulate, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!norm_shape_ok(rows, C, ldy, lddy) || !norm_shape_ok(rows, C, lddx, lddx)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((rows + kNormRows - 1) / kNormRows)), block(WAVE * kNormRows);
  const int nv = (C + 255) / 256;
#define GNOT_LNB(NV)                                                                                             \
  hipLaunchKernelGGL(layer_norm_bwd_kernel<NV>, grid, block, 0, s, y, ldy, rstd, dy, lddy, rows, C, dx, lddx, \
                     accumulate)
  if (nv == 1) GNOT_LNB(1);
  else if (nv == 2) GNOT_LNB(2);
  else if (nv == 3) GNOT_LNB(3);
  else GNOT_LNB(4);
#undef GNOT_LNB
  return hipGetLastError();
}

}  // namespace gnot
