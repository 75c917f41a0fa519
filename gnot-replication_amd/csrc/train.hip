// The training step on either side of the GNOT path, on the GPU:
//
//   rel_l2_*  RelL2Loss (reference loss.py:14-23) over packed predictions: per-sample segment sums
//             of (p - t)^2 and t^2 (the dgl SumPooling of loss.py:20-21), loss = mean over (sample,
//             channel) of sqrt(num / den), and d loss / d pred in the same pass.  Deterministic:
//             per-split partial sums reduced in a fixed order, no atomics.
//   adamw     torch.optim.AdamW's update (main.py:51; decoupled weight decay, bias-corrected moments)
//             over ONE flat fp32 arena of parameters / gradients / moments, in torch's op order.
//             Hyper-parameters come from a small device array so a captured hipGraph replays
//             whatever the host's schedule (OneCycleLR, main.py:52/106) wrote there.
//   mse_*     MSELoss (reference loss.py:4-12): per-sample means of (p - t)^2 (dgl AvgPooling), in the
//             shape of the rel_l2 passes.
//   grad_clip global L2 norm of the flat gradient and torch.nn.utils.clip_grad_norm_'s coefficient, on
//             the device (two fixed-order stages), consumed by the update through its clip argument.
//   guarded   the clipped update behind a device-side test of that norm: a NaN or infinite norm leaves
//             the parameters and both moments untouched and counts the skipped step (the guard argument).
//   ema       an exponential moving average of the parameters, ema += w (param - ema), as one more stream of
//             the update (adamw_update_kernel<true>: plain, clipped or guarded) or as a pass of its own
//             (ema_update_kernel); w comes from device memory like the other hyper-parameters.
//   affine    both losses on a normalised prediction: p' = pred * std[c] + mean[c] against the raw target, and
//             the gradient scaled by std[c], inside the same passes (Stats of the partial and grad kernels).
//   lp_*      the named losses of the original GNOT recipe (rel2, rel1, relinf, mse, l1, linf) with component
//             weights and the per-(sample, channel) terms as an output, in the shape of the rel_l2 passes
//             (gnot_lp_loss); rel2 / mse without weights are the arithmetic of rel_l2_* / mse_*.
// adamw, its clipped and guarded forms and the fused average are one kernel, adamw_update_kernel<kEma>.
#include "gnot_common.h"
#include "gnot_kernels.h"

namespace gnot {

constexpr int kLossRows = 2048;   // rows per partial-sum workgroup

// the sample b of packed row r: off[b] <= r < off[b + 1], for 0 <= r < off[B]
__device__ __forceinline__ int sample_of_row(const long* __restrict__ off, int B, long r) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the grid of an elementwise grid-stride kernel over n >= 1 elements, 256 threads a workgroup
static unsigned flat_grid(long n) { return (unsigned)std::min<long>((n + 255) / 256, 2048); }

// The _affine losses (gnot_rel_l2_loss_affine, gnot_mse_loss_affine): pred is a normalised prediction and the
// loss that of p' = pred * std[c] + mean[c] against the raw target, stats = {mean[C], std[C], rstd[C]}
// (stats.hip).  The product and the sum are each rounded -- torch's pred * std + mean, bit for bit -- and
// d loss / d pred = (d loss / d p') * std[c] is one more rounded product.  The partial and the gradient kernels
// take the block as a template parameter pack, Stats: empty -- kernel<>, the plain loss, with the argument list
// and so the code it had before there was anything else -- or one const float*.
__device__ __forceinline__ float denormalised(float p, const float* __restrict__ stats, int C, int c) {
  return __fadd_rn(mul_rn(p, stats[C + c]), stats[c]);
}

// partial[b][split][0..2C) = (sum (p-t)^2 [C], sum t^2 [C]) over the split's rows of sample b
template <typename... Stats>
__global__ void __launch_bounds__(256) rel_l2_partial_kernel(const float* __restrict__ pred,
                                                             const float* __restrict__ tgt,
                                                             const long* __restrict__ off, int C, int nsplit,
                                                             float* __restrict__ partial, Stats... stats_arg) {
  __shared__ float red[256];
  const int b = blockIdx.x / nsplit, split = blockIdx.x % nsplit;
  const long r0 = off[b] + (long)split * kLossRows;
  const long r1 = min(off[b + 1], r0 + kLossRows);
  for (int c = 0; c < C; ++c) {
    float num = 0.f, den = 0.f;
    for (long r = r0 + threadIdx.x; r < r1; r += 256) {
      const float t = tgt[r * C + c];
      float d;
      if constexpr (sizeof...(Stats) == 1) d = denormalised(pred[r * C + c], (stats_arg, ...), C, c) - t;
      else d = pred[r * C + c] - t;
      num = fmaf(d, d, num);
      den = fmaf(t, t, den);
    }
    num = block_sum(num, red);
    den = block_sum(den, red);
    if (threadIdx.x == 0) {
      float* P = partial + ((long)b * nsplit + split) * 2 * C;
      P[c] = num;
      P[C + c] = den;
    }
  }
}

// one workgroup: num/den per (b, c) in split order, loss = mean sqrt(num/den), and the per-(b, c)
// gradient scale d loss / d pred = (p - t) / (B C den sqrt(num/den))
__global__ void __launch_bounds__(256) rel_l2_finish_kernel(const float* __restrict__ partial, int B, int C,
                                                            int nsplit, float* __restrict__ scale,
                                                            float* __restrict__ loss) {
  __shared__ float red[256];
  float acc = 0.f;
  for (int i = threadIdx.x; i < B * C; i += 256) {
    const int b = i / C, c = i % C;
    float num = 0.f, den = 0.f;
    for (int s = 0; s < nsplit; ++s) {
      const float* P = partial + ((long)b * nsplit + s) * 2 * C;
      num += P[c];
      den += P[C + c];
    }
    const float r = sqrtf(num / den);
    acc += r;
    scale[i] = 1.0f / ((float)(B * C) * den * r);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) *loss = acc / (float)(B * C);
}

template <typename... Stats>
__global__ void __launch_bounds__(256) rel_l2_grad_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                          const long* __restrict__ off, int B, int C,
                                                          const float* __restrict__ scale, float* __restrict__ dpred,
                                                          long rows, Stats... stats_arg) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * C) return;
  const long r = i / C;
  const int c = (int)(i % C);
  if constexpr (sizeof...(Stats) == 1) {
    const float* __restrict__ stats = (stats_arg, ...);
    const float g = (denormalised(pred[i], stats, C, c) - tgt[i]) * scale[sample_of_row(off, B, r) * C + c];
    dpred[i] = mul_rn(g, stats[C + c]);
  } else {
    dpred[i] = (pred[i] - tgt[i]) * scale[sample_of_row(off, B, r) * C + c];
  }
}

int rel_l2_splits(const long* off_host, int B) {
  long mx = 1;
  for (int b = 0; b < B; ++b) mx = std::max(mx, off_host[b + 1] - off_host[b]);
  return (int)((mx + kLossRows - 1) / kLossRows);
}

template <typename... Stats>
static hipError_t launch_rel_l2_t(const float* pred, const float* tgt, const long* off_dev, int B, int C, int nsplit,
                                  long rows, float* work, float* loss, float* dpred, hipStream_t s, Stats... stats) {
  float* partial = work;                                  // [B][nsplit][2C]
  float* scale = work + (size_t)B * nsplit * 2 * C;       // [B][C]
  hipLaunchKernelGGL(rel_l2_partial_kernel<Stats...>, dim3(B * nsplit), dim3(256), 0, s, pred, tgt, off_dev, C, nsplit,
                     partial, stats...);
  hipLaunchKernelGGL(rel_l2_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)partial, B, C, nsplit, scale, loss);
  if (dpred && rows > 0)
    hipLaunchKernelGGL(rel_l2_grad_kernel<Stats...>, dim3((unsigned)((rows * C + 255) / 256)), dim3(256), 0, s, pred,
                       tgt, off_dev, B, C, (const float*)scale, dpred, rows, stats...);
  return hipGetLastError();
}

// stats == nullptr: the plain loss
hipError_t launch_rel_l2(const float* pred, const float* tgt, const long* off_dev, int B, int C, int nsplit,
                         long rows, const float* stats, float* work, float* loss, float* dpred, hipStream_t s) {
  return stats ? launch_rel_l2_t(pred, tgt, off_dev, B, C, nsplit, rows, work, loss, dpred, s, stats)
               : launch_rel_l2_t(pred, tgt, off_dev, B, C, nsplit, rows, work, loss, dpred, s);
}

// ---------------------------------------------------------------- MSELoss (reference loss.py:4-12)
// dgl AvgPooling of (p - t)^2 = per-sample mean over points, then the mean over (sample, channel); the
// passes have the shape of the RelL2 ones above (which stay as they are, bit for bit).
// partial[b][split][0..C) = sum (p-t)^2 over the split's rows of sample b
template <typename... Stats>
__global__ void __launch_bounds__(256) mse_partial_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                          const long* __restrict__ off, int C, int nsplit,
                                                          float* __restrict__ partial, Stats... stats_arg) {
  __shared__ float red[256];
  const int b = blockIdx.x / nsplit, split = blockIdx.x % nsplit;
  const long r0 = off[b] + (long)split * kLossRows;
  const long r1 = min(off[b + 1], r0 + kLossRows);
  for (int c = 0; c < C; ++c) {
    float num = 0.f;
    for (long r = r0 + threadIdx.x; r < r1; r += 256) {
      float d;
      if constexpr (sizeof...(Stats) == 1) d = denormalised(pred[r * C + c], (stats_arg, ...), C, c) - tgt[r * C + c];
      else d = pred[r * C + c] - tgt[r * C + c];
      num = fmaf(d, d, num);
    }
    num = block_sum(num, red);
    if (threadIdx.x == 0) partial[((long)b * nsplit + split) * C + c] = num;
  }
}

// one workgroup: sum per (b, c) in split order, loss = 1/(B C) sum_b sum_c num / N_b
__global__ void __launch_bounds__(256) mse_finish_kernel(const float* __restrict__ partial,
                                                         const long* __restrict__ off, int B, int C, int nsplit,
                                                         float* __restrict__ loss) {
  __shared__ float red[256];
  float acc = 0.f;
  for (int i = threadIdx.x; i < B * C; i += 256) {
    const int b = i / C, c = i % C;
    float num = 0.f;
    for (int s = 0; s < nsplit; ++s) num += partial[((long)b * nsplit + s) * C + c];
    acc += num / (float)(off[b + 1] - off[b]);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) *loss = acc / (float)(B * C);
}

// d loss / d pred = 2 (p - t) / (B C N_b)
template <typename... Stats>
__global__ void __launch_bounds__(256) mse_grad_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                       const long* __restrict__ off, int B, int C,
                                                       float* __restrict__ dpred, long rows, Stats... stats_arg) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * C) return;
  const int b = sample_of_row(off, B, i / C);
  if constexpr (sizeof...(Stats) == 1) {
    const float* __restrict__ stats = (stats_arg, ...);
    const int c = (int)(i % C);
    const float g = (denormalised(pred[i], stats, C, c) - tgt[i]) *
                    (2.0f / ((float)(B * C) * (float)(off[b + 1] - off[b])));
    dpred[i] = mul_rn(g, stats[C + c]);
  } else {
    dpred[i] = (pred[i] - tgt[i]) * (2.0f / ((float)(B * C) * (float)(off[b + 1] - off[b])));
  }
}

// work: B*nsplit*C floats
template <typename... Stats>
static hipError_t launch_mse_t(const float* pred, const float* tgt, const long* off_dev, int B, int C, int nsplit,
                               long rows, float* work, float* loss, float* dpred, hipStream_t s, Stats... stats) {
  hipLaunchKernelGGL(mse_partial_kernel<Stats...>, dim3(B * nsplit), dim3(256), 0, s, pred, tgt, off_dev, C, nsplit,
                     work, stats...);
  hipLaunchKernelGGL(mse_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)work, off_dev, B, C, nsplit, loss);
  if (dpred && rows > 0)
    hipLaunchKernelGGL(mse_grad_kernel<Stats...>, dim3((unsigned)((rows * C + 255) / 256)), dim3(256), 0, s, pred, tgt,
                       off_dev, B, C, dpred, rows, stats...);
  return hipGetLastError();
}

// stats == nullptr: the plain loss
hipError_t launch_mse(const float* pred, const float* tgt, const long* off_dev, int B, int C, int nsplit, long rows,
                      const float* stats, float* work, float* loss, float* dpred, hipStream_t s) {
  return stats ? launch_mse_t(pred, tgt, off_dev, B, C, nsplit, rows, work, loss, dpred, s, stats)
               : launch_mse_t(pred, tgt, off_dev, B, C, nsplit, rows, work, loss, dpred, s);
}

// ---------------------------------------------------------------- Lp losses (gnot_lp_loss)
// The loss family of the original GNOT recipe in the shape of the passes above: per (sample, channel) a term
//   e[b, c] = ||d||_p / ||t||_p  (kRel: rel2, rel1, relinf)   or   sum |d|^p / N_b  (mse, l1),  max |d|  (linf),
// d = p' - t with p' the prediction or its de-normalisation, p = kNorm (2, 1, or 0 for the maximum norm), and
//   loss = (1/B) sum_b sum_c w^_c e[b, c],  w^_c = w_c / sum_c w_c  (1/C without weights).
// Without weights the instantiations for rel2 and mse are the arithmetic of the rel_l2_* / mse_* kernels above,
// operation for operation, so loss and gradient have their bits; the plain forms without weights and terms are
// not instantiated at all (launch_lp runs the kernels above).  The maximum is taken so that a NaN stays one.
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

// block_sum's tree with nan_max in place of the sum
__device__ __forceinline__ float block_max(float x, float* red) {
  red[threadIdx.x] = x;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = nan_max(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const float m = red[0];
  __syncthreads();
  return m;
}

// one more element v of a channel's norm: sum v^2, sum |v|, max |v|
template <int kNorm>
__device__ __forceinline__ float lp_accumulate(float v, float acc) {
  if constexpr (kNorm == 2) return fmaf(v, v, acc);
  else if constexpr (kNorm == 1) return acc + fabsf(v);
  else return nan_max(acc, fabsf(v));
}

template <int kNorm>
__device__ __forceinline__ float lp_block(float x, float* red) {
  if constexpr (kNorm == 0) return block_max(x, red);
  else return block_sum(x, red);
}

// partial[b][split][0..kW C), kW = kRel ? 2 : 1: the norm's sum (or maximum) of d [C] and, kRel, of t [C] over
// the split's rows of sample b (an empty split: zeros)
template <int kNorm, bool kRel, typename... Stats>
__global__ void __launch_bounds__(256) lp_partial_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                         const long* __restrict__ off, int C, int nsplit,
                                                         float* __restrict__ partial, Stats... stats_arg) {
  __shared__ float red[256];
  constexpr int kW = kRel ? 2 : 1;
  const int b = blockIdx.x / nsplit, split = blockIdx.x % nsplit;
  const long r0 = off[b] + (long)split * kLossRows;
  const long r1 = min(off[b + 1], r0 + kLossRows);
  for (int c = 0; c < C; ++c) {
    float num = 0.f, den = 0.f;
    for (long r = r0 + threadIdx.x; r < r1; r += 256) {
      const float t = tgt[r * C + c];
      float d;
      if constexpr (sizeof...(Stats) == 1) d = denormalised(pred[r * C + c], (stats_arg, ...), C, c) - t;
      else d = pred[r * C + c] - t;
      num = lp_accumulate<kNorm>(d, num);
      if constexpr (kRel) den = lp_accumulate<kNorm>(t, den);
    }
    num = lp_block<kNorm>(num, red);
    if constexpr (kRel) den = lp_block<kNorm>(den, red);
    if (threadIdx.x == 0) {
      float* P = partial + ((long)b * nsplit + split) * kW * C;
      P[c] = num;
      if constexpr (kRel) P[C + c] = den;
    }
  }
}

// one workgroup: the norms per (b, c) in split order, the term e[b, c] (to terms, if asked for), the loss and
// the per-(b, c) gradient scale s: d loss / d p' = s d (kNorm 2) or s sign(d) (kNorm 1).  w == nullptr: the
// mean over (sample, channel) as rel_l2_finish_kernel / mse_finish_kernel take it; else w^_c from w[C], summed
// in index order.
template <int kNorm, bool kRel>
__global__ void __launch_bounds__(256) lp_finish_kernel(const float* __restrict__ partial, const long* __restrict__ off,
                                                        int B, int C, int nsplit, const float* __restrict__ w,
                                                        float* __restrict__ scale, float* __restrict__ loss,
                                                        float* __restrict__ terms) {
  __shared__ float red[256];
  constexpr int kW = kRel ? 2 : 1;
  float wsum = 0.f;
  if (w) for (int c = 0; c < C; ++c) wsum += w[c];
  float acc = 0.f;
  for (int i = threadIdx.x; i < B * C; i += 256) {
    const int b = i / C, c = i % C;
    float num = 0.f, den = 0.f;
    for (int s = 0; s < nsplit; ++s) {
      const float* P = partial + ((long)b * nsplit + s) * kW * C;
      if constexpr (kNorm == 0) num = nan_max(num, P[c]); else num += P[c];
      if constexpr (kRel) {
        if constexpr (kNorm == 0) den = nan_max(den, P[C + c]); else den += P[C + c];
      }
    }
    const float n = (float)(off[b + 1] - off[b]);
    float e;
    if constexpr (kRel) e = kNorm == 2 ? sqrtf(num / den) : num / den;
    else e = kNorm == 0 ? num : num / n;
    if (terms) terms[i] = e;
    // the mean's factor: 1 / (B C), or w^_c / B
    const float wc = w ? w[c] / wsum : 1.0f;
    const float count = w ? (float)B : (float)(B * C);
    if (w) acc += mul_rn(wc, e); else acc += e;
    if constexpr (kNorm == 2 && kRel) scale[i] = wc / (count * den * e);
    else if constexpr (kNorm == 1 && kRel) scale[i] = wc / (count * den);
    else if constexpr (kNorm == 2) scale[i] = mul_rn(2.0f, wc) / (count * n);
    else if constexpr (kNorm == 1) scale[i] = wc / (count * n);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) *loss = acc / (w ? (float)B : (float)(B * C));
}

// d loss / d pred, elementwise; a channel of weight zero is written as zeros whatever d holds
template <int kNorm, typename... Stats>
__global__ void __launch_bounds__(256) lp_grad_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                      const long* __restrict__ off, int B, int C,
                                                      const float* __restrict__ w, const float* __restrict__ scale,
                                                      float* __restrict__ dpred, long rows, Stats... stats_arg) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * C) return;
  const long r = i / C;
  const int c = (int)(i % C);
  if (w && w[c] == 0.f) { dpred[i] = 0.f; return; }
  const float s = scale[sample_of_row(off, B, r) * C + c];
  float d;
  if constexpr (sizeof...(Stats) == 1) d = denormalised(pred[i], (stats_arg, ...), C, c) - tgt[i];
  else d = pred[i] - tgt[i];
  float g;
  if constexpr (kNorm == 2) g = d * s;
  else g = d > 0.f ? s : d < 0.f ? -s : mul_rn(d, 0.f);      // sign(0) = 0; a NaN stays one
  if constexpr (sizeof...(Stats) == 1) {
    const float* __restrict__ stats = (stats_arg, ...);
    dpred[i] = mul_rn(g, stats[C + c]);
  } else {
    dpred[i] = g;
  }
}

template <int kNorm, bool kRel, typename... Stats>
static hipError_t launch_lp_t(const float* pred, const float* tgt, const long* off_dev, int B, int C, int nsplit,
                              long rows, const float* w, float* work, float* loss, float* terms, float* dpred,
                              hipStream_t s, Stats... stats) {
  float* partial = work;                                              // [B][nsplit][kW C]
  float* scale = work + (size_t)B * nsplit * (kRel ? 2 : 1) * C;      // [B][C]
  hipLaunchKernelGGL((lp_partial_kernel<kNorm, kRel, Stats...>), dim3(B * nsplit), dim3(256), 0, s, pred, tgt, off_dev,
                     C, nsplit, partial, stats...);
  hipLaunchKernelGGL((lp_finish_kernel<kNorm, kRel>), dim3(1), dim3(256), 0, s, (const float*)partial, off_dev, B, C,
                     nsplit, w, scale, loss, terms);
  if constexpr (kNorm != 0) {
    if (dpred && rows > 0)
      hipLaunchKernelGGL((lp_grad_kernel<kNorm, Stats...>), dim3((unsigned)((rows * C + 255) / 256)), dim3(256), 0, s,
                         pred, tgt, off_dev, B, C, w, (const float*)scale, dpred, rows, stats...);
  }
  return hipGetLastError();
}

// kind: GNOT_LP_* (gnot_hip.h), checked by the caller, as is dpred == nullptr for the two maximum norms.
// work: B*nsplit*2C + B*C floats (nsplit = rel_l2_splits); every sample has at least one row.  w, stats, terms,
// dpred may be null.  rel2 and mse without w and terms: launch_rel_l2 / launch_mse, the same kernels.
hipError_t launch_lp(int kind, const float* pred, const float* tgt, const long* off_dev, int B, int C, int nsplit,
                     long rows, const float* w, const float* stats, float* work, float* loss, float* terms,
                     float* dpred, hipStream_t s) {
  if (!w && !terms && kind == 0) return launch_rel_l2(pred, tgt, off_dev, B, C, nsplit, rows, stats, work, loss, dpred, s);
  if (!w && !terms && kind == 3) return launch_mse(pred, tgt, off_dev, B, C, nsplit, rows, stats, work, loss, dpred, s);
#define GNOT_LP_CASE(K, NORM, REL)                                                                                   \
  case K:                                                                                                            \
    return stats ? launch_lp_t<NORM, REL>(pred, tgt, off_dev, B, C, nsplit, rows, w, work, loss, terms, dpred, s,    \
                                          stats)                                                                     \
                 : launch_lp_t<NORM, REL>(pred, tgt, off_dev, B, C, nsplit, rows, w, work, loss, terms, dpred, s);
  switch (kind) {
    GNOT_LP_CASE(0, 2, true)
    GNOT_LP_CASE(1, 1, true)
    GNOT_LP_CASE(2, 0, true)
    GNOT_LP_CASE(3, 2, false)
    GNOT_LP_CASE(4, 1, false)
    GNOT_LP_CASE(5, 0, false)
  }
#undef GNOT_LP_CASE
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------- global gradient norm and clip coefficient
// torch.nn.utils.clip_grad_norm_ (L2, error_if_nonfinite=False) over the flat gradient arena, on the device.
// Stage 1: workgroup k sums g^2 over elements [k kClipSlice, (k + 1) kClipSlice) -- the number of partials
// depends on n alone, never on the device -- in a fixed order; stage 2: one workgroup sums the partials in
// index order.  No atomics: the same pointer and n give the same bits every run.
constexpr long kClipSlice = 8192;   // elements per stage-1 workgroup: 8 float4 loads per thread

long grad_clip_partials(long n) { return n < 1 ? 0 : (n + kClipSlice - 1) / kClipSlice; }

// sum g^2 over p[0, len), 1 <= len <= kClipSlice, by the 256 threads of a workgroup in a fixed order (every thread
// returns the sum)
__device__ __forceinline__ float slice_sumsq(const float* __restrict__ p, int len, float* red) {
  // 16-byte loads over the aligned body of the slice; the (up to 3) elements before and after it one by one
  const int head = min(len, (int)((4 - (((uintptr_t)p >> 2) & 3)) & 3));
  const int body4 = (len - head) >> 2;
  const int tail = len - head - 4 * body4;
  const float4* q = reinterpret_cast<const float4*>(p + head);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
  for (int j = threadIdx.x; j < body4; j += 256) {
    const float4 g = q[j];
    a0 = fmaf(g.x, g.x, a0);
    a1 = fmaf(g.y, g.y, a1);
    a2 = fmaf(g.z, g.z, a2);
    a3 = fmaf(g.w, g.w, a3);
  }
  if ((int)threadIdx.x < head) {
    const float g = p[threadIdx.x];
    a0 = fmaf(g, g, a0);
  }
  if ((int)threadIdx.x < tail) {
    const float g = p[head + 4 * body4 + threadIdx.x];
    a1 = fmaf(g, g, a1);
  }
  return block_sum((a0 + a1) + (a2 + a3), red);
}

__global__ void __launch_bounds__(256) grad_sumsq_kernel(const float* __restrict__ grad, long n,
                                                         float* __restrict__ partial) {
  __shared__ float red[256];
  const long s0 = (long)blockIdx.x * kClipSlice;
  const float sum = slice_sumsq(grad + s0, (int)min(kClipSlice, n - s0), red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// The same stage 1 over a slice table (gnot_grad_norm_groups / gnot_grad_clip_groups): workgroup k sums g^2 over
// [begin, begin + len) of row k = {begin, len, group}, so an element outside every row is never read.
constexpr int kSliceCols = 3;

__global__ void __launch_bounds__(256) grad_sumsq_slices_kernel(const float* __restrict__ grad,
                                                                const long* __restrict__ slices,
                                                                float* __restrict__ partial) {
  __shared__ float red[256];
  const long* S = slices + (long)blockIdx.x * kSliceCols;
  const float sum = slice_sumsq(grad + S[0], (int)S[1], red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// clip[0] = |grad_scale| sqrt(sum g^2), the norm of the gradient AdamW consumes (hyper[7] scales it);
// clip[1] = min(1, max_norm / (norm + 1e-6)) as torch clamps it: a NaN norm stays a NaN coefficient.
// norm_only (gnot_grad_norm): the same norm, no max_norm, clip[1] = 1.0f.
__global__ void __launch_bounds__(256) grad_clip_finish_kernel(const float* __restrict__ partial, long nparts,
                                                               const float* __restrict__ hyper, float max_norm,
                                                               int norm_only, float* __restrict__ clip) {
  __shared__ float red[256];
  float acc = 0.f;
  for (long i = threadIdx.x; i < nparts; i += 256) acc += partial[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const float norm = fabsf(hyper[7]) * sqrtf(acc);
    const float c = max_norm / (norm + 1e-6f);
    clip[0] = norm;
    clip[1] = (norm_only || c > 1.0f) ? 1.0f : c;
  }
}

// work: grad_clip_partials(n) floats
static hipError_t launch_grad_norm_stages(const float* grad, long n, const float* hyper, float max_norm, int norm_only,
                                          float* work, float* clip, hipStream_t s) {
  const long nparts = grad_clip_partials(n);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nparts), dim3(256), 0, s, grad, n, work);
  hipLaunchKernelGGL(grad_clip_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)work, nparts, hyper, max_norm,
                     norm_only, clip);
  return hipGetLastError();
}

// work: nslices floats; the table's rows are validated by the caller
hipError_t launch_grad_norm_slices(const float* grad, const long* slices, long nslices, const float* hyper,
                                   float max_norm, int norm_only, float* work, float* clip, hipStream_t s) {
  hipLaunchKernelGGL(grad_sumsq_slices_kernel, dim3((unsigned)nslices), dim3(256), 0, s, grad, slices, work);
  hipLaunchKernelGGL(grad_clip_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)work, nslices, hyper, max_norm,
                     norm_only, clip);
  return hipGetLastError();
}

hipError_t launch_grad_clip(const float* grad, long n, const float* hyper, float max_norm, float* work, float* clip,
                            hipStream_t s) {
  return launch_grad_norm_stages(grad, n, hyper, max_norm, 0, work, clip, s);
}

hipError_t launch_grad_norm(const float* grad, long n, const float* hyper, float* work, float* clip, hipStream_t s) {
  return launch_grad_norm_stages(grad, n, hyper, 1.0f, 1, work, clip, s);
}

// ---------------------------------------------------------------- AdamW over a flat arena
// hyper = {lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2, grad_scale[, ema weight]}
//
// One kernel for every update: torch's AdamW on the gradient (grad[i] * grad_scale) * coef.
//   clip   what launch_grad_clip / launch_grad_norm wrote, read from device memory so a captured graph applies
//          the coefficient of the step it replays; nullptr: no coefficient (the plain update).
//   guard  the non-finite guard (needs clip): every thread reads the norm clip[0] -- one value for the whole
//          grid, so the decision is uniform -- and on a NaN or +-inf (exponent bits all ones) no element of
//          param / m / v / ema is written.  guard = {skipped launches since the caller zeroed it, 1 if this
//          launch skipped else 0}, written by thread 0 of workgroup 0 alone; launches on one stream are
//          ordered, so the count needs no atomic.  nullptr: no test.
//   kEma   the element's average follows the parameter value just stored, ema = fma(w, p - ema, ema) with
//          w = hyper[8] -- ema_update_kernel's expression on the same operands, so fused and stand-alone agree
//          bit for bit; param / m / v are computed exactly as without it.
// The multiply-adds are written out and no others are allowed (which ones a compiler fuses depends on the code
// around them): they are the fusions the first, plain-only form of this kernel was compiled with, in torch's
// operation order.  A coefficient of 1.0f multiplies exactly, so every variant computes the same exp_avg_sq,
// denominator and parameter from the same scaled gradient.
template <bool kEma>
__global__ void __launch_bounds__(256) adamw_update_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           float* __restrict__ ema, long n,
                                                           const float* __restrict__ hyper,
                                                           const float* __restrict__ clip, int* __restrict__ guard) {
#pragma clang fp contract(off)
  if (guard) {
    const bool finite = (__float_as_uint(clip[0]) & 0x7f800000u) != 0x7f800000u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (!finite) guard[0] = guard[0] + 1;
      guard[1] = finite ? 0 : 1;
    }
    if (!finite) return;
  }
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4];
  const float bc1 = hyper[5], bc2 = hyper[6], gs = hyper[7];
  const float step_size = lr / bc1;
  const float bc2_sqrt = sqrtf(bc2);
  const float decay = fmaf(-lr, wd, 1.0f);               // decoupled weight decay
  const float coef = clip ? clip[1] : 1.0f;
  const float w = kEma ? hyper[8] : 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float gi = grad[i] * gs;
    const float g = gi * coef;
    float mi = m[i];
    // g - exp_avg: the plain update without the average was first compiled with the scaling fused into the
    // subtraction (grad[i] * grad_scale not rounded), every other variant multiplies the rounded gi by the
    // coefficient.  The two differ when grad_scale is not a power of two; each entry keeps its own bits.
    const float inner = (kEma || clip) ? fmaf(gi, coef, -mi) : fmaf(grad[i], gs, -mi);
    mi = fmaf(1.0f - b1, inner, mi);                        // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = fmaf(g, (1.0f - b2) * g, v[i] * b2);   // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    const float p = fmaf(decay, param[i], -(step_size * (mi / denom)));   // param.addcdiv_(exp_avg, denom, -step_size)
    param[i] = p;
    m[i] = mi;
    v[i] = vi;
    if (kEma) {
      const float e = ema[i];
      ema[i] = fmaf(w, p - e, e);
    }
  }
}

// ema == nullptr: no average (hyper has 8 floats), else hyper has 9.  n >= 1 when there is a guard (the grid's
// first thread writes it); n <= 0 launches nothing.
hipError_t launch_adamw_update(float* param, const float* grad, float* m, float* v, float* ema, long n,
                               const float* hyper, const float* clip, int* guard, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (ema)
    hipLaunchKernelGGL(adamw_update_kernel<true>, dim3(flat_grid(n)), dim3(256), 0, s, param, grad, m, v, ema, n, hyper,
                       clip, guard);
  else
    hipLaunchKernelGGL(adamw_update_kernel<false>, dim3(flat_grid(n)), dim3(256), 0, s, param, grad, m, v, ema, n,
                       hyper, clip, guard);
  return hipGetLastError();
}

// ---------------------------------------------------------------- AdamW per slice, with group constants
// adamw_update_kernel's element expression over a slice table instead of [0, n): workgroup k updates the elements
// [begin, begin + len) of row k = {begin, len, group} (len <= kClipSlice) with lr = hyper[0] * ghyper[group][0],
// the product rounded to fp32 once, and weight_decay = ghyper[group][1]; hyper[4] is not read.  An element outside
// every row is neither read nor written, in any array.  The moment's inner term is always the rounded-product
// form fmaf(gi, coef, -mi) of the clipped update (coef = 1.0f without a clip): with one group {1, hyper[4]} whose
// rows cover [0, n) the results are adamw_update_kernel's bit for bit, for the plain update when hyper[7] is a
// power of two.  guard: as there, written by thread 0 of workgroup 0 (at least one row).
template <bool kEma>
__global__ void __launch_bounds__(256) adamw_groups_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           float* __restrict__ ema, const float* __restrict__ hyper,
                                                           const float* __restrict__ ghyper,
                                                           const long* __restrict__ slices,
                                                           const float* __restrict__ clip, int* __restrict__ guard) {
#pragma clang fp contract(off)
  if (guard) {
    const bool finite = (__float_as_uint(clip[0]) & 0x7f800000u) != 0x7f800000u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (!finite) guard[0] = guard[0] + 1;
      guard[1] = finite ? 0 : 1;
    }
    if (!finite) return;
  }
  const long* S = slices + (long)blockIdx.x * kSliceCols;
  const long begin = S[0];
  const int len = (int)S[1];
  const float* gh = ghyper + 2 * S[2];
  const float lr = hyper[0] * gh[0], wd = gh[1];
  const float b1 = hyper[1], b2 = hyper[2], eps = hyper[3];
  const float bc1 = hyper[5], bc2 = hyper[6], gs = hyper[7];
  const float step_size = lr / bc1;
  const float bc2_sqrt = sqrtf(bc2);
  const float decay = fmaf(-lr, wd, 1.0f);               // decoupled weight decay
  const float coef = clip ? clip[1] : 1.0f;
  const float w = kEma ? hyper[8] : 0.f;
  for (int j = threadIdx.x; j < len; j += 256) {
    const long i = begin + j;
    const float gi = grad[i] * gs;
    const float g = gi * coef;
    float mi = m[i];
    mi = fmaf(1.0f - b1, fmaf(gi, coef, -mi), mi);
    const float vi = fmaf(g, (1.0f - b2) * g, v[i] * b2);
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    const float p = fmaf(decay, param[i], -(step_size * (mi / denom)));
    param[i] = p;
    m[i] = mi;
    v[i] = vi;
    if (kEma) {
      const float e = ema[i];
      ema[i] = fmaf(w, p - e, e);
    }
  }
}

// nslices >= 1; the table's rows are validated by the caller.  ema, clip, guard as in launch_adamw_update.
hipError_t launch_adamw_groups(float* param, const float* grad, float* m, float* v, float* ema, const float* hyper,
                               const float* ghyper, const long* slices, long nslices, const float* clip, int* guard,
                               hipStream_t s) {
  if (ema)
    hipLaunchKernelGGL(adamw_groups_kernel<true>, dim3((unsigned)nslices), dim3(256), 0, s, param, grad, m, v, ema,
                       hyper, ghyper, slices, clip, guard);
  else
    hipLaunchKernelGGL(adamw_groups_kernel<false>, dim3((unsigned)nslices), dim3(256), 0, s, param, grad, m, v, ema,
                       hyper, ghyper, slices, clip, guard);
  return hipGetLastError();
}

// ---------------------------------------------------------------- weight EMA
// ema = fma(w, param - ema, ema) over n elements, w = weight[0] from device memory (a captured graph picks up
// each step's value).  The subtraction is rounded on its own: the expression of adamw_update_kernel<true>.
__global__ void __launch_bounds__(256) ema_update_kernel(float* __restrict__ ema, const float* __restrict__ param,
                                                         long n, const float* __restrict__ weight) {
#pragma clang fp contract(off)
  const float w = weight[0];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float e = ema[i];
    ema[i] = fmaf(w, param[i] - e, e);
  }
}

// n >= 1
hipError_t launch_ema_update(float* ema, const float* param, long n, const float* weight, hipStream_t s) {
  hipLaunchKernelGGL(ema_update_kernel, dim3(flat_grid(n)), dim3(256), 0, s, ema, param, n, weight);
  return hipGetLastError();
}

}  // namespace gnot

