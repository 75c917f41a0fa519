// The training step on either side of the GNOT path, on the GPU:
//
//   lp_*      every loss, over packed predictions: per-sample segment norms of d = p - t and, for the relative
//             kinds, of t (the dgl SumPooling / AvgPooling of reference loss.py), the mean over (sample, channel)
//             of the per-(sample, channel) terms, and d loss / d pred in the same pass.  One kernel family,
//             lp_{partial,finish,grad}_kernel<kNorm, kRel>, for the six named losses of the original GNOT recipe
//             (rel2, rel1, relinf, mse, l1, linf), with component weights and the terms as an output
//             (gnot_lp_loss).  RelL2Loss (loss.py:14-23; gnot_rel_l2_loss) and MSELoss (loss.py:4-12;
//             gnot_mse_loss) are its kinds 0 and 3 with w == terms == nullptr.  Deterministic: per-split partial
//             sums reduced in a fixed order, no atomics.
//   affine    a loss on a normalised prediction: p' = pred * std[c] + mean[c] against the raw target, and the
//             gradient scaled by std[c], inside the same passes (Stats of the partial and grad kernels).
//   weighted  a loss with one weight per packed row (gnot_lp_loss_weighted: quadrature weights, masks): sums of
//             w |d|^p over the rows with w > 0 and sum w for N_b, as one more entry of the same pack
//             (PointWeights); the unweighted instantiations keep their argument lists and code.
//   adamw     torch.optim.AdamW's update (main.py:51; decoupled weight decay, bias-corrected moments)
//             over ONE flat fp32 arena of parameters / gradients / moments, in torch's op order.
//             Hyper-parameters come from a small device array so a captured hipGraph replays
//             whatever the host's schedule (OneCycleLR, main.py:52/106) wrote there.
//   grad_clip global L2 norm of the flat gradient and torch.nn.utils.clip_grad_norm_'s coefficient, on
//             the device (two fixed-order stages), consumed by the update through its clip argument.
//   guarded   the clipped update behind a device-side test of that norm: a NaN or infinite norm leaves
//             the parameters and both moments untouched and counts the skipped step (the guard argument).
//   ema       an exponential moving average of the parameters, ema += w (param - ema), as one more stream of
//             the update (adamw_update_kernel<true>: plain, clipped or guarded) or as a pass of its own
//             (ema_update_kernel); w comes from device memory like the other hyper-parameters.
// adamw, its clipped and guarded forms and the fused average are one kernel, adamw_update_kernel<kEma>; the
// slice-table form adamw_groups_kernel<kEma> runs the same guard and the same element update (adamw_element).
#include <type_traits>

#include "gnot_common.h"
#include "gnot_kernels.h"

namespace gnot {

constexpr int kLossRows = 2048;  // rows per partial-sum workgroup

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

// A loss with a stats block (gnot_rel_l2_loss_affine, gnot_mse_loss_affine, gnot_lp_loss with out_stats): pred is
// a normalised prediction and the loss that of p' = pred * std[c] + mean[c] against the raw target, stats =
// {mean[C], std[C], rstd[C]} (stats.hip).  The product and the sum are each rounded -- torch's pred * std + mean,
// bit for bit -- and d loss / d pred = (d loss / d p') * std[c] is one more rounded product.  The partial and the
// gradient kernels take the block as a template parameter pack, Stats: empty -- kernel<>, the plain loss, whose
// argument list and code know nothing of it -- or one const float*.
__device__ __forceinline__ float denormalised(float p, const float* __restrict__ stats, int C, int c) {
  return __fadd_rn(mul_rn(p, stats[C + c]), stats[c]);
}

// A loss with per-point weights (gnot_lp_loss_weighted): one weight w_r >= 0 per packed row, which multiplies
// the row's |d|^p and |t|^p in the sums and its gradient, and sum w stands where N_b stood.  It is one more entry
// of the same pack, PointWeights, behind the stats block if there is one: Stats is {}, {const float*},
// {PointWeights} or {const float*, PointWeights}, and the first two are the kernels above, argument for argument.
//   * a row with w_r == 0 (anything that is not > 0) is skipped before its pred / tgt are loaded -- a NaN under a
//     mask never meets a 0 * NaN -- and its gradient elements are stored as zeros;
//   * w_r == 1 everywhere gives the unweighted kernels' bits: fmaf(w d, d, acc), acc + w |d| and (w d) s multiply
//     by one exactly, in the unweighted order, and sum w == N_b exactly below 2^24 rows a sample;
//   * w_r times a power of two over a whole sample scales every sum exactly and cancels in every term and in
//     w_r * scale: no bit of loss, terms or gradient moves.
struct PointWeights {
  const float* w;   // DEVICE [rows]
};
template <typename... A>
inline constexpr bool kHasStats = (std::is_same_v<A, const float*> || ...);
template <typename... A>
inline constexpr bool kHasPointW = (std::is_same_v<A, PointWeights> || ...);
__device__ __forceinline__ const float* stats_of(const float* s) { return s; }
__device__ __forceinline__ const float* stats_of(const float* s, PointWeights) { return s; }
__device__ __forceinline__ const float* point_w_of(PointWeights p) { return p.w; }
__device__ __forceinline__ const float* point_w_of(const float*, PointWeights p) { return p.w; }

// the 2048-row splits of the longest sample: partial sums per (sample, split), at least one split
int rel_l2_splits(const long* off_host, int B) {
  long mx = 1;
  for (int b = 0; b < B; ++b) mx = std::max(mx, off_host[b + 1] - off_host[b]);
  return (int)((mx + kLossRows - 1) / kLossRows);
}

// ---------------------------------------------------------------- the losses
// Per (sample, channel) a term
//   e[b, c] = ||d||_p / ||t||_p  (kRel: rel2, rel1, relinf)   or   sum |d|^p / N_b  (mse, l1),  max |d|  (linf),
// d = p' - t with p' the prediction or its de-normalisation, p = kNorm (2, 1, or 0 for the maximum norm), and
//   loss = (1/B) sum_b sum_c w^_c e[b, c],  w^_c = w_c / sum_c w_c  (1/C without weights).
// Three passes: partial norms per (sample, 2048-row split), one workgroup that finishes them in split order, and
// the elementwise gradient.  The maximum is taken so that a NaN stays one.
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

// ... and of a row of weight w > 0: sum w v^2, sum w |v|, and the maximum over the weighted rows, which w does
// not scale.  w == 1 is lp_accumulate, bit for bit.
template <int kNorm>
__device__ __forceinline__ float lp_accumulate_w(float w, float v, float acc) {
  if constexpr (kNorm == 2) return fmaf(mul_rn(w, v), v, acc);
  else if constexpr (kNorm == 1) return acc + mul_rn(w, fabsf(v));
  else return nan_max(acc, fabsf(v));
}

// floats per channel of a partial: the norm of d and, for a relative kind, of t; a weighted mean kind (mse, l1
// with PointWeights) carries sum w in the second place
template <int kNorm, bool kRel, bool kPointW>
constexpr int lp_partial_width() { return (kRel || (kPointW && kNorm != 0)) ? 2 : 1; }

// partial[b][split][0..kW C), kW = lp_partial_width: the norm's sum (or maximum) of d [C] and, kRel, of t [C] over
// the split's rows of sample b (an empty split: zeros); with PointWeights over its rows of positive weight, and
// sum w [C] (every channel's the same) in t's place for mse / l1
template <int kNorm, bool kRel, typename... Stats>
__global__ void __launch_bounds__(256) lp_partial_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                         const long* __restrict__ off, int C, int nsplit,
                                                         float* __restrict__ partial, Stats... stats_arg) {
  __shared__ float red[256];
  constexpr bool kPointW = kHasPointW<Stats...>;
  constexpr bool kSumW = kPointW && !kRel && kNorm != 0;
  constexpr int kW = lp_partial_width<kNorm, kRel, kPointW>();
  const int b = blockIdx.x / nsplit, split = blockIdx.x % nsplit;
  const long r0 = off[b] + (long)split * kLossRows;
  const long r1 = min(off[b + 1], r0 + kLossRows);
  for (int c = 0; c < C; ++c) {
    float num = 0.f, den = 0.f;
    for (long r = r0 + threadIdx.x; r < r1; r += 256) {
      if constexpr (kPointW) {
        const float pw = point_w_of(stats_arg...)[r];
        if (!(pw > 0.f)) continue;      // not read into any sum: its pred and tgt are not even loaded
        const float t = tgt[r * C + c];
        float d;
        if constexpr (kHasStats<Stats...>) d = denormalised(pred[r * C + c], stats_of(stats_arg...), C, c) - t;
        else d = pred[r * C + c] - t;
        num = lp_accumulate_w<kNorm>(pw, d, num);
        if constexpr (kRel) den = lp_accumulate_w<kNorm>(pw, t, den);
        if constexpr (kSumW) den += pw;
      } else {
        const float t = tgt[r * C + c];
        float d;
        if constexpr (kHasStats<Stats...>) d = denormalised(pred[r * C + c], stats_of(stats_arg...), C, c) - t;
        else d = pred[r * C + c] - t;
        num = lp_accumulate<kNorm>(d, num);
        if constexpr (kRel) den = lp_accumulate<kNorm>(t, den);
      }
    }
    num = lp_block<kNorm>(num, red);
    if constexpr (kRel) den = lp_block<kNorm>(den, red);
    if constexpr (kSumW) den = block_sum(den, red);
    if (threadIdx.x == 0) {
      float* P = partial + ((long)b * nsplit + split) * kW * C;
      P[c] = num;
      if constexpr (kW == 2) P[C + c] = den;
    }
  }
}

// one workgroup: the norms per (b, c) in split order, the term e[b, c] (to terms, if asked for), the loss and
// the per-(b, c) gradient scale s: d loss / d p' = s d (kNorm 2) or s sign(d) (kNorm 1).  w == nullptr: the
// plain mean over (sample, channel), sum e / (B C); else w^_c from w[C], summed in index order.  kPointW (the
// partials of a weighted pass): the mean kinds divide by the sample's sum w, summed in split order like the
// norms -- N_b exactly when every weight is 1 -- and every other kind finishes as without weights.
template <int kNorm, bool kRel, bool kPointW = false>
__global__ void __launch_bounds__(256) lp_finish_kernel(const float* __restrict__ partial, const long* __restrict__ off,
                                                        int B, int C, int nsplit, const float* __restrict__ w,
                                                        float* __restrict__ scale, float* __restrict__ loss,
                                                        float* __restrict__ terms) {
  __shared__ float red[256];
  constexpr int kW = lp_partial_width<kNorm, kRel, kPointW>();
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
      } else if constexpr (kW == 2) {
        den += P[C + c];
      }
    }
    const float n = (kW == 2 && !kRel) ? den : (float)(off[b + 1] - off[b]);
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
  [[maybe_unused]] float pw = 1.0f;
  if constexpr (kHasPointW<Stats...>) {      // a row of weight zero: exact zeros, its pred and tgt not loaded
    pw = point_w_of(stats_arg...)[r];
    if (!(pw > 0.f)) { dpred[i] = 0.f; return; }
  }
  const float s = scale[sample_of_row(off, B, r) * C + c];
  float d;
  if constexpr (kHasStats<Stats...>) d = denormalised(pred[i], stats_of(stats_arg...), C, c) - tgt[i];
  else d = pred[i] - tgt[i];
  float g;
  if constexpr (kHasPointW<Stats...>) {      // the row's weight times the unweighted expression; w == 1: its bits
    const float ws = mul_rn(pw, s);
    if constexpr (kNorm == 2) g = mul_rn(pw, d) * s;
    else g = d > 0.f ? ws : d < 0.f ? -ws : mul_rn(d, 0.f);
  } else {
    if constexpr (kNorm == 2) g = d * s;
    else g = d > 0.f ? s : d < 0.f ? -s : mul_rn(d, 0.f);      // sign(0) = 0; a NaN stays one
  }
  if constexpr (kHasStats<Stats...>) {
    const float* __restrict__ stats = stats_of(stats_arg...);
    dpred[i] = mul_rn(g, stats[C + c]);
  } else {
    dpred[i] = g;
  }
}

template <int kNorm, bool kRel, typename... Stats>
static hipError_t launch_lp_t(const float* pred, const float* tgt, const long* off_dev, int B, int C, int nsplit,
                              long rows, const float* w, float* work, float* loss, float* terms, float* dpred,
                              hipStream_t s, Stats... stats) {
  constexpr bool kPointW = kHasPointW<Stats...>;
  float* partial = work;                                              // [B][nsplit][kW C]
  float* scale = work + (size_t)B * nsplit * lp_partial_width<kNorm, kRel, kPointW>() * C;      // [B][C]
  hipLaunchKernelGGL((lp_partial_kernel<kNorm, kRel, Stats...>), dim3(B * nsplit), dim3(256), 0, s, pred, tgt, off_dev,
                     C, nsplit, partial, stats...);
  // (only the weighted mean kinds finish differently: every other weighted pass shares the unweighted kernel)
  hipLaunchKernelGGL((lp_finish_kernel<kNorm, kRel, kPointW && !kRel && kNorm != 0>), dim3(1), dim3(256), 0, s,
                     (const float*)partial, off_dev, B, C, nsplit, w, scale, loss, terms);
  if constexpr (kNorm != 0) {
    if (dpred && rows > 0)
      hipLaunchKernelGGL((lp_grad_kernel<kNorm, Stats...>), dim3((unsigned)((rows * C + 255) / 256)), dim3(256), 0, s,
                         pred, tgt, off_dev, B, C, w, (const float*)scale, dpred, rows, stats...);
  }
  return hipGetLastError();
}

// kind: GNOT_LP_* (gnot_hip.h), checked by the caller, as is dpred == nullptr for the two maximum norms.
// work: B*nsplit*kW*C + B*C floats, kW = 2 for the relative kinds, else 1 (nsplit = rel_l2_splits).  A sample
// without rows has zero norms: rel2's term is then sqrt(0 / 0), a NaN (the caller refuses it for every other
// kind).  w, stats, terms, dpred may be null.  point_w (per-row weights, [rows]; nullptr: none): the weighted
// kernels, whose partials are two floats wide for every kind but linf.
hipError_t launch_lp(int kind, const float* pred, const float* tgt, const float* point_w, const long* off_dev, int B,
                     int C, int nsplit, long rows, const float* w, const float* stats, float* work, float* loss,
                     float* terms, float* dpred, hipStream_t s) {
#define GNOT_LP_ARGS pred, tgt, off_dev, B, C, nsplit, rows, w, work, loss, terms, dpred, s
#define GNOT_LP_CASE(K, NORM, REL)                                                                                   \
  case K:                                                                                                            \
    if (point_w)                                                                                                     \
      return stats ? launch_lp_t<NORM, REL>(GNOT_LP_ARGS, stats, PointWeights{point_w})                              \
                   : launch_lp_t<NORM, REL>(GNOT_LP_ARGS, PointWeights{point_w});                                    \
    return stats ? launch_lp_t<NORM, REL>(GNOT_LP_ARGS, stats) : launch_lp_t<NORM, REL>(GNOT_LP_ARGS);
  switch (kind) {
    GNOT_LP_CASE(0, 2, true)
    GNOT_LP_CASE(1, 1, true)
    GNOT_LP_CASE(2, 0, true)
    GNOT_LP_CASE(3, 2, false)
    GNOT_LP_CASE(4, 1, false)
    GNOT_LP_CASE(5, 0, false)
  }
#undef GNOT_LP_CASE
#undef GNOT_LP_ARGS
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
struct AdamwStep {   // what an element's update takes besides its arrays: one set per launch, or per slice
  float b1, b2, eps, gs, step_size, bc2_sqrt, decay, coef, w;
};

// the guard of a launch (above; nullptr: none): false when no element may be written
__device__ __forceinline__ bool adamw_guard_passes(const float* __restrict__ clip, int* __restrict__ guard) {
#pragma clang fp contract(off)
  if (!guard) return true;
  const bool finite = (__float_as_uint(clip[0]) & 0x7f800000u) != 0x7f800000u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (!finite) guard[0] = guard[0] + 1;
    guard[1] = finite ? 0 : 1;
  }
  return finite;
}

// element i of every update kernel.  fused_scale: the moment's inner term g - exp_avg is fmaf(grad[i], gs, -mi),
// the scaling not rounded (the plain update without the average alone); else fmaf(gi, coef, -mi).
template <bool kEma>
__device__ __forceinline__ void adamw_element(float* __restrict__ param, const float* __restrict__ grad,
                                              float* __restrict__ m, float* __restrict__ v, float* __restrict__ ema,
                                              long i, const AdamwStep& k, bool fused_scale) {
#pragma clang fp contract(off)
  const float gi = grad[i] * k.gs;
  const float g = gi * k.coef;
  float mi = m[i];
  const float inner = fused_scale ? fmaf(grad[i], k.gs, -mi) : fmaf(gi, k.coef, -mi);
  mi = fmaf(1.0f - k.b1, inner, mi);                          // exp_avg.lerp_(grad, 1 - beta1)
  const float vi = fmaf(g, (1.0f - k.b2) * g, v[i] * k.b2);   // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = sqrtf(vi) / k.bc2_sqrt + k.eps;
  const float p = fmaf(k.decay, param[i], -(k.step_size * (mi / denom)));   // param.addcdiv_(exp_avg, denom, -step_size)
  param[i] = p;
  m[i] = mi;
  v[i] = vi;
  if (kEma) {
    const float e = ema[i];
    ema[i] = fmaf(k.w, p - e, e);
  }
}

template <bool kEma>
__global__ void __launch_bounds__(256) adamw_update_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           float* __restrict__ ema, long n,
                                                           const float* __restrict__ hyper,
                                                           const float* __restrict__ clip, int* __restrict__ guard) {
#pragma clang fp contract(off)
  if (!adamw_guard_passes(clip, guard)) return;
  const float lr = hyper[0], wd = hyper[4], bc1 = hyper[5], bc2 = hyper[6];
  const AdamwStep k = {hyper[1], hyper[2], hyper[3], hyper[7], lr / bc1, sqrtf(bc2),
                       fmaf(-lr, wd, 1.0f),                 // decoupled weight decay
                       clip ? clip[1] : 1.0f, kEma ? hyper[8] : 0.f};
  // g - exp_avg: the plain update without the average was first compiled with the scaling fused into the
  // subtraction (grad[i] * grad_scale not rounded), every other variant multiplies the rounded gi by the
  // coefficient.  The two differ when grad_scale is not a power of two; each entry keeps its own bits.
  const bool fused_scale = !(kEma || clip);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    adamw_element<kEma>(param, grad, m, v, ema, i, k, fused_scale);
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
// adamw_element over a slice table instead of [0, n): workgroup k updates the elements
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
  if (!adamw_guard_passes(clip, guard)) return;
  const long* S = slices + (long)blockIdx.x * kSliceCols;
  const long begin = S[0];
  const int len = (int)S[1];
  const float* gh = ghyper + 2 * S[2];
  const float lr = hyper[0] * gh[0], wd = gh[1], bc1 = hyper[5], bc2 = hyper[6];
  const AdamwStep k = {hyper[1], hyper[2], hyper[3], hyper[7], lr / bc1, sqrtf(bc2),
                       fmaf(-lr, wd, 1.0f),                 // decoupled weight decay
                       clip ? clip[1] : 1.0f, kEma ? hyper[8] : 0.f};
  for (int j = threadIdx.x; j < len; j += 256) adamw_element<kEma>(param, grad, m, v, ema, begin + j, k, false);
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

