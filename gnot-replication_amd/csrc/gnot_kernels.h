// Internal (C++) launcher interface between the engine and the HIP kernels.
// The public C-ABI lives in include/gnot_hip.h; nothing here crosses the library boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnot {

// ------------------------------------------------------------------ weight packing (pack.hip)
// One Linear (W [out, in] row-major, bias [out]) written into the fragment-order image used as the
// MFMA A operand (see gnot_common.h).  transposed=0: A = W   (forward, out = x W^T + b)
//                                       transposed=1: A = W^T (backward data, dx = dy W)
// Tile (o, T) of this matrix lands at dst[((o0 + o) * ktot + t0 + T) * 64 + lane] (float4 units), so
// several Linears can be concatenated along either dimension of one packed matrix.
struct PackJob {
  const float* W;
  const float* b;      // may be null; only used when bias_dst != null
  float4* dst;
  float* bias_dst;     // padded bias copy (16*OTp floats, zero filled), or null
  int out, in;
  int transposed;
  int o0, t0, ktot;
  int OTp, KTp;        // tile counts of this job's image (>= what out/in need; the rest is zero)
  int x6;              // 1: bf16x6 image (3 bf16 pieces per 16x32 block, k-major, gnot_common.h); 2: the
                       //    same output-major (chain2.hip); 3: output-major, 1 RNE bf16 piece; 4: k-major,
                       //    1 RNE bf16 piece (chain.hip in the bf16 mode); 0: fp32
  int otot;            // x6: output tiles of the whole image (its k-major block stride)
  // padded heads (a head width d / H that is not a multiple of 4): W's rows come in H heads of hr real rows,
  // the image holds them in heads of hp >= hr (row h * hp + j <- W row h * hr + j, j < hr; the rest zero).
  // out is then H * hp.  Applies to the image rows (forward) or the contraction index (transposed) and to
  // the bias copy.  0: rows map 1:1
  int hr = 0, hp = 0;
  // internal widths above 512 (fp32 images): the contraction in two halves of kh tiles, each half a whole
  // image of its own -- tile (o, T) at ((T / kh) * otot + o) * kh + T % kh -- so that a projection runs as two
  // K-segments of the 320 .. 512-wide kernels (launch_linear).  0: one image, ktot tiles deep
  int kh = 0;
};
// pack tiles of a job: fp32 images have OTp*KTp tiles, x6 images OTp*ceil(KTp/2) blocks
inline int pack_tiles(const PackJob& J) { return J.x6 ? J.OTp * ((J.KTp + 1) / 2) : J.OTp * J.KTp; }
hipError_t launch_pack(const PackJob* jobs_dev, const int* tile_prefix_dev, int njobs,
                       int total_tiles, hipStream_t s);

// ------------------------------------------------------------------ tuning switches (tuning.cpp)
// The plan's switches, read from the environment ONCE, when the plan is created (gnot_plan_create; microbench.cpp
// for its own launches): a plan's kernel forms and workspace layout never change with the environment afterwards.
struct Tuning {
  int wgrad_overlap = -1;               // GNOT_WGRAD_OVERLAP: 0 serial / 1 forked weight gradients; -1 (unset): by size
  bool moe_stored = false;              // GNOT_MOE_STORED_STREAMS=1: the stored soft-MoE row streams
  // GNOT_STATE_MFMA_MIN: state_mfma_kernel only from this many points in a state group; below it the 256-point
  // MFMA workgroups leave most CUs idle and the 64-point VALU kernel is faster (configs[1], 10k points: 3.60 vs
  // 3.94 ms per step)
  long state_mfma_min_points = 65536;
  // GNOT_APPLY_MFMA_MIN: the fp32-MFMA attention passes only from this many 64-point chunks; below it they run
  // fewer than ~128 workgroups, each staging the state images before its few chunks, and the VALU kernels are
  // faster (configs[1], 10k points: apply bwd 23 vs 70 us per call)
  int apply_mfma_min_chunks = 512;
};
Tuning tuning_from_env();

// ------------------------------------------------------------------ projections (linear.hip)
enum LinearEpi { EPI_STORE = 0, EPI_ACCUM = 1 };
constexpr int kMaxSeg = 8;
struct LinearArgs {
  int nseg;                          // K-segments: Y = sum_s X[s] . A_s (+ bias)
  const float* X[kMaxSeg];           // segment input rows X[s] + p*ldx, K columns each
  const float4* Wp[kMaxSeg];         // segment packed A images (NO/16 x ceil(K/16) tiles)
  long ldx;
  int nsum;                          // segment 0 only: input = sum_{t<nsum} X[0][t*sum_stride + ...]
  long sum_stride;
  int K;                             // real input columns (<= D)
  const float* bias;                 // padded bias or null
  float* Y;
  long ldy;
  int NO;                            // output columns (multiple of D)
  int P;                             // rows
  int epi;                           // LinearEpi
  int nsoft;                         // feature-softmax on output columns [0, nsoft)
  int dh;                            // head width for that softmax
  int np = 3;                        // linear2: operand pieces (3 = bf16x6, 1 = bf16 mode)
  // linear.hip: 0 = fp32 fragment images on the fp32 MFMA (widths 16 and 320 .. 512); 1 / 3 = output-major
  // bf16-piece images (d <= 192: the bf16 mode / the fp32 mode's bf16x6).  The plan's rule: gnot_plan::lin_img
  int img = 0;
  // padded hidden width (the plan runs a real width dr < D in tiles of D, engine.cpp gnot_plan_create):
  // output column c with c % D >= dreal is written as 0 (the softmax of a head's features must not leak
  // into the pad columns, which the next kernels read as exact zeros); 0 = no pad columns
  int dreal = 0;
  // padded heads: heads of dh internal features of which the first dhr are real; the feature softmax
  // excludes (and writes 0 to) the others.  0: every feature of a head is real
  int dhr = 0;
  int ncol = 0;                      // store only output columns [0, ncol) (row pitch ldy < NO); 0 = all NO
  // the width of the output blocks dreal / dhr repeat in (the internal width); 0 = the kernel's K width D.
  // Set by launch_linear's K-split, whose kernels run at half the internal width
  int dblk = 0;
  int kcols[kMaxSeg] = {};           // per-segment input columns when they differ (K-split); 0 = K
};
// D: the K width the kernel is instantiated at (the internal width for the projections, a layer's input
// tiles x 16 for the chains).  img = 0 runs at D = 16 and 320 .. 512 only (what a plan reaches: chainw.hip's
// Linears and the d > 256 projections); any other width is hipErrorInvalidValue.  D in (512, 1024] (a multiple of 128): the contraction runs as two K-halves of
// every segment on the D / 2 kernels -- X[s] + D / 2 for the second half and an image made of two half
// images (PackJob::kh), the second (NO / 16) x (D / 32) tiles after the first -- in launches of at most
// kMaxSeg segments (later ones accumulate; a softmax epilogue must fit one launch); a.K must then be D
hipError_t launch_linear(const LinearArgs& a, int D, hipStream_t s);
// output tiles per workgroup of linear.hip for an NO-column projection with a softmax epilogue over its
// first nsoft columns in heads of dh (-1: no tiling keeps whole heads per workgroup)
int linear_oc(int D, int NO, int nsoft, int dh);
// d = 256 projections on bf16x6 MFMA (linear2.hip): Wp[s] are OUTPUT-MAJOR x6 images (pack x6 = 2)
bool linear2_supported(const LinearArgs& a, int D);
hipError_t launch_linear2(const LinearArgs& a, hipStream_t s);
// jobs_dev: device array of independent LinearArgs (same D and NO), one per grid.z
hipError_t launch_linear_batch(const LinearArgs* jobs_dev, int njobs, int maxP, int NO, int D, int dh, hipStream_t s);

// ------------------------------------------------------------------ fused MLP chains (chain.hip)
enum ChainMode { CH_STORE = 0, CH_SOFTMAX = 1, CH_MOE = 2 };
// points per workgroup of the d = 256 chain kernels (chain2.hip: 16 per wave): one block of the soft-MoE
// expert grid
constexpr int kC2Rows = 128;
struct ChainLayer {
  const float4* Wp;    // packed forward weights of this layer
  const float4* WpT;   // packed transposed weights (backward)
  const float* bias;   // padded bias
};
struct ChainArgs {
  int D;               // hidden width
  int KT0, OTL;        // input / last-output tile counts (1 or D/16)
  int nlin;            // number of Linears (>= 2)
  int in_dim, out_dim;
  int P;
  int nchains;         // grid.y
  const ChainLayer* layers;          // device table [nchains * nlin]
  // d > 256 (chainw.hip, one Linear at a time): the same table in host memory and 2 * P * D floats of
  // scratch (the activations between two Linears)
  const ChainLayer* layers_host = nullptr;
  float* scratch = nullptr;
  // forward
  const float* X; long ldx;          // chain input (shared by all chains)
  float* Y; long ldy; long y_chain_stride;   // output (CH_STORE/CH_SOFTMAX) or MoE stage
  const float* scores; int ldsc;     // CH_MOE: expert weights scores[p*ldsc + chain]; CH_SOFTMAX bwd: s
  int mode;
  float* save; long save_layer_stride; long save_chain_stride;  // pre-activations [P, D] per layer (ld D)
  // backward
  const float* dY; long lddy;        // incoming grad (CH_STORE: [P,out]; CH_MOE: dquery [P,D]);
  float* dscore;                     // CH_MOE: dscore[p*ldsc + chain] += dq . y ; CH_SOFTMAX: d(scores)
  float* dz; long dz_layer_stride; long dz_chain_stride;          // per layer dZ [P, D] for wgrad
  // CH_MOE, d = 256, fp32: dz_{nlin-1} = s_e dq is not stored (the weight gradients of the last Linear read
  // dq and scale it themselves, WgradJob::scale)
  int skip_dz_last = 0;
  float* dX; long lddx; long dx_chain_stride;                     // chain input grad or null
  int np = 3;                        // d = 256: operand pieces (3 = bf16x6 fp32-exact, 1 = bf16 mode)
#ifdef GNOT_DIAG_STAMP
  unsigned long long* dbg = nullptr;  // diagnostic builds: per-wave stamp sums (x6_core.h C2Pipe)
#endif
  int grid_mode = 0;                 // set by the launcher (chain2.hip c2_grid_pos)
  // CH_MOE, d = 256, np = 1 (bf16 mode): bf16 activation storage.  Saves and dZ are bf16 "pair-
  // interleaved" rows (gnot_common.h, 512 B per point; strides above then count 4-byte units, so a
  // [P, 256] bf16 layer is P * 128 of them).  Per chain, save slots 0 .. nlin-2 hold gelu'(h_l) of the
  // GELU layers (the backward's factor, computed with gelu(h_l) in the forward), slot nlin-1 the expert's
  // bf16 score-scaled term s y (the stage row the combine sums; the backward's d score = dq . (s y) / s),
  // slots nlin + l the RNE bf16 input of Linear l (= gelu(h_{l-1}), the
  // MFMA operand the forward used), written for the weight gradients; slot nlin + 0 (the shared MoE
  // input) only in chain 0.
  int b16s = 0;
  // b16s expert grid: the stage terms (forward s_e y_e, backward dX_e) go to the [E, P, d] stage as bf16
  // pair-interleaved rows (the strides are the fp32 stage's), summed by launch_moe_combine_b16
  int stage_b16 = 0;
};
// d > 256: chains one Linear at a time (linear.hip + elementwise passes, chainw.hip)
hipError_t launch_chainw(const ChainArgs& a, bool bwd, hipStream_t s);
hipError_t launch_chain_fwd(const ChainArgs& a, hipStream_t s);
hipError_t launch_chain_bwd(const ChainArgs& a, hipStream_t s);
// d = 256 chains (chain2.hip): bf16x6 in both directions, output-major x6 images (pack x6 = 2) for Wp
// AND WpT
hipError_t launch_chain2(const ChainArgs& a, bool bwd, hipStream_t s);

// ------------------------------------------------------------------ point-reduction GEMM (wgrad.hip, state.hip)
// One job of a point reduction.  Weight gradients (wgrad.hip): dW[out, in] = sum_p dz[p, :out]^T x[p, :in] over the
// job's points, db = the column sums of dz.  Attention states (state.hip): the same sums per head, see below.
// (alignas(16): 128 bytes per job, so that in the device tables -- 256-byte aligned, engine.cpp bind -- no job
// straddles a 128-byte line and the kernels' scalar loads of its fields stay aligned)
struct alignas(16) WgradJob {
  const float* dz; long lddz;        // A rows [P, out]
  const float* x;  long ldx;         // B rows [P, in]
  int x_gelu;                        // 1: B = gelu(x) (x is a saved pre-activation)
  int out, in;
  int ldscale;                       // stride (floats) between two points' scale
  float* dW;                         // [out, in] row-major, or the state [H][dh*dh + dh] (state_dh > 0)
  float* db;                         // [out] column sums of A, or null
  const float* w; long ldw;          // state jobs: optional per-(point, head) weight of the column sums
  int pad0_;                         // (keeps every field's offset and the 128 bytes)
  int state_dh;                      // state jobs: the head width dh (> 0); weight-gradient jobs: 0
  int pad1_;
  int P;
  int tiles_o, tiles_i;              // 128x128 output tiles
  int splits;                        // split-K count over points
  long slab_off;                     // offset (floats) of this job's partial slabs
  // optional per-point scale of the A rows (wide 256 x 256 kernel only): A[p, :] = scale[p * ldscale] * dz[p, :],
  // one rounded fp32 multiply before the mask, the column sums and the split.  The soft-MoE calls' last Linear:
  // dz = dquery (shared by the E experts), scale = the expert's score column -- the rows s_e dq the chain
  // backward would otherwise store per expert (ChainArgs::skip_dz_last)
  const float* scale;
};
static_assert(sizeof(WgradJob) == 128, "WgradJob: one 128-byte line per job");
// A group's device tables: its jobs, the per-job prefix sums of workgroups and of reduce elements, and (the
// balanced form of the two one-workgroup-per-split kernels, optional) per-workgroup point ranges -- workgroup w runs
// segs[seg_start[w] .. seg_start[w+1]) = {job, slab slot, first point, end point}; each job's `splits` then counts
// the ranges that touch it (slots 0 .. splits-1)
struct WgradTables {
  const WgradJob* jobs = nullptr;
  int njobs = 0;
  const int* wg_prefix = nullptr;    // [njobs]
  int total_wgs = 0;
  const int* red_prefix = nullptr;   // [njobs]; weight gradients: ntile * 128 * 129 elements per job
  int total_red = 0;
  const int4* segs = nullptr;
  const int* seg_start = nullptr;
};
// The weight-gradient kernels (all bf16 MFMA, one slab layout, one reduce):
enum class WgradKernel {
  Tile128,   // any out / in: one workgroup per (job, 128 x 128 tile, split)
  Wide256,   // out, in <= 256 (d = 256): one workgroup per (job, split) owns the whole gradient
  Wide128,   // out, in <= 128 (d <= 128): the same design at a 128 x 128 output
  B16Rows,   // bf16-storage jobs (ChainArgs::b16s): dz and x are bf16 pair-interleaved rows [P, 256] (x already
             // the Linear's input, no GELU), out = in = 256, one workgroup per (job, split)
};
// np: operand pieces of the fp32-row kernels (3 = bf16x6, 1 = the bf16 mode); B16Rows ignores it
// scaled: the group holds jobs with WgradJob::scale (Wide256 at np = 3 only, else hipErrorInvalidValue): the
// kernel instantiation that stages them; a scale in any other launch is ignored
// accumulate: the split-K finish adds its sum onto dW / db instead of overwriting them (per launch, not in
// the job tables: one bound plan overwrites in one backward and accumulates in the next)
// segs / seg_start: Wide256 and B16Rows only
hipError_t launch_wgrad(WgradKernel kind, const WgradTables& t, float* slab, int np, bool scaled, bool accumulate,
                        hipStream_t s);

// ------------------------------------------------------------------ attention states (state.hip)
// Jobs are WgradJobs with state_dh > 0: A = dz/lddz, B = x/ldx, optional w/ldw, out = dW as
// [H][dh*dh + dh], `splits` partials of state_pts(d) points each at slab + slab_off.  state.hip has its own
// partial-state kernels and its own reduce (always overwrites); it reads the tables' jobs and two prefixes.
// Two kernels: state_mfma (fp32 MFMA, rows straight from HBM, dh = 16/32/64 with H % 4 == 0;
// below Tuning::state_mfma_min_points points the VALU form) and the VALU state_partial (LDS-staged rows, any width).
// (the instantiated state_mfma_kernel<DH, HPW> forms, HPW = heads per wave = d / dh / 4: 1 / 2 / 4 at dh 16 and
// 32, 1 / 2 at 64; any other head count runs the VALU kernel -- round 6: 12 heads of 16 at d = 192 used to pass
// this test and fail the launch on meshes past the threshold)
inline bool state_mfma_ok(int d, int dh) {
  if (!((dh == 16 || dh == 32 || dh == 64) && d % dh == 0 && (d / dh) % 4 == 0)) return false;
  const int hpw = d / dh / 4;
  return hpw == 1 || hpw == 2 || (hpw == 4 && dh <= 32);
}
// points per partial-state workgroup: 256 on MFMA (4 waves per SIMD at 262k points, partials ~6 % of
// the row bytes); VALU: the workgroup's A and B rows fill <= 32 KiB of LDS each (64 at d <= 128,
// 8192 / d above; measured: 32 and 16 are slower at cfg2)
inline int state_pts(bool mfma, int d) { return mfma ? 256 : d <= 128 ? 64 : 8192 / d; }
// d: row width, pts: points per workgroup, nw: per-point weights (0 or H), mfma: state_mfma_kernel (state_mfma_ok)
hipError_t launch_state(const WgradTables& t, float* slab, int d, int dh, int pts, int nw, bool mfma, hipStream_t s);

// ------------------------------------------------------------------ attention (attn.hip)
struct AttnApplyArgs {
  const float* q; long ldq;          // post-softmax q, point-major
  int nsrc;                          // number of (S, z) sets to average (I, or 1 for self)
  const float* state[8];             // [B][H][dh*dh + dh] per source
  const int4* chunks; int nchunks;
  const long* off;                   // [B+1] sample offsets (device)
  int H, dh;
  float* res;                        // [P, d] head-major per sample (the scramble)
  // padded heads: the scramble holds heads of dhr real features (element (h, n, j) at (h N_b + n) dhr + j,
  // j < dhr), while q / states / du / dq run heads of dh (pad features zero).  0: dhr = dh
  int dhr = 0;
  // backward
  const float* dres;                 // [P, d] head-major per sample
  float* dq_pre; long lddq;          // grad wrt pre-softmax q, point-major
  float* du[8]; long lddu;           // per source du, point-major
  float* dden[8];                    // per source [P, H]
};
struct AttnKVBwdArgs {
  const float* k; const float* v; long ldkv;   // post-softmax k, v (point-major)
  const float* dstate;               // [B][H][dh*dh + dh]  (dS, dz)
  const int4* chunks; int nchunks;
  int H, dh;
  float* dk; float* dv; long lddkv;  // pre-softmax dK, dV
};
// The kernel form of an attention pass.  The plan chooses it once per batch geometry (attn_kernel, stored by
// gnot_plan_set_batch); the launchers run the form they are given and return hipErrorInvalidValue for one the
// arguments cannot run -- there is no fallback
enum class AttnKernel {
  Narrow,   // attn.hip's DH-templated VALU kernels: dh <= 64, a multiple of 4
  Wide,     // attn.hip's NB-templated VALU kernels: 64 < dh <= 256, a multiple of 4
  Mfma,     // attn_mfma.hip, fp32 MFMA: dh = 16 / 32 / 64, 4-aligned pitches, the state images within 160 KiB of LDS
};
enum class AttnPass { ApplyFwd, ApplyBwd, KVBwd };
// The form of one pass (attn_mfma.hip), a function of shapes and the threshold alone.  Mfma where all of these
// hold: dh is 16, 32 or 64; the heads are not padded (dhr is 0 or dh; the K/V backward's rows are whole internal
// heads, it ignores dhr); the images of nsrc sets of states (1 .. 8; the K/V backward: 1) fit the LDS; aligned4:
// every row pitch the pass uses (apply forward: ldq; backward: ldq, lddq, lddu; K/V: ldkv, lddkv) is a multiple
// of 4; the pass has at least min_chunks (Tuning::apply_mfma_min_chunks) 64-point chunks, the batched K/V
// backward counting maxchunks * njobs.  Otherwise Wide above a head width of 64 and Narrow up to it
AttnKernel attn_kernel(AttnPass pass, int dh, int dhr, int H, int nsrc, long nchunks, bool aligned4, int min_chunks);
hipError_t launch_attn_apply(AttnKernel form, const AttnApplyArgs& a, bool bwd, hipStream_t s);
// K/V backward: one job (a), or the independent jobs of jobs_dev (every block x input function, a == null) in
// one launch, job = grid.z, maxchunks the largest chunk count among them; H and dh are those of every job
hipError_t launch_attn_kv_bwd(AttnKernel form, const AttnKVBwdArgs* a, const AttnKVBwdArgs* jobs_dev, int njobs,
                              int maxchunks, int H, int dh, hipStream_t s);

// ------------------------------------------------------------------ small elementwise (misc.hip)
hipError_t launch_concat_theta(const float* x, long ldx, int in_dim, const float* theta, int th_dim,
                               const long* off, int B, float* xin, long ldxin, int P, hipStream_t s);
// out = (base ? base : 0) + sum_e stage[e]
hipError_t launch_moe_combine(const float* base, const float* stage, long stage_stride, int E,
                              float* out, long n, hipStream_t s);
// out[p, :] = base[p, :] + sum_e scores[p * ldsc + e] * y[e * y_stride + p * D + :] in expert order, each
// product its own rounded fp32 multiply (gnot_common.h mul_rn): the bits of moe_combine over the stage rows
// s_e y_e a CH_MOE chain forward writes, from the experts' saved outputs y_e (save slot nlin-1) instead.  D a
// multiple of 4
hipError_t launch_moe_combine_scaled(const float* base, const float* y, long y_stride, const float* scores, int ldsc,
                                     int E, float* out, long P, int D, hipStream_t s);
// the same over bf16 pair-interleaved stage rows (ChainArgs::stage_b16: 512 B per point at the start of each
// expert's fp32-sized region, stage_stride in floats); base / out fp32 [P, 256]
hipError_t launch_moe_combine_b16(const float* base, const float* stage, long stage_stride, int E, float* out,
                                  long P, hipStream_t s);
// out[r][c] = a[r][c] + b[r][c] (b null: a copy), c < cols, out dense [rows, cols]
hipError_t launch_add_cols(const float* a, long lda, const float* b, long ldb, int cols, float* out, long rows,
                           hipStream_t s);
// out[b][t] = sum over rows [off[b], off[b+1]) of a[row][c0 + t], t < ncols (fixed order)
hipError_t launch_seg_colsum(const float* a, long lda, int c0, int ncols, const long* off, int B, float* out,
                             hipStream_t s);
// Fourier embedding of order n in [1, 8] (fourier.hip), W = 4 n + 3: src [rows, C] (pitch lds) -> dst [rows, ld],
// channel c as columns c W .. c W + W - 1 = [v, cos(2^(k-n) v), sin(2^(k-n) v)], k = 0 .. 2 n; columns C W .. ld - 1
// zeros.  The backward reads cos / sin from the embedded rows emb and the gradient as ga + gb (gb may be null):
// dv [rows, C] dense
hipError_t launch_fourier_embed(const float* src, long lds, int C, int n, float* dst, long ld, long rows,
                                hipStream_t s);
hipError_t launch_fourier_embed_bwd(const float* emb, long ld, const float* ga, long ldga, const float* gb, long ldgb,
                                    int C, int n, float* dv, long rows, hipStream_t s);
// Parameter-free LayerNorm over the C <= 1024 real columns of a row (norm.hip), one wave per row.  Forward:
// y[r, :C] = (x[r, :C] - mean) / sqrtf(var + eps), columns C .. ldy - 1 zeros, input pad columns masked, rstd [rows]
// kept unless null.  Backward from the saved y and rstd: dx = rstd (dy - mean(dy) - y mean(dy y)), stored (pad
// columns zeros) or, accumulate != 0, added onto dx (pad columns untouched); dx may alias dy.  Pitches: multiples
// of 4 that are at least C, below 2^31; pointers 16-byte aligned
hipError_t launch_layer_norm(const float* x, long ldx, long rows, int C, float eps, float* y, long ldy, float* rstd,
                             hipStream_t s);
hipError_t launch_layer_norm_bwd(const float* y, long ldy, const float* rstd, const float* dy, long lddy, long rows,
                                 int C, float* dx, long lddx, int accumulate, hipStream_t s);
// Keyed dropout in place on [rows, ld] rows of C <= 1024 real columns (dropout.hip), one wave per row: element
// (r, c) is kept and scaled iff word c % 4 of Philox4x32-10((n, b, site << 8 | c / 4, key[2]), (key[0], key[1])) is
// at least T, else +0; b the row's sample in off [B + 1], n = r - off[b] + glo[b]; key: 4 uint32 in device memory,
// read when the kernel runs.  T = 0: no launch.  Columns C .. ld - 1 are untouched
hipError_t launch_dropout_rows(float* x, long ld, long rows, int C, const long* off, const long* glo, int B,
                               const uint32_t* key, uint32_t site, uint32_t T, float scale, hipStream_t s);
// test hook: y = gelu(x), dy = gelu_grad(x), (y2, dy2) = gelu_and_grad(x) over n contiguous floats
hipError_t launch_debug_gelu(const float* x, float* y, float* dy, float* y2, float* dy2, long n, hipStream_t s);
// segmented copy: dst[seg.dst + i] = src[seg.src + i], i < seg.len (floats); reverse swaps the roles of
// src/dst offsets.  unit 4: every offset and length a multiple of 4 (float4 copies), unit 1: any.  prefix:
// prefix sums of the lengths in units [nseg + 1], total = prefix[nseg].
struct CopySeg {
  long a, b, len;      // a = source offset, b = destination offset (forward direction)
};
hipError_t launch_segcopy(const CopySeg* segs, const int* prefix, int nseg, int total, const float* src, float* dst,
                          bool reverse, hipStream_t s, int unit = 4);

// ------------------------------------------------------------------ training step (train.hip)
// the 2048-row splits of the longest sample (at least 1)
int rel_l2_splits(const long* off_host, int B);
// every loss, one kernel family: kind = GNOT_LP_* (0 rel2, 1 rel1, 2 relinf, 3 mse, 4 l1, 5 linf), checked by the
// caller; gnot_rel_l2_loss / gnot_mse_loss are kinds 0 / 3 with w == terms == nullptr.  w (C component weights),
// terms ([B][C], the unweighted terms) and dpred may be null, dpred must be for relinf / linf.  stats != nullptr
// (a stats block {mean[C], std[C], rstd[C]}, stats.hip): the loss of pred * std[c] + mean[c] and its gradient
// times std[c]; nullptr: the plain loss.  work: B*nsplit*kW*C + B*C floats (nsplit = rel_l2_splits; kW = 2 for
// the relative kinds 0-2, else 1).  A sample without rows makes sense for rel2 alone (its term is a NaN).
// point_w != nullptr (one weight >= 0 per packed row, device [rows]): the weighted terms of gnot_lp_loss_weighted,
// rows of weight zero not read; kW is then 2 for every kind but linf (mse / l1 carry sum w).  nullptr: the
// unweighted kernels, untouched.
hipError_t launch_lp(int kind, const float* pred, const float* tgt, const float* point_w, const long* off_dev, int B,
                     int C, int nsplit, long rows, const float* w, const float* stats, float* work, float* loss,
                     float* terms, float* dpred, hipStream_t s);
// stage-1 partial sums of sum g^2 over n elements (a function of n alone); 0 for n < 1
long grad_clip_partials(long n);
// work: grad_clip_partials(n) floats; clip: 2 floats {norm, coefficient}
hipError_t launch_grad_clip(const float* grad, long n, const float* hyper, float max_norm, float* work, float* clip,
                            hipStream_t s);
// the same two stages without a max_norm: clip = {norm (launch_grad_clip's bits), 1.0f}
hipError_t launch_grad_norm(const float* grad, long n, const float* hyper, float* work, float* clip, hipStream_t s);
// ema = fma(weight[0], param - ema, ema); n >= 1, ema and param distinct arrays
hipError_t launch_ema_update(float* ema, const float* param, long n, const float* weight, hipStream_t s);
// AdamW on the gradient (grad[i] * hyper[7]) * clip[1], every variant in one kernel.  clip == nullptr: no
// coefficient (the plain update).  guard != nullptr (needs clip, n >= 1): nothing but guard (2 ints {skipped
// count, skipped now}) is written when clip[0] is NaN or +-inf.  ema != nullptr: launch_ema_update's pass on the
// stored parameter fused in; hyper then has 9 floats, hyper[8] the EMA weight.  n <= 0 launches nothing.
hipError_t launch_adamw_update(float* param, const float* grad, float* m, float* v, float* ema, long n,
                               const float* hyper, const float* clip, int* guard, hipStream_t s);
// The slice-table forms (gnot_adamw_step_groups, gnot_grad_norm_groups, gnot_grad_clip_groups).  slices: device
// rows of three longs {begin, len, group}, 1 <= len <= 8192, validated by the caller; nslices >= 1, one workgroup
// per row; nothing outside the rows is read or written.
// The norm stages over the rows' elements: work nslices floats, clip as above; norm_only: no max_norm, clip[1] = 1
hipError_t launch_grad_norm_slices(const float* grad, const long* slices, long nslices, const float* hyper,
                                   float max_norm, int norm_only, float* work, float* clip, hipStream_t s);
// launch_adamw_update's element expression with lr = hyper[0] * ghyper[group][0] and weight_decay =
// ghyper[group][1] (ghyper: device, two floats per group)
hipError_t launch_adamw_groups(float* param, const float* grad, float* m, float* v, float* ema, const float* hyper,
                               const float* ghyper, const long* slices, long nslices, const float* clip, int* guard,
                               hipStream_t s);


// ------------------------------------------------------------------ batch assembly (gather.hip)
// table: one row of kGatherCols longs per segment {src_row0, n, dst_row0, k, key_lo, key_hi}; dst row
// dst_row0 + j = src row src_row0 + j (k == n) or src_row0 + pi(j; n, key) (k < n), 0 <= j < k.
// rows = sum of k >= 1; the table is validated by the caller (gnot_gather_rows).  stats != nullptr: every value
// is written as (s - mean[c]) * rstd[c] from the stats block {mean[C], std[C], rstd[C]}; nullptr: the plain copy
constexpr int kGatherCols = 6;
hipError_t launch_gather_rows(const float* src, int C, const long* table, int B, const float* stats, float* dst,
                              long rows, hipStream_t s);

// ------------------------------------------------------------------ channel statistics (stats.hip)
// stage-1 slices over `rows` rows (a function of rows alone); 0 for rows < 1
long channel_stats_slices(long rows);
// stats = {mean[C], std[C], rstd[C]} of src [rows, C] (unbiased std, rstd = 1 / (std + eps); a constant channel:
// std 0, rstd 1).  work: channel_stats_slices(rows) * 3 * C floats; rows >= 1, C >= 1
hipError_t launch_channel_stats(const float* src, long rows, int C, float eps, float* work, float* stats,
                                hipStream_t s);
// the same block with a weight w[r] >= 0 per row (device [rows]): mean = sum w x / sum w, the reliability-weights
// variance (divisor sum w - sum w^2 / sum w; not positive: a constant channel), rows of weight zero not read.
// work: channel_stats_slices(rows) * (2 + 3 * C) floats
hipError_t launch_channel_stats_weighted(const float* src, const float* w, long rows, int C, float eps, float* work,
                                         float* stats, hipStream_t s);

}  // namespace gnot
