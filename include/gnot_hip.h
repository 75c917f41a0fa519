/* gnot_hip.h — C ABI of the MI355X-native GNOT core (libgnot_hip.so).
 *
 * Drop-in boundary for the reference's hot path: `GNOT.forward` (reference model.py:154-173) and the
 * backward that `loss.backward()` (main.py:102) runs through it.  The reference is pure PyTorch and
 * has no FFI; these entry points are what its `GNOT` module binds in our host mirror
 * (gnot-replication_amd/gnot_amd/model.py, via ctypes — see INTEGRATION.md):
 *
 *   reference                                   replaced by
 *   GNOT.__init__(...)            model.py:143   gnot_plan_create (same 12 constructor arguments)
 *   nn.Linear parameters          model.py:9-14, 43-51  gnot_plan_bind_params (state_dict order)
 *   padding / batching       utils.py:3-4, main.py:60-89  gnot_plan_set_batch (packed offsets)
 *   GNOT.forward                  model.py:154-173  gnot_forward
 *   autograd backward             main.py:102    gnot_backward
 *
 * Conventions: plain pointers and sizes only, no torch types.  All device memory (inputs, outputs,
 * parameters, the workspace) is allocated and owned by the caller; the library never allocates
 * device memory.  Every compute entry point is asynchronous and stream-ordered on the hipStream_t
 * it is given (pass NULL for the default stream), launches kernels only (graph-capturable) and
 * returns 0 on success or a negative GNOT_E* code; gnot_last_error() then describes the failure.
 */
#ifndef GNOT_HIP_H
#define GNOT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gnot_plan gnot_plan; /* opaque */

/* GNOT constructor arguments, reference model.py:143 (positional order of main.py:44).
 * n_attn_hidden_dim, n_mlp_hidden_dim and n_input_hidden_dim must be equal (the reference's
 * residual adds, model.py:131/137, require it); any d and n_head with d/n_head up to 256 whose internal width
 * is at most 1024: a head width that is not a multiple of 4 runs on heads padded to one (n_head x that many
 * internal columns), and the internal width is the next multiple of 16 up to 192, 256 (heads of 16 / 32 / 64 /
 * 128 / 256, unpadded), the next multiple of 64 up to 512, else the next multiple of 128 (heads dividing 64),
 * with exact-zero pad columns; parameters, gradients and outputs keep d.
 * input_dim, input_dim + theta_dim, out_dim and n_expert are in [1, d]; input_func_dim is at most d and, when
 * n_input_functions > 0, at least 1; theta_dim may be 0 (theta is then [B, 0]: gnot_forward takes a null theta
 * and gnot_input_grads writes no dtheta), never negative; n_input_functions is in [0, 8]; n_attn_layers >= 0
 * (0: encoder and decoder only, the input functions then do not reach the output and their gradients are
 * zero); n_mlp_num_layers <= 1 gives two Linears per MLP.  GNOT_E_INVALID otherwise. */
typedef struct gnot_config {
  int input_dim;
  int theta_dim;
  int input_func_dim;
  int out_dim;
  int n_attn_layers;
  int n_attn_hidden_dim;
  int n_mlp_num_layers;
  int n_mlp_hidden_dim;
  int n_input_hidden_dim;
  int n_expert;
  int n_head;
  int n_input_functions;
} gnot_config;

enum {
  GNOT_OK = 0,
  GNOT_E_INVALID = -1,     /* bad argument / unsupported configuration */
  GNOT_E_HIP = -2,         /* a HIP runtime call failed */
  GNOT_E_STATE = -3,       /* call out of order (e.g. forward before bind) */
  GNOT_E_WORKSPACE = -4    /* workspace missing or too small */
};

/* Plan lifetime. */
int gnot_plan_create(const gnot_config* cfg, gnot_plan** out);
void gnot_plan_destroy(gnot_plan* plan);

/* Linears in reference state_dict order (named_parameters() order of model.py's GNOT).
 * dims[2*i] = out_features, dims[2*i+1] = in_features. */
int gnot_plan_num_linears(const gnot_plan* plan);
int gnot_plan_linear_dims(const gnot_plan* plan, int32_t* dims);

/* Device pointers of every Linear's weight [out, in] (row-major) and bias [out], fp32, in the order
 * above.  Pointers must stay valid (parameters are updated in place by the optimizer). */
int gnot_plan_bind_params(gnot_plan* plan, const float* const* weights, const float* const* biases);

/* Batch geometry.  x_off: host array [B+1] of point offsets (packed, no padding: sample b owns rows
 * x_off[b] .. x_off[b+1]-1); fn_off: host array [n_input_functions * (B+1)] of the same for every
 * input function.  A zero-padded batch (main.py:60-82) is simply x_off = {0, N, 2N, ...}.
 * training != 0 keeps the activations the backward needs.
 * A sample may have no query points, and an input-function segment no points, as long as the batch has
 * a query point: an empty sample contributes no output rows, a zero d theta row and zero d fn rows
 * (tests/test_gpu_geometry.py).  A sample that HAS query points but an input function with no points is
 * not supported: the reference divides by a zero key sum there (model.py LinearAttention, 1 / (q . sum k))
 * and returns NaN, so the case has no reference and is untested.
 * Limits: fewer than 2^29 points per plan (query points, and points of each input function: the
 * kernels' job tables hold 32-bit point indices; their buffer resources are based per workgroup or per
 * split-K range, so no activation array size bounds a plan).  GNOT_E_INVALID beyond it; the real bound
 * is the workspace (gnot_plan_workspace_bytes) against the device memory. */
int gnot_plan_set_batch(gnot_plan* plan, int B, const int64_t* x_off, const int64_t* fn_off, int training);

/* MoE activation recompute (off by default): training keeps only each MoE call's input and the
 * backward re-runs that call's expert forward (model.py:128/134's ffn1/ffn2 experts) into one shared
 * save buffer just before its chain backward -- the E*nl*P*d saved pre-activations exist once instead
 * of once per MoE call (2 per block), at the cost of one more MoE forward per call.  Changing it
 * invalidates the batch: call gnot_plan_set_batch (and bind) again.  No reference counterpart (a
 * memory option of this library; torch.utils.checkpoint is the analogue). */
int gnot_plan_set_moe_recompute(gnot_plan* plan, int on);

/* Arithmetic mode of the MFMA kernels up to hidden width 256 (MLP chains, attention projections, weight
 * gradients): bf16 == 0 (default) runs them as bf16x6 -- three exact bf16 pieces per fp32 operand, six
 * products, fp32-level results (north_star's 1e-4 bar; the d <= 192 chain backward-data on exact fp32
 * MFMA); bf16 != 0 runs ONE round-to-nearest-even bf16 piece per operand with fp32 accumulation
 * (BASELINE configs[2]'s bf16 training, configs[1]'s "fp32 and bf16"; north_star's 1e-2 bar), and at
 * d = 256 the soft-MoE expert chains keep their training saves, dZ and Linear inputs as bf16 rows (the
 * MoE weight gradients read them directly).  Parameters, the other activations, states, gradients and
 * the attention contractions stay fp32 either way; above d = 256 the mode changes nothing.  Changing it
 * invalidates the batch (set_batch + bind again). */
int gnot_plan_set_precision(gnot_plan* plan, int bf16);

/* Multi-scale Fourier embedding of the inputs (off by default; the original GNOT code's horiz_fourier_dim -- the
 * replicated model.py takes raw inputs).  For an order n >= 1, W = 4 n + 3 and f_k = 2^(k - n), k = 0 .. 2 n,
 * channel c of a row (value v) becomes the W consecutive columns c W .. c W + W - 1
 *     [ v, cos(f_0 v) .. cos(f_2n v), sin(f_0 v) .. sin(f_2n v) ]
 * (channel-major).  nx embeds x (the gating MLP sees the embedded x too; theta is concatenated raw, behind it),
 * nf every input function; 0 means none, orders run 0 .. 8 (GNOT_E_INVALID otherwise).  The gnot_config keeps
 * carrying the EMBEDDED widths -- the Linear shapes, and what the width limits of gnot_config bound: input_dim
 * must be a multiple of 4 nx + 3 and input_func_dim one of 4 nf + 3 (GNOT_E_INVALID otherwise), and the
 * caller's rows have input_dim / (4 nx + 3) and input_func_dim / (4 nf + 3) columns.  gnot_forward then reads
 * x and fns[i] with those raw widths and embeds them as it stages them into the workspace, and
 * gnot_input_grads writes dx and dfns[i] with the raw widths,
 *     dv = g_0 + sum_k f_k (cos(f_k v) g_sin,k - sin(f_k v) g_cos,k)   (g_0 first, then k = 0 .. 2 n),
 * from the embedded rows of the forward: no trigonometry in the backward.  The model IS the reference model
 * of the embedded widths applied to the embedded inputs; parameters, gradients and theta are untouched.
 * Call after gnot_plan_create and before gnot_plan_set_batch; changing an order invalidates the batch
 * (set_batch + bind again). */
int gnot_plan_set_fourier(gnot_plan* plan, int nx, int nf);

/* Parameter-free pre-norm of the attention inputs (the original GNOT code's LayerNorms ln1 .. ln5, which the
 * replicated model.py dropped; no gamma / beta: in front of a Linear they fold into its W and b, so the
 * parameter list, the gradient arena and every checkpoint key stay the reference's).  With on != 0 and
 * LN(h) = (h - mean) / sqrtf(var + eps) over the n_attn_hidden_dim real features of a row (biased variance),
 * a block (model.py:126-139) becomes
 *     query1 = query  + sum_e s_e ffn1_e( cross_attention(LN(query),  [LN(enc_i)]) )
 *     query2 = query1 + sum_e s_e ffn2_e( self_attention (LN(query1)) )
 * Without input functions cross attention takes LN(query) as query and as key/value source (model.py:88-104).
 * LN(enc_i) has no parameters and is computed once per input function for every block.  The residual stream,
 * the gating, the encoders, the decoder and the softmaxed-q residual inside the attention are unchanged.  The
 * backward pulls the projections' input gradients through the norm from the saved rows and their rstd (no
 * statistics recomputed); every mode of the plan (sharding, MoE recompute, bf16 arithmetic -- the norm stays
 * fp32 --, gradient accumulation, graph capture) works as without it.  gnot_debug_buffer names: "b{l}.n1",
 * "b{l}.n2" [P, D], "fnn{i}" [Q_i, D], and in training "b{l}.r1", "b{l}.r2", "fnr{i}" (rstd per row), "dnorm".
 * eps must be finite and positive (GNOT_E_INVALID otherwise; 1e-5 is torch's default).  Call after
 * gnot_plan_create and before gnot_plan_set_batch; a change invalidates the batch (set_batch + bind again). */
int gnot_plan_set_pre_norm(gnot_plan* plan, int on, float eps);

/* Keyed dropout on the attention outputs (off by default; the original GNOT code's resid_drop1 / resid_drop2,
 * which the replicated model.py dropped).  With p > 0 every attention call's output rows -- fc_out's result, the
 * input of the block's soft-MoE experts; gnot_debug_buffer "b{l}.a" (cross) and "b{l}.bb" (self) -- are masked in
 * place right after fc_out, and in the backward the gradient of those rows is masked with the same mask right
 * before fc_out's backward.  No mask is stored: element (point n of sample b, column c) of call site
 * s = 2 l (cross attention of block l) or 2 l + 1 (self attention) is kept iff word c % 4 of
 *     Philox4x32-10( counter = (n, b, s << 8 | c / 4, step), key = (seed_lo, seed_hi) )
 * is at least T = floor(p 2^32 + 0.5) (computed in double), and then multiplied by fp32(2^32 / (2^32 - T));
 * a dropped element becomes +0 whatever it held (a select, not a product).  n counts within the WHOLE sample,
 * so a point-sharded run drops exactly the elements of the unsharded one.  key_dev: 4 uint32 in DEVICE memory,
 * {seed_lo, seed_hi, step, 0}, read when the kernels run (a captured graph drops a fresh mask on every replay
 * once the caller has rewritten it); a backward needs the key its forward ran with.  It must be non-null when
 * T > 0.  p must be finite and in [0, 1) (GNOT_E_INVALID otherwise); T = 0 is off: no launch, no table, the
 * launch sequence of a plan without the call.  Training and inference plans alike.  Call after gnot_plan_create
 * and before gnot_plan_set_batch; a change invalidates the batch (set_batch + bind again).
 * gnot_plan_set_dropout_active: a launch-time switch (it does not invalidate the batch; on once a p is set):
 * gnot_forward drops only while it is on, and gnot_backward mirrors what the last gnot_forward did. */
int gnot_plan_set_dropout(gnot_plan* plan, float p, const uint32_t* key_dev);
int gnot_plan_set_dropout_active(gnot_plan* plan, int on);

/* Input gradients (off by default).  The reference's autograd also differentiates w.r.t. x, theta and
 * the input functions when they require grad (model.py:154-173: x feeds the gating MLP and, through
 * torch.cat with the broadcast theta, the query encoder; the input functions feed their encoder
 * MLPs).  With on != 0 the backward also runs the first Linear's backward-data of those four encoders;
 * gnot_input_grads then writes dx [P, input_dim], dtheta [B, theta_dim] (sums over each sample's
 * points) and dfns[i] [Q_i, input_func_dim] (any pointer may be null: skipped).  Training plans only.
 * With point sharding dx holds this rank's rows, and dtheta / dfns -- one partial per rank, theta being
 * broadcast over all points and the input functions replicated -- are summed over the ranks through the
 * plan's gnot_comm (every rank must call gnot_input_grads).  Changing it invalidates the batch
 * (set_batch + bind again). */
int gnot_plan_set_input_grads(gnot_plan* plan, int on);
int gnot_input_grads(gnot_plan* plan, float* dx, float* dtheta, float* const* dfns, void* stream);

/* Workspace: bytes needed for the current config + batch; bind a device buffer of at least that
 * size (256-byte aligned).  Binding uploads the plan's small device tables: gnot_plan_bind_workspace
 * synchronously; gnot_plan_bind_workspace_async as one copy from pinned staging ordered on `stream`
 * (no host wait -- a per-batch geometry change, main.py:41's shuffled variable-size meshes, costs the
 * host planning (~0.1-0.3 ms) and that copy only).  Either replaces the reference's per-batch
 * padding/mask set-up, main.py:60-82. */
size_t gnot_plan_workspace_bytes(const gnot_plan* plan);
int gnot_plan_bind_workspace(gnot_plan* plan, void* workspace, size_t bytes);
int gnot_plan_bind_workspace_async(gnot_plan* plan, void* workspace, size_t bytes, void* stream);

/* Parameter-gradient arena: offsets (in floats) of every Linear's weight gradient and bias gradient,
 * grad_off[2*i] / grad_off[2*i+1], relative to whichever arena is in use (the workspace's, or the
 * caller's of gnot_plan_set_grad_arena). */
int gnot_plan_grad_offsets(const gnot_plan* plan, int64_t* grad_off);

/* Size of the gradient arena in floats: the sum over gnot_plan_linear_dims of out * in + out.  A function
 * of the config alone, valid from gnot_plan_create on (0 for a null plan). */
int64_t gnot_plan_grad_floats(const gnot_plan* plan);

/* Caller-owned gradient arena.  By default the arena is a buffer of the workspace, which a new batch
 * geometry re-plans (and may move or, with padded widths, clear at bind): gradients summed over several
 * backwards cannot live there.  With arena != NULL (device memory, 16-byte aligned, `floats` >=
 * gnot_plan_grad_floats -- GNOT_E_INVALID otherwise) the weight-gradient jobs, the gradient collectives of
 * gnot_plan_set_grad_comm and gnot_debug_buffer("grads") use the caller's buffer instead, which no
 * set_batch / bind touches; several plans may share one arena.  NULL returns to the workspace arena.  The
 * workspace layout and size are the same either way.  Changing the arena invalidates the batch, like the
 * other setters: set_batch + bind again.  No reference counterpart (torch's .grad tensors play this role). */
int gnot_plan_set_grad_arena(gnot_plan* plan, float* arena, int64_t floats);

/* Re-pack the bound parameters into the kernels' MFMA operand images (call after every optimizer
 * step, before gnot_forward). */
int gnot_pack_weights(gnot_plan* plan, void* stream);

/* Forward (reference GNOT.forward, model.py:154-173).
 * x [P, input_dim], theta [B, theta_dim], fns[i] [Q_i, input_func_dim] (packed, device, fp32,
 * contiguous); out [P, out_dim].  theta may be null when theta_dim = 0.  With gnot_plan_set_fourier x and
 * fns[i] have the raw widths and are embedded on the way into the workspace. */
int gnot_forward(gnot_plan* plan, const float* x, const float* theta, const float* const* fns,
                 float* out, void* stream);

/* The embedding of gnot_plan_set_fourier on its own, for point-by-point tests and for feeding a model of the
 * embedded width (no plan; one launch on `stream`; fp32 device pointers).
 * gnot_fourier_embed: src [rows, C] contiguous -> dst [rows, ld], ld >= C (4 n + 3); column 0 of each channel's
 * block is the input bit for bit, f_k v is an exact product, cos / sin are the full-range single-precision
 * routines, and the pad columns C (4 n + 3) .. ld - 1 are written as zeros.
 * gnot_fourier_embed_bwd: emb [rows, ld] as gnot_fourier_embed wrote it, the gradient of the embedded rows as
 * g [rows, ldg] + g2 [rows, ldg2] (g2 may be null: g alone; the engine passes d x_in and d x_gate) ->
 * dv [rows, C] contiguous, summed in the fixed order given above.
 * n in [1, 8], rows >= 1, C >= 1, ld and C (4 n + 3) below 2^31; GNOT_E_INVALID before any launch otherwise. */
int gnot_fourier_embed(const float* src, int64_t rows, int C, int n, float* dst, int64_t ld, void* stream);
int gnot_fourier_embed_bwd(const float* emb, int64_t ld, const float* g, int64_t ldg, const float* g2, int64_t ldg2,
                           int64_t rows, int C, int n, float* dv, void* stream);

/* The row kernels of gnot_plan_set_pre_norm on their own, for row-by-row tests (no plan; one launch on
 * `stream`; fp32 device pointers; one wave per row, the row in registers, every row sum in one fixed order, so
 * a row's bits do not depend on the call it is part of).
 * gnot_layer_norm: y[r, :C] = (x[r, :C] - mean) * rstd, rstd = 1 / sqrtf(var + eps), var the biased variance
 * summed from (x - mean)^2, the mean kept as two floats hi + lo with lo = mean(x - hi), so that a common offset
 * of the row costs y and rstd nothing and a constant row gives exact zeros;
 * columns C .. ldy - 1 of y are written as exact zeros, columns C .. ldx - 1 of x are ignored (not assumed
 * zero); rstd [rows] is written unless null.
 * gnot_layer_norm_bwd: dx = rstd (dy - mean_C(dy) - y mean_C(dy y)) from the y and rstd the forward wrote;
 * accumulate == 0 stores it (columns C .. lddx - 1 as zeros), otherwise it is added onto dx, one rounded add
 * per element (pad columns untouched).  dx may alias dy.
 * GNOT_E_INVALID before any launch for a null pointer (rstd may be null in the forward), rows outside
 * [1, 2^31), C outside [1, 1024], a row pitch below C, not a multiple of 4 or not below 2^31, a pointer that is
 * not 16-byte aligned, or an eps that is not finite and positive. */
int gnot_layer_norm(const float* x, int64_t ldx, int64_t rows, int C, float eps, float* y, int64_t ldy, float* rstd,
                    void* stream);
int gnot_layer_norm_bwd(const float* y, int64_t ldy, const float* rstd, const float* dy, int64_t lddy, int64_t rows,
                        int C, float* dx, int64_t lddx, int accumulate, void* stream);

/* The row kernel of gnot_plan_set_dropout on its own, for bit-level tests (no plan; one launch on `stream`):
 * x [rows, ld] fp32 in place, columns C .. ld - 1 untouched; off_dev [B + 1] the samples' row offsets and
 * glo_dev [B] the global index of the first row of every sample (int64, device); key_dev and site as above.
 * p = 0 (T = 0) launches nothing.  GNOT_E_INVALID before any launch for a null pointer, rows outside [1, 2^31),
 * C outside [1, 1024], a row pitch below C, not a multiple of 4 or not below 2^31, an x that is not 16-byte
 * aligned, B < 1, site >= 2^24, or a p outside [0, 1). */
int gnot_dropout_rows(float* x, int64_t ld, int64_t rows, int C, const int64_t* off_dev, const int64_t* glo_dev, int B,
                      const uint32_t* key_dev, uint32_t site, float p, void* stream);

/* Backward of the last gnot_forward: dout [P, out_dim] -> every parameter gradient, written
 * (overwritten) into the gradient arena.  The same as gnot_backward_ex(plan, dout, 0, stream). */
int gnot_backward(gnot_plan* plan, const float* dout, void* stream);

/* Backward with options (gradient accumulation over micro-batches: the reference takes one optimizer
 * step per batch of four meshes, main.py:41, which need not fit one plan).
 *   GNOT_BWD_ACCUMULATE      every parameter gradient is ADDED onto the arena: the split-K finish of each
 *                            weight-gradient job stores old + s, s being the fixed-order sum the plain
 *                            backward stores (one add per element, no atomics: deterministic).  Needs a
 *                            caller-owned arena (GNOT_E_STATE otherwise: the workspace arena does not
 *                            survive a geometry change).  The first micro-batch of a group runs without
 *                            the flag, so no clear is needed.  The attention states and the input
 *                            gradients (gnot_input_grads) are per backward and never accumulated.
 *   GNOT_BWD_SKIP_GRAD_COMM  this backward issues none of the gradient collectives of
 *                            gnot_plan_set_grad_comm (no work on their stream, no join): every micro-batch
 *                            but the last of a group.  The point-shard state all-reduces and the scramble
 *                            all-to-all are not gradient collectives and always run.
 * Unknown flag bits give GNOT_E_INVALID.  The flags are launch arguments, not part of the bound tables:
 * one bound plan may overwrite in one backward and accumulate in the next, and a captured graph replays
 * with the flags it was captured with. */
enum { GNOT_BWD_ACCUMULATE = 1, GNOT_BWD_SKIP_GRAD_COMM = 2 };
int gnot_backward_ex(gnot_plan* plan, const float* dout, int flags, void* stream);

/* ---------------------------------------------------------------- point sharding (multi-GPU)
 * One process per GPU.  Every sample b of a batch is split over `world` ranks in contiguous point
 * ranges: rank r owns global points [floor(r*N_b/world), floor((r+1)*N_b/world)) (gnot_shard_range).
 * Everything per point stays local (gating, encoders, projections, MoE chains, residuals); the
 * reference's attention needs two exchanges:
 *   - the self-attention states S = sum k^T v, z = sum k (model.py:98-100), and in the backward
 *     dS, dz, are sums over ALL points of a sample: partial states are all-reduced (sum);
 *   - the head-major "scramble" of model.py:81/103-104 maps output token n' to flat rows
 *     n'*H .. n'*H+H-1 of [H, N, dh], i.e. to ALL points of a head range: the apply pass output is
 *     exchanged all-to-all (and the gradient back in the backward).
 * The input-function branch of cross attention is replicated on every rank; its backward needs no
 * exchange (every gradient downstream of dS is linear in it, so the per-rank partials add up in the
 * caller's gradient all-reduce).  The caller sums the parameter gradients over ranks.
 * The collectives are caller-provided callbacks (RCCL through torch.distributed in gnot_amd); they
 * are invoked synchronously from gnot_forward / gnot_backward and must be ordered on `stream`. */
typedef struct gnot_comm {
  void* user;
  /* in-place sum over ranks of `count` floats */
  int (*allreduce_sum)(void* user, float* buf, int64_t count, void* stream);
  /* all-to-all-v: send_counts[t] floats to rank t (packed in rank order in `send`), receive
   * recv_counts[s] floats from rank s (packed in rank order into `recv`) */
  int (*alltoallv)(void* user, const float* send, const int64_t* send_counts, float* recv,
                   const int64_t* recv_counts, void* stream);
} gnot_comm;

/* Gradient all-reduce overlapped with the backward (data-parallel training over ranks: sample-DP, or the
 * parameter gradients of a point-sharded batch).  With comm != NULL, gnot_backward sums every weight-
 * gradient group's contiguous (dW, db) ranges of the gradient arena over the ranks (comm->allreduce_sum,
 * in place) on a stream of its own as soon as that group's kernels have written them, and joins that
 * stream into `stream` before it returns -- the arena then holds the rank sums.  NULL switches it off
 * (the caller reduces the arena itself).  `comm` is copied; only allreduce_sum is used.  No reference
 * counterpart (main.py:27 is single-device); SURVEY.md section 5 "weight-grad all-reduce overlapped with
 * backward". */
int gnot_plan_set_grad_comm(gnot_plan* plan, const gnot_comm* comm);

/* Declare the rank's shard of the next batch: n_global[b] = points of sample b over all ranks.
 * Call before gnot_plan_set_batch, whose x_off then gives the LOCAL slices (validated against
 * gnot_shard_range).  world == 1 (or comm == NULL) switches sharding off.  `comm` is copied.
 * Padded hidden widths (see gnot_config) shard too: the exchanges move the real width's rows. */
int gnot_plan_set_shard(gnot_plan* plan, int rank, int world, int B, const int64_t* n_global, const gnot_comm* comm);

/* Host-only helpers (no GPU): the canonical point range of a rank, and the rank's side of the
 * scramble all-to-all.  Segments are rows of 4 int64 {dir, local_off, buf_off, len} in floats:
 * dir 0 copies local head-major apply output -> send buffer, dir 1 copies receive buffer -> local
 * token-order rows.  *nseg returns the number of segments (at most `cap` are written). */
int gnot_shard_range(int64_t n, int rank, int world, int64_t* lo, int64_t* hi);
int gnot_shard_exchange(int B, const int64_t* n_global, int n_head, int head_dim, int rank, int world,
                        int64_t* send_counts, int64_t* recv_counts, int64_t* segs, int64_t cap, int64_t* nseg);

/* ---------------------------------------------------------------- the training step around the path
 * (stateless, stream-ordered, no allocation)
 *
 * RelL2Loss (reference loss.py:14-23, the dgl SumPooling of main.py:87-98 as packed segment sums):
 * pred/tgt [rows, C] fp32 packed by the device offsets off_dev[B+1] (off_host = the same on the host,
 * for sizing); writes the scalar loss = mean over (sample, channel) of sqrt(sum (p-t)^2 / sum t^2)
 * to *loss (device) and, if dpred != NULL, d loss / d pred.  work: device scratch of
 * gnot_rel_l2_work_floats(off_host, B, C) floats.  Deterministic (fixed-order reductions). */
size_t gnot_rel_l2_work_floats(const int64_t* off_host, int B, int C);
int gnot_rel_l2_loss(const float* pred, const float* tgt, const int64_t* off_dev, const int64_t* off_host, int B,
                     int C, float* work, float* loss, float* dpred, void* stream);

/* One torch.optim.AdamW step (main.py:51) over flat fp32 arrays of n elements (param, grad, exp_avg,
 * exp_avg_sq), in torch's operation order.  hyper: DEVICE array of 8 floats {lr, beta1, beta2, eps,
 * weight_decay, 1 - beta1^t, 1 - beta2^t, grad_scale}, so a captured graph picks up the schedule the
 * host writes there (OneCycleLR changes lr and beta1, main.py:52). */
int gnot_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* hyper,
                    void* stream);

/* MSELoss (reference loss.py:4-12, the dgl AvgPooling as packed segment means), same arguments as
 * gnot_rel_l2_loss: loss = 1/(B C) sum_b sum_c (1/N_b) sum_n (p-t)^2 to *loss (device) and, if
 * dpred != NULL, d loss / d pred = 2 (p-t) / (B C N_b).  work: device scratch of
 * gnot_mse_work_floats(off_host, B, C) floats = B*nsplit*C + B*C (nsplit: the 2048-row splits of the longest
 * sample): the partial sums [B][nsplit][C], then the gradient scale 2 / (B C N_b) per (sample, channel) [B][C].
 * Size the buffer by the query, never by a formula of your own.  Every sample needs at least one row
 * (GNOT_E_INVALID, "empty sample": its mean is undefined).  Deterministic (fixed-order reductions).
 * gnot_rel_l2_loss and gnot_mse_loss are GNOT_LP_REL2 and GNOT_LP_MSE of gnot_lp_loss (below) without
 * comp_weights and terms: the same kernels. */
size_t gnot_mse_work_floats(const int64_t* off_host, int B, int C);
int gnot_mse_loss(const float* pred, const float* tgt, const int64_t* off_dev, const int64_t* off_host, int B, int C,
                  float* work, float* loss, float* dpred, void* stream);

/* torch.nn.utils.clip_grad_norm_(params, max_norm) with its defaults (L2 norm, error_if_nonfinite=False)
 * over a flat fp32 gradient of n >= 1 elements (any 4-byte-aligned pointer), computed on the device:
 * clip[0] = norm = |hyper[7]| sqrt(sum g^2), the norm of the scaled gradient gnot_adamw_step consumes
 * (hyper as below), clip[1] = min(1, max_norm / (norm + 1e-6)); a non-finite norm gives a non-finite
 * coefficient that propagates, as in torch.  clip: DEVICE array of 2 floats; work: device scratch of
 * gnot_grad_clip_work_floats(n) floats (a function of n alone).  Two fixed-order reduction stages, no
 * atomics: the same arguments give the same bits on every run and device.  max_norm must be positive
 * and finite.  `grad` is only read. */
size_t gnot_grad_clip_work_floats(int64_t n);
int gnot_grad_clip(const float* grad, int64_t n, const float* hyper, float max_norm, float* work, float* clip,
                   void* stream);

/* gnot_adamw_step on the clipped gradient (grad[i] * hyper[7]) * clip[1], clip as written by gnot_grad_clip
 * and read from device memory when the kernel runs (a captured graph applies each replay's own
 * coefficient); with clip[1] == 1 and a hyper[7] of 1 (or any power of two) the result is
 * gnot_adamw_step's bit for bit. */
int gnot_adamw_step_clipped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                            const float* hyper, const float* clip, void* stream);

/* The two reduction stages of gnot_grad_clip without a max_norm: clip[0] = |hyper[7]| sqrt(sum g^2), with
 * the bits gnot_grad_clip writes there for the same grad, n and hyper, and clip[1] = 1.0f.  work as for
 * gnot_grad_clip (gnot_grad_clip_work_floats(n) floats); n >= 1.  The norm in front of
 * gnot_adamw_step_guarded when nothing is clipped. */
int gnot_grad_norm(const float* grad, int64_t n, const float* hyper, float* work, float* clip, void* stream);

/* gnot_adamw_step_clipped behind a device-side test of the norm: clip as written by gnot_grad_clip or
 * gnot_grad_norm, read from device memory when the kernel runs.  guard: DEVICE array of two int32,
 * {steps skipped since the caller zeroed it, 1 if this launch skipped else 0}.
 *   clip[0] finite:      the update of gnot_adamw_step_clipped, bit for bit; guard[1] = 0.
 *   clip[0] NaN or +-inf: no element of param, exp_avg or exp_avg_sq is written; guard[0] += 1, guard[1] = 1.
 * Kernel launches only, stream-ordered, nothing read back: capturable, and every replay of a captured
 * graph decides on its own clip.  n >= 1.
 * A skipped step still consumes its step number and its schedule slot: the host writes t and the bias
 * corrections of hyper before the device knows the outcome, so only the parameters and the moments are
 * left alone.  (torch's GradScaler, in contrast, does not call optimizer.step() on a skip, so there the
 * optimizer's step count does not advance.)  A finite gradient whose sum of squares overflows fp32 has
 * an infinite norm and is skipped as well. */
int gnot_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                            const float* hyper, const float* clip, int32_t* guard, void* stream);

/* An exponential moving average of the parameters over flat fp32 arrays of n >= 1 elements, a pass of its
 * own: ema[i] = fmaf(w, param[i] - ema[i], ema[i]) with the difference rounded first, w = weight[0] =
 * 1 - decay of this step, read from DEVICE memory when the kernel runs (a captured graph picks up each
 * replay's value).  `param` is only read; ema must not be the same array as param (GNOT_E_INVALID). */
int gnot_ema_update(float* ema, const float* param, int64_t n, const float* weight, void* stream);

/* One AdamW step with gnot_ema_update fused in: every element's average follows the parameter value the step
 * just stored, in the same kernel.  hyper: DEVICE array of 9 floats, the 8 of gnot_adamw_step, then w.
 *   clip == NULL, guard == NULL: param / exp_avg / exp_avg_sq as gnot_adamw_step leaves them, bit for bit
 *                                (for a hyper[7] of 1 or any power of two, as for gnot_adamw_step_clipped);
 *   clip != NULL, guard == NULL: as gnot_adamw_step_clipped;
 *   clip != NULL, guard != NULL: as gnot_adamw_step_guarded -- on a NaN or infinite clip[0] no element of
 *                                param, exp_avg, exp_avg_sq or ema is written, only guard;
 *   a guard without a clip is refused (GNOT_E_INVALID).
 * In every form ema ends as gnot_ema_update(ema, param, n, &hyper[8]) after that entry would leave it, bit
 * for bit.  n >= 1; ema must not be the same array as param.  One kernel launch, stream-ordered, nothing read
 * back: capturable.  The 8-float hyper of the other entries is unchanged. */
int gnot_adamw_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                        const float* hyper, const float* clip, int32_t* guard, void* stream);

/* Frozen Linears (fine-tuning).  mask: one byte per Linear in gnot_plan_num_linears order, non-zero = trainable;
 * NULL (the default): all trainable.  A Linear is the unit -- its dW and db come out of one weight-gradient job.
 * Call after gnot_plan_create and before gnot_plan_set_batch; a change invalidates the batch, like the other
 * setters.  Training plans only; the forward and the saved activations do not change, and the workspace keeps
 * their size (its split-K slab and job tables shrink with the jobs; freeing the saves below the cut is the
 * known follow-up).
 *   - No weight-gradient job is planned for a frozen Linear.  A group left without a job launches nothing, takes
 *     no split-K slab, records no profile scope and issues no gradient collective; with gnot_plan_set_grad_comm a
 *     group reduces only the arena ranges of its trainable Linears, one call per contiguous run.
 *   - The arena ranges of a frozen Linear are never written: not by the backward (with or without
 *     GNOT_BWD_ACCUMULATE), not by bind (the clear of padded widths goes around them), in the workspace arena
 *     and in a caller's arena alike.
 *   - Removing jobs changes a group's split counts and balanced ranges, so the remaining gradients equal the
 *     unfrozen run's to rounding, not bit for bit.
 *   - Early stop.  Stages: the encoders (the x MLP, gating, every input-function encoder), blocks 0 .. L-1, the
 *     decoder.  With c the lowest stage that holds a trainable Linear (the encoders when
 *     gnot_plan_set_input_grads is on), gnot_backward runs from the decoder down to stage c and issues no kernel
 *     of the stages below it; inside block c everything runs as before.  Of the batched key/value backward of
 *     the input functions only the jobs of the blocks that ran are launched, and only when one of their
 *     key/value Linears is trainable.  Everything frozen and no input gradients: the backward launches nothing
 *     and returns GNOT_OK.  Every side stream a shortened backward forks is joined before it returns.
 * gnot_debug_backward_plan (host only, needs gnot_plan_set_batch): *wgrad_jobs = the weight-gradient jobs over all
 * groups, *lowest_stage = the lowest stage the backward enters: -1 the encoders, l block l, L the decoder alone,
 * L + 1 nothing. */
int gnot_plan_set_trainable(gnot_plan* plan, const uint8_t* mask);
int gnot_debug_backward_plan(const gnot_plan* plan, int* wgrad_jobs, int* lowest_stage);

/* The update and the norm over PARTS of an arena with per-group constants: frozen tensors and AdamW parameter
 * groups (fine-tuning).  One slice table serves both: `nslices` rows of three int64 {begin, len, group}, built on
 * the host -- every trainable tensor of the arena cut into slices of at most 8192 elements, a frozen tensor
 * has no row -- and uploaded once (slices_dev on the device, slices_host the same on the host, for validation).
 * Rows must be sorted and disjoint, lie inside [0, n), have 1 <= len <= 8192 and 0 <= group < G, 1 <= nslices
 * < 2^24; anything else is GNOT_E_INVALID before any launch.  One workgroup per row.  An element outside every
 * row is neither read nor written, in param, grad, exp_avg, exp_avg_sq and ema alike (a NaN in a frozen range of
 * grad is never seen).
 *
 * gnot_adamw_step_groups: the element expression of gnot_adamw_step with lr = hyper[0] * ghyper[group][0], the
 * product rounded to fp32 once, and weight_decay = ghyper[group][1]; ghyper: DEVICE array of G pairs {lr_scale,
 * weight_decay}; hyper[4] is not read.  ema, clip and guard may be NULL in the combinations gnot_adamw_step_ema
 * accepts (a guard needs a clip); with ema, hyper has 9 floats.  With one group {1, hyper[4]} whose rows cover
 * [0, n) the results are bit for bit those of gnot_adamw_step_clipped, _guarded and _ema for the same inputs, a
 * guarded skip that writes nothing but guard included; with clip == NULL and ema == NULL they are
 * gnot_adamw_step's bit for bit when hyper[7] is a power of two (the limit gnot_adamw_step_clipped states).
 * One kernel launch, stream-ordered, nothing read back: capturable.
 *
 * gnot_grad_norm_groups / gnot_grad_clip_groups: gnot_grad_norm / gnot_grad_clip over the rows' elements only,
 * the norm of the trainable gradient.  Stage 1 sums g^2 per row in a fixed order, stage 2 the partials in row
 * order; work: nslices floats.  No atomics: the same arguments give the same bits on every run and device.  The
 * bits differ from the plain entries' for the same gradient, because the rows start at tensor boundaries and not
 * at multiples of 8192.  The group column is neither read nor checked. */
int gnot_adamw_step_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                           const float* hyper, const float* ghyper, int G, const int64_t* slices_dev,
                           const int64_t* slices_host, int64_t nslices, const float* clip, int32_t* guard,
                           void* stream);
int gnot_grad_norm_groups(const float* grad, int64_t n, const float* hyper, const int64_t* slices_dev,
                          const int64_t* slices_host, int64_t nslices, float* work, float* clip, void* stream);
int gnot_grad_clip_groups(const float* grad, int64_t n, const float* hyper, float max_norm, const int64_t* slices_dev,
                          const int64_t* slices_host, int64_t nslices, float* work, float* clip, void* stream);

/* Batch assembly from a dataset that lives in device memory (no reference counterpart: main.py:57-58 batches
 * on the host).  src [rows, C] and dst [sum k, C] are fp32; the table has one row of six int64 per segment b,
 * {src_row0, n, dst_row0, k, key_lo, key_hi} (table_dev on the device, table_host the same on the host, for
 * validation before the launch).  For 0 <= j < k the kernel copies row src_row0 + sigma(j) of src to row
 * dst_row0 + j of dst:
 *   k == n: sigma(j) = j, the segment whole and in its own order;
 *   k <  n: sigma(j) = pi(j; n, key_lo, key_hi), the first k values of a keyed permutation of [0, n): a uniform
 *           subsample without replacement, a pure function of (key, n) -- no device random state.
 * pi is a cycle-walking Feistel permutation, all arithmetic uint32 (mod 2^32):
 *   fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
 *   n <= 1: pi(0) = 0.  n >= 2: bits = bit_length(n - 1), h = (bits + 1) / 2, mask = 2^h - 1
 *   rk_r = fmix32(key_lo ^ (r * 0x9E3779B9)) + key_hi, r = 0..5
 *   E(x): L = x >> h, R = x & mask; for r = 0..5: (L, R) = (R, L ^ (fmix32(R ^ rk_r) & mask)); (L << h) | R
 *   pi(j) = the first of E(j), E(E(j)), ... that is < n
 * The same table with another C gathers a second array's corresponding rows (x and y of a mesh); segments of
 * n = k = 1 gather single rows (theta).  GNOT_E_INVALID before any launch for: null pointers; B < 1 or C < 1;
 * src_row0 < 0, n < 0, n >= 2^31, k < 0 or k > n; a key outside [0, 2^32); dst_row0[0] != 0 or
 * dst_row0[b+1] != dst_row0[b] + k[b].  That src holds src_row0 + n rows and dst sum k rows is the caller's to
 * ensure.  sum k == 0 launches nothing.  One kernel launch whatever B is; stateless, stream-ordered, no
 * allocation. */
int gnot_gather_rows(const float* src, int C, const int64_t* table_dev, const int64_t* table_host, int B, float* dst,
                     void* stream);

/* Unit-Gaussian normalisation of inputs and targets (the original GNOT code's UnitTransformer,
 * (x - mean) / (std + 1e-8) per channel; the replicated main.py trains on raw values).  A "stats block" for C
 * channels is a DEVICE array of 3 C floats, {mean[C], std[C], rstd[C]}.
 *
 * gnot_channel_stats fills one from src [rows, C] (fp32, device): mean[c], the unbiased standard deviation
 * std[c] (divisor rows - 1, as torch.std) and rstd[c] = 1 / (std[c] + eps).  A channel counts as constant and
 * gets std[c] = 0, rstd[c] = 1 -- both transforms then only shift it -- when rows == 1 or
 * std[c] <= 1e-6 |mean[c]| (std == 0, and the fp32 noise a truly constant channel leaves).
 * The variance is not taken as E[x^2] - E[x]^2 of raw values: slices of 4096 rows are each reduced about
 * their own mean in two passes and merged exactly (Chan et al.), every difference between nearby values, so
 * a channel like 1e4 + N(0, 1) keeps std to fp32 rounding.  Two fixed-order reduction stages, no atomics: the
 * same arguments give the same bits on every run.  work: device scratch of
 * gnot_channel_stats_work_floats(rows, C) floats (a function of rows and C alone; 0 for arguments out of
 * range).  1 <= rows < 2^31, C >= 1.  GNOT_E_INVALID before any launch for: null pointers; rows < 1 or
 * rows >= 2^31; C < 1; eps negative or not finite.  Two kernel launches; stateless, stream-ordered, no
 * allocation, capturable. */
size_t gnot_channel_stats_work_floats(int64_t rows, int C);
int gnot_channel_stats(const float* src, int64_t rows, int C, float eps, float* work, float* stats, void* stream);

/* gnot_gather_rows with the normalisation applied as the rows are copied: the same table, validation and
 * permutation, and every copied value s of channel c is written as (s - mean[c]) * rstd[c] from `stats` (a
 * stats block for C channels).  The difference and the product are each rounded to fp32, so dst holds, bit
 * for bit, what gnot_gather_rows followed by torch's (g - mean) * rstd gives; a block of mean 0, rstd 1
 * reproduces the plain gather.  A null stats is GNOT_E_INVALID.  One kernel launch; stateless, stream-ordered,
 * no allocation. */
int gnot_gather_rows_affine(const float* src, int C, const int64_t* table_dev, const int64_t* table_host, int B,
                            const float* stats, float* dst, void* stream);

/* gnot_rel_l2_loss / gnot_mse_loss of a NORMALISED prediction against the RAW target: the loss of
 * p' = pred * std[c] + mean[c] (out_stats: the targets' stats block for C channels), the product and the sum
 * each rounded to fp32, and, if dpred != NULL, d loss / d pred = ((p' - t) * scale[b, c]) * std[c] with the last
 * product rounded on its own.  Loss and gradient are bit for bit the plain entry applied to torch's
 * pred * std + mean, the gradient then multiplied by std -- without the two elementwise passes and the two
 * prediction-sized temporaries.  Same arguments otherwise, the same work sizes
 * (gnot_rel_l2_work_floats / gnot_mse_work_floats), the same refusals; a null out_stats is GNOT_E_INVALID. */
int gnot_rel_l2_loss_affine(const float* pred, const float* tgt, const int64_t* off_dev, const int64_t* off_host,
                            int B, int C, const float* out_stats, float* work, float* loss, float* dpred,
                            void* stream);
int gnot_mse_loss_affine(const float* pred, const float* tgt, const int64_t* off_dev, const int64_t* off_host, int B,
                         int C, const float* out_stats, float* work, float* loss, float* dpred, void* stream);

/* The Lp loss family with component weights and per-sample terms, over the packed arguments of gnot_rel_l2_loss.
 * With d = p' - t (p' = pred, or pred * std[c] + mean[c] rounded as in the _affine entries when out_stats is not
 * NULL) and n over the N_b rows of sample b, the term of (sample b, channel c) is
 *   GNOT_LP_REL2    sqrt(sum d^2 / sum t^2)        GNOT_LP_MSE   sum d^2 / N_b
 *   GNOT_LP_REL1    sum |d| / sum |t|              GNOT_LP_L1    sum |d| / N_b
 *   GNOT_LP_RELINF  max |d| / max |t|              GNOT_LP_LINF  max |d|
 * and *loss (device) = (1/B) sum_b sum_c w^_c e[b, c], w^_c = w_c / sum_c w_c from comp_weights (DEVICE array of C
 * non-negative weights with a positive sum, normalised on the device in index order) or 1/C when it is NULL.
 * terms, if not NULL: DEVICE [B, C], the unweighted e[b, c]; they do not depend on comp_weights.  dpred, if not
 * NULL: d loss / d pred, (w^_c / B) d e / d p' -- sign(d) / sum |t| for rel1, sign(d) / N_b for l1, sign(0) = 0 --
 * times std[c] as one more rounded product with out_stats; a channel of weight zero gets exact zeros.  relinf and
 * linf are metrics only: a dpred with them is GNOT_E_INVALID, as are an unknown kind and a sample without rows
 * ("empty sample"), all before any launch.  A relative kind with an all-zero target channel gives inf / NaN, like
 * gnot_rel_l2_loss (no epsilon).  Without comp_weights, REL2 and MSE give the bits of gnot_rel_l2_loss(_affine) /
 * gnot_mse_loss(_affine), loss and dpred alike (those entries are these two kinds: one set of kernels).  work: device
 * scratch of gnot_lp_loss_work_floats(off_host, B, C) floats.  Three launches at most (partial sums per 2048-row
 * split, one finish workgroup, the elementwise gradient), fixed-order reductions, no atomics, no host
 * synchronisation: deterministic and capturable. */
enum { GNOT_LP_REL2 = 0, GNOT_LP_REL1 = 1, GNOT_LP_RELINF = 2, GNOT_LP_MSE = 3, GNOT_LP_L1 = 4, GNOT_LP_LINF = 5 };
size_t gnot_lp_loss_work_floats(const int64_t* off_host, int B, int C);
int gnot_lp_loss(const float* pred, const float* tgt, const int64_t* off_dev, const int64_t* off_host, int B, int C,
                 int kind, const float* comp_weights, const float* out_stats, float* work, float* loss, float* terms,
                 float* dpred, void* stream);

/* gnot_lp_loss with one weight per query point: point_w is a DEVICE array [rows] (rows = off[B]) of weights
 * w_n >= 0 -- FEM lumped-mass or quadrature weights, a 0/1 mask, anything else -- and the term of (sample b,
 * channel c) becomes, with d as in gnot_lp_loss (out_stats included),
 *   GNOT_LP_REL2    sqrt(sum w d^2 / sum w t^2)          GNOT_LP_MSE   sum w d^2 / sum w
 *   GNOT_LP_REL1    sum w |d| / sum w |t|                GNOT_LP_L1    sum w |d| / sum w
 *   GNOT_LP_RELINF  max_{w>0} |d| / max_{w>0} |t|        GNOT_LP_LINF  max_{w>0} |d|
 * loss, comp_weights, terms, the refusals and the launch structure are gnot_lp_loss's (three launches at most,
 * fixed-order reductions, no atomics, no host synchronisation, capturable); dpred is the exact derivative: w_n
 * multiplies the element's gradient and the mean kinds divide by sum w where N_b stood.
 *   - A row with w_n == 0 contributes nothing and is not read into any sum: a NaN or Inf in pred or tgt there
 *     (a masked target) changes no bit of loss, terms or any other row's gradient, and its own dpred elements are
 *     exact zeros.
 *   - Every w_n == 1.0f gives the bits of gnot_lp_loss -- loss, terms and dpred, every kind, with and without
 *     comp_weights / out_stats -- while a sample has fewer than 2^24 rows (sum w is then N_b exactly in fp32).
 *   - Multiplying every weight of a sample by one power of two (no overflow, no denormals) changes no bit.
 * point_w is not validated (that would take a host synchronisation): a negative or NaN weight counts as zero,
 * and a sample whose weights are all zero gives 0 / 0, like an all-zero target channel of a relative kind.  A
 * null point_w is GNOT_E_INVALID; every host check of gnot_lp_loss applies unchanged.  work: device scratch of
 * gnot_lp_loss_weighted_work_floats(off_host, B, C) floats (the per-split partials of mse / l1 carry sum w). */
size_t gnot_lp_loss_weighted_work_floats(const int64_t* off_host, int B, int C);
int gnot_lp_loss_weighted(const float* pred, const float* tgt, const float* point_w, const int64_t* off_dev,
                          const int64_t* off_host, int B, int C, int kind, const float* comp_weights,
                          const float* out_stats, float* work, float* loss, float* terms, float* dpred, void* stream);

/* gnot_channel_stats with one weight per row, w: DEVICE [rows], w >= 0.  With V1 = sum w and V2 = sum w^2,
 * mean[c] = sum w v / V1 and std[c]^2 = sum w (v - mean)^2 / (V1 - V2 / V1), the reliability-weights estimator
 * (rows - 1 at w == 1); rstd, eps and the constant-channel rule are gnot_channel_stats's, and a channel with
 * V1 - V2 / V1 <= 0 (one weighted row) is constant.  Rows with w == 0 are not read (a NaN there is harmless); the
 * weights are not validated, and no weighted row at all gives mean = 0 / 0.  The same scheme: slices of 4096
 * rows reduced about a pivoted mean (the pivot is the slice's first row with w > 0; a slice without one is
 * skipped) and merged about the global mean, never E[x^2] - E[x]^2; two launches, fixed order, no atomics,
 * capturable.  work: gnot_channel_stats_weighted_work_floats(rows, C) floats.  The refusals of
 * gnot_channel_stats, and a null w. */
size_t gnot_channel_stats_weighted_work_floats(int64_t rows, int C);
int gnot_channel_stats_weighted(const float* src, const float* w, int64_t rows, int C, float eps, float* work,
                                float* stats, void* stream);

/* Live kernel timing for the bench's roofline:while enabled, every launch of kernel class `kind`
 * ("moe_fwd" fused expert chains forward, "moe_bwd" their backward, "wgrad" weight-gradient GEMMs;
 * "" disables) is bracketed by hipEvents on its stream.  gnot_profile_read synchronizes on those
 * events and returns the summed device time, the launch count and the algorithmic FLOPs of those
 * launches, then resets the counters. */
int gnot_profile_enable(gnot_plan* plan, const char* kind);
int gnot_profile_read(gnot_plan* plan, double* ms_total, int64_t* launches, double* flops_total);

/* Debug/test hook: device pointer + row stride (floats) of a named intermediate buffer
 * ("scores", "query0", "out_h0", ...); returns GNOT_E_INVALID for unknown names. */
int gnot_debug_buffer(const gnot_plan* plan, const char* name, float** ptr, int64_t* ld);

/* Debug/test hook: the kernel forms the plan chose for the current batch geometry, as one line of
 * space-separated key=value pairs written into text (cap bytes with the terminator; 256 suffice;
 * GNOT_E_INVALID when too small).  Needs gnot_plan_set_batch (GNOT_E_STATE before) and no GPU.  The keys:
 *   apply_fwd.self  apply_fwd.cross  apply_bwd.self  apply_bwd.cross  kv_bwd  kv_bwd_batch
 *       the attention passes: narrow | wide (the VALU kernels up to / above a head width of 64) | mfma.
 *       self / cross: one set of states / those of the input functions (without input functions cross is one
 *       set too); kv_bwd the K/V backward over the query points, kv_bwd_batch the one launch over every
 *       (block, input function), none without input functions or blocks
 *   state.query  state.fn
 *       the attention-state groups: valu | mfma | none (no such group).  Every group over the query points
 *       (forward and backward, self and cross) holds the same points and has one form; state.fn is the batched
 *       forward group of all (block, input function, sample)
 *   serial_wgrad  moe_direct_out  moe_direct_dz
 *       0 | 1: weight gradients on the caller's stream instead of forked; the two soft-MoE row streams done
 *       without
 * The forms follow from the shapes and the GNOT_* switches read when the plan was created. */
int gnot_debug_kernel_forms(const gnot_plan* plan, char* text, size_t cap);

/* Debug/test hook: the device GELU every chain epilogue and weight-gradient loader inlines, evaluated
 * elementwise over n >= 1 contiguous floats (one launch on `stream`): y = gelu(x), dy = gelu'(x), and (y2, dy2)
 * the fused value-and-derivative form, bitwise equal to (y, dy).  No plan; the hot path never calls it. */
int gnot_debug_gelu(const float* x, float* y, float* dy, float* y2, float* dy2, int64_t n, void* stream);

const char* gnot_last_error(void);
const char* gnot_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GNOT_HIP_H */
