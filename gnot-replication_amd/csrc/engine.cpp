// GNOT engine: the native host runtime behind the C ABI (include/gnot_hip.h).
//
// It owns no device memory.  From the constructor arguments (reference model.py:143) it derives the
// canonical Linear list (state_dict order), from the batch offsets (the packed replacement for
// utils.py:3-4 / main.py:60-89 padding) it carves one caller-provided workspace into named
// activation buffers, builds every small device table once (weight-pack jobs, chain layer tables,
// weight-gradient job lists, point-segment lists) and then runs the whole forward
// (model.py:154-173) and backward as a fixed sequence of kernel launches on the caller's stream —
// no allocation, no host sync, capturable into a hipGraph.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/gnot_hip.h"
#include "gnot_kernels.h"

namespace gnot {

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define GNOT_CK(expr)                                                                           \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return fail(GNOT_E_HIP, std::string(#expr) + " -> " + hipGetErrorString(e_));             \
  } while (0)

static inline long r4(long x) { return (x + 3) & ~3L; }
static inline int tiles16(int x) { return (x + 15) / 16; }

constexpr int kSeg = 64;             // points per attention segment (one wave of the apply kernels)
constexpr int kPTile = 128;          // output tile edge of the point-reduction GEMM (wgrad.hip)
constexpr int kMinSplitPoints = 128; // never split below this many points

struct Img {                 // one packed MFMA A-operand image in the packed arena
  size_t off4 = 0;           // offset in float4 units
  int OT = 0, KT = 0;
  const float4* p = nullptr;
};

struct Buf {
  size_t off = 0;            // bytes
  long ld = 0;
  float* p = nullptr;
};

struct WgradGroup {
  std::vector<WgradJob> jobs;
  std::vector<int> wg_prefix, red_prefix;
  int total_wgs = 0, total_red = 0;
  size_t slab_floats = 0;
  WgradKernel kind = WgradKernel::Tile128;   // weight-gradient groups: the kernel they run (finish_group)
  bool scaled = false;               // Wide256: some job has a per-point scale (WgradJob::scale), the scaled form
  std::vector<int> lins;             // weight-gradient groups: the canonical Linears whose (dW, db) they write
  int state_pts = 0, state_nw = 0;
  bool state_mfma = false;   // state groups: points per workgroup, per-point weights (0 or H)
  // balanced groups: per-workgroup point ranges {job, slot, begin, end} (WgradTables::segs) and the first
  // range of every workgroup (+ the end)
  std::vector<int4> segs;
  std::vector<int> seg_start;
  WgradJob* d_jobs = nullptr;        // device copies (workspace tables)
  int* d_wg_prefix = nullptr;
  int* d_red_prefix = nullptr;
  int4* d_segs = nullptr;
  int* d_seg_start = nullptr;
  WgradTables tables() const {
    return {d_jobs, (int)jobs.size(), d_wg_prefix, total_wgs, d_red_prefix, total_red, d_segs, d_seg_start};
  }
};

// One MLP chain call site: gating, the query encoder, an input-function encoder, one soft-MoE call of a block
// or the decoder.  build_chains states each once; plan_images, the device tables, the weight-gradient groups
// and the forward / backward launches read it from here
struct Chain {
  std::vector<int> firsts;           // the first canonical Linear of each parallel chain
  int in_dim = 0, out_dim = 0;
  int KT0 = 1, OTL = 1;              // input / last-output tile counts (1 up to 16 columns, else D / 16)
  int kcall = 0;                     // backward slot: its dZ goes to dz_name(kcall)
  long rows = 0;                     // P, or Q[i] of an input-function encoder
  std::string x, save;               // input buffer (row pitch: its ld) and saved pre-activations
  int mode = CH_STORE;
  std::vector<ChainLayer> layers;    // [firsts.size() * NL] layer table, filled at bind
  ChainLayer* d_layers = nullptr;
  WgradGroup wg;                     // the weight gradients of its Linears
};

// One set of states an attention call's apply passes read: the query points' own (a fused call) or those of input
// function `fn` (ckv: its K | V rows, dkv: their gradient, enc: the encoding rows the K / V projections read)
struct AttnSrc {
  std::string state, du, dden, dstate;   // S | z per sample; the backward's du, dden rows and its dS | dz
  int fn = -1;
  std::string ckv, dkv, enc;
  WgradGroup st, dst;                // forward states (fused calls; input-function sources: the batched st_fn) and dS | dz
};

// One LinearAttention call of a block: cross (reading the block's query) or self (reading query1).
// build_attn_calls states each once; plan_images, the carve, the groups, the batched input-function tables and
// the forward / backward launches read it from here.  Buffers are names, resolved with P_ at use
struct AttnCall {
  int l = 0;
  bool cross = false;
  uint32_t site = 0;                 // dropout site: 2 l cross, 2 l + 1 self
  bool fused = true;                 // one q|k|v projection of the query rows; else q alone and input-function sources
  int nsrc = 1;                      // state sets the apply passes read (= src.size())
  int q = 0, o = 0;                  // canonical Linears
  std::vector<int> k, v;
  Img proj_img, o_img;               // packed images (proj: q or q|k|v) and bias offsets in pbias (floats)
  std::vector<Img> kv_img;           // K | V of every input-function source
  size_t bproj = 0, bo = 0;
  std::vector<size_t> bkv;
  std::string in_raw, in, rstd;      // the rows it reads: raw, as projected (pre-norm: normalised, else in_raw), their rstd
  std::string proj;                  // q or q | k | v rows
  long pitch = 0;                    // ... of D or 3 D floats
  std::vector<AttnSrc> src;
  std::string res, out;              // scramble rows (Dr floats per token) and fc_out's rows
  std::string dsum, dqkv;            // backward slots: d out, d proj
  WgradGroup wg;                     // the weight gradients of o, q (and k, v of a fused call)
  AttnKernel apply_fwd = {}, apply_bwd = {};   // kernel forms (choose_attn_forms)
};

// b + off, or null while b is unbound: the sizing pass of set_batch builds every job table for its size
// only and forms no address
template <typename T>
static inline T* at(T* b, long off) { return b ? b + off : nullptr; }

}  // namespace gnot

using namespace gnot;

struct gnot_plan {
  gnot_config c{};
  int D = 0, H = 0, dh = 0, E = 0, NL = 0, L = 0, I = 0, KI = 0, DT = 0;
  // Dr: the model's hidden width (n_embed); D: the width the kernels run, Dr rounded up to whole
  // 16-wide tiles when Dr is not one the kernels take (gnot_plan_create).  Every activation row keeps D
  // columns whose pad columns Dr .. D-1 stay exact zeros (zero weight rows / columns and biases in the
  // packed images, pad columns of the feature softmax zeroed); parameters and gradients have Dr.
  int Dr = 0;
  bool padded() const { return Dr != D; }
  // padded heads (a head width Dr / H that is not a multiple of 4, d <= 192): the attention runs heads of
  // dh = the next multiple of 4 (q / k / v projections place head h's rows at h * dh, the feature softmax
  // masks the pad features, pack.hip PackJob::hr / hp), while the scramble rows (model.py:81-83) keep the
  // real head width dhr = Dr / H.  dhr == dh otherwise
  int dhr = 0;
  bool head_padded() const { return dhr != dh; }
  int hd() const { return H * dh; }                 // attention feature columns (<= D)
  // the projections' feature-softmax pad columns: features past the H heads of dh are written as 0
  int attn_dreal() const { return hd() < D ? hd() : 0; }
  int in = 0, th = 0, F = 0, out = 0;
  // Fourier embedding (gnot_plan_set_fourier): orders of x and of the input functions (0: none) and the widths
  // of the caller's rows; in / F above stay the embedded widths, which the Linears and the workspace have
  int nx = 0, nf = 0, in_raw = 0, F_raw = 0;
  // pre-norm (gnot_plan_set_pre_norm): the attention calls read the parameter-free LayerNorm (over the Dr real
  // columns, norm.hip) of the residual stream ("b{l}.n1" / "b{l}.n2") and of the input-function encodings
  // ("fnn{i}", shared by every block); the residual stream itself is untouched
  bool pre_norm = false;
  float norm_eps = 1e-5f;
  // keyed dropout on the attention outputs (gnot_plan_set_dropout, dropout.hip): "b{l}.a" / "b{l}.bb" right
  // after fc_out in the forward, the rows' gradient ("dsum0" / "dsum1") right before fc_out's backward.
  // drop_T = 0: off, no launch and no table
  uint32_t drop_T = 0;
  float drop_scale = 1.f;
  const uint32_t* drop_key = nullptr;   // device {seed_lo, seed_hi, step, 0}, read when the kernels run
  bool drop_active = true;              // gnot_plan_set_dropout_active: the next forward drops
  bool drop_fwd = false;                // the last gnot_forward dropped: its backward masks the same elements
  long* d_glo = nullptr;                // [B] global index of this rank's first point of every sample
  std::vector<int> lin_o, lin_i;   // out / in features per canonical Linear
  std::vector<const float*> W, b;
  bool params_bound = false;

  // batch
  int B = 0;
  long P = 0;
  std::vector<long> xoff;
  std::vector<std::vector<long>> fnoff;
  std::vector<long> Q;
  bool training = true;
  bool batch_set = false;

  // workspace layout
  size_t ws_need = 0;
  char* ws = nullptr;
  std::map<std::string, Buf> bufs;
  std::vector<std::string> buf_order;

  // packed weights
  size_t packed4 = 0, pbias = 0;
  std::vector<PackJob> pack_jobs;       // dst/bias_dst hold OFFSETS until bind
  std::vector<size_t> pack_dst_off4, pack_bias_off;
  std::vector<int> pack_prefix;
  int pack_tiles = 0;
  // images
  std::vector<Img> fwd_img, T_img;      // per canonical linear (fwd_img unused for attention q/k/v)
  std::vector<size_t> fwd_bias;         // per canonical linear: offset of padded bias (floats) in pbias

  // grads
  std::vector<long> grad_off;           // 2 per linear
  long grad_floats = 0;

  // the MLP chain call sites in build_chains' order: x, gating, input functions, (ffn1, ffn2) per block, decoder
  std::vector<Chain> chains;
  Chain& ch_x() { return chains[0]; }
  Chain& ch_gate() { return chains[1]; }
  Chain& ch_fn(int i) { return chains[2 + i]; }
  Chain& ch_moe(int l, bool m1) { return chains[2 + I + 2 * l + (m1 ? 0 : 1)]; }
  Chain& ch_out() { return chains.back(); }
  // the attention calls in build_attn_calls' order: (cross, self) per block
  std::vector<AttnCall> attn;
  AttnCall& call(int l, bool cross) { return attn[2 * l + (cross ? 0 : 1)]; }
  const AttnCall& call(int l, bool cross) const { return attn[2 * l + (cross ? 0 : 1)]; }
  long per_state() const { return (long)H * (dh * dh + dh); }   // floats of one sample's attention state (S, z)
  long Qmax() const { return Q.empty() ? 0 : *std::max_element(Q.begin(), Q.end()); }

  // device tables
  std::vector<int4> qchunks;
  std::vector<int> qchunk_off;
  std::vector<std::vector<int4>> fchunks;
  std::vector<std::vector<int>> fchunk_off;
  // cross attention with input functions: the input-function side of EVERY block is batched (built by walking
  // the cross calls' sources)
  WgradGroup st_fn;                                    // forward states of all (block, fn, sample)
  WgradGroup wg_fnkv;                                  // weight grads of all key/value projections
  std::vector<LinearArgs> fwd_kv_jobs;                 // key/value projections of all (block, fn)
  std::vector<AttnKVBwdArgs> kvbwd_jobs;               // dK/dV of all (block, fn)
  std::vector<std::vector<LinearArgs>> dfn_jobs;       // d(fn encoding): launches of <= kMaxSeg segments
  LinearArgs* d_fwd_kv_jobs = nullptr;
  AttnKVBwdArgs* d_kvbwd_jobs = nullptr;
  std::vector<LinearArgs*> d_dfn_jobs;
  size_t table_bytes = 0;
  size_t slab_wgrad_floats = 0, slab_state_floats = 0;

  // weight-gradient groups run on the caller's stream after the chain backward that produced their dZ,
  // or forked onto the side stream; every buffer a forked group reads is double-buffered and guarded
  // by the event of its last side-stream reader.  Measured, one box each, interleaved x2
  // (profiles/r04_wgrad_overlap_ab.txt): configs[2] (262,144 points) 235.3 / 236.2 ms per step serial
  // against 236.8 / 236.7 forked -- the chains and GEMMs fill every CU, so overlapping them buys
  // nothing; configs[1] (10,000 points, d = 128) 4.12 / 4.12 serial against 3.64 / 3.72 forked and
  // configs[0] (16,384 points) 9.62 / 9.65 against 9.56 / 9.55 -- small launches leave CUs idle that
  // the concurrent GEMMs fill.  So plans below kWgradSerialPoints fork, larger ones run serially;
  // Tuning::wgrad_overlap = 0 / 1 (env GNOT_WGRAD_OVERLAP) forces either form (bitwise equal).
  static constexpr long kWgradSerialPoints = 65536;
  hipStream_t side = nullptr;
  hipStream_t side2 = nullptr;          // input-function branch, concurrent with the query branch
  // the switches of gnot_kernels.h Tuning, read from the environment once, in gnot_plan_create: every kernel
  // form and size below that depends on one reads it here, so it cannot differ between set_batch, bind and launch
  Tuning tune;
  bool serial_wgrad() const { return tune.wgrad_overlap >= 0 ? tune.wgrad_overlap == 0 : P >= kWgradSerialPoints; }
  // The two row streams a fp32 d = 256 soft-MoE call does without; said once here, read by
  // moe_forward, the backward's chain launch and the call's weight-gradient jobs (chain_group):
  //   moe_direct_out: the training forward writes no [E, P, d] stage; the combine forms s_e y_e from the saved
  //                   y_e (save slot NL-1) and the scores -- the bits of the stage rows;
  //   moe_direct_dz:  the backward stores no dz_{NL-1} = s_e dq; the last Linear's jobs read dquery with the
  //                   expert's score column as their scale.  Only where the group runs on the caller's stream
  //                   right after the chain backward: a forked group reads later, beside main-stream kernels
  //                   that accumulate into dquery, and keeps the stored rows.
  // Tuning::moe_stored (env GNOT_MOE_STORED_STREAMS=1) restores both stored forms (bitwise equal)
  bool moe_direct_out() const { return !tune.moe_stored && D == 256 && npk() == 3; }
  bool moe_direct_dz() const { return moe_direct_out() && serial_wgrad(); }
  // The kernel form of every attention pass, chosen by choose_attn_forms from the batch geometry and `tune`
  // (attn_kernel, gnot_kernels.h); the apply passes' forms are the calls' (AttnCall::apply_fwd / apply_bwd)
  AttnKernel kv_bwd = {}, kv_bwd_batch = {};   // the query points' K/V backward; all (block, input function) jobs
  int kv_batch_maxchunks = 0;                   // the largest chunk count among the batched jobs
  std::vector<hipEvent_t> evs;
  size_t ev_next = 0;
  // pinned staging ring for the table uploads of gnot_plan_bind_workspace_async: slot k is rewritten
  // only after the copy that last read it has executed (stage_ev[k])
  static constexpr int kStageSlots = 4;
  void* stage[kStageSlots] = {};
  size_t stage_cap[kStageSlots] = {};
  hipEvent_t stage_ev[kStageSlots] = {};
  bool stage_used[kStageSlots] = {};
  int stage_next = 0;
  std::map<const float*, hipEvent_t> readers;
  // forked weight-gradient groups whose side-stream launch waits until the caller's stream has enqueued
  // its next kernel (run_wgrad_side / flush_deferred)
  struct DeferredWgrad {
    const WgradGroup* G;
    std::vector<const float*> reads;
    hipEvent_t fork;
  };
  std::vector<DeferredWgrad> deferred;
  int4* d_qchunks = nullptr;
  int* d_qchunk_off = nullptr;
  std::vector<int4*> d_fchunks;
  std::vector<int*> d_fchunk_off;
  long* d_xoff = nullptr;
  std::vector<long*> d_fnoff;
  PackJob* d_pack_jobs = nullptr;
  int* d_pack_prefix = nullptr;
  bool ws_bound = false;
  bool packed = false;
  bool fwd_done = false;
  bool bwd_done = false;      // a gnot_backward ran after the last gnot_forward (gnot_input_grads needs it)
  bool ig_reduced = false;    // sharded: the input-function gradients of that backward are rank sums already

  // point sharding (gnot_plan_set_shard): sample b's points are split over `world` ranks
  int world = 1, rank = 0;
  gnot_comm comm{};
  // gradient all-reduce overlapped with the backward (gnot_plan_set_grad_comm): each weight-gradient
  // group's (dW, db) ranges are summed over the ranks on `comm_stream` as soon as the group is written
  gnot_comm grad_comm{};
  bool grad_comm_on = false;
  // the running gnot_backward_ex: its gradient collectives are live (grad_comm_on without
  // GNOT_BWD_SKIP_GRAD_COMM) and its split-K finishes add onto the arena (GNOT_BWD_ACCUMULATE)
  bool grad_comm_live = false;
  bool bwd_accumulate = false;
  // caller-owned gradient arena (gnot_plan_set_grad_arena): the job tables' dW / db, the gradient
  // collectives and gnot_debug_buffer("grads") use it; null: the workspace's "grads" buffer
  float* user_grads = nullptr;
  float* grads() const { return user_grads ? user_grads : P_("grads"); }
  long arena_floats() const {
    long g = 0;
    for (size_t li = 0; li < lin_o.size(); ++li) g += (long)lin_o[li] * lin_i[li] + lin_o[li];
    return g;
  }
  hipStream_t comm_stream = nullptr;
  std::vector<long> nglob;                 // [B] global points per sample (sharded batches)
  bool sharded = false;                    // world > 1 for the current batch
  // MoE activation recompute (gnot_plan_set_moe_recompute): training keeps only each MoE call's
  // input; the backward re-runs that call's expert forward into ONE shared save buffer ("mrsave")
  // just before its chain backward -- E*NL*P*D floats once instead of per MoE call
  bool moe_recompute = false;
  // input gradients (gnot_plan_set_input_grads): the x / gating / input-function encoders' first Linears
  // also run their backward-data into dxin / dxg / dfnin<i>
  bool input_grads = false;
  // operand pieces of the d = 256 bf16-MFMA kernels (chain2, linear2, wide weight gradients):
  // 3 = bf16x6 (fp32-exact, default), 1 = bf16 arithmetic mode (gnot_plan_set_precision)
  int np = 3;
  // bf16 mode stores the soft-MoE chains' saves and dZ as bf16 (ChainArgs::b16s): one [P, 256] bf16 layer
  // is P * D / 2 four-byte units, a chain's 2 * NL save slots take what NL fp32 layers did
  bool b16s() const { return np == 1 && D == 256; }
  // operand pieces of the kernels this plan runs: the bf16 mode covers every width up to 256 (chain.hip /
  // linear.hip / the 128-tile weight gradients at d <= 192 as well); above 256 (chainw.hip) the fp32 path
  int npk() const { return D <= 256 ? np : 3; }
  // linear.hip's image kind of the attention projections (LinearArgs::img).  d <= 192: output-major bf16-piece
  // images, one RNE piece in the bf16 mode (1), the exact three-piece split in the fp32 mode (3: bf16x6, as
  // linear2.hip at d = 256; round 5, in place of the exact fp32 MFMA on fp32 fragment images -- configs[1]
  // (d = 128), one box, interleaved x2: 3.37 / 3.35 ms per step against 3.44 / 3.44, profiles/r05o*).
  // d > 256: fp32 fragment images (0), the form chainw.hip's Linears run too
  int lin_img() const { return D > 192 ? 0 : npk() == 1 ? 1 : 3; }
  std::string msave(int l, bool m1) const {
    return moe_recompute ? std::string("mrsave") : "b" + std::to_string(l) + (m1 ? ".m1save" : ".m2save");
  }
  std::vector<CopySeg> xsend, xrecv;       // scramble all-to-all: hm -> send buffer, recv buffer -> tokens
  std::vector<int> xsend_prefix, xrecv_prefix;   // prefix sums in copy units (xunit floats) for the copy kernel
  int xunit = 4;                                  // 4 (float4 runs), 1 with padded heads (runs of dhr floats)
  std::vector<int64_t> xsend_counts, xrecv_counts;
  CopySeg* d_xsend = nullptr;
  CopySeg* d_xrecv = nullptr;
  int* d_xsend_prefix = nullptr;
  int* d_xrecv_prefix = nullptr;

  // live kernel timing (bench roofline): hipEvents around every launch of one kernel class
  std::string prof_kind;
  std::vector<hipEvent_t> prof_events;   // pool, pairs
  size_t prof_used = 0;
  double prof_flops = 0.0;
  long prof_launches = 0;

  // ------------------------------------------------------------------ canonical indices
  int lin_x(int j) const { return j; }
  int lin_g(int j) const { return NL + j; }
  int lin_fn(int i, int j) const { return 2 * NL + i * NL + j; }
  int blk0() const { return 2 * NL + I * NL; }
  int per_block() const { return 6 + 2 * KI + 2 * E * NL; }
  // block l: cross q, fc_out, KI keys, KI values; self q, fc_out, key, value (build_attn_calls); ffn1, ffn2 experts
  int blk(int l) const { return blk0() + l * per_block(); }
  int lin_f1(int l, int e, int j) const { return blk(l) + 6 + 2 * KI + e * NL + j; }
  int lin_f2(int l, int e, int j) const { return lin_f1(l, E, 0) + e * NL + j; }
  int lin_out(int j) const { return blk0() + L * per_block() + j; }
  int n_lin() const { return lin_out(NL - 1) + 1; }
  // gnot_plan_set_trainable: one byte per canonical Linear; empty: all trainable.  A frozen Linear has no
  // weight-gradient job (build_groups), so its arena ranges are never written.
  std::vector<uint8_t> trainable;
  bool frozen(int li) const { return !trainable.empty() && !trainable[li]; }
  // the stage of a Linear: -1 the encoders (x MLP, gating, input-function encoders), l block l, L the decoder
  int stage_of(int li) const { return li < blk0() ? -1 : li >= lin_out(0) ? L : (li - blk0()) / per_block(); }
  // the lowest stage the backward enters (canonical order ascends through the stages): -1 .. L as stage_of,
  // L + 1: nothing to do.  Input gradients come out of the encoders' chain backwards.
  int lowest_stage() const {
    if (input_grads) return -1;
    for (int li = 0; li < n_lin(); ++li)
      if (!frozen(li)) return stage_of(li);
    return L + 1;
  }

  std::string final_query() const {
    return L > 0 ? "b" + std::to_string(L - 1) + ".query2" : std::string("query0");
  }
  std::string block_query(int l) const {   // query entering block l
    return l == 0 ? std::string("query0") : "b" + std::to_string(l - 1) + ".query2";
  }
  // double-buffer slots, fixed by the (static) backward order
  std::string dz_buf(int chain_call) const { return "dz" + std::to_string(chain_call & 1); }
  int k_out() const { return 0; }
  int k_m2(int l) const { return 1 + 2 * (L - 1 - l); }
  int k_m1(int l) const { return 2 + 2 * (L - 1 - l); }
  int k_fn(int i) const { return 1 + 2 * L + i; }
  int k_x() const { return 1 + 2 * L + I; }
  int k_gate() const { return 2 + 2 * L + I; }
  // input-function encoder chains run on side2 with their own dZ buffer; the others alternate dz0/dz1
  std::string dz_name(int kcall) const { return (kcall >= k_fn(0) && kcall < k_fn(0) + I) ? "dzf" : dz_buf(kcall); }
  // a named buffer's address (+ an element offset); null until the workspace is bound
  float* P_(const std::string& name, long off = 0) const { return at(bufs.at(name).p, off); }
};

// ====================================================================== construction
static void add_linear(gnot_plan* p, int out, int in) {
  p->lin_o.push_back(out);
  p->lin_i.push_back(in);
}

extern "C" int gnot_plan_create(const gnot_config* cfg, gnot_plan** out) {
  if (!cfg || !out) return fail(GNOT_E_INVALID, "null argument");
  const gnot_config& c = *cfg;
  if (c.n_attn_hidden_dim != c.n_mlp_hidden_dim || c.n_attn_hidden_dim != c.n_input_hidden_dim)
    return fail(GNOT_E_INVALID,
                "n_attn_hidden_dim, n_mlp_hidden_dim and n_input_hidden_dim must be equal (the residual "
                "adds of model.py:131/137 need it)");
  const int Dr = c.n_attn_hidden_dim;
  if (c.n_head <= 0 || Dr <= 0 || Dr % c.n_head != 0)
    return fail(GNOT_E_INVALID, "n_embed should be divisible by head");   // model.py:41
  const int dhr = Dr / c.n_head;
  // the attention passes take head widths that are a multiple of 4 (4-aligned lane slices up to 64, 4-feature
  // quads over 16 lanes above, attn.hip; the fp32-MFMA forms at 16 / 32 / 64); any other runs on heads padded
  // to the next multiple of 4 (gnot_plan::head_padded): q / k / v rows at h * dh, H * dh internal columns
  const int dh = (dhr + 3) / 4 * 4;
  if (dh > 256)
    return fail(GNOT_E_INVALID, "head width d/n_head must be at most 256 on the MI355X kernels");
  // the internal width D (Dr real columns + exact-zero pad columns): chain.hip / linear.hip run any multiple of
  // 16 up to 192 (whole 16-wide MFMA tiles, activations in registers); chain2.hip / linear2.hip d = 256 with
  // unpadded heads of 16 / 32 / 64 / 128 / 256 (the projections' softmax head groups); everything else up to
  // 512 runs at the next multiple of 64 from 320 on chainw.hip (one Linear at a time on linear.hip, whose
  // whole-row tilings keep any head in one workgroup)
  const int need = std::max(Dr, c.n_head * dh);
  const bool l2_heads = dh == dhr && (dh == 16 || dh == 32 || dh == 64 || dh == 128 || dh == 256);
  // Above 512 the internal width is the next multiple of 128 up to 1024: the projections then contract in two
  // halves of 320 .. 512 (launch_linear's K-split, half images PackJob::kh)
  int D;
  if (need <= 192) D = (need + 15) / 16 * 16;
  else if (need <= 256 && l2_heads) D = 256;
  else if (need <= 512) D = std::max(320, (need + 63) / 64 * 64);
  else D = (need + 127) / 128 * 128;
  if (D > 1024)
    return fail(GNOT_E_INVALID, "hidden width must be at most 1024 on the MI355X kernels (n_head times the head "
                                "width rounded up to a multiple of 4, with padded heads)");
  if (D > 512 && 64 % dh != 0)
    return fail(GNOT_E_INVALID, "above an internal width of 512 the head width must divide 64 on the MI355X "
                                "kernels");
  if ((D != 256 && (linear_oc(D, 3 * D, 2 * D, dh) < 0 || linear_oc(D, D, D, dh) < 0)) || linear_oc(D, 2 * D, 1, dh) < 0)
    return fail(GNOT_E_INVALID, "no projection tiling keeps whole heads of this head width on the MI355X kernels");
  if (c.n_expert < 1 || c.n_attn_layers < 0 || c.n_input_functions < 0 || c.n_input_functions > 8)
    return fail(GNOT_E_INVALID, "bad n_expert / n_attn_layers / n_input_functions");
  if (c.input_dim + c.theta_dim > Dr || c.input_dim > Dr || c.input_func_dim > Dr || c.out_dim > Dr ||
      c.n_expert > Dr || c.input_dim < 1 || c.out_dim < 1)
    return fail(GNOT_E_INVALID, "input/output widths must be in [1, hidden width]");
  if (c.theta_dim < 0) return fail(GNOT_E_INVALID, "theta_dim must not be negative");
  if (c.n_input_functions > 0 && c.input_func_dim < 1)
    return fail(GNOT_E_INVALID, "input_func_dim must be in [1, hidden width] when n_input_functions > 0");
  gnot_plan* p = new gnot_plan();
  p->c = c;
  p->D = D; p->Dr = Dr; p->H = c.n_head; p->dh = dh; p->dhr = dhr; p->E = c.n_expert; p->L = c.n_attn_layers;
  p->I = c.n_input_functions; p->KI = std::max(p->I, 1); p->DT = D / 16;
  p->NL = std::max(c.n_mlp_num_layers, 1) + 1;   // MLP(nl) has max(nl,1)+1 Linears (model.py:9-14)
  p->in = c.input_dim; p->th = c.theta_dim; p->F = c.input_func_dim; p->out = c.out_dim;
  p->in_raw = p->in; p->F_raw = p->F;
  const int NL = p->NL;
  // canonical Linears at the model's width Dr (= named_parameters() shapes)
  auto mlp = [&](int in, int outd) {
    for (int j = 0; j < NL; ++j) add_linear(p, j == NL - 1 ? outd : Dr, j == 0 ? in : Dr);
  };
  mlp(p->in + p->th, Dr);                                  // x
  mlp(p->in, p->E);                                        // gating
  for (int i = 0; i < p->I; ++i) mlp(p->F, Dr);            // input_func_mlps
  for (int l = 0; l < p->L; ++l) {
    for (int k = 0; k < 2 + 2 * p->KI; ++k) add_linear(p, Dr, Dr);   // cross q, fc_out, keys, values
    for (int k = 0; k < 4; ++k) add_linear(p, Dr, Dr);               // self q, fc_out, key, value
    for (int e = 0; e < 2 * p->E; ++e) mlp(Dr, Dr);                  // ffn1, ffn2 experts
  }
  mlp(Dr, p->out);                                         // out
  if ((int)p->lin_o.size() != p->n_lin()) {
    delete p;
    return fail(GNOT_E_INVALID, "internal: linear count mismatch");
  }
  p->W.assign(p->n_lin(), nullptr);
  p->b.assign(p->n_lin(), nullptr);
  p->tune = tuning_from_env();
  *out = p;
  return GNOT_OK;
}

extern "C" void gnot_plan_destroy(gnot_plan* plan) {
  if (!plan) return;
  for (hipEvent_t e : plan->prof_events) (void)hipEventDestroy(e);
  for (hipEvent_t e : plan->evs) (void)hipEventDestroy(e);
  for (int k = 0; k < gnot_plan::kStageSlots; ++k) {
    if (plan->stage_ev[k]) {
      (void)hipEventSynchronize(plan->stage_ev[k]);
      (void)hipEventDestroy(plan->stage_ev[k]);
    }
    if (plan->stage[k]) (void)hipHostFree(plan->stage[k]);
  }
  if (plan->side) (void)hipStreamDestroy(plan->side);
  if (plan->comm_stream) (void)hipStreamDestroy(plan->comm_stream);
  if (plan->side2) (void)hipStreamDestroy(plan->side2);
  delete plan;
}

extern "C" int gnot_plan_num_linears(const gnot_plan* p) { return p ? p->n_lin() : 0; }

extern "C" int gnot_plan_linear_dims(const gnot_plan* p, int32_t* dims) {
  if (!p || !dims) return fail(GNOT_E_INVALID, "null argument");
  for (int i = 0; i < p->n_lin(); ++i) {
    dims[2 * i] = p->lin_o[i];
    dims[2 * i + 1] = p->lin_i[i];
  }
  return GNOT_OK;
}

extern "C" int gnot_plan_bind_params(gnot_plan* p, const float* const* weights, const float* const* biases) {
  if (!p || !weights || !biases) return fail(GNOT_E_INVALID, "null argument");
  for (int i = 0; i < p->n_lin(); ++i) {
    if (!weights[i] || !biases[i]) return fail(GNOT_E_INVALID, "null parameter pointer");
    p->W[i] = weights[i];
    p->b[i] = biases[i];
  }
  p->params_bound = true;
  p->packed = false;
  return GNOT_OK;
}

// ====================================================================== layout
namespace {

struct Carver {
  size_t top = 0;
  gnot_plan* p;
  void add(const std::string& name, size_t nfloats, long ld) {
    Buf b;
    b.off = top;
    b.ld = ld;
    top += ((nfloats * sizeof(float) + 255) / 256) * 256;
    p->bufs[name] = b;
    p->buf_order.push_back(name);
  }
  size_t raw(size_t bytes) {
    const size_t o = top;
    top += ((bytes + 255) / 256) * 256;
    return o;
  }
};

void make_chunks(const std::vector<long>& off, std::vector<int4>& ch, std::vector<int>& choff) {
  ch.clear();
  choff.assign(1, 0);
  const int B = (int)off.size() - 1;
  for (int b = 0; b < B; ++b) {
    for (long s = off[b]; s < off[b + 1]; s += kSeg) {
      const int len = (int)std::min<long>(kSeg, off[b + 1] - s);
      ch.push_back(make_int4(b, (int)s, len, 0));
    }
    choff.push_back((int)ch.size());
  }
}

}  // namespace

// the chain call sites of the current batch, in the one order gnot_plan::ch_x() .. ch_out() index
static void build_chains(gnot_plan* p) {
  const int D = p->D, NL = p->NL;
  p->chains.clear();
  auto add = [&](std::vector<int> firsts, int in_dim, int out_dim, int kcall, long rows, const std::string& x,
                 const std::string& save, int mode) {
    Chain C;
    C.in_dim = in_dim; C.out_dim = out_dim;
    C.KT0 = in_dim <= 16 ? 1 : p->DT;
    C.OTL = out_dim <= 16 ? 1 : p->DT;
    C.kcall = kcall; C.rows = rows; C.x = x; C.save = save; C.mode = mode;
    C.layers.assign(firsts.size() * NL, ChainLayer{nullptr, nullptr, nullptr});
    C.firsts = std::move(firsts);
    p->chains.push_back(std::move(C));
  };
  add({p->lin_x(0)}, p->in + p->th, D, p->k_x(), p->P, "xin", "x_save", CH_STORE);
  add({p->lin_g(0)}, p->in, p->E, p->k_gate(), p->P, "x", "gate_save", CH_SOFTMAX);
  for (int i = 0; i < p->I; ++i) {
    const std::string si = std::to_string(i);
    add({p->lin_fn(i, 0)}, p->F, D, p->k_fn(i), p->Q[i], "fn" + si, "fn_save" + si, CH_STORE);
  }
  for (int l = 0; l < p->L; ++l) {
    const std::string s = "b" + std::to_string(l) + ".";
    std::vector<int> f1, f2;
    for (int e = 0; e < p->E; ++e) { f1.push_back(p->lin_f1(l, e, 0)); f2.push_back(p->lin_f2(l, e, 0)); }
    add(f1, D, D, p->k_m1(l), p->P, s + "a", p->msave(l, true), CH_MOE);
    add(f2, D, D, p->k_m2(l), p->P, s + "bb", p->msave(l, false), CH_MOE);
  }
  add({p->lin_out(0)}, D, p->out, p->k_out(), p->P, p->final_query(), "out_save", CH_STORE);
}

// the attention calls of the current batch, in the one order gnot_plan::call(l, cross) indexes.  A cross call with
// input functions projects q alone and reads one source per input function, whose K | V rows, states and
// backward run batched over all blocks; every other call (self, and a cross module without input functions)
// is fused: one q|k|v projection of its own rows, one source
static void build_attn_calls(gnot_plan* p) {
  p->attn.clear();
  for (int l = 0; l < p->L; ++l)
    for (bool cross : {true, false}) {
      const std::string b = "b" + std::to_string(l) + ".", s = b + (cross ? "c" : "s");
      AttnCall a;
      a.l = l; a.cross = cross; a.site = (uint32_t)(2 * l + (cross ? 0 : 1));
      a.fused = !(cross && p->I > 0);
      a.nsrc = a.fused ? 1 : p->I;
      // canonical Linears of block l: cross q, fc_out, KI keys, KI values, then self q, fc_out, key, value
      const int nkv = cross ? p->KI : 1;
      a.q = p->blk(l) + (cross ? 0 : 2 + 2 * p->KI);
      a.o = a.q + 1;
      for (int i = 0; i < nkv; ++i) { a.k.push_back(a.q + 2 + i); a.v.push_back(a.q + 2 + nkv + i); }
      a.in_raw = cross ? p->block_query(l) : b + "query1";
      a.in = p->pre_norm ? b + (cross ? "n1" : "n2") : a.in_raw;
      a.rstd = b + (cross ? "r1" : "r2");
      a.proj = s + "q"; a.pitch = (a.fused ? 3 : 1) * (long)p->D;
      a.res = s + "res"; a.out = b + (cross ? "a" : "bb");
      a.dsum = cross ? "dsum1" : "dsum0"; a.dqkv = cross ? "dqkv1" : "dqkv0";
      for (int i = 0; i < a.nsrc; ++i) {
        const std::string si = std::to_string(i), li = std::to_string(l) + "_" + si;
        AttnSrc r;
        r.state = s + "state" + (cross ? si : "");
        r.du = "du" + si; r.dden = "dden" + si;
        r.dstate = "dstate0";
        if (!a.fused) {                      // its dS | dz and dK | dV are kept per (block, source) for the batched side
          r.fn = i; r.ckv = s + "kv" + si; r.enc = (p->pre_norm ? "fnn" : "fnenc") + si;
          r.dstate = "dstate" + li; r.dkv = "dkv" + li;
        }
        a.src.push_back(std::move(r));
      }
      p->attn.push_back(std::move(a));
    }
}

// build the packed-weight images and pack jobs (offsets relative to the packed arena)
static void plan_images(gnot_plan* p) {
  const int DT = p->DT, NL = p->NL;
  p->pack_jobs.clear();
  p->pack_dst_off4.clear();
  p->pack_bias_off.clear();
  p->fwd_img.assign(p->n_lin(), Img());
  p->T_img.assign(p->n_lin(), Img());
  p->fwd_bias.assign(p->n_lin(), 0);
  p->packed4 = 0;
  p->pbias = 0;
  auto new_img = [&](int OT, int KT) {
    Img im;
    im.off4 = p->packed4;
    im.OT = OT;
    im.KT = KT;
    p->packed4 += (size_t)OT * KT * 64;
    return im;
  };
  // bf16x6 image (chain kernels): OT x ceil(KT/2) blocks of `np` pieces x 64 lanes x 16 B
  auto new_img_x6 = [&](int OT, int KT, int np = 3) {
    Img im;
    im.off4 = p->packed4;
    im.OT = OT;
    im.KT = KT;
    p->packed4 += (size_t)OT * ((KT + 1) / 2) * np * 64;
    return im;
  };
  auto new_bias = [&](int n) {
    const size_t o = p->pbias;
    p->pbias += (size_t)((n + 63) / 64) * 64;
    return o;
  };
  // job: linear li into image im at tile offsets (o0, t0); transposed flag; bias destination
  // heads: a q / k / v projection (padded heads: its rows placed in heads of dh, PackJob::hr / hp)
  auto job = [&](int li, const Img& im, int o0, int t0, int OTp, int KTp, int tr, long bias_off, int x6 = 0,
                 bool heads = false) {
    PackJob J{};
    J.x6 = x6;
    J.out = p->lin_o[li];
    J.in = p->lin_i[li];
    if (heads && p->head_padded()) {
      J.hr = p->dhr;
      J.hp = p->dh;
      J.out = p->hd();
    }
    J.transposed = tr;
    J.o0 = o0; J.t0 = t0; J.ktot = im.KT; J.otot = im.OT;
    // internal widths above 512: a full-width contraction packed as two half images (launch_linear's K-split)
    if (x6 == 0 && p->D > 512 && im.KT == p->DT) J.kh = p->DT / 2;
    J.OTp = OTp; J.KTp = KTp;
    p->pack_jobs.push_back(J);
    p->pack_dst_off4.push_back(im.off4);
    p->pack_bias_off.push_back(bias_off < 0 ? (size_t)-1 : (size_t)bias_off);
    // remember which linear: encode in W/b later
    p->pack_jobs.back().W = reinterpret_cast<const float*>((intptr_t)li);
  };
  // d = 256: chain2.hip, bf16x6 output-major images in both directions; else chain.hip, k-major x6
  // forward image + exact fp32 backward-data image (bf16 mode: k-major one-piece images both ways, and the
  // projections on output-major one-piece images, linear.hip)
  const bool c2 = p->D == 256;
  const int c2np = c2 ? p->np : 3;                 // pieces of the output-major images
  const int c2x6 = c2np == 1 ? 3 : 2;              // their pack mode
  // d > 256 (chainw.hip: each Linear on linear.hip): fp32 fragment images in both directions
  const bool cw = p->D > 256;
  const bool b1 = !c2 && !cw && p->npk() == 1;      // d <= 192 in the bf16 mode
  auto chain_imgs = [&](const Chain& C, int c) {     // the images of parallel chain c of call site C
    for (int j = 0; j < NL; ++j) {
      const int li = C.firsts[c] + j;
      const int KTp = (j == 0) ? C.KT0 : DT;
      const int OTp = (j == NL - 1) ? C.OTL : DT;
      Img f = cw ? new_img(OTp, KTp) : new_img_x6(OTp, KTp, c2 ? c2np : b1 ? 1 : 3);
      const size_t bo = new_bias(16 * OTp);
      job(li, f, 0, 0, OTp, KTp, 0, (long)bo, cw ? 0 : c2 ? c2x6 : b1 ? 4 : 1);
      // backward-data image: d <= 192 k-major x6 or one-piece (bf16 mode), else fp32 tiles
      const bool tx6 = !c2 && !cw;
      Img t = c2 ? new_img_x6(KTp, OTp, c2np) : tx6 ? new_img_x6(KTp, OTp, b1 ? 1 : 3) : new_img(KTp, OTp);
      job(li, t, 0, 0, KTp, OTp, 1, -1, c2 ? c2x6 : tx6 ? (b1 ? 4 : 1) : 0);
      p->fwd_img[li] = f;
      p->T_img[li] = t;
      p->fwd_bias[li] = bo;
    }
  };
  // the order images are created in IS the packed arena's layout: encoders, then per block the attention
  // images and per expert ffn1_e, ffn2_e, then the decoder
  chain_imgs(p->ch_x(), 0);
  chain_imgs(p->ch_gate(), 0);
  for (int i = 0; i < p->I; ++i) chain_imgs(p->ch_fn(i), 0);
  // attention projections: at d = 256 the q | q|k|v | fc_out images and the backward-data images that
  // linear2.hip uses are output-major bf16x6; the input-function K/V images and their backward-data
  // images stay fp32 for the batched linear.hip kernel
  auto attn_imgs = [&](AttnCall& A) {
    const int D = p->D;
    const bool lx6 = p->lin_img() == 3;   // fp32 mode at d <= 192: output-major x6
    const int x6 = c2 ? c2x6 : b1 ? 3 : lx6 ? 2 : 0;
    auto img = [&](int OT, int KT) {
      return c2 ? new_img_x6(OT, KT, c2np) : b1 ? new_img_x6(OT, KT, 1) : lx6 ? new_img_x6(OT, KT, 3) : new_img(OT, KT);
    };
    A.proj_img = img((int)(A.pitch / 16), DT);
    A.bproj = new_bias((int)A.pitch);
    job(A.q, A.proj_img, 0, 0, DT, DT, 0, (long)A.bproj, x6, true);
    if (A.fused) {
      job(A.k[0], A.proj_img, DT, 0, DT, DT, 0, (long)(A.bproj + D), x6, true);
      job(A.v[0], A.proj_img, 2 * DT, 0, DT, DT, 0, (long)(A.bproj + 2 * D), x6, true);
    }
    for (int i = 0; i < (A.fused ? 0 : A.nsrc); ++i) {   // K | V of the input-function sources: batched fp32 kernel
      Img kv = new_img(2 * DT, DT);
      const size_t bkv = new_bias(2 * D);
      job(A.k[i], kv, 0, 0, DT, DT, 0, (long)bkv, 0, true);
      job(A.v[i], kv, DT, 0, DT, DT, 0, (long)(bkv + D), 0, true);
      A.kv_img.push_back(kv);
      A.bkv.push_back(bkv);
    }
    A.o_img = img(DT, DT);
    A.bo = new_bias(D);
    job(A.o, A.o_img, 0, 0, DT, DT, 0, (long)A.bo, x6);
    // backward-data images: q, fc_out, then the keys / values (input-function ones: the batched fp32 kernel's)
    auto t_img = [&](int li, bool own, bool heads) {
      Img t = own ? img(DT, DT) : new_img(DT, DT);
      job(li, t, 0, 0, DT, DT, 1, -1, own ? x6 : 0, heads);
      p->T_img[li] = t;
    };
    t_img(A.q, true, true);
    t_img(A.o, true, false);
    for (size_t i = 0; i < A.k.size(); ++i) { t_img(A.k[i], A.fused, true); t_img(A.v[i], A.fused, true); }
  };
  for (int l = 0; l < p->L; ++l) {
    attn_imgs(p->call(l, true));
    attn_imgs(p->call(l, false));
    for (int e = 0; e < p->E; ++e) {
      chain_imgs(p->ch_moe(l, true), e);
      chain_imgs(p->ch_moe(l, false), e);
    }
  }
  chain_imgs(p->ch_out(), 0);
  p->pack_prefix.clear();
  int acc = 0;
  for (auto& J : p->pack_jobs) {
    p->pack_prefix.push_back(acc);
    acc += pack_tiles(J);
  }
  p->pack_tiles = acc;
}

// ====================================================================== point-reduction GEMM groups
// the workgroup count balanced_wgrad tests the job count against
constexpr long kBalanceWgs = 256;
// balanced point ranges for a Wide256 / B16Rows group (finish_group) when a per-job split count would leave CUs
// idle and every job has a point range of its own (no zero-point jobs).
// kBalanceWgs is the large plans' target; a small plan's group aims at 128 or 64 workgroups (finish_group) and is
// still tested against 256 here.  Kept as it is on purpose: testing against the group's own target would move
// range boundaries, hence the summation order and the bits of those plans' gradients
static bool balanced_wgrad(const WgradGroup& G) {
  if (G.jobs.size() < 2) return false;
  for (const auto& J : G.jobs)
    if (J.P <= 0) return false;
  return kBalanceWgs % (long)G.jobs.size() != 0;
}
// One weight-gradient group (jobs of lin_job: dz, x, out, in, P): its kernel, split-K counts, slab offsets and
// launch tables.  b16_rows: the jobs' rows are bf16 storage (moe_group_b16)
static void finish_group(gnot_plan* p, WgradGroup& G, bool b16_rows = false) {
  // the kernel.  d = 256: every job's whole 256 x 256 gradient in one workgroup (8 waves, 96 KiB LDS: one per
  // CU).  d <= 128 (configs[1]): the same design at a 128 x 128 output (4 waves, staging interleaved with the
  // MFMAs, raw rows by LDS-DMA) instead of the 128-tile kernel (round 5: configs[1] 3.44 -> 3.37 ms)
  auto within = [&](int edge) {
    for (const auto& J : G.jobs)
      if (J.out > edge || J.in > edge) return false;
    return !G.jobs.empty();
  };
  G.kind = b16_rows                     ? WgradKernel::B16Rows
           : p->D == 256 && within(256) ? WgradKernel::Wide256
           : p->D <= 128 && within(128) ? WgradKernel::Wide128
                                        : WgradKernel::Tile128;
  const bool tiled = G.kind == WgradKernel::Tile128;   // else one workgroup per (job, split)
  G.scaled = false;
  for (const auto& J : G.jobs)
    if (J.scale != nullptr || J.ldscale != 0) G.scaled = true;   // (ldscale: the sizing pass has null pointers)
  // the split-K target, in workgroups.  The 128-tile kernel holds ~240 registers per lane: one workgroup per CU
  // leaves the other half of every SIMD's register file to the concurrent main-stream kernels.  The 256 x 256
  // kernels' target is fixed (r02bh: 192-512 all within noise), so the split counts the parity tests exercise
  // are the ones every run uses.
  // Plans below kWgradSerialPoints fork their weight gradients beside the caller's stream (serial_wgrad): a
  // group holding every CU's register file (the 256 x 256 kernel: 8 waves of 256 registers per CU) leaves the
  // concurrent critical-path kernels no room, so such plans' groups take fewer workgroups.  Keyed on the plan
  // size, not on the fork itself, so a plan gives bitwise the same gradients forked or serial
  // (GNOT_WGRAD_OVERLAP, tests/test_gpu_recompute.py).  Measured (round 6, interleaved sweeps
  // `profiles/r06sw*`): configs[0] (d = 256) 128 workgroups in fp32 (9.54 -> 9.00 ms per step against 256),
  // 64 in the bf16 mode (5.88 -> 5.47); configs[1] (the 128 x 128 kernel) 192 in fp32 (3.28 -> 3.21), 128 in
  // the bf16 mode (the round-5 value)
  const bool small = p->P < gnot_plan::kWgradSerialPoints;
  const bool bf16 = p->npk() == 1;
  const long target = tiled                          ? 256
                      : G.kind == WgradKernel::Wide128 ? (small && !bf16 ? 192 : 128)
                                                       : (!small ? 256 : bf16 ? 64 : 128);
  long tiles = 0;
  for (auto& J : G.jobs) {
    J.tiles_o = (J.out + kPTile - 1) / kPTile;
    J.tiles_i = (J.in + kPTile - 1) / kPTile;
    tiles += tiled ? J.tiles_o * J.tiles_i : 1;
  }
  // floor, not ceil: never more than `target` workgroups, so no CU runs one more than planned
  const long want = std::max<long>(1, target / std::max<long>(tiles, 1));
  // the one-workgroup-per-split kernels address a split through a buffer resource based at its first row with
  // 32-bit offsets: a split's rows (+ the stage loaded past its end) stay below 2^31 bytes (every kind is
  // split by this bound)
  auto row_bytes = [&](const WgradJob& J) {
    return b16_rows ? 512L : 4L * std::max<long>(std::max<long>(J.lddz, J.ldx), 1);
  };
  G.wg_prefix.clear();
  G.red_prefix.clear();
  G.segs.clear();
  G.seg_start.clear();
  G.slab_floats = 0;
  const bool balanced = (G.kind == WgradKernel::Wide256 || G.kind == WgradKernel::B16Rows) && balanced_wgrad(G);
  if (balanced) {
    // the 256 x 256 kernel holds one workgroup per CU: a per-job split count leaves target % jobs CUs idle
    // (the 40 soft-MoE jobs of configs[2]: 6 splits each = 240 of 256), so cut the group's concatenated
    // points into `target` equal ranges instead (a range crossing a job boundary runs as two segments)
    long T = 0, maxrow = 1;
    for (const auto& J : G.jobs) {
      T += J.P;
      maxrow = std::max<long>(maxrow, row_bytes(J));
    }
    long C = std::max<long>((T + target - 1) / target, kMinSplitPoints);
    C = (C + 31) / 32 * 32;                                 // whole stages (kWStage 16, kBStage 32 points)
    C = std::min<long>(C, ((1L << 31) - 1) / maxrow - 64);  // a range's rows stay below 2^31 bytes
    std::vector<long> jstart(G.jobs.size() + 1, 0);
    for (size_t j = 0; j < G.jobs.size(); ++j) jstart[j + 1] = jstart[j] + G.jobs[j].P;
    std::vector<int> nslots(G.jobs.size(), 0);
    size_t jj = 0;
    for (long w0 = 0; w0 < T; w0 += C) {
      const long w1 = std::min(T, w0 + C);
      G.seg_start.push_back((int)G.segs.size());
      while (jj < G.jobs.size() && jstart[jj + 1] <= w0) ++jj;
      for (size_t j = jj; j < G.jobs.size() && jstart[j] < w1; ++j) {
        const long b = std::max(w0, jstart[j]) - jstart[j], e = std::min(w1, jstart[j + 1]) - jstart[j];
        if (e > b) G.segs.push_back(int4{(int)j, nslots[j]++, (int)b, (int)e});
      }
    }
    G.seg_start.push_back((int)G.segs.size());
    for (size_t j = 0; j < G.jobs.size(); ++j) G.jobs[j].splits = std::max(1, nslots[j]);
  } else {
    for (auto& J : G.jobs) {
      const long minpts = kMinSplitPoints;   // >= 4 LDS stages per workgroup: bounds the split-K slab traffic
      const long maxs = std::max<long>(1, (J.P + minpts - 1) / minpts);
      J.splits = (int)std::min<long>(std::min<long>(want, maxs), 256);
      const long max_pts = ((1L << 31) - 1) / row_bytes(J) - 64;
      J.splits = (int)std::max<long>(J.splits, (J.P + max_pts - 1) / max_pts);
    }
  }
  // slab offsets and the two prefixes (balanced: the workgroups are the ranges, the kernel reads no prefix)
  int wg = 0, red = 0;
  for (auto& J : G.jobs) {
    const int nt = J.tiles_o * J.tiles_i;
    J.slab_off = (long)G.slab_floats;
    G.slab_floats += (size_t)J.splits * nt * kPTile * (kPTile + 1);
    G.wg_prefix.push_back(balanced ? 0 : wg);
    wg += (tiled ? nt : 1) * J.splits;
    G.red_prefix.push_back(red);
    red += nt * kPTile * (kPTile + 1);
  }
  G.total_wgs = balanced ? (int)G.seg_start.size() - 1 : wg;
  G.total_red = red;
  p->slab_wgrad_floats = std::max(p->slab_wgrad_floats, G.slab_floats);
}

// attention-state group (state.hip): one job per sample, ceil(P / kStatePts) partial states each
static void finish_state_group(gnot_plan* p, WgradGroup& G) {
  if (!G.jobs.empty()) {
    const int d = G.jobs[0].out;
    const int dh = G.jobs[0].state_dh;
    long total = 0;
    for (const auto& J : G.jobs) total += J.P;
    G.state_mfma = state_mfma_ok(d, dh) && total >= p->tune.state_mfma_min_points;
    G.state_pts = state_pts(G.state_mfma, d);
    G.state_nw = 0;
    for (const auto& J : G.jobs)
      if (J.ldw > 0) G.state_nw = d / J.state_dh;
  }
  G.wg_prefix.clear();
  G.red_prefix.clear();
  G.slab_floats = 0;
  int wg = 0, red = 0;
  for (auto& J : G.jobs) {
    const int per = J.out / J.state_dh * (J.state_dh * J.state_dh + J.state_dh);
    J.splits = std::max(1, (J.P + G.state_pts - 1) / G.state_pts);
    J.slab_off = (long)G.slab_floats;
    G.slab_floats += (size_t)J.splits * per;
    G.wg_prefix.push_back(wg);
    wg += J.splits;
    G.red_prefix.push_back(red);
    red += per;
  }
  G.total_wgs = wg;
  G.total_red = red;
  p->slab_state_floats = std::max(p->slab_state_floats, G.slab_floats);
}

template <typename F>
static void for_each_group(gnot_plan* p, F&& f) {
  if (p->training) {
    for (Chain& C : p->chains) f(C.wg);
    for (int l = 0; l < p->L; ++l) { f(p->call(l, false).wg); f(p->call(l, true).wg); }
    f(p->wg_fnkv);
  }
  f(p->st_fn);
  for (int l = 0; l < p->L; ++l)             // per block: the forward states of both calls, then the backward's
    for (int bwd = 0; bwd <= (p->training ? 1 : 0); ++bwd)
      for (bool cross : {true, false})
        for (AttnSrc& r : p->call(l, cross).src) f(bwd ? r.dst : r.st);
}

// (Re)build every job list from the current buffer pointers.  Before bind every buffer is null and so is every
// pointer in the jobs (P_ / at): that pass is for the table and slab sizes, which depend on shapes alone.
static void build_groups(gnot_plan* p) {
  p->slab_wgrad_floats = 0;
  p->slab_state_floats = 0;
  const long P = p->P;
  const int D = p->D, NL = p->NL, dh = p->dh;
  const bool tr = p->training;
  const long per_state = p->per_state();
  float* const grads = p->grads();
  for (Chain& C : p->chains) C.wg = {};
  p->wg_fnkv = {};
  p->st_fn = {};
  for (AttnCall& a : p->attn) {
    a.wg = {};
    for (AttnSrc& r : a.src) r.st = r.dst = {};
  }

  auto lin_job = [&](WgradGroup& G, int li, const float* dz, long lddz, const float* x, long ldx, int gelu,
                     long rows) {
    if (p->frozen(li)) return;
    WgradJob J{};
    J.dz = dz; J.lddz = lddz; J.x = x; J.ldx = ldx; J.x_gelu = gelu;
    J.out = p->lin_o[li]; J.in = p->lin_i[li];
    J.dW = at(grads, p->grad_off[2 * li]);
    J.db = at(grads, p->grad_off[2 * li + 1]);
    J.P = (int)rows;
    G.jobs.push_back(J);
    G.lins.push_back(li);
  };
  // a q / k / v projection's gradients: dz in heads of dh; padded heads: one job per head (its dhr real
  // rows of the canonical dW / db)
  auto lin_job_heads = [&](WgradGroup& G, int li, const float* dz, long lddz, const float* x, long ldx, long rows) {
    if (p->frozen(li)) return;
    if (!p->head_padded()) {
      lin_job(G, li, dz, lddz, x, ldx, 0, rows);
      return;
    }
    const int in = p->lin_i[li];
    for (int h = 0; h < p->H; ++h) {
      WgradJob J{};
      J.dz = at(dz, (long)h * dh); J.lddz = lddz; J.x = x; J.ldx = ldx; J.x_gelu = 0;
      J.out = p->dhr; J.in = in;
      J.dW = at(grads, p->grad_off[2 * li] + (long)h * p->dhr * in);
      J.db = at(grads, p->grad_off[2 * li + 1] + (long)h * p->dhr);
      J.P = (int)rows;
      G.jobs.push_back(J);
    }
    G.lins.push_back(li);
  };
  // chain c of a call site: Linear j reads dZ_j from dz[(c*NL + j)*rows*D] and its input from the
  // chain input (j = 0) or gelu(saved pre-activation j-1)
  auto chain_group = [&](Chain& C) {
    const float* dz = p->P_(p->dz_name(C.kcall));
    const float* save = p->P_(C.save);
    const Buf& x0 = p->bufs.at(C.x);
    const long rows = C.rows;
    // moe_direct_dz: expert c's last Linear reads dquery scaled by its score column instead of a stored dz
    const bool direct = C.mode == CH_MOE && p->moe_direct_dz();
    const Buf& sc = p->bufs.at("scores");
    for (size_t c = 0; c < C.firsts.size(); ++c)
      for (int j = 0; j < NL; ++j) {
        const float* dzp = at(dz, ((long)c * NL + j) * rows * D);
        if (j == 0) {
          lin_job(C.wg, C.firsts[c] + j, dzp, D, x0.p, x0.ld, 0, rows);
        } else if (direct && j == NL - 1) {
          if (p->frozen(C.firsts[c] + j)) continue;      // no job whose scale to set
          lin_job(C.wg, C.firsts[c] + j, p->P_("dquery"), D, at(save, ((long)c * NL + j - 1) * rows * D), D, 1, rows);
          C.wg.jobs.back().scale = at(sc.p, (long)c);
          C.wg.jobs.back().ldscale = (int)sc.ld;
        } else {
          lin_job(C.wg, C.firsts[c] + j, dzp, D, at(save, ((long)c * NL + j - 1) * rows * D), D, 1, rows);
        }
      }
    finish_group(p, C.wg);
  };
  // bf16-storage soft-MoE group (bf16 mode): dZ_j of chain c at dz + (c NL + j) lay, the input of Linear
  // j > 0 in save slot NL + j of chain c, Linear 0's (the shared MoE input) in chain 0's slot NL
  auto moe_group_b16 = [&](Chain& C) {
    const float* dz = p->P_(p->dz_name(C.kcall));
    const float* save = p->P_(C.save);
    const long lay = P * D / 2;
    for (size_t c = 0; c < C.firsts.size(); ++c)
      for (int j = 0; j < NL; ++j) {
        const float* x = at(save, (j == 0 ? NL : (long)c * 2 * NL + NL + j) * lay);
        lin_job(C.wg, C.firsts[c] + j, at(dz, ((long)c * NL + j) * lay), D, x, D, 0, P);
      }
    finish_group(p, C.wg, true);
  };
  auto state_group = [&](WgradGroup& G, const float* A, long lda, const float* Bm, long ldb, const float* w,
                         long ldw, const std::vector<long>& off, float* state) {
    for (int b = 0; b < p->B; ++b) {
      WgradJob J{};
      J.dz = at(A, off[b] * lda); J.lddz = lda;
      J.x = at(Bm, off[b] * ldb); J.ldx = ldb;
      J.out = p->hd(); J.in = p->hd();            // H heads of dh (the internal head width)
      J.dW = at(state, b * per_state);
      J.db = J.dW;
      J.w = at(w, off[b] * ldw); J.ldw = ldw;
      J.state_dh = dh;
      J.P = (int)(off[b + 1] - off[b]);
      G.jobs.push_back(J);
    }
    finish_state_group(p, G);
  };

  for (AttnCall& a : p->attn) {
    // a fused call's forward states S = k^T v, z = sum k (the input-function sources of all blocks: st_fn, below)
    if (a.fused)
      state_group(a.src[0].st, p->P_(a.proj, D), a.pitch, p->P_(a.proj, 2 * D), a.pitch, nullptr, 0, p->xoff,
                  p->P_(a.src[0].state));
    // backward states dS = sum q^T du, dz = sum dden q
    for (AttnSrc& r : a.src)
      if (tr) state_group(r.dst, p->P_(a.proj), a.pitch, p->P_(r.du), D, p->P_(r.dden), p->H, p->xoff, p->P_(r.dstate));
  }
  // the batched input-function side, walking the unfused calls' sources in (block, fn) order
  for (AttnCall& a : p->attn)
    for (int i = 0; i < (a.fused ? 0 : a.nsrc); ++i) {
      const AttnSrc& r = a.src[i];
      // one state job per sample: S = k^T v, z = sum k over that sample's input-function points
      float* kv = p->P_(r.ckv);
      float* st = p->P_(r.state);
      for (int b = 0; b < p->B; ++b) {
        WgradJob J{};
        const long o = p->fnoff[r.fn][b];
        J.dz = at(kv, o * 2 * D); J.lddz = 2 * D; J.x = at(kv, D + o * 2 * D); J.ldx = 2 * D;
        J.out = p->hd(); J.in = p->hd(); J.dW = at(st, b * per_state); J.db = J.dW;
        J.state_dh = dh; J.P = (int)(p->fnoff[r.fn][b + 1] - o);
        p->st_fn.jobs.push_back(J);
      }
      if (!tr) continue;
      lin_job_heads(p->wg_fnkv, a.k[i], p->P_(r.dkv), 2 * D, p->P_(r.enc), D, p->Q[r.fn]);
      lin_job_heads(p->wg_fnkv, a.v[i], p->P_(r.dkv, D), 2 * D, p->P_(r.enc), D, p->Q[r.fn]);
    }
  if (p->I > 0) finish_state_group(p, p->st_fn);
  if (!tr) return;
  if (p->I > 0) finish_group(p, p->wg_fnkv);

  for (Chain& C : p->chains) {
    if (C.mode == CH_MOE && p->b16s()) moe_group_b16(C);
    else chain_group(C);
  }
  for (AttnCall& a : p->attn) {
    const float* in = p->P_(a.in);
    lin_job(a.wg, a.o, p->P_(a.dsum), D, p->P_(a.res), p->Dr, 0, P);
    lin_job_heads(a.wg, a.q, p->P_(a.dqkv), a.pitch, in, D, P);
    if (a.fused) {                                 // (an unfused call's key / value gradients: wg_fnkv)
      lin_job_heads(a.wg, a.k[0], p->P_(a.dqkv, D), a.pitch, in, D, P);
      lin_job_heads(a.wg, a.v[0], p->P_(a.dqkv, 2 * D), a.pitch, in, D, P);
    }
    finish_group(p, a.wg);
  }
}

// internal widths above 512: a batched projection job's segments as K-halves (launch_linear's K-split done on
// the host: the batched kernel reads its jobs from device memory and runs at D / 2)
static void ksplit_job(const gnot_plan* p, LinearArgs& a) {
  if (p->D <= 512) return;
  const int Kh = p->D / 2;
  const long half4 = (long)(a.NO / 16) * (Kh / 16) * 64;   // the second half image (64 float4 per tile)
  LinearArgs b = a;
  b.nseg = 2 * a.nseg;
  for (int k = 0; k < b.nseg; ++k) {
    b.X[k] = at(a.X[k / 2], (k % 2) * Kh);
    b.Wp[k] = at(a.Wp[k / 2], (k % 2) * half4);
  }
  b.K = Kh;
  b.dblk = p->D;
  a = b;
}

// The kernel form of every attention pass of this batch geometry: a function of the shapes and p->tune alone,
// so set_batch decides once and every launch obeys.  Every pitch the passes use (attn_forward, attn_backward,
// build_attn_tables) is D, 2 D or 3 D floats, D a multiple of 16
static AttnKernel attn_form(const gnot_plan* p, AttnPass pass, int nsrc, long nchunks) {
  return attn_kernel(pass, p->dh, p->dhr, p->H, nsrc, nchunks, true, p->tune.apply_mfma_min_chunks);
}
static AttnKernel apply_form(const gnot_plan* p, AttnPass pass, int nsrc) {   // a pass over the query points
  return attn_form(p, pass, nsrc, (long)p->qchunks.size());
}
static void choose_attn_forms(gnot_plan* p) {
  for (AttnCall& a : p->attn) {
    a.apply_fwd = apply_form(p, AttnPass::ApplyFwd, a.nsrc);
    a.apply_bwd = apply_form(p, AttnPass::ApplyBwd, a.nsrc);
  }
  p->kv_bwd = apply_form(p, AttnPass::KVBwd, 1);
  p->kv_batch_maxchunks = 0;
  for (int i = 0; i < p->I; ++i) p->kv_batch_maxchunks = std::max(p->kv_batch_maxchunks, (int)p->fchunks[i].size());
  p->kv_bwd_batch = attn_form(p, AttnPass::KVBwd, 1, (long)p->kv_batch_maxchunks * p->L * p->I);
}

// Device job tables of the batched input-function side of cross attention (pointers are null
// before bind: sizing only).
static void build_attn_tables(gnot_plan* p) {
  const int D = p->D, I = p->I, L = p->L;
  p->fwd_kv_jobs.clear();
  p->kvbwd_jobs.clear();
  p->dfn_jobs.clear();
  if (I == 0 || L == 0) return;
  for (int l = 0; l < L; ++l)
    for (int i = 0; i < I; ++i) {
      const AttnCall& A = p->call(l, true);
      const AttnSrc& r = A.src[i];
      LinearArgs a{};
      a.nseg = 1; a.X[0] = p->P_(r.enc); a.ldx = D; a.Wp[0] = A.kv_img[i].p; a.nsum = 1; a.K = D;
      a.bias = p->P_("pbias", A.bkv[i]); a.Y = p->P_(r.ckv); a.ldy = 2 * D; a.NO = 2 * D; a.P = (int)p->Q[i];
      a.epi = EPI_STORE; a.nsoft = D; a.dh = p->dh; a.dreal = p->attn_dreal();
      a.dhr = p->head_padded() ? p->dhr : 0;
      ksplit_job(p, a);
      p->fwd_kv_jobs.push_back(a);
    }
  if (!p->training) return;
  for (int l = 0; l < L; ++l)
    for (int i = 0; i < I; ++i) {
      const AttnSrc& r = p->call(l, true).src[i];
      const float* kv = p->P_(r.ckv);
      float* dkv = p->P_(r.dkv);
      AttnKVBwdArgs kb{};
      kb.k = kv; kb.v = at(kv, D); kb.ldkv = 2 * D; kb.dstate = p->P_(r.dstate);
      kb.chunks = p->d_fchunks[i];               // (walk_tables places the chunk tables before these jobs)
      kb.nchunks = (int)p->fchunks[i].size(); kb.H = p->H; kb.dh = p->dh;
      kb.dk = dkv; kb.dv = at(dkv, D); kb.lddkv = 2 * D;
      p->kvbwd_jobs.push_back(kb);
    }
  // d(fn encoding i) = sum_l dK_{l,i} Wk_{l,i} + dV_{l,i} Wv_{l,i}: 2L K-segments, <= kMaxSeg per launch (half
  // as many above an internal width of 512, each then two K-halves)
  const int nseg = 2 * L;
  const int per = D > 512 ? kMaxSeg / 2 : kMaxSeg;
  for (int k0 = 0; k0 < nseg; k0 += per) {
    std::vector<LinearArgs> launch;
    for (int i = 0; i < I; ++i) {
      LinearArgs a{};
      a.nseg = std::min(per, nseg - k0);
      for (int sg = 0; sg < a.nseg; ++sg) {
        const int l = (k0 + sg) / 2, kv = (k0 + sg) % 2;
        const AttnCall& A = p->call(l, true);
        a.X[sg] = p->P_(A.src[i].dkv, kv * D);
        a.Wp[sg] = p->T_img[kv ? A.v[i] : A.k[i]].p;
      }
      a.ldx = 2 * D; a.nsum = 1; a.K = D; a.bias = nullptr; a.Y = p->P_("dfn" + std::to_string(i)); a.ldy = D;
      a.NO = D; a.P = (int)p->Q[i]; a.epi = k0 == 0 ? EPI_STORE : EPI_ACCUM; a.nsoft = 0; a.dh = p->dh;
      ksplit_job(p, a);
      launch.push_back(a);
    }
    p->dfn_jobs.push_back(launch);
  }
}

// ====================================================================== device tables
// The tables lie one after another in the workspace's "__tables" region, each rounded up to 256 bytes.
// set_batch walks them unbound (no host image, no device base) to add up the region's size; bind walks them
// again to fill the host image that is uploaded and to set every device pointer.
struct TableWalk {
  char* host = nullptr;      // the region's host image (cap bytes), or null: sizing only
  char* dev = nullptr;       // the region's device address
  size_t cap = 0, cur = 0;
  void* put(const void* src, size_t bytes) {
    void* d = dev ? dev + cur : nullptr;
    if (host && bytes && cur + bytes <= cap) std::memcpy(host + cur, src, bytes);
    cur += ((bytes + 255) / 256) * 256;
    return d;
  }
  template <typename T>
  void operator()(const std::vector<T>& v, T*& d) { d = static_cast<T*>(put(v.data(), v.size() * sizeof(T))); }
};

static void shard_range(long n, int rank, int world, long& lo, long& hi);

// dropout's glo table: the global index of this rank's first point of every sample (0 unsharded), so that a
// sharded run keys its rows as the unsharded one does; empty while dropout is off
static std::vector<long> drop_first_points(const gnot_plan* p) {
  std::vector<long> glo;
  if (p->drop_T == 0) return glo;
  glo.assign(p->B, 0);
  for (int b = 0; b < p->B && p->sharded; ++b) {
    long hi;
    shard_range(p->nglob[b], p->rank, p->world, glo[b], hi);
  }
  return glo;
}

// every device table once: its host data and where its device pointer goes.  The job lists are (re)built
// here from the current buffer pointers, after the chunk tables they point into
static void walk_tables(gnot_plan* p, TableWalk& w) {
  const int I = p->I, NL = p->NL;
  // pack jobs with real pointers (the plan's own hold offsets and the Linear's index in W), resolved images
  std::vector<PackJob> jobs = p->pack_jobs;
  if (w.host) {
    float4* packed = reinterpret_cast<float4*>(p->P_("packed"));
    float* pbias = p->P_("pbias");
    for (size_t k = 0; k < jobs.size(); ++k) {
      const int li = (int)reinterpret_cast<intptr_t>(jobs[k].W);
      jobs[k].W = p->W[li];
      jobs[k].b = p->b[li];
      jobs[k].dst = packed + p->pack_dst_off4[k];
      jobs[k].bias_dst = (p->pack_bias_off[k] == (size_t)-1) ? nullptr : pbias + p->pack_bias_off[k];
    }
    auto rimg = [&](Img& im) { im.p = packed + im.off4; };
    for (auto& im : p->fwd_img) rimg(im);
    for (auto& im : p->T_img) rimg(im);
    for (AttnCall& A : p->attn) {
      rimg(A.proj_img); rimg(A.o_img);
      for (auto& k : A.kv_img) rimg(k);
    }
    for (Chain& C : p->chains) {
      C.layers.clear();
      for (int f : C.firsts)
        for (int li = f; li < f + NL; ++li)
          C.layers.push_back(ChainLayer{p->fwd_img[li].p, p->T_img[li].p, pbias + p->fwd_bias[li]});
    }
  }
  w(jobs, p->d_pack_jobs);
  w(p->pack_prefix, p->d_pack_prefix);
  for (Chain& C : p->chains) w(C.layers, C.d_layers);
  w(p->qchunks, p->d_qchunks);
  w(p->qchunk_off, p->d_qchunk_off);
  p->d_fchunks.assign(I, nullptr);
  p->d_fchunk_off.assign(I, nullptr);
  for (int i = 0; i < I; ++i) {
    w(p->fchunks[i], p->d_fchunks[i]);
    w(p->fchunk_off[i], p->d_fchunk_off[i]);
  }
  {
    std::vector<long> offs(p->xoff);
    for (int i = 0; i < I; ++i) offs.insert(offs.end(), p->fnoff[i].begin(), p->fnoff[i].end());
    w(offs, p->d_xoff);
    p->d_fnoff.assign(I, nullptr);
    for (int i = 0; i < I; ++i) p->d_fnoff[i] = at(p->d_xoff, (long)(p->B + 1) * (i + 1));
  }
  w(drop_first_points(p), p->d_glo);         // (empty without dropout: no table)
  build_groups(p);
  for_each_group(p, [&](WgradGroup& G) {
    w(G.jobs, G.d_jobs);
    std::vector<int> pre(G.wg_prefix);
    pre.insert(pre.end(), G.red_prefix.begin(), G.red_prefix.end());
    w(pre, G.d_wg_prefix);
    G.d_red_prefix = at(G.d_wg_prefix, (long)G.jobs.size());
    G.d_segs = nullptr;              // null: the launch is not a balanced one (finish_group)
    G.d_seg_start = nullptr;
    if (!G.segs.empty()) {
      w(G.segs, G.d_segs);
      w(G.seg_start, G.d_seg_start);
    }
  });
  build_attn_tables(p);
  w(p->fwd_kv_jobs, p->d_fwd_kv_jobs);
  w(p->kvbwd_jobs, p->d_kvbwd_jobs);
  p->d_dfn_jobs.assign(p->dfn_jobs.size(), nullptr);
  for (size_t k = 0; k < p->dfn_jobs.size(); ++k) w(p->dfn_jobs[k], p->d_dfn_jobs[k]);
  w(p->xsend, p->d_xsend);
  w(p->xrecv, p->d_xrecv);
  w(p->xsend_prefix, p->d_xsend_prefix);
  w(p->xrecv_prefix, p->d_xrecv_prefix);
}

// ====================================================================== point sharding
static void shard_range(long n, int rank, int world, long& lo, long& hi) {
  lo = n * rank / world;
  hi = n * (rank + 1) / world;
}

// The scramble all-to-all of one rank (see gnot_hip.h).  Flat row r = h*N_b + n of sample b's
// head-major [H, N_b, dh] apply output belongs to output token r / H.  Rank s computes the rows of
// its points n in [lo_s, hi_s) (local head-major layout: loff_s*d + (h*cnt_s + n - lo_s)*dh); rank t
// owns the tokens [lo_t, hi_t), i.e. flat rows [lo_t*H, hi_t*H), stored in token order at
// loff_t*d + (r - lo_t*H)*dh.  For every (peer, sample, head) the intersection is ONE contiguous run
// on both sides; packets are ordered (peer, sample, head) on both sides.
static void build_exchange(int B, const std::vector<long>& nglob, int H, int dh, int me, int world,
                           std::vector<CopySeg>& send, std::vector<CopySeg>& recv, std::vector<int64_t>& send_counts,
                           std::vector<int64_t>& recv_counts) {
  const long d = (long)H * dh;
  std::vector<std::vector<long>> lo(world, std::vector<long>(B)), hi = lo, loff = lo;
  for (int r = 0; r < world; ++r) {
    long acc = 0;
    for (int b = 0; b < B; ++b) {
      shard_range(nglob[b], r, world, lo[r][b], hi[r][b]);
      loff[r][b] = acc;
      acc += hi[r][b] - lo[r][b];
    }
  }
  send.clear(); recv.clear();
  send_counts.assign(world, 0);
  recv_counts.assign(world, 0);
  long scur = 0, rcur = 0;
  auto run = [&](int s, int t, int b, int h, long& r0, long& r1) {
    const long N = nglob[b];
    r0 = std::max((long)h * N + lo[s][b], lo[t][b] * H);
    r1 = std::min((long)h * N + hi[s][b], hi[t][b] * H);
    return r0 < r1;
  };
  for (int t = 0; t < world; ++t)          // me = source
    for (int b = 0; b < B; ++b)
      for (int h = 0; h < H; ++h) {
        long r0, r1;
        if (!run(me, t, b, h, r0, r1)) continue;
        const long cnt = hi[me][b] - lo[me][b];
        const long len = (r1 - r0) * dh;
        send.push_back(CopySeg{loff[me][b] * d + (h * cnt + (r0 - (long)h * nglob[b] - lo[me][b])) * dh, scur, len});
        scur += len;
        send_counts[t] += len;
      }
  for (int s = 0; s < world; ++s)          // me = destination
    for (int b = 0; b < B; ++b)
      for (int h = 0; h < H; ++h) {
        long r0, r1;
        if (!run(s, me, b, h, r0, r1)) continue;
        const long len = (r1 - r0) * dh;
        recv.push_back(CopySeg{rcur, loff[me][b] * d + (r0 - lo[me][b] * H) * dh, len});
        rcur += len;
        recv_counts[s] += len;
      }
}

static std::vector<int> seg_prefix(const std::vector<CopySeg>& segs, int unit) {
  std::vector<int> pre;
  int acc = 0;
  for (const auto& sg : segs) {
    pre.push_back(acc);
    acc += (int)(sg.len / unit);
  }
  pre.push_back(acc);
  return pre;
}

extern "C" int gnot_shard_range(int64_t n, int rank, int world, int64_t* lo, int64_t* hi) {
  if (world < 1 || rank < 0 || rank >= world || n < 0 || !lo || !hi) return fail(GNOT_E_INVALID, "bad shard range");
  long l, h;
  shard_range(n, rank, world, l, h);
  *lo = l;
  *hi = h;
  return GNOT_OK;
}

extern "C" int gnot_shard_exchange(int B, const int64_t* n_global, int n_head, int head_dim, int rank, int world,
                                   int64_t* send_counts, int64_t* recv_counts, int64_t* segs, int64_t cap,
                                   int64_t* nseg) {
  if (B <= 0 || !n_global || n_head <= 0 || head_dim <= 0 || world < 1 || rank < 0 || rank >= world || !nseg)
    return fail(GNOT_E_INVALID, "bad shard exchange arguments");
  std::vector<long> ng(n_global, n_global + B);
  std::vector<CopySeg> snd, rcv;
  std::vector<int64_t> sc, rc;
  build_exchange(B, ng, n_head, head_dim, rank, world, snd, rcv, sc, rc);
  if (send_counts) std::copy(sc.begin(), sc.end(), send_counts);
  if (recv_counts) std::copy(rc.begin(), rc.end(), recv_counts);
  *nseg = (int64_t)(snd.size() + rcv.size());
  int64_t k = 0;
  for (int dir = 0; dir < 2; ++dir)
    for (const auto& sg : dir == 0 ? snd : rcv) {
      if (segs && k < cap) {
        segs[4 * k] = dir;
        segs[4 * k + 1] = dir == 0 ? sg.a : sg.b;    // local offset (hm for send, tokens for recv)
        segs[4 * k + 2] = dir == 0 ? sg.b : sg.a;    // buffer offset
        segs[4 * k + 3] = sg.len;
      }
      ++k;
    }
  return GNOT_OK;
}

extern "C" int gnot_plan_set_shard(gnot_plan* p, int rank, int world, int B, const int64_t* n_global,
                                   const gnot_comm* comm) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  if (world <= 1 || !comm) {
    p->world = 1; p->rank = 0; p->nglob.clear(); p->comm = gnot_comm{};
    return GNOT_OK;
  }
  if (rank < 0 || rank >= world || B <= 0 || !n_global || !comm->allreduce_sum || !comm->alltoallv)
    return fail(GNOT_E_INVALID, "bad shard arguments");
  p->world = world;
  p->rank = rank;
  p->comm = *comm;
  p->nglob.assign(n_global, n_global + B);
  return GNOT_OK;
}

extern "C" int gnot_plan_set_grad_comm(gnot_plan* p, const gnot_comm* comm) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  if (comm && !comm->allreduce_sum) return fail(GNOT_E_INVALID, "gnot_comm.allreduce_sum is required");
  p->grad_comm_on = comm != nullptr;
  p->grad_comm = comm ? *comm : gnot_comm{};
  return GNOT_OK;
}

extern "C" int64_t gnot_plan_grad_floats(const gnot_plan* p) { return p ? (int64_t)p->arena_floats() : 0; }

extern "C" int gnot_plan_set_grad_arena(gnot_plan* p, float* arena, int64_t floats) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  if (arena) {
    if (floats < (int64_t)p->arena_floats())
      return fail(GNOT_E_INVALID, "gradient arena smaller than gnot_plan_grad_floats");
    if (reinterpret_cast<uintptr_t>(arena) & 15) return fail(GNOT_E_INVALID, "gradient arena must be 16-byte aligned");
  }
  if (p->user_grads != arena) {
    p->user_grads = arena;
    p->batch_set = false;          // the job tables hold the arena's pointers: set_batch + bind again
    p->ws_bound = false;
  }
  return GNOT_OK;
}

extern "C" int gnot_plan_set_precision(gnot_plan* p, int bf16) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  const int np = bf16 ? 1 : 3;
  if (p->np != np) {
    p->np = np;
    p->batch_set = false;          // image sizes change: set_batch + bind again
    p->ws_bound = false;
    p->packed = false;
  }
  return GNOT_OK;
}

extern "C" int gnot_plan_set_fourier(gnot_plan* p, int nx, int nf) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  if (nx < 0 || nx > 8 || nf < 0 || nf > 8)
    return fail(GNOT_E_INVALID, "Fourier orders must be in [0, 8] (0: no embedding)");
  const int Wx = nx > 0 ? 4 * nx + 3 : 1, Wf = nf > 0 ? 4 * nf + 3 : 1;
  if (p->in % Wx != 0)
    return fail(GNOT_E_INVALID, "input_dim must be the embedded width, a multiple of 4 x_fourier + 3 "
                                "(gnot_config carries the embedded widths)");
  if (p->F % Wf != 0)
    return fail(GNOT_E_INVALID, "input_func_dim must be the embedded width, a multiple of 4 fn_fourier + 3 "
                                "(gnot_config carries the embedded widths)");
  if (p->nx != nx || p->nf != nf) {
    p->nx = nx; p->nf = nf;
    p->in_raw = p->in / Wx; p->F_raw = p->F / Wf;
    p->batch_set = false;          // the staging of the inputs changes: set_batch + bind again
    p->ws_bound = false;
  }
  return GNOT_OK;
}

extern "C" int gnot_plan_set_pre_norm(gnot_plan* p, int on, float eps) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  if (!std::isfinite(eps) || !(eps > 0.f)) return fail(GNOT_E_INVALID, "pre-norm: eps must be finite and positive");
  if (p->pre_norm != (on != 0) || p->norm_eps != eps) {
    p->pre_norm = on != 0;
    p->norm_eps = eps;
    p->batch_set = false;          // the workspace layout changes: set_batch + bind again
    p->ws_bound = false;
  }
  return GNOT_OK;
}

// T = floor(p 2^32 + 0.5) and scale = fp32(2^32 / (2^32 - T)) of a drop probability (computed in double: the
// expectation is exact for the probability actually used); false for a p outside [0, 1) or not finite
static bool drop_threshold(float prob, uint32_t& T, float& scale) {
  if (!std::isfinite(prob) || !(prob >= 0.f) || !(prob < 1.f)) return false;
  const double t = std::floor((double)prob * 4294967296.0 + 0.5);   // <= 2^32 - 2^8: the largest float below 1
  T = (uint32_t)t;
  scale = (float)(4294967296.0 / (4294967296.0 - t));
  return true;
}

extern "C" int gnot_plan_set_dropout(gnot_plan* p, float prob, const uint32_t* key_dev) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  uint32_t T = 0;
  float scale = 1.f;
  if (!drop_threshold(prob, T, scale)) return fail(GNOT_E_INVALID, "dropout: p must be finite and in [0, 1)");
  if (T > 0 && !key_dev) return fail(GNOT_E_INVALID, "dropout: a device key {seed_lo, seed_hi, step, 0} is required");
  if (T > 0 && (reinterpret_cast<uintptr_t>(key_dev) & 3)) return fail(GNOT_E_INVALID, "dropout: the key must be 4-byte aligned");
  if (T == 0) key_dev = nullptr;
  if (p->drop_T != T || p->drop_key != key_dev) {
    p->drop_T = T;
    p->drop_scale = scale;
    p->drop_key = key_dev;
    p->drop_active = true;
    p->batch_set = false;          // the tables gain or lose the samples' first points: set_batch + bind again
    p->ws_bound = false;
  }
  return GNOT_OK;
}

extern "C" int gnot_plan_set_dropout_active(gnot_plan* p, int on) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  p->drop_active = on != 0;        // a launch-time switch: the next gnot_forward reads it, the batch stays
  return GNOT_OK;
}

extern "C" int gnot_plan_set_moe_recompute(gnot_plan* p, int on) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  if (p->moe_recompute != (on != 0)) {
    p->moe_recompute = on != 0;
    p->batch_set = false;          // the workspace layout changes: set_batch + bind again
    p->ws_bound = false;
  }
  return GNOT_OK;
}

extern "C" int gnot_plan_set_trainable(gnot_plan* p, const uint8_t* mask) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  std::vector<uint8_t> t;
  if (mask) {
    t.assign(mask, mask + p->n_lin());
    for (auto& b : t) b = b ? 1 : 0;
    if (std::find(t.begin(), t.end(), (uint8_t)0) == t.end()) t.clear();     // all trainable: the default
  }
  if (t != p->trainable) {
    p->trainable.swap(t);
    p->batch_set = false;          // the weight-gradient job lists change: set_batch + bind again
    p->ws_bound = false;
  }
  return GNOT_OK;
}

extern "C" int gnot_debug_backward_plan(const gnot_plan* p, int* wgrad_jobs, int* lowest_stage) {
  if (!p || !wgrad_jobs || !lowest_stage) return fail(GNOT_E_INVALID, "null argument");
  if (!p->batch_set) return fail(GNOT_E_STATE, "set_batch first");
  int jobs = 0;
  if (p->training) {
    for (const Chain& C : p->chains) jobs += (int)C.wg.jobs.size();
    for (const AttnCall& a : p->attn) jobs += (int)a.wg.jobs.size();
    jobs += (int)p->wg_fnkv.jobs.size();
  }
  *wgrad_jobs = jobs;
  *lowest_stage = p->lowest_stage();
  return GNOT_OK;
}

extern "C" int gnot_plan_set_input_grads(gnot_plan* p, int on) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  if (p->input_grads != (on != 0)) {
    p->input_grads = on != 0;
    p->batch_set = false;          // the workspace layout changes: set_batch + bind again
    p->ws_bound = false;
  }
  return GNOT_OK;
}

extern "C" int gnot_plan_set_batch(gnot_plan* p, int B, const int64_t* x_off, const int64_t* fn_off,
                                   int training) {
  if (!p || B <= 0 || !x_off) return fail(GNOT_E_INVALID, "bad batch arguments");
  if (p->I > 0 && !fn_off) return fail(GNOT_E_INVALID, "fn_off required when n_input_functions > 0");
  p->B = B;
  p->xoff.assign(x_off, x_off + B + 1);
  if (p->xoff[0] != 0) return fail(GNOT_E_INVALID, "x_off[0] must be 0");
  for (int b = 0; b < B; ++b)
    if (p->xoff[b + 1] < p->xoff[b]) return fail(GNOT_E_INVALID, "x_off must be non-decreasing");
  p->P = p->xoff[B];
  p->fnoff.assign(p->I, {});
  p->Q.assign(p->I, 0);
  for (int i = 0; i < p->I; ++i) {
    p->fnoff[i].assign(fn_off + i * (B + 1), fn_off + (i + 1) * (B + 1));
    if (p->fnoff[i][0] != 0) return fail(GNOT_E_INVALID, "fn_off[i][0] must be 0");
    for (int b = 0; b < B; ++b)
      if (p->fnoff[i][b + 1] < p->fnoff[i][b]) return fail(GNOT_E_INVALID, "fn_off must be non-decreasing");
    p->Q[i] = p->fnoff[i][B];
  }
  if (p->P <= 0) return fail(GNOT_E_INVALID, "empty batch (no query points)");
  // point / chunk indices are 32-bit in the kernels' job tables (the buffer resources of the streaming
  // kernels are based per workgroup or per split, so no activation array size bounds a plan)
  if (p->P >= (1L << 31) / 4) return fail(GNOT_E_INVALID, "batch too large for 32-bit segment indices");
  for (int i = 0; i < p->I; ++i)
    if (p->Q[i] >= (1L << 31) / 4) return fail(GNOT_E_INVALID, "input functions too large for 32-bit segment indices");
  p->training = training != 0;
  p->sharded = p->world > 1;
  if (p->sharded) {
    if ((int)p->nglob.size() != B) return fail(GNOT_E_INVALID, "gnot_plan_set_shard was declared for another B");
    for (int b = 0; b < B; ++b) {
      long lo, hi;
      shard_range(p->nglob[b], p->rank, p->world, lo, hi);
      if (p->xoff[b + 1] - p->xoff[b] != hi - lo)
        return fail(GNOT_E_INVALID, "x_off does not match this rank's shard of n_global (gnot_shard_range)");
    }
    build_exchange(B, p->nglob, p->H, p->dhr, p->rank, p->world, p->xsend, p->xrecv, p->xsend_counts,
                   p->xrecv_counts);
    // the runs are multiples of the real head width (offsets too): float4 copies unless it is not a multiple of 4
    p->xunit = p->dhr % 4 == 0 ? 4 : 1;
    p->xsend_prefix = seg_prefix(p->xsend, p->xunit);
    p->xrecv_prefix = seg_prefix(p->xrecv, p->xunit);
  } else {
    p->xsend.clear(); p->xrecv.clear(); p->xsend_prefix.clear(); p->xrecv_prefix.clear();
  }

  // ---------------- workspace carve
  build_chains(p);
  build_attn_calls(p);
  plan_images(p);
  p->bufs.clear();
  p->buf_order.clear();
  Carver C{0, p};
  const long P = p->P, D = p->D, E = p->E, NL = p->NL, H = p->H;
  const long per_state = p->per_state(), Qmax = p->Qmax();
  const int I = p->I, KI = p->KI;
  // a call's forward buffers, from its description: the names and pitches the launches use are the ones carved
  auto carve_call = [&](const AttnCall& a) {
    C.add(a.proj, P * a.pitch, a.pitch);
    for (const AttnSrc& r : a.src)
      if (r.fn >= 0) C.add(r.ckv, p->Q[r.fn] * 2 * D, 2 * D);
    for (const AttnSrc& r : a.src) C.add(r.state, p->B * per_state, per_state);
    C.add(a.res, P * D, p->Dr);        // scramble rows: Dr floats per token (attn_forward)
    C.add(a.out, P * D, D);
  };
  C.add("packed", p->packed4 * 4, 0);
  C.add("pbias", p->pbias, 0);
  // gradient arena
  p->grad_off.clear();
  long g = 0;
  for (int li = 0; li < p->n_lin(); ++li) {
    p->grad_off.push_back(g);
    g += (long)p->lin_o[li] * p->lin_i[li];
    p->grad_off.push_back(g);
    g += p->lin_o[li];
  }
  p->grad_floats = g;
  C.add("grads", g, 0);
  const bool tr = p->training;
  C.add("x", P * r4(p->in), r4(p->in));
  C.add("theta", (long)p->B * p->th, p->th);
  C.add("xin", P * r4(p->in + p->th), r4(p->in + p->th));
  for (int i = 0; i < I; ++i) C.add("fn" + std::to_string(i), p->Q[i] * r4(p->F), r4(p->F));
  const long ldsc = r4(E);
  C.add("scores", P * ldsc, ldsc);
  if (tr) {
    C.add("dscore", P * ldsc, ldsc);
    C.add("gate_save", NL * P * D, D);
    C.add("x_save", NL * P * D, D);
    C.add("out_save", NL * P * D, D);
  }
  C.add("query0", P * D, D);
  for (int i = 0; i < I; ++i) {
    if (tr) C.add("fn_save" + std::to_string(i), NL * p->Q[i] * D, D);
    C.add("fnenc" + std::to_string(i), p->Q[i] * D, D);
  }
  for (int l = 0; l < p->L; ++l) {
    const std::string s = "b" + std::to_string(l) + ".";
    carve_call(p->call(l, true));
    if (tr && !p->moe_recompute) C.add(s + "m1save", E * NL * P * D, D);
    C.add(s + "query1", P * D, D);
    carve_call(p->call(l, false));
    if (tr && !p->moe_recompute) C.add(s + "m2save", E * NL * P * D, D);
    C.add(s + "query2", P * D, D);
  }
  C.add("stage", E * P * D, D);
  if (D > 256) {                             // chainw.hip scratch: query-branch chains / input-function branch
    C.add("lw_scr", 2 * P * D, D);
    if (I > 0) C.add("lw_scr2", 2 * Qmax * D, D);
  }
  if (tr && p->moe_recompute && p->L > 0) C.add("mrsave", E * NL * P * D, D);
  if (p->sharded) {                          // scramble exchange scratch: head-major rows / packed peers
    C.add("xa", P * D, p->Dr);
    C.add("xb", P * D, p->Dr);
  }
  if (p->pre_norm && p->L > 0) {
    // the normalised attention inputs, kept per block (the q / k / v weight gradients read their Linear's
    // input) and once per input function (no parameters: the same rows for every block); training keeps
    // each row's rstd for the backward
    for (const AttnCall& a : p->attn) {
      C.add(a.in, P * D, D);
      if (tr) C.add(a.rstd, P, 1);
    }
    for (int i = 0; i < I; ++i) {
      C.add("fnn" + std::to_string(i), p->Q[i] * D, D);
      if (tr) C.add("fnr" + std::to_string(i), p->Q[i], 1);
    }
    if (tr) C.add("dnorm", P * D, D);          // d(normalised rows) of one attention call, origin stream only
  }
  // attention segments
  make_chunks(p->xoff, p->qchunks, p->qchunk_off);
  p->fchunks.assign(I, {});
  p->fchunk_off.assign(I, {});
  for (int i = 0; i < I; ++i) make_chunks(p->fnoff[i], p->fchunks[i], p->fchunk_off[i]);
  choose_attn_forms(p);
  if (tr) {
    C.add("dout", P * r4(p->out), r4(p->out));
    C.add("dquery", P * D, D);
    C.add("dsum0", P * D, D);
    C.add("dsum1", P * D, D);
    C.add("dres", P * D, p->Dr);
    C.add("dqkv0", P * 3 * D, 3 * D);
    C.add("dqkv1", P * 3 * D, 3 * D);
    for (int i = 0; i < KI; ++i) {
      C.add("du" + std::to_string(i), P * D, D);
      C.add("dden" + std::to_string(i), P * H, H);
    }
    C.add("dstate0", p->B * per_state, per_state);
    for (const AttnCall& a : p->attn)                  // kept per (block, source) for the batched K/V backward
      for (const AttnSrc& r : a.src)
        if (r.fn >= 0) {
          C.add(r.dstate, p->B * per_state, per_state);
          C.add(r.dkv, p->Q[r.fn] * 2 * D, 2 * D);
        }
    for (int i = 0; i < I; ++i) {
      C.add("dfn" + std::to_string(i), p->Q[i] * D, D);
    }
    if (p->input_grads) {
      C.add("dtheta_ws", (long)p->B * std::max(p->th, 1), std::max(p->th, 1));   // d theta before the copy out
      C.add("dxin", P * r4(p->in + p->th), r4(p->in + p->th));
      C.add("dxg", P * r4(p->in), r4(p->in));
      for (int i = 0; i < I; ++i) C.add("dfnin" + std::to_string(i), p->Q[i] * r4(p->F), r4(p->F));
    }
    C.add("dz0", E * NL * std::max(P, Qmax) * D, D);
    C.add("dz1", E * NL * P * D, D);
    if (I > 0) C.add("dzf", NL * Qmax * D, D);
  }

  // ---------------- device tables: sized now (every buffer still unbound), filled and uploaded at bind; the
  // same walk builds the point-reduction GEMM groups, whose split-K slabs are carved here
  TableWalk sizing;
  walk_tables(p, sizing);
  p->table_bytes = sizing.cur;
  C.add("slab_wgrad", p->slab_wgrad_floats, 0);
  if (I > 0 && tr) C.add("slab_wgrad2", p->slab_wgrad_floats, 0);   // weight grads on side2
  C.add("slab_state", p->slab_state_floats, 0);
  const size_t table_off = C.raw(p->table_bytes);
  p->bufs["__tables"] = Buf{table_off, 0, nullptr};
  p->ws_need = C.top;
  p->batch_set = true;
  p->ws_bound = false;
  p->packed = false;
  p->fwd_done = false;
  return GNOT_OK;
}

extern "C" size_t gnot_plan_workspace_bytes(const gnot_plan* p) { return (p && p->batch_set) ? p->ws_need : 0; }

extern "C" int gnot_plan_grad_offsets(const gnot_plan* p, int64_t* grad_off) {
  if (!p || !grad_off || !p->batch_set) return fail(GNOT_E_STATE, "set_batch first");
  for (size_t i = 0; i < p->grad_off.size(); ++i) grad_off[i] = p->grad_off[i];
  return GNOT_OK;
}

// ====================================================================== bind
extern "C" int gnot_plan_bind_workspace_async(gnot_plan* p, void* workspace, size_t bytes, void* stream);
extern "C" int gnot_plan_bind_workspace(gnot_plan* p, void* workspace, size_t bytes) {
  const int rc = gnot_plan_bind_workspace_async(p, workspace, bytes, nullptr);
  if (rc != GNOT_OK) return rc;
  GNOT_CK(hipStreamSynchronize(nullptr));
  return GNOT_OK;
}

// Stream-ordered bind: the table image goes through a pinned staging slot and one hipMemcpyAsync on
// `stream`, so a new batch geometry costs no host synchronisation (the copy is ordered after the
// previous step's kernels on that stream, which have joined every side stream by then).
extern "C" int gnot_plan_bind_workspace_async(gnot_plan* p, void* workspace, size_t bytes, void* stream) {
  if (!p || !p->batch_set) return fail(GNOT_E_STATE, "set_batch first");
  if (!p->params_bound) return fail(GNOT_E_STATE, "bind_params first");
  if (!workspace || bytes < p->ws_need) return fail(GNOT_E_WORKSPACE, "workspace missing or too small");
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(GNOT_E_WORKSPACE, "workspace must be 256-byte aligned");
  p->ws = static_cast<char*>(workspace);
  for (auto& kv : p->bufs) kv.second.p = reinterpret_cast<float*>(p->ws + kv.second.off);

  // ---- tables in the workspace tail: the walk set_batch sized, now with every buffer bound
  char* tp = p->ws + p->bufs["__tables"].off;
  std::vector<char> host(p->table_bytes, 0);
  TableWalk fill{host.data(), tp, host.size(), 0};
  const size_t slab_need = p->slab_wgrad_floats, slab_state_need = p->slab_state_floats;
  walk_tables(p, fill);
  if (p->slab_wgrad_floats != slab_need || p->slab_state_floats != slab_state_need)
    return fail(GNOT_E_INVALID, "internal: slab size changed at bind");
  if (fill.cur != p->table_bytes) return fail(GNOT_E_INVALID, "internal: table overflow (the walk changed at bind)");
  const size_t cur = fill.cur;
  {
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int k = p->stage_next;
    p->stage_next = (k + 1) % gnot_plan::kStageSlots;
    if (!p->stage_ev[k]) GNOT_CK(hipEventCreateWithFlags(&p->stage_ev[k], hipEventDisableTiming));
    if (p->stage_used[k]) GNOT_CK(hipEventSynchronize(p->stage_ev[k]));   // only when the ring wraps in flight
    if (p->stage_cap[k] < cur) {
      if (p->stage[k]) GNOT_CK(hipHostFree(p->stage[k]));
      p->stage[k] = nullptr;
      p->stage_cap[k] = 0;
      const size_t cap = cur + cur / 2 + 4096;                           // headroom: growth is rare
      GNOT_CK(hipHostMalloc(&p->stage[k], cap, hipHostMallocDefault));
      p->stage_cap[k] = cap;
    }
    std::memcpy(p->stage[k], host.data(), cur);
    GNOT_CK(hipMemcpyAsync(tp, p->stage[k], cur, hipMemcpyHostToDevice, s));
    GNOT_CK(hipEventRecord(p->stage_ev[k], s));
    p->stage_used[k] = true;
  }
  // a padded width: the pad columns of rows that kernels write per head only (the attention backward's
  // dq / dk / dv, du) are read as exact zeros by the next backward-data products: clear the activation
  // part of the workspace once per bind (the tables follow it, uploaded after this on the same stream)
  // The ranges of frozen Linears in a workspace arena are left out: nothing writes them (gnot_plan_set_trainable)
  if (p->padded()) {
    const hipStream_t s = static_cast<hipStream_t>(stream);
    size_t from = 0;
    if (!p->user_grads && p->training)
      for (int li = 0; li < p->n_lin(); ++li) {
        if (!p->frozen(li)) continue;
        const size_t lo = p->bufs["grads"].off + (size_t)p->grad_off[2 * li] * 4;
        const size_t hi = p->bufs["grads"].off + ((size_t)p->grad_off[2 * li + 1] + p->lin_o[li]) * 4;
        if (lo > from) GNOT_CK(hipMemsetAsync(p->ws + from, 0, lo - from, s));
        from = hi;
      }
    GNOT_CK(hipMemsetAsync(p->ws + from, 0, p->bufs["__tables"].off - from, s));
  }
  if (!p->side2) GNOT_CK(hipStreamCreateWithFlags(&p->side2, hipStreamNonBlocking));
  if (!p->side) {
    // same priority as the caller's stream: measured on MI355X, a low- (or high-) priority side
    // stream serialises against the main one and the step takes ~1.9x longer (round 1)
    GNOT_CK(hipStreamCreateWithPriority(&p->side, hipStreamNonBlocking, 0));
  }
  while (p->evs.size() < 256) {
    hipEvent_t e;
    GNOT_CK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    p->evs.push_back(e);
  }
  p->ws_bound = true;
  p->packed = false;
  p->fwd_done = false;
  p->bwd_done = false;
  return GNOT_OK;
}

extern "C" int gnot_pack_weights(gnot_plan* p, void* stream) {
  if (!p || !p->ws_bound) return fail(GNOT_E_STATE, "bind_workspace first");
  GNOT_CK(launch_pack(p->d_pack_jobs, p->d_pack_prefix, (int)p->pack_jobs.size(), p->pack_tiles,
                      static_cast<hipStream_t>(stream)));
  p->packed = true;
  return GNOT_OK;
}

// ====================================================================== forward / backward
namespace {

struct Ctx {
  gnot_plan* p;
  hipStream_t s;
};

// records a start/stop event pair around one launch when `kind` is the profiled kernel class
struct ProfScope {
  Ctx& c;
  bool on = false;
  size_t idx = 0;
  hipStream_t st;
  ProfScope(Ctx& c_, const char* kind, double flops, hipStream_t stream = nullptr) : c(c_), st(stream ? stream : c_.s) {
    gnot_plan* p = c.p;
    if (p->prof_kind.empty() || p->prof_kind != kind) return;
    while (p->prof_events.size() < p->prof_used + 2) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return;
      p->prof_events.push_back(e);
    }
    idx = p->prof_used;
    p->prof_used += 2;
    p->prof_flops += flops;
    p->prof_launches += 1;
    on = hipEventRecord(p->prof_events[idx], st) == hipSuccess;
  }
  ~ProfScope() {
    if (on) (void)hipEventRecord(c.p->prof_events[idx + 1], st);
  }
};

// ncol > 0: store only output columns [0, ncol) (a row pitch below NO: the attention's head-major
// scramble rows of the real width, attn_backward)
int run_linear(Ctx& c, const float* X, long ldx, int K, const Img& A, const float* bias, float* Y, long ldy,
               int NO, long P, int epi, int nsoft, int ncol = 0) {
  LinearArgs a{};
  a.nseg = 1; a.X[0] = X; a.Wp[0] = A.p; a.ldx = ldx; a.nsum = 1; a.sum_stride = 0; a.K = K;
  a.bias = bias; a.Y = Y; a.ldy = ldy; a.NO = NO; a.P = (int)P;
  a.epi = epi; a.nsoft = nsoft; a.dh = c.p->dh; a.np = c.p->npk(); a.img = c.p->lin_img();
  a.dreal = nsoft > 0 ? c.p->attn_dreal() : 0;
  a.dhr = (nsoft > 0 && c.p->head_padded()) ? c.p->dhr : 0;
  a.ncol = ncol;
  GNOT_CK(c.p->D == 256 ? launch_linear2(a, c.s) : launch_linear(a, c.p->D, c.s));
  return GNOT_OK;
}

// Y (+)= sum_s X_s A_s over K-segments that share one row pitch (backward-data of several Linears)
int run_linear_seg(Ctx& c, std::initializer_list<std::pair<const float*, const Img*>> segs, long ldx, float* Y,
                   long ldy, long P, int epi) {
  LinearArgs a{};
  a.nseg = 0;
  for (const auto& sg : segs) {
    a.X[a.nseg] = sg.first;
    a.Wp[a.nseg] = sg.second->p;
    ++a.nseg;
  }
  a.ldx = ldx; a.nsum = 1; a.K = c.p->D; a.bias = nullptr; a.Y = Y; a.ldy = ldy; a.NO = c.p->D; a.P = (int)P;
  a.epi = epi; a.nsoft = 0; a.dh = c.p->dh; a.np = c.p->npk(); a.img = c.p->lin_img();
  GNOT_CK(c.p->D == 256 ? launch_linear2(a, c.s) : launch_linear(a, c.p->D, c.s));
  return GNOT_OK;
}

// d > 256: the chainw.hip scratch of the stream a chain call runs on (the input-function branch on side2
// runs concurrently with the query branch)
ChainArgs& cw_scratch(gnot_plan* p, ChainArgs& a, hipStream_t s) {
  if (p->D > 256) a.scratch = p->P_(s == p->side2 ? "lw_scr2" : "lw_scr");
  return a;
}

// What a launch of chain call C takes from its description: shape, layer tables, mode, the forward's input
// (X) or the backward's d scores, the gating scores a soft-MoE (and the gating's backward) reads, and the save
// buffer with its layout.  `save` null: a forward that keeps no pre-activations.  The forward adds Y, the
// backward dY / dX (and chain_bwd_launch the dZ slot)
ChainArgs chain_args(gnot_plan* p, const Chain& C, bool bwd, float* save) {
  const long D = p->D, NL = p->NL;
  ChainArgs a{};
  a.D = p->D; a.KT0 = C.KT0; a.OTL = C.OTL; a.nlin = p->NL;
  a.layers_host = C.layers.data();
  a.in_dim = C.in_dim; a.out_dim = C.out_dim; a.P = (int)C.rows; a.nchains = (int)C.firsts.size();
  a.layers = C.d_layers;
  a.np = p->npk();
  a.mode = C.mode;
  if (!bwd) {
    const Buf& x = p->bufs.at(C.x);
    a.X = x.p; a.ldx = x.ld;
  }
  if (C.mode == CH_MOE || (bwd && C.mode == CH_SOFTMAX)) {
    a.scores = p->P_("scores"); a.ldsc = (int)p->bufs.at("scores").ld;
    if (bwd) a.dscore = p->P_("dscore");
  }
  a.save = save;
  if (C.mode == CH_MOE) {
    // a soft-MoE call's saves (and dZ): fp32 [NL][P][D] per expert, or in bf16 mode 2 NL bf16 layers per
    // expert (ChainArgs::b16s: bf16 expert terms with or without saves) and bf16 stage rows
    a.b16s = a.stage_b16 = p->b16s() ? 1 : 0;
    a.save_layer_stride = a.b16s ? C.rows * D / 2 : C.rows * D;
    a.save_chain_stride = NL * C.rows * D;
  } else if (save) {
    a.save_layer_stride = C.rows * D;
    a.save_chain_stride = NL * C.rows * D;
  }
  return a;
}

double group_flops(const WgradGroup& G) {
  double fl = 0.0;
  for (const auto& J : G.jobs) fl += 2.0 * J.P * (double)J.out * J.in;
  return fl;
}

// attention-state reductions: on the main stream (they are on the critical path)
int run_state(Ctx& c, const WgradGroup& G) {
  if (G.jobs.empty()) return GNOT_OK;
  ProfScope ps(c, "state", group_flops(G));
  GNOT_CK(launch_state(G.tables(), c.p->P_("slab_state"), G.jobs[0].out, G.jobs[0].state_dh, G.state_pts,
                       G.state_nw, G.state_mfma, c.s));
  return GNOT_OK;
}

hipEvent_t next_event(gnot_plan* p) {
  hipEvent_t e = p->evs[p->ev_next];
  p->ev_next = (p->ev_next + 1) % p->evs.size();
  return e;
}

// before the main stream overwrites `buf`, wait for the side-stream group that last read it
int flush_deferred(Ctx& c);
int guard_write(Ctx& c, const float* buf) {
  // a deferred group reads buf: launch it (and register) first.  flush_deferred empties the vector, so
  // decide before calling it
  const auto& dq = c.p->deferred;
  if (std::any_of(dq.begin(), dq.end(), [buf](const gnot_plan::DeferredWgrad& d) {
        return std::find(d.reads.begin(), d.reads.end(), buf) != d.reads.end();
      })) {
    const int rc = flush_deferred(c);
    if (rc != GNOT_OK) return rc;
  }
  auto it = c.p->readers.find(buf);
  if (it != c.p->readers.end()) {
    GNOT_CK(hipStreamWaitEvent(c.s, it->second, 0));
    c.p->readers.erase(it);
  }
  return GNOT_OK;
}

#define GNOT_RUN(expr)              \
  do {                              \
    const int rc_ = (expr);         \
    if (rc_ != GNOT_OK) return rc_; \
  } while (0)

// one weight-gradient group's launches (point-reduction GEMM + split-K reduce)
int launch_group(gnot_plan* p, const WgradGroup& G, float* slab, hipStream_t s) {
  GNOT_CK(launch_wgrad(G.kind, G.tables(), slab, p->npk(), G.scaled, p->bwd_accumulate, s));
  return GNOT_OK;
}
// its profiling class: the bf16-row MoE weight gradients are HBM-bound, the others are not
const char* wgrad_class(const WgradGroup& G) { return G.kind == WgradKernel::B16Rows ? "wgrad_b16" : "wgrad"; }

// the group's gradient ranges summed over the ranks (gnot_plan_set_grad_comm) on the comm stream, once
// the event `done` (the group's kernels) has passed: consecutive canonical Linears are adjacent in the
// arena ((dW, db) per Linear), so a group is a few contiguous ranges, one collective each
int grad_allreduce(gnot_plan* p, const WgradGroup& G, hipEvent_t done) {
  GNOT_CK(hipStreamWaitEvent(p->comm_stream, done, 0));
  std::vector<int> ls(G.lins);
  std::sort(ls.begin(), ls.end());
  float* grads = p->grads();
  for (size_t k = 0; k < ls.size();) {
    size_t m = k + 1;
    while (m < ls.size() && ls[m] == ls[m - 1] + 1) ++m;
    const long lo = p->grad_off[2 * ls[k]];
    const long hi = p->grad_off[2 * ls[m - 1] + 1] + p->lin_o[ls[m - 1]];
    if (p->grad_comm.allreduce_sum(p->grad_comm.user, grads + lo, hi - lo, p->comm_stream) != 0)
      return fail(GNOT_E_HIP, "gnot_comm.allreduce_sum (gradients) failed");
    k = m;
  }
  return GNOT_OK;
}

// one weight-gradient group in order on c's stream with split-K slab `slab`, then its gradient all-reduce
int run_wgrad_here(Ctx& c, const WgradGroup& G, float* slab) {
  if (G.jobs.empty()) return GNOT_OK;
  {
    ProfScope ps(c, wgrad_class(G), group_flops(G));
    GNOT_RUN(launch_group(c.p, G, slab, c.s));
  }
  if (c.p->grad_comm_live) {
    hipEvent_t done = next_event(c.p);
    GNOT_CK(hipEventRecord(done, c.s));
    GNOT_RUN(grad_allreduce(c.p, G, done));
  }
  return GNOT_OK;
}

// weight gradients: on the caller's stream (plans of >= 65,536 points), or forked onto the side stream;
// `reads` are the main-stream buffers the group consumes, guarded until it finishes
int run_wgrad_side(Ctx& c, const WgradGroup& G, std::initializer_list<const float*> reads) {
  if (G.jobs.empty()) return GNOT_OK;
  gnot_plan* p = c.p;
  const bool serial = p->serial_wgrad();
  // Only the caller's (capture-origin) stream forks to the side stream.  A fork from the forked
  // input-function stream side2 segfaults the HIP runtime in hipStreamEndCapture (ROCm 7.2, torch
  // 2.10), while eager execution of the same sequence is correct.  Four topologies, each run once:
  //   r1   side2 -> side (side already forked from the origin), side joined into the origin only
  //   r2a  the same, side's event also joined back into side2 before side2 joins the origin
  //   r2b  side2 -> side3 (a stream used by nothing else), side3 joined into side2
  //   r2c  r2b + side3 also joined into the origin
  // all crash at the first capture; only first-level forks from the origin capture.  side2's weight
  // gradients therefore run in order on side2 with their own slab: they are the input-function
  // encoders' and the cross K/V Linears' (M ~ 10^3 points: tens of microseconds).  DESIGN.md
  // "capture fault".
  if (serial || c.s == p->side2) return run_wgrad_here(c, G, p->P_(c.s == p->side2 ? "slab_wgrad2" : "slab_wgrad"));
  // forked: the side stream waits for what the caller's stream has issued so far (the fork event is
  // recorded now), but its launches are captured only after the caller's NEXT kernel (flush_deferred).  A
  // captured graph keeps a node's first-captured child on the node's own hardware queue; with the side
  // launch captured first, the main chain hopped to another queue at every fork, ~10 us of cross-queue
  // wait each (configs[1] trace, profiles/r05m_*: 8 MoE calls x 2 forks per step)
  hipEvent_t fork = next_event(p);
  GNOT_CK(hipEventRecord(fork, c.s));
  p->deferred.push_back({&G, std::vector<const float*>(reads), fork});
  return GNOT_OK;
}

// the deferred side-stream weight-gradient groups, in order; `c` is the capture-origin stream's context
int flush_deferred(Ctx& c) {
  gnot_plan* p = c.p;
  std::vector<gnot_plan::DeferredWgrad> pend;
  pend.swap(p->deferred);
  for (const auto& d : pend) {
    GNOT_CK(hipStreamWaitEvent(p->side, d.fork, 0));
    {
      ProfScope ps(c, wgrad_class(*d.G), group_flops(*d.G), p->side);
      GNOT_RUN(launch_group(p, *d.G, p->P_("slab_wgrad"), p->side));
    }
    hipEvent_t done = next_event(p);
    GNOT_CK(hipEventRecord(done, p->side));
    for (const float* r : d.reads) p->readers[r] = done;
    if (p->grad_comm_live) GNOT_RUN(grad_allreduce(p, *d.G, done));
  }
  return GNOT_OK;
}

// sum a state buffer over the ranks of a sharded batch
int shard_allreduce(Ctx& c, float* buf, long count) {
  gnot_plan* p = c.p;
  if (!p->sharded || count <= 0) return GNOT_OK;
  if (p->comm.allreduce_sum(p->comm.user, buf, count, c.s) != 0)
    return fail(GNOT_E_HIP, "gnot_comm.allreduce_sum failed");
  return GNOT_OK;
}

// forward scramble: local head-major apply output `hm` -> this rank's output tokens `tok`
// backward (reverse): token-order gradient `tok` -> local head-major `hm`
int shard_exchange(Ctx& c, float* hm, float* tok, bool reverse) {
  gnot_plan* p = c.p;
  float* xa = p->P_("xa");
  float* xb = p->P_("xb");
  const int ns = (int)p->xsend.size(), nr = (int)p->xrecv.size();
  if (!reverse) {
    GNOT_CK(launch_segcopy(p->d_xsend, p->d_xsend_prefix, ns, p->xsend_prefix.back(), hm, xa, false, c.s, p->xunit));
    if (p->comm.alltoallv(p->comm.user, xa, p->xsend_counts.data(), xb, p->xrecv_counts.data(), c.s) != 0)
      return fail(GNOT_E_HIP, "gnot_comm.alltoallv failed");
    GNOT_CK(launch_segcopy(p->d_xrecv, p->d_xrecv_prefix, nr, p->xrecv_prefix.back(), xb, tok, false, c.s, p->xunit));
  } else {
    GNOT_CK(launch_segcopy(p->d_xrecv, p->d_xrecv_prefix, nr, p->xrecv_prefix.back(), tok, xb, true, c.s, p->xunit));
    if (p->comm.alltoallv(p->comm.user, xb, p->xrecv_counts.data(), xa, p->xsend_counts.data(), c.s) != 0)
      return fail(GNOT_E_HIP, "gnot_comm.alltoallv failed");
    GNOT_CK(launch_segcopy(p->d_xsend, p->d_xsend_prefix, ns, p->xsend_prefix.back(), xa, hm, true, c.s, p->xunit));
  }
  return GNOT_OK;
}

// what every attention apply pass over the query points takes: their segments and the head geometry
AttnApplyArgs apply_args(const gnot_plan* p) {
  AttnApplyArgs ap{};
  ap.chunks = p->d_qchunks; ap.nchunks = (int)p->qchunks.size(); ap.off = p->d_xoff;
  ap.H = p->H; ap.dh = p->dh; ap.dhr = p->head_padded() ? p->dhr : 0;
  return ap;
}

// keyed dropout of one attention call's output rows (forward) or of their gradient (backward), in place on
// this stream, keyed on the call's site.  Only when the last forward dropped (gnot_plan_set_dropout +
// gnot_plan_set_dropout_active)
int drop_rows(Ctx& c, float* rows, const AttnCall& a) {
  gnot_plan* p = c.p;
  if (!p->drop_fwd) return GNOT_OK;
  GNOT_CK(launch_dropout_rows(rows, p->D, p->P, p->Dr, p->d_xoff, p->d_glo, p->B, p->drop_key, a.site, p->drop_T,
                              p->drop_scale, c.s));
  return GNOT_OK;
}

// the q, S | z (and, in the backward, du, dden) operands of call a's apply passes
AttnApplyArgs call_apply_args(const gnot_plan* p, const AttnCall& a, bool bwd) {
  AttnApplyArgs ap = apply_args(p);
  ap.q = p->P_(a.proj); ap.ldq = a.pitch; ap.nsrc = a.nsrc;
  for (int i = 0; i < a.nsrc; ++i) {
    ap.state[i] = p->P_(a.src[i].state);
    if (bwd) { ap.du[i] = p->P_(a.src[i].du); ap.dden[i] = p->P_(a.src[i].dden); }
  }
  return ap;
}

// one LinearAttention call (model.py:53-107): a.in [P, D] -> a.out, the scramble rows kept in a.res
int attn_forward(Ctx& c, const AttnCall& a) {
  gnot_plan* p = c.p;
  const long P = p->P;
  const int D = p->D;
  const float* q_in = p->P_(a.in);
  float* res_out = p->P_(a.res);
  float* out = p->P_(a.out);
  float* pbias = p->P_("pbias");
  AttnApplyArgs ap = call_apply_args(p, a, false);
  ap.res = p->sharded ? p->P_("xb") : res_out;
  // q, or q | k | v (feature softmax over q and k); an unfused call's keys / values / states were computed for
  // every block up front
  GNOT_RUN(run_linear(c, q_in, D, D, a.proj_img, pbias + a.bproj, p->P_(a.proj), a.pitch, (int)a.pitch, P, EPI_STORE,
                      a.fused ? 2 * D : D));
  if (a.fused) {
    GNOT_RUN(run_state(c, a.src[0].st));
    GNOT_RUN(shard_allreduce(c, p->P_(a.src[0].state), p->B * p->per_state()));   // S, z over all ranks
  }
  GNOT_CK(launch_attn_apply(a.apply_fwd, ap, false, c.s));
  if (p->sharded) GNOT_RUN(shard_exchange(c, p->P_("xb"), res_out, false));   // the scramble, across ranks
  // fc_out over the scramble rows: Dr columns per token (the head-major apply output viewed as rows of
  // H * dh = Dr floats, model.py:81-83), read zero-filled to the padded width
  GNOT_RUN(run_linear(c, res_out, p->Dr, p->Dr, a.o_img, pbias + a.bo, out, D, D, P, EPI_STORE, 0));
  GNOT_RUN(drop_rows(c, out, a));            // everything downstream reads the dropped rows
  return GNOT_OK;
}

// backward of one LinearAttention call; its output gradient is materialised in a.dsum.
// Accumulates d(query input) into dquery and forks the weight gradients of its Linears.
int attn_backward(Ctx& c, const AttnCall& a) {
  gnot_plan* p = c.p;
  const long P = p->P;
  const int D = p->D;
  float* dsum = p->P_(a.dsum);
  float* dres = p->P_("dres");
  float* dquery = p->P_("dquery");
  float* dqkv = p->P_(a.dqkv);
  // pre-norm: the projections' backward-data is the gradient of the NORMALISED rows: stored into "dnorm"
  // (written and read on this stream only; no forked weight gradient reads it), then pulled through the norm
  // and added onto dquery
  float* dq_dst = p->pre_norm ? p->P_("dnorm") : dquery;
  const int dq_epi = p->pre_norm ? EPI_STORE : EPI_ACCUM;
  GNOT_RUN(guard_write(c, dqkv));
  // dropout: the forward's mask again, regenerated from the key, before fc_out's backward-data and its weight
  // gradients (a forked group reads the masked rows)
  GNOT_RUN(drop_rows(c, dsum, a));
  // fc_out backward-data: dres = dout W_o (token order); sharded: back to this rank's head-major rows
  GNOT_RUN(run_linear(c, dsum, D, D, p->T_img[a.o], nullptr, dres, p->Dr, D, P, EPI_STORE, 0, p->Dr));
  if (p->sharded) {
    GNOT_RUN(shard_exchange(c, p->P_("xb"), dres, true));
    dres = p->P_("xb");
  }
  AttnApplyArgs ap = call_apply_args(p, a, true);
  ap.dres = dres; ap.dq_pre = dqkv; ap.lddu = D; ap.lddq = a.pitch;
  GNOT_CK(launch_attn_apply(a.apply_bwd, ap, true, c.s));
  // dS, dz per source (an input-function source keeps its own per block: the dK/dV side of every block runs
  // batched later)
  for (const AttnSrc& r : a.src) GNOT_RUN(run_state(c, r.dst));
  if (a.fused) {
    // the call's own K/V backward and the backward-data of q, k and v in one three-segment product
    const float* qkv = ap.q;
    float* dst = p->P_(a.src[0].dstate);
    GNOT_RUN(shard_allreduce(c, dst, p->B * p->per_state()));   // dS, dz over all ranks
    AttnKVBwdArgs kb{};
    kb.k = qkv + D; kb.v = qkv + 2 * D; kb.ldkv = 3 * D; kb.dstate = dst; kb.chunks = ap.chunks;
    kb.nchunks = ap.nchunks; kb.H = p->H; kb.dh = p->dh; kb.dk = dqkv + D; kb.dv = dqkv + 2 * D; kb.lddkv = 3 * D;
    GNOT_CK(launch_attn_kv_bwd(p->kv_bwd, &kb, nullptr, 1, kb.nchunks, kb.H, kb.dh, c.s));
    GNOT_RUN(run_linear_seg(c, {{dqkv, &p->T_img[a.q]}, {dqkv + D, &p->T_img[a.k[0]]}, {dqkv + 2 * D, &p->T_img[a.v[0]]}},
                            3 * D, dq_dst, D, P, dq_epi));
  } else {
    GNOT_RUN(run_linear(c, dqkv, D, D, p->T_img[a.q], nullptr, dq_dst, D, D, P, dq_epi, 0));
  }
  if (p->pre_norm)
    GNOT_CK(launch_layer_norm_bwd(p->P_(a.in), D, p->P_(a.rstd), dq_dst, D, P, p->Dr, dquery, D, 1, c.s));
  GNOT_RUN(run_wgrad_side(c, a.wg, {dsum, dqkv}));
  return GNOT_OK;
}

}  // namespace

// the soft-MoE experts of one call: the expert grid writes the [E, P, d] stage (bf16 mode at d = 256: bf16
// stage rows), a moe_combine pass sums residual + experts in expert order (chain2.hip names the forms that
// were measured slower and removed)
// stage_stride: floats between two experts' stage rows (the stage buffer's P * D; the bf16 training forward's
// stage rows are its save slot nl-1, one save chain apart)
static hipError_t launch_moe_pass(gnot_plan* p, const float* base, const float* stage, float* out, hipStream_t s,
                                  long stage_stride = 0) {
  const long P = p->P, D = p->D;
  if (stage_stride == 0) stage_stride = P * D;
  return p->b16s() ? launch_moe_combine_b16(base, stage, stage_stride, p->E, out, P, s)
                   : launch_moe_combine(base, stage, stage_stride, p->E, out, P * D, s);
}

// qout = qin + sum_e s_e ffn_e(C's input); save: the call's saves, or null (inference, MoE recompute)
static int moe_forward(Ctx& c, const Chain& C, const float* qin, float* qout, float* save) {
  gnot_plan* p = c.p;
  const long P = p->P;
  const int D = p->D, E = p->E, NL = p->NL;
  ChainArgs a = chain_args(p, C, false, save);
  a.ldy = D;
  a.Y = p->P_("stage"); a.y_chain_stride = P * D;
  // fp32 training at d = 256: no stage; the combine scales the saved expert outputs itself
  const bool direct = save && p->moe_direct_out();
  if (direct) a.Y = nullptr;
  if (p->b16s() && save) {
    // bf16 training: the experts' bf16 score-scaled terms are kept in save slot nl-1 (the backward's d score
    // operand), so the stage rows ARE that slot (chain2.hip): no separate stage write
    a.Y = save + (NL - 1) * a.save_layer_stride;
    a.y_chain_stride = a.save_chain_stride;
  }
  {
    ProfScope ps(c, "moe_fwd", 2.0 * E * P * NL * (double)D * D);
    GNOT_CK(launch_chain_fwd(cw_scratch(p, a, c.s), c.s));
  }
  if (direct)
    GNOT_CK(launch_moe_combine_scaled(qin, save + (NL - 1) * a.save_layer_stride, a.save_chain_stride, a.scores, a.ldsc,
                                      E, qout, P, D, c.s));
  else
    GNOT_CK(launch_moe_pass(p, qin, a.Y, qout, c.s, a.y_chain_stride));
  return GNOT_OK;
}

// A call that fails part-way through a stream capture (e.g. a collective callback refused) leaves the side
// streams it forked into the capture unjoined, and hipStreamEndCapture then fails with "unjoined work" and
// leaves the caller's stream capturing.  Every side stream still in the capture joins the caller's stream
// again before the error returns, so the capture ends (the caller discards the graph); eager calls skip it.
static void rejoin_side_streams(gnot_plan* p, hipStream_t origin) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(origin, &st) != hipSuccess || st != hipStreamCaptureStatusActive) return;
  for (hipStream_t s : {p->side, p->side2, p->comm_stream}) {
    hipStreamCaptureStatus ss = hipStreamCaptureStatusNone;
    if (!s || hipStreamIsCapturing(s, &ss) != hipSuccess || ss != hipStreamCaptureStatusActive) continue;
    hipEvent_t e = next_event(p);
    if (hipEventRecord(e, s) == hipSuccess) (void)hipStreamWaitEvent(origin, e, 0);
  }
}

static int forward_impl(gnot_plan* p, const float* x, const float* theta, const float* const* fns, float* out,
                        void* stream);
static int backward_impl(gnot_plan* p, const float* dout, int flags, void* stream);
extern "C" int gnot_forward(gnot_plan* p, const float* x, const float* theta, const float* const* fns,
                            float* out, void* stream) {
  const int rc = forward_impl(p, x, theta, fns, out, stream);
  if (rc != GNOT_OK && p) rejoin_side_streams(p, static_cast<hipStream_t>(stream));
  return rc;
}
extern "C" int gnot_backward_ex(gnot_plan* p, const float* dout, int flags, void* stream) {
  // flag validation comes first: it fails before any launch (and before the side streams are touched)
  if (flags & ~(GNOT_BWD_ACCUMULATE | GNOT_BWD_SKIP_GRAD_COMM))
    return fail(GNOT_E_INVALID, "unknown gnot_backward_ex flag bits");
  if (p && (flags & GNOT_BWD_ACCUMULATE) && !p->user_grads)
    return fail(GNOT_E_STATE, "GNOT_BWD_ACCUMULATE needs a caller-owned arena (gnot_plan_set_grad_arena): the "
                              "workspace arena does not survive a geometry change (a re-plan moves or clears it)");
  const int rc = backward_impl(p, dout, flags, stream);
  if (rc != GNOT_OK && p) rejoin_side_streams(p, static_cast<hipStream_t>(stream));
  return rc;
}
extern "C" int gnot_backward(gnot_plan* p, const float* dout, void* stream) {
  return gnot_backward_ex(p, dout, 0, stream);
}

static int forward_impl(gnot_plan* p, const float* x, const float* theta, const float* const* fns, float* out,
                        void* stream) {
  if (!p || !p->ws_bound) return fail(GNOT_E_STATE, "bind_workspace first");
  if (!p->packed) return fail(GNOT_E_STATE, "gnot_pack_weights must run before gnot_forward");
  // theta_dim = 0: theta is [B, 0], whose pointer may be null
  if (!x || (!theta && p->th > 0) || !out || (p->I > 0 && !fns)) return fail(GNOT_E_INVALID, "null input");
  Ctx c{p, static_cast<hipStream_t>(stream)};
  const long P = p->P;
  const int D = p->D;
  const bool tr = p->training;
  p->drop_fwd = p->drop_T > 0 && p->drop_active;   // remembered: gnot_backward mirrors what this forward does
  // the input-function branch (encoders, every block's K/V projections and states) depends only on
  // the input functions: it runs on side2 while the query branch (gating, x encoder) runs here.  The
  // query branch is issued first (graph replay dispatches in capture order).
  const bool br = p->I > 0;
  Ctx cf{p, br ? p->side2 : c.s};
  if (br) {
    hipEvent_t fork = next_event(p);
    GNOT_CK(hipEventRecord(fork, c.s));
    GNOT_CK(hipStreamWaitEvent(cf.s, fork, 0));
  }
  // inputs into the workspace (row pitch rounded to 16 B); with a Fourier order the caller's rows are the raw
  // ones and the staging embeds them (fourier.hip), the pad columns written as zeros
  if (p->nx > 0)
    GNOT_CK(launch_fourier_embed(x, p->in_raw, p->in_raw, p->nx, p->P_("x"), p->bufs["x"].ld, P, c.s));
  else
    GNOT_CK(hipMemcpy2DAsync(p->P_("x"), p->bufs["x"].ld * 4, x, p->in * 4, p->in * 4, P, hipMemcpyDeviceToDevice, c.s));
  if (p->th > 0)
    GNOT_CK(hipMemcpyAsync(p->P_("theta"), theta, (size_t)p->B * p->th * 4, hipMemcpyDeviceToDevice, c.s));
  GNOT_CK(launch_concat_theta(p->P_("x"), p->bufs["x"].ld, p->in, p->P_("theta"), p->th, p->d_xoff, p->B,
                              p->P_("xin"), p->bufs["xin"].ld, (int)P, c.s));
  // one encoder / decoder chain: C's input -> Y, keeping the pre-activations when training
  auto chain_fwd = [&](Ctx& cc, const Chain& C, float* Y, long ldy) -> int {
    ChainArgs a = chain_args(p, C, false, tr ? p->P_(C.save) : nullptr);
    a.Y = Y; a.ldy = ldy;
    GNOT_CK(launch_chain_fwd(cw_scratch(p, a, cc.s), cc.s));
    return GNOT_OK;
  };
  // gating (model.py:155-156) and query encoder (model.py:158-161)
  GNOT_RUN(chain_fwd(c, p->ch_gate(), p->P_("scores"), p->bufs["scores"].ld));
  GNOT_RUN(chain_fwd(c, p->ch_x(), p->P_("query0"), D));
  for (int i = 0; i < p->I; ++i) {
    const std::string n = "fn" + std::to_string(i);
    if (p->Q[i] <= 0) continue;
    if (p->nf > 0)
      GNOT_CK(launch_fourier_embed(fns[i], p->F_raw, p->F_raw, p->nf, p->P_(n), p->bufs[n].ld, p->Q[i], cf.s));
    else
      GNOT_CK(hipMemcpy2DAsync(p->P_(n), p->bufs[n].ld * 4, fns[i], p->F * 4, p->F * 4, p->Q[i],
                               hipMemcpyDeviceToDevice, cf.s));
  }
  // input-function encoders (model.py:164-166)
  for (int i = 0; i < p->I; ++i) GNOT_RUN(chain_fwd(cf, p->ch_fn(i), p->P_("fnenc" + std::to_string(i)), D));
  // key/value projections (model.py:67-75) and states (model.py:77-79) of every (block, input
  // function): they depend only on the input-function encodings, so all L*I of them run batched here
  // one normalisation of the rows an attention call reads (pre-norm): src [rows, D] -> dst, rstd kept in training
  auto norm_fwd = [&](Ctx& cc, const float* src, long rows, const std::string& dst, const std::string& rstd) -> int {
    GNOT_CK(launch_layer_norm(src, D, rows, p->Dr, p->norm_eps, p->P_(dst), D, tr ? p->P_(rstd) : nullptr, cc.s));
    return GNOT_OK;
  };
  if (p->I > 0 && p->L > 0) {
    if (p->pre_norm)
      for (int i = 0; i < p->I; ++i) {
        const std::string si = std::to_string(i);
        GNOT_RUN(norm_fwd(cf, p->P_("fnenc" + si), p->Q[i], "fnn" + si, "fnr" + si));
      }
    GNOT_CK(launch_linear_batch(p->d_fwd_kv_jobs, (int)p->fwd_kv_jobs.size(), (int)p->Qmax(), 2 * D,
                                D > 512 ? D / 2 : D, p->dh, cf.s));
    GNOT_RUN(run_state(cf, p->st_fn));
  }
  if (br) {                                // join the input-function branch
    hipEvent_t join = next_event(p);
    GNOT_CK(hipEventRecord(join, cf.s));
    GNOT_CK(hipStreamWaitEvent(c.s, join, 0));
  }
  // blocks (model.py:126-139)
  for (int l = 0; l < p->L; ++l) {
    const AttnCall &ac = p->call(l, true), &as = p->call(l, false);
    float* query1 = p->P_(as.in_raw);
    // pre-norm: the attention calls read LN(query) / LN(query1); the residual adds below keep the raw rows
    if (p->pre_norm) GNOT_RUN(norm_fwd(c, p->P_(ac.in_raw), P, ac.in, ac.rstd));
    GNOT_RUN(attn_forward(c, ac));
    // ffn1 experts: query1 = query + sum_e s_e ffn1_e(a)   (model.py:128-131)
    const bool keep = tr && !p->moe_recompute;   // recompute: the backward re-runs the call into "mrsave"
    const Chain &m1 = p->ch_moe(l, true), &m2 = p->ch_moe(l, false);
    GNOT_RUN(moe_forward(c, m1, p->P_(ac.in_raw), query1, keep ? p->P_(m1.save) : nullptr));
    if (p->pre_norm) GNOT_RUN(norm_fwd(c, query1, P, as.in, as.rstd));
    GNOT_RUN(attn_forward(c, as));
    // ffn2 experts: query2 = query1 + sum_e s_e ffn2_e(bb)   (model.py:134-137)
    GNOT_RUN(moe_forward(c, m2, query1, p->P_(p->block_query(l + 1)), keep ? p->P_(m2.save) : nullptr));
  }
  // decoder (model.py:171)
  GNOT_RUN(chain_fwd(c, p->ch_out(), out, p->out));
  p->fwd_done = true;
  p->bwd_done = false;
  return GNOT_OK;
}

static int backward_impl(gnot_plan* p, const float* dout, int flags, void* stream) {
  if (!p || !p->ws_bound || !p->fwd_done) return fail(GNOT_E_STATE, "gnot_forward must run before gnot_backward");
  if (!p->training) return fail(GNOT_E_STATE, "plan was set up with training = 0");
  if (!dout) return fail(GNOT_E_INVALID, "null dout");
  p->bwd_accumulate = (flags & GNOT_BWD_ACCUMULATE) != 0;
  p->grad_comm_live = p->grad_comm_on && !(flags & GNOT_BWD_SKIP_GRAD_COMM);
  Ctx c{p, static_cast<hipStream_t>(stream)};
  const long P = p->P;
  const int D = p->D, E = p->E, NL = p->NL;
  float* dquery = p->P_("dquery");
  float* stage = p->P_("stage");
  // the lowest stage that holds a trainable Linear (gnot_plan_set_trainable): the backward runs from the decoder
  // down to it and issues no kernel of the stages below; nothing trainable and no input gradients: nothing at all
  const int stop = p->lowest_stage();
  if (stop > p->L) {
    p->bwd_done = true;
    p->ig_reduced = false;
    return GNOT_OK;
  }
  p->readers.clear();
  p->deferred.clear();
  if (p->grad_comm_live) {                   // the comm stream joins here (a first-level fork of the caller's)
    if (!p->comm_stream) GNOT_CK(hipStreamCreateWithFlags(&p->comm_stream, hipStreamNonBlocking));
    hipEvent_t fork = next_event(p);
    GNOT_CK(hipEventRecord(fork, c.s));
    GNOT_CK(hipStreamWaitEvent(p->comm_stream, fork, 0));
  }
  GNOT_CK(hipMemcpy2DAsync(p->P_("dout"), p->bufs["dout"].ld * 4, dout, p->out * 4, p->out * 4, P,
                           hipMemcpyDeviceToDevice, c.s));
  GNOT_CK(hipMemsetAsync(p->P_("dscore"), 0, P * p->bufs["dscore"].ld * 4, c.s));
  // the backward's ChainArgs of call site C: the saves of its forward, the incoming gradient dY and, where
  // asked for (dxbuf: a buffer's name), the gradient of its input
  auto bwd_args = [&](const Chain& C, const float* dY, long lddy, const std::string& dxbuf = std::string()) {
    ChainArgs a = chain_args(p, C, true, p->P_(C.save));
    a.dY = dY; a.lddy = lddy;
    if (!dxbuf.empty()) { a.dX = p->P_(dxbuf); a.lddx = p->bufs.at(dxbuf).ld; a.dx_chain_stride = 0; }
    return a;
  };
  // launch one chain backward: dZ of every Linear into the chain call's dz slot
  auto chain_bwd_launch = [&](Ctx& cc, const Chain& C, ChainArgs& a, const char* prof) -> int {
    float* dz = p->P_(p->dz_name(C.kcall));
    GNOT_RUN(guard_write(cc, dz));
    a.dz = dz; a.dz_layer_stride = C.rows * D; a.dz_chain_stride = NL * C.rows * D;
    if (a.b16s) { a.dz_layer_stride /= 2; a.dz_chain_stride /= 2; }   // bf16 dZ layers
    a.skip_dz_last = (C.mode == CH_MOE && p->moe_direct_dz()) ? 1 : 0;
    {
      ProfScope ps(cc, prof, 2.0 * a.nchains * C.rows * NL * (double)D * D);
      GNOT_CK(launch_chain_bwd(cw_scratch(p, a, cc.s), cc.s));
    }
    if (cc.s == c.s) GNOT_RUN(flush_deferred(cc));   // earlier groups' side launches after this kernel
    return GNOT_OK;
  };
  // ... and dispatch its weight gradients: in order, or forked to the side stream
  auto chain_bwd = [&](Ctx& cc, const Chain& C, ChainArgs& a, const char* prof) -> int {
    GNOT_RUN(chain_bwd_launch(cc, C, a, prof));
    // the weight gradients read the saved pre-activations too: a recomputed (shared) save buffer
    // must not be overwritten by the next MoE's recompute before they finish.  That guard is the
    // readers map, which only run_wgrad_side from the capture-origin stream registers (side2 runs its
    // groups in order without it): the MoE chains must therefore stay on the origin stream
    if (p->moe_recompute && a.mode == CH_MOE) {
      if (cc.s != c.s) return fail(GNOT_E_STATE, "internal: MoE recompute backward off the origin stream");
      return run_wgrad_side(cc, C.wg, {a.dz, a.save});
    }
    return run_wgrad_side(cc, C.wg, {a.dz});
  };
  // decoder (model.py:171)
  {
    ChainArgs a = bwd_args(p->ch_out(), p->P_("dout"), p->bufs["dout"].ld, "dquery");
    GNOT_RUN(chain_bwd(c, p->ch_out(), a, "chain_bwd"));
  }
  for (int l = p->L - 1; l >= std::max(stop, 0); --l) {
    // ffn2 experts: query2 = query1 + sum_e s_e ffn2_e(bb)   (model.py:134-137)
    for (int m = 2; m >= 1; --m) {
      const bool m1 = (m == 1);
      const Chain& C = p->ch_moe(l, m1);
      if (p->moe_recompute) {
        // re-run this call's expert forward (inputs kept: "a" / "bb") into the shared save buffer
        float* mr = p->P_(C.save);
        GNOT_RUN(guard_write(c, mr));
        ChainArgs f = chain_args(p, C, false, mr);
        // only the saves are needed: no output (Y = null), no combine
        f.ldy = D; f.Y = nullptr; f.y_chain_stride = P * D;
        ProfScope ps(c, "moe_recompute", 2.0 * E * P * NL * (double)D * D);
        GNOT_CK(launch_chain_fwd(cw_scratch(p, f, c.s), c.s));
      }
      ChainArgs a = bwd_args(C, dquery, D);
      const AttnCall& ac = p->call(l, m1);       // the call whose output this MoE read
      float* dsum = p->P_(ac.dsum);
      // d(MoE input) = sum_e W_e0^T dz_e0: each expert's term into the stage, summed by moe_combine
      GNOT_RUN(guard_write(c, dsum));
      a.dX = stage; a.lddx = D; a.dx_chain_stride = P * D;
      GNOT_RUN(chain_bwd(c, C, a, "moe_bwd"));
      GNOT_CK(launch_moe_pass(p, nullptr, stage, dsum, c.s));
      GNOT_RUN(flush_deferred(c));            // the chain's weight gradients: side launch after the pass
      // m2: self attention (model.py:133) ; m1: cross attention (model.py:127)
      GNOT_RUN(attn_backward(c, ac));
    }
  }
  // the input-function branch again runs on side2, concurrently with the query encoder and gating.  A backward
  // that stops above the encoders (stop >= 0) enters it only for the key/value weight gradients of the blocks it
  // ran, and only when one of them is trainable.
  const bool enc = stop < 0;
  const bool kv = p->I > 0 && p->L > 0 && (enc || !p->wg_fnkv.jobs.empty());
  const bool br = p->I > 0 && (enc || kv);
  Ctx cf{p, br ? p->side2 : c.s};
  // ranks issue their gradient collectives in one host order whatever serial_wgrad() says (it is chosen
  // per rank from the local point count): a forked rank still holds the last attention call's groups
  // (block 0's cross call's) deferred here, and side2 issues its groups' all-reduces at once -- flush first
  if (p->grad_comm_live) GNOT_RUN(flush_deferred(c));
  if (br) {
    hipEvent_t fork = next_event(p);
    GNOT_CK(hipEventRecord(fork, c.s));
    GNOT_CK(hipStreamWaitEvent(cf.s, fork, 0));
  }
  // dK, dV of every (block, input function), the encodings' gradient and the key/value weight
  // gradients, batched over blocks (the jobs are in block order: those of the blocks that ran are a suffix)
  if (kv) {
    const int l0 = std::max(stop, 0);
    GNOT_CK(launch_attn_kv_bwd(p->kv_bwd_batch, nullptr, p->d_kvbwd_jobs + (long)l0 * p->I, (p->L - l0) * p->I,
                               p->kv_batch_maxchunks, p->H, p->dh, cf.s));
    if (enc)
      for (size_t k = 0; k < p->d_dfn_jobs.size(); ++k)
        GNOT_CK(launch_linear_batch(p->d_dfn_jobs[k], p->I, (int)p->Qmax(), D, D > 512 ? D / 2 : D, p->dh, cf.s));
    GNOT_RUN(run_wgrad_side(cf, p->wg_fnkv, {}));
    // pre-norm: dfn{i} is so far the gradient of the normalised encodings; pulled through the norm in place
    // (a row is read whole before it is written) before the encoder's chain backward reads it
    if (enc && p->pre_norm)
      for (int i = 0; i < p->I; ++i) {
        const std::string si = std::to_string(i);
        float* dfn = p->P_("dfn" + si);
        GNOT_CK(launch_layer_norm_bwd(p->P_("fnn" + si), D, p->P_("fnr" + si), dfn, D, p->Q[i], p->Dr, dfn, D, 0, cf.s));
      }
  }
  const bool gate_here = enc && br && !p->serial_wgrad();
  if (enc) {
    if (p->I > 0 && p->L == 0)   // encodings unused by the output: zero gradients
      for (int i = 0; i < p->I; ++i)
        GNOT_CK(hipMemsetAsync(p->P_("dfn" + std::to_string(i)), 0, p->Q[i] * D * 4, cf.s));
    // input-function encoders (their inputs need no gradient)
    for (int i = 0; i < p->I; ++i) {
      const std::string si = std::to_string(i);
      ChainArgs a = bwd_args(p->ch_fn(i), p->P_("dfn" + si), D, p->input_grads ? "dfnin" + si : std::string());
      GNOT_RUN(chain_bwd(cf, p->ch_fn(i), a, "chain_bwd"));
    }
    // query encoder
    {
      ChainArgs a = bwd_args(p->ch_x(), dquery, D, p->input_grads ? "dxin" : "");
      GNOT_RUN(chain_bwd(c, p->ch_x(), a, "chain_bwd"));
    }
    // gating: d scores accumulated over every MoE above -> softmax backward -> chain.  With the weight
    // gradients forked and an input-function branch, the gating's own group runs HERE after the branch has
    // joined, on the branch's slab (free by then): forked, it queued behind the query encoder's group on the
    // side stream and ended the step ~45 us later (configs[1] trace); its all-reduce keeps its place, last
    // (its incoming gradient is dscore, no dY)
    ChainArgs a = bwd_args(p->ch_gate(), nullptr, 0, p->input_grads ? "dxg" : "");
    // gate_here: the launch alone (its flush is the query encoder's group: side launch after this kernel)
    if (gate_here) GNOT_RUN(chain_bwd_launch(c, p->ch_gate(), a, "chain_bwd"));
    else GNOT_RUN(chain_bwd(c, p->ch_gate(), a, "chain_bwd"));
  }
  if (br) {                                // join the input-function branch
    hipEvent_t joinf = next_event(p);
    GNOT_CK(hipEventRecord(joinf, cf.s));
    GNOT_CK(hipStreamWaitEvent(c.s, joinf, 0));
  }
  if (gate_here) GNOT_RUN(run_wgrad_here(c, p->ch_gate().wg, p->P_("slab_wgrad2")));
  GNOT_RUN(flush_deferred(c));
  // join the side stream: every gradient is complete when the caller's stream moves on
  hipEvent_t join = next_event(p);
  GNOT_CK(hipEventRecord(join, p->side));
  GNOT_CK(hipStreamWaitEvent(c.s, join, 0));
  if (p->grad_comm_live) {                   // ... and summed over the ranks
    hipEvent_t joinc = next_event(p);
    GNOT_CK(hipEventRecord(joinc, p->comm_stream));
    GNOT_CK(hipStreamWaitEvent(c.s, joinc, 0));
  }
  p->readers.clear();
  p->bwd_done = true;
  p->ig_reduced = false;
  return GNOT_OK;
}

// reference autograd's gradients of x, theta and the input functions (model.py:155-166), from the
// encoders' input gradients of the last gnot_backward
extern "C" int gnot_input_grads(gnot_plan* p, float* dx, float* dtheta, float* const* dfns, void* stream) {
  if (!p || !p->input_grads || !p->ws_bound || !p->training)
    return fail(GNOT_E_STATE, "gnot_plan_set_input_grads(plan, 1) and a training batch are required");
  if (!p->bwd_done)
    return fail(GNOT_E_STATE, "gnot_input_grads reads the encoders' input gradients of a gnot_backward, which must "
                              "follow the last gnot_forward");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const Buf& xin = p->bufs.at("dxin");
  const Buf& xg = p->bufs.at("dxg");
  // with a Fourier order the embedded rows of the forward still sit in "x" / "fn{i}": their cos / sin columns
  // are the factors of the embedding's derivative (fourier.hip), and dx / dfns have the raw widths
  if (dx && p->nx > 0) {
    const Buf& xe = p->bufs.at("x");
    GNOT_CK(launch_fourier_embed_bwd(xe.p, xe.ld, xin.p, xin.ld, xg.p, xg.ld, p->in_raw, p->nx, dx, p->P, s));
  } else if (dx) {
    GNOT_CK(launch_add_cols(xin.p, xin.ld, xg.p, xg.ld, p->in, dx, p->P, s));
  }
  // point-sharded: x's rows are local, but theta (broadcast over ALL points of a sample) and the input
  // functions (replicated on every rank, reached through every rank's attention states) get one partial
  // gradient per rank -- summed over the ranks (every rank must call this: the sums are collectives)
  float* dth = p->P_("dtheta_ws");
  if (dtheta || p->sharded) GNOT_CK(launch_seg_colsum(xin.p, xin.ld, p->in, p->th, p->d_xoff, p->B, dth, s));
  if (p->sharded && p->th > 0) {
    Ctx c{p, s};
    GNOT_RUN(shard_allreduce(c, dth, (long)p->B * p->th));
  }
  if (dtheta && p->th > 0)
    GNOT_CK(hipMemcpyAsync(dtheta, dth, (size_t)p->B * p->th * 4, hipMemcpyDeviceToDevice, s));
  for (int i = 0; i < p->I; ++i) {
    const Buf& f = p->bufs.at("dfnin" + std::to_string(i));
    if (p->sharded && !p->ig_reduced) {
      Ctx c{p, s};
      GNOT_RUN(shard_allreduce(c, f.p, p->Q[i] * f.ld));
    }
    if (!dfns || !dfns[i]) continue;
    if (p->nf > 0) {
      const Buf& fe = p->bufs.at("fn" + std::to_string(i));
      GNOT_CK(launch_fourier_embed_bwd(fe.p, fe.ld, f.p, f.ld, nullptr, 0, p->F_raw, p->nf, dfns[i], p->Q[i], s));
    } else {
      GNOT_CK(launch_add_cols(f.p, f.ld, nullptr, 0, p->F, dfns[i], p->Q[i], s));
    }
  }
  p->ig_reduced = true;
  return GNOT_OK;
}

extern "C" int gnot_profile_enable(gnot_plan* p, const char* kind) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  p->prof_kind = kind ? kind : "";
  p->prof_used = 0;
  p->prof_flops = 0.0;
  p->prof_launches = 0;
  return GNOT_OK;
}

extern "C" int gnot_profile_read(gnot_plan* p, double* ms_total, int64_t* launches, double* flops_total) {
  if (!p) return fail(GNOT_E_INVALID, "null plan");
  double ms = 0.0;
  for (size_t k = 0; k + 1 < p->prof_used; k += 2) {
    GNOT_CK(hipEventSynchronize(p->prof_events[k + 1]));
    float t = 0.f;
    GNOT_CK(hipEventElapsedTime(&t, p->prof_events[k], p->prof_events[k + 1]));
    ms += t;
  }
  if (ms_total) *ms_total = ms;
  if (launches) *launches = p->prof_launches;
  if (flops_total) *flops_total = p->prof_flops;
  p->prof_used = 0;
  p->prof_flops = 0.0;
  p->prof_launches = 0;
  return GNOT_OK;
}

extern "C" int gnot_debug_kernel_forms(const gnot_plan* p, char* text, size_t cap) {
  if (!p || !text) return fail(GNOT_E_INVALID, "null argument");
  if (!p->batch_set) return fail(GNOT_E_STATE, "set_batch first");
  auto attn = [](AttnKernel k) { return k == AttnKernel::Mfma ? "mfma" : k == AttnKernel::Wide ? "wide" : "narrow"; };
  auto state = [](const WgradGroup* G) { return !G || G->jobs.empty() ? "none" : G->state_mfma ? "mfma" : "valu"; };
  std::string t;
  auto put = [&](const char* key, const char* value) { t += (t.empty() ? "" : " ") + std::string(key) + "=" + value; };
  // the apply forms of block 0's calls (every block's are the same); without a block, those its calls would take
  auto apply = [&](bool cross, bool bwd) {
    if (p->L == 0) return attn(apply_form(p, bwd ? AttnPass::ApplyBwd : AttnPass::ApplyFwd, cross ? p->KI : 1));
    return attn(bwd ? p->call(0, cross).apply_bwd : p->call(0, cross).apply_fwd);
  };
  put("apply_fwd.self", apply(false, false));
  put("apply_fwd.cross", apply(true, false));
  put("apply_bwd.self", apply(false, true));
  put("apply_bwd.cross", apply(true, true));
  put("kv_bwd", attn(p->kv_bwd));
  put("kv_bwd_batch", p->I > 0 && p->L > 0 ? attn(p->kv_bwd_batch) : "none");
  put("state.query", state(p->L > 0 ? &p->call(0, false).src[0].st : nullptr));
  put("state.fn", state(&p->st_fn));
  put("serial_wgrad", p->serial_wgrad() ? "1" : "0");
  put("moe_direct_out", p->moe_direct_out() ? "1" : "0");
  put("moe_direct_dz", p->moe_direct_dz() ? "1" : "0");
  if (t.size() + 1 > cap) return fail(GNOT_E_INVALID, "text buffer too small");
  std::memcpy(text, t.c_str(), t.size() + 1);
  return GNOT_OK;
}

extern "C" int gnot_debug_buffer(const gnot_plan* p, const char* name, float** ptr, int64_t* ld) {
  if (!p || !name || !ptr || !p->ws_bound) return fail(GNOT_E_STATE, "bind_workspace first");
  auto it = p->bufs.find(name);
  if (it == p->bufs.end()) return fail(GNOT_E_INVALID, std::string("unknown buffer ") + name);
  *ptr = (p->user_grads && it->first == "grads") ? p->user_grads : it->second.p;
  if (ld) *ld = it->second.ld;
  return GNOT_OK;
}

// ====================================================================== training step
// packed offsets of a loss entry: off[0] = 0, non-decreasing; allow_empty: a sample may have no rows
static int check_loss_offsets(const std::vector<long>& off, bool allow_empty) {
  if (off[0] != 0) return fail(GNOT_E_INVALID, "off[0] must be 0");
  for (size_t b = 0; b + 1 < off.size(); ++b) {
    if (off[b + 1] < off[b]) return fail(GNOT_E_INVALID, "offsets must be non-decreasing");
    if (!allow_empty && off[b + 1] == off[b])
      return fail(GNOT_E_INVALID, "empty sample: its mean over points is undefined");
  }
  return GNOT_OK;
}

// the arrays every AdamW entry takes
static bool adamw_pointers(const float* param, const float* grad, const float* exp_avg, const float* exp_avg_sq,
                           const float* hyper) {
  return param && grad && exp_avg && exp_avg_sq && hyper;
}

// work of the relative kinds: [B][nsplit][2C] partial norms and the [B][C] gradient scales
extern "C" size_t gnot_rel_l2_work_floats(const int64_t* off_host, int B, int C) {
  if (!off_host || B <= 0 || C <= 0) return 0;
  std::vector<long> off(off_host, off_host + B + 1);
  return (size_t)B * rel_l2_splits(off.data(), B) * 2 * C + (size_t)B * C;
}

// ... and of the others: [B][nsplit][C] and the same scales
extern "C" size_t gnot_mse_work_floats(const int64_t* off_host, int B, int C) {
  if (!off_host || B <= 0 || C <= 0) return 0;
  std::vector<long> off(off_host, off_host + B + 1);
  return (size_t)B * rel_l2_splits(off.data(), B) * C + (size_t)B * C;
}

extern "C" size_t gnot_lp_loss_work_floats(const int64_t* off_host, int B, int C) {
  return gnot_rel_l2_work_floats(off_host, B, C);      // the widest layout of the family: two norms per channel
}

// Every loss entry: `name` is the caller's in messages; allow_empty: a sample may have no rows; point_w: the
// per-row weights of gnot_lp_loss_weighted (nullptr: every other entry, the unweighted kernels).
static int loss_entry(const char* name, int kind, bool allow_empty, const float* pred, const float* tgt,
                      const float* point_w, const int64_t* off_dev, const int64_t* off_host, int B, int C, const float* comp_weights,
                      const float* stats, float* work, float* loss, float* terms, float* dpred, void* stream) {
  static_assert(GNOT_LP_REL2 == 0 && GNOT_LP_REL1 == 1 && GNOT_LP_RELINF == 2 && GNOT_LP_MSE == 3 &&
                GNOT_LP_L1 == 4 && GNOT_LP_LINF == 5, "launch_lp's kinds");
  if (!pred || !tgt || !off_dev || !off_host || B <= 0 || C <= 0 || !work || !loss)
    return fail(GNOT_E_INVALID, std::string("bad ") + name + " arguments");
  if (kind < GNOT_LP_REL2 || kind > GNOT_LP_LINF)      // gnot_lp_loss alone passes a caller's number on
    return fail(GNOT_E_INVALID, "lp_loss: unknown kind " + std::to_string(kind));
  if (dpred && (kind == GNOT_LP_RELINF || kind == GNOT_LP_LINF))
    return fail(GNOT_E_INVALID, "lp_loss: relinf and linf are metrics only: they have no gradient (dpred must be null)");
  std::vector<long> off(off_host, off_host + B + 1);
  if (int rc = check_loss_offsets(off, allow_empty)) return rc;
  GNOT_CK(launch_lp(kind, pred, tgt, point_w, reinterpret_cast<const long*>(off_dev), B, C,
                    rel_l2_splits(off.data(), B), off[B], comp_weights, stats, work, loss, terms, dpred,
                    static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_rel_l2_loss(const float* pred, const float* tgt, const int64_t* off_dev, const int64_t* off_host,
                                int B, int C, float* work, float* loss, float* dpred, void* stream) {
  return loss_entry("rel_l2", GNOT_LP_REL2, true, pred, tgt, nullptr, off_dev, off_host, B, C, nullptr, nullptr, work,
                    loss, nullptr, dpred, stream);
}

extern "C" int gnot_rel_l2_loss_affine(const float* pred, const float* tgt, const int64_t* off_dev,
                                       const int64_t* off_host, int B, int C, const float* out_stats, float* work,
                                       float* loss, float* dpred, void* stream) {
  if (!out_stats) return fail(GNOT_E_INVALID, "rel_l2_loss_affine: null out_stats");
  return loss_entry("rel_l2", GNOT_LP_REL2, true, pred, tgt, nullptr, off_dev, off_host, B, C, nullptr, out_stats, work,
                    loss, nullptr, dpred, stream);
}

extern "C" int gnot_mse_loss(const float* pred, const float* tgt, const int64_t* off_dev, const int64_t* off_host,
                             int B, int C, float* work, float* loss, float* dpred, void* stream) {
  return loss_entry("mse", GNOT_LP_MSE, false, pred, tgt, nullptr, off_dev, off_host, B, C, nullptr, nullptr, work,
                    loss, nullptr, dpred, stream);
}

extern "C" int gnot_mse_loss_affine(const float* pred, const float* tgt, const int64_t* off_dev,
                                    const int64_t* off_host, int B, int C, const float* out_stats, float* work,
                                    float* loss, float* dpred, void* stream) {
  if (!out_stats) return fail(GNOT_E_INVALID, "mse_loss_affine: null out_stats");
  return loss_entry("mse", GNOT_LP_MSE, false, pred, tgt, nullptr, off_dev, off_host, B, C, nullptr, out_stats, work,
                    loss, nullptr, dpred, stream);
}

extern "C" int gnot_lp_loss(const float* pred, const float* tgt, const int64_t* off_dev, const int64_t* off_host,
                            int B, int C, int kind, const float* comp_weights, const float* out_stats, float* work,
                            float* loss, float* terms, float* dpred, void* stream) {
  return loss_entry("lp_loss", kind, false, pred, tgt, nullptr, off_dev, off_host, B, C, comp_weights, out_stats, work,
                    loss, terms, dpred, stream);
}

extern "C" size_t gnot_lp_loss_weighted_work_floats(const int64_t* off_host, int B, int C) {
  return gnot_rel_l2_work_floats(off_host, B, C);      // two floats per channel: the norms, or the norm and sum w
}

extern "C" int gnot_lp_loss_weighted(const float* pred, const float* tgt, const float* point_w, const int64_t* off_dev,
                                     const int64_t* off_host, int B, int C, int kind, const float* comp_weights,
                                     const float* out_stats, float* work, float* loss, float* terms, float* dpred,
                                     void* stream) {
  if (!point_w) return fail(GNOT_E_INVALID, "lp_loss_weighted: null point_w");
  return loss_entry("lp_loss_weighted", kind, false, pred, tgt, point_w, off_dev, off_host, B, C, comp_weights,
                    out_stats, work, loss, terms, dpred, stream);
}

extern "C" int gnot_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                               const float* hyper, void* stream) {
  if (!adamw_pointers(param, grad, exp_avg, exp_avg_sq, hyper) || n < 0)
    return fail(GNOT_E_INVALID, "bad adamw arguments");
  GNOT_CK(launch_adamw_update(param, grad, exp_avg, exp_avg_sq, nullptr, n, hyper, nullptr, nullptr,
                              static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" size_t gnot_grad_clip_work_floats(int64_t n) { return (size_t)grad_clip_partials(n); }

extern "C" int gnot_grad_clip(const float* grad, int64_t n, const float* hyper, float max_norm, float* work,
                              float* clip, void* stream) {
  if (!grad || !hyper || !work || !clip) return fail(GNOT_E_INVALID, "bad grad_clip arguments");
  // stage 1 launches one workgroup of 256 threads per partial: 2^32 threads per grid at the most
  if (n < 1 || grad_clip_partials(n) >= (1L << 24)) return fail(GNOT_E_INVALID, "grad_clip: n out of range");
  if (!(max_norm > 0.f) || !std::isfinite(max_norm))
    return fail(GNOT_E_INVALID, "grad_clip: max_norm must be positive and finite");
  GNOT_CK(launch_grad_clip(grad, n, hyper, max_norm, work, clip, static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_adamw_step_clipped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                       const float* hyper, const float* clip, void* stream) {
  if (!adamw_pointers(param, grad, exp_avg, exp_avg_sq, hyper) || n < 0 || !clip)
    return fail(GNOT_E_INVALID, "bad adamw arguments");
  GNOT_CK(launch_adamw_update(param, grad, exp_avg, exp_avg_sq, nullptr, n, hyper, clip, nullptr,
                              static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_grad_norm(const float* grad, int64_t n, const float* hyper, float* work, float* clip, void* stream) {
  if (!grad || !hyper || !work || !clip) return fail(GNOT_E_INVALID, "bad grad_norm arguments");
  if (n < 1 || grad_clip_partials(n) >= (1L << 24)) return fail(GNOT_E_INVALID, "grad_norm: n out of range");
  GNOT_CK(launch_grad_norm(grad, n, hyper, work, clip, static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                       const float* hyper, const float* clip, int32_t* guard, void* stream) {
  if (!adamw_pointers(param, grad, exp_avg, exp_avg_sq, hyper) || n < 1 || !clip || !guard)
    return fail(GNOT_E_INVALID, "bad guarded adamw arguments");
  GNOT_CK(launch_adamw_update(param, grad, exp_avg, exp_avg_sq, nullptr, n, hyper, clip, guard,
                              static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_ema_update(float* ema, const float* param, int64_t n, const float* weight, void* stream) {
  if (!ema || !param || n < 1 || !weight) return fail(GNOT_E_INVALID, "bad ema_update arguments");
  if (ema == param) return fail(GNOT_E_INVALID, "ema_update: ema must not alias param");
  GNOT_CK(launch_ema_update(ema, param, n, weight, static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_adamw_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                                   int64_t n, const float* hyper, const float* clip, int32_t* guard, void* stream) {
  if (!adamw_pointers(param, grad, exp_avg, exp_avg_sq, hyper) || !ema || n < 1)
    return fail(GNOT_E_INVALID, "bad ema adamw arguments");
  if (guard && !clip) return fail(GNOT_E_INVALID, "adamw_step_ema: a guard needs a clip");
  if (ema == param) return fail(GNOT_E_INVALID, "adamw_step_ema: ema must not alias param");
  GNOT_CK(launch_adamw_update(param, grad, exp_avg, exp_avg_sq, ema, n, hyper, clip, guard,
                              static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

// the host copy of a slice table {begin, len, group}: rows sorted and disjoint inside [0, n), 1 <= len <= 8192,
// 0 <= group < G (G < 0: the caller does not read the group column, it is not checked); one workgroup per row,
// so fewer than 2^24 rows as for gnot_grad_clip's partials
static int check_slices(const char* who, const int64_t* slices_host, int64_t nslices, int64_t n, int64_t G) {
  if (!slices_host) return fail(GNOT_E_INVALID, std::string(who) + ": null slices_host");
  if (nslices < 1 || nslices >= (1L << 24)) return fail(GNOT_E_INVALID, std::string(who) + ": nslices out of range");
  // every step of a training loop walks the table here: integer compares alone, the message only on a refusal
  int64_t end = 0;
  for (int64_t k = 0; k < nslices; ++k) {
    const int64_t begin = slices_host[3 * k], len = slices_host[3 * k + 1], group = slices_host[3 * k + 2];
    const char* bad = (len < 1 || len > 8192) ? " has a length outside [1, 8192]"
                      : begin < end           ? " is not sorted behind and disjoint from the one before it"
                      : begin > n - len       ? " does not lie inside [0, n)"
                      : (G >= 0 && (group < 0 || group >= G)) ? " names a group outside [0, G)" : nullptr;
    if (bad) return fail(GNOT_E_INVALID, std::string(who) + ": slice " + std::to_string(k) + bad);
    end = begin + len;
  }
  return GNOT_OK;
}

extern "C" int gnot_adamw_step_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                                      int64_t n, const float* hyper, const float* ghyper, int G,
                                      const int64_t* slices_dev, const int64_t* slices_host, int64_t nslices,
                                      const float* clip, int32_t* guard, void* stream) {
  if (!adamw_pointers(param, grad, exp_avg, exp_avg_sq, hyper) || !ghyper || !slices_dev || n < 1 || G < 1)
    return fail(GNOT_E_INVALID, "bad adamw_step_groups arguments");
  if (guard && !clip) return fail(GNOT_E_INVALID, "adamw_step_groups: a guard needs a clip");
  if (ema && ema == param) return fail(GNOT_E_INVALID, "adamw_step_groups: ema must not alias param");
  if (int rc = check_slices("adamw_step_groups", slices_host, nslices, n, G)) return rc;
  GNOT_CK(launch_adamw_groups(param, grad, exp_avg, exp_avg_sq, ema, hyper, ghyper,
                              reinterpret_cast<const long*>(slices_dev), nslices, clip, guard,
                              static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

// gnot_grad_norm_groups (norm_only) and gnot_grad_clip_groups; the group column is not read by the norm
static int grad_norm_groups(const char* who, const float* grad, int64_t n, const float* hyper, float max_norm,
                            int norm_only, const int64_t* slices_dev, const int64_t* slices_host, int64_t nslices,
                            float* work, float* clip, void* stream) {
  if (!grad || !hyper || !slices_dev || !work || !clip || n < 1)
    return fail(GNOT_E_INVALID, std::string("bad ") + who + " arguments");
  if (int rc = check_slices(who, slices_host, nslices, n, -1)) return rc;
  GNOT_CK(launch_grad_norm_slices(grad, reinterpret_cast<const long*>(slices_dev), nslices, hyper, max_norm, norm_only,
                                  work, clip, static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_grad_norm_groups(const float* grad, int64_t n, const float* hyper, const int64_t* slices_dev,
                                     const int64_t* slices_host, int64_t nslices, float* work, float* clip,
                                     void* stream) {
  return grad_norm_groups("grad_norm_groups", grad, n, hyper, 1.0f, 1, slices_dev, slices_host, nslices, work, clip,
                          stream);
}

extern "C" int gnot_grad_clip_groups(const float* grad, int64_t n, const float* hyper, float max_norm,
                                     const int64_t* slices_dev, const int64_t* slices_host, int64_t nslices,
                                     float* work, float* clip, void* stream) {
  if (!(max_norm > 0.f) || !std::isfinite(max_norm))
    return fail(GNOT_E_INVALID, "grad_clip_groups: max_norm must be positive and finite");
  return grad_norm_groups("grad_clip_groups", grad, n, hyper, max_norm, 0, slices_dev, slices_host, nslices, work, clip,
                          stream);
}

// gnot_gather_rows (stats == nullptr) and gnot_gather_rows_affine
static int gather_rows(const float* src, int C, const int64_t* table_dev, const int64_t* table_host, int B,
                       const float* stats, float* dst, void* stream) {
  if (!src || !table_dev || !table_host || !dst) return fail(GNOT_E_INVALID, "gather_rows: null argument");
  if (B < 1 || C < 1) return fail(GNOT_E_INVALID, "gather_rows: B and C must be at least 1");
  long rows = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t* T = table_host + (long)b * kGatherCols;      // {src_row0, n, dst_row0, k, key_lo, key_hi}
    if (T[0] < 0) return fail(GNOT_E_INVALID, "gather_rows: src_row0 must not be negative");
    if (T[1] < 0 || T[1] >= (1L << 31)) return fail(GNOT_E_INVALID, "gather_rows: n must be in [0, 2^31)");
    if (T[3] < 0 || T[3] > T[1]) return fail(GNOT_E_INVALID, "gather_rows: k must be in [0, n]");
    if (T[4] < 0 || T[4] >= (1L << 32) || T[5] < 0 || T[5] >= (1L << 32))
      return fail(GNOT_E_INVALID, "gather_rows: keys must be in [0, 2^32)");
    if (T[2] != rows)
      return fail(GNOT_E_INVALID, "gather_rows: dst_row0 must start at 0 and continue by k from segment to segment");
    rows += T[3];
  }
  if (rows == 0) return GNOT_OK;
  GNOT_CK(launch_gather_rows(src, C, reinterpret_cast<const long*>(table_dev), B, stats, dst, rows,
                             static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_gather_rows(const float* src, int C, const int64_t* table_dev, const int64_t* table_host, int B,
                                float* dst, void* stream) {
  return gather_rows(src, C, table_dev, table_host, B, nullptr, dst, stream);
}

extern "C" int gnot_gather_rows_affine(const float* src, int C, const int64_t* table_dev, const int64_t* table_host,
                                       int B, const float* stats, float* dst, void* stream) {
  if (!stats) return fail(GNOT_E_INVALID, "gather_rows_affine: null stats");
  return gather_rows(src, C, table_dev, table_host, B, stats, dst, stream);
}

extern "C" size_t gnot_channel_stats_work_floats(int64_t rows, int C) {
  if (rows < 1 || C < 1) return 0;
  return (size_t)channel_stats_slices(rows) * 3 * (size_t)C;
}

extern "C" int gnot_channel_stats(const float* src, int64_t rows, int C, float eps, float* work, float* stats,
                                  void* stream) {
  if (!src || !work || !stats) return fail(GNOT_E_INVALID, "channel_stats: null argument");
  if (rows < 1 || rows >= (1L << 31)) return fail(GNOT_E_INVALID, "channel_stats: rows must be in [1, 2^31)");
  if (C < 1) return fail(GNOT_E_INVALID, "channel_stats: C must be at least 1");
  if (!(eps >= 0.f) || !std::isfinite(eps))
    return fail(GNOT_E_INVALID, "channel_stats: eps must be finite and not negative");
  GNOT_CK(launch_channel_stats(src, rows, C, eps, work, stats, static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" size_t gnot_channel_stats_weighted_work_floats(int64_t rows, int C) {
  if (rows < 1 || C < 1) return 0;
  return (size_t)channel_stats_slices(rows) * (2 + 3 * (size_t)C);
}

extern "C" int gnot_channel_stats_weighted(const float* src, const float* w, int64_t rows, int C, float eps,
                                           float* work, float* stats, void* stream) {
  if (!src || !w || !work || !stats) return fail(GNOT_E_INVALID, "channel_stats_weighted: null argument");
  if (rows < 1 || rows >= (1L << 31))
    return fail(GNOT_E_INVALID, "channel_stats_weighted: rows must be in [1, 2^31)");
  if (C < 1) return fail(GNOT_E_INVALID, "channel_stats_weighted: C must be at least 1");
  if (!(eps >= 0.f) || !std::isfinite(eps))
    return fail(GNOT_E_INVALID, "channel_stats_weighted: eps must be finite and not negative");
  GNOT_CK(launch_channel_stats_weighted(src, w, rows, C, eps, work, stats, static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_debug_gelu(const float* x, float* y, float* dy, float* y2, float* dy2, int64_t n, void* stream) {
  if (!x || !y || !dy || !y2 || !dy2 || n < 1) return fail(GNOT_E_INVALID, "bad debug_gelu arguments");
  GNOT_CK(launch_debug_gelu(x, y, dy, y2, dy2, n, static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_fourier_embed(const float* src, int64_t rows, int C, int n, float* dst, int64_t ld, void* stream) {
  if (!src || !dst) return fail(GNOT_E_INVALID, "fourier_embed: null pointer");
  if (rows < 1 || C < 1) return fail(GNOT_E_INVALID, "fourier_embed: rows and C must be at least 1");
  if (n < 1 || n > 8) return fail(GNOT_E_INVALID, "fourier_embed: the order must be in [1, 8]");
  if (ld < (int64_t)C * (4 * n + 3)) return fail(GNOT_E_INVALID, "fourier_embed: ld is less than C (4 n + 3)");
  if (ld >= (1LL << 31)) return fail(GNOT_E_INVALID, "fourier_embed: ld must be below 2^31 (32-bit column indices)");
  GNOT_CK(launch_fourier_embed(src, C, C, n, dst, ld, rows, static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_fourier_embed_bwd(const float* emb, int64_t ld, const float* g, int64_t ldg, const float* g2,
                                      int64_t ldg2, int64_t rows, int C, int n, float* dv, void* stream) {
  if (!emb || !g || !dv) return fail(GNOT_E_INVALID, "fourier_embed_bwd: null pointer");
  if (rows < 1 || C < 1) return fail(GNOT_E_INVALID, "fourier_embed_bwd: rows and C must be at least 1");
  if (n < 1 || n > 8) return fail(GNOT_E_INVALID, "fourier_embed_bwd: the order must be in [1, 8]");
  const int64_t CW = (int64_t)C * (4 * n + 3);
  if (ld < CW || ldg < CW || (g2 && ldg2 < CW))
    return fail(GNOT_E_INVALID, "fourier_embed_bwd: a row pitch is less than C (4 n + 3)");
  if (CW >= (1LL << 31)) return fail(GNOT_E_INVALID, "fourier_embed_bwd: C (4 n + 3) must be below 2^31");
  GNOT_CK(launch_fourier_embed_bwd(emb, ld, g, ldg, g2, ldg2, C, n, dv, rows, static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

// what both LayerNorm entries refuse about one [rows, ld] array of C real columns
static const char* norm_array_error(const void* ptr, int64_t ld, int C) {
  if (ld < C) return "a row pitch is less than C";
  if (ld % 4 != 0) return "a row pitch is not a multiple of 4";
  if (ld >= (1LL << 31)) return "a row pitch must be below 2^31";
  if (reinterpret_cast<uintptr_t>(ptr) & 15) return "pointers must be 16-byte aligned";
  return nullptr;
}
static const char* norm_shape_error(int64_t rows, int C) {
  if (rows < 1 || rows >= (1LL << 31)) return "rows must be in [1, 2^31)";
  if (C < 1 || C > 1024) return "C must be in [1, 1024]";
  return nullptr;
}

extern "C" int gnot_layer_norm(const float* x, int64_t ldx, int64_t rows, int C, float eps, float* y, int64_t ldy,
                               float* rstd, void* stream) {
  if (!x || !y) return fail(GNOT_E_INVALID, "layer_norm: null pointer");
  const char* e = norm_shape_error(rows, C);
  if (!e) e = norm_array_error(x, ldx, C);
  if (!e) e = norm_array_error(y, ldy, C);
  if (!e && (reinterpret_cast<uintptr_t>(rstd) & 15)) e = "pointers must be 16-byte aligned";
  if (!e && (!std::isfinite(eps) || !(eps > 0.f))) e = "eps must be finite and positive";
  if (e) return fail(GNOT_E_INVALID, std::string("layer_norm: ") + e);
  GNOT_CK(launch_layer_norm(x, ldx, rows, C, eps, y, ldy, rstd, static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_layer_norm_bwd(const float* y, int64_t ldy, const float* rstd, const float* dy, int64_t lddy,
                                   int64_t rows, int C, float* dx, int64_t lddx, int accumulate, void* stream) {
  if (!y || !rstd || !dy || !dx) return fail(GNOT_E_INVALID, "layer_norm_bwd: null pointer");
  const char* e = norm_shape_error(rows, C);
  if (!e) e = norm_array_error(y, ldy, C);
  if (!e) e = norm_array_error(dy, lddy, C);
  if (!e) e = norm_array_error(dx, lddx, C);
  if (!e && (reinterpret_cast<uintptr_t>(rstd) & 15)) e = "pointers must be 16-byte aligned";
  if (e) return fail(GNOT_E_INVALID, std::string("layer_norm_bwd: ") + e);
  GNOT_CK(launch_layer_norm_bwd(y, ldy, rstd, dy, lddy, rows, C, dx, lddx, accumulate, static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" int gnot_dropout_rows(float* x, int64_t ld, int64_t rows, int C, const int64_t* off_dev,
                                 const int64_t* glo_dev, int B, const uint32_t* key_dev, uint32_t site, float prob,
                                 void* stream) {
  if (!x || !off_dev || !glo_dev || !key_dev) return fail(GNOT_E_INVALID, "dropout_rows: null pointer");
  const char* e = norm_shape_error(rows, C);
  if (!e) e = norm_array_error(x, ld, C);
  if (!e && B < 1) e = "B must be at least 1";
  if (!e && ((reinterpret_cast<uintptr_t>(off_dev) | reinterpret_cast<uintptr_t>(glo_dev)) & 7)) e = "the offsets must be 8-byte aligned";
  if (!e && (reinterpret_cast<uintptr_t>(key_dev) & 3)) e = "the key must be 4-byte aligned";
  if (!e && site >= (1u << 24)) e = "site must be below 2^24";
  uint32_t T = 0;
  float scale = 1.f;
  if (!e && !drop_threshold(prob, T, scale)) e = "p must be finite and in [0, 1)";
  if (e) return fail(GNOT_E_INVALID, std::string("dropout_rows: ") + e);
  GNOT_CK(launch_dropout_rows(x, ld, rows, C, reinterpret_cast<const long*>(off_dev),
                              reinterpret_cast<const long*>(glo_dev), B, key_dev, site, T, scale,
                              static_cast<hipStream_t>(stream)));
  return GNOT_OK;
}

extern "C" const char* gnot_last_error(void) { return g_err.c_str(); }
extern "C" const char* gnot_version(void) { return "gnot-mi355x 0.1 (gfx950, fp32 MFMA)"; }
