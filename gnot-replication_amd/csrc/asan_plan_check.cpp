// Host-side planning check, built with AddressSanitizer on the HOST code only (csrc/Makefile `asan`):
// exercises every C-ABI entry point that needs no GPU -- plan creation for the supported widths and for the edges
// of the other constructor arguments (depth, blocks, theta_dim 0, experts, input functions, input / output widths), packed
// batch geometries (ragged, empty samples, many meshes, padded-equal strides), MoE recompute and
// precision switches, the pre-norm option, the shapes of an attention call (fused, input-function sources, padded heads,
// frozen blocks) with their backward plans, workspace sizing, gradient offsets, the caller-owned gradient arena, the flag
// validation of gnot_backward_ex, the point-shard exchange tables and the error paths -- so heap overflows / use-after-free in engine.cpp's table building show up on the CPU.
// Run by tests/test_asan.py; exit status 0 = every check passed and ASan reported nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "gnot_hip.h"

static int g_fail = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "CHECK failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond,   \
                   gnot_last_error());                                                   \
      ++g_fail;                                                                          \
    }                                                                                    \
  } while (0)

// FNV-1a over every workspace size the program sees, in order: two builds of the planning code that print the
// same digest lay every geometry below out in the same number of bytes
static uint64_t g_digest = 0xcbf29ce484222325ull;
static void fold(uint64_t v) {
  for (int k = 0; k < 8; ++k) g_digest = (g_digest ^ (v >> (8 * k) & 0xff)) * 0x100000001b3ull;
}
static size_t ws_bytes(const gnot_plan* p) {
  const size_t v = gnot_plan_workspace_bytes(p);
  fold(v);
  return v;
}
// ... and over the backward plan of every training plan: its weight-gradient job count and lowest stage
static void fold_backward_plan(const gnot_plan* p) {
  int jobs = -1, stage = -99;
  CHECK(gnot_debug_backward_plan(p, &jobs, &stage) == GNOT_OK);
  CHECK(jobs >= 0);
  fold((uint64_t)(int64_t)jobs);
  fold((uint64_t)(int64_t)stage);
}

static int fake_allreduce(void*, float*, int64_t, void*) { return 0; }
static int fake_alltoallv(void*, const float*, const int64_t*, float*, const int64_t*, void*) { return 0; }

static std::vector<int64_t> offsets(const std::vector<int64_t>& n) {
  std::vector<int64_t> o(1, 0);
  for (int64_t v : n) o.push_back(o.back() + v);
  return o;
}

// one plan: several batch geometries, both precisions and recompute settings, sharded geometries
static void exercise(const gnot_config& cfg, std::mt19937& rng) {
  gnot_plan* p = nullptr;
  CHECK(gnot_plan_create(&cfg, &p) == GNOT_OK);
  if (!p) return;
  const int nlin = gnot_plan_num_linears(p);
  CHECK(nlin > 0);
  std::vector<int32_t> dims(2 * nlin);
  CHECK(gnot_plan_linear_dims(p, dims.data()) == GNOT_OK);
  const int I = cfg.n_input_functions;
  for (int trial = 0; trial < 12; ++trial) {
    const int B = 1 + (int)(rng() % (trial < 6 ? 4 : 64));
    std::vector<int64_t> n(B), m(B);
    for (int b = 0; b < B; ++b) {
      n[b] = (trial == 2 && b == 0) ? 0 : 1 + (int64_t)(rng() % 3000);   // an empty sample once
      m[b] = 1 + (int64_t)(rng() % 900);
    }
    if (trial == 1) for (int b = 0; b < B; ++b) n[b] = n[0] ? n[0] : 1;  // padded-equal strides
    const auto xo = offsets(n);
    std::vector<int64_t> fo;
    for (int i = 0; i < I; ++i) {
      const auto o = offsets(m);
      fo.insert(fo.end(), o.begin(), o.end());
    }
    for (int rc = 0; rc < 2; ++rc)
      for (int bf = 0; bf < 2; ++bf) {
        CHECK(gnot_plan_set_moe_recompute(p, rc) == GNOT_OK);
        CHECK(gnot_plan_set_precision(p, bf) == GNOT_OK);
        for (int tr = 0; tr < 2; ++tr) {
          const int st = gnot_plan_set_batch(p, B, xo.data(), I ? fo.data() : nullptr, tr);
          if (xo.back() == 0) {
            CHECK(st == GNOT_E_INVALID);
            continue;
          }
          CHECK(st == GNOT_OK);
          CHECK(ws_bytes(p) > 0);
          if (tr) fold_backward_plan(p);
          std::vector<int64_t> go(2 * nlin);
          CHECK(gnot_plan_grad_offsets(p, go.data()) == GNOT_OK);
          int64_t expect = 0;
          for (int k = 0; k < nlin; ++k) {
            CHECK(go[2 * k] == expect);
            expect += (int64_t)dims[2 * k] * dims[2 * k + 1];
            CHECK(go[2 * k + 1] == expect);
            expect += dims[2 * k];
          }
        }
      }
    // point sharding: every rank's local geometry of the same global batch
    const int world = 2 + (int)(rng() % 7);
    gnot_comm comm{nullptr, fake_allreduce, fake_alltoallv};
    for (int r = 0; r < world; ++r) {
      CHECK(gnot_plan_set_shard(p, r, world, B, n.data(), &comm) == GNOT_OK);
      std::vector<int64_t> loc(B);
      for (int b = 0; b < B; ++b) {
        int64_t lo, hi;
        CHECK(gnot_shard_range(n[b], r, world, &lo, &hi) == GNOT_OK);
        loc[b] = hi - lo;
      }
      const auto lo = offsets(loc);
      const int st = gnot_plan_set_batch(p, B, lo.data(), I ? fo.data() : nullptr, 1);
      CHECK(st == GNOT_OK || lo.back() == 0);
      if (st == GNOT_OK) {
        CHECK(ws_bytes(p) > 0);
        fold_backward_plan(p);
      }
      // a geometry that does not match the declared shard is refused
      if (lo.back() > 0) {
        auto bad = lo;
        bad.back() += 1;
        CHECK(gnot_plan_set_batch(p, B, bad.data(), I ? fo.data() : nullptr, 1) == GNOT_E_INVALID);
      }
    }
    CHECK(gnot_plan_set_shard(p, 0, 1, B, n.data(), nullptr) == GNOT_OK);
  }
  // caller-owned gradient arena: the size is known from create on; a short or misaligned arena is refused;
  // a good one invalidates the batch and leaves workspace size and offsets as they were (the pointer is
  // only stored in the job tables here, nothing dereferences it without a GPU)
  {
    int64_t gf = 0;
    for (int k = 0; k < nlin; ++k) gf += (int64_t)dims[2 * k] * dims[2 * k + 1] + dims[2 * k];
    CHECK(gnot_plan_grad_floats(p) == gf);
    CHECK(gnot_plan_grad_floats(nullptr) == 0);
    const std::vector<int64_t> n2 = {300, 77}, m2 = {40, 40};
    const auto xo = offsets(n2);
    std::vector<int64_t> fo;
    for (int i = 0; i < I; ++i) {
      const auto o = offsets(m2);
      fo.insert(fo.end(), o.begin(), o.end());
    }
    CHECK(gnot_plan_set_batch(p, 2, xo.data(), I ? fo.data() : nullptr, 1) == GNOT_OK);
    const size_t ws = ws_bytes(p);
    std::vector<float> host(gf + 8);
    float* arena = host.data();
    while (reinterpret_cast<uintptr_t>(arena) & 15) ++arena;
    CHECK(gnot_plan_set_grad_arena(p, arena, gf - 1) == GNOT_E_INVALID);
    CHECK(gnot_plan_set_grad_arena(p, arena + 1, gf) == GNOT_E_INVALID);
    CHECK(gnot_plan_set_grad_arena(nullptr, arena, gf) == GNOT_E_INVALID);
    CHECK(ws_bytes(p) == ws);               // the refusals changed nothing
    // the flag validation of gnot_backward_ex fails before any launch
    float dout = 0.f;
    CHECK(gnot_backward_ex(p, &dout, 4, nullptr) == GNOT_E_INVALID);
    CHECK(gnot_backward_ex(p, &dout, GNOT_BWD_ACCUMULATE | 8, nullptr) == GNOT_E_INVALID);
    CHECK(gnot_backward_ex(p, &dout, GNOT_BWD_ACCUMULATE, nullptr) == GNOT_E_STATE);   // no caller arena
    CHECK(gnot_plan_set_grad_arena(p, arena, gf) == GNOT_OK);
    CHECK(ws_bytes(p) == 0);                // batch invalidated
    CHECK(gnot_plan_set_batch(p, 2, xo.data(), I ? fo.data() : nullptr, 1) == GNOT_OK);
    CHECK(ws_bytes(p) == ws);               // same layout with a caller arena
    std::vector<int64_t> go(2 * nlin);
    CHECK(gnot_plan_grad_offsets(p, go.data()) == GNOT_OK);
    CHECK(go[0] == 0 && go[2 * nlin - 1] + dims[2 * nlin - 2] == gf);
    CHECK(gnot_plan_set_grad_arena(p, arena, gf) == GNOT_OK);   // the same arena again: nothing invalidated
    CHECK(ws_bytes(p) == ws);
    CHECK(gnot_plan_set_grad_arena(p, nullptr, 0) == GNOT_OK);  // back to the workspace arena
    CHECK(ws_bytes(p) == 0);
    CHECK(gnot_backward_ex(p, &dout, GNOT_BWD_ACCUMULATE | GNOT_BWD_SKIP_GRAD_COMM, nullptr) == GNOT_E_STATE);
  }
  gnot_plan_destroy(p);
}

// the scramble exchange tables: what rank r sends to t is what t receives from r, and the segments
// cover the local buffers exactly
static void exchange(std::mt19937& rng) {
  for (int trial = 0; trial < 40; ++trial) {
    const int B = 1 + (int)(rng() % 5), world = 1 + (int)(rng() % 8);
    const int H = 1 + (int)(rng() % 8), dh = 4 * (1 + (int)(rng() % 8));
    std::vector<int64_t> n(B);
    for (int b = 0; b < B; ++b) n[b] = (int64_t)(rng() % 5000);
    std::vector<std::vector<int64_t>> sc(world, std::vector<int64_t>(world)), rc = sc;
    for (int r = 0; r < world; ++r) {
      int64_t nseg = 0;
      CHECK(gnot_shard_exchange(B, n.data(), H, dh, r, world, sc[r].data(), rc[r].data(), nullptr, 0, &nseg) ==
            GNOT_OK);
      std::vector<int64_t> segs(4 * (nseg + 1));
      int64_t nseg2 = 0;
      CHECK(gnot_shard_exchange(B, n.data(), H, dh, r, world, nullptr, nullptr, segs.data(), nseg, &nseg2) ==
            GNOT_OK);
      CHECK(nseg2 == nseg);
      int64_t local = 0, sent = 0, recvd = 0, tot_s = 0, tot_r = 0;
      for (int b = 0; b < B; ++b) {
        int64_t lo, hi;
        gnot_shard_range(n[b], r, world, &lo, &hi);
        local += (hi - lo) * H * dh;
      }
      for (int64_t k = 0; k < nseg; ++k) {
        CHECK(segs[4 * k + 3] >= 0);
        (segs[4 * k] == 0 ? sent : recvd) += segs[4 * k + 3];
      }
      for (int t = 0; t < world; ++t) {
        tot_s += sc[r][t];
        tot_r += rc[r][t];
      }
      CHECK(sent == tot_s && recvd == tot_r);
      CHECK(tot_s == local && tot_r == local);
    }
    for (int r = 0; r < world; ++r)
      for (int t = 0; t < world; ++t) CHECK(sc[r][t] == rc[t][r]);
  }
  // argument errors
  int64_t lo, hi, nseg;
  CHECK(gnot_shard_range(10, 2, 2, &lo, &hi) == GNOT_E_INVALID);
  CHECK(gnot_shard_exchange(0, nullptr, 8, 32, 0, 1, nullptr, nullptr, nullptr, 0, &nseg) == GNOT_E_INVALID);
}

// pre-norm (gnot_plan_set_pre_norm): training and inference plans with and without input functions at a plain,
// a padded and a layer-wise width; the option adds buffers and re-targets job tables, on-then-off restores the
// plain layout, and the stand-alone entries refuse bad arguments before any launch.  (Its sizes stay out of
// the layout digest, and it draws from a generator of its own: the digest keeps describing the plain plans.)
static void pre_norm() {
  std::mt19937 rng(777);
  const int widths[][2] = {{64, 4}, {40, 2}, {30, 5}, {256, 8}, {320, 5}, {576, 9}};
  for (const auto& wh : widths)
    for (int I = 0; I <= 2; ++I) {
      gnot_config c{};
      c.input_dim = 2; c.theta_dim = 1; c.input_func_dim = 3; c.out_dim = 2; c.n_attn_layers = 1 + I;
      c.n_attn_hidden_dim = c.n_mlp_hidden_dim = c.n_input_hidden_dim = wh[0];
      c.n_mlp_num_layers = 2; c.n_expert = 3; c.n_head = wh[1]; c.n_input_functions = I;
      gnot_plan* p = nullptr;
      CHECK(gnot_plan_create(&c, &p) == GNOT_OK);
      if (!p) continue;
      CHECK(gnot_plan_set_pre_norm(p, 1, 0.f) == GNOT_E_INVALID);
      CHECK(gnot_plan_set_pre_norm(p, 1, -1e-5f) == GNOT_E_INVALID);
      CHECK(gnot_plan_set_pre_norm(p, 1, std::numeric_limits<float>::quiet_NaN()) == GNOT_E_INVALID);
      for (int trial = 0; trial < 4; ++trial) {
        const int B = 1 + (int)(rng() % 5);
        std::vector<int64_t> n(B), m(B);
        for (int b = 0; b < B; ++b) {
          n[b] = (trial == 1 && b == 0 && B > 1) ? 0 : 1 + (int64_t)(rng() % 2000);   // an empty sample once
          m[b] = n[b] ? 1 + (int64_t)(rng() % 300) : 0;
        }
        const auto xo = offsets(n);
        std::vector<int64_t> fo;
        for (int i = 0; i < I; ++i) {
          const auto o = offsets(m);
          fo.insert(fo.end(), o.begin(), o.end());
        }
        for (int tr = 0; tr < 2; ++tr)
          for (int rc = 0; rc < 2; ++rc) {
            CHECK(gnot_plan_set_moe_recompute(p, rc) == GNOT_OK);
            CHECK(gnot_plan_set_pre_norm(p, 0, 1e-5f) == GNOT_OK);
            CHECK(gnot_plan_set_batch(p, B, xo.data(), I ? fo.data() : nullptr, tr) == GNOT_OK);
            const size_t plain = gnot_plan_workspace_bytes(p);
            CHECK(gnot_plan_set_pre_norm(p, 1, 1e-5f) == GNOT_OK);
            CHECK(gnot_plan_workspace_bytes(p) == 0);                  // batch invalidated
            CHECK(gnot_plan_set_batch(p, B, xo.data(), I ? fo.data() : nullptr, tr) == GNOT_OK);
            CHECK(gnot_plan_workspace_bytes(p) > plain);
            CHECK(gnot_plan_set_pre_norm(p, 0, 1e-5f) == GNOT_OK);
            CHECK(gnot_plan_set_batch(p, B, xo.data(), I ? fo.data() : nullptr, tr) == GNOT_OK);
            CHECK(gnot_plan_workspace_bytes(p) == plain);              // on, then off: the plain layout
          }
        // sharded, with the option on
        gnot_comm comm{nullptr, fake_allreduce, fake_alltoallv};
        CHECK(gnot_plan_set_pre_norm(p, 1, 1e-5f) == GNOT_OK);
        for (int r = 0; r < 2; ++r) {
          CHECK(gnot_plan_set_shard(p, r, 2, B, n.data(), &comm) == GNOT_OK);
          std::vector<int64_t> loc(B);
          for (int b = 0; b < B; ++b) {
            int64_t lo, hi;
            CHECK(gnot_shard_range(n[b], r, 2, &lo, &hi) == GNOT_OK);
            loc[b] = hi - lo;
          }
          const auto lo = offsets(loc);
          const int st = gnot_plan_set_batch(p, B, lo.data(), I ? fo.data() : nullptr, 1);
          CHECK(st == GNOT_OK || lo.back() == 0);
        }
        CHECK(gnot_plan_set_shard(p, 0, 1, B, n.data(), nullptr) == GNOT_OK);
      }
      gnot_plan_destroy(p);
    }
  alignas(16) static float buf[8];
  CHECK(gnot_layer_norm(nullptr, 4, 1, 4, 1e-5f, buf, 4, nullptr, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_layer_norm(buf, 4, 0, 4, 1e-5f, buf + 4, 4, nullptr, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_layer_norm(buf, 4, 1, 1025, 1e-5f, buf + 4, 4, nullptr, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_layer_norm(buf, 2, 1, 2, 1e-5f, buf + 4, 4, nullptr, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_layer_norm(buf + 1, 4, 1, 3, 1e-5f, buf + 4, 4, nullptr, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_layer_norm(buf, 4, 1, 4, 0.f, buf + 4, 4, nullptr, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_layer_norm_bwd(buf, 4, nullptr, buf, 4, 1, 4, buf + 4, 4, 0, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_layer_norm_bwd(buf, 4, buf, buf, 4, 1, 4, buf + 4, 6, 0, nullptr) == GNOT_E_INVALID);
}

// dropout (gnot_plan_set_dropout): the option adds one small table (the samples' first points) and no buffer, also
// for a sharded batch with an empty sample; on-then-off restores the plain layout; the launch-time switch leaves
// the batch alone; bad arguments are refused.  (Its own generator, outside the layout digest, as above.)
static void dropout() {
  std::mt19937 rng(4242);
  alignas(16) static uint32_t key[4];
  alignas(16) static float buf[8];
  static int64_t tab[2];
  const int widths[][2] = {{64, 4}, {40, 2}, {256, 8}, {320, 5}};
  for (const auto& wh : widths)
    for (int I = 0; I <= 1; ++I) {
      gnot_config c{};
      c.input_dim = 2; c.theta_dim = 1; c.input_func_dim = 3; c.out_dim = 2; c.n_attn_layers = 1 + I;
      c.n_attn_hidden_dim = c.n_mlp_hidden_dim = c.n_input_hidden_dim = wh[0];
      c.n_mlp_num_layers = 2; c.n_expert = 3; c.n_head = wh[1]; c.n_input_functions = I;
      gnot_plan* p = nullptr;
      CHECK(gnot_plan_create(&c, &p) == GNOT_OK);
      if (!p) continue;
      CHECK(gnot_plan_set_dropout(p, 1.f, key) == GNOT_E_INVALID);
      CHECK(gnot_plan_set_dropout(p, -0.1f, key) == GNOT_E_INVALID);
      CHECK(gnot_plan_set_dropout(p, std::numeric_limits<float>::quiet_NaN(), key) == GNOT_E_INVALID);
      CHECK(gnot_plan_set_dropout(p, 0.25f, nullptr) == GNOT_E_INVALID);
      CHECK(gnot_plan_set_dropout_active(nullptr, 1) == GNOT_E_INVALID);
      for (int trial = 0; trial < 3; ++trial) {
        const int B = 2 + (int)(rng() % 4);
        std::vector<int64_t> n(B), m(B);
        for (int b = 0; b < B; ++b) {
          n[b] = (trial == 1 && b == 1) ? 0 : 1 + (int64_t)(rng() % 2000);   // an empty sample once
          m[b] = n[b] ? 1 + (int64_t)(rng() % 300) : 0;
        }
        const auto xo = offsets(n), fo = offsets(m);
        for (int tr = 0; tr < 2; ++tr) {
          CHECK(gnot_plan_set_dropout(p, 0.f, nullptr) == GNOT_OK);
          CHECK(gnot_plan_set_batch(p, B, xo.data(), I ? fo.data() : nullptr, tr) == GNOT_OK);
          const size_t plain = gnot_plan_workspace_bytes(p);
          CHECK(gnot_plan_set_dropout(p, 0.25f, key) == GNOT_OK);
          CHECK(gnot_plan_workspace_bytes(p) == 0);                  // batch invalidated
          CHECK(gnot_plan_set_batch(p, B, xo.data(), I ? fo.data() : nullptr, tr) == GNOT_OK);
          const size_t on = gnot_plan_workspace_bytes(p);
          CHECK(on >= plain && on <= plain + 256);                   // one table of B offsets, no rows
          CHECK(gnot_plan_set_dropout_active(p, 0) == GNOT_OK);
          CHECK(gnot_plan_workspace_bytes(p) == on);                 // a launch-time switch
          CHECK(gnot_plan_set_dropout(p, 0.f, nullptr) == GNOT_OK);
          CHECK(gnot_plan_set_batch(p, B, xo.data(), I ? fo.data() : nullptr, tr) == GNOT_OK);
          CHECK(gnot_plan_workspace_bytes(p) == plain);              // on, then off: the plain layout
        }
        gnot_comm comm{nullptr, fake_allreduce, fake_alltoallv};
        CHECK(gnot_plan_set_dropout(p, 0.25f, key) == GNOT_OK);
        for (int r = 0; r < 2; ++r) {
          CHECK(gnot_plan_set_shard(p, r, 2, B, n.data(), &comm) == GNOT_OK);
          std::vector<int64_t> loc(B);
          for (int b = 0; b < B; ++b) {
            int64_t lo, hi;
            CHECK(gnot_shard_range(n[b], r, 2, &lo, &hi) == GNOT_OK);
            loc[b] = hi - lo;
          }
          const auto lo = offsets(loc);
          const int st = gnot_plan_set_batch(p, B, lo.data(), I ? fo.data() : nullptr, 1);
          CHECK(st == GNOT_OK || lo.back() == 0);
        }
        CHECK(gnot_plan_set_shard(p, 0, 1, B, n.data(), nullptr) == GNOT_OK);
      }
      gnot_plan_destroy(p);
    }
  CHECK(gnot_dropout_rows(nullptr, 4, 1, 4, tab, tab, 1, key, 0, 0.25f, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_dropout_rows(buf, 4, 0, 4, tab, tab, 1, key, 0, 0.25f, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_dropout_rows(buf, 4, 1, 1025, tab, tab, 1, key, 0, 0.25f, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_dropout_rows(buf, 2, 1, 2, tab, tab, 1, key, 0, 0.25f, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_dropout_rows(buf + 1, 4, 1, 3, tab, tab, 1, key, 0, 0.25f, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_dropout_rows(buf, 4, 1, 4, tab, tab, 0, key, 0, 0.25f, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_dropout_rows(buf, 4, 1, 4, tab, tab, 1, nullptr, 0, 0.25f, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_dropout_rows(buf, 4, 1, 4, tab, tab, 1, key, 1u << 24, 0.25f, nullptr) == GNOT_E_INVALID);
  CHECK(gnot_dropout_rows(buf, 4, 1, 4, tab, tab, 1, key, 0, 1.f, nullptr) == GNOT_E_INVALID);
}

// the shapes of an attention call (inside the layout digest): a cross module without input functions (the fused
// q|k|v form) over two blocks, two input functions, padded heads (d = 100, 4 heads: one weight-gradient job per
// head), and the encoders and block 0 frozen (the batched input-function side runs a suffix of the blocks) --
// each with and without pre-norm and gnot_plan_set_input_grads, on a batch with empty samples, a one-point
// sample and a sample that ends on a 64-point segment edge
static void attn_calls() {
  const std::vector<int64_t> n = {65, 0, 1, 0, 128}, m = {17, 5, 1, 0, 64};
  const auto xo = offsets(n);
  const int models[][4] = {{32, 4, 0, 0}, {32, 4, 2, 0}, {100, 4, 1, 0}, {32, 4, 2, 1}};   // d, H, I, frozen
  for (const auto& md : models) {
    const int I = md[2];
    gnot_config c{};
    c.input_dim = 2; c.theta_dim = 1; c.input_func_dim = 3; c.out_dim = 2; c.n_attn_layers = 2;
    c.n_attn_hidden_dim = c.n_mlp_hidden_dim = c.n_input_hidden_dim = md[0];
    c.n_mlp_num_layers = 2; c.n_expert = 2; c.n_head = md[1]; c.n_input_functions = I;
    gnot_plan* p = nullptr;
    CHECK(gnot_plan_create(&c, &p) == GNOT_OK);
    if (!p) continue;
    std::vector<int64_t> fo;
    for (int i = 0; i < I; ++i) {
      const auto o = offsets(m);
      fo.insert(fo.end(), o.begin(), o.end());
    }
    const int nlin = gnot_plan_num_linears(p), NL = 3, KI = I > 0 ? I : 1;
    std::vector<uint8_t> mask(nlin, 1);
    const int frozen_upto = 2 * NL + I * NL + 6 + 2 * KI + 2 * c.n_expert * NL;   // the encoders and block 0
    for (int k = 0; k < frozen_upto && md[3]; ++k) mask[k] = 0;
    CHECK(gnot_plan_set_trainable(p, md[3] ? mask.data() : nullptr) == GNOT_OK);
    int plain_jobs = -1;
    for (int pn = 0; pn < 2; ++pn)
      for (int ig = 0; ig < 2; ++ig) {
        CHECK(gnot_plan_set_pre_norm(p, pn, 1e-5f) == GNOT_OK);
        CHECK(gnot_plan_set_input_grads(p, ig) == GNOT_OK);
        CHECK(gnot_plan_set_batch(p, (int)n.size(), xo.data(), I ? fo.data() : nullptr, 0) == GNOT_OK);
        CHECK(ws_bytes(p) > 0);
        CHECK(gnot_plan_set_batch(p, (int)n.size(), xo.data(), I ? fo.data() : nullptr, 1) == GNOT_OK);
        CHECK(ws_bytes(p) > 0);
        fold_backward_plan(p);
        int jobs = 0, stage = 0;
        CHECK(gnot_debug_backward_plan(p, &jobs, &stage) == GNOT_OK);
        CHECK(stage == (ig ? -1 : md[3] ? 1 : -1));
        if (plain_jobs < 0) plain_jobs = jobs;
        CHECK(jobs == plain_jobs);             // neither option adds or removes a weight-gradient job
        char forms[512];
        CHECK(gnot_debug_kernel_forms(p, forms, sizeof forms) == GNOT_OK);
      }
    gnot_plan_destroy(p);
  }
}

int main() {
  std::mt19937 rng(12345);
  // {width, heads}: 96 / 192 have head widths 12 / 24; 320 runs chainw.hip, 576 (internal width 640) the
  // K-split tables, 100 (heads of 25) padded heads
  const int widths[][2] = {{16, 4}, {32, 4}, {48, 3}, {64, 8}, {96, 8}, {128, 8}, {144, 3}, {192, 8}, {256, 8},
                           {320, 10}, {576, 9}, {100, 4}};
  for (const auto& wh : widths)
    for (int I = 0; I <= 2; ++I) {
      const int d = wh[0];
      gnot_config c{};
      c.input_dim = 2 + (d & 1);
      c.theta_dim = 1;
      c.input_func_dim = 3;
      c.out_dim = 1 + I;
      c.n_attn_layers = 1 + (d % 3);
      c.n_attn_hidden_dim = c.n_mlp_hidden_dim = c.n_input_hidden_dim = d;
      c.n_mlp_num_layers = 2 + (d % 3);
      c.n_expert = d == 32 ? 2 : d == 48 ? 3 : d == 256 ? 8 : 4;
      c.n_head = wh[1];
      c.n_input_functions = I;
      exercise(c, rng);
    }
  // configuration edges (tests/test_gpu_config_edges.py): one argument at a time away from a base of
  // (in 2, theta 1, fn 3, out 2), L = 1, two-layer MLPs, 2 experts, 1 input function
  auto edge = [](int d, int H) {
    gnot_config c{};
    c.input_dim = 2; c.theta_dim = 1; c.input_func_dim = 3; c.out_dim = 2; c.n_attn_layers = 1;
    c.n_attn_hidden_dim = c.n_mlp_hidden_dim = c.n_input_hidden_dim = d;
    c.n_mlp_num_layers = 2; c.n_expert = 2; c.n_head = H; c.n_input_functions = 1;
    return c;
  };
  const int fams[][2] = {{64, 4}, {256, 8}, {320, 10}};
  for (const auto& f : fams) {
    const int d = f[0], H = f[1];
    for (int nl : {0, 6}) { gnot_config c = edge(d, H); c.n_mlp_num_layers = nl; exercise(c, rng); }
    for (int L : {0, 5}) { gnot_config c = edge(d, H); c.n_attn_layers = L; c.n_mlp_num_layers = 1; exercise(c, rng); }
    { gnot_config c = edge(d, H); c.n_attn_layers = 0; c.n_input_functions = 0; exercise(c, rng); }
    { gnot_config c = edge(d, H); c.theta_dim = 0; exercise(c, rng); }
    for (int E : {1, 16, 17, 64}) { gnot_config c = edge(d, H); c.n_expert = E; exercise(c, rng); }
    for (int I : {3, 8}) { gnot_config c = edge(d, H); c.n_input_functions = I; exercise(c, rng); }
    // the first full-width input / output set (ragged), and every width equal to d
    { gnot_config c = edge(d, H); c.input_dim = 9; c.theta_dim = 8; c.input_func_dim = c.out_dim = 17; exercise(c, rng); }
    { gnot_config c = edge(d, H); c.input_dim = d - 24; c.theta_dim = 24; c.input_func_dim = c.out_dim = d; exercise(c, rng); }
  }
  { gnot_config c = edge(64, 4); c.n_expert = 64; c.n_input_functions = 0; exercise(c, rng); }   // E = d, the cap
  // internal width 640: 2 L = 10 d(fn) segments in launches of 4, 4, 2; 8 input functions on the K-split tables
  { gnot_config c = edge(640, 10); c.n_attn_layers = 5; c.n_mlp_num_layers = 1; c.n_input_functions = 2; exercise(c, rng); }
  { gnot_config c = edge(640, 10); c.n_input_functions = 8; exercise(c, rng); }
  // bad configurations are refused without leaking
  gnot_config bad{};
  bad.input_dim = 2; bad.theta_dim = 1; bad.input_func_dim = 3; bad.out_dim = 1; bad.n_attn_layers = 1;
  bad.n_attn_hidden_dim = 32; bad.n_mlp_num_layers = 2; bad.n_mlp_hidden_dim = 64; bad.n_input_hidden_dim = 32;
  bad.n_expert = 2; bad.n_head = 4;
  gnot_plan* p = nullptr;
  CHECK(gnot_plan_create(&bad, &p) == GNOT_E_INVALID);
  // a negative theta_dim is refused (0 is a width), and so is an input function of width 0 (with no input
  // function the width is unused and 0 is accepted)
  {
    gnot_config c = edge(64, 4);
    c.input_dim = 3; c.theta_dim = -1;
    CHECK(gnot_plan_create(&c, &p) == GNOT_E_INVALID);
    c.theta_dim = 0;
    CHECK(gnot_plan_create(&c, &p) == GNOT_OK);
    gnot_plan_destroy(p);
    c = edge(64, 4);
    c.input_func_dim = 0;
    CHECK(gnot_plan_create(&c, &p) == GNOT_E_INVALID);
    c.n_input_functions = 0;
    CHECK(gnot_plan_create(&c, &p) == GNOT_OK);
    gnot_plan_destroy(p);
  }
  exchange(rng);
  attn_calls();
  pre_norm();
  dropout();
  std::printf("layout digest: %016llx\n", (unsigned long long)g_digest);
  std::printf("asan_plan_check: %s (%d failed checks)\n", g_fail ? "FAILED" : "ok", g_fail);
  return g_fail ? 1 : 0;
}
