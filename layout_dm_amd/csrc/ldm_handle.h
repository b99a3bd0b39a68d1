// Host side of libldm_hip.so, shared declarations: the handle (packed weights, per-lane activation workspaces, staging
// buffers, hipGraph cache, profiling) and the helpers the translation units of the C-ABI share.
//   ldm_engine_plan.h  which engine a configuration runs, its geometry and buffer sizes — or why it is refused (host-pure; ldm_handle::plan)
//   ldm_api.cpp      lifecycle, parity hooks, result packaging, near-tie report, introspection
//   ldm_weight_plan.h  what a checkpoint is to the handle: variant, keys read, the size of every derived buffer — or why it is refused; the
//                      split mode's weight cast (host-pure; ldm_handle::wplan)
//   ldm_weights.cpp  checkpoint upload, fp16 / LDS weight images, parameter tables (ldm_load_weight / ldm_finalize_weights)
//   ldm_denoise.cpp  the launch sequence of one denoiser pass over a chunk, per numerics mode
//   ldm_vb_api.cpp   scoring given layouts: forward noising draw, variational-bound terms (ldm_q_sample / ldm_vb_terms / ldm_vb_step)
//   ldm_loop_plan.h  a sampling call's cut into passes and lanes, its graph key, the timestep range rule (host-pure)
//   ldm_loop.cpp     the hot path: one reverse step, the one-launch loop, the per-lane hipGraph loop (ldm_sample_step / _loop)
#pragma once
#include "../../include/ldm_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "ldm_kernels.h"
#include "ldm_loop_plan.h"
#include "ldm_pack.h"
#include "ldm_weight_plan.h"

using namespace ldm;


#define HIP_OK(h, expr)                                                                        \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) return (h)->fail(-2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                           __FILE__, __LINE__);                                \
  } while (0)


// Entry points run on the handle's device but leave the calling thread's current device as they found it
// (PyTorch tracks its own notion of the current device per thread).
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
    else if (err == hipSuccess) prev = -1;  // nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
// (also drops a stale sticky error of an unrelated earlier runtime call — e.g. the caller's framework probing a host
//  pointer with hipPointerGetAttributes — so that the hipGetLastError() after our launches reports only our own)
#define ON_DEVICE(h)                                                                                    \
  DeviceGuard _dev_guard((h)->device);                                                                  \
  (void)hipGetLastError();                                                                              \
  if (_dev_guard.err != hipSuccess) return (h)->fail(-2, "hipSetDevice(%d) failed: %s", (h)->device,    \
                                                     hipGetErrorString(_dev_guard.err))

struct Raw {  // a checkpoint tensor as loaded, fp32: the device copy the exact engine and the table kernels read, and the host copy the
              // images, padded copies and tables are built from (one pass, one upload per buffer) — kept where this handle's engine builds
              // from it: every vector (biases, norms, schedules), and the matrices of a handle that packs fp16 images from them (fast,
              // hybrid's fused FFN); a split-type handle needs of a matrix only its scale
  float* d = nullptr;
  std::vector<float> host;
  float split_scale = 1.f;   // split-type handles, matrices: ldm_weight_plan.h split_scale of the tensor
  std::vector<int64_t> shape;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

struct LayerW {
  const float *w_in, *b_in, *w_out, *b_out, *w1, *b1, *w2, *b2, *g2, *be2;  // fp32 views
  __half *w_in16, *w_in16lo, *w_out16, *w_out16lo, *w1_16, *w1_16lo, *w2_16, *w2_16lo;
  float s_in = 1.f, s_out = 1.f, s1 = 1.f, s2 = 1.f;  // split mode: 2^-k of each tensor's power-of-two pre-scale (GemmArgs.out_scale)
  void *x3_qkv = nullptr, *x3_ffn1 = nullptr;         // split mode: hi | lo tile images of in_proj / linear1 (kernels_lngemm.hip)
  void* x3_ffn2_slab = nullptr;                      // ... K-slab image of linear2 (the GEMM prologue of the next row-resident launch)
  // r06, fused attention + out_proj (kernels_attnout.hip): in_proj with head-padded output columns (48 tiles, bias [1536]) and
  // out_proj as a k-step image (ldm_pack::pack_x3_kstep_image)
  void *x3_qkv_pad = nullptr, *x3_out_kstep = nullptr;
  void* ffn16_img = nullptr;   // hybrid: the plain-fp16 FFN's chunk image (kernels_attnout.hip FFN; the fast mode's pack_ffn_image_pipelined)
  float* b_in_pad = nullptr;
};

struct ProfEntry {
  std::string name;
  double ms = 0;
  int64_t launches = 0;
  double flops = 0, bytes = 0;
};

struct PendingEvent {
  int entry;
  hipEvent_t a, b;
};

struct GraphEntry {
  GraphKey key;                       // ldm_loop_plan.h
  std::vector<hipGraph_t> graph;      // one per lane
  std::vector<hipGraphExec_t> exec;
  void destroy() {
    for (auto e : exec)
      if (e) (void)hipGraphExecDestroy(e);
    for (auto g : graph)
      if (g) (void)hipGraphDestroy(g);
    exec.clear();
    graph.clear();
  }
};

// The captured loops of a handle, oldest first.  The one place that destroys a cached graph; a caller that drops entries a replay may still
// be executing synchronises the device first (the cache itself never does).
struct GraphCache {
  static constexpr size_t kMaxEntries = 8;
  std::vector<GraphEntry> entries;
  int captures = 0;   // entries inserted since create, one per key whatever its lane count (ldm_dev_graph_cache)
  bool empty() const { return entries.empty(); }
  GraphEntry* find(const GraphKey& key) {
    for (auto& g : entries)
      if (g.key == key) return &g;
    return nullptr;
  }
  GraphEntry* insert(const GraphEntry& e) {
    if (entries.size() >= kMaxEntries) drop(0);   // small LRU-less cache: the oldest goes (no device synchronisation in front of it)
    entries.push_back(e);
    ++captures;
    return &entries.back();
  }
  void drop_all() {
    while (!entries.empty()) drop(entries.size() - 1);
  }
  // the relation edge staging at `old` is about to be freed: no graph that recorded its address may be replayed again
  void drop_where_rel_edges(const void* old) {
    for (size_t i = entries.size(); i-- > 0;)
      if (entries[i].key.rel_edges == old) drop(i);
  }

 private:
  void drop(size_t i) {
    entries[i].destroy();
    entries.erase(entries.begin() + i);
  }
};

// The activations of ONE chunk of layouts on their way through the denoiser.  ldm_create allocates the members the plan counts
// (ldm_engine_plan.h WorkspaceCounts, member for member) and leaves the others nullptr.
struct Workspace {
  float *P = nullptr, *Q = nullptr;   // residual stream, ping-pong [rows, D]
  float* logits = nullptr;            // [chunk * S, Cp]
  float *qkv32 = nullptr, *att32 = nullptr, *h32 = nullptr, *hid32 = nullptr;   // exact (qkv32: split as well)
  __half *a16 = nullptr, *att16 = nullptr, *h16 = nullptr, *hid16 = nullptr, *qkv16 = nullptr;       // fast / split: fp16 (hi) operands
  __half *a16lo = nullptr, *att16lo = nullptr, *h16lo = nullptr, *hid16lo = nullptr;                 // split: their lo halves
  __half *qkvp_hi = nullptr, *qkvp_lo = nullptr;   // split, row-resident: q / k / v as head-padded panels [48][panel_rows][32]
  float2* stats_a = nullptr;          // fast, stack kernel: per-row (mean, rstd) of the raw embedding rows in P
  float* rel_logp = nullptr;          // cond=relation, three-launch step: adjusted log-probabilities (chunk, C, S); allocated by check_relation
};

struct ldm_handle {
  ldm_config cfg{};    // as the caller gave it
  EnginePlan plan;     // what this handle runs: engine structure and options, derived geometry, chunk / lanes (ldm_engine_plan.h)
  int device = 0;
  std::string err;
  int D = 0, F = 0, H = 0, L = 0, T = 0;   // cfg's d_model, d_ff, n_head, n_layer, n_step
  VocabTables vocab{};
  // weights
  std::map<std::string, Raw> raw;
  bool finalized = false;
  WeightPlan wplan;    // what the last ldm_finalize_weights read from the key set: the denoiser variant (ldm_describe names it where it is not
                       // the default), the keys, the derived buffers' sizes (ldm_weight_plan.h)
  std::vector<LayerW> layers;
  float *pos = nullptr, *adaln = nullptr, *sched = nullptr;
  const float *emb = nullptr, *head_g = nullptr, *head_b = nullptr, *head_w = nullptr;
  __half *head_w16 = nullptr, *head_w16lo = nullptr;
  float head_s = 1.f;
  void* x3_head = nullptr;   // RowResident: hi | lo tile image of the vocabulary head (kernels_lngemm.hip)
  std::vector<void*> owned;    // everything hipMalloc'ed by the handle for its lifetime
  std::vector<void*> derived;  // what ldm_finalize_weights derives from the checkpoint (fp16 / split copies, LDS images, parameter
                               // tables): freed and rebuilt when the weights are finalized again (a reload used to leak them)
  int n_cu = 256;              // compute units of the device: the batch quantum of the one-launch loop (one workgroup per layout)
  // Lanes (plan.n_lanes, plan.lane_offset_us): chunks c, c + n_lanes, ... form lane (c % n_lanes); every lane has its own workspace (ws[lane]: what its launches
  // and its captured graph are given), stream and captured graph, and the lanes run CONCURRENTLY, lane l starting
  // l * lane_offset_us late.  Why: the fused kernels alternate HBM-bound phases (row loads / stores, ~30 % of a block) with
  // MFMA-bound phases, and with one kernel on the whole chip every CU hits the memory phase at the same moment (all-CU burst
  // ~4 TB/s, then HBM idles).  Two half-chip kernels out of phase halve each burst (profiles/r02_call2_phase_vs_blocks.txt).
  // The parity hooks and the loop without graphs run every chunk through ws[0].
  std::vector<Workspace> ws;
  std::vector<hipStream_t> lane_stream;
  std::vector<hipEvent_t> lane_done;
  hipEvent_t fork_ev = nullptr;
  // fast-mode (fp16 LDS-DMA GEMM + MFMA attention) layout: K padded to 64, heads padded 58 -> 64 (plan.Dq / HD / Fq)
  struct FastLayer {
    __half *w_in = nullptr, *w_out = nullptr, *w1 = nullptr, *w2 = nullptr;  // head-padded fp16 copies (generic tiled GEMMs)
    void* attn_head_img_ks = nullptr;  // per head: 6 in_proj tiles (k-slot K) + its 2 out-proj slabs (stack kernel)
    void* ffn_img_pipe = nullptr;      // W1 tile i | W2 slab i - 1 per stage: the software-pipelined chunk stream (stack kernel)
    float* b_in = nullptr;
    float* b_out_v = nullptr;  // out_proj bias + W_out b_v (the stack kernel never adds the V bias: softmax rows sum to 1)
  };
  std::vector<FastLayer> fast;
  __half* fast_head = nullptr;
  void* head_img_ks = nullptr;  // vocabulary head as 32-class tile images, K axis in k-slot order (stack kernel)
  // parameter-table LDS images of the loop kernel (ldm_kernels.h StackTables), built by build_loop_tables
  float *tbl_att_static = nullptr, *tbl_att_dyn = nullptr, *tbl_ffn = nullptr, *tbl_head = nullptr;
  // Step-0 logits cache of the one-launch loop (ldm_loop.cpp run_loop_fused, kernels_stack.hip): an unconditional call starts
  // from all-[MASK] layouts, whose first denoiser pass depends on the checkpoint, the first timestep and S alone.  The first
  // ldm_sample_loop call with a new (t_model[0], S) runs that pass once for ONE layout (same kernel, writing the head's tiles
  // in register order) on the caller's stream in front of the real launch; from then on every all-[MASK] layout reads the table.
  // At most kStep0Slots keys, the oldest replaced; every (re)load of a weight drops all of them (plan.step0_cache).
  struct Step0Entry {
    int t = -1, S = 0, slot = 0;
    hipStream_t built_on = nullptr;   // the build is ordered in front of later work of this stream ...
    bool settled = false;             // ... and, once its event has been seen complete, of every stream
  };
  float* step0_tab = nullptr;        // [kStep0Slots][kStackStep0Floats]
  int32_t* step0_tok = nullptr;      // an all-[MASK] row [S] | the build launch's token output [S]
  uint8_t* step0_flags = nullptr;    // [max_batch]: 1 = the layout of the last ldm_sample_loop call took the shortcut
  hipEvent_t step0_ev[kStep0Slots] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<Step0Entry> step0;     // oldest first
  // near-tie report of deterministic decoding (ldm_set_tie_report): flags [tie_steps][max_batch]
  float tie_rel = 0.f, tie_abs = 0.f;
  uint8_t* tie_flags = nullptr;
  int tie_steps = 0;
  // cond staging (handle-owned, fixed addresses) so a captured graph does not depend on caller pointers
  int32_t* st_cond_seq = nullptr;
  uint8_t* st_strong = nullptr;
  float* st_weak = nullptr;
  int32_t* st_inter = nullptr;  // (n_step, max_batch, S) intermediates of a graph-captured loop
  // cond=relation: staging of the caller's graph (fixed addresses)
  int32_t* st_rel_off = nullptr;        // (max_batch + 1)
  int32_t* st_rel_edges = nullptr;      // 3 x st_rel_cap : src | dst | attr
  size_t st_rel_cap = 0;
  float* st_rel_centres = nullptr;      // (4, n_bin)
  int32_t *tok_a = nullptr, *tok_b = nullptr;  // loop state ping-pong (max_batch)
  uint64_t* rng = nullptr;                      // device {seed, first_layout}
  int32_t* vb_err = nullptr;                    // error word of the scoring entry points (ldm_vb_api.cpp), allocated on first use
  // per-layout timesteps (ldm_*_t): the call's host arrays staged on the device, max_batch entries each, allocated on first use
  int32_t* st_t = nullptr;
  uint64_t* st_layout = nullptr;
  std::vector<int32_t> st_t_host;               // pageable copies the uploads read: the caller's arrays are done with at return
  std::vector<uint64_t> st_layout_host;
  // profiling
  bool profiling = false;
  std::vector<ProfEntry> prof;
  std::vector<PendingEvent> pending;
  hipEvent_t loop_a = nullptr, loop_b = nullptr;
  bool loop_timed = false;
  GraphCache graphs;

  int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }

  // `into`: the list that owns the allocation — `owned`, or `derived` (ldm_weights.cpp)
  template <typename Tp>
  int dalloc(Tp** out, size_t count, bool zero = true, std::vector<void*>* into = nullptr) {
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(Tp), 16);
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return fail(-3, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    if (zero) {
      e = hipMemset(p, 0, bytes);
      if (e != hipSuccess) return fail(-3, "hipMemset failed: %s", hipGetErrorString(e));
    }
    (into ? *into : owned).push_back(p);
    *out = reinterpret_cast<Tp*>(p);
    return 0;
  }

  int prof_entry(const char* name) {
    for (size_t i = 0; i < prof.size(); ++i)
      if (prof[i].name == name) return (int)i;
    ProfEntry e;
    e.name = name;
    prof.push_back(e);
    return (int)prof.size() - 1;
  }

  // bracket one launch with events when profiling (never during graph capture)
  struct Scope {
    ldm_handle* h;
    hipStream_t st;
    int entry = -1;
    hipEvent_t a = nullptr, b = nullptr;
    bool ok = false;
    Scope(ldm_handle* h_, hipStream_t st_, const char* name, double flops, double bytes) : h(h_), st(st_) {
      if (!h->profiling) return;
      entry = h->prof_entry(name);
      h->prof[entry].launches += 1;
      h->prof[entry].flops += flops;
      h->prof[entry].bytes += bytes;
      // a failed event call only loses this timing sample (ok stays false); the launch itself is unaffected
      ok = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventRecord(a, st) == hipSuccess;
    }
    ~Scope() {
      if (entry < 0) return;
      if (ok && hipEventRecord(b, st) == hipSuccess) {
        h->pending.push_back({entry, a, b});
        return;
      }
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  };

  void drain_profile() {
    for (auto& pe : pending) {
      float ms = 0;
      if (hipEventSynchronize(pe.b) == hipSuccess && hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess)
        prof[pe.entry].ms += ms;
      (void)hipEventDestroy(pe.a);
      (void)hipEventDestroy(pe.b);
    }
    pending.clear();
  }
};

// ---- shared between the translation units (definitions: see the list at the top)
namespace ldm_host {
std::string& create_error();   // last ldm_create error of this thread (ldm_last_error(NULL))
double gemm_flops(int M, int N, int K);
// d_t: nullptr, or the chunk's Bc per-layout timesteps on the device (t is then not read); -4 where the engine has no per-layout form
int denoise_chunk(ldm_handle* h, Workspace& ws, const int32_t* d_tokens, int t, int Bc, hipStream_t st, bool skip_embed = false,
                  const int32_t* d_t = nullptr);
// h_t (B host timesteps, checked against [0, T)) -> the handle's staging buffer; *d_t = its device address (ldm_api.cpp)
int stage_timesteps(ldm_handle* h, const int32_t* h_t, int B, hipStream_t st, const int32_t** d_t);
// the arguments of the row-resident LayerNorm + GEMM launches on workspace `ws` (ldm_denoise.cpp; also ldm_dev.cpp ldm_dev_lngemm_run)
ldm::LnGemmArgs lngemm_in_proj_args(const ldm_handle* h, const Workspace& ws, const int32_t* d_tokens, int t, int i, int M, bool pre,
                                    const int32_t* d_t = nullptr);
ldm::LnGemmArgs lngemm_linear1_args(const ldm_handle* h, const Workspace& ws, int i, int M);
ldm::LnGemmArgs lngemm_head_args(const ldm_handle* h, const Workspace& ws, int M, bool pre);
// ... and of the fused attention + out_proj (+ FFN) launch of layer i over Bc layouts (also ldm_dev.cpp ldm_dev_attnout_run)
ldm::AttnOutArgs attnout_args(const ldm_handle* h, const Workspace& ws, int i);
// the stack kernel's view of the loaded weights: per-layer images and parameters (AdaLN rows of timestep t, or nullptr: the loop kernel
// reads its tables), the vocabulary head writing to `logits` (or nullptr), the loop kernel's parameter tables
struct StackWeights {
  ldm::FusedLayerSet ls;
  ldm::StackHead head;
  ldm::StackTables tables;
};
StackWeights stack_weights(const ldm_handle* h, int t, float* logits);
void fill_post(ldm_handle* h, ldm::PostArgs& p, const ldm_cond* cond, const ldm_sampler* s, size_t layout_off, int Bc);
int check_ready(ldm_handle* h, int B);
int check_sampler(ldm_handle* h, const ldm_sampler* s);
int check_live_temperature(ldm_handle* h, const ldm_sampler* s);  // step / loop only (ldm_loop.cpp)
int set_rng(ldm_handle* h, uint64_t seed, uint64_t first_layout, hipStream_t st);
void fill_rel(ldm_handle* h, ldm::RelArgs& a, const ldm_relation* rel, size_t layout_off, int Bc);
bool loop_fusable(const ldm_handle* h, const ldm_relation* rel);
}  // namespace ldm_host

