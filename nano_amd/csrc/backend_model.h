// backend_model.h -- the model struct of the C-ABI device backend and what its translation units share.  Internal: nothing here is part
// of the C ABI (include/nano_mi355x.h), and nothing declared here is exported by the library.  The model holds what lasts from call to
// call; what one step is travels as a StepSpec value (step_spec.h, with the graph key built from it), never as fields set around a call.
//   backend.hip          create / destroy / layout, the forward / prefill / greedy entry points, the sticky error word and the re-issue policy
//   backend_step.hip     the argument builders, the fast step, the reference-order step, graphs, run_step, the strict / exact switches
//   backend_kv.hip       where the KV cache's rows are, the paged cache, fork, release, KV images (save / restore)
//   backend_sampler.hip  the device-side sampler's scratch and its four entry points
//   backend_lookup.hip   greedy decode with lookup drafts: the loop, the verify entry
//   backend_lookup_rows.hip   lookup drafts for several sequences: the planner, the loop of ragged verify passes
//   backend_rows.hip     what calls get back per fed row (RowWant: the scratch, the sink, the decode-step entry) and ragged steps
//   backend_probe.hip    measurement, state read-back, the hand-off switches and fault injection
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_fp16.h>
#include "../../include/nano_mi355x.h"
#include "kernels.h"
#include "kv_image.h"
#include "pool_plan.h"
#include "step_spec.h"

using namespace nano;
extern "C" void nano_hip_set_error_(const char *msg);      // backend.hip: the thread's nano_hip_last_error() text

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            char _b[512];                                                                          \
            snprintf(_b, sizeof _b, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            nano_hip_set_error_(_b);                                                               \
            return NANO_HIP_ERUNTIME;                                                              \
        }                                                                                          \
    } while (0)
#define FAIL(code, ...)                                                                            \
    do {                                                                                           \
        char _b[512];                                                                              \
        snprintf(_b, sizeof _b, __VA_ARGS__);                                                      \
        nano_hip_set_error_(_b);                                                                   \
        return (code);                                                                             \
    } while (0)

#pragma GCC visibility push(hidden)

enum { WQ = 0, WK, WV, WO, W1, W2, W3, WCOUNT };
constexpr size_t PF_GRAPH_CAP = 64;                    // prefill-chunk graphs kept per model (keyed by KV slot x range bucket)
constexpr uint32_t STAMP_MAX_LAUNCHES = 512, STAMP_WGS = 2048;
constexpr uint32_t KV_NO_PAGE = 0xffffffffu;           // a page-table entry without a page

struct TensorRef { const void *w = nullptr; const float *s = nullptr; };
struct Sampler;                                        // backend_sampler.hip

struct NanoHipModel {
    NanoModelDesc d{};
    int device = 0, cus = 0;
    uint32_t S = 0, maxB = 0, hd = 0, QD = 0, KD = 0;
    uint32_t Bs = 0;                                      // rows of the per-token scratch (>= maxB: a prefill chunk processes Bs prompt tokens of ONE sequence)
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    bool probe_ext = false;                               // the last step with StepSpec::probe_cls took the classifier kernel's own timestamps (ev0 / ev1), not events around it
    uint8_t *arena = nullptr;
    size_t arena_bytes = 0;
    const float *rms_attn = nullptr, *rms_ffn = nullptr, *rms_final = nullptr;
    const float *q_norm = nullptr, *k_norm = nullptr, *rope_cos = nullptr, *rope_sin = nullptr;
    TensorRef tok, cls;
    std::vector<TensorRef> W[WCOUNT];
    // per-sequence state
    float *x = nullptr, *q = nullptr, *kraw = nullptr, *xba = nullptr, *hb = nullptr, *logits = nullptr;
    float *attn_part = nullptr, *attn_ml = nullptr;       // split-attention partials [B][nsplit][QD], [B][n_head][nsplit][2]
    float *tile_max = nullptr;                            // classifier arg-max partials [B][<=V][2]
    // LoRA (Nano architecture, reference infer.c:434-498).  A module is 8 FP32 tensors in one device buffer; the steps read the module of
    // every KV slot from `desc`.  Either ONE attached module (nano_hip_lora_attach: `at`, in every slot's descriptor) or a table of up to
    // NANO_LORA_TABLE_MAX (nano_hip_lora_table_set / nano_hip_lora_bind: `e`, each slot's descriptor from `bound`); they exclude each
    // other.  lora_on: a module is attached, or the table is not empty, and switched on -- all that the gates and step decisions read.
    float *lora_o1 = nullptr; bool lora_on = false;       // the o branch's addend [Bs][E]
    struct LoraTable {
        struct Entry { float *buf = nullptr; LoraSlotDesc d{}; };   // d.t[]: qa qb ka kb va vb oa ob inside buf, each [L][...]
        Entry at;                                         // the attached module (buf == nullptr: none)
        std::vector<Entry> e;                             // NANO_LORA_TABLE_MAX entries once the first is stored (buf == nullptr: empty)
        std::vector<uint32_t> bound;                      // [maxB] the entry of each slot, or NANO_LORA_NONE (empty without a table)
        LoraSlotDesc *desc = nullptr;                     // device [maxB]: `at` in every slot, or what `bound` says; at an address fixed for the model's life
        uint32_t n = 0, max_rank = 0;                     // table entries stored; the largest rank a descriptor may name (the launches' LDS)
    } lt;
    int8_t *gq = nullptr; float *gxs = nullptr;           // MFMA GEMM path (batch > 8, Q80): quantized activations of all sequences
    uint8_t *q4x = nullptr; size_t q4x_bytes = 0;         // Q4K, 2 .. 64 sequences: the staged activation groups (gemv_q4k_chunk.hip, gemm_q4k.hip)
    float *f32x = nullptr; size_t f32x_floats = 0;        // FP32, 9 .. 64 sequences: the operand-order activations of a GEMM launch (gemm_f32.hip)
    uint32_t f32_min_nb = 9;                              // FP32: sequences per step from which projections go to the MFMA GEMM: max(its own measured minimum, mfma_min_nb)
    uint32_t pf_chunk = 8;                                // prompt tokens per weight read of batched prefill: 64 (Q80; Q4K and FP32 whose per-layer projections the MFMA GEMM takes) | 8
    float *rope_cur = nullptr;                            // RoPE rows of the current positions [B][2][hd/2], staged by the embed kernel
    float *kcache = nullptr, *vcache = nullptr;
    uint32_t *tokens = nullptr, *pos = nullptr, *amax = nullptr, *trace = nullptr, *pos0 = nullptr;
    uint32_t trace_cap = 0, nsplit = 1;                  // nsplit: splits xba still has to be combined from after the LAST enqueued step (1: final)
    uint32_t nsplit_cap = 8;                             // the partial buffers are sized for it (32 beyond 2048 positions)
    // pinned host staging
    uint32_t *h_tokens = nullptr, *h_pos = nullptr, *h_amax = nullptr;
    // what calls get back per fed row (backend_rows.hip: rows_scratch is the one allocator, the rows_* functions the one sink).  Everything
    // here is allocated on the first call whose RowWant needs it: nano_hip_forward / _decode_greedy allocate none of it, nano_hip_prefill the fed
    // tokens and positions only, a model that never asks for k >= 1 neither keys nor entries.
    struct RowScratch {
        // pass buffers: enqueue_step's MODE_SCORE / MODE_VERIFY branches read and write them and chunk graphs hold their addresses, so each is
        // allocated once and never moved.  R = max(pf_chunk, max_batch): a decode step scores max_batch rows
        float *logits = nullptr;                          // [pf_chunk][V] a pass's logits: m->logits holds max_batch rows, not chunk rows
        ScorePartial *part = nullptr;                     // [R][score_tiles(V)] tile partials of the statistics kernel
        uint32_t *targets = nullptr;                      // [R] a pass's targets (a chunk graph reads them here, like m->tokens)
        NanoHipTokenScore *rows = nullptr;                // [R] a pass's records
        uint32_t *amax = nullptr;                         // [max(pf_chunk, LOOKUP_MAX_ROWS)] a pass's row arg-maxes (m->amax holds max_batch rows)
        unsigned long long *keys = nullptr;               // [R][score_tiles(V)][NANO_TOPK_MAX] the tiles' best keys of the selection
        // call buffers: one block of `cap` = max(max_seq_len, rows of the largest call so far) rows of what the calls so far needed (`have`).
        // Only copies and eager launches outside any captured region touch them, so a larger or needier call replaces the block.
        uint8_t *call = nullptr; uint32_t cap = 0, have = 0;
        uint32_t *tok = nullptr, *pos = nullptr, *slot = nullptr;   // the call's fed tokens | positions | KV slots, in the order it feeds them
        uint32_t *tgt = nullptr, *out_amax = nullptr;     // its targets; its row arg-maxes
        NanoHipTokenScore *sc = nullptr;                  // its records
        NanoHipTopEntry *top = nullptr;                   // [cap][NANO_TOPK_MAX] its entries (row i's k entries at i * k)
        uint32_t *pool_map = nullptr;                     // C_POOL: PoolPlan::map of the call (at most 5 words per row)
        float *pool_acc = nullptr, *pool_out = nullptr;   // C_POOL: [max_batch][n_embd] running sums of segments that straddle passes | the call's vectors [n_segs][dim]
    } rb;
    // greedy decode with lookup drafts (backend_lookup.hip), allocated on the first call that needs it
    struct Lookup {
        uint32_t *hist = nullptr; uint32_t cap = 0;       // slot 0's ids on the device (lookup.hip appends to them); cap = max_seq_len + 1 rounded up to 4
        std::vector<uint32_t> shadow;                     // what hist holds, host side: a history that extends it uploads only the new ids
        uint32_t *state = nullptr;                        // LookupArgs::state (4 words), then the step record (LOOKUP_REC_WORDS)
        uint32_t *h_rec = nullptr;                        // pinned: the record of the last step
        bool graph = true;                                // verify chunks of the loop replay a graph per (K, range bucket); NANO_LOOKUP_GRAPH=0: eager
    } lk;
    // lookup drafts for several sequences (backend_lookup_rows.hip), allocated on the first call that needs it
    struct LookupRows {
        uint32_t *hist = nullptr; uint32_t cap = 0;       // [max_batch][cap] one history per KV slot (lookup_rows.hip appends to them); cap as Lookup::cap
        std::vector<std::vector<uint32_t>> shadow;        // [max_batch] what each slot's history holds, host side
        uint32_t *ctl = nullptr;                          // one block: state [max_batch][4] | seq_slot | trace_base | row_start | nb [max_batch] each | records [max_batch][8] | stage [max_batch][16]
        uint32_t *slot = nullptr;                         // [rows of a pass] the next pass's row -> slot map
        uint32_t *tok = nullptr, *pos = nullptr, *amax = nullptr;   // [rows of a pass] strict / exact mode: the round's rows and their arg-maxes (m->tokens / m->pos / m->amax hold the row being fed)
        uint32_t *h_rec = nullptr;                        // pinned: [max_batch][8] the records of the last round
    } lkr;
    // greedy decode with a draft model (backend_draft.hip), on the TARGET, allocated on the first call; the history, the state and the
    // record are lk's
    struct Draft {
        uint32_t *iota = nullptr;                         // [lk.cap] 0, 1, 2, ..: the positions of the draft's catch-up rows are copied from here
        hipEvent_t ev_t = nullptr, ev_d = nullptr;        // the target's stream has the history up | the draft's stream has the round's ids
        // measurement (NANO_DRAFT_TIMING=1, read on the first call; tools/draft_probe.py): events around a drafted round's three parts and their summed times
        bool timing = false;
        hipEvent_t tm[4] = {nullptr, nullptr, nullptr, nullptr};   // draft stream: before the catch-up | before the draft's steps | behind them; target stream: behind ACCEPT
        double ms[3] = {0, 0, 0}; uint32_t timed = 0;     // catch-up | draft steps | stage + chunk + accept, over `timed` drafted rounds
    } dr;
    // ragged steps (nano_hip_step_rows, backend_rows.hip): rows that each carry their own (slot, position)
    struct Rows {
        using Group = RowGroup;                           // (step_spec.h; a call keeps its passes' groups itself: StepSpec::groups)
        float *vraw = nullptr;                            // [Bs][KD] fresh v rows of a pass on the contiguous FP32 cache (the FP16 cache has m->vraw)
    } rows;
    uint32_t *h_err = nullptr, *dev_err = nullptr;        // sticky error word: host-mapped, written by kernels that give up a bounded wait (kernels.h NANO_DEVERR_*)
    float *h_logits = nullptr;
    std::map<uint64_t, hipGraphExec_t> graphs;
    std::vector<uint64_t> pf_graph_keys;                  // prefill-chunk graphs in creation order (bounded: PF_GRAPH_CAP)
    uint64_t weight_bytes_per_step = 0;
    bool use_graph = true;
    uint32_t mfma_min_nb = 9;                             // sequences per step from which Q80 and Q4K projections go to their MFMA GEMMs (NANO_MFMA_MIN_NB: measurement; 65 = never)
    // the in-launch hand-offs of the fused one-sequence launches
    struct Handoff {
        bool fuse_qkv_attn = true;                        // one sequence, Q80 gs 64, Qwen3 head_dim 128: q|k|v projection + attention in one launch; NANO_FUSE_LAUNCHES bit 0
        unsigned long long *hand = nullptr;               // its granule buffer (q_dim + 2 kv_dim entries of {tag, value}; tags are epochs: device_common.h)
        bool fuse_wo_w13 = true;                          // one sequence, Q80 gs 64: Wo + W1|W3 in one launch (x as granules); NANO_FUSE_LAUNCHES bit 1
        unsigned long long *hand2 = nullptr;              // its granule buffer (n_embd entries)
        bool combine_wave = true;                         // Wo behind split attention: the splits' weights made inside each wave (SLAB_CW); NANO_COMBINE_WAVE=0: the table form
        uint32_t *tick = nullptr;                         // device words of the in-launch hand-offs: [0] step counter (the epoch), [1] fault word, [2] abort flag, [3] spare
        uint32_t fallbacks = 0;                           // times a hand-off gave up and the call was re-issued through the plain launches (fusion stays off after the first)
        bool reissue = true;                              // (nano_hip_debug_fault bit 1 clears it: the give-up then surfaces as NANO_HIP_ERUNTIME)
        uint32_t last_dev_err = 0;                        // the code bits of the last give-up (diagnostics)
    } ho;
    std::vector<uint32_t> fw_tokens, fw_pos; uint32_t fw_causal = 0; int fw_logits = 0, fw_argmax = 0;   // the step queued by nano_hip_forward_begin (for its re-issue)
    Sampler *smp = nullptr;                               // device-side sampler scratch (max_batch rows), created on first use
    uint32_t rope_rows = 0;       // rows of the RoPE tables on the device: positions >= rope_rows are rejected
    uint32_t pending_batch = 0;   // sequences of the step queued by nano_hip_forward_begin
    uint32_t kv_half = 0;         // the cache's element format (kernels.h KV_FMT_*).  Opt-in FP16 / FP8 KV cache: rows hold __half / e4m3 bytes, v passes through vraw like k through kraw
    float *vraw = nullptr;        // [Bs][KD] fresh v rows (FP16 / FP8 cache only)
    // paged KV cache (opt-in): kcache / vcache are pools [L][pages][64][KD]; pt = first pool row of every 64-position block
    struct PagedKv {
        bool paged = false;
        uint32_t pages = 0, pt_stride = 0;                // pages in the pool; page-table entries per slot = ceil(S / 64)
        uint32_t *pt = nullptr, *kvrow = nullptr;         // device: [maxB][pt_stride] (KV_NO_PAGE = no page), [Bs] pool row of the step's position
        uint32_t *h_pt = nullptr;                         // pinned host mirror of pt
        std::vector<uint32_t> free_pages;
        std::vector<uint32_t> page_owners;                // slots whose table points at each page (0: free; > 1: shared, read-only until copied on write)
        uint64_t cow_copies = 0;                          // pages copied because a slot was about to write into a page it shared
        std::vector<std::vector<uint32_t>> pt_stage;      // staging copies of page-table rows / copy jobs whose upload may still be queued (backend_kv.hip)
        // row copies between slots / pages (kv_copy.hip): the device job list of the launch being queued, grown on demand
        uint32_t *jobs = nullptr; size_t jobs_cap = 0;    // capacity in 32-bit words
        bool copy_nt = false;                             // NANO_KV_COPY_NT=1: non-temporal stores in the copy kernel (measurement, tools/prefix_probe.py)
    } kv;
    // strict-parity / per-phase mode (strict.hip): eager, one kernel per reference operator, reference summation order
    bool strict = false;
    float *xn = nullptr, *hb2 = nullptr, *att = nullptr;   // normalised x [Bs][E], W3 output [Bs][H], attention scores [Bs][n_head][S]
    nano_hip_phase_fn phase_fn = nullptr; void *phase_env = nullptr;
    // exact mode (exact.hip): strict mode's bits from a step that is captured once per (batch, mode, is_causal[, prefill slot]) and replayed
    bool exact = false;
    std::map<uint64_t, uint32_t> exact_nodes;             // kernel nodes of each exact-mode graph (same keys as `graphs`)
    uint32_t exact_launches = 0;                          // ... of the last enqueued exact step (0: graphs are off, nothing was counted)
    // measurement (stamps build, tools/stamp_probe.py): per-launch, per-workgroup phase stamps of the steps run after nano_hip_stamps_begin
    struct Stamps {
        unsigned long long *buf = nullptr; uint32_t launches = 0; bool on = false;
        std::vector<uint32_t> kinds;
    } stamp;
    // KV images (nano_hip_kv_save / _restore, backend_kv.hip): the transport between the cache and host memory, allocated on the first call
    struct KvImageIo {
        uint8_t *dev = nullptr, *host = nullptr;          // device staging | pinned host memory: two halves of `half` bytes each, a half holds one chunk in image order
        size_t half = 0; uint32_t chunk_blocks = 0;       // bytes of a half = chunk_blocks whole 64-position blocks
        hipStream_t cp = nullptr;                         // the copies between dev and host run here, beside the pack / unpack launches on the model's stream
        hipEvent_t staged[2] = {nullptr, nullptr};        // device half h holds its chunk (save: packed, on the model's stream; restore: copied in, on cp)
        hipEvent_t freed[2] = {nullptr, nullptr};         // ... has been consumed (save: copied out, on cp; restore: unpacked, on the model's stream)
        uint32_t *jobs = nullptr; size_t jobs_cap = 0;    // the device job list of the call being queued (capacity in 32-bit words)
    } kvi;
    uint64_t params_bytes = 0;                            // what create was given: a word of the KV image's model tag (kv_image.h)
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline size_t kv_esz(const NanoHipModel *m) { return kv_fmt_bytes(m->kv_half); }      // bytes of a KV cache element: 4, 2 (FP16) or 1 (FP8)
// bytes of n_weights weights in a format: FP32 | Q80 int8 + one FP32 scale per group | Q4K 160-byte blocks of 256
inline uint64_t weight_bytes(uint32_t quant, uint32_t gs, uint64_t n_weights) {
    return quant == NANO_QUANT_F32 ? 4 * n_weights : quant == NANO_QUANT_Q80 ? n_weights + 4 * (n_weights / gs) : n_weights * 160 / 256;
}

// ---- backend.hip: the sticky error word and the hand-offs' fallback ----
uint32_t dev_err_take(NanoHipModel *m);
int dev_err_fail(uint32_t c);
int dev_err_check(NanoHipModel *m);
void handoff_fallback(NanoHipModel *m);
void drop_graphs(NanoHipModel *m);
int check_batch(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch, uint32_t extra_steps);
// What a call wants of the rows it feeds, built by the extern "C" entry points: nothing, every row's arg-max (verify), or every row's score
// record for targets (null: for its own arg-max) and -- k >= 1 -- its k best entries, or -- POOL, ragged steps only -- one pooled
// final-norm vector per segment (pool.hip; no classifier runs).  Every switch derived from that is answered here.
struct RowWant {
    enum Kind : uint32_t { NONE, ARGMAX, SCORE, POOL } kind = NONE;
    const uint32_t *targets = nullptr; uint32_t k = 0;                      // SCORE: the caller's targets (host), entries per row
    uint32_t *argmax_out = nullptr; NanoHipTokenScore *scores_out = nullptr; NanoHipTopEntry *top_out = nullptr;    // the caller's arrays, caller order
    const NanoHipPoolParams *pool = nullptr; float *pool_out = nullptr;     // POOL: the caller's parameters; its vectors [n_segs][pool_dim]
    uint32_t pool_segs = 0, pool_dim = 0; const PoolPlan *pool_plan = nullptr;   // ... the call's segments, dim resolved (0 -> n_embd), its plan (set by the ragged step)
    static RowWant argmaxes(uint32_t *out) { RowWant w; if (out) { w.kind = ARGMAX; w.argmax_out = out; } return w; }
    static RowWant scores(const uint32_t *targets, uint32_t k, NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out) {
        RowWant w; w.kind = SCORE; w.targets = targets; w.k = k; w.scores_out = scores_out; w.top_out = top_out; return w;
    }
    static RowWant pooled(const NanoHipPoolParams *p, float *out) { RowWant w; w.kind = POOL; w.pool = p; w.pool_out = out; return w; }
    bool use_targets() const { return kind == SCORE && targets; }
    uint32_t mode_row() const { return kind == ARGMAX ? MODE_ARGMAX : kind == SCORE ? MODE_LOGITS : MODE_NOCLS; }     // step mode of a row fed alone
    uint32_t mode_pass() const { return kind == ARGMAX ? MODE_VERIFY : kind == SCORE ? MODE_SCORE : MODE_NOCLS; }     // ... of a pass of several rows
    // KEY_KIND of a chunk graph's key (step_spec.h): 0 plain, 1 scored for targets, 2 scored for the arg-max, 3 verify (different nodes: none replays another's graph)
    uint32_t key_kind() const { return kind == ARGMAX ? 3u : kind == SCORE ? (targets ? 1u : 2u) : 0u; }
    uint32_t need(bool passes) const;                                       // the result buffers of rows_scratch it uses; passes: MODE_SCORE / MODE_VERIFY passes run
                                                                            // (false: every row is left in m->logits / m->amax -- reference-order steps, a decode step)
};
// rows_scratch's buffers: P_* pass buffers (P_STATS: partials, targets, records), C_* parts of the call block (C_FEED: tokens and positions)
enum : uint32_t { P_LOGITS = 1, P_STATS = 2, P_AMAX = 4, P_KEYS = 8, C_FEED = 0x10, C_SLOT = 0x20, C_TGT = 0x40, C_SC = 0x80, C_AMAX = 0x100, C_TOP = 0x200, C_POOL = 0x400, C_ALL = 0x7f0 };
inline uint32_t RowWant::need(bool passes) const {
    if (kind == ARGMAX) return (passes ? P_LOGITS | P_AMAX : 0u) | C_AMAX;
    if (kind == POOL) return C_POOL;
    if (kind != SCORE) return 0u;
    return (passes ? P_LOGITS : 0u) | P_STATS | C_SC | (targets ? C_TGT : 0u) | (k ? P_KEYS | C_TOP : 0u);
}
// ---- backend_rows.hip: the scratch and the sink of the row outputs ----
// what every entry point with a RowWant refuses before anything is queued (m is not null)
int rows_check(const NanoHipModel *m, const RowWant &w);
// THE allocator of RowScratch: the pass buffers of `need` that are not there yet, and a call block that holds need's parts (and those of
// earlier calls) for call_rows rows.  NANO_HIP_ENOMEM leaves the model usable: pass buffers as they were, and -- where the call block had
// to be replaced (wait, free, allocate) -- no call block, so the next call allocates one.
int rows_scratch(NanoHipModel *m, uint32_t need, size_t call_rows);
void rows_free(NanoHipModel *m);
// the selection behind the statistics: `rows` rows of logits (row stride V), their records in scores (queued before) -> out[rows][k]
hipError_t enqueue_topk_rows(NanoHipModel *m, const float *logits, uint32_t rows, uint32_t k, const NanoHipTokenScore *scores, NanoHipTopEntry *out);
// a call of `total` rows begins: room for w.need(passes) | more, and the targets (host, in the order the call feeds its rows) on the device
int rows_begin(NanoHipModel *m, const RowWant &w, bool passes, uint32_t more, size_t total, const uint32_t *targets);
// the call's tokens, positions and (null: none) KV slots, in feeding order, on the device once (pageable sources: the caller keeps them until it has waited)
int rows_feed(NanoHipModel *m, size_t total, const uint32_t *tokens, const uint32_t *pos, const uint32_t *slots);
// a step left rows 0 .. nb - 1 in m->logits / m->amax (a reference-order step of one row, a decode step): their statistics and selection,
// or their arg-maxes, into the call's slots at ..
hipError_t rows_after_step(NanoHipModel *m, const RowWant &w, size_t at, uint32_t nb);
// a MODE_SCORE / MODE_VERIFY pass of nb rows is to run: its targets from the call's; it has run: its records or arg-maxes into the call's
// slots at .., and the selection on its logits before the next pass overwrites them.  POOL (a MODE_NOCLS pass; a reference-order step
// in rows_after_step): the pool launch on the pass's rows in m->x, before the next pass overwrites them
hipError_t rows_pass_targets(NanoHipModel *m, const RowWant &w, size_t at, uint32_t nb);
hipError_t rows_after_pass(NanoHipModel *m, const RowWant &w, size_t at, uint32_t nb);
// strict / exact mode: the call's rows one by one, each a reference-order step on its staged token and position in KV slot row_slot[i] (null: slot)
int rows_run_ordered(NanoHipModel *m, const RowWant &w, size_t total, uint32_t slot, const uint32_t *row_slot);
// the call's results to the caller's arrays and the call's one wait (check: then dev_err_check).  where (null: feeding order is caller
// order, straight into the caller's arrays): caller row r was fed as row where[r]
int rows_back(NanoHipModel *m, const RowWant &w, size_t total, const uint32_t *where, bool check);
// batched prefill of one slot, as nano_hip_prefill / _prefill_score / _prefill_score_topk / _verify_draft call it
int prefill_run(NanoHipModel *m, uint32_t slot, const uint32_t *tokens, uint32_t pos0, uint32_t count, const RowWant &want);
// one prefill chunk of nb rows of `slot` (m->tokens / m->pos hold them; last_pos = the last row's position) of a call that wants `want` of
// its rows, eager or -- replay -- through the bounded cache of chunk graphs
hipError_t enqueue_chunk(NanoHipModel *m, uint32_t slot, uint32_t nb, const RowWant &want, uint32_t last_pos, bool replay);
int lookup_scratch(NanoHipModel *m);                   // backend_lookup.hip
void lookup_free(NanoHipModel *m);
void lookup_rows_free(NanoHipModel *m);                // backend_lookup_rows.hip
// one ragged pass of nb rows (m->tokens / m->pos hold them, row_slot their slots on the device, groups their buckets), eager (backend_rows.hip)
hipError_t enqueue_rows_pass(NanoHipModel *m, uint32_t nb, const RowWant &want, const uint32_t *row_slot, const std::vector<RowGroup> &groups);
void draft_free(NanoHipModel *m);                      // backend_draft.hip
// THE re-issue policy of every entry point that hands results over (round-6 advice: correctness after a give-up depends on every one of
// them re-issuing at the same positions).  attempt(again) queues the call's work and synchronises the stream; an error it returns is
// the call's, without a look at the sticky word.  A hand-off that gave up gets the same work once more (again = true: same tokens,
// same positions, the KV rows are rewritten) through the plain launches: the caller sees the results, not an error.  Any other code, a
// second give-up, or re-issue switched off fails the call.
template <class Attempt>
static int with_reissue(NanoHipModel *m, Attempt attempt) {
    for (int again = 0;; again++) {
        if (const int rc = attempt(again != 0)) return rc;
        const uint32_t code = dev_err_take(m);
        if (!code) return 0;
        if (again || !m->ho.reissue || code != NANO_DEVERR_HANDOFF) return dev_err_fail(code);
        handoff_fallback(m);
    }
}

// ---- backend_kv.hip ----
// The KV rows of one step, built once per enqueue_step / enqueue_step_ordered from the step's spec (of): sequence b lives in KV slot
// `slot` + b, or -- one_slot, batched prefill -- every token is a position of `slot`, or -- ragged -- row b is a position of the slot the
// pass's row map names (slot 0 as the base).  Contiguous cache: [slot][layer][S][kv_dim].  Paged cache: pools
// [layer][page][64][kv_dim], a slot's table names the first pool row of each of its 64-position blocks.  Elements are FP32, or FP16
// (kv_half); the caches are held as float *, so an offset into an FP16 cache goes through at() -- float * arithmetic counts 4-byte units.
struct KvRows {
    const NanoHipModel *m; uint32_t slot; bool one_slot; bool ragged = false;
    static KvRows of(const NanoHipModel *m, const StepSpec &s) { return KvRows{ m, s.ragged() ? 0u : s.slot, s.one_slot(), s.ragged() }; }
    size_t layer_elems() const { return (size_t)m->S * m->KD; }                                   // contiguous: one layer of one slot
    size_t slot_elems() const { return (size_t)m->d.n_layer * layer_elems(); }
    size_t plane_elems() const { return (size_t)m->kv.pages * 64 * m->KD; }                       // paged: one layer plane of the pool
    float *at(float *cache, size_t elems) const { return reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(cache) + elems * kv_esz(m)); }
    // FP32 rows of layer l of `slot`, contiguous layout, and the floats between the step's sequences: the LoRA branch's v / v_bstride on every cache it is let near (step_served())
    float *v_flat(uint32_t l) const { return m->vcache + (size_t)slot * slot_elems() + l * layer_elems(); }
    uint32_t v_flat_bstride() const { return one_slot ? 0u : (uint32_t)slot_elems(); }
    // where the q | k | v launch puts layer l's fresh v row: out + b * bstride + pos[b] * pstride
    struct VTarget { float *out; uint32_t bstride, pstride; const uint32_t *pos; };
    VTarget v_target(uint32_t l) const;
    // the attention launch's K / V bases and the rows between its sequences (the kernel adds the layer itself)
    void attention(AttnArgs &a) const;
    // element offset of the row of (layer, pos) of `slot` in kcache / vcache (nano_hip_read_state); false: paged, and no page holds it yet
    bool row(uint32_t layer, uint32_t pos, size_t *elems) const;
};
int kv_ensure(NanoHipModel *m, const uint32_t *slots, const uint32_t *first, const uint32_t *need, uint32_t n);
int kv_ensure_batch(NanoHipModel *m, const uint32_t *pos, uint32_t batch, uint32_t extra, bool whole_context);
void kv_image_free(NanoHipModel *m);                   // the transport of nano_hip_kv_save / _restore
void sampler_free(Sampler *sp);                        // backend_sampler.hip

// ---- backend_step.hip ----
hipError_t enqueue_classifier(NanoHipModel *m, uint32_t nb, uint32_t *ntiles_out = nullptr, float *dst = nullptr);    // dst: nullptr = m->logits
hipError_t enqueue_score_rows(NanoHipModel *m, const float *logits, uint32_t rows, const uint32_t *targets, NanoHipTokenScore *out);
// the fast step `s` describes, queued eagerly.  It writes nothing into the model but stamp bookkeeping and probe_ext: its caller records
// m->nsplit = xba_nsplit(m, s), whether the step ran here or in a replay
hipError_t enqueue_step(NanoHipModel *m, const StepSpec &s);
bool strict_serves(const NanoHipModel *m);
bool exact_serves(const NanoHipModel *m);
int step_served(const NanoHipModel *m, bool prefill);
// splits nano_hip_read_state still has to combine xba from after step `s` (1: the step leaves it final -- every chunk, ragged pass and
// reference-order step (ordered), and a decode step whose range is not split or whose splits a kernel of its own combines)
uint32_t xba_nsplit(const NanoHipModel *m, const StepSpec &s, bool ordered = false);
// THE graph key of step `s` on this model (step_spec.h); key_kind: RowWant::key_kind of a chunk's call; ordered: the reference-order
// step runs it.  STEP_NO_KEY: run it eagerly
inline uint64_t step_key(const NanoHipModel *m, const StepSpec &s, uint32_t key_kind = 0, bool ordered = false) {
    return step_key(s, ordered, key_kind, m->lora_on, m->stamp.on);
}
int run_step_ordered(NanoHipModel *m, uint32_t nb, uint32_t is_causal, uint32_t mode, uint32_t slot0);
int stage_batch(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch, bool also_pos0, uint32_t *max_pos = nullptr);
uint32_t range_hint_of(const NanoHipModel *m, uint32_t nb, uint32_t is_causal, uint32_t max_pos);
// skip_embed: the greedy loop's steps after the first (StepSpec::skip_embed)
int run_step(NanoHipModel *m, uint32_t nb, uint32_t is_causal, uint32_t mode, uint32_t max_pos, bool skip_embed = false);
// HIP graphs of a step: replay the graph stored under `key`, or -- first use -- run enqueue() eagerly (the launchers set their kernel
// attributes and validate their arguments outside any capture), capture the same enqueue() for the replays to come, instantiate and
// store it.  Reports and leaves the policy to the caller: `step` is the error of the work this call had to queue (the replay or the
// eager run), `capture` that of making the graph (the step itself has run), `stored` / `nodes` a graph made by this call.
// enqueue is a template parameter: a replay pays the map lookup and hipGraphLaunch, nothing for the callable.
struct GraphRun { hipError_t step = hipSuccess, capture = hipSuccess; bool stored = false; uint32_t nodes = 0; };
template <class Enqueue>
static GraphRun graph_step(NanoHipModel *m, uint64_t key, Enqueue enqueue) {
    GraphRun r;
    auto it = m->graphs.find(key);
    if (it != m->graphs.end()) { r.step = hipGraphLaunch(it->second, m->st); return r; }
    if ((r.step = enqueue()) != hipSuccess) return r;
    if ((r.capture = hipStreamBeginCapture(m->st, hipStreamCaptureModeRelaxed)) != hipSuccess) return r;
    hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
    r.capture = enqueue();
    const hipError_t e2 = hipStreamEndCapture(m->st, &g);               // (always: the stream must leave capture mode)
    if (r.capture == hipSuccess) r.capture = e2;
    size_t nodes = 0;
    if (r.capture == hipSuccess) (void)hipGraphGetNodes(g, nullptr, &nodes);
    if (r.capture == hipSuccess) r.capture = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    if (g) (void)hipGraphDestroy(g);
    if (r.capture == hipSuccess) { m->graphs.emplace(key, ge); r.stored = true; r.nodes = (uint32_t)nodes; }
    return r;
}

#pragma GCC visibility pop
