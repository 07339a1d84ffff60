// step_spec.h -- what one step is, as a value, and the key of its HIP graph.  Host C++ with no HIP include (tools/step_key_check.cpp
// compiles it alone).
//   StepSpec   everything that decides which launches enqueue_step / enqueue_step_ordered (backend_step.hip) queue and with which
//              arguments, beyond what is fixed when the model is created or switched (LoRA, strict / exact, stamps, the cache's format).
//              Callers build one per step and pass it down; nothing about the step in progress lives in the model.
//   step_key   THE graph key of a step: named bit fields, a value that does not fit its field is "no key" (the step runs eagerly).
#pragma once
#include <stdint.h>

enum StepMode : uint32_t { MODE_NOCLS = 0, MODE_LOGITS = 1, MODE_ARGMAX = 2, MODE_LOOP = 3,
                           MODE_SCORE = 4,     // a pass that goes on into the classifier for all its rows (-> rb.logits) and the row statistics (-> rb.rows)
                           MODE_VERIFY = 5 };  // a pass whose rows' arg-maxes are wanted (-> rb.amax): the classifier into rb.logits, no statistics

struct RowGroup { uint32_t row0, n, hint; };           // a contiguous run of a ragged pass's rows that share a range hint: one attention launch

struct StepSpec {
    enum Rows : uint32_t { SEQS,                       // row b is KV slot `slot` + b: a decode step (slot 0), a reference-order step (its slot0)
                           CHUNK,                      // the rows are consecutive positions of `slot`: a prefill / scoring / verify chunk
                           RAGGED };                   // row b is a position of slot row_slot[b]; the rows come sorted into `groups`
    uint32_t nb = 0, is_causal = 1, mode = MODE_NOCLS;
    uint32_t range_hint = 0;                           // host-side upper bound of the attended range of every row (RAGGED: the last group's, the largest)
    Rows rows = SEQS;
    uint32_t slot = 0;                                 // (the fast step serves SEQS from slot 0 only: its paged-table base and its key carry no slot)
    const uint32_t *row_slot = nullptr;                // RAGGED: device [nb]
    const RowGroup *groups = nullptr; uint32_t n_groups = 0;    // RAGGED: the caller's storage, alive while the step is queued
    bool skip_embed = false;                           // greedy loop: the previous step's arg-max kernel embedded this step's token (honoured with MODE_LOOP only)
    bool probe_cls = false;                            // record the model's events around the classifier launch (eager steps of the probe)
    bool use_targets = false;                          // MODE_SCORE: statistics for rb.targets (false: for each row's own arg-max)

    static StepSpec seqs(uint32_t nb, uint32_t is_causal, uint32_t mode, uint32_t range_hint, uint32_t slot0 = 0) {
        StepSpec s; s.nb = nb; s.is_causal = is_causal; s.mode = mode; s.range_hint = range_hint; s.slot = slot0; return s;
    }
    static StepSpec chunk(uint32_t slot, uint32_t nb, uint32_t mode, uint32_t range_hint, bool use_targets) {
        StepSpec s = seqs(nb, 1, mode, range_hint, slot); s.rows = CHUNK; s.use_targets = use_targets; return s;
    }
    static StepSpec ragged(uint32_t nb, uint32_t mode, const uint32_t *row_slot, const RowGroup *groups, uint32_t n_groups, bool use_targets) {
        StepSpec s = seqs(nb, 1, mode, n_groups ? groups[n_groups - 1].hint : 0u); s.rows = RAGGED;
        s.row_slot = row_slot; s.groups = groups; s.n_groups = n_groups; s.use_targets = use_targets; return s;
    }
    bool ragged() const { return rows == RAGGED; }
    bool one_slot() const { return rows == CHUNK; }
    // a chunk's or ragged pass's rows each split their attention as their own one-sequence decode step would, and a kernel of its own combines
    bool rows_split_alone() const { return rows != SEQS; }
    bool embeds() const { return !(skip_embed && mode == MODE_LOOP); }
};

// ---- the graph key ----
// Three families that never share a key: the fast decode step, a chunk (under RowWant::key_kind), the reference-order step of exact
// mode.  What each family's nodes depend on beyond the model's creation-time facts and what drop_graphs() guards:
//   fast     stamps, skip_embed (with MODE_LOOP), LoRA, range_hint, nb, is_causal, mode
//   chunk    key_kind, LoRA, slot, range_hint, nb                (mode and the targets switch follow from key_kind)
//   ordered  slot (its slot0), nb, is_causal, mode                (every kernel reads positions from device memory: no hint)
// A ragged pass has no key.  Fields a family does not list stay 0 in its keys.
struct KeyField { uint32_t shift, width; };
constexpr KeyField KEY_NB{0, 8}, KEY_MODE{8, 4}, KEY_CAUSAL{12, 1}, KEY_LORA{13, 1}, KEY_SKIP_EMBED{14, 1}, KEY_STAMPS{15, 1},
                   KEY_SLOT{16, 16}, KEY_HINT{32, 26}, KEY_KIND{58, 2}, KEY_FAMILY{60, 2};
enum StepFamily : uint32_t { FAMILY_FAST = 1, FAMILY_CHUNK = 2, FAMILY_ORDERED = 3 };       // (never 0: no key is 0)
constexpr uint64_t STEP_NO_KEY = 0;

// ordered: the reference-order step serves the model (exact mode).  key_kind: RowWant::key_kind of the call (chunks; else 0).
inline uint64_t step_key(const StepSpec &s, bool ordered, uint32_t key_kind, bool lora_on, bool stamps_on) {
    uint64_t key = 0; bool fits = true;
    auto put = [&](KeyField f, uint64_t v) { if (v >> f.width) fits = false; key |= v << f.shift; };
    if (s.ragged() || (ordered && s.rows != StepSpec::SEQS)) return STEP_NO_KEY;
    put(KEY_NB, s.nb);
    if (ordered) {
        put(KEY_FAMILY, FAMILY_ORDERED); put(KEY_SLOT, s.slot); put(KEY_CAUSAL, s.is_causal); put(KEY_MODE, s.mode);
    } else if (s.rows == StepSpec::CHUNK) {
        put(KEY_FAMILY, FAMILY_CHUNK); put(KEY_KIND, key_kind); put(KEY_LORA, lora_on); put(KEY_SLOT, s.slot); put(KEY_HINT, s.range_hint);
    } else {
        if (s.slot) return STEP_NO_KEY;
        put(KEY_FAMILY, FAMILY_FAST); put(KEY_STAMPS, stamps_on); put(KEY_SKIP_EMBED, !s.embeds()); put(KEY_LORA, lora_on);
        put(KEY_HINT, s.range_hint); put(KEY_CAUSAL, s.is_causal); put(KEY_MODE, s.mode);
    }
    return fits ? key : STEP_NO_KEY;
}
