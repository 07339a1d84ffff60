// backend_rows.hip -- ragged steps (nano_hip_step_rows): rows that each carry their own (KV slot, position).  The planner that cuts a
// call's rows into passes (device-free, queryable), the host predicate of what the row map can address, and the entry point that stages
// the call once and queues its passes through enqueue_step (backend_step.hip: m->rows).
#include <algorithm>

#include "backend_model.h"

namespace {
// how a call's rows are cut: per row in caller order its pass, its row inside the pass and its range hint
struct RowsPlan {
    std::vector<uint32_t> pass, index, hint;
    uint32_t n_passes = 0;
    size_t rows() const { return pass.size(); }
};
}  // namespace

// Passes fill in caller order up to `cap` rows, so a slot's rows ascend over (pass, position) and no pass is left partly empty but the
// last; inside a pass rows are ordered by range hint, stably: rows of one bucket are contiguous (one attention launch) and a slot's rows
// of one bucket keep their order.  A row's hint is that of its own one-sequence decode step (range_hint_of(m, 1, 1, pos)).  Nothing
// forces a cut: every row of a pass finds the earlier rows of its slot in the cache, whichever passes or buckets they are in (all k / v
// rows of a pass are stored before any of its rows attends).
static int rows_plan(const NanoHipRowSeg *segs, uint32_t n_segs, uint32_t cap, uint32_t S, RowsPlan *out) {
    if (n_segs && !segs) FAIL(NANO_HIP_EINVAL, "null segment list");
    if (!cap || !S) FAIL(NANO_HIP_EINVAL, "rows per pass and max_seq_len must not be 0");
    uint64_t total = 0;
    std::vector<uint32_t> slots(n_segs);
    for (uint32_t i = 0; i < n_segs; i++) {
        const NanoHipRowSeg &s = segs[i];
        if (s.reserved) FAIL(NANO_HIP_EINVAL, "segment %u: reserved must be 0", i);
        if ((uint64_t)s.pos0 + s.count > S) FAIL(NANO_HIP_EINVAL, "segment %u: positions %u..%llu exceed max_seq_len %u", i, s.pos0, (unsigned long long)s.pos0 + s.count, S);
        slots[i] = s.slot; total += s.count;
    }
    std::sort(slots.begin(), slots.end());
    for (uint32_t i = 1; i < n_segs; i++) if (slots[i] == slots[i - 1]) FAIL(NANO_HIP_EINVAL, "slot %u is named by two segments", slots[i]);
    if (total > 0x7fffffffull) FAIL(NANO_HIP_EINVAL, "too many rows");
    RowsPlan p;
    p.pass.resize(total); p.index.resize(total); p.hint.resize(total);
    size_t r = 0;
    for (uint32_t i = 0; i < n_segs; i++)
        for (uint32_t k = 0; k < segs[i].count; k++, r++) {
            const uint32_t pos = segs[i].pos0 + k, h = ((pos + 64u) / 64u) * 64u;
            p.pass[r] = (uint32_t)(r / cap); p.hint[r] = h > S ? S : h;
        }
    p.n_passes = (uint32_t)((total + cap - 1) / cap);
    std::vector<uint32_t> order(cap);
    for (size_t r0 = 0; r0 < total; r0 += cap) {
        const size_t n = std::min<size_t>(cap, total - r0);
        for (size_t k = 0; k < n; k++) order[k] = (uint32_t)k;
        std::stable_sort(order.begin(), order.begin() + n, [&](uint32_t a, uint32_t b) { return p.hint[r0 + a] < p.hint[r0 + b]; });
        for (size_t k = 0; k < n; k++) p.index[r0 + order[k]] = (uint32_t)k;
    }
    *out = std::move(p);
    return 0;
}

extern "C" int nano_hip_rows_plan(const NanoHipRowSeg *segs, uint32_t n_segs, uint32_t cap, uint32_t max_seq_len,
                                  uint32_t *row_pass, uint32_t *row_index, uint32_t *row_hint, uint32_t *n_passes) {
    RowsPlan p;
    if (const int rc = rows_plan(segs, n_segs, cap, max_seq_len, &p)) return rc;
    if (row_pass) std::copy(p.pass.begin(), p.pass.end(), row_pass);
    if (row_index) std::copy(p.index.begin(), p.index.end(), row_index);
    if (row_hint) std::copy(p.hint.begin(), p.hint.end(), row_hint);
    if (n_passes) *n_passes = p.n_passes;
    return NANO_HIP_OK;
}

// What the attention kernel's row map reaches on a contiguous cache [slot][layer][S][kv_dim]: the rows between slots travel as a 32-bit
// count (AttnArgs::cache_bstride_rows; the product with the slot is taken in 64 bits) and a layer of one slot lies behind one buffer
// descriptor (32-bit byte offsets).  The v rows never go through a projection epilogue's position arithmetic (KvRows::v_target).
extern "C" int nano_hip_rows_addressable(uint32_t n_layer, uint32_t max_seq_len, uint32_t kv_dim, uint32_t elem_bytes) {
    if (!n_layer || !max_seq_len || !kv_dim || !elem_bytes) return 0;
    if ((uint64_t)n_layer * max_seq_len > 0xffffffffull) return 0;
    return (uint64_t)max_seq_len * kv_dim * elem_bytes < (1ull << 32) ? 1 : 0;
}

// one ragged pass of nb rows (m->tokens / m->pos hold them, row_slot their slots, groups their buckets): eager, with m->pf for the
// per-row split rule and the combine kernel
static hipError_t enqueue_rows_pass(NanoHipModel *m, uint32_t nb, uint32_t mode, const uint32_t *row_slot) {
    m->pf = true; m->pf_slot = 0; m->rows.on = true; m->rows.row_slot = row_slot;
    const hipError_t e = enqueue_step(m, nb, 1, mode, m->rows.groups.back().hint);
    m->pf = false; m->rows.on = false; m->rows.row_slot = nullptr;
    m->nsplit = 1;                                                     // (as a prefill chunk: xba is left final)
    return e;
}

// A ragged step, as nano_hip_step_rows (argmax_out: every row's arg-max, may be null) and nano_hip_step_rows_score (score: every row's
// record for targets -- null: its own arg-max -- and, k >= 1, its k entries) call it.  A scoring pass is a MODE_SCORE pass: the classifier
// over all its rows into score.logits and the statistics for the pass's targets, staged in pass order; the selection's two launches
// follow eagerly on the same buffers.  Records and entries are gathered to caller order through where[].
static int step_rows_run(NanoHipModel *m, const NanoHipRowSeg *segs, uint32_t n_segs, const uint32_t *tokens, uint32_t *argmax_out,
                         bool score, const uint32_t *targets, uint32_t k, NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    if (score) { if (const int rc = topk_check(m, k, scores_out, top_out)) return rc; }
    if (n_segs == 0) return 0;
    if (!segs) FAIL(NANO_HIP_EINVAL, "null argument");
    const uint32_t cap = nano_hip_prefill_chunk_tokens(m);
    RowsPlan plan;
    if (const int rc = rows_plan(segs, n_segs, cap, m->S, &plan)) return rc;
    const size_t total = plan.rows();
    if (total && !tokens) FAIL(NANO_HIP_EINVAL, "null argument");
    for (uint32_t i = 0; i < n_segs; i++) {
        if (segs[i].slot >= m->maxB) FAIL(NANO_HIP_EINVAL, "segment %u: slot %u out of range (max_batch %u)", i, segs[i].slot, m->maxB);
        if ((uint64_t)segs[i].pos0 + segs[i].count > m->rope_rows) FAIL(NANO_HIP_EINVAL, "segment %u: positions %u..%u exceed the model's RoPE table (%u rows = block_size)", i, segs[i].pos0, segs[i].pos0 + segs[i].count, m->rope_rows);
    }
    for (size_t r = 0; r < total; r++) if (tokens[r] >= m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "token %u out of vocabulary", tokens[r]);
    if (score && targets) for (size_t r = 0; r < total; r++) if (targets[r] >= m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "target %u out of vocabulary", targets[r]);
    if (m->lora_on) FAIL(NANO_HIP_EINVAL, "ragged steps are not available with the LoRA side branches (their v branch addresses the cache by a flat stride)");
    if (!m->kv.paged && !nano_hip_rows_addressable(m->d.n_layer, m->S, m->KD, (uint32_t)kv_esz(m)))
        FAIL(NANO_HIP_EINVAL, "the row map cannot address a cache of %u layers x %u positions x %u elements", m->d.n_layer, m->S, m->KD);
    if (total == 0) return 0;
    HIP_TRY(hipSetDevice(m->device));
    if (const int rc = step_served(m, true)) return rc;
    const bool verify = argmax_out != nullptr, ordered = strict_serves(m) || exact_serves(m);
    if (verify) {
        int rc = score_scratch(m);
        if (!rc) rc = lookup_scratch(m);
        if (rc) return rc;
    }
    if (score) {
        int rc = score_scratch(m);
        if (!rc) rc = topk_scratch(m, total);
        if (rc) return rc;
    }
    if (!ordered && !m->kv_half && !m->kv.paged && !m->rows.vraw && hipMalloc(reinterpret_cast<void **>(&m->rows.vraw), (size_t)m->Bs * m->KD * 4) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(NANO_HIP_ENOMEM, "hipMalloc of the ragged steps' v scratch failed");
    }
    if (total > m->rows.cap) {
        if (m->rows.stage) { HIP_TRY(hipStreamSynchronize(m->st)); (void)hipFree(m->rows.stage); m->rows.stage = nullptr; m->rows.cap = 0; }
        const size_t want = std::max<size_t>(total, (size_t)m->S);
        if (hipMalloc(reinterpret_cast<void **>(&m->rows.stage), want * 16) != hipSuccess) { (void)hipGetLastError(); FAIL(NANO_HIP_ENOMEM, "hipMalloc of the ragged steps' staging buffer failed"); }
        m->rows.cap = (uint32_t)want;
    }
    if (m->kv.paged) {                                                      // every page of every segment, all or nothing, before anything is queued
        std::vector<uint32_t> slots, first, need;
        for (uint32_t i = 0; i < n_segs; i++)
            if (segs[i].count) { slots.push_back(segs[i].slot); first.push_back(segs[i].pos0); need.push_back(segs[i].pos0 + segs[i].count - 1); }
        if (const int rc = kv_ensure(m, slots.data(), first.data(), need.data(), (uint32_t)slots.size())) return rc;
    }
    // the call's rows in pass order: where caller row r went, and its token, position and slot there -- on the device ONCE
    std::vector<uint32_t> pass_start(plan.n_passes + 1, 0u), where(total), stage(3 * total), tstage(score && targets ? total : 0);
    for (size_t r = 0; r < total; r++) pass_start[plan.pass[r] + 1]++;
    for (uint32_t p = 0; p < plan.n_passes; p++) pass_start[p + 1] += pass_start[p];
    {
        size_t r = 0;
        for (uint32_t i = 0; i < n_segs; i++)
            for (uint32_t j = 0; j < segs[i].count; j++, r++) {
                const size_t w = where[r] = pass_start[plan.pass[r]] + plan.index[r];
                stage[w] = tokens[r]; stage[total + w] = segs[i].pos0 + j; stage[2 * total + w] = segs[i].slot;
                if (!tstage.empty()) tstage[w] = targets[r];
            }
    }
    uint32_t *const d_tok = m->rows.stage, *const d_pos = d_tok + m->rows.cap, *const d_slot = d_pos + m->rows.cap, *const d_amax = d_slot + m->rows.cap;
    HIP_TRY(hipMemcpyAsync(d_tok, stage.data(), total * 4, hipMemcpyHostToDevice, m->st));
    HIP_TRY(hipMemcpyAsync(d_pos, stage.data() + total, total * 4, hipMemcpyHostToDevice, m->st));
    HIP_TRY(hipMemcpyAsync(d_slot, stage.data() + 2 * total, total * 4, hipMemcpyHostToDevice, m->st));
    const uint32_t *const d_tgt = tstage.empty() ? nullptr : m->tk.tg;       // the call's targets, pass order
    if (d_tgt) HIP_TRY(hipMemcpyAsync(m->tk.tg, tstage.data(), total * 4, hipMemcpyHostToDevice, m->st));
    if (score) m->score.use_targets = d_tgt != nullptr;
    if (ordered) {
        // strict / exact mode: one pass = one row (cap 1, so pass order is caller order): a reference-order step in the row's slot
        const uint32_t mode1 = verify ? MODE_ARGMAX : score ? MODE_LOGITS : MODE_NOCLS;
        for (size_t w = 0; w < total; w++) {
            HIP_TRY(hipMemcpyAsync(m->tokens, d_tok + w, 4, hipMemcpyDeviceToDevice, m->st));
            HIP_TRY(hipMemcpyAsync(m->pos, d_pos + w, 4, hipMemcpyDeviceToDevice, m->st));
            if (const int rc = run_step_ordered(m, 1, 1, mode1, stage[2 * total + w])) return rc;
            if (verify) HIP_TRY(hipMemcpyAsync(d_amax + w, m->amax, 4, hipMemcpyDeviceToDevice, m->st));
            if (score) {                                                   // the row's logits are row 0 of m->logits, as in prefill_run
                HIP_TRY(enqueue_score_rows(m, m->logits, 1, d_tgt ? d_tgt + w : nullptr, m->tk.sc + w));
                if (k) HIP_TRY(enqueue_topk_rows(m, m->logits, 1, k, m->tk.sc + w, m->tk.out + w * k));
            }
        }
    } else {
        for (uint32_t p = 0; p < plan.n_passes; p++) {
            const size_t w0 = pass_start[p];
            const uint32_t nb = pass_start[p + 1] - pass_start[p];
            HIP_TRY(hipMemcpyAsync(m->tokens, d_tok + w0, nb * 4, hipMemcpyDeviceToDevice, m->st));
            HIP_TRY(hipMemcpyAsync(m->pos, d_pos + w0, nb * 4, hipMemcpyDeviceToDevice, m->st));
            m->rows.groups.clear();
            for (uint32_t j = 0; j < nb; j++) {                            // (sorted by hint: a group is a run of equal hints)
                const uint32_t pos = stage[total + w0 + j], h = range_hint_of(m, 1, 1, pos);
                if (m->rows.groups.empty() || m->rows.groups.back().hint != h) m->rows.groups.push_back({j, 1u, h});
                else m->rows.groups.back().n++;
            }
            if (d_tgt) HIP_TRY(hipMemcpyAsync(m->score.targets, d_tgt + w0, nb * 4, hipMemcpyDeviceToDevice, m->st));
            HIP_TRY(enqueue_rows_pass(m, nb, verify ? MODE_VERIFY : score ? MODE_SCORE : MODE_NOCLS, d_slot + w0));
            if (verify) HIP_TRY(hipMemcpyAsync(d_amax + w0, m->lk.amax, nb * 4, hipMemcpyDeviceToDevice, m->st));
            if (score) {
                HIP_TRY(hipMemcpyAsync(m->tk.sc + w0, m->score.rows, nb * sizeof(NanoHipTokenScore), hipMemcpyDeviceToDevice, m->st));
                if (k) HIP_TRY(enqueue_topk_rows(m, m->score.logits, nb, k, m->score.rows, m->tk.out + w0 * k));
            }
        }
    }
    std::vector<uint32_t> amax(verify ? total : 0);
    std::vector<NanoHipTokenScore> sc(score && scores_out ? total : 0);
    std::vector<NanoHipTopEntry> top(score ? total * k : 0);
    if (verify) HIP_TRY(hipMemcpyAsync(amax.data(), d_amax, total * 4, hipMemcpyDeviceToHost, m->st));
    if (!sc.empty()) HIP_TRY(hipMemcpyAsync(sc.data(), m->tk.sc, total * sizeof(NanoHipTokenScore), hipMemcpyDeviceToHost, m->st));
    if (!top.empty()) HIP_TRY(hipMemcpyAsync(top.data(), m->tk.out, total * k * sizeof(NanoHipTopEntry), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));                                   // the call's one wait
    if (const int rc = dev_err_check(m)) return rc;
    for (size_t r = 0; r < (verify ? total : 0); r++) argmax_out[r] = amax[where[r]];
    for (size_t r = 0; r < (sc.empty() ? 0 : total); r++) scores_out[r] = sc[where[r]];
    for (size_t r = 0; r < (top.empty() ? 0 : total); r++) std::copy(top.begin() + where[r] * k, top.begin() + (where[r] + 1) * k, top_out + r * k);
    return 0;
}

extern "C" int nano_hip_step_rows(NanoHipModel *m, const NanoHipRowSeg *segs, uint32_t n_segs, const uint32_t *tokens, uint32_t *argmax_out) {
    return step_rows_run(m, segs, n_segs, tokens, argmax_out, false, nullptr, 0, nullptr, nullptr);
}
extern "C" int nano_hip_step_rows_score(NanoHipModel *m, const NanoHipRowSeg *segs, uint32_t n_segs, const uint32_t *tokens,
                                        const uint32_t *targets, uint32_t k, NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out) {
    return step_rows_run(m, segs, n_segs, tokens, nullptr, true, targets, k, scores_out, top_out);
}
