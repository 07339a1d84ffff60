// backend_lookup_rows.hip -- lookup drafts for several sequences (include/nano_mi355x.h nano_hip_decode_lookup_rows, DESIGN.md section
// 10): the device-free planner of a round's pass, the scratch (one device history per KV slot) and the loop.  A round is one ragged
// pass over the live sequences' rows (backend_rows.hip enqueue_rows_pass; strict / exact mode: one reference-order step per live
// sequence) and the two launches of lookup_rows.hip behind it, which run lookup.hip's definitions per sequence and stage the next pass
// on the device.  The host waits once per round for the sequences' 32-byte records.
#include <algorithm>

#include "backend_model.h"

// The host's copy of lookup_rows_pack_kernel: the live sequences (nb_next > 0) ordered stably by the range hint of position n - 1.
extern "C" int nano_hip_lookup_rows_plan(const uint32_t *n, const uint32_t *nb_next, uint32_t n_seqs, uint32_t max_seq_len,
                                         uint32_t *order, uint32_t *row_start, uint32_t *group_hint, uint32_t *group_rows, uint32_t *n_groups) {
    if (n_seqs && (!n || !nb_next)) FAIL(NANO_HIP_EINVAL, "lookup_rows_plan: null argument");
    if (!max_seq_len) FAIL(NANO_HIP_EINVAL, "lookup_rows_plan: max_seq_len must not be 0");
    std::vector<uint32_t> live;
    for (uint32_t i = 0; i < n_seqs; i++) {
        if (!nb_next[i]) continue;
        if (nb_next[i] > LOOKUP_MAX_ROWS) FAIL(NANO_HIP_EINVAL, "lookup_rows_plan: sequence %u: %u rows exceed %u", i, nb_next[i], LOOKUP_MAX_ROWS);
        if (n[i] == 0 || (uint64_t)n[i] - 1 + nb_next[i] > max_seq_len)
            FAIL(NANO_HIP_EINVAL, "lookup_rows_plan: sequence %u: positions %u .. %llu are not inside max_seq_len %u", i, n[i] - 1u, (unsigned long long)n[i] - 1 + nb_next[i], max_seq_len);
        live.push_back(i);
    }
    std::stable_sort(live.begin(), live.end(), [&](uint32_t a, uint32_t b) { return lookup_rows_hint(n[a], max_seq_len) < lookup_rows_hint(n[b], max_seq_len); });
    if (row_start) std::fill(row_start, row_start + n_seqs, LOOKUP_ROW_NONE);
    uint32_t row = 0, groups = 0;
    for (size_t k = 0; k < live.size(); k++) {
        const uint32_t i = live[k], h = lookup_rows_hint(n[i], max_seq_len);
        if (order) order[k] = i;
        if (row_start) row_start[i] = row;
        if (k == 0 || h != lookup_rows_hint(n[live[k - 1]], max_seq_len)) {
            if (group_hint) group_hint[groups] = h;
            if (group_rows) group_rows[groups] = 0;
            groups++;
        }
        if (group_rows) group_rows[groups - 1] += nb_next[i];
        row += nb_next[i];
    }
    if (n_groups) *n_groups = groups;
    return NANO_HIP_OK;
}

void lookup_rows_free(NanoHipModel *m) {
    void *dev[] = { m->lkr.hist, m->lkr.ctl, m->lkr.slot, m->lkr.tok, m->lkr.pos, m->lkr.amax };
    for (void *p : dev) if (p) (void)hipFree(p);
    if (m->lkr.h_rec) (void)hipHostFree(m->lkr.h_rec);
    m->lkr = NanoHipModel::LookupRows();
}

namespace {
// words of LookupRows::ctl per sequence: state, seq_slot, trace_base, row_start, nb, record, stage
constexpr uint32_t CTL_WORDS = LOOKUP_ST_WORDS + 4 + LOOKUP_REC_WORDS + LOOKUP_MAX_ROWS;
// what the host uploads per call: state [B][4] | seq_slot [B] | trace_base [B] | row_start [B] | nb [B], the block's first words
constexpr uint32_t CTL_UP_WORDS = LOOKUP_ST_WORDS + 4;
size_t pass_rows_cap(const NanoHipModel *m) { return std::max<size_t>(m->pf_chunk, m->maxB); }
}  // namespace

// all or nothing: a failure leaves the model as it was
static int lookup_rows_scratch(NanoHipModel *m) {
    if (m->lkr.hist) return 0;
    NanoHipModel::LookupRows s;
    s.cap = (m->S + 1u + 3u) & ~3u;
    const size_t B = m->maxB, R = pass_rows_cap(m);
    auto dm = [](uint32_t **p, size_t words) { return hipMalloc(reinterpret_cast<void **>(p), words * 4) == hipSuccess; };
    const bool ok = dm(&s.hist, B * s.cap) && dm(&s.ctl, B * CTL_WORDS) && dm(&s.slot, R) && dm(&s.tok, R) && dm(&s.pos, R) && dm(&s.amax, R) &&
                    hipHostMalloc(reinterpret_cast<void **>(&s.h_rec), B * LOOKUP_REC_WORDS * 4) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        void *got[] = { s.hist, s.ctl, s.slot, s.tok, s.pos, s.amax };
        for (void *p : got) if (p) (void)hipFree(p);
        if (s.h_rec) (void)hipHostFree(s.h_rec);
        FAIL(NANO_HIP_ENOMEM, "hipMalloc of the lookup decode buffers of %zu slots failed", B);
    }
    s.shadow.resize(B);
    m->lkr = std::move(s);
    return 0;
}

extern "C" int nano_hip_decode_lookup_rows(NanoHipModel *m, const NanoHipLookupSeq *seqs, uint32_t n_seqs, const uint32_t *const *histories,
                                           const NanoHipLookupParams *p, uint32_t *const *out_ids, uint32_t *n_out, NanoHipLookupStats *stats,
                                           uint32_t *rounds) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    if (rounds) *rounds = 0;
    if (n_seqs == 0) return 0;
    if (!seqs || !histories || !p || !out_ids || !n_out) FAIL(NANO_HIP_EINVAL, "null argument");
    if (p->max_draft > LOOKUP_MAX_ROWS - 1) FAIL(NANO_HIP_EINVAL, "max_draft %u beyond %u", p->max_draft, LOOKUP_MAX_ROWS - 1);
    if (p->ngram_max < 1 || p->ngram_max > LOOKUP_MAX_NGRAM || p->ngram_min < 1 || p->ngram_min > p->ngram_max)
        FAIL(NANO_HIP_EINVAL, "ngram_max %u outside 1 .. %u or ngram_min %u outside 1 .. ngram_max", p->ngram_max, LOOKUP_MAX_NGRAM, p->ngram_min);
    const uint32_t limit = m->S < m->rope_rows ? m->S : m->rope_rows;
    uint64_t total_new = 0;
    std::vector<uint32_t> seen;
    for (uint32_t i = 0; i < n_seqs; i++) {
        const NanoHipLookupSeq &q = seqs[i];
        if (q.reserved) FAIL(NANO_HIP_EINVAL, "sequence %u: reserved must be 0", i);
        if (q.slot >= m->maxB) FAIL(NANO_HIP_EINVAL, "sequence %u: slot %u out of range (max_batch %u)", i, q.slot, m->maxB);
        if (!histories[i] || !out_ids[i]) FAIL(NANO_HIP_EINVAL, "sequence %u: null argument", i);
        if (q.n_history == 0) FAIL(NANO_HIP_EINVAL, "sequence %u: empty history: the last id of the history is the one fed first", i);
        if ((uint64_t)q.n_history - 1 + q.max_new > limit)
            FAIL(NANO_HIP_EINVAL, "sequence %u: positions %u .. %llu exceed max_seq_len %u or the model's RoPE table (%u rows)", i, q.n_history - 1,
                 (unsigned long long)q.n_history - 1 + q.max_new, m->S, m->rope_rows);
        for (uint32_t k = 0; k < q.n_history; k++) if (histories[i][k] >= m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "sequence %u: token %u out of vocabulary", i, histories[i][k]);
        seen.push_back(q.slot); total_new += q.max_new;
    }
    std::sort(seen.begin(), seen.end());
    for (uint32_t i = 1; i < n_seqs; i++) if (seen[i] == seen[i - 1]) FAIL(NANO_HIP_EINVAL, "slot %u is named by two sequences", seen[i]);
    if (total_new > m->trace_cap) FAIL(NANO_HIP_EINVAL, "the sum of max_new (%llu) exceeds trace capacity %u", (unsigned long long)total_new, m->trace_cap);
    if (m->lora_on) FAIL(NANO_HIP_EINVAL, "ragged steps are not available with the LoRA side branches (their v branch addresses the cache by a flat stride)");
    if (!m->kv.paged && !nano_hip_rows_addressable(m->d.n_layer, m->S, m->KD, (uint32_t)kv_esz(m)))
        FAIL(NANO_HIP_EINVAL, "the row map cannot address a cache of %u layers x %u positions x %u elements", m->d.n_layer, m->S, m->KD);
    const bool ordered = strict_serves(m) || exact_serves(m);
    const uint32_t chunk = nano_hip_prefill_chunk_tokens(m);
    if (!ordered && n_seqs > chunk) FAIL(NANO_HIP_EINVAL, "%u sequences exceed the %u rows of one pass", n_seqs, chunk);
    for (uint32_t i = 0; i < n_seqs; i++) n_out[i] = 0;
    if (stats) std::fill(stats, stats + n_seqs, NanoHipLookupStats{});
    if (total_new == 0) return 0;
    // fixed for the whole call: a round is always exactly one pass
    const uint32_t D = ordered ? 0u : std::min(p->max_draft, chunk / n_seqs - 1u), K = D + 1;

    int rc;
    HIP_TRY(hipSetDevice(m->device));
    if ((rc = step_served(m, true))) return rc;
    if ((rc = lookup_rows_scratch(m))) return rc;
    if (!ordered && (rc = rows_scratch(m, P_LOGITS | P_AMAX, 0))) return rc;
    if (!ordered && !m->kv_half && !m->kv.paged && !m->rows.vraw && hipMalloc(reinterpret_cast<void **>(&m->rows.vraw), (size_t)m->Bs * m->KD * 4) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(NANO_HIP_ENOMEM, "hipMalloc of the ragged steps' v scratch failed");
    }
    if (m->kv.paged) {                                                      // every page the loop will enter, all or nothing, before anything is queued
        std::vector<uint32_t> slots, first, need;
        for (uint32_t i = 0; i < n_seqs; i++)
            if (seqs[i].max_new) { slots.push_back(seqs[i].slot); first.push_back(seqs[i].n_history - 1); need.push_back(seqs[i].n_history - 2 + seqs[i].max_new); }
        if ((rc = kv_ensure(m, slots.data(), first.data(), need.data(), (uint32_t)slots.size()))) return rc;
    }
    NanoHipModel::LookupRows &lk = m->lkr;
    const size_t B = m->maxB;
    // the histories: only what the device does not hold yet; until the call has succeeded the device copies are not described
    for (uint32_t i = 0; i < n_seqs; i++) {
        if (!seqs[i].max_new) continue;
        std::vector<uint32_t> &sh = lk.shadow[seqs[i].slot];
        const uint32_t nh = seqs[i].n_history;
        size_t have = 0;
        if (sh.size() <= nh && (sh.empty() || memcmp(sh.data(), histories[i], sh.size() * 4) == 0)) have = sh.size();
        sh.clear();
        if (have < nh) HIP_TRY(hipMemcpyAsync(lk.hist + (size_t)seqs[i].slot * lk.cap + have, histories[i] + have, (nh - have) * 4, hipMemcpyHostToDevice, m->st));
    }
    uint32_t *d_state = lk.ctl, *d_slot = d_state + B * LOOKUP_ST_WORDS, *d_base = d_slot + B, *d_start = d_base + B, *d_nb = d_start + B,
             *d_rec = d_nb + B, *d_stage = d_rec + B * LOOKUP_REC_WORDS;
    std::vector<uint32_t> up(B * CTL_UP_WORDS, 0u), base(n_seqs);
    {
        uint32_t at = 0;
        for (uint32_t i = 0; i < n_seqs; i++) {
            uint32_t *st = up.data() + (size_t)i * LOOKUP_ST_WORDS;
            st[LOOKUP_ST_N] = seqs[i].n_history; st[LOOKUP_ST_LEFT] = seqs[i].max_new;
            up[B * LOOKUP_ST_WORDS + i] = seqs[i].slot;
            up[B * (LOOKUP_ST_WORDS + 1) + i] = base[i] = at;
            up[B * (LOOKUP_ST_WORDS + 2) + i] = LOOKUP_ROW_NONE;
            at += seqs[i].max_new;
        }
    }
    HIP_TRY(hipMemcpyAsync(lk.ctl, up.data(), up.size() * 4, hipMemcpyHostToDevice, m->st));   // (a pageable source: staged by the runtime before the call returns)

    LookupRowsArgs la{};
    la.n_seqs = n_seqs; la.hist = lk.hist; la.cap = lk.cap; la.seq_slot = d_slot; la.state = d_state; la.row_start = d_start; la.nb = d_nb;
    la.max_draft = D; la.ngram_max = p->ngram_max; la.ngram_min = p->ngram_min; la.stop_token = p->stop_token; la.seq_limit = limit; la.max_seq_len = m->S;
    la.stage = d_stage; la.record = d_rec; la.trace = m->trace; la.trace_base = d_base; la.trace_cap = m->trace_cap;
    // the fast pass reads m->tokens / m->pos and leaves rb.amax; a reference-order step uses row 0 of m->tokens / m->pos / m->amax, so the round's rows live beside them
    la.fed = la.next_tokens = ordered ? lk.tok : m->tokens; la.next_pos = ordered ? lk.pos : m->pos; la.next_slot = lk.slot;
    la.amax = ordered ? lk.amax : m->rb.amax;
    RowWant verify; verify.kind = RowWant::ARGMAX;                         // (no caller array: the accept reads rb.amax, where the pass leaves the rows' arg-maxes)

    volatile const uint32_t *rec = lk.h_rec;
    std::vector<NanoHipLookupStats> s(n_seqs);
    std::vector<uint32_t> n(n_seqs), nb(n_seqs, 0u), nb_next(n_seqs), order(n_seqs), row_start(n_seqs), g_hint(n_seqs), g_rows(n_seqs);
    std::vector<uint8_t> fin(n_seqs, 0);
    std::vector<RowGroup> groups;
    for (uint32_t i = 0; i < n_seqs; i++) n[i] = seqs[i].n_history;
    uint32_t passes = 0;
    for (;;) {
        HIP_TRY(launch_lookup_rows_round(la, m->st));
        HIP_TRY(hipMemcpyAsync(lk.h_rec, d_rec, (size_t)n_seqs * LOOKUP_REC_WORDS * 4, hipMemcpyDeviceToHost, m->st));
        HIP_TRY(hipStreamSynchronize(m->st));                               // the round's one wait
        if ((rc = dev_err_check(m))) return rc;                             // (no hand-off runs in an eager ragged pass: a set word is an error, not a re-issue)
        bool live = false;
        for (uint32_t i = 0; i < n_seqs; i++) {
            const volatile uint32_t *r = rec + (size_t)i * LOOKUP_REC_WORDS;
            const uint32_t emitted = r[LOOKUP_REC_EMITTED], next = r[LOOKUP_REC_NB_NEXT], done = r[LOOKUP_REC_DONE];
            if (fin[i]) {
                if (emitted || next || !done) FAIL(NANO_HIP_ERUNTIME, "lookup decode: sequence %u had finished and reports emitted %u, next %u, done %u", i, emitted, next, done);
                nb_next[i] = 0;
                continue;
            }
            if (r[LOOKUP_REC_N] != n[i] + emitted || emitted > nb[i] || r[LOOKUP_REC_N] > limit + 1u || (done ? next != 0u : (next != 1u && (next != K || K == 1u))) ||
                s[i].emitted + emitted + r[LOOKUP_REC_LEFT] != seqs[i].max_new)
                FAIL(NANO_HIP_ERUNTIME, "lookup decode: the record of sequence %u is not acceptable (emitted %u of %u rows, n %u after %u, next step %u rows, K %u, left %u, done %u)",
                     i, emitted, nb[i], r[LOOKUP_REC_N], n[i], next, K, r[LOOKUP_REC_LEFT], done);
            if (nb[i] > 1) { s[i].steps_verify++; s[i].drafted += D; s[i].accepted += r[LOOKUP_REC_ACCEPTED]; }
            else if (nb[i] == 1) s[i].steps_plain++;
            s[i].emitted += emitted;
            n[i] = r[LOOKUP_REC_N]; nb[i] = nb_next[i] = next;
            if (done) { fin[i] = 1; nb[i] = 0; } else live = true;
        }
        if (!live || (p->max_steps && passes == p->max_steps)) break;
        passes++;
        uint32_t ng = 0;
        if ((rc = nano_hip_lookup_rows_plan(n.data(), nb_next.data(), n_seqs, m->S, order.data(), row_start.data(), g_hint.data(), g_rows.data(), &ng))) return NANO_HIP_ERUNTIME;
        uint32_t total = 0;
        groups.clear();
        for (uint32_t g = 0; g < ng; g++) { groups.push_back({ total, g_rows[g], g_hint[g] }); total += g_rows[g]; }
        if (!total || total > (ordered ? pass_rows_cap(m) : (size_t)chunk)) FAIL(NANO_HIP_ERUNTIME, "lookup decode: a round of %u rows", total);
        if (ordered) {
            // strict / exact mode: one row per live sequence, a reference-order step in its slot
            for (uint32_t k = 0; k < total; k++) {
                HIP_TRY(hipMemcpyAsync(m->tokens, lk.tok + k, 4, hipMemcpyDeviceToDevice, m->st));
                HIP_TRY(hipMemcpyAsync(m->pos, lk.pos + k, 4, hipMemcpyDeviceToDevice, m->st));
                if ((rc = run_step_ordered(m, 1, 1, MODE_ARGMAX, seqs[order[k]].slot))) return rc;
                HIP_TRY(hipMemcpyAsync(lk.amax + k, m->amax, 4, hipMemcpyDeviceToDevice, m->st));
            }
        } else {
            HIP_TRY(enqueue_rows_pass(m, total, verify, lk.slot, groups));
        }
    }
    // the emitted ids: every sequence's region of the trace, copied out once
    uint32_t hi = 0;
    for (uint32_t i = 0; i < n_seqs; i++) if (s[i].emitted) hi = std::max(hi, base[i] + s[i].emitted);
    if (hi) {
        HIP_TRY(hipMemcpyAsync(m->h_amax, m->trace, (size_t)hi * 4, hipMemcpyDeviceToHost, m->st));
        HIP_TRY(hipStreamSynchronize(m->st));
    }
    for (uint32_t i = 0; i < n_seqs; i++) {
        if (s[i].emitted) memcpy(out_ids[i], m->h_amax + base[i], (size_t)s[i].emitted * 4);
        n_out[i] = s[i].emitted;
        if (stats) stats[i] = s[i];
        if (!seqs[i].max_new) continue;
        std::vector<uint32_t> &sh = lk.shadow[seqs[i].slot];
        sh.assign(histories[i], histories[i] + seqs[i].n_history);
        sh.insert(sh.end(), out_ids[i], out_ids[i] + s[i].emitted);
    }
    if (rounds) *rounds = passes;
    return 0;
}
