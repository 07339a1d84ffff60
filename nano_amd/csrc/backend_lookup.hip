// backend_lookup.hip -- greedy decode with lookup drafts (include/nano_mi355x.h): the scratch, the loop of
// nano_hip_decode_lookup and nano_hip_verify_draft.  The between-steps logic is lookup.hip's kernel; a verify chunk is a prefill chunk
// that goes on into the classifier and the arg-max of all its rows (backend_step.hip MODE_VERIFY, backend.hip enqueue_chunk).
#include "backend_model.h"

// the device history (max_seq_len + 1 ids: the call's last emitted id has no position yet), the loop's state and record (a verify chunk's
// logits and arg-maxes are rows_scratch's pass buffers).  All or nothing: a failure leaves the model as it was.
int lookup_scratch(NanoHipModel *m) {
    if (m->lk.hist) return 0;
    NanoHipModel::Lookup s;
    s.cap = (m->S + 1u + 3u) & ~3u;
    const bool ok = hipMalloc(reinterpret_cast<void **>(&s.hist), (size_t)s.cap * 4) == hipSuccess &&
                    hipMalloc(reinterpret_cast<void **>(&s.state), (4 + LOOKUP_REC_WORDS) * 4) == hipSuccess &&
                    hipHostMalloc(reinterpret_cast<void **>(&s.h_rec), LOOKUP_REC_WORDS * 4) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        void *got[] = { s.hist, s.state };
        for (void *p : got) if (p) (void)hipFree(p);
        if (s.h_rec) (void)hipHostFree(s.h_rec);
        FAIL(NANO_HIP_ENOMEM, "hipMalloc of the lookup decode buffers failed");
    }
    if (const char *g = getenv("NANO_LOOKUP_GRAPH")) s.graph = *g && *g != '0';
    m->lk = std::move(s);
    return 0;
}
void lookup_free(NanoHipModel *m) {
    void *dev[] = { m->lk.hist, m->lk.state };
    for (void *p : dev) if (p) (void)hipFree(p);
    if (m->lk.h_rec) (void)hipHostFree(m->lk.h_rec);
    m->lk = NanoHipModel::Lookup();
}

extern "C" int nano_hip_verify_draft(NanoHipModel *m, uint32_t slot, const uint32_t *tokens, uint32_t pos0, uint32_t count,
                                     uint32_t *argmax_out, uint32_t *n_accepted) {
    if (!m || !tokens || !argmax_out || !count) FAIL(NANO_HIP_EINVAL, "null argument or no tokens");
    const int rc = prefill_run(m, slot, tokens, pos0, count, RowWant::argmaxes(argmax_out));
    if (rc) return rc;
    uint32_t a = 0;
    while (a + 1 < count && tokens[a + 1] == argmax_out[a]) a++;
    if (n_accepted) *n_accepted = a;
    return 0;
}

// one pass of the loop: history up, first step staged, then per step: the step and lookup_step_kernel queued, the 32-byte record copied
// back, waited for and checked.  D: max_draft as this model in its current mode runs it.
static int decode_lookup_once(NanoHipModel *m, const uint32_t *history, uint32_t n_history, uint32_t max_new, const NanoHipLookupParams &p, uint32_t D,
                              uint32_t limit, uint32_t *out_ids, uint32_t *n_out, NanoHipLookupStats *stats) {
    int rc;
    HIP_TRY(hipSetDevice(m->device));
    if ((rc = step_served(m, false))) return rc;
    if ((rc = lookup_scratch(m))) return rc;
    if (D >= 1 && (rc = rows_scratch(m, P_LOGITS | P_AMAX, 0))) return rc;
    const uint32_t K = D + 1, slot = 0;
    RowWant verify; verify.kind = RowWant::ARGMAX;                         // what a verify chunk wants of its rows (no caller array: lookup.hip reads rb.amax, where the pass leaves them)
    if (m->kv.paged) {                                                     // every page the loop will enter, up front (a chunk stays inside its first row's block)
        const uint32_t first = n_history - 1, need = n_history - 2 + max_new;
        if ((rc = kv_ensure(m, &slot, &first, &need, 1))) return rc;
    }
    // the history: only what the device does not hold yet (as the sampler's per-slot record of marked ids does)
    std::vector<uint32_t> &sh = m->lk.shadow;
    size_t have = 0;
    if (sh.size() <= n_history && (sh.empty() || memcmp(sh.data(), history, sh.size() * 4) == 0)) have = sh.size();
    sh.clear();                                                             // (until the call has succeeded the device copy is not described)
    if (have < n_history) HIP_TRY(hipMemcpyAsync(m->lk.hist + have, history + have, (n_history - have) * 4, hipMemcpyHostToDevice, m->st));   // (a pageable source: staged by the runtime before the call returns)
    const uint32_t st0[4] = { n_history, max_new, 0u, 0u };
    HIP_TRY(hipMemcpyAsync(m->lk.state, st0, sizeof st0, hipMemcpyHostToDevice, m->st));

    LookupArgs la{};
    la.hist = m->lk.hist; la.cap = m->lk.cap; la.state = m->lk.state; la.record = m->lk.state + 4;
    la.max_draft = D; la.ngram_max = p.ngram_max; la.ngram_min = p.ngram_min; la.stop_token = p.stop_token; la.seq_limit = limit;
    la.next_tokens = m->tokens; la.next_pos = m->pos; la.trace = m->trace; la.trace_cap = m->trace_cap;
    la.fed = m->tokens;
    volatile const uint32_t *rec = m->lk.h_rec;
    NanoHipLookupStats s{};
    uint32_t n = n_history, nb = 0, steps = 0;
    bool lost = false;                                                      // a hand-off gave up: the records are not to be trusted, with_reissue() takes over
    for (;;) {
        la.nb = nb; la.amax = nb > 1 ? m->rb.amax : m->amax;
        HIP_TRY(launch_lookup_step(la, m->st));
        HIP_TRY(hipMemcpyAsync(m->lk.h_rec, la.record, LOOKUP_REC_WORDS * 4, hipMemcpyDeviceToHost, m->st));
        HIP_TRY(hipStreamSynchronize(m->st));
        if (*reinterpret_cast<volatile uint32_t *>(m->h_err)) { lost = true; break; }
        const uint32_t emitted = rec[LOOKUP_REC_EMITTED], nb_next = rec[LOOKUP_REC_NB_NEXT], done = rec[LOOKUP_REC_DONE];
        if (rec[LOOKUP_REC_N] != n + emitted || emitted > nb || rec[LOOKUP_REC_N] > limit + 1u || (done ? nb_next != 0u : (nb_next != 1u && (nb_next != K || K == 1u))) ||
            s.emitted + emitted + rec[LOOKUP_REC_LEFT] != max_new)
            FAIL(NANO_HIP_ERUNTIME, "lookup decode: the step record is not acceptable (emitted %u of %u rows, n %u after %u, next step %u rows, K %u, left %u, done %u)",
                 emitted, nb, rec[LOOKUP_REC_N], n, nb_next, K, rec[LOOKUP_REC_LEFT], done);
        if (nb > 1) { s.steps_verify++; s.drafted += D; s.accepted += rec[LOOKUP_REC_ACCEPTED]; }
        else if (nb == 1) s.steps_plain++;
        s.emitted += emitted;
        n = rec[LOOKUP_REC_N]; nb = nb_next;
        if (done || (p.max_steps && steps == p.max_steps)) break;
        steps++;
        if (nb == 1) {
            if ((rc = run_step(m, 1, 1, MODE_ARGMAX, n - 1))) return rc;   // the fused launches and graphs of a one-row step, as nano_hip_forward's
        } else {
            // verify chunks recur with the same (K, range bucket): replayed (profiles/lookup_decode.txt has the eager form beside it)
            HIP_TRY(enqueue_chunk(m, slot, nb, verify, n - 2 + nb, m->use_graph && m->lk.graph));
        }
    }
    if (lost) { HIP_TRY(hipStreamSynchronize(m->st)); return 0; }
    if (s.emitted) {
        HIP_TRY(hipMemcpyAsync(m->h_amax, m->trace, (size_t)s.emitted * 4, hipMemcpyDeviceToHost, m->st));
        HIP_TRY(hipStreamSynchronize(m->st));
        memcpy(out_ids, m->h_amax, (size_t)s.emitted * 4);
    }
    sh.assign(history, history + n_history);
    sh.insert(sh.end(), out_ids, out_ids + s.emitted);
    *n_out = s.emitted;
    if (stats) *stats = s;
    return 0;
}

extern "C" int nano_hip_decode_lookup(NanoHipModel *m, const uint32_t *history, uint32_t n_history, uint32_t max_new,
                                      const NanoHipLookupParams *p, uint32_t *out_ids, uint32_t *n_out, NanoHipLookupStats *stats) {
    if (!m || !history || !p || !out_ids || !n_out) FAIL(NANO_HIP_EINVAL, "null argument");
    if (n_history == 0) FAIL(NANO_HIP_EINVAL, "empty history: the last id of the history is the one fed first");
    if (p->max_draft > LOOKUP_MAX_ROWS - 1) FAIL(NANO_HIP_EINVAL, "max_draft %u beyond %u", p->max_draft, LOOKUP_MAX_ROWS - 1);
    if (p->ngram_max < 1 || p->ngram_max > LOOKUP_MAX_NGRAM || p->ngram_min < 1 || p->ngram_min > p->ngram_max)
        FAIL(NANO_HIP_EINVAL, "ngram_max %u outside 1 .. %u or ngram_min %u outside 1 .. ngram_max", p->ngram_max, LOOKUP_MAX_NGRAM, p->ngram_min);
    const uint32_t limit = m->S < m->rope_rows ? m->S : m->rope_rows;
    if ((uint64_t)n_history - 1 + max_new > limit) FAIL(NANO_HIP_EINVAL, "positions %u .. %llu exceed max_seq_len %u or the model's RoPE table (%u rows)", n_history - 1,
                                                        (unsigned long long)n_history - 1 + max_new, m->S, m->rope_rows);
    if (max_new > m->trace_cap) FAIL(NANO_HIP_EINVAL, "max_new %u exceeds trace capacity %u", max_new, m->trace_cap);
    for (uint32_t i = 0; i < n_history; i++) if (history[i] >= m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "token %u out of vocabulary", history[i]);
    *n_out = 0;
    if (stats) *stats = NanoHipLookupStats{};
    if (max_new == 0) return 0;
    // strict and exact mode: plain reference-order steps only.  A chunk holds no more rows than the per-token scratch serves per weight read.
    uint32_t D = (strict_serves(m) || exact_serves(m)) ? 0u : p->max_draft;
    if (D + 1 > m->pf_chunk) D = m->pf_chunk - 1;
    // A hand-off that gives up somewhere in the loop leaves every later step of it on garbage: the whole call again (with_reissue).
    return with_reissue(m, [&](bool again) {
        if (again) m->lk.shadow.clear();
        *n_out = 0;
        return decode_lookup_once(m, history, n_history, max_new, *p, D, limit, out_ids, n_out, stats);
    });
}
