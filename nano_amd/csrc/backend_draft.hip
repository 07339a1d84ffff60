// backend_draft.hip -- greedy decode with a draft model (include/nano_mi355x.h): the loop of nano_hip_decode_draft
// over two resident models.  The target's side is backend_lookup.hip's (the device history, the state, the record, verify chunks as
// MODE_VERIFY graphs); the draft's side is the greedy loop's MODE_LOOP steps and batched prefill without outputs; between them runs
// draft.hip's kernel.  The two models' streams are ordered by events; the host waits once per round, for the record.
#include "backend_model.h"

static_assert(DRAFT_REC_WORDS == LOOKUP_REC_WORDS, "the draft loop's record lives in the lookup loop's record buffers");

// the target's scratch of the loop beyond lookup_scratch's: the position source of the draft's catch-up rows and the two events
static int draft_scratch(NanoHipModel *m) {
    if (m->dr.iota) return 0;
    NanoHipModel::Draft s;
    std::vector<uint32_t> iota(m->lk.cap);
    for (uint32_t i = 0; i < m->lk.cap; i++) iota[i] = i;
    const bool ok = hipMalloc(reinterpret_cast<void **>(&s.iota), (size_t)m->lk.cap * 4) == hipSuccess &&
                    hipMemcpy(s.iota, iota.data(), (size_t)m->lk.cap * 4, hipMemcpyHostToDevice) == hipSuccess &&
                    hipEventCreateWithFlags(&s.ev_t, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&s.ev_d, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (s.iota) (void)hipFree(s.iota);
        for (hipEvent_t ev : { s.ev_t, s.ev_d }) if (ev) (void)hipEventDestroy(ev);
        FAIL(NANO_HIP_ENOMEM, "allocating the draft decode buffers failed");
    }
    if (const char *g = getenv("NANO_DRAFT_TIMING")) s.timing = *g && *g != '0';
    if (s.timing) for (hipEvent_t &ev : s.tm) if (hipEventCreate(&ev) != hipSuccess) { (void)hipGetLastError(); s.timing = false; }
    m->dr = s;
    return 0;
}
void draft_free(NanoHipModel *m) {
    if (m->dr.iota) (void)hipFree(m->dr.iota);
    for (hipEvent_t ev : m->dr.tm) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : { m->dr.ev_t, m->dr.ev_d }) if (ev) (void)hipEventDestroy(ev);
    m->dr = NanoHipModel::Draft();
}

static uint32_t seq_limit_of(const NanoHipModel *m) { return m->S < m->rope_rows ? m->S : m->rope_rows; }

// the draft's catch-up: hist[from .. from + rows) at those positions into the draft's slot 0, as nano_hip_prefill's chunks (no outputs)
static int draft_catch_up(NanoHipModel *t, NanoHipModel *d, uint32_t from, uint32_t rows) {
    if (rows == 1) {
        // the one row behind a fully accepted or a plain round: the draft's one-row step without a classifier, a graph replay (an eager
        // one-row chunk is every layer's launches one by one: measured 0.70 ms on Qwen3-0.6B shapes, more than a whole replayed step)
        HIP_TRY(hipMemcpyAsync(d->tokens, t->lk.hist + from, 4, hipMemcpyDeviceToDevice, d->st));
        HIP_TRY(hipMemcpyAsync(d->pos, t->dr.iota + from, 4, hipMemcpyDeviceToDevice, d->st));
        return run_step(d, 1, 1, MODE_NOCLS, from);
    }
    const uint32_t chunk_max = d->pf_chunk;
    for (uint32_t done = 0; done < rows;) {
        uint32_t nb = rows - done < chunk_max ? rows - done : chunk_max;
        const uint32_t to_bucket_end = 64u - (from + done) % 64u;
        if (nb > to_bucket_end) nb = to_bucket_end;
        HIP_TRY(hipMemcpyAsync(d->tokens, t->lk.hist + from + done, nb * 4, hipMemcpyDeviceToDevice, d->st));
        HIP_TRY(hipMemcpyAsync(d->pos, t->dr.iota + from + done, nb * 4, hipMemcpyDeviceToDevice, d->st));
        const bool replay = d->use_graph && nb == chunk_max && chunk_max == 64u;
        HIP_TRY(enqueue_chunk(d, 0, nb, RowWant(), from + done + nb - 1, replay));
        done += nb;
    }
    return 0;
}

// one pass of the loop.  D: max_draft as the target in its current mode runs it; seq_limit: the smaller of the two models' limits;
// dn: positions of the history the draft holds
static int decode_draft_once(NanoHipModel *t, NanoHipModel *d, const uint32_t *history, uint32_t n_history, uint32_t max_new, const NanoHipDraftParams &p,
                             uint32_t D, uint32_t seq_limit, uint32_t dn, uint32_t *out_ids, uint32_t *n_out, NanoHipDraftStats *stats) {
    int rc;
    HIP_TRY(hipSetDevice(t->device));
    if ((rc = step_served(t, false))) return rc;
    if (D >= 1 && (rc = step_served(d, true))) return rc;
    if ((rc = lookup_scratch(t))) return rc;
    if ((rc = draft_scratch(t))) return rc;
    if (D >= 1 && (rc = rows_scratch(t, P_LOGITS | P_AMAX, 0))) return rc;
    const uint32_t slot = 0;
    RowWant verify; verify.kind = RowWant::ARGMAX;
    if (t->kv.paged) {                                                      // every page the loop will enter, up front, in both models
        const uint32_t first = n_history - 1, need = n_history - 2 + max_new;
        if ((rc = kv_ensure(t, &slot, &first, &need, 1))) return rc;
    }
    if (D >= 1 && d->kv.paged) {
        const uint32_t first = dn;
        uint32_t need = n_history - 2 + max_new;
        if (need > seq_limit - 1) need = seq_limit - 1;
        if (first <= need && (rc = kv_ensure(d, &slot, &first, &need, 1))) return rc;
    }
    std::vector<uint32_t> &sh = t->lk.shadow;
    size_t have = 0;
    if (sh.size() <= n_history && (sh.empty() || memcmp(sh.data(), history, sh.size() * 4) == 0)) have = sh.size();
    sh.clear();
    if (have < n_history) HIP_TRY(hipMemcpyAsync(t->lk.hist + have, history + have, (n_history - have) * 4, hipMemcpyHostToDevice, t->st));
    const uint32_t st0[4] = { n_history, max_new, 0u, 0u };
    HIP_TRY(hipMemcpyAsync(t->lk.state, st0, sizeof st0, hipMemcpyHostToDevice, t->st));

    DraftArgs da{};
    da.hist = t->lk.hist; da.cap = t->lk.cap; da.state = t->lk.state; da.record = t->lk.state + 4;
    da.max_draft = D; da.stop_token = p.stop_token; da.seq_limit = seq_limit;
    da.next_tokens = t->tokens; da.next_pos = t->pos; da.trace = t->trace; da.trace_cap = t->trace_cap;
    da.fed = t->tokens; da.ids = d->trace;
    if (D >= 1) { da.d_tokens = d->tokens; da.d_pos = d->pos; da.d_pos0 = d->pos0; }
    volatile const uint32_t *rec = t->lk.h_rec;
    NanoHipDraftStats s{};
    uint32_t n = n_history, left = max_new, nb = 0, rounds = 0;
    bool lost = false, edge = false;
    const bool timing = t->dr.timing;
    for (;;) {
        da.role = DRAFT_ROLE_ACCEPT; da.nb = nb; da.amax = nb > 1 ? t->rb.amax : t->amax; da.dn = dn;
        HIP_TRY(launch_draft_round(da, t->st));
        HIP_TRY(hipMemcpyAsync(t->lk.h_rec, da.record, DRAFT_REC_WORDS * 4, hipMemcpyDeviceToHost, t->st));
        if (timing && nb > 1) HIP_TRY(hipEventRecord(t->dr.tm[3], t->st));
        HIP_TRY(hipStreamSynchronize(t->st));                               // THE wait of the round (the target's stream has waited for the draft's)
        if (timing && nb > 1) {
            for (int i = 0; i < 3; i++) { float ms = 0; if (hipEventElapsedTime(&ms, t->dr.tm[i], t->dr.tm[i + 1]) == hipSuccess) t->dr.ms[i] += ms; else (void)hipGetLastError(); }
            t->dr.timed++;
        }
        if (*reinterpret_cast<volatile uint32_t *>(t->h_err) || *reinterpret_cast<volatile uint32_t *>(d->h_err)) { lost = true; break; }
        const uint32_t emitted = rec[DRAFT_REC_EMITTED], nb_next = rec[DRAFT_REC_NB_NEXT], done = rec[DRAFT_REC_DONE], n_new = rec[DRAFT_REC_N], left_new = rec[DRAFT_REC_LEFT];
        if (n_new != n + emitted || emitted > nb || n_new > seq_limit_of(t) + 1u || left_new + emitted != left || rec[DRAFT_REC_DN] + 1u > n_new ||
            nb_next != (done ? 0u : draft_round_rows(n_new, left_new, D, seq_limit)))
            FAIL(NANO_HIP_ERUNTIME, "draft decode: the round record is not acceptable (emitted %u of %u rows, n %u after %u, next round %u rows, left %u, dn %u, done %u)",
                 emitted, nb, n_new, n, nb_next, left_new, rec[DRAFT_REC_DN], done);
        if (nb > 1) { s.rounds_verify++; s.drafted += nb - 1; s.accepted += rec[DRAFT_REC_ACCEPTED]; }
        else if (nb == 1) s.rounds_plain++;
        s.emitted += emitted;
        n = n_new; left = left_new; dn = rec[DRAFT_REC_DN]; nb = nb_next;
        if (done || (p.max_rounds && rounds == p.max_rounds)) break;
        rounds++;
        if (nb == 1) {
            if ((rc = run_step(t, 1, 1, MODE_ARGMAX, n - 1))) return rc;
            continue;
        }
        // the draft reads the device history: behind the upload once per call (every later append has been waited for by the host)
        if (!edge) { HIP_TRY(hipEventRecord(t->dr.ev_t, t->st)); HIP_TRY(hipStreamWaitEvent(d->st, t->dr.ev_t, 0)); edge = true; }
        const uint32_t behind = n - 1 - dn;
        if (timing) HIP_TRY(hipEventRecord(t->dr.tm[0], d->st));
        if (behind) {
            if ((rc = draft_catch_up(t, d, dn, behind))) return rc;
            da.role = DRAFT_ROLE_BEGIN;                                     // (the chunk used the token and position rows the ACCEPT launch had staged)
            HIP_TRY(launch_draft_round(da, d->st));
            s.draft_rows_fed += behind;
        }
        if (timing) HIP_TRY(hipEventRecord(t->dr.tm[1], d->st));
        for (uint32_t i = 0; i + 1 < nb; i++)
            if ((rc = run_step(d, 1, 1, MODE_LOOP, n - 1 + i, i > 0))) return rc;
        if (timing) HIP_TRY(hipEventRecord(t->dr.tm[2], d->st));
        HIP_TRY(hipEventRecord(t->dr.ev_d, d->st));
        HIP_TRY(hipStreamWaitEvent(t->st, t->dr.ev_d, 0));
        da.role = DRAFT_ROLE_STAGE; da.nb = nb;
        HIP_TRY(launch_draft_round(da, t->st));
        // the full chunk recurs with the same (rows, range bucket): replayed, where the lookup loop replays; the shorter ones at a bucket's end run eagerly
        HIP_TRY(enqueue_chunk(t, slot, nb, verify, n - 2 + nb, t->use_graph && t->lk.graph && nb == D + 1));
    }
    if (lost) { HIP_TRY(hipStreamSynchronize(d->st)); HIP_TRY(hipStreamSynchronize(t->st)); return 0; }
    if (s.emitted) {
        HIP_TRY(hipMemcpyAsync(t->h_amax, t->trace, (size_t)s.emitted * 4, hipMemcpyDeviceToHost, t->st));
        HIP_TRY(hipStreamSynchronize(t->st));
        memcpy(out_ids, t->h_amax, (size_t)s.emitted * 4);
    }
    sh.assign(history, history + n_history);
    sh.insert(sh.end(), out_ids, out_ids + s.emitted);
    *n_out = s.emitted;
    s.draft_held = dn;
    if (stats) *stats = s;
    return 0;
}

// measurement: the summed times of the drafted rounds' three parts since the last query (NANO_DRAFT_TIMING=1), then reset
extern "C" int nano_hip_draft_phase_ms(NanoHipModel *t, double out_ms[3], uint32_t *rounds) {
    if (!t || !out_ms || !rounds) FAIL(NANO_HIP_EINVAL, "null argument");
    for (int i = 0; i < 3; i++) { out_ms[i] = t->dr.ms[i]; t->dr.ms[i] = 0; }
    *rounds = t->dr.timed; t->dr.timed = 0;
    return 0;
}

extern "C" int nano_hip_decode_draft(NanoHipModel *t, NanoHipModel *d, const uint32_t *history, uint32_t n_history, uint32_t max_new,
                                     const NanoHipDraftParams *p, uint32_t *out_ids, uint32_t *n_out, NanoHipDraftStats *stats) {
    if (!t || !d || !history || !p || !out_ids || !n_out) FAIL(NANO_HIP_EINVAL, "null argument");
    if (d == t) FAIL(NANO_HIP_EINVAL, "the draft model is the target itself: a second handle is needed (the two keep separate KV caches)");
    if (d->device != t->device) FAIL(NANO_HIP_EINVAL, "the draft model lives on device %d, the target on device %d", d->device, t->device);
    if (d->d.vocab_size != t->d.vocab_size) FAIL(NANO_HIP_EINVAL, "the draft's vocabulary has %u ids, the target's %u", d->d.vocab_size, t->d.vocab_size);
    if (n_history == 0) FAIL(NANO_HIP_EINVAL, "empty history: the last id of the history is the one fed first");
    if (p->max_draft > LOOKUP_MAX_ROWS - 1) FAIL(NANO_HIP_EINVAL, "max_draft %u beyond %u", p->max_draft, LOOKUP_MAX_ROWS - 1);
    if (strict_serves(d) || exact_serves(d) || d->lora_on) FAIL(NANO_HIP_EINVAL, "the draft model is in strict or exact mode or has LoRA on: it drafts through the fast step only");
    const uint32_t limit = seq_limit_of(t), dlimit = seq_limit_of(d);
    if (p->draft_held > n_history - 1 || p->draft_held > dlimit) FAIL(NANO_HIP_EINVAL, "draft_held %u beyond the history's %u fed positions or the draft's %u", p->draft_held, n_history - 1, dlimit);
    if ((uint64_t)n_history - 1 + max_new > limit) FAIL(NANO_HIP_EINVAL, "positions %u .. %llu exceed max_seq_len %u or the model's RoPE table (%u rows)", n_history - 1,
                                                        (unsigned long long)n_history - 1 + max_new, t->S, t->rope_rows);
    if (max_new > t->trace_cap) FAIL(NANO_HIP_EINVAL, "max_new %u exceeds trace capacity %u", max_new, t->trace_cap);
    for (uint32_t i = 0; i < n_history; i++) if (history[i] >= t->d.vocab_size) FAIL(NANO_HIP_EINVAL, "token %u out of vocabulary", history[i]);
    *n_out = 0;
    if (stats) { *stats = NanoHipDraftStats{}; stats->draft_held = p->draft_held; }
    if (max_new == 0) return 0;
    uint32_t D = (strict_serves(t) || exact_serves(t)) ? 0u : p->max_draft;
    if (D + 1 > t->pf_chunk) D = t->pf_chunk - 1;
    if (D > d->trace_cap) D = d->trace_cap;                                 // (the draft's loop steps leave their ids in its trace)
    const uint32_t seq_limit = limit < dlimit ? limit : dlimit;
    // THE re-issue policy (backend_model.h with_reissue) over two models: a hand-off that gave up in either leaves every later step of
    // the loop on garbage.  The whole call once more, the history uploaded and the draft fed from position 0 again.
    for (int again = 0;; again++) {
        if (again) t->lk.shadow.clear();
        *n_out = 0;
        if (const int rc = decode_draft_once(t, d, history, n_history, max_new, *p, D, seq_limit, again ? 0u : p->draft_held, out_ids, n_out, stats)) return rc;
        const uint32_t ct = dev_err_take(t), cd = dev_err_take(d);
        if (!ct && !cd) return 0;
        const uint32_t code = ct ? ct : cd;
        if (again || (ct && (!t->ho.reissue || ct != NANO_DEVERR_HANDOFF)) || (cd && (!d->ho.reissue || cd != NANO_DEVERR_HANDOFF))) return dev_err_fail(code);
        if (ct) handoff_fallback(t);
        if (cd) handoff_fallback(d);
    }
}
