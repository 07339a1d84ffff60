// backend_topk.hip -- top-k alternatives behind the row statistics (topk.hip): the scratch, the enqueue every entry point shares, what
// they all refuse, and the decode-step entry (nano_hip_forward_topk).  The scoring prefill's form lives in prefill_run (backend.hip),
// the ragged step's in backend_rows.hip.
#include <algorithm>

#include "backend_model.h"

int topk_check(const NanoHipModel *m, uint32_t k, const NanoHipTokenScore *scores_out, const NanoHipTopEntry *top_out) {
    if (k > NANO_TOPK_MAX) FAIL(NANO_HIP_EINVAL, "k = %u exceeds NANO_TOPK_MAX (%u)", k, NANO_TOPK_MAX);
    if (k > m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "k = %u exceeds the vocabulary (%u)", k, m->d.vocab_size);
    if (k ? !top_out : !scores_out) FAIL(NANO_HIP_EINVAL, "null argument");
    return 0;
}

void topk_free(NanoHipModel *m) {
    void *dev[] = { m->tk.part, m->tk.spart, m->tk.targets, m->tk.rows, m->tk.out, m->tk.sc, m->tk.tg };
    for (void *p : dev) if (p) (void)hipFree(p);
    m->tk = NanoHipModel::Topk();
}

// The selection's scratch, on the first call that asks for entries: the tiles' keys, a decode step's own statistics partials, targets and
// records (max(pf_chunk, max_batch) rows: score.part holds pf_chunk), and the call's entries, records and targets (max(max_seq_len, call_rows)
// rows: a ragged step may carry more rows than one sequence has positions; a larger call replaces the three).  All or nothing: a failure
// leaves the model as it was.
int topk_scratch(NanoHipModel *m, size_t call_rows) {
    const size_t V = m->d.vocab_size, nt = score_tiles((uint32_t)V), R = std::max<size_t>(m->pf_chunk, m->maxB);
    if (!m->tk.part) {
        NanoHipModel::Topk t;
        const bool ok = hipMalloc(reinterpret_cast<void **>(&t.part), R * nt * NANO_TOPK_MAX * sizeof(unsigned long long)) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void **>(&t.spart), R * nt * sizeof(ScorePartial)) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void **>(&t.targets), R * 4) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void **>(&t.rows), R * sizeof(NanoHipTokenScore)) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            void *got[] = { t.part, t.spart, t.targets, t.rows };
            for (void *p : got) if (p) (void)hipFree(p);
            FAIL(NANO_HIP_ENOMEM, "hipMalloc of the top-k selection's buffers failed (%zu rows x %zu tiles)", R, nt);
        }
        t.rows_cap = (uint32_t)R;
        m->tk = t;
    }
    if (m->tk.out && call_rows <= m->tk.cap) return 0;
    const size_t cap = std::max<size_t>(m->S, call_rows);
    NanoHipTopEntry *out = nullptr; NanoHipTokenScore *sc = nullptr; uint32_t *tg = nullptr;
    const bool ok = hipMalloc(reinterpret_cast<void **>(&out), cap * NANO_TOPK_MAX * sizeof(NanoHipTopEntry)) == hipSuccess &&
                    hipMalloc(reinterpret_cast<void **>(&sc), cap * sizeof(NanoHipTokenScore)) == hipSuccess &&
                    hipMalloc(reinterpret_cast<void **>(&tg), cap * 4) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        void *got[] = { out, sc, tg };
        for (void *p : got) if (p) (void)hipFree(p);
        if (!m->tk.out) topk_free(m);                                       // the first call: nothing stays behind
        FAIL(NANO_HIP_ENOMEM, "hipMalloc of the top-k entries of a call of %zu rows failed", cap);
    }
    if (m->tk.out) {                                                        // a larger call: work queued on the old buffers first
        HIP_TRY(hipStreamSynchronize(m->st));
        void *old[] = { m->tk.out, m->tk.sc, m->tk.tg };
        for (void *p : old) (void)hipFree(p);
    }
    m->tk.out = out; m->tk.sc = sc; m->tk.tg = tg; m->tk.cap = (uint32_t)cap;
    return 0;
}

hipError_t enqueue_topk_rows(NanoHipModel *m, const float *logits, uint32_t rows, uint32_t k, const NanoHipTokenScore *scores, NanoHipTopEntry *out) {
    if (rows > m->tk.rows_cap) return hipErrorInvalidValue;
    TopkArgs a{};
    a.logits = logits; a.V = m->d.vocab_size; a.ntiles = score_tiles(a.V); a.k = k; a.part = m->tk.part; a.scores = scores; a.out = out;
    return launch_topk_rows(a, rows, m->st);
}

// one attempt of nano_hip_forward_topk: the step as nano_hip_forward_begin queues it with logits wanted (without the copy of the logits),
// the statistics and the selection on its rows of m->logits, the records back, the wait
static int forward_topk_once(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch, const uint32_t *targets, uint32_t k,
                             NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out) {
    int rc;
    if ((rc = kv_ensure_batch(m, pos, batch, 0, false))) return rc;
    uint32_t max_pos = 0;
    if ((rc = stage_batch(m, tokens, pos, batch, false, &max_pos))) return rc;
    if ((rc = run_step(m, batch, 1u, MODE_LOGITS, max_pos))) return rc;
    if (targets) HIP_TRY(hipMemcpyAsync(m->tk.targets, targets, (size_t)batch * 4, hipMemcpyHostToDevice, m->st));
    HIP_TRY(enqueue_score_rows(m, m->logits, batch, targets ? m->tk.targets : nullptr, m->tk.rows, m->tk.spart));
    if (k) {
        HIP_TRY(enqueue_topk_rows(m, m->logits, batch, k, m->tk.rows, m->tk.out));
        HIP_TRY(hipMemcpyAsync(top_out, m->tk.out, (size_t)batch * k * sizeof(NanoHipTopEntry), hipMemcpyDeviceToHost, m->st));
    }
    if (scores_out) HIP_TRY(hipMemcpyAsync(scores_out, m->tk.rows, (size_t)batch * sizeof(NanoHipTokenScore), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    return 0;
}

extern "C" int nano_hip_forward_topk(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                     const uint32_t *targets, uint32_t k, NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null argument");
    int rc;
    if ((rc = topk_check(m, k, scores_out, top_out))) return rc;
    if ((rc = check_batch(m, tokens, pos, batch, 0))) return rc;
    if (targets) for (uint32_t i = 0; i < batch; i++) if (targets[i] >= m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "target %u out of vocabulary", targets[i]);
    HIP_TRY(hipSetDevice(m->device));
    if ((rc = step_served(m, false))) return rc;
    if ((rc = topk_scratch(m, batch))) return rc;
    // (a hand-off that gave up: the same step once more through the plain launches, as nano_hip_forward_end does)
    return with_reissue(m, [&](bool) { return forward_topk_once(m, tokens, pos, batch, targets, k, scores_out, top_out); });
}
