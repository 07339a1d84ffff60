// backend_sampler.hip -- the device-side sampler (sampler.hip, sampler_wide.hip): its scratch, the mask table and the sample entry points.
#include "backend_model.h"
#include <algorithm>
#include <cmath>

// device-side sampler (sampler.hip): max_batch rows of scratch at a fixed stride + pinned staging + the host's record of every
// row's `seen` set, created on first use
struct Sampler {
    uint8_t *block = nullptr;                             // [maxB] rows (y, e, seen, approx, spec, fn, cells, pmax, bins, cand) + results + params|ids
    SampleRows b{};
    SampleRowParams *params = nullptr, *h_params = nullptr;   // the rows' parameters, then their new history ids (byte offsets from
                                                              // row 0's seen plane): one upload per call
    NanoHipSample *h_res = nullptr;
    uint8_t *wide = nullptr; void *wide_temp = nullptr; size_t wide_temp_bytes = 0;      // second phase, shared by the rows one after another
    SampleArgs wide_a{};                                  // its buffers
    // per slot: ids already marked in that row's `seen`, in history order.  A one-row call is slot 0 of a batch of one, so slot 0's
    // record serves one-row and batched calls alike; that is sound because a record is only used as a prefix of the incoming history
    // (anything else starts the set over), whichever call wrote it.
    std::vector<std::vector<uint32_t>> applied;
    // logit edits (nano_mi355x.h "logit edits").  The mask table: n_masks x W words on the device, replaced as a whole.  The staging of
    // per-call masks and bias lists, created by the first call that carries an edit: one device and one pinned block that hold the rows'
    // parameters and new history ids as before and the call's masks and lists behind them, so that all of it still goes up in one copy;
    // `params` / `h_params` point into these from then on (the first blocks keep the scratch and the results).
    uint32_t *mask_tab = nullptr; uint32_t n_masks = 0;
    uint8_t *edit_dev = nullptr, *edit_host = nullptr;
    uint8_t *h_block = nullptr;                           // the first pinned block (params, ids, results): what sampler_free releases
};

void sampler_free(Sampler *sp) {
    if (!sp) return;
    if (sp->block) (void)hipFree(sp->block);
    if (sp->wide) (void)hipFree(sp->wide);
    if (sp->h_block) (void)hipHostFree(sp->h_block);         // (one pinned block: params, ids, results)
    if (sp->mask_tab) (void)hipFree(sp->mask_tab);
    if (sp->edit_dev) (void)hipFree(sp->edit_dev);
    if (sp->edit_host) (void)hipHostFree(sp->edit_host);
    delete sp;
}

// ---- device-side sampling (reference infer.c:1156-1189) ------------------------------------------------
// Slots 0 .. batch-1 of one decode step, each with its own parameters and history; a one-row call is a batch of one.  Every row has
// its own scratch at a fixed stride (about 1.5 MB at V = 151 936); the six kernels run once for all rows (sampler.hip
// launch_sample_rows).  Rows at temperature 0 take the penalised arg-max over their `y` row; rows whose nucleus does not fit the LDS
// sorter go through the wide phase one after another, on one shared scratch.
static int sampler_init(NanoHipModel *m) {
    if (m->smp) return 0;
    const uint32_t V = m->d.vocab_size, R = m->maxB;
    const uint32_t nch = (((V + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK) + 3u) & ~3u;
    if (nch > SAMPLE_MAX_CHUNKS) FAIL(NANO_HIP_EINVAL, "vocabulary %u too large for the device sampler (max %u)", V, SAMPLE_MAX_CHUNKS * SAMPLE_CHUNK);
    const size_t npad = (size_t)nch * SAMPLE_CHUNK;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_y = take(npad * 4), o_e = take(npad * 4), o_seen = take(npad), o_approx = take(nch * 4), o_spec = take(nch * 4),
                 o_fn = take(nch * 8), o_cells = take(256), o_pmax = take(nch), o_bins = take(SAMPLE_BINS * 12), o_cand = take((size_t)SAMPLE_MAX_CANDIDATES * 8);
    const size_t rstride = off;
    // the seen_set kernel marks byte offsets from row 0's seen plane: every row's plane must lie below 4 GiB of it
    if ((uint64_t)rstride * R >= (1ull << 32)) FAIL(NANO_HIP_EINVAL, "sampler scratch of %u rows exceeds 4 GiB", R);
    off = rstride * R;
    // params[batch] and behind them at most batch * (max_seq_len + 1) new history ids, uploaded together
    const size_t up_bytes = (size_t)R * sizeof(SampleRowParams) + (size_t)R * (m->S + 1) * 4;
    const size_t o_res = take((size_t)R * sizeof(NanoHipSample)), o_up = take(up_bytes);
    const size_t h_res = align_up(up_bytes, 256);
    Sampler *sp = new Sampler();
    uint8_t *hb = nullptr;
    if (hipMalloc(&sp->block, off) != hipSuccess || hipMemset(sp->block, 0, off) != hipSuccess ||
        hipHostMalloc((void **)&hb, h_res + (size_t)R * sizeof(NanoHipSample)) != hipSuccess) {
        sp->h_block = hb;
        sampler_free(sp);
        (void)hipGetLastError();                                            // (the model stays usable)
        FAIL(NANO_HIP_ENOMEM, "sampler scratch allocation failed (%zu bytes for %u rows)", off, R);
    }
    uint8_t *b = sp->block;
    SampleArgs &a = sp->b.a;
    a.V = V; a.nch = nch;
    a.y = (float *)(b + o_y); a.e = (float *)(b + o_e); a.seen = b + o_seen;
    a.approx = (float *)(b + o_approx); a.spec = (uint32_t *)(b + o_spec); a.fn = (uint2 *)(b + o_fn);
    uint32_t *cells = (uint32_t *)(b + o_cells);
    a.ncand = cells + 1; a.sum = (float *)(cells + 2); a.ndrop = cells + 3; a.dropmax = cells + 4; a.bstar = cells + 5;
    a.pmax = (float *)(b + o_pmax);
    a.bin_mass = (unsigned long long *)(b + o_bins); a.bin_cnt = (uint32_t *)(b + o_bins + SAMPLE_BINS * 8);
    a.cand = (unsigned long long *)(b + o_cand); a.cap = SAMPLE_MAX_CANDIDATES; a.res = (NanoHipSample *)(b + o_res);
    sp->b.rstride = rstride; sp->b.lstride = V;
    sp->params = (SampleRowParams *)(b + o_up); sp->b.rp = sp->params;
    sp->h_block = hb; sp->h_params = (SampleRowParams *)hb; sp->h_res = (NanoHipSample *)(hb + h_res);
    sp->applied.assign(R, {});
    m->smp = sp;
    return 0;
}
static inline uint32_t mask_words(uint32_t V) { return (V + 31u) / 32u; }
// does a mask allow any token below V?  (bits of tokens >= V in the last word do not count)
static bool mask_allows_any(const uint32_t *w, uint32_t V) {
    const uint32_t W = mask_words(V);
    for (uint32_t j = 0; j + 1 < W; j++) if (w[j]) return true;
    return (w[W - 1] & (V % 32u ? (1u << (V % 32u)) - 1u : 0xffffffffu)) != 0;
}
static inline bool row_edited(const NanoHipSampleParamsEdit &e) { return e.allow || e.mask_id || e.n_bias; }
// the checks of a row's edit
static int check_row_edit(NanoHipModel *m, uint32_t i, const NanoHipSampleParamsEdit &e) {
    const uint32_t V = m->d.vocab_size;
    if (e.allow && e.mask_id) FAIL(NANO_HIP_EINVAL, "row %u gives both a mask (allow) and a mask_id", i);
    if (e.mask_id > (m->smp ? m->smp->n_masks : 0u)) FAIL(NANO_HIP_EINVAL, "mask_id %u of row %u beyond the mask table (%u masks)", e.mask_id, i, m->smp ? m->smp->n_masks : 0u);
    if (e.allow && !mask_allows_any(e.allow, V)) FAIL(NANO_HIP_EINVAL, "the mask of row %u allows no token", i);
    if (e.n_bias > NANO_BIAS_MAX) FAIL(NANO_HIP_EINVAL, "n_bias %u of row %u exceeds NANO_BIAS_MAX (%u)", e.n_bias, i, NANO_BIAS_MAX);
    if (e.n_bias && !e.bias) FAIL(NANO_HIP_EINVAL, "null bias list of row %u", i);
    uint32_t tok[NANO_BIAS_MAX];
    for (uint32_t k = 0; k < e.n_bias; k++) {
        const float bv = e.bias[k].bias;
        if (e.bias[k].token >= V) FAIL(NANO_HIP_EINVAL, "bias token %u of row %u out of vocabulary", e.bias[k].token, i);
        if (std::isnan(bv) || (std::isinf(bv) && bv > 0.0f)) FAIL(NANO_HIP_EINVAL, "bias of token %u of row %u is NaN or +inf", e.bias[k].token, i);
        tok[k] = e.bias[k].token;
    }
    std::sort(tok, tok + e.n_bias);
    for (uint32_t k = 1; k < e.n_bias; k++) if (tok[k] == tok[k - 1]) FAIL(NANO_HIP_EINVAL, "bias token %u of row %u is listed twice", tok[k], i);
    return 0;
}
// the checks of every row (before anything is queued)
static int check_sample_rows(NanoHipModel *m, uint32_t batch, const NanoHipSampleParamsEdit *params, const NanoHipSample *out) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null argument");
    if (batch == 0 || batch > m->maxB || batch > NANO_MAX_BATCH) FAIL(NANO_HIP_EINVAL, "batch %u out of range (max_batch %u)", batch, m->maxB);
    if (!params || !out) FAIL(NANO_HIP_EINVAL, "null argument");
    const uint32_t V = m->d.vocab_size;
    for (uint32_t i = 0; i < batch; i++) {
        const NanoHipSampleParams &p = params[i].ex.p;
        if (params[i].ex.reserved[0] | params[i].ex.reserved[1] | params[i].ex.reserved[2]) FAIL(NANO_HIP_EINVAL, "reserved words of row %u are not 0", i);
        if (p.n_history && !p.history) FAIL(NANO_HIP_EINVAL, "null history of row %u", i);
        if (row_edited(params[i])) if (const int rc = check_row_edit(m, i, params[i])) return rc;
        if (p.repetition_penalty == 1.0f) continue;                        // (the history is not read)
        if (p.n_history > m->S + 1) FAIL(NANO_HIP_EINVAL, "history of %u ids of row %u exceeds max_seq_len + 1", p.n_history, i);
        for (uint32_t k = 0; k < p.n_history; k++) if (p.history[k] >= V) FAIL(NANO_HIP_EINVAL, "history id %u of row %u out of vocabulary", p.history[k], i);
    }
    return 0;
}
// Bytes of staging one row's edit may take: its mask and a full bias list, each starting at a multiple of 16.
static inline size_t edit_row_bytes(uint32_t V) { return align_up((size_t)mask_words(V) * 4, 16) + (size_t)NANO_BIAS_MAX * sizeof(NanoHipLogitBias) + 16; }
// the first call that carries an edit: parameters, ids, masks and lists get one device and one pinned block of their own
static int sampler_edit_init(NanoHipModel *m) {
    Sampler *sp = m->smp;
    if (sp->edit_dev) return 0;
    const uint32_t R = m->maxB;
    const size_t bytes = align_up((size_t)R * sizeof(SampleRowParams) + (size_t)R * (m->S + 1) * 4, 16) + (size_t)R * edit_row_bytes(m->d.vocab_size);
    uint8_t *d = nullptr, *h = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess || hipHostMalloc((void **)&h, bytes) != hipSuccess) {
        if (d) (void)hipFree(d);
        (void)hipGetLastError();                                            // (the model stays usable)
        FAIL(NANO_HIP_ENOMEM, "logit-edit staging allocation failed (%zu bytes for %u rows)", bytes, R);
    }
    sp->edit_dev = d; sp->edit_host = h;
    sp->params = (SampleRowParams *)d; sp->b.rp = sp->params; sp->h_params = (SampleRowParams *)h;
    return 0;
}
extern "C" int nano_hip_mask_table_set(NanoHipModel *m, const uint32_t *words, uint32_t n_masks) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null argument");
    if (n_masks && !words) FAIL(NANO_HIP_EINVAL, "null argument");
    const uint32_t V = m->d.vocab_size, W = mask_words(V);
    for (uint32_t k = 0; k < n_masks; k++)
        if (!mask_allows_any(words + (size_t)k * W, V)) FAIL(NANO_HIP_EINVAL, "mask %u of the table allows no token", k + 1);
    HIP_TRY(hipSetDevice(m->device));
    if (const int rc = sampler_init(m)) return rc;
    Sampler *sp = m->smp;
    uint32_t *tab = nullptr;
    if (n_masks) {
        const size_t bytes = (size_t)n_masks * W * 4;
        if (hipMalloc(&tab, bytes) != hipSuccess) { (void)hipGetLastError(); FAIL(NANO_HIP_ENOMEM, "mask table allocation failed (%zu bytes)", bytes); }
        if (hipMemcpy(tab, words, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(tab); (void)hipGetLastError(); FAIL(NANO_HIP_ERUNTIME, "mask table upload failed"); }
    }
    HIP_TRY(hipStreamSynchronize(m->st));                                  // (no queued row still reads the old table)
    if (sp->mask_tab) (void)hipFree(sp->mask_tab);
    sp->mask_tab = tab; sp->n_masks = n_masks;
    return 0;
}
// queue the sampler behind whatever produced logits[batch][V] (device) on the model's stream, wait, fill out[batch].  Returns 0 with
// the stream synchronised: the caller then looks at the sticky error word (and may re-issue the forward).
static int sampler_run(NanoHipModel *m, const float *logits, uint32_t batch, const NanoHipSampleParamsEdit *params, NanoHipSample *out) {
    Sampler *sp = m->smp;
    SampleRows b = sp->b;
    b.a.logits = logits;
    const uint32_t V = b.a.V;
    const size_t npad = (size_t)b.a.nch * SAMPLE_CHUNK;
    bool any_softmax = false, any_argmax = false;
    // the seen sets: per slot, start over when the history is not an extension of what the slot holds.  The new ids of all rows
    // follow the rows' parameters, and both go up in one copy.
    uint32_t *h_ids = reinterpret_cast<uint32_t *>(sp->h_params + batch);
    size_t n_ids = 0;
    for (uint32_t i = 0; i < batch; i++) {
        const NanoHipSampleParams &p = params[i].ex.p;
        SampleRowParams &q = sp->h_params[i];
        q.penalty = p.repetition_penalty; q.temperature = p.temperature; q.top_p = p.top_p; q.coin = p.coin; q.top_k = params[i].ex.top_k;
        q.allow = nullptr; q.bias = nullptr; q.n_bias = 0; q._pad = 0;
        q.cutoff = (1.0f - p.top_p) / (float)((int)V - 1);                  // (1.0f - top_p) / (n - 1), infer.c:1064
        (p.temperature == 0.0f ? any_argmax : any_softmax) = true;
        if (p.repetition_penalty == 1.0f) continue;                        // x / 1.0f is exact: no set needed
        std::vector<uint32_t> &ap = sp->applied[i];
        if (ap.size() > p.n_history || memcmp(ap.data(), p.history, ap.size() * 4) != 0) {
            HIP_TRY(hipMemsetAsync(const_cast<uint8_t *>(b.a.seen) + (size_t)i * b.rstride, 0, npad, m->st));
            ap.clear();
        }
        for (uint32_t k = (uint32_t)ap.size(); k < p.n_history; k++) h_ids[n_ids++] = (uint32_t)((uint64_t)i * b.rstride + p.history[k]);
        ap.insert(ap.end(), p.history + ap.size(), p.history + p.n_history);
    }
    // the rows' edits: a table mask is referenced where it lies; per-call masks and bias lists follow the ids in the same upload
    size_t up = batch * sizeof(SampleRowParams) + n_ids * 4;
    bool edited = false;
    const uint32_t W = mask_words(V);
    for (uint32_t i = 0; i < batch; i++) {
        const NanoHipSampleParamsEdit &e = params[i];
        SampleRowParams &q = sp->h_params[i];
        if (e.mask_id) q.allow = sp->mask_tab + (size_t)(e.mask_id - 1) * W;
        edited = edited || row_edited(e);
        if (!e.allow && !e.n_bias) continue;
        up = align_up(up, 16);                                              // (sampler_edit_init sized the blocks for every row's largest edit)
        if (e.allow) {
            memcpy(sp->edit_host + up, e.allow, (size_t)W * 4);
            q.allow = reinterpret_cast<const uint32_t *>(sp->edit_dev + up);
            up += align_up((size_t)W * 4, 16);
        }
        if (e.n_bias) {
            memcpy(sp->edit_host + up, e.bias, (size_t)e.n_bias * sizeof(NanoHipLogitBias));
            q.bias = reinterpret_cast<const NanoHipLogitBias *>(sp->edit_dev + up); q.n_bias = e.n_bias;
            up += (size_t)e.n_bias * sizeof(NanoHipLogitBias);
        }
    }
    HIP_TRY(hipMemcpyAsync(sp->params, sp->h_params, up, hipMemcpyHostToDevice, m->st));
    HIP_TRY(launch_seen_set(reinterpret_cast<const uint32_t *>(sp->params + batch), (uint32_t)n_ids, const_cast<uint8_t *>(b.a.seen), m->st));
    HIP_TRY(launch_sample_rows(b, batch, any_softmax, edited, m->st));
    if (any_argmax) {                                                      // penalised arg-max (infer.c:1169-1171) over every row's y
        ArgmaxArgs aa{ b.a.y, V, (uint32_t)(b.rstride / 4), m->amax, nullptr, m->pos, nullptr, m->pos0, batch, nullptr, 0 };
        HIP_TRY(launch_argmax(aa, batch, m->st));
        HIP_TRY(hipMemcpyAsync(m->h_amax, m->amax, batch * 4, hipMemcpyDeviceToHost, m->st));
    }
    if (any_softmax) HIP_TRY(hipMemcpyAsync(sp->h_res, b.a.res, batch * sizeof(NanoHipSample), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    // nuclei beyond the LDS sorter (near-uniform distributions): the wide phase (sampler_wide.hip) on that row's numerators and
    // denominator -- every candidate sorted by a device radix sort, the same cut and draw -- one row after another
    bool wide_ran = false;
    for (uint32_t i = 0; i < batch && any_softmax; i++) {
        if (params[i].ex.p.temperature == 0.0f || sp->h_res[i].status != NANO_SAMPLE_FALLBACK || sp->h_res[i].n_candidates == 0) continue;
        if (!sp->wide) {
            sp->wide_temp_bytes = sample_wide_temp_bytes((uint32_t)npad);
            const size_t tb = (sp->wide_temp_bytes + 255) & ~(size_t)255;
            if (!sp->wide_temp_bytes || hipMalloc(&sp->wide, npad * 20 + tb) != hipSuccess) { sp->wide = nullptr; (void)hipGetLastError(); break; }   // (the caller's host loops)
            sp->wide_a.wide_in = (unsigned long long *)sp->wide; sp->wide_a.wide_out = sp->wide_a.wide_in + npad;
            sp->wide_a.wide_p = (float *)(sp->wide_a.wide_out + npad); sp->wide_a.wide_cap = (uint32_t)npad;
            sp->wide_temp = sp->wide + npad * 20;
        }
        SampleArgs a = sample_row(b, i, sp->h_params[i]);
        a.wide_in = sp->wide_a.wide_in; a.wide_out = sp->wide_a.wide_out; a.wide_p = sp->wide_a.wide_p; a.wide_cap = sp->wide_a.wide_cap;
        HIP_TRY(launch_sample_wide(a, sp->wide_temp, sp->wide_temp_bytes, m->st));
        wide_ran = true;
    }
    if (wide_ran) {
        HIP_TRY(hipMemcpyAsync(sp->h_res, b.a.res, batch * sizeof(NanoHipSample), hipMemcpyDeviceToHost, m->st));
        HIP_TRY(hipStreamSynchronize(m->st));
    }
    for (uint32_t i = 0; i < batch; i++) {
        if (params[i].ex.p.temperature == 0.0f) { memset(&out[i], 0, sizeof out[i]); out[i].token = m->h_amax[i]; out[i].status = NANO_SAMPLE_OK; }
        else out[i] = sp->h_res[i];
    }
    return 0;
}

// does any row carry a per-call mask or a bias list?  (a table mask needs no staging)
static bool any_staged_edit(uint32_t batch, const NanoHipSampleParamsEdit *params) {
    for (uint32_t i = 0; i < batch; i++) if (params[i].allow || params[i].n_bias) return true;
    return false;
}
extern "C" int nano_hip_forward_sample_batch_edit(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                                  const NanoHipSampleParamsEdit *params, NanoHipSample *out) {
    int rc;
    if ((rc = check_sample_rows(m, batch, params, out))) return rc;
    if ((rc = check_batch(m, tokens, pos, batch, 0))) return rc;
    HIP_TRY(hipSetDevice(m->device));
    if ((rc = sampler_init(m))) return rc;
    if (any_staged_edit(batch, params) && (rc = sampler_edit_init(m))) return rc;
    if ((rc = kv_ensure_batch(m, pos, batch, 0, false))) return rc;
    return with_reissue(m, [&](bool) {
        uint32_t max_pos = 0;
        if (const int rs = stage_batch(m, tokens, pos, batch, false, &max_pos)) return rs;
        if (const int rs = run_step(m, batch, 1u, MODE_LOGITS, max_pos)) return rs;
        return sampler_run(m, m->logits, batch, params, out);
    });
}

extern "C" int nano_hip_op_sample_batch_edit(NanoHipModel *m, const float *logits, uint32_t batch, const NanoHipSampleParamsEdit *params, NanoHipSample *out) {
    int rc;
    if ((rc = check_sample_rows(m, batch, params, out))) return rc;
    if (!logits) FAIL(NANO_HIP_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(m->device));
    if ((rc = sampler_init(m))) return rc;
    if (any_staged_edit(batch, params) && (rc = sampler_edit_init(m))) return rc;
    const size_t V = m->d.vocab_size;
    memcpy(m->h_logits, logits, batch * V * 4);
    HIP_TRY(hipMemcpyAsync(m->logits, m->h_logits, batch * V * 4, hipMemcpyHostToDevice, m->st));
    if ((rc = sampler_run(m, m->logits, batch, params, out))) return rc;
    return dev_err_check(m);
}
// The entry points without an edit: the same rows with no mask and no bias list.  A null `params` or a batch beyond NANO_MAX_BATCH is passed
// on unread, as with_top_k_off does below: the _edit call refuses it before it reads a row.
template <class Call> static int with_no_edit(uint32_t batch, const NanoHipSampleParamsEx *params, Call call) {
    NanoHipSampleParamsEdit ed[NANO_MAX_BATCH];
    if (!params || batch > NANO_MAX_BATCH) return call(static_cast<const NanoHipSampleParamsEdit *>(nullptr));
    for (uint32_t i = 0; i < batch; i++) ed[i] = NanoHipSampleParamsEdit{ params[i], nullptr, nullptr, 0u, 0u };
    return call(static_cast<const NanoHipSampleParamsEdit *>(ed));
}
extern "C" int nano_hip_forward_sample_batch_ex(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                                const NanoHipSampleParamsEx *params, NanoHipSample *out) {
    return with_no_edit(batch, params, [&](const NanoHipSampleParamsEdit *ed) { return nano_hip_forward_sample_batch_edit(m, tokens, pos, batch, ed, out); });
}
extern "C" int nano_hip_op_sample_batch_ex(NanoHipModel *m, const float *logits, uint32_t batch, const NanoHipSampleParamsEx *params, NanoHipSample *out) {
    return with_no_edit(batch, params, [&](const NanoHipSampleParamsEdit *ed) { return nano_hip_op_sample_batch_edit(m, logits, batch, ed, out); });
}
// The entry points without top_k: the same rows with top_k = 0.  A null `params` or a batch beyond NANO_MAX_BATCH is passed on unread:
// the _ex call refuses it (a null model first, then the batch, then null pointers) before it reads a row.
template <class Call> static int with_top_k_off(uint32_t batch, const NanoHipSampleParams *params, Call call) {
    NanoHipSampleParamsEx ex[NANO_MAX_BATCH];
    if (!params || batch > NANO_MAX_BATCH) return call(static_cast<const NanoHipSampleParamsEx *>(nullptr));
    for (uint32_t i = 0; i < batch; i++) ex[i] = NanoHipSampleParamsEx{ params[i], 0u, { 0u, 0u, 0u } };
    return call(static_cast<const NanoHipSampleParamsEx *>(ex));
}
extern "C" int nano_hip_forward_sample_batch(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                             const NanoHipSampleParams *params, NanoHipSample *out) {
    return with_top_k_off(batch, params, [&](const NanoHipSampleParamsEx *ex) { return nano_hip_forward_sample_batch_ex(m, tokens, pos, batch, ex, out); });
}
extern "C" int nano_hip_op_sample_batch(NanoHipModel *m, const float *logits, uint32_t batch, const NanoHipSampleParams *params, NanoHipSample *out) {
    return with_top_k_off(batch, params, [&](const NanoHipSampleParamsEx *ex) { return nano_hip_op_sample_batch_ex(m, logits, batch, ex, out); });
}
// one row: slot 0, a batch of one
extern "C" int nano_hip_forward_sample(NanoHipModel *m, uint32_t token, uint32_t pos, const uint32_t *history, uint32_t n_history,
                                       float repetition_penalty, float temperature, float top_p, float coin, NanoHipSample *out) {
    const NanoHipSampleParams p{ repetition_penalty, temperature, top_p, coin, history, n_history };
    return nano_hip_forward_sample_batch(m, &token, &pos, 1, &p, out);
}

extern "C" int nano_hip_op_sample(NanoHipModel *m, const float *logits, const uint32_t *history, uint32_t n_history,
                                  float repetition_penalty, float temperature, float top_p, float coin, NanoHipSample *out) {
    const NanoHipSampleParams p{ repetition_penalty, temperature, top_p, coin, history, n_history };
    return nano_hip_op_sample_batch(m, logits, 1, &p, out);
}
