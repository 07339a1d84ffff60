// backend_rows.hip -- what calls get back per fed row, and ragged steps.
// Row outputs (RowWant, backend_model.h): the one allocator of their scratch (rows_scratch), the sink that batched prefill (backend.hip),
// ragged steps and the decode step with scores (nano_hip_forward_topk, below) share, and the one loop of strict / exact mode.
// Ragged steps (nano_hip_step_rows): rows that each carry their own (KV slot, position).  The planner that cuts a call's rows into passes
// (device-free, queryable), the host predicate of what the row map can address, and the entry point that stages the call once and queues
// its passes through enqueue_step as RAGGED specs (step_spec.h) over row groups the call itself keeps.
// Text embeddings (nano_hip_step_rows_pool): the ragged step with RowWant::POOL, and the one builder of its kernel's map (pool_plan).
#include <algorithm>

#include "backend_model.h"

int rows_check(const NanoHipModel *m, const RowWant &w) {
    if (w.kind == RowWant::POOL) {
        if (!w.pool || !w.pool_out) FAIL(NANO_HIP_EINVAL, "null argument");
        if (w.pool->pooling > NANO_POOL_MEAN || w.pool->normalize > 1u) FAIL(NANO_HIP_EINVAL, "pooling = %u / normalize = %u out of range", w.pool->pooling, w.pool->normalize);
        if (w.pool->dim > m->d.n_embd) FAIL(NANO_HIP_EINVAL, "dim = %u exceeds n_embd (%u)", w.pool->dim, m->d.n_embd);
        if (w.pool->reserved) FAIL(NANO_HIP_EINVAL, "NanoHipPoolParams::reserved must be 0");
        return 0;
    }
    if (w.kind != RowWant::SCORE) return 0;
    if (w.k > NANO_TOPK_MAX) FAIL(NANO_HIP_EINVAL, "k = %u exceeds NANO_TOPK_MAX (%u)", w.k, NANO_TOPK_MAX);
    if (w.k > m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "k = %u exceeds the vocabulary (%u)", w.k, m->d.vocab_size);
    if (w.k ? !w.top_out : !w.scores_out) FAIL(NANO_HIP_EINVAL, "null argument");
    return 0;
}

static size_t pass_rows(const NanoHipModel *m) { return std::max<size_t>(m->pf_chunk, m->maxB); }
void rows_free(NanoHipModel *m) {
    NanoHipModel::RowScratch &s = m->rb;
    void *dev[] = { s.logits, s.part, s.targets, s.rows, s.amax, s.keys, s.call };
    for (void *p : dev) if (p) (void)hipFree(p);
    s = NanoHipModel::RowScratch();
}
int rows_scratch(NanoHipModel *m, uint32_t need, size_t call_rows) {
    NanoHipModel::RowScratch &s = m->rb;
    const size_t V = m->d.vocab_size, nt = score_tiles((uint32_t)V), R = pass_rows(m);
    struct Buf { uint32_t bit; void **p; size_t bytes, fixed; };            // (of the call block: bytes per row, plus bytes whatever the rows)
    auto P = [](auto **p) { return reinterpret_cast<void **>(p); };
    // pass buffers: allocated once each; a failure frees what this call added
    const Buf pass[] = { { P_LOGITS, P(&s.logits), m->pf_chunk * V * 4 }, { P_STATS, P(&s.part), R * nt * sizeof(ScorePartial) }, { P_STATS, P(&s.targets), R * 4 },
                         { P_STATS, P(&s.rows), R * sizeof(NanoHipTokenScore) }, { P_AMAX, P(&s.amax), std::max<size_t>(m->pf_chunk, LOOKUP_MAX_ROWS) * 4 },
                         { P_KEYS, P(&s.keys), R * nt * NANO_TOPK_MAX * sizeof(unsigned long long) } };
    void **fresh[sizeof pass / sizeof *pass]; size_t n_fresh = 0;
    for (const Buf &b : pass) {
        if (!(need & b.bit) || *b.p) continue;
        if (hipMalloc(b.p, b.bytes) == hipSuccess) { fresh[n_fresh++] = b.p; continue; }
        (void)hipGetLastError();
        *b.p = nullptr;
        while (n_fresh) { void **f = fresh[--n_fresh]; (void)hipFree(*f); *f = nullptr; }
        FAIL(NANO_HIP_ENOMEM, "hipMalloc of the row outputs' pass buffers failed (%zu rows, %zu logits each)", R, V);
    }
    // the call block: one capacity, one grow path (wait for the stream, free, allocate), one allocation to unwind
    const uint32_t parts = s.have | (need & C_ALL);
    if (!call_rows || (parts == s.have && call_rows <= s.cap)) return 0;
    const size_t cap = std::max<size_t>({ (size_t)m->S, call_rows, (size_t)s.cap });
    const Buf call[] = { { C_FEED, P(&s.tok), 4 }, { C_FEED, P(&s.pos), 4 }, { C_SLOT, P(&s.slot), 4 }, { C_TGT, P(&s.tgt), 4 }, { C_AMAX, P(&s.out_amax), 4 },
                         { C_SC, P(&s.sc), sizeof(NanoHipTokenScore) }, { C_TOP, P(&s.top), NANO_TOPK_MAX * sizeof(NanoHipTopEntry) },
                         // (a call names every slot once: at most max_batch segments, whatever its rows)
                         { C_POOL, P(&s.pool_map), (POOL_GROUP_WORDS + 1) * 4 }, { C_POOL, P(&s.pool_acc), 0, (size_t)m->maxB * align_up(m->d.n_embd, 4) * 4 },
                         { C_POOL, P(&s.pool_out), 0, (size_t)m->maxB * m->d.n_embd * 4 } };
    if (s.call) { HIP_TRY(hipStreamSynchronize(m->st)); (void)hipFree(s.call); }
    s.call = nullptr; s.cap = s.have = 0;
    size_t bytes = 0;
    for (const Buf &b : call) { *b.p = nullptr; if (parts & b.bit) bytes += align_up(cap * b.bytes + b.fixed, 256); }
    if (hipMalloc(reinterpret_cast<void **>(&s.call), bytes) != hipSuccess) {
        (void)hipGetLastError();
        s.call = nullptr;
        FAIL(NANO_HIP_ENOMEM, "hipMalloc of the row outputs' buffers of a call of %zu rows failed", cap);
    }
    size_t off = 0;
    for (const Buf &b : call) { *b.p = (parts & b.bit) ? s.call + off : nullptr; if (parts & b.bit) off += align_up(cap * b.bytes + b.fixed, 256); }
    s.cap = (uint32_t)cap; s.have = parts;
    return 0;
}

hipError_t enqueue_topk_rows(NanoHipModel *m, const float *logits, uint32_t rows, uint32_t k, const NanoHipTokenScore *scores, NanoHipTopEntry *out) {
    if (rows > pass_rows(m)) return hipErrorInvalidValue;
    TopkArgs a{};
    a.logits = logits; a.V = m->d.vocab_size; a.ntiles = score_tiles(a.V); a.k = k; a.part = m->rb.keys; a.scores = scores; a.out = out;
    return launch_topk_rows(a, rows, m->st);
}

// ---- the sink (backend_model.h says what each does) ----
int rows_begin(NanoHipModel *m, const RowWant &w, bool passes, uint32_t more, size_t total, const uint32_t *targets) {
    if (const int rc = rows_scratch(m, w.need(passes) | more, total)) return rc;
    if (w.use_targets() && total) HIP_TRY(hipMemcpyAsync(m->rb.tgt, targets, total * 4, hipMemcpyHostToDevice, m->st));     // (a pageable source)
    if (w.kind == RowWant::POOL && total) {                                 // the call's map, and zeros for the segments without rows
        const std::vector<uint32_t> &map = w.pool_plan->map;
        HIP_TRY(hipMemcpyAsync(m->rb.pool_map, map.data(), map.size() * 4, hipMemcpyHostToDevice, m->st));
        HIP_TRY(hipMemsetAsync(m->rb.pool_out, 0, (size_t)w.pool_segs * w.pool_dim * 4, m->st));
    }
    return 0;
}
// POOL: the pool launch behind the pass that fed rows at .. of the call; x: the pass's rows (stride n_embd), norm_w: the final norm's
// weights, or nullptr -- the rows are normed already (the ordered form of pool.hip)
static hipError_t enqueue_pool_rows(NanoHipModel *m, const RowWant &w, size_t at, uint32_t nb, const float *x, const float *norm_w) {
    const PoolPlan &pl = *w.pool_plan;
    const uint32_t p = (uint32_t)(std::upper_bound(pl.pass_start.begin(), pl.pass_start.end(), (uint32_t)at) - pl.pass_start.begin()) - 1u;
    if (pl.pass_start[p] != at || pl.pass_start[p + 1] - pl.pass_start[p] != nb) return hipErrorInvalidValue;
    const uint32_t g0 = pl.group_start[p], g1 = pl.group_start[p + 1];
    PoolArgs a{};
    a.x = x; a.x_stride = m->d.n_embd; a.rows_max = nb; a.w = norm_w;
    a.groups = m->rb.pool_map + (size_t)g0 * POOL_GROUP_WORDS; a.lists = m->rb.pool_map + (size_t)pl.n_groups() * POOL_GROUP_WORDS;
    a.acc = m->rb.pool_acc; a.out = m->rb.pool_out;
    a.n_embd = m->d.n_embd; a.dim = w.pool_dim; a.mean = w.pool->pooling == NANO_POOL_MEAN; a.normalize = w.pool->normalize;
    return launch_pool_rows(a, g1 - g0, m->st);
}
int rows_feed(NanoHipModel *m, size_t total, const uint32_t *tokens, const uint32_t *pos, const uint32_t *slots) {
    HIP_TRY(hipMemcpyAsync(m->rb.tok, tokens, total * 4, hipMemcpyHostToDevice, m->st));          // (pageable sources: staged by the runtime before the call returns)
    HIP_TRY(hipMemcpyAsync(m->rb.pos, pos, total * 4, hipMemcpyHostToDevice, m->st));
    if (slots) HIP_TRY(hipMemcpyAsync(m->rb.slot, slots, total * 4, hipMemcpyHostToDevice, m->st));
    return 0;
}
hipError_t rows_after_step(NanoHipModel *m, const RowWant &w, size_t at, uint32_t nb) {
    const NanoHipModel::RowScratch &s = m->rb;
    if (w.kind == RowWant::ARGMAX) return hipMemcpyAsync(s.out_amax + at, m->amax, nb * 4, hipMemcpyDeviceToDevice, m->st);
    if (w.kind == RowWant::POOL) {                                          // a reference-order step without classifier left the residual row in m->x
        const PoolPlan &pl = *w.pool_plan;                                  // (one row per pass: a row that is not pooled needs no norm)
        if (nb != 1 || pl.group_start[at] == pl.group_start[at + 1]) return nb == 1 ? hipSuccess : hipErrorInvalidValue;
        const uint32_t E = m->d.n_embd;
        const hipError_t e = exact_serves(m) ? launch_exact_rmsnorm(m->xn, m->x, m->rms_final, E, 1, E, E, m->st)
                                             : launch_strict_rmsnorm(m->xn, m->x, m->rms_final, E, 1, E, E, m->st);
        return e != hipSuccess ? e : enqueue_pool_rows(m, w, at, 1, m->xn, nullptr);
    }
    if (w.kind != RowWant::SCORE) return hipSuccess;
    const hipError_t e = enqueue_score_rows(m, m->logits, nb, w.use_targets() ? s.tgt + at : nullptr, s.sc + at);
    return (e != hipSuccess || !w.k) ? e : enqueue_topk_rows(m, m->logits, nb, w.k, s.sc + at, s.top + at * w.k);
}
hipError_t rows_pass_targets(NanoHipModel *m, const RowWant &w, size_t at, uint32_t nb) {
    const NanoHipModel::RowScratch &s = m->rb;
    return w.use_targets() ? hipMemcpyAsync(s.targets, s.tgt + at, nb * 4, hipMemcpyDeviceToDevice, m->st) : hipSuccess;
}
hipError_t rows_after_pass(NanoHipModel *m, const RowWant &w, size_t at, uint32_t nb) {
    const NanoHipModel::RowScratch &s = m->rb;
    if (w.kind == RowWant::ARGMAX) return hipMemcpyAsync(s.out_amax + at, s.amax, nb * 4, hipMemcpyDeviceToDevice, m->st);
    if (w.kind == RowWant::POOL) return enqueue_pool_rows(m, w, at, nb, m->x, m->rms_final);      // (a MODE_NOCLS pass: its residual rows are in m->x)
    if (w.kind != RowWant::SCORE) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(s.sc + at, s.rows, nb * sizeof(NanoHipTokenScore), hipMemcpyDeviceToDevice, m->st);
    return (e != hipSuccess || !w.k) ? e : enqueue_topk_rows(m, s.logits, nb, w.k, s.rows, s.top + at * w.k);
}
int rows_run_ordered(NanoHipModel *m, const RowWant &w, size_t total, uint32_t slot, const uint32_t *row_slot) {
    for (size_t i = 0; i < total; i++) {
        HIP_TRY(hipMemcpyAsync(m->tokens, m->rb.tok + i, 4, hipMemcpyDeviceToDevice, m->st));
        HIP_TRY(hipMemcpyAsync(m->pos, m->rb.pos + i, 4, hipMemcpyDeviceToDevice, m->st));
        if (const int rc = run_step_ordered(m, 1, 1, w.mode_row(), row_slot ? row_slot[i] : slot)) return rc;
        HIP_TRY(rows_after_step(m, w, i, 1));
    }
    return 0;
}
int rows_back(NanoHipModel *m, const RowWant &w, size_t total, const uint32_t *where, bool check) {
    const NanoHipModel::RowScratch &s = m->rb;
    const bool score = w.kind == RowWant::SCORE;
    const size_t k = score ? w.k : 0;
    // (where: through host copies in feeding order, gathered after the wait)
    std::vector<uint32_t> amax(where && w.kind == RowWant::ARGMAX ? total : 0);
    std::vector<NanoHipTokenScore> sc(where && score && w.scores_out ? total : 0);
    std::vector<NanoHipTopEntry> top(where ? total * k : 0);
    if (w.kind == RowWant::ARGMAX) HIP_TRY(hipMemcpyAsync(where ? amax.data() : w.argmax_out, s.out_amax, total * 4, hipMemcpyDeviceToHost, m->st));
    if (k) HIP_TRY(hipMemcpyAsync(where ? top.data() : w.top_out, s.top, total * k * sizeof(NanoHipTopEntry), hipMemcpyDeviceToHost, m->st));
    if (score && w.scores_out) HIP_TRY(hipMemcpyAsync(where ? sc.data() : w.scores_out, s.sc, total * sizeof(NanoHipTokenScore), hipMemcpyDeviceToHost, m->st));
    if (w.kind == RowWant::POOL) HIP_TRY(hipMemcpyAsync(w.pool_out, s.pool_out, (size_t)w.pool_segs * w.pool_dim * 4, hipMemcpyDeviceToHost, m->st));   // (per segment: no gather)
    HIP_TRY(hipStreamSynchronize(m->st));                                   // the call's one wait
    if (check) { if (const int rc = dev_err_check(m)) return rc; }
    for (size_t r = 0; r < amax.size(); r++) w.argmax_out[r] = amax[where[r]];
    for (size_t r = 0; r < sc.size(); r++) w.scores_out[r] = sc[where[r]];
    for (size_t r = 0; r < (top.empty() ? 0 : total); r++) std::copy(top.begin() + where[r] * k, top.begin() + (where[r] + 1) * k, w.top_out + r * k);
    return 0;
}

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
// the order a call feeds its rows in (pass after pass, a pass's rows by index): the first fed row of every pass, and where caller row r goes
static void rows_placement(const RowsPlan &plan, std::vector<uint32_t> *pass_start, std::vector<uint32_t> *where) {
    const size_t total = plan.rows();
    pass_start->assign(plan.n_passes + 1, 0u); where->resize(total);
    for (size_t r = 0; r < total; r++) (*pass_start)[plan.pass[r] + 1]++;
    for (uint32_t p = 0; p < plan.n_passes; p++) (*pass_start)[p + 1] += (*pass_start)[p];
    for (size_t r = 0; r < total; r++) (*where)[r] = (*pass_start)[plan.pass[r]] + plan.index[r];
}

// ---- text embeddings: the map of a pooled call (pool_plan.h) ----
// p->pass_start / p->where are the call's placement.  Per fed row its segment and its ordinal among the segment's pooled rows (LAST: the
// segment's last row is ordinal 0, no other row is pooled; MEAN: row j of the segment is ordinal j); from those alone the workgroups of
// every pass: one per segment with pooled rows in the pass, its rows ascending by pass row -- which is ascending position, a slot's rows
// of one pass being ordered by range hint, stably -- "began earlier" = its first ordinal is not 0, "ends here" = its last ordinal is
// the segment's last.
static void pool_map_fill(const NanoHipRowSeg *segs, uint32_t n_segs, uint32_t pooling, PoolPlan *p) {
    const size_t total = p->where.size();
    const uint32_t n_passes = (uint32_t)p->pass_start.size() - 1u, none = 0xffffffffu;
    p->row_seg.assign(total, 0u); p->row_ordinal.assign(total, none);
    size_t r = 0;
    for (uint32_t i = 0; i < n_segs; i++)
        for (uint32_t j = 0; j < segs[i].count; j++, r++) {
            const uint32_t w = p->where[r];
            p->row_seg[w] = i;
            if (pooling == NANO_POOL_MEAN) p->row_ordinal[w] = j;
            else if (j == segs[i].count - 1u) p->row_ordinal[w] = 0u;
        }
    std::vector<uint32_t> groups, lists, rows;
    p->group_start.assign(n_passes + 1, 0u);
    for (uint32_t ps = 0; ps < n_passes; ps++) {
        const uint32_t w0 = p->pass_start[ps], w1 = p->pass_start[ps + 1];
        rows.clear();
        for (uint32_t w = w0; w < w1; w++) if (p->row_ordinal[w] != none) rows.push_back(w);
        std::stable_sort(rows.begin(), rows.end(), [&](uint32_t a, uint32_t b) { return p->row_seg[a] < p->row_seg[b]; });
        for (size_t k = 0; k < rows.size();) {
            const uint32_t seg = p->row_seg[rows[k]], at = (uint32_t)lists.size();
            size_t e = k;
            for (; e < rows.size() && p->row_seg[rows[e]] == seg; e++) lists.push_back(rows[e] - w0);
            const uint32_t last = pooling == NANO_POOL_MEAN ? segs[seg].count - 1u : 0u;
            const uint32_t flags = (p->row_ordinal[rows[k]] != 0u ? POOL_BEGUN : 0u) | (p->row_ordinal[rows[e - 1]] == last ? POOL_ENDS : 0u);
            const uint32_t g[POOL_GROUP_WORDS] = { seg, at, (uint32_t)(e - k) | flags, segs[seg].count };
            groups.insert(groups.end(), g, g + POOL_GROUP_WORDS);
            k = e;
        }
        p->group_start[ps + 1] = (uint32_t)(groups.size() / POOL_GROUP_WORDS);
    }
    p->map = std::move(groups);
    p->map.insert(p->map.end(), lists.begin(), lists.end());
}
int nano::pool_plan(const NanoHipRowSeg *segs, uint32_t n_segs, uint32_t cap, uint32_t max_seq_len, uint32_t pooling, PoolPlan *out) {
    if (pooling > NANO_POOL_MEAN) FAIL(NANO_HIP_EINVAL, "pooling = %u out of range", pooling);
    RowsPlan plan;
    if (const int rc = rows_plan(segs, n_segs, cap, max_seq_len, &plan)) return rc;
    PoolPlan p;
    rows_placement(plan, &p.pass_start, &p.where);
    pool_map_fill(segs, n_segs, pooling, &p);
    *out = std::move(p);
    return 0;
}
extern "C" int nano_hip_rows_pool_plan(const NanoHipRowSeg *segs, uint32_t n_segs, uint32_t cap, uint32_t max_seq_len, uint32_t pooling,
                                       uint32_t *row_seg, uint32_t *row_ordinal) {
    PoolPlan p;
    if (const int rc = pool_plan(segs, n_segs, cap, max_seq_len, pooling, &p)) return rc;
    if (row_seg) std::copy(p.row_seg.begin(), p.row_seg.end(), row_seg);
    if (row_ordinal) std::copy(p.row_ordinal.begin(), p.row_ordinal.end(), row_ordinal);
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

// one ragged pass of nb rows (m->tokens / m->pos hold them, row_slot their slots, groups their buckets): eager; every row splits as
// its own decode step and a kernel of its own combines, as in a prefill chunk
hipError_t enqueue_rows_pass(NanoHipModel *m, uint32_t nb, const RowWant &want, const uint32_t *row_slot, const std::vector<RowGroup> &groups) {
    const StepSpec s = StepSpec::ragged(nb, want.mode_pass(), row_slot, groups.data(), (uint32_t)groups.size(), want.use_targets());
    m->nsplit = xba_nsplit(m, s);                                      // 1 (as a prefill chunk: xba is left final)
    return enqueue_step(m, s);
}

// A ragged step, as nano_hip_step_rows (every row's arg-max, or nothing) and nano_hip_step_rows_score (every row's record and, k >= 1, its
// k entries) call it.  A scoring pass is a MODE_SCORE pass: the classifier over all its rows and the statistics for the pass's targets,
// staged in pass order; the selection's two launches follow eagerly on the same buffers (rows_after_pass).  Results are gathered to caller
// order through where[].
static int step_rows_run(NanoHipModel *m, const NanoHipRowSeg *segs, uint32_t n_segs, const uint32_t *tokens, const RowWant &want_in) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    if (const int rc = rows_check(m, want_in)) return rc;
    RowWant want = want_in;                                                 // (POOL: completed below with the call's plan)
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
    if (want.use_targets()) for (size_t r = 0; r < total; r++) if (want.targets[r] >= m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "target %u out of vocabulary", want.targets[r]);
    if (m->lora_on) FAIL(NANO_HIP_EINVAL, "ragged steps are not available with the LoRA side branches (their v branch addresses the cache by a flat stride)");
    if (!m->kv.paged && !nano_hip_rows_addressable(m->d.n_layer, m->S, m->KD, (uint32_t)kv_esz(m)))
        FAIL(NANO_HIP_EINVAL, "the row map cannot address a cache of %u layers x %u positions x %u elements", m->d.n_layer, m->S, m->KD);
    if (total == 0) {
        if (want.kind == RowWant::POOL) std::fill(want.pool_out, want.pool_out + (size_t)n_segs * (want.pool->dim ? want.pool->dim : m->d.n_embd), 0.0f);
        return 0;
    }
    HIP_TRY(hipSetDevice(m->device));
    if (const int rc = step_served(m, true)) return rc;
    const bool ordered = strict_serves(m) || exact_serves(m);
    if (!ordered && !m->kv_half && !m->kv.paged && !m->rows.vraw && hipMalloc(reinterpret_cast<void **>(&m->rows.vraw), (size_t)m->Bs * m->KD * 4) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(NANO_HIP_ENOMEM, "hipMalloc of the ragged steps' v scratch failed");
    }
    // the call's rows in pass order: where caller row r went, and its token, position, slot and target there -- on the device ONCE
    PoolPlan pp;                                                            // (POOL: the call's map too, from the same placement)
    std::vector<uint32_t> &pass_start = pp.pass_start, &where = pp.where, stage(3 * total), tstage(want.use_targets() ? total : 0);
    rows_placement(plan, &pass_start, &where);
    if (want.kind == RowWant::POOL) {
        pool_map_fill(segs, n_segs, want.pool->pooling, &pp);
        want.pool_plan = &pp; want.pool_segs = n_segs; want.pool_dim = want.pool->dim ? want.pool->dim : m->d.n_embd;
    }
    {
        size_t r = 0;
        for (uint32_t i = 0; i < n_segs; i++)
            for (uint32_t j = 0; j < segs[i].count; j++, r++) {
                const size_t w = where[r];
                stage[w] = tokens[r]; stage[total + w] = segs[i].pos0 + j; stage[2 * total + w] = segs[i].slot;
                if (!tstage.empty()) tstage[w] = want.targets[r];
            }
    }
    if (m->kv.paged) {                                                      // every page of every segment, all or nothing, before anything is queued
        std::vector<uint32_t> slots, first, need;
        for (uint32_t i = 0; i < n_segs; i++)
            if (segs[i].count) { slots.push_back(segs[i].slot); first.push_back(segs[i].pos0); need.push_back(segs[i].pos0 + segs[i].count - 1); }
        if (const int rc = kv_ensure(m, slots.data(), first.data(), need.data(), (uint32_t)slots.size())) return rc;
    }
    if (const int rc = rows_begin(m, want, !ordered, C_FEED | C_SLOT, total, tstage.data())) return rc;
    if (const int rc = rows_feed(m, total, stage.data(), stage.data() + total, stage.data() + 2 * total)) return rc;
    if (ordered) {
        // strict / exact mode: one pass = one row (cap 1, so pass order is caller order): a reference-order step in the row's slot
        if (const int rc = rows_run_ordered(m, want, total, 0, stage.data() + 2 * total)) return rc;
    } else {
        std::vector<RowGroup> groups;
        for (uint32_t p = 0; p < plan.n_passes; p++) {
            const size_t w0 = pass_start[p];
            const uint32_t nb = pass_start[p + 1] - pass_start[p];
            HIP_TRY(hipMemcpyAsync(m->tokens, m->rb.tok + w0, nb * 4, hipMemcpyDeviceToDevice, m->st));
            HIP_TRY(hipMemcpyAsync(m->pos, m->rb.pos + w0, nb * 4, hipMemcpyDeviceToDevice, m->st));
            groups.clear();
            for (uint32_t j = 0; j < nb; j++) {                            // (sorted by hint: a group is a run of equal hints)
                const uint32_t pos = stage[total + w0 + j], h = range_hint_of(m, 1, 1, pos);
                if (groups.empty() || groups.back().hint != h) groups.push_back({j, 1u, h});
                else groups.back().n++;
            }
            HIP_TRY(rows_pass_targets(m, want, w0, nb));
            HIP_TRY(enqueue_rows_pass(m, nb, want, m->rb.slot + w0, groups));
            HIP_TRY(rows_after_pass(m, want, w0, nb));
        }
    }
    return rows_back(m, want, total, where.data(), true);
}

extern "C" int nano_hip_step_rows(NanoHipModel *m, const NanoHipRowSeg *segs, uint32_t n_segs, const uint32_t *tokens, uint32_t *argmax_out) {
    return step_rows_run(m, segs, n_segs, tokens, RowWant::argmaxes(argmax_out));
}
// The pooled form (text embeddings): MODE_NOCLS passes, the pool launch behind each (rows_after_pass), one vector per segment back.
extern "C" int nano_hip_step_rows_pool(NanoHipModel *m, const NanoHipRowSeg *segs, uint32_t n_segs, const uint32_t *tokens,
                                       const NanoHipPoolParams *p, float *out) {
    return step_rows_run(m, segs, n_segs, tokens, RowWant::pooled(p, out));
}
extern "C" int nano_hip_step_rows_score(NanoHipModel *m, const NanoHipRowSeg *segs, uint32_t n_segs, const uint32_t *tokens,
                                        const uint32_t *targets, uint32_t k, NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out) {
    return step_rows_run(m, segs, n_segs, tokens, RowWant::scores(targets, k, scores_out, top_out));
}

// The decode step with scores: the step as nano_hip_forward_begin queues it with logits wanted (without the copy of the logits), the
// statistics and the selection on its rows of m->logits, the results back, the wait.  A hand-off that gave up: the same step once more
// through the plain launches, as nano_hip_forward_end does (with_reissue takes the sticky word: no check in rows_back).
extern "C" int nano_hip_forward_topk(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch,
                                     const uint32_t *targets, uint32_t k, NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null argument");
    const RowWant want = RowWant::scores(targets, k, scores_out, top_out);
    int rc;
    if ((rc = rows_check(m, want))) return rc;
    if ((rc = check_batch(m, tokens, pos, batch, 0))) return rc;
    if (targets) for (uint32_t i = 0; i < batch; i++) if (targets[i] >= m->d.vocab_size) FAIL(NANO_HIP_EINVAL, "target %u out of vocabulary", targets[i]);
    HIP_TRY(hipSetDevice(m->device));
    if ((rc = step_served(m, false))) return rc;
    if ((rc = rows_begin(m, want, false, 0, batch, targets))) return rc;     // (the step's rows are in m->logits: no pass buffer for logits)
    return with_reissue(m, [&](bool) {
        int rc;
        if ((rc = kv_ensure_batch(m, pos, batch, 0, false))) return rc;
        uint32_t max_pos = 0;
        if ((rc = stage_batch(m, tokens, pos, batch, false, &max_pos))) return rc;
        if ((rc = run_step(m, batch, 1u, MODE_LOGITS, max_pos))) return rc;
        HIP_TRY(rows_after_step(m, want, 0, batch));
        return rows_back(m, want, batch, nullptr, false);
    });
}
