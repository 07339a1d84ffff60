// ops.hip -- single-operator entry points of the C-ABI (nano_hip_op_*): host pointers in, host
// pointers out, running the SAME device kernels the fused forward uses.  They exist for the
// operator-level parity tests (oracle-fed inputs, SURVEY 7 "parity definition" tier ii).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <string>
#include <vector>

#include "../../include/nano_mi355x.h"
#include "kernels.h"
#include "pool_plan.h"

using namespace nano;

extern "C" const char *nano_hip_last_error(void);
namespace { thread_local std::string g_op_err; }

// error text is shared through backend.hip's thread-local via this helper
extern "C" void nano_hip_set_error_(const char *msg);

struct DevBufs {
    std::vector<void *> ptrs;
    ~DevBufs() { for (void *p : ptrs) (void)hipFree(p); }
    template <typename T> T *alloc(size_t n) {
        void *p = nullptr;
        if (hipMalloc(&p, n * sizeof(T) + 16) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return reinterpret_cast<T *>(p);
    }
    template <typename T> T *upload(const T *h, size_t n) {
        T *d = alloc<T>(n);
        if (d && hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
};

#define OP_CHECK(cond, msg) do { if (!(cond)) { nano_hip_set_error_(msg); return NANO_HIP_ERUNTIME; } } while (0)
#define OP_HIP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { nano_hip_set_error_(hipGetErrorString(_e)); return NANO_HIP_ERUNTIME; } } while (0)

static int begin(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { nano_hip_set_error_("no HIP device visible (no CPU fallback)"); return NANO_HIP_ENODEV; }
    if (device < 0 || device >= n) { nano_hip_set_error_("device out of range"); return NANO_HIP_EINVAL; }
    OP_HIP(hipSetDevice(device));
    return 0;
}

extern "C" int nano_hip_op_rmsnorm(int device, float *out, const float *x, const float *w, uint32_t n) {
    int rc; if ((rc = begin(device))) return rc;
    DevBufs B; float *dx = B.upload(x, n), *dw = B.upload(w, n), *dout = B.alloc<float>(n);
    OP_CHECK(dx && dw && dout, "device alloc failed");
    OP_HIP(launch_rmsnorm(dout, dx, dw, n, 0));
    OP_HIP(hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

static int run_gemv(uint32_t quant, GemvArgs &a) {
    hipError_t e = (quant == NANO_QUANT_Q4K) ? launch_gemv_q4k(a, 0) : launch_gemv(quant, a, 0);
    OP_HIP(e);
    OP_HIP(hipDeviceSynchronize());
    return 0;
}

extern "C" int nano_hip_op_matmul_f32(int device, float *out, const float *x, const float *w, uint32_t n, uint32_t d) {
    int rc; if ((rc = begin(device))) return rc;
    if (n % 4) { nano_hip_set_error_("n must be a multiple of 4"); return NANO_HIP_EINVAL; }
    DevBufs B; float *dx = B.upload(x, n), *dw = B.upload(w, (size_t)n * d), *dout = B.alloc<float>(d);
    OP_CHECK(dx && dw && dout, "device alloc failed");
    GemvArgs a{}; a.nseg = 1; a.seg[0].w = dw; a.seg[0].out = dout; a.seg[0].rows = d; a.seg[0].out_bstride = d;
    a.n = n; a.nb = 1; a.xin = dx; a.xin_bstride = n; a.epi = GEMV_EPI_STORE;
    if ((rc = run_gemv(NANO_QUANT_F32, a))) return rc;
    OP_HIP(hipMemcpy(out, dout, (size_t)d * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nano_hip_op_quantize_q80(int device, const float *x, uint32_t n, uint32_t gs, int8_t *q, float *s) {
    int rc; if ((rc = begin(device))) return rc;
    if (!(gs == 32 || gs == 64 || gs == 128 || gs == 256) || n % gs) { nano_hip_set_error_("bad group size"); return NANO_HIP_EINVAL; }
    DevBufs B; float *dx = B.upload(x, n); int8_t *dq = B.alloc<int8_t>(n); float *ds = B.alloc<float>(n / gs);
    OP_CHECK(dx && dq && ds, "device alloc failed");
    OP_HIP(launch_quantize_q80(dx, n, gs, dq, ds, 0));
    OP_HIP(hipMemcpy(q, dq, n, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(s, ds, (size_t)(n / gs) * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nano_hip_op_matmul_q80(int device, float *out, const int8_t *xq, const float *xs, const int8_t *wq,
                                      const float *ws, uint32_t n, uint32_t d, uint32_t gs) {
    int rc; if ((rc = begin(device))) return rc;
    if (!(gs == 32 || gs == 64 || gs == 128 || gs == 256) || n % gs || n % 16) { nano_hip_set_error_("bad n / group size"); return NANO_HIP_EINVAL; }
    DevBufs B;
    int8_t *dxq = B.upload(xq, n), *dwq = B.upload(wq, (size_t)n * d);
    float *dxs = B.upload(xs, n / gs), *dws = B.upload(ws, (size_t)n * d / gs), *dout = B.alloc<float>(d);
    OP_CHECK(dxq && dwq && dxs && dws && dout, "device alloc failed");
    GemvArgs a{}; a.nseg = 1; a.seg[0].w = dwq; a.seg[0].ws = dws; a.seg[0].out = dout; a.seg[0].rows = d; a.seg[0].out_bstride = d;
    a.n = n; a.gs = gs; a.nb = 1; a.epi = GEMV_EPI_STORE; a.xq_in = dxq; a.xs_in = dxs;
    a.ordered = 1;      // the operator-level certificate: the reference's ascending group order (the fast path's canonical fold is tested through nano_hip_op_fused_gemv)
    if ((rc = run_gemv(NANO_QUANT_Q80, a))) return rc;
    OP_HIP(hipMemcpy(out, dout, (size_t)d * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nano_hip_op_quantize_q4k(int device, const float *x, uint32_t n, uint8_t *blocks_out) {
    int rc; if ((rc = begin(device))) return rc;
    const size_t nbytes = (size_t)((n + 255) / 256) * 160;
    DevBufs B; float *dx = B.upload(x, n); uint8_t *db = B.alloc<uint8_t>(nbytes);
    OP_CHECK(dx && db, "device alloc failed");
    OP_HIP(hipMemset(db, 0, nbytes));
    OP_HIP(launch_quantize_q4k(dx, n, db, 0));
    OP_HIP(hipMemcpy(blocks_out, db, nbytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nano_hip_op_matmul_q4k(int device, float *out, const uint8_t *x_blocks, const uint8_t *w_blocks, uint32_t n, uint32_t d) {
    int rc; if ((rc = begin(device))) return rc;
    const size_t bpl = (n + 255) / 256;
    DevBufs B; uint8_t *dx = B.upload(x_blocks, bpl * 160), *dw = B.upload(w_blocks, (size_t)d * bpl * 160);
    float *dout = B.alloc<float>(d);
    OP_CHECK(dx && dw && dout, "device alloc failed");
    GemvArgs a{}; a.nseg = 1; a.seg[0].w = dw; a.seg[0].out = dout; a.seg[0].rows = d; a.seg[0].out_bstride = d;
    a.n = n; a.nb = 1; a.epi = GEMV_EPI_STORE; a.x4_in = dx;
    if ((rc = run_gemv(NANO_QUANT_Q4K, a))) return rc;
    OP_HIP(hipMemcpy(out, dout, (size_t)d * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nano_hip_op_rope(int device, float *head, uint32_t hd, const float *fcr, const float *fci, int qwen3_style) {
    int rc; if ((rc = begin(device))) return rc;
    if (hd > 512 || hd % 2) { nano_hip_set_error_("bad head_dim"); return NANO_HIP_EINVAL; }
    DevBufs B; float *dh = B.upload(head, hd), *dc = B.upload(fcr, hd / 2), *ds = B.upload(fci, hd / 2);
    OP_CHECK(dh && dc && ds, "device alloc failed");
    OP_HIP(launch_rope(dh, hd, dc, ds, qwen3_style, 0));
    OP_HIP(hipMemcpy(head, dh, hd * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nano_hip_op_attention(int device, float *out, const float *q, const float *k_cache, const float *v_cache,
                                     uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t range) {
    int rc; if ((rc = begin(device))) return rc;
    if (!range || !n_kv_head || n_head % n_kv_head || head_dim % 4 || head_dim > 256) { nano_hip_set_error_("bad attention shape"); return NANO_HIP_EINVAL; }
    const size_t QD = (size_t)n_head * head_dim, KD = (size_t)n_kv_head * head_dim;
    const uint32_t nsplit = attention_nsplit(range, head_dim);
    DevBufs B; float *dq = B.upload(q, QD), *dk = B.upload(k_cache, range * KD), *dv = B.upload(v_cache, range * KD), *dout = B.alloc<float>(QD);
    float *dpart = B.alloc<float>(nsplit * QD), *dml = B.alloc<float>((size_t)n_head * nsplit * 2);
    OP_CHECK(dq && dk && dv && dout && dpart && dml, "device alloc failed");
    AttnArgs a{};
    a.q = dq; a.q_out = nullptr; a.kraw = nullptr; a.kcache = dk; a.vcache = dv; a.pos = nullptr; a.out = dpart; a.ml = dml; a.nsplit = nsplit;
    a.layer = 0; a.n_layer = 1; a.S = range; a.hd = head_dim; a.n_head = n_head; a.n_kv_head = n_kv_head;
    a.q_dim = (uint32_t)QD; a.kv_dim = (uint32_t)KD; a.is_causal = 1; a.cache_bstride_rows = range; a.fixed_range = range;
    a.xba_out = dout; a.range_hint = range;
    OP_HIP(launch_attention(a, 1, 0));
    if (nsplit > 1) OP_HIP(launch_attn_combine(dpart, dml, dout, n_head, head_dim, nsplit, 0));
    OP_HIP(hipMemcpy(out, dout, QD * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nano_hip_op_swiglu(int device, float *hb, const float *hb2, uint32_t n) {
    int rc; if ((rc = begin(device))) return rc;
    DevBufs B; float *d1 = B.upload(hb, n), *d2 = B.upload(hb2, n);
    OP_CHECK(d1 && d2, "device alloc failed");
    OP_HIP(launch_swiglu(d1, d2, n, 0));
    OP_HIP(hipMemcpy(hb, d1, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nano_hip_op_exact_rmsnorm(int device, float *out, const float *x, const float *w, uint32_t n) {
    int rc; if ((rc = begin(device))) return rc;
    DevBufs B; float *dx = B.upload(x, n), *dw = B.upload(w, n), *dout = B.alloc<float>(n);
    OP_CHECK(dx && dw && dout, "device alloc failed");
    OP_HIP(launch_exact_rmsnorm(dout, dx, dw, n, 1, n, n, 0));
    OP_HIP(hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nano_hip_op_exact_attention(int device, const NanoExactAttnDesc *d) {
    int rc; if ((rc = begin(device))) return rc;
    if (!d || !d->q || !d->k_cache || !d->v_cache || !d->out) { nano_hip_set_error_("null argument"); return NANO_HIP_EINVAL; }
    if (!d->n_head || !d->n_kv_head || d->n_head % d->n_kv_head || !d->hd || d->hd % 4 || d->hd > 256 || !d->S ||
        (d->is_causal && (d->range == 0 || d->range > d->S))) { nano_hip_set_error_("bad attention shape"); return NANO_HIP_EINVAL; }
    if (!d->long_form && !exact_attention_fits(d->hd, d->S)) { nano_hip_set_error_("S rows do not fit the one-launch kernel's LDS: set long_form"); return NANO_HIP_EINVAL; }
    const uint32_t qd = d->n_head * d->hd, kvd = d->n_kv_head * d->hd, pos = d->is_causal ? d->range - 1u : 0u;
    DevBufs B;
    float *dq = B.upload(d->q, qd), *dk = B.upload(d->k_cache, (size_t)d->S * kvd), *dv = B.upload(d->v_cache, (size_t)d->S * kvd);
    float *dout = B.alloc<float>(qd), *datt = d->long_form ? B.alloc<float>((size_t)d->n_head * d->S) : nullptr;
    uint32_t *dpos = B.upload(&pos, 1);
    OP_CHECK(dq && dk && dv && dout && dpos && (datt || !d->long_form), "device alloc failed");
    StrictAttnArgs sa{};
    sa.q = dq; sa.kcache = dk; sa.vcache = dv; sa.pos = dpos; sa.att = datt; sa.xba = dout;
    sa.n_head = d->n_head; sa.n_kv_head = d->n_kv_head; sa.hd = d->hd; sa.q_dim = qd; sa.kv_dim = kvd;
    sa.layer = 0; sa.n_layer = 1; sa.S = d->S; sa.slot0 = 0; sa.is_causal = d->is_causal ? 1u : 0u;
    OP_HIP(d->long_form ? launch_strict_attention(sa, 1, 0) : launch_exact_attention(sa, 1, 0));
    OP_HIP(hipMemcpy(d->out, dout, (size_t)qd * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nano_hip_op_argmax(int device, const float *x, uint32_t n, uint32_t *idx) {
    int rc; if ((rc = begin(device))) return rc;
    DevBufs B; float *dx = B.upload(x, n); uint32_t *di = B.alloc<uint32_t>(1);
    OP_CHECK(dx && di, "device alloc failed");
    ArgmaxArgs a{ dx, n, n, di, nullptr, nullptr, nullptr, nullptr, 1 };
    OP_HIP(launch_argmax(a, 1, 0));
    OP_HIP(hipMemcpy(idx, di, 4, hipMemcpyDeviceToHost));
    return 0;
}

// the row-statistics kernel alone (score.hip).  The arguments are checked before a device is asked for.
extern "C" int nano_hip_op_score_rows(int device, const float *logits, uint32_t rows, uint32_t V, const uint32_t *targets, NanoHipTokenScore *out) {
    if (!logits || !out || !rows || !V) { nano_hip_set_error_("score_rows: null logits / out, or no rows / no vocabulary"); return NANO_HIP_EINVAL; }
    if (targets) for (uint32_t r = 0; r < rows; r++) if (targets[r] >= V) { nano_hip_set_error_("score_rows: target out of vocabulary"); return NANO_HIP_EINVAL; }
    int rc; if ((rc = begin(device))) return rc;
    DevBufs B;
    ScoreArgs a{};
    a.V = V; a.ntiles = score_tiles(V);
    a.logits = B.upload(logits, (size_t)rows * V);
    a.targets = targets ? B.upload(targets, rows) : nullptr;
    a.part = B.alloc<ScorePartial>((size_t)rows * a.ntiles); a.out = B.alloc<NanoHipTokenScore>(rows);
    OP_CHECK(a.logits && (a.targets || !targets) && a.part && a.out, "device alloc failed");
    OP_HIP(launch_score_rows(a, rows, 0));
    OP_HIP(hipMemcpy(out, a.out, (size_t)rows * sizeof(NanoHipTokenScore), hipMemcpyDeviceToHost));
    return 0;
}

// the row statistics and, behind them, the top-k selection (topk.hip) alone.  The arguments are checked before a device is asked for.
extern "C" int nano_hip_op_topk_rows(int device, const float *logits, uint32_t rows, uint32_t V, uint32_t k, const uint32_t *targets,
                                     NanoHipTokenScore *scores_out, NanoHipTopEntry *top_out) {
    if (!logits || !top_out || !rows || !V || !k) { nano_hip_set_error_("topk_rows: null logits / top_out, or no rows / no vocabulary / k of 0"); return NANO_HIP_EINVAL; }
    if (k > NANO_TOPK_MAX || k > V) { nano_hip_set_error_("topk_rows: k exceeds NANO_TOPK_MAX or the vocabulary"); return NANO_HIP_EINVAL; }
    if (rows > 65535u) { nano_hip_set_error_("topk_rows: more than 65535 rows"); return NANO_HIP_EINVAL; }
    if (targets) for (uint32_t r = 0; r < rows; r++) if (targets[r] >= V) { nano_hip_set_error_("topk_rows: target out of vocabulary"); return NANO_HIP_EINVAL; }
    int rc; if ((rc = begin(device))) return rc;
    DevBufs B;
    ScoreArgs a{};
    a.V = V; a.ntiles = score_tiles(V);
    a.logits = B.upload(logits, (size_t)rows * V);
    a.targets = targets ? B.upload(targets, rows) : nullptr;
    a.part = B.alloc<ScorePartial>((size_t)rows * a.ntiles); a.out = B.alloc<NanoHipTokenScore>(rows);
    TopkArgs t{};
    t.logits = a.logits; t.V = V; t.ntiles = a.ntiles; t.k = k; t.scores = a.out;
    t.part = B.alloc<unsigned long long>((size_t)rows * a.ntiles * k); t.out = B.alloc<NanoHipTopEntry>((size_t)rows * k);
    OP_CHECK(a.logits && (a.targets || !targets) && a.part && a.out && t.part && t.out, "device alloc failed");
    OP_HIP(launch_score_rows(a, rows, 0));
    OP_HIP(launch_topk_rows(t, rows, 0));
    OP_HIP(hipMemcpy(top_out, t.out, (size_t)rows * k * sizeof(NanoHipTopEntry), hipMemcpyDeviceToHost));
    if (scores_out) OP_HIP(hipMemcpy(scores_out, a.out, (size_t)rows * sizeof(NanoHipTokenScore), hipMemcpyDeviceToHost));
    return 0;
}

// the pool kernel alone (pool.hip), driven as a model drives it: the plan of nano_hip_step_rows_pool (pool_plan(), segments in slots
// 0 .. n_segs-1 from position 0), the rows uploaded in the order a call feeds them, one launch per pass on that pass's rows.  The
// arguments are checked before a device is asked for.
extern "C" int nano_hip_op_pool_rows(int device, const float *x, uint32_t rows, uint32_t n_embd, const float *w_final, const uint32_t *seg_count,
                                     uint32_t n_segs, const NanoHipPoolParams *p, uint32_t pass_cap, float *out) {
    if (!x || !w_final || !seg_count || !p || !out || !n_segs || !n_embd) { nano_hip_set_error_("pool_rows: null argument, or no segments / n_embd of 0"); return NANO_HIP_EINVAL; }
    if (p->pooling > NANO_POOL_MEAN || p->normalize > 1u || p->dim > n_embd || p->reserved) { nano_hip_set_error_("pool_rows: pooling / normalize / dim out of range, or reserved != 0"); return NANO_HIP_EINVAL; }
    if (!pass_cap || pass_cap > POOL_MAX_ROWS) { nano_hip_set_error_("pool_rows: pass_cap of 0 or above 256"); return NANO_HIP_EINVAL; }
    uint64_t sum = 0;
    uint32_t longest = 1;
    std::vector<NanoHipRowSeg> segs(n_segs);
    for (uint32_t i = 0; i < n_segs; i++) { segs[i] = NanoHipRowSeg{ i, 0u, seg_count[i], 0u }; sum += seg_count[i]; longest = seg_count[i] > longest ? seg_count[i] : longest; }
    if (sum != rows) { nano_hip_set_error_("pool_rows: rows is not the sum of the segments' counts"); return NANO_HIP_EINVAL; }
    PoolPlan pl;
    int rc; if ((rc = pool_plan(segs.data(), n_segs, pass_cap, longest, p->pooling, &pl))) return rc;
    if ((rc = begin(device))) return rc;
    const uint32_t dim = p->dim ? p->dim : n_embd, dpad = (dim + 3u) & ~3u;
    std::fill(out, out + (size_t)n_segs * dim, 0.0f);
    if (!rows) return 0;
    std::vector<float> fed((size_t)rows * n_embd);                          // caller row r is fed as row where[r]
    for (uint32_t r = 0; r < rows; r++) memcpy(fed.data() + (size_t)pl.where[r] * n_embd, x + (size_t)r * n_embd, (size_t)n_embd * 4);
    DevBufs B;
    PoolArgs a{};
    const float *dx = B.upload(fed.data(), fed.size());
    const uint32_t *dmap = B.upload(pl.map.data(), pl.map.size());
    a.w = B.upload(w_final, n_embd); a.acc = B.alloc<float>((size_t)n_segs * dpad); a.out = B.alloc<float>((size_t)n_segs * dim);
    OP_CHECK(dx && dmap && a.w && a.acc && a.out, "device alloc failed");
    OP_HIP(hipMemset(a.out, 0, (size_t)n_segs * dim * 4));
    a.x_stride = n_embd; a.lists = dmap + (size_t)pl.n_groups() * POOL_GROUP_WORDS;
    a.n_embd = n_embd; a.dim = dim; a.mean = p->pooling == NANO_POOL_MEAN; a.normalize = p->normalize;
    for (uint32_t ps = 0; ps < pl.n_passes(); ps++) {
        a.x = dx + (size_t)pl.pass_start[ps] * n_embd; a.rows_max = pl.pass_start[ps + 1] - pl.pass_start[ps];
        a.groups = dmap + (size_t)pl.group_start[ps] * POOL_GROUP_WORDS;
        OP_HIP(launch_pool_rows(a, pl.group_start[ps + 1] - pl.group_start[ps], 0));
    }
    OP_HIP(hipMemcpy(out, a.out, (size_t)n_segs * dim * 4, hipMemcpyDeviceToHost));
    return 0;
}

// the between-steps kernel of greedy decode with lookup drafts alone (lookup.hip).  The arguments are checked before a device is asked for.
extern "C" int nano_hip_op_lookup_step(int device, uint32_t *history, uint32_t n, const uint32_t *fed, const uint32_t *amax, uint32_t nb,
                                       const NanoHipLookupParams *p, uint32_t left, uint32_t seq_limit, uint32_t *record_out,
                                       uint32_t *next_tokens_out, uint32_t *next_pos_out) {
    if (!history || !p || !record_out || !next_tokens_out || !next_pos_out || (nb && (!fed || !amax))) { nano_hip_set_error_("lookup_step: null argument"); return NANO_HIP_EINVAL; }
    if (n == 0 || n > 65536u || nb > LOOKUP_MAX_ROWS) { nano_hip_set_error_("lookup_step: n outside 1 .. 65536, or more than 16 rows"); return NANO_HIP_EINVAL; }
    if (p->max_draft > LOOKUP_MAX_ROWS - 1 || p->ngram_max < 1 || p->ngram_max > LOOKUP_MAX_NGRAM || p->ngram_min < 1 || p->ngram_min > p->ngram_max) {
        nano_hip_set_error_("lookup_step: max_draft beyond 15, ngram_max outside 1 .. 4, or ngram_min outside 1 .. ngram_max"); return NANO_HIP_EINVAL;
    }
    int rc; if ((rc = begin(device))) return rc;
    DevBufs B;
    LookupArgs a{};
    a.cap = (n + LOOKUP_MAX_ROWS + 3u) & ~3u;
    a.hist = B.alloc<uint32_t>(a.cap);
    const uint32_t st[4] = { n, left, 0u, 0u };
    a.state = B.upload(st, 4);
    a.fed = nb ? B.upload(fed, nb) : nullptr; a.amax = nb ? B.upload(amax, nb) : nullptr; a.nb = nb;
    a.max_draft = p->max_draft; a.ngram_max = p->ngram_max; a.ngram_min = p->ngram_min; a.stop_token = p->stop_token; a.seq_limit = seq_limit;
    a.next_tokens = B.alloc<uint32_t>(LOOKUP_MAX_ROWS); a.next_pos = B.alloc<uint32_t>(LOOKUP_MAX_ROWS); a.record = B.alloc<uint32_t>(LOOKUP_REC_WORDS);
    OP_CHECK(a.hist && a.state && (!nb || (a.fed && a.amax)) && a.next_tokens && a.next_pos && a.record, "device alloc failed");
    OP_HIP(hipMemset(a.hist, 0xff, (size_t)a.cap * 4));
    OP_HIP(hipMemcpy(a.hist, history, (size_t)n * 4, hipMemcpyHostToDevice));
    OP_HIP(hipMemset(a.next_tokens, 0xff, LOOKUP_MAX_ROWS * 4)); OP_HIP(hipMemset(a.next_pos, 0xff, LOOKUP_MAX_ROWS * 4));
    OP_HIP(launch_lookup_step(a, 0));
    OP_HIP(hipMemcpy(record_out, a.record, LOOKUP_REC_WORDS * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(history, a.hist, (size_t)(n + LOOKUP_MAX_ROWS) * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(next_tokens_out, a.next_tokens, LOOKUP_MAX_ROWS * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(next_pos_out, a.next_pos, LOOKUP_MAX_ROWS * 4, hipMemcpyDeviceToHost));
    return 0;
}

// the two between-rounds launches of lookup drafts for several sequences alone (lookup_rows.hip).  The arguments are checked before a
// device is asked for; every device index the kernels form from them stays inside the buffers made here.
extern "C" int nano_hip_op_lookup_rows_round(int device, uint32_t n_seqs, uint32_t *const *histories, const uint32_t *n, const uint32_t *left,
                                             const uint32_t *slots, const uint32_t *fed, const uint32_t *amax, uint32_t n_rows,
                                             const uint32_t *row_start, const uint32_t *nb, const NanoHipLookupParams *p,
                                             uint32_t seq_limit, uint32_t max_seq_len, uint32_t *records_out, uint32_t *next_tokens_out,
                                             uint32_t *next_pos_out, uint32_t *next_slot_out, uint32_t *row_start_out) {
    constexpr uint32_t MAXQ = 64;
    if (!histories || !n || !left || !slots || !row_start || !nb || !p || !records_out || !next_tokens_out || !next_pos_out || !next_slot_out || !row_start_out ||
        (n_rows && (!fed || !amax))) { nano_hip_set_error_("lookup_rows_round: null argument"); return NANO_HIP_EINVAL; }
    if (n_seqs == 0 || n_seqs > MAXQ || !max_seq_len) { nano_hip_set_error_("lookup_rows_round: n_seqs outside 1 .. 64, or max_seq_len 0"); return NANO_HIP_EINVAL; }
    if (p->max_draft > LOOKUP_MAX_ROWS - 1 || p->ngram_max < 1 || p->ngram_max > LOOKUP_MAX_NGRAM || p->ngram_min < 1 || p->ngram_min > p->ngram_max) {
        nano_hip_set_error_("lookup_rows_round: max_draft beyond 15, ngram_max outside 1 .. 4, or ngram_min outside 1 .. ngram_max"); return NANO_HIP_EINVAL;
    }
    uint32_t n_max = 0, slot_max = 0;
    uint64_t seen = 0;
    for (uint32_t i = 0; i < n_seqs; i++) {
        if (!histories[i] || n[i] == 0 || n[i] > 65536u || nb[i] > LOOKUP_MAX_ROWS || (nb[i] && (uint64_t)row_start[i] + nb[i] > n_rows) || slots[i] >= MAXQ || (seen >> slots[i] & 1u)) {
            nano_hip_set_error_("lookup_rows_round: a null history, n outside 1 .. 65536, rows outside the pass, or a slot >= 64 or named twice"); return NANO_HIP_EINVAL;
        }
        seen |= 1ull << slots[i];
        n_max = std::max(n_max, n[i]); slot_max = std::max(slot_max, slots[i]);
    }
    int rc; if ((rc = begin(device))) return rc;
    DevBufs B;
    LookupRowsArgs a{};
    a.n_seqs = n_seqs;
    a.cap = (n_max + LOOKUP_MAX_ROWS + 4u) & ~3u;                           // (beyond n + 16: a full chunk's ids never end a sequence at the cap)
    const size_t hist_words = (size_t)(slot_max + 1u) * a.cap, out_rows = (size_t)n_seqs * LOOKUP_MAX_ROWS;
    a.hist = B.alloc<uint32_t>(hist_words);
    std::vector<uint32_t> st((size_t)n_seqs * LOOKUP_ST_WORDS, 0u);
    for (uint32_t i = 0; i < n_seqs; i++) { st[(size_t)i * LOOKUP_ST_WORDS + LOOKUP_ST_N] = n[i]; st[(size_t)i * LOOKUP_ST_WORDS + LOOKUP_ST_LEFT] = left[i]; }
    a.state = B.upload(st.data(), st.size());
    a.seq_slot = B.upload(slots, n_seqs);
    const uint32_t none = 0;
    a.fed = n_rows ? B.upload(fed, n_rows) : B.upload(&none, 1); a.amax = n_rows ? B.upload(amax, n_rows) : B.upload(&none, 1);
    a.row_start = B.upload(row_start, n_seqs); a.nb = B.upload(nb, n_seqs);
    a.max_draft = p->max_draft; a.ngram_max = p->ngram_max; a.ngram_min = p->ngram_min; a.stop_token = p->stop_token; a.seq_limit = seq_limit; a.max_seq_len = max_seq_len;
    a.stage = B.alloc<uint32_t>(out_rows); a.record = B.alloc<uint32_t>((size_t)n_seqs * LOOKUP_REC_WORDS);
    a.next_tokens = B.alloc<uint32_t>(out_rows); a.next_pos = B.alloc<uint32_t>(out_rows); a.next_slot = B.alloc<uint32_t>(out_rows);
    OP_CHECK(a.hist && a.state && a.seq_slot && a.fed && a.amax && a.row_start && a.nb && a.stage && a.record && a.next_tokens && a.next_pos && a.next_slot, "device alloc failed");
    OP_HIP(hipMemset(a.hist, 0xff, hist_words * 4));
    for (uint32_t i = 0; i < n_seqs; i++) OP_HIP(hipMemcpy(a.hist + (size_t)slots[i] * a.cap, histories[i], (size_t)n[i] * 4, hipMemcpyHostToDevice));
    OP_HIP(hipMemset(a.next_tokens, 0xff, out_rows * 4)); OP_HIP(hipMemset(a.next_pos, 0xff, out_rows * 4)); OP_HIP(hipMemset(a.next_slot, 0xff, out_rows * 4));
    OP_HIP(launch_lookup_rows_round(a, 0));
    OP_HIP(hipMemcpy(records_out, a.record, (size_t)n_seqs * LOOKUP_REC_WORDS * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n_seqs; i++) OP_HIP(hipMemcpy(histories[i], a.hist + (size_t)slots[i] * a.cap, (size_t)(n[i] + LOOKUP_MAX_ROWS) * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(next_tokens_out, a.next_tokens, out_rows * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(next_pos_out, a.next_pos, out_rows * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(next_slot_out, a.next_slot, out_rows * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(row_start_out, a.row_start, n_seqs * 4, hipMemcpyDeviceToHost));
    return 0;
}

// the between-steps kernel of greedy decode with a draft model alone (draft.hip): STAGE on fed[1 .. nb), then ACCEPT.  The arguments
// are checked before a device is asked for.
extern "C" int nano_hip_op_draft_round(int device, uint32_t *history, uint32_t n, const uint32_t *fed, const uint32_t *amax, uint32_t nb,
                                       const NanoHipDraftParams *p, uint32_t left, uint32_t seq_limit, uint32_t dn, uint32_t *record_out,
                                       uint32_t *next_tokens_out, uint32_t *next_pos_out) {
    if (!history || !p || !record_out || !next_tokens_out || !next_pos_out || (nb && (!fed || !amax))) { nano_hip_set_error_("draft_round: null argument"); return NANO_HIP_EINVAL; }
    if (n == 0 || n > 65536u || nb > LOOKUP_MAX_ROWS) { nano_hip_set_error_("draft_round: n outside 1 .. 65536, or more than 16 rows"); return NANO_HIP_EINVAL; }
    if (p->max_draft > LOOKUP_MAX_ROWS - 1 || dn > n - 1) { nano_hip_set_error_("draft_round: max_draft beyond 15, or dn beyond n - 1"); return NANO_HIP_EINVAL; }
    int rc; if ((rc = begin(device))) return rc;
    DevBufs B;
    DraftArgs a{};
    const uint32_t room = n + LOOKUP_MAX_ROWS, full = seq_limit < room ? seq_limit + 1u : room;      // the loop's history holds max_seq_len + 1 ids
    a.cap = ((full > n ? full : n) + 3u) & ~3u;
    a.hist = B.alloc<uint32_t>(a.cap > room ? a.cap : room);
    const uint32_t st[4] = { n, left, 0u, 0u };
    a.state = B.upload(st, 4);
    uint32_t *toks = B.alloc<uint32_t>(LOOKUP_MAX_ROWS);
    a.fed = toks; a.amax = nb ? B.upload(amax, nb) : nullptr; a.ids = nb > 1 ? B.upload(fed + 1, nb - 1) : nullptr; a.nb = nb;
    a.max_draft = p->max_draft; a.stop_token = p->stop_token; a.seq_limit = seq_limit; a.dn = dn;
    a.next_tokens = toks; a.next_pos = B.alloc<uint32_t>(LOOKUP_MAX_ROWS); a.record = B.alloc<uint32_t>(DRAFT_REC_WORDS);
    OP_CHECK(a.hist && a.state && toks && (!nb || a.amax) && (nb < 2 || a.ids) && a.next_pos && a.record, "device alloc failed");
    OP_HIP(hipMemset(a.hist, 0xff, (size_t)(a.cap > room ? a.cap : room) * 4));
    OP_HIP(hipMemcpy(a.hist, history, (size_t)n * 4, hipMemcpyHostToDevice));
    OP_HIP(hipMemset(toks, 0xff, LOOKUP_MAX_ROWS * 4)); OP_HIP(hipMemset(a.next_pos, 0xff, LOOKUP_MAX_ROWS * 4));
    if (nb) OP_HIP(hipMemcpy(toks, fed, 4, hipMemcpyHostToDevice));          // row 0: what the ACCEPT launch of the round before staged
    if (nb > 1) { a.role = DRAFT_ROLE_STAGE; OP_HIP(launch_draft_round(a, 0)); }
    a.role = DRAFT_ROLE_ACCEPT;
    OP_HIP(launch_draft_round(a, 0));
    OP_HIP(hipMemcpy(record_out, a.record, DRAFT_REC_WORDS * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(history, a.hist, (size_t)room * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(next_tokens_out, toks, LOOKUP_MAX_ROWS * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(next_pos_out, a.next_pos, LOOKUP_MAX_ROWS * 4, hipMemcpyDeviceToHost));
    return 0;
}

// what is wrong with the SHAPE fields of a fused-gemv descriptor (no pointer but norm_w / attn_part / resid_add, read as flags), or nullptr
static const char *fused_desc_shape_error(const NanoFusedGemvDesc &d) {
    if (d.kind > 2 || d.nseg == 0 || d.nseg > 3 || (d.kind == 2 && d.nseg != 2) || d.nb == 0 || d.nb > NANO_MAX_BATCH || d.n % 4) return "bad fused-gemv descriptor";
    if (d.quant == NANO_QUANT_Q80 && (!(d.gs == 32 || d.gs == 64 || d.gs == 128 || d.gs == 256) || d.n % d.gs || d.n % 16)) return "bad n / group size";
    for (uint32_t s = 0; s < d.nseg; s++) if (!d.rows[s]) return "missing weight tensor";
    if (d.kind == 2 && d.rows[0] != d.rows[1]) return "W1 / W3 row counts differ";
    if (d.resid_add && (d.kind != 1 || d.resid_add_stride < d.rows[0])) return "bad residual addend";
    if (d.attn_part && (!d.attn_nsplit || d.attn_nsplit > 8 || !d.attn_n_head || d.attn_n_head * d.attn_hd != d.n || d.kind != 1 || (d.nb > 8 && d.quant != NANO_QUANT_Q4K))) return "bad attention partials";
    return nullptr;
}

// ---- ONE path from a fused-gemv descriptor to the router's inputs: nano_hip_op_fused_gemv and the five plan queries below all start here,
// so that a query answers for the launch the operator issues.
// FusedLaunch = the arguments (shape and flag fields only: every pointer is the descriptor's HOST pointer, read as a flag; the operator
// replaces each with its device copy), the route with the step's switches, and the scratch the route may use -- sizes only, the pointers
// null: the operator allocates exactly these sizes, a query points every non-empty one at a flag (flag_scratch()).
//   Q80   the fragment-order activations of the batched routes and the quantized rows of ROUTE_GEMV_PREQ (gq bytes, gxs floats): always
//   Q4K   the staged groups of a several-sequence chunk launch (<= 8) or of the GEMM's tokens (r.q4x_bytes): from two sequences on
//   FP32  the operand-order activations of gemm_f32.hip (r.f32x_floats, f32_min_nb = 9): F32X_ASKED -- the caller asks for the GEMM route
//         (use_gemm) and nb > 8; F32X_MODEL -- as in a model: present, of any size; F32X_NONE -- never (the sliced route of every batch)
// use_gemm = 1 forces the fragment-order route of batched Q80 steps (quantizer launch + G6 MODE F / GC / G2) and lets FP32 ask for its
// GEMM (Q4K: the operator refuses it, the query does not read it); ordered = 1 is strict mode (the reference's group order in every
// kernel).  cus = 0: 256.
enum F32Scratch { F32X_NONE, F32X_ASKED, F32X_MODEL };
struct FusedLaunch {
    GemvArgs a;
    Q80Route r;
    size_t gq_bytes, gxs_floats;
};
static FusedLaunch fused_launch(const NanoFusedGemvDesc &d, uint32_t cus, F32Scratch f32x) {
    FusedLaunch L{};
    GemvArgs &a = L.a;
    Q80Route &r = L.r;
    for (uint32_t s = 0; s < d.nseg; s++) a.seg[s].rows = d.rows[s];
    a.nseg = d.nseg; a.n = d.n; a.gs = d.gs; a.nb = d.nb; a.cus = cus ? cus : 256u;
    a.epi = d.kind == 0 ? GEMV_EPI_STORE : d.kind == 1 ? GEMV_EPI_RESID : GEMV_EPI_SWIGLU;
    a.norm_w = d.norm_w;
    if (d.attn_part) { a.attn_part = d.attn_part; a.attn_nsplit = d.attn_nsplit; a.attn_n_head = d.attn_n_head; a.attn_hd = d.attn_hd; }
    // (operators and queries only, never a model's step: NANO_COMBINE_WAVE=0 keeps the combine's table form, as a model created under it does)
    if (d.attn_part) { const char *cwv = getenv("NANO_COMBINE_WAVE"); a.attn_table = (cwv && *cwv == '0') ? 1u : 0u; }
    if (d.resid_add) { a.resid_add = d.resid_add; a.resid_add_bstride = d.resid_add_stride; }
    a.ordered = d.ordered ? 1u : 0u;
    r.quant = d.quant; r.cus = (int)a.cus; r.mfma_min_nb = (d.use_gemm && d.quant == NANO_QUANT_Q80) ? 1u : 9u;
    if (d.quant == NANO_QUANT_Q80) {
        // token tiles of 16 as the batched kernels walk them: 1, 2 or 4 (G2's TT, gemm_q80.hip) -- 33..48 tokens run the four-tile
        // kernel, which loads the fragments of all four tiles (a model's buffers always hold 64 tokens); three tiles here left the
        // fourth tile's loads beyond the allocation
        const size_t n16 = (d.n + 15) & ~(size_t)15, tiles = (d.nb + 15) / 16, tt = tiles > 2 ? 4 : tiles;
        L.gq_bytes = tt * 16 * n16; L.gxs_floats = tt * 16 * (d.n / d.gs);
    }
    if (d.quant == NANO_QUANT_Q4K && d.nb > 1) r.q4x_bytes = (size_t)(d.nb > 8 ? d.nb : 8u) * ((d.n + 255) & ~(size_t)255);
    if (d.quant == NANO_QUANT_F32 && (f32x == F32X_MODEL || (f32x == F32X_ASKED && d.use_gemm && d.nb > 8))) {   // a shape the GEMM refuses keeps the slices
        r.f32_min_nb = 9u;
        r.f32x_floats = f32x == F32X_MODEL ? ~(size_t)0 : (size_t)((d.nb + 15) / 16) * 16 * ((d.n + 127) & ~(size_t)127);
    }
    return L;
}
// a query's pointers: one flag stands for every buffer the operator would allocate or upload -- compared with null, never followed
alignas(8) static uint8_t g_flag[8];
static void flag_scratch(FusedLaunch &L) {
    uint8_t *const flag = g_flag;
    if (L.gq_bytes) L.r.gq = reinterpret_cast<int8_t *>(flag);
    if (L.gxs_floats) L.r.gxs = reinterpret_cast<float *>(flag);
    if (L.r.q4x_bytes) L.r.q4x = flag;
    if (L.r.f32x_floats) L.r.f32x = reinterpret_cast<float *>(flag);
}
// The start of every plan query: the arguments checked, out zeroed, the launch as the operator builds it for `cus` compute units.
// Host arithmetic only from here on -- no device is touched, and of the descriptor's pointers only norm_w, attn_part and resid_add are
// looked at (null or not), never followed; `ordered` and `use_gemm` as flags.
static int query_begin(const NanoFusedGemvDesc *dp, uint32_t cus, uint32_t *out, uint32_t words, uint32_t quant, const char *not_quant,
                       F32Scratch f32x, FusedLaunch *L) {
    if (!dp || !out) { nano_hip_set_error_("null argument"); return NANO_HIP_EINVAL; }
    if (dp->quant != quant) { nano_hip_set_error_(not_quant); return NANO_HIP_EINVAL; }
    if (const char *msg = fused_desc_shape_error(*dp)) { nano_hip_set_error_(msg); return NANO_HIP_EINVAL; }
    memset(out, 0, words * sizeof(uint32_t));
    *L = fused_launch(*dp, cus, f32x);
    flag_scratch(*L);
    return 0;
}
// The end of the three GEMV-route queries: the first of the slices route_gemv_slices() cuts the batch into, planned by the format's
// planner -- the functions the router and the launcher themselves follow.  out = {fields(plan)..., launches, seqs_per_launch, takes = 1};
// a shape the slicer or the planner refuses leaves out as it is (zeros: takes = 0).
template <uint32_t WORDS, typename Plan, typename Fields>
static int report_first_slice(FusedLaunch &L, uint32_t *out, bool (*plan)(const GemvArgs &, Plan *), Fields fields) {
    GemvArgs &a = L.a;
    uint32_t per = 0, launches = 0;
    Plan p;
    if (!route_gemv_slices(L.r.quant, a, &per, &launches)) return 0;
    a.nb = per;
    if (launches > 1) a.tile_max = nullptr;                          // (gemv_slice(): a sliced launch writes no partials)
    if (!plan(a, &p)) return 0;
    const auto v = fields(p);
    static_assert(std::tuple_size<decltype(v)>::value + 3 <= WORDS, "the plan's fields and the three words of the slicing fit the query's output");
    memcpy(out, v.data(), sizeof(v));
    const uint32_t tail[3] = { launches, per, 1u };
    memcpy(out + v.size(), tail, sizeof(tail));
    return 0;
}
template <size_t N> using Words = std::array<uint32_t, N>;

// The FP32 launch route_projection() issues for a descriptor on the sliced route (its first slice when it cuts the batch).
// out = {role, B, nv, upw, rw, nw, grid, lds_bytes, launches, seqs_per_launch, takes, 0}; takes = 0: the router refuses the shape
// (hipErrorInvalidValue before any launch) and the other entries are 0.
extern "C" int nano_hip_f32_gemv_plan(const NanoFusedGemvDesc *dp, uint32_t cus, uint32_t out[NANO_F32_GEMV_PLAN_WORDS]) {
    FusedLaunch L;
    if (int rc = query_begin(dp, cus, out, NANO_F32_GEMV_PLAN_WORDS, NANO_QUANT_F32, "not an FP32 launch", F32X_NONE, &L)) return rc;
    return report_first_slice<NANO_F32_GEMV_PLAN_WORDS>(L, out, gemv_f32_plan, [](const F32GemvPlan &p) {
        return Words<8>{{ p.role, p.B, p.nv, p.upw, p.rw, p.nw, p.grid, p.lds_bytes }}; });
}

// The FP32 MFMA GEMM launch route_projection() issues for a descriptor of 9..64 sequences in a model (F32X_MODEL; nano_hip_op_fused_gemv
// reaches it with use_gemm = 1): route_kind() and the F32GemmPlan (kernels.h) the launcher consumes.
// out = {route, the plan's fields in the order of the struct, takes}; a descriptor the GEMM refuses reports the sliced route, takes = 1 and
// zeros for the plan (nano_hip_f32_gemv_plan reports those launches, and their refusals).
extern "C" int nano_hip_f32_gemm_plan(const NanoFusedGemvDesc *dp, uint32_t cus, uint32_t out[NANO_F32_GEMM_PLAN_WORDS]) {
    static_assert(sizeof(F32GemmPlan) == (NANO_F32_GEMM_PLAN_WORDS - 2) * sizeof(uint32_t), "the query reports every field of the plan");
    FusedLaunch L;
    if (int rc = query_begin(dp, cus, out, NANO_F32_GEMM_PLAN_WORDS, NANO_QUANT_F32, "not an FP32 launch", F32X_MODEL, &L)) return rc;
    const RouteKind k = route_kind(L.r, L.a);
    out[0] = (uint32_t)k;
    F32GemmPlan p{};
    if (k == ROUTE_F32_GEMM && gemm_f32_plan(L.a, &p)) memcpy(out + 1, &p, sizeof(p));
    out[NANO_F32_GEMM_PLAN_WORDS - 1] = 1u;
    return 0;
}

// The Q80 launch route_projection() issues for a descriptor: route_kind(), then for the routes that end in the Q80 GEMV kernels
// gemv_q80_plan() of the first slice.
// out = {route, kernel, role, gs, B, nv, upw, rw, nw, grid, lds_bytes, variant, pre, launches, seqs_per_launch, takes, cw}; the batched routes
// (G6 / G7 / G2 / GC) report the route, one launch of nb sequences and zeros for the kernel fields.  takes = 0: the router refuses the
// shape (hipErrorInvalidValue before any launch) and every other entry is 0.
extern "C" int nano_hip_q80_gemv_plan(const NanoFusedGemvDesc *dp, uint32_t cus, uint32_t out[NANO_Q80_GEMV_PLAN_WORDS]) {
    FusedLaunch L;
    if (int rc = query_begin(dp, cus, out, NANO_Q80_GEMV_PLAN_WORDS, NANO_QUANT_Q80, "not a Q80 launch", F32X_NONE, &L)) return rc;
    GemvArgs &a = L.a;
    const uint32_t k = (uint32_t)route_kind(L.r, a);
    if (route_takes_fragments((RouteKind)k)) {
        out[0] = k; out[13] = 1u; out[14] = a.nb; out[15] = 1u;
        return 0;
    }
    if (k == ROUTE_GEMV_PREQ) { a.xq_in = L.r.gq; a.xs_in = L.r.gxs; a.norm_w = nullptr; }      // (as route_projection() hands it on)
    // (word 16, behind takes: the plan's cw -- the first 16 words are what they were)
    return report_first_slice<NANO_Q80_GEMV_PLAN_WORDS>(L, out, gemv_q80_plan, [k, out](const Q80GemvPlan &p) {
        out[16] = p.cw;
        return Words<13>{{ k, p.kernel, p.role, p.gs, p.B, p.nv, p.upw, p.rw, p.nw, p.grid, p.lds_bytes, p.variant, p.pre }}; });
}

// The batched Q80 launch route_projection() issues for a descriptor: route_kind() and the Q80GemmPlan (kernels.h) it hands to the launcher.
// out = {route, the plan's fields in the order of the struct, takes}; a descriptor whose route ends in the GEMV kernels reports the route,
// takes = 1 and zeros for the plan (nano_hip_q80_gemv_plan reports those launches, and their refusals).
extern "C" int nano_hip_q80_gemm_plan(const NanoFusedGemvDesc *dp, uint32_t cus, uint32_t out[NANO_Q80_GEMM_PLAN_WORDS]) {
    static_assert(sizeof(Q80GemmPlan) == (NANO_Q80_GEMM_PLAN_WORDS - 2) * sizeof(uint32_t), "the query reports every field of the plan");
    FusedLaunch L;
    if (int rc = query_begin(dp, cus, out, NANO_Q80_GEMM_PLAN_WORDS, NANO_QUANT_Q80, "not a Q80 launch", F32X_NONE, &L)) return rc;
    Q80GemmPlan p{};
    out[0] = (uint32_t)route_kind(L.r, L.a, &p);
    memcpy(out + 1, &p, sizeof(p));
    out[NANO_Q80_GEMM_PLAN_WORDS - 1] = 1u;
    return 0;
}

// The Q4K launch route_projection() issues for a descriptor: route_kind(), then for the GEMV route gemv_q4k_plan() of the first slice.
// A launch of one STORE tensor is planned as the step's classifier asks for it: with a request for arg-max partials.
// out = {route, kernel, role, B, nv, ipt, d, loop, rounds, wg[3], rw, nthr, grid, lds_bytes, pre, quant_rows, quant_nthr, quant_nv,
// partials, launches, seqs_per_launch, takes}; the GEMM route reports the route, one launch of nb sequences and zeros for the kernel
// fields.  takes = 0: the router refuses the shape (hipErrorInvalidValue before any launch) and every other entry is 0.
extern "C" int nano_hip_q4k_gemv_plan(const NanoFusedGemvDesc *dp, uint32_t cus, uint32_t out[NANO_Q4K_GEMV_PLAN_WORDS]) {
    static float asked;                             // stands for the partials' buffer: compared with null, never followed
    FusedLaunch L;
    if (int rc = query_begin(dp, cus, out, NANO_Q4K_GEMV_PLAN_WORDS, NANO_QUANT_Q4K, "not a Q4K launch", F32X_NONE, &L)) return rc;
    GemvArgs &a = L.a;
    if (a.epi == GEMV_EPI_STORE && a.nseg == 1) a.tile_max = &asked;
    const uint32_t k = (uint32_t)route_kind(L.r, a);
    if (k == ROUTE_Q4K_GEMM) {
        out[0] = k; out[21] = 1u; out[22] = a.nb; out[23] = 1u;
        return 0;
    }
    route_fill(L.r, a);
    return report_first_slice<NANO_Q4K_GEMV_PLAN_WORDS>(L, out, gemv_q4k_plan, [k](const Q4kGemvPlan &p) {
        return Words<21>{{ k, p.kernel, p.role, p.B, p.nv, p.ipt, p.d, p.loop, p.rounds, p.wg[0], p.wg[1], p.wg[2], p.rw, p.nthr, p.grid,
                           p.lds_bytes, p.pre, p.quant_rows, p.quant_nthr, p.quant_nv, p.partials }}; });
}

// the weight tensors of a descriptor -> device copies in the arguments' segments
static int upload_weights(DevBufs &B, const NanoFusedGemvDesc &d, GemvArgs &a) {
    const size_t bpl = (d.n + 255) / 256;
    for (uint32_t s = 0; s < d.nseg; s++) {
        const size_t rows = d.rows[s];
        if (!d.w[s]) { nano_hip_set_error_("missing weight tensor"); return NANO_HIP_EINVAL; }
        if (d.quant == NANO_QUANT_Q80) {
            a.seg[s].w = B.upload(reinterpret_cast<const int8_t *>(d.w[s]), rows * d.n);
            a.seg[s].ws = B.upload(d.ws[s], rows * d.n / d.gs);
            OP_CHECK(a.seg[s].ws, "device alloc failed");
        } else if (d.quant == NANO_QUANT_Q4K) a.seg[s].w = B.upload(reinterpret_cast<const uint8_t *>(d.w[s]), rows * bpl * 160);
        else a.seg[s].w = B.upload(reinterpret_cast<const float *>(d.w[s]), rows * d.n);
        OP_CHECK(a.seg[s].w, "device alloc failed");
    }
    return 0;
}

// One fused GEMV launch as enqueue_step() issues it (backend_step.hip): the role-specialised kernels on caller-chosen inputs, through the
// step's own router (route.hip).
// With d.tile_max the launch is the step's classifier launch where route_partials() (route.hip, enqueue_classifier's own question) says
// so: it is handed the caller's partials buffer -- uploaded whole, read back whole -- and writes nb x route_partials() pairs into it as
// into the step's buffer; *d.ntiles_out reports that count (0: not asked).  With d.argmax_out the arg-max kernel runs behind the launch
// as a MODE_ARGMAX step builds it (backend_step.hip): over the launch's output, from the partials if the launch was asked for them.
extern "C" int nano_hip_op_fused_gemv(int device, const NanoFusedGemvDesc *dp) {
    int rc; if ((rc = begin(device))) return rc;
    if (!dp) { nano_hip_set_error_("null descriptor"); return NANO_HIP_EINVAL; }
    const NanoFusedGemvDesc &d = *dp;
    if (!d.out) { nano_hip_set_error_("bad fused-gemv descriptor"); return NANO_HIP_EINVAL; }
    if (!d.x && !d.attn_part) { nano_hip_set_error_("no activation"); return NANO_HIP_EINVAL; }
    if (const char *msg = fused_desc_shape_error(d)) { nano_hip_set_error_(msg); return NANO_HIP_EINVAL; }
    if (d.attn_part && !d.attn_ml) { nano_hip_set_error_("bad attention partials"); return NANO_HIP_EINVAL; }
    hipDeviceProp_t prop; OP_HIP(hipGetDeviceProperties(&prop, device));
    FusedLaunch L = fused_launch(d, (uint32_t)prop.multiProcessorCount, F32X_ASKED);
    GemvArgs &a = L.a;
    Q80Route &r = L.r;
    DevBufs B;
    if (int rc2 = upload_weights(B, d, a)) return rc2;
    uint32_t rows_total = 0;
    for (uint32_t s = 0; s < d.nseg; s++) if (d.kind != 2 || s == 0) rows_total += d.rows[s];
    // out_slots / out_stride (operator tests): out holds more sequence slots than nb and more floats per slot than rows -- guard
    // elements that go to the device and come back with the result, so the caller sees every element the launch wrote
    const uint32_t slots = d.out_slots ? d.out_slots : d.nb, stride = d.out_stride ? d.out_stride : rows_total;
    if (slots < d.nb || stride < rows_total) { nano_hip_set_error_("out_slots / out_stride smaller than the result"); return NANO_HIP_EINVAL; }
    float *dout = B.upload(d.out, (size_t)slots * stride);          // (kind 1: the residual stream; otherwise overwritten)
    OP_CHECK(dout, "device alloc failed");
    uint32_t off = 0;
    for (uint32_t s = 0; s < d.nseg; s++) {
        a.seg[s].out = d.kind == 2 ? dout : dout + off;
        a.seg[s].out_bstride = stride;
        if (d.kind != 2) off += d.rows[s];
    }
    // every host pointer fused_launch() left in the arguments as a flag -> its device copy
    if (d.x) { a.xin = B.upload(d.x, (size_t)d.nb * d.n); OP_CHECK(a.xin, "device alloc failed"); a.xin_bstride = d.n; }
    if (d.norm_w) { a.norm_w = B.upload(d.norm_w, d.n); OP_CHECK(a.norm_w, "device alloc failed"); }
    if (d.attn_part) {
        a.attn_part = B.upload(d.attn_part, (size_t)d.nb * d.attn_nsplit * d.n);
        a.attn_ml = B.upload(d.attn_ml, (size_t)d.nb * d.attn_n_head * d.attn_nsplit * 2);
        OP_CHECK(a.attn_part && a.attn_ml, "device alloc failed");
        if (!a.xin) { a.xin = a.attn_part; a.xin_bstride = d.n; }     // never read: the prologue combines the partials
    }
    if (d.resid_add) { a.resid_add = B.upload(d.resid_add, (size_t)d.nb * d.resid_add_stride); OP_CHECK(a.resid_add, "device alloc failed"); }
    // the scratch, exactly as fused_launch() sizes it
    if (L.gq_bytes) { r.gq = B.alloc<int8_t>(L.gq_bytes); r.gxs = B.alloc<float>(L.gxs_floats); OP_CHECK(r.gq && r.gxs, "device alloc failed"); }
    if (r.q4x_bytes) { r.q4x = B.alloc<uint8_t>(r.q4x_bytes); OP_CHECK(r.q4x, "device alloc failed"); }
    if (r.f32x_floats) { r.f32x = B.alloc<float>(r.f32x_floats); OP_CHECK(r.f32x, "device alloc failed"); }
    if (d.use_gemm && d.quant != NANO_QUANT_F32 && (d.quant != NANO_QUANT_Q80 || !route_takes_fragments(route_kind(r, a)))) { nano_hip_set_error_("the batched GEMM route does not take this launch"); return NANO_HIP_EINVAL; }
    if (d.route_out) *d.route_out = (uint32_t)route_kind(r, a);
    // the step's arg-max partials (enqueue_classifier): asked for where route_partials() says so, into the caller's buffer
    float *dtm = nullptr;
    uint32_t ntiles = 0;
    const size_t tm_floats = (size_t)d.tile_slots * d.tile_pairs * 2;
    if (d.tile_max) {
        if (d.tile_slots < d.nb) { nano_hip_set_error_("tile_slots smaller than the batch"); return NANO_HIP_EINVAL; }
        dtm = tm_floats ? B.upload(d.tile_max, tm_floats) : B.alloc<float>(1);
        OP_CHECK(dtm, "device alloc failed");
        if (const uint32_t n = route_partials(r, a)) {
            if (d.tile_pairs < n) { nano_hip_set_error_("tile_pairs smaller than the launch's partials"); return NANO_HIP_EINVAL; }
            a.tile_max = dtm; ntiles = n;
        }
    }
    if (d.ntiles_out) *d.ntiles_out = ntiles;
    uint32_t *damax = nullptr;
    if (d.argmax_out) { damax = B.alloc<uint32_t>(d.nb); OP_CHECK(damax, "device alloc failed"); }
    const hipError_t e = route_projection(r, a, 0);
    OP_HIP(e);
    if (damax) {                                                    // (backend_step.hip MODE_ARGMAX: no token / trace / embedding state)
        ArgmaxArgs aa{ dout, rows_total, stride, damax, nullptr, nullptr, nullptr, nullptr, d.nb, ntiles ? dtm : nullptr, ntiles };
        OP_HIP(launch_argmax(aa, d.nb, 0));
    }
    OP_HIP(hipDeviceSynchronize());
    OP_HIP(hipMemcpy(d.out, dout, (size_t)slots * stride * 4, hipMemcpyDeviceToHost));
    if (dtm && tm_floats) OP_HIP(hipMemcpy(d.tile_max, dtm, tm_floats * 4, hipMemcpyDeviceToHost));
    if (damax) OP_HIP(hipMemcpy(d.argmax_out, damax, (size_t)d.nb * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- the LoRA side-branch launches (lora.hip), LoraRowsArgs filled as enqueue_step() fills them (backend_step.hip), with row b in "slot" b of
// a descriptor array built from row_adapter (layer 0 of one-layer adapters).  Two front ends, each with its own argument check before a
// device is asked for, and one body: the single-module operators are one adapter with every row bound to it.
static const char *lora_desc_error(const NanoLoraOpDesc *d, bool qkv) {
    if (!d || !d->x || !d->a[0] || !d->b[0] || !d->q) return "lora: null argument";
    if (qkv && (!d->norm_w || !d->a[1] || !d->b[1] || !d->a[2] || !d->b[2] || !d->pos || !d->kraw || !d->v)) return "lora: null argument";
    if (d->nb == 0 || d->nb > NANO_MAX_BATCH) return "lora: nb outside 1 .. NANO_MAX_BATCH";
    if (const char *msg = lora_shape_error(d->E, d->rank)) return msg;
    if (d->q_floats < (uint64_t)d->nb * d->E) return "lora: q smaller than nb rows of E";
    if (!qkv) return nullptr;
    if (d->KD == 0 || d->k_floats < (uint64_t)d->nb * d->KD) return "lora: KD of 0, or kraw smaller than nb rows of KD";
    for (uint32_t b = 0; b < d->nb; b++) {
        if (d->pos[b] >= d->S) return "lora: position beyond S";
        if ((uint64_t)b * d->v_bstride + ((uint64_t)d->pos[b] + 1) * d->KD > d->v_floats) return "lora: a v row beyond v_floats";
    }
    return nullptr;
}
static const char *lora_rows_desc_error(const NanoLoraRowsOpDesc *d, bool qkv) {
    if (!d || !d->x || !d->q || !d->adapters || !d->row_adapter) return "lora rows: null argument";
    if (qkv && (!d->norm_w || !d->pos || !d->kraw || !d->v)) return "lora rows: null argument";
    if (d->nb == 0 || d->nb > NANO_MAX_BATCH) return "lora rows: nb outside 1 .. NANO_MAX_BATCH";
    if (d->n_adapters == 0 || d->n_adapters > NANO_LORA_TABLE_MAX) return "lora rows: n_adapters outside 1 .. NANO_LORA_TABLE_MAX";
    for (uint32_t i = 0; i < d->n_adapters; i++) {
        const NanoLoraAdapter &ad = d->adapters[i];
        if (!ad.a[0] || !ad.b[0] || (qkv && (!ad.a[1] || !ad.b[1] || !ad.a[2] || !ad.b[2]))) return "lora rows: null argument";
        if (const char *msg = lora_shape_error(d->E, ad.rank)) return msg;
    }
    for (uint32_t b = 0; b < d->nb; b++)
        if (d->row_adapter[b] != NANO_LORA_NONE && d->row_adapter[b] >= d->n_adapters) return "lora rows: row_adapter names no adapter";
    if (d->q_floats < (uint64_t)d->nb * d->E) return "lora rows: q smaller than nb rows of E";
    if (!qkv) return nullptr;
    if (d->KD == 0 || d->k_floats < (uint64_t)d->nb * d->KD) return "lora rows: KD of 0, or kraw smaller than nb rows of KD";
    for (uint32_t b = 0; b < d->nb; b++) {
        if (d->pos[b] >= d->S) return "lora rows: position beyond S";
        if ((uint64_t)b * d->v_bstride + ((uint64_t)d->pos[b] + 1) * d->KD > d->v_floats) return "lora rows: a v row beyond v_floats";
    }
    return nullptr;
}
// the body behind both: d passed its front end's check
static int lora_run(int device, const NanoLoraRowsOpDesc *d, bool qkv) {
    int rc; if ((rc = begin(device))) return rc;
    const size_t E = d->E, KD = d->KD;
    DevBufs B;
    std::vector<LoraSlotDesc> ent(d->n_adapters);
    uint32_t max_rank = 0;
    for (uint32_t i = 0; i < d->n_adapters; i++) {
        const NanoLoraAdapter &ad = d->adapters[i];
        const size_t r = ad.rank;
        LoraSlotDesc &t = ent[i];
        t = LoraSlotDesc{};
        t.rank = ad.rank; t.alpha = ad.alpha;
        if (ad.rank > max_rank) max_rank = ad.rank;
        if (qkv) {
            t.t[0] = B.upload(ad.a[0], r * E); t.t[1] = B.upload(ad.b[0], E * r); t.t[2] = B.upload(ad.a[1], r * E); t.t[3] = B.upload(ad.b[1], KD * r);
            t.t[4] = B.upload(ad.a[2], r * E); t.t[5] = B.upload(ad.b[2], KD * r);
            OP_CHECK(t.t[0] && t.t[1] && t.t[2] && t.t[3] && t.t[4] && t.t[5], "device alloc failed");
        } else {
            t.t[6] = B.upload(ad.a[0], r * E); t.t[7] = B.upload(ad.b[0], E * r);
            OP_CHECK(t.t[6] && t.t[7], "device alloc failed");
        }
    }
    std::vector<LoraSlotDesc> rows(d->nb);
    for (uint32_t b = 0; b < d->nb; b++) rows[b] = d->row_adapter[b] == NANO_LORA_NONE ? LoraSlotDesc{} : ent[d->row_adapter[b]];
    LoraRowsArgs la{};
    la.desc = B.upload(rows.data(), rows.size());
    la.x = B.upload(d->x, d->nb * E);
    la.q = B.upload(d->q, (size_t)d->q_floats);
    OP_CHECK(la.desc && la.x && la.q, "device alloc failed");
    la.E = d->E; la.KD = d->KD; la.layer = 0; la.slot0 = 0; la.slot_stride = 1; la.max_rank = max_rank;
    if (qkv) {
        la.norm_w = B.upload(d->norm_w, E);
        la.kraw = B.upload(d->kraw, (size_t)d->k_floats); la.v = B.upload(d->v, (size_t)d->v_floats);
        la.pos = B.upload(d->pos, d->nb); la.v_bstride = d->v_bstride;
        OP_CHECK(la.norm_w && la.kraw && la.v && la.pos, "device alloc failed");
    }
    OP_HIP(qkv ? launch_lora_qkv_rows(la, d->nb, 0) : launch_lora_o_rows(la, d->nb, 0));
    OP_HIP(hipDeviceSynchronize());
    OP_HIP(hipMemcpy(d->q, la.q, (size_t)d->q_floats * 4, hipMemcpyDeviceToHost));
    if (qkv) {
        OP_HIP(hipMemcpy(d->kraw, la.kraw, (size_t)d->k_floats * 4, hipMemcpyDeviceToHost));
        OP_HIP(hipMemcpy(d->v, la.v, (size_t)d->v_floats * 4, hipMemcpyDeviceToHost));
    }
    return 0;
}
static int lora_op(int device, const NanoLoraOpDesc *d, bool qkv) {
    if (const char *msg = lora_desc_error(d, qkv)) { nano_hip_set_error_(msg); return NANO_HIP_EINVAL; }
    const NanoLoraAdapter ad{ d->rank, d->alpha, { d->a[0], d->a[1], d->a[2] }, { d->b[0], d->b[1], d->b[2] } };
    const std::vector<uint32_t> rows(d->nb, 0u);
    NanoLoraRowsOpDesc r{};
    r.E = d->E; r.KD = d->KD; r.nb = d->nb; r.S = d->S; r.v_bstride = d->v_bstride; r.n_adapters = 1;
    r.x = d->x; r.norm_w = d->norm_w; r.adapters = &ad; r.row_adapter = rows.data(); r.pos = d->pos;
    r.q = d->q; r.kraw = d->kraw; r.v = d->v; r.q_floats = d->q_floats; r.k_floats = d->k_floats; r.v_floats = d->v_floats;
    return lora_run(device, &r, qkv);
}
static int lora_rows_op(int device, const NanoLoraRowsOpDesc *d, bool qkv) {
    if (const char *msg = lora_rows_desc_error(d, qkv)) { nano_hip_set_error_(msg); return NANO_HIP_EINVAL; }
    return lora_run(device, d, qkv);
}
extern "C" int nano_hip_op_lora_qkv(int device, const NanoLoraOpDesc *d) { return lora_op(device, d, true); }
extern "C" int nano_hip_op_lora_o(int device, const NanoLoraOpDesc *d) { return lora_op(device, d, false); }
extern "C" int nano_hip_op_lora_qkv_rows(int device, const NanoLoraRowsOpDesc *d) { return lora_rows_op(device, d, true); }
extern "C" int nano_hip_op_lora_o_rows(int device, const NanoLoraRowsOpDesc *d) { return lora_rows_op(device, d, false); }

// ---- ONE path from an attention-decode descriptor to the launch's arguments: nano_hip_op_attention_decode, the fused q | k | v + attention
// operator and its plan query start here.  Every shape field as enqueue_step() fills it (backend_step.hip); of the pointers q_norm / k_norm
// arrive as the descriptor's HOST pointers, read as flags -- an operator replaces them, and sets every other pointer, with device copies.
static AttnArgs attn_launch(const NanoAttnDecodeDesc &d, uint32_t nsplit) {
    AttnArgs a{};
    a.q_norm = d.q_norm; a.k_norm = d.k_norm;
    a.nsplit = nsplit; a.range_hint = d.range_hint;
    a.layer = d.layer; a.n_layer = d.n_layer; a.S = d.S; a.hd = d.hd; a.n_head = d.n_head; a.n_kv_head = d.n_kv_head;
    a.q_dim = d.n_head * d.hd; a.kv_dim = d.n_kv_head * d.hd; a.rope_qwen3 = d.rope_qwen3 ? 1u : 0u; a.is_causal = 1;
    a.cache_bstride_rows = d.chunk ? 0u : d.n_layer * d.S; a.fixed_range = 0;
    a.kv_half = d.kv_half;                                          // the element format: 0 FP32, 1 FP16, 2 FP8 (kernels.h KV_FMT_*)
    if (d.pool_rows) { a.pt_stride = d.pt_stride; a.pt_bstride = d.chunk ? 0u : d.pt_stride; a.pool_rows = d.pool_rows; }
    return a;
}
static uint32_t attn_desc_nsplit(const NanoAttnDecodeDesc &d) { return d.nsplit ? d.nsplit : attention_nsplit(d.range_hint, d.hd); }

// One decode attention launch as enqueue_step() issues it without the fused q|k|v launch (backend_step.hip: the AttnArgs block before
// launch_attention), or with `chunk` the two passes of a batched prefill chunk; split partials are combined by the batched / prefill
// combine.  The plan that ran comes from attention_plan(), the function the launcher itself follows.
extern "C" int nano_hip_op_attention_decode(int device, const NanoAttnDecodeDesc *dp) {
    int rc; if ((rc = begin(device))) return rc;
    if (!dp) { nano_hip_set_error_("null descriptor"); return NANO_HIP_EINVAL; }
    const NanoAttnDecodeDesc &d = *dp;
#define OP_ARG(cond, msg) do { if (!(cond)) { nano_hip_set_error_(msg); return NANO_HIP_EINVAL; } } while (0)
    OP_ARG(d.nb >= 1 && d.nb <= NANO_MAX_BATCH, "nb out of range");
    OP_ARG(d.n_kv_head && d.n_head && d.n_head % d.n_kv_head == 0 && d.hd >= 4 && d.hd % 4 == 0 && d.hd <= 256, "bad attention shape");
    OP_ARG(d.n_layer && d.layer < d.n_layer && d.S, "bad layer / S");
    OP_ARG(d.q && d.k && d.pos && d.rope_cos && d.rope_sin && d.k_cache && d.v_cache && d.out, "missing tensor");
    OP_ARG(!d.q_norm == !d.k_norm, "q_norm and k_norm go together");
    const uint32_t nb = d.nb, QD = d.n_head * d.hd, KD = d.n_kv_head * d.hd, half = d.hd / 2;
    uint32_t maxpos = 0;
    for (uint32_t b = 0; b < nb; b++) {
        maxpos = d.pos[b] > maxpos ? d.pos[b] : maxpos;
        OP_ARG(!d.chunk || d.pos[b] == d.pos[0] + b, "chunk: positions must be consecutive");
    }
    OP_ARG(d.range_hint >= maxpos + 1 && d.range_hint <= d.S, "range_hint must cover max(pos) + 1 and stay <= S");
    const uint32_t nsplit = attn_desc_nsplit(d);
    OP_ARG(nsplit >= 1 && nsplit <= ATTN_MAX_NSPLIT, "nsplit out of range");
    OP_ARG(!d.want_frag || (nsplit == 1 && d.hd % 64 == 0 && d.xf && d.xsf), "fragment output: nsplit 1 and hd % 64 == 0 only");
    const bool paged = d.pool_rows != 0;
    const uint32_t seqs = d.chunk ? 1u : nb;                       // cache slots / page-table rows
    OP_ARG(d.kv_half <= KV_FMT_FP8, "kv_half: 0 (FP32), 1 (FP16) or 2 (FP8 e4m3) cache elements");
    const size_t esz = kv_fmt_bytes(d.kv_half);
    const size_t cache_elems = paged ? (size_t)d.n_layer * d.pool_rows * KD : (size_t)seqs * d.n_layer * d.S * KD;
    std::vector<uint32_t> kvrow(nb, 0u);
    if (paged) {
        OP_ARG(d.pool_rows % 64 == 0 && d.pt_rows && d.pt_stride, "paged: pool_rows % 64, page table");
        for (size_t i = 0; i < (size_t)seqs * d.pt_stride; i++)
            OP_ARG(d.pt_rows[i] == 0xffffffffu || (d.pt_rows[i] % 64 == 0 && d.pt_rows[i] < d.pool_rows && d.pool_rows - d.pt_rows[i] >= 64), "paged: a page-table entry lies outside the pool");
        for (uint32_t b = 0; b < nb; b++) {                        // (as the embed kernel stages it)
            const uint32_t blk = d.pos[b] >> 6, e = d.pt_rows[(size_t)(d.chunk ? 0 : b) * d.pt_stride + (blk < d.pt_stride ? blk : 0)];
            OP_ARG(blk < d.pt_stride && e != 0xffffffffu, "paged: no page holds pos");
            kvrow[b] = e + (d.pos[b] & 63u);
        }
    }
    std::vector<float> rope_cur((size_t)nb * 2 * half);             // rope_cur[b] = { cos[pos[b]], sin[pos[b]] } (launch_embed)
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t i = 0; i < half; i++) {
            rope_cur[(size_t)b * 2 * half + i] = d.rope_cos[(size_t)d.pos[b] * half + i];
            rope_cur[(size_t)b * 2 * half + half + i] = d.rope_sin[(size_t)d.pos[b] * half + i];
        }
    DevBufs B;
    float *dq = B.upload(d.q, (size_t)nb * QD), *dk = B.upload(d.k, (size_t)nb * KD);
    uint32_t *dpos = B.upload(d.pos, nb);
    float *dcos = B.upload(d.rope_cos, (size_t)d.S * half), *dsin = B.upload(d.rope_sin, (size_t)d.S * half), *dcur = B.upload(rope_cur.data(), rope_cur.size());
    unsigned char *dkc = B.upload(reinterpret_cast<const unsigned char *>(d.k_cache), cache_elems * esz);
    unsigned char *dvc = B.upload(reinterpret_cast<const unsigned char *>(d.v_cache), cache_elems * esz);
    float *dout = B.alloc<float>((size_t)nb * QD), *dpart = B.alloc<float>((size_t)nb * nsplit * QD), *dml = B.alloc<float>((size_t)nb * d.n_head * nsplit * 2);
    OP_CHECK(dq && dk && dpos && dcos && dsin && dcur && dkc && dvc && dout && dpart && dml, "device alloc failed");
    AttnArgs a = attn_launch(d, nsplit);
    if (d.q_norm) { a.q_norm = B.upload(d.q_norm, d.hd); a.k_norm = B.upload(d.k_norm, d.hd); OP_CHECK(a.q_norm && a.k_norm, "device alloc failed"); }
    if (d.kv_half && d.vraw) { a.vraw = B.upload(d.vraw, (size_t)nb * KD); OP_CHECK(a.vraw, "device alloc failed"); }
    const size_t ntile = (nb + 15) / 16, ng = QD / 64;
    if (d.want_frag) {
        a.xf_out = B.alloc<int8_t>(ntile * ng * 1024); a.xsf_out = B.alloc<float>(ntile * ng * 16);
        OP_CHECK(a.xf_out && a.xsf_out, "device alloc failed");
        OP_HIP(hipMemset(a.xf_out, 0, ntile * ng * 1024)); OP_HIP(hipMemset(a.xsf_out, 0, ntile * ng * 16 * 4));
    }
    if (paged) {
        a.pt_rows = B.upload(d.pt_rows, (size_t)seqs * d.pt_stride); a.kvrow = B.upload(kvrow.data(), nb);
        OP_CHECK(a.pt_rows && a.kvrow, "device alloc failed");
    }
    a.q = dq; a.kraw = dk; a.kcache = reinterpret_cast<float *>(dkc); a.vcache = reinterpret_cast<float *>(dvc); a.pos = dpos;
    a.rope_cos = dcos; a.rope_sin = dsin; a.rope_cur = dcur; a.out = dpart; a.ml = dml; a.xba_out = dout;
    uint32_t plan[2][10] = {};
    auto record = [&](const AttnArgs &x, uint32_t *row) -> bool {
        AttnPlan p;
        if (!attention_plan(x, nb, &p)) return false;
        const uint32_t v[10] = { p.mode, p.lpr, p.qv, p.kvm, p.npt, p.w16, p.paged, p.kv_half, p.nsplit, p.kv_log2 != 0xffffffffu ? 1u : 0u };
        memcpy(row, v, sizeof(v));
        return true;
    };
    if (d.chunk) {                                                   // batched prefill, pass 1: every token's k row into the cache
        a.prep_only = 1;
        OP_ARG(record(a, plan[0]), "attention arguments refused");
        OP_HIP(launch_attention(a, nb, 0));
        a.prep_only = 0;
    }
    OP_ARG(record(a, plan[d.chunk ? 1 : 0]), "attention arguments refused");
    OP_HIP(launch_attention(a, nb, 0));
    if (nsplit > 1) OP_HIP(launch_attn_combine_tokens(dpart, dml, dout, d.n_head, d.hd, nsplit, nb, nullptr, nullptr, 0));
    OP_HIP(hipDeviceSynchronize());
    OP_HIP(hipMemcpy(d.out, dout, (size_t)nb * QD * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(d.k_cache, dkc, cache_elems * esz, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(d.v_cache, dvc, cache_elems * esz, hipMemcpyDeviceToHost));
    if (d.want_frag) {
        OP_HIP(hipMemcpy(d.xf, a.xf_out, ntile * ng * 1024, hipMemcpyDeviceToHost));
        OP_HIP(hipMemcpy(d.xsf, a.xsf_out, ntile * ng * 16 * 4, hipMemcpyDeviceToHost));
    }
    if (d.plan) memcpy(d.plan, plan, sizeof(plan));
#undef OP_ARG
    return 0;
}

// ---- the two fused one-sequence launches: plan queries and operators --------------------------------------------------------------------
// ONE resolution each, shared by the query and the operator: the descriptors through fused_launch() / attn_launch() above, the conditions
// enqueue_step() (backend_step.hip) puts in front of the launch -- the projection's route is the one GEMV (Q4K: the one Q4K) launch -- and
// the launcher's own plan.  Pointers the launch needs and a query does not have stand as flags (compared with null, never followed); the
// operator replaces every one with its device copy.  false: the step issues the plain launches.
static bool qkv_attn_fused_resolve(const NanoFusedGemvDesc &g, const NanoAttnDecodeDesc &ad, uint32_t cus, FusedLaunch &L, AttnArgs &a, QkvAttnFusedPlan &p) {
    if (fused_desc_shape_error(g) || g.kind != 0 || g.nb != 1 || ad.nb != 1 || ad.chunk || ad.want_frag) return false;
    if (!ad.n_head || !ad.n_kv_head || ad.n_head % ad.n_kv_head || !ad.hd || !ad.range_hint) return false;
    L = fused_launch(g, cus, F32X_MODEL);
    flag_scratch(L);
    route_fill(L.r, L.a);
    a = attn_launch(ad, attn_desc_nsplit(ad));
    const float *flag = reinterpret_cast<const float *>(g_flag);
    a.kraw = flag; a.rope_cos = flag; a.rope_sin = flag; a.rope_cur = flag;      // (the step always has them)
    if (ad.pool_rows) a.pt_rows = reinterpret_cast<const uint32_t *>(g_flag);
    if (route_kind(L.r, L.a) != (g.quant == NANO_QUANT_Q4K ? ROUTE_Q4K : ROUTE_GEMV)) return false;
    return qkv_attn_fused_plan(g.quant, L.a, a, &p);
}
static bool wo_w13_fused_resolve(const NanoFusedGemvDesc &wo, const NanoFusedGemvDesc &w13, uint32_t cus, FusedLaunch &La, FusedLaunch &Lb, WoW13FusedPlan &p) {
    if (fused_desc_shape_error(wo) || fused_desc_shape_error(w13) || wo.quant != NANO_QUANT_Q80 || w13.quant != NANO_QUANT_Q80) return false;
    if (wo.kind != 1 || w13.kind != 2 || wo.nb != 1 || w13.nb != 1 || wo.nseg != 1) return false;
    La = fused_launch(wo, cus, F32X_NONE); Lb = fused_launch(w13, cus, F32X_NONE);
    flag_scratch(La); flag_scratch(Lb);
    route_fill(La.r, La.a); route_fill(Lb.r, Lb.a);
    La.a.seg[0].out = reinterpret_cast<float *>(g_flag); Lb.a.xin = La.a.seg[0].out;       // (W1|W3 reads the stream Wo writes)
    if (route_kind(La.r, La.a) != ROUTE_GEMV || route_kind(Lb.r, Lb.a) != ROUTE_GEMV) return false;
    return wo_w13_fused_plan(La.a, Lb.a, &p);
}
static void plan_words(const QkvAttnFusedPlan &p, uint32_t *out) {
    const uint32_t v[NANO_QKV_ATTN_FUSED_PLAN_WORDS] = { p.kernel, p.nv, p.upw, p.d, p.qv, p.threads, p.n_attn, p.ngemv, p.lds_bytes, p.rw, p.wg[0], p.wg[1], p.wg[2], p.rounds, 0u, 1u };
    memcpy(out, v, sizeof(v));
}
static void plan_words(const WoW13FusedPlan &p, uint32_t *out) {
    const uint32_t v[NANO_WO_W13_FUSED_PLAN_WORDS] = { p.sig, p.threads, p.role, p.wf, p.wfc, p.nv_a, p.upw_a, p.nv_b, p.upw_b, p.wa, p.wb, p.lds_bytes, p.rw_a, p.rw_b, 0u, 1u, p.cw };
    memcpy(out, v, sizeof(v));
}

extern "C" int nano_hip_qkv_attn_fused_plan(const NanoFusedGemvDesc *qkv, const NanoAttnDecodeDesc *attn, uint32_t cus, uint32_t out[NANO_QKV_ATTN_FUSED_PLAN_WORDS]) {
    if (!qkv || !attn || !out) { nano_hip_set_error_("null argument"); return NANO_HIP_EINVAL; }
    memset(out, 0, NANO_QKV_ATTN_FUSED_PLAN_WORDS * sizeof(uint32_t));
    FusedLaunch L; AttnArgs a; QkvAttnFusedPlan p;
    if (qkv_attn_fused_resolve(*qkv, *attn, cus, L, a, p)) plan_words(p, out);
    return 0;
}
extern "C" int nano_hip_wo_w13_fused_plan(const NanoFusedGemvDesc *wo, const NanoFusedGemvDesc *w13, uint32_t cus, uint32_t out[NANO_WO_W13_FUSED_PLAN_WORDS]) {
    if (!wo || !w13 || !out) { nano_hip_set_error_("null argument"); return NANO_HIP_EINVAL; }
    memset(out, 0, NANO_WO_W13_FUSED_PLAN_WORDS * sizeof(uint32_t));
    FusedLaunch La, Lb; WoW13FusedPlan p;
    if (wo_w13_fused_resolve(*wo, *w13, cus, La, Lb, p)) plan_words(p, out);
    return 0;
}

// what a fused-launch operator borrows from a model: the hand-off words and granules (backend.hip handoff_alloc) and the sticky error word
struct HandoffState {
    uint32_t *tick = nullptr; unsigned long long *hand = nullptr;
    uint32_t *h_err = nullptr, *dev_err = nullptr;
    ~HandoffState() { (void)hipFree(tick); (void)hipFree(hand); if (h_err) (void)hipHostFree(h_err); }
    // granules zeroed or the caller's, tick[0] = tick0 + 1 (the embed kernel opens a new epoch), the error word 0
    int init(size_t granules, const unsigned long long *hand_init, uint32_t tick0) {
        OP_HIP(handoff_alloc(&tick, &hand, granules, nullptr, 0));
        if (hand_init) OP_HIP(hipMemcpy(hand, hand_init, granules * 8, hipMemcpyHostToDevice));
        const uint32_t t = tick0 + 1u;
        OP_HIP(hipMemcpy(tick, &t, 4, hipMemcpyHostToDevice));
        OP_HIP(hipHostMalloc(reinterpret_cast<void **>(&h_err), 64, hipHostMallocMapped));
        *h_err = 0;
        OP_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&dev_err), h_err, 0));
        return 0;
    }
    // behind the synchronisation: the error word; a give-up is the call's failure
    int finish(uint32_t *err_out) {
        const uint32_t c = *reinterpret_cast<volatile uint32_t *>(h_err);
        if (err_out) *err_out = c;
        if (c & NANO_DEVERR_HANDOFF) { nano_hip_set_error_("a consumer of the fused launch gave up waiting for its producers: no result is valid"); return NANO_HIP_ERUNTIME; }
        return 0;
    }
};
#define OP_ARG(cond, msg) do { if (!(cond)) { nano_hip_set_error_(msg); return NANO_HIP_EINVAL; } } while (0)

extern "C" int nano_hip_op_qkv_attn_fused(int device, const NanoQkvAttnFusedDesc *dp) {
    int rc; if ((rc = begin(device))) return rc;
    OP_ARG(dp && dp->qkv && dp->attn, "null descriptor");
    const NanoFusedGemvDesc &g = *dp->qkv;
    const NanoAttnDecodeDesc &d = *dp->attn;
    OP_ARG(dp->layer1 >= 1 && dp->layer1 <= 127, "layer1 outside 1 .. 127");
    if (const char *msg = fused_desc_shape_error(g)) { nano_hip_set_error_(msg); return NANO_HIP_EINVAL; }
    OP_ARG(g.x && g.norm_w, "the projection needs x and norm_w");
    OP_ARG(d.nb == 1 && d.n_layer && d.layer < d.n_layer && d.S, "bad nb / layer / S");
    OP_ARG(d.pos && d.rope_cos && d.rope_sin && d.k_cache && d.v_cache && d.out, "missing tensor");
    OP_ARG(!d.q_norm == !d.k_norm, "q_norm and k_norm go together");
    OP_ARG(d.range_hint >= d.pos[0] + 1 && d.range_hint <= d.S, "range_hint must cover pos + 1 and stay <= S");
    hipDeviceProp_t prop; OP_HIP(hipGetDeviceProperties(&prop, device));
    FusedLaunch L; AttnArgs a; QkvAttnFusedPlan p;
    OP_ARG(qkv_attn_fused_resolve(g, d, (uint32_t)prop.multiProcessorCount, L, a, p), "the fused q|k|v + attention launch does not take this shape");
    GemvArgs &ga = L.a;
    const uint32_t QD = a.q_dim, KD = a.kv_dim, half = d.hd / 2, nsplit = a.nsplit;
    const size_t cache_elems = (size_t)d.n_layer * d.S * KD;
    std::vector<float> rope_cur((size_t)2 * half);                  // { cos[pos], sin[pos] } (launch_embed)
    for (uint32_t i = 0; i < half; i++) {
        rope_cur[i] = d.rope_cos[(size_t)d.pos[0] * half + i];
        rope_cur[half + i] = d.rope_sin[(size_t)d.pos[0] * half + i];
    }
    DevBufs B;
    if ((rc = upload_weights(B, g, ga))) return rc;
    float *dq = B.alloc<float>(QD), *dk = B.alloc<float>(KD);
    uint32_t *dpos = B.upload(d.pos, 1);
    float *dcos = B.upload(d.rope_cos, (size_t)d.S * half), *dsin = B.upload(d.rope_sin, (size_t)d.S * half), *dcur = B.upload(rope_cur.data(), rope_cur.size());
    float *dkc = B.upload(reinterpret_cast<const float *>(d.k_cache), cache_elems), *dvc = B.upload(reinterpret_cast<const float *>(d.v_cache), cache_elems);
    float *dout = B.alloc<float>(QD), *dpart = B.alloc<float>((size_t)nsplit * QD), *dml = B.alloc<float>((size_t)d.n_head * nsplit * 2);
    OP_CHECK(dq && dk && dpos && dcos && dsin && dcur && dkc && dvc && dout && dpart && dml, "device alloc failed");
    OP_HIP(hipMemset(dq, 0, QD * 4)); OP_HIP(hipMemset(dk, 0, KD * 4)); OP_HIP(hipMemset(dout, 0, QD * 4));
    OP_HIP(hipMemset(dpart, 0, (size_t)nsplit * QD * 4)); OP_HIP(hipMemset(dml, 0, (size_t)d.n_head * nsplit * 8));
    // the projection as qkv_args() builds it: q and the raw k row to scratch, v straight to its cache row
    ga.xin = B.upload(g.x, g.n); ga.xin_bstride = g.n;
    ga.norm_w = B.upload(g.norm_w, g.n);
    OP_CHECK(ga.xin && ga.norm_w, "device alloc failed");
    ga.seg[0].out = dq; ga.seg[0].out_bstride = QD;
    ga.seg[1].out = dk; ga.seg[1].out_bstride = KD;
    ga.seg[2].out = dvc + (size_t)d.layer * d.S * KD; ga.seg[2].out_bstride = d.n_layer * d.S * KD; ga.seg[2].out_pstride = KD;
    ga.pos = dpos; ga.ordered = 0;
    if (d.q_norm) { a.q_norm = B.upload(d.q_norm, d.hd); a.k_norm = B.upload(d.k_norm, d.hd); OP_CHECK(a.q_norm && a.k_norm, "device alloc failed"); }
    a.q = dq; a.kraw = dk; a.kcache = dkc; a.vcache = dvc; a.pos = dpos;
    a.rope_cos = dcos; a.rope_sin = dsin; a.rope_cur = dcur; a.out = dpart; a.ml = dml; a.xba_out = dout;
    HandoffState H;
    if ((rc = H.init((size_t)QD + 2 * (size_t)KD, dp->hand_init, dp->tick0))) return rc;
    ga.err = H.dev_err; a.err = H.dev_err;
    QkvAttnFusedPlan ran;
    OP_ARG(qkv_attn_fused_plan(g.quant, ga, a, &ran) && !memcmp(&ran, &p, sizeof(p)), "the plan moved between the query's arguments and the launch's");
    OP_HIP(launch_qkv_attn_fused(g.quant, ga, a, H.hand, H.tick, dp->layer1, 0));
    OP_HIP(hipDeviceSynchronize());
    if ((rc = H.finish(dp->err_out))) return rc;
    if (nsplit > 1) {
        if (dp->part_out) OP_HIP(hipMemcpy(dp->part_out, dpart, (size_t)nsplit * QD * 4, hipMemcpyDeviceToHost));
        if (dp->ml_out) OP_HIP(hipMemcpy(dp->ml_out, dml, (size_t)d.n_head * nsplit * 8, hipMemcpyDeviceToHost));
        OP_HIP(launch_attn_combine_tokens(dpart, dml, dout, d.n_head, d.hd, nsplit, 1, nullptr, nullptr, 0));
        OP_HIP(hipDeviceSynchronize());
    }
    OP_HIP(hipMemcpy(d.out, dout, (size_t)QD * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(d.k_cache, dkc, cache_elems * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(d.v_cache, dvc, cache_elems * 4, hipMemcpyDeviceToHost));
    if (g.out) {
        OP_HIP(hipMemcpy(g.out, dq, (size_t)QD * 4, hipMemcpyDeviceToHost));
        OP_HIP(hipMemcpy(g.out + QD, dk, (size_t)KD * 4, hipMemcpyDeviceToHost));
    }
    if (dp->plan_out) plan_words(ran, dp->plan_out);
    return 0;
}

extern "C" int nano_hip_op_wo_w13_fused(int device, const NanoWoW13FusedDesc *dp) {
    int rc; if ((rc = begin(device))) return rc;
    OP_ARG(dp && dp->wo && dp->w13, "null descriptor");
    const NanoFusedGemvDesc &wo = *dp->wo, &w13 = *dp->w13;
    OP_ARG(dp->layer1 >= 1 && dp->layer1 <= 127, "layer1 outside 1 .. 127");
    if (const char *msg = fused_desc_shape_error(wo)) { nano_hip_set_error_(msg); return NANO_HIP_EINVAL; }
    if (const char *msg = fused_desc_shape_error(w13)) { nano_hip_set_error_(msg); return NANO_HIP_EINVAL; }
    OP_ARG(wo.out && w13.out && w13.norm_w && (wo.x || wo.attn_part) && (!wo.attn_part || wo.attn_ml), "missing tensor");
    hipDeviceProp_t prop; OP_HIP(hipGetDeviceProperties(&prop, device));
    FusedLaunch La, Lb; WoW13FusedPlan p;
    OP_ARG(wo_w13_fused_resolve(wo, w13, (uint32_t)prop.multiProcessorCount, La, Lb, p), "the fused Wo + W1|W3 launch does not take this shape");
    GemvArgs &a = La.a, &b = Lb.a;
    const uint32_t E = wo.rows[0], H13 = w13.rows[0];
    DevBufs B;
    if ((rc = upload_weights(B, wo, a))) return rc;
    if ((rc = upload_weights(B, w13, b))) return rc;
    float *dx = B.upload(wo.out, E), *dhb = B.alloc<float>(H13);      // the residual stream; hb
    OP_CHECK(dx && dhb, "device alloc failed");
    OP_HIP(hipMemset(dhb, 0, (size_t)H13 * 4));
    a.seg[0].out = dx; a.seg[0].out_bstride = E;
    if (wo.x) { a.xin = B.upload(wo.x, wo.n); OP_CHECK(a.xin, "device alloc failed"); a.xin_bstride = wo.n; }
    if (wo.attn_part) {
        a.attn_part = B.upload(wo.attn_part, (size_t)wo.attn_nsplit * wo.n);
        a.attn_ml = B.upload(wo.attn_ml, (size_t)wo.attn_n_head * wo.attn_nsplit * 2);
        OP_CHECK(a.attn_part && a.attn_ml, "device alloc failed");
        if (!a.xin) { a.xin = a.attn_part; a.xin_bstride = wo.n; }   // never read: the prologue combines the partials
    }
    b.xin = dx; b.xin_bstride = E;                                   // as the step wires it: W1|W3 reads what Wo leaves
    b.norm_w = B.upload(w13.norm_w, w13.n); OP_CHECK(b.norm_w, "device alloc failed");
    b.seg[0].out = dhb; b.seg[0].out_bstride = H13; b.seg[1].out = dhb; b.seg[1].out_bstride = H13;
    a.ordered = 0; b.ordered = 0;
    HandoffState H;
    if ((rc = H.init(E, dp->hand_init, dp->tick0))) return rc;
    a.err = H.dev_err; b.err = H.dev_err;
    WoW13FusedPlan ran;
    OP_ARG(wo_w13_fused_plan(a, b, &ran) && !memcmp(&ran, &p, sizeof(p)), "the plan moved between the query's arguments and the launch's");
    OP_HIP(launch_wo_w13_fused(a, b, H.hand, H.tick, dp->layer1, 0));
    OP_HIP(hipDeviceSynchronize());
    if ((rc = H.finish(dp->err_out))) return rc;
    OP_HIP(hipMemcpy(wo.out, dx, (size_t)E * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(w13.out, dhb, (size_t)H13 * 4, hipMemcpyDeviceToHost));
    if (dp->plan_out) plan_words(ran, dp->plan_out);
    return 0;
}
#undef OP_ARG
