// backend_step.hip -- one step, enqueued on m->st: the argument builders, the fast step, the reference-order step of strict and
// exact mode, the graphs of a step, run_step, and which step serves the model's switches.  Both steps take a StepSpec (step_spec.h) and
// read nothing about the step from the model: the same spec queues the same launches, eagerly or under capture, and step_key() of it is
// the graph's key.  The runners (run_step, run_step_ordered; enqueue_chunk in backend.hip, the ragged pass in backend_rows.hip) record
// m->nsplit = xba_nsplit(m, spec) themselves: a replay never runs the enqueue.
#include "backend_model.h"

namespace nano { extern hipEvent_t g_q80_probe_start, g_q80_probe_stop; }     // gemv_q80.hip: exact start / stop of the next STREAM launch

// the stamp slab of the next launch of kind k (1 QKV, 2 attention, 3 Wo, 4 W1|W3, 5 W2, 6 classifier), or nullptr
static unsigned long long *next_stamps(NanoHipModel *m, uint32_t kind) {
    if (!m->stamp.on || m->stamp.launches >= STAMP_MAX_LAUNCHES) return nullptr;
    m->stamp.kinds.push_back(kind);
    return m->stamp.buf + (size_t)(m->stamp.launches++) * STAMP_WGS * 8;
}

static GemvSeg mkseg(const TensorRef &t, float *out, uint32_t rows, uint32_t bstride, uint32_t pstride = 0) {
    GemvSeg s{}; s.w = t.w; s.ws = t.s; s.out = out; s.rows = rows; s.out_bstride = bstride; s.out_pstride = pstride;
    return s;
}
// the router's view of the model (route.hip): which kernel a projection launch goes to
static Q80Route route_of(const NanoHipModel *m) {
    Q80Route r{};
    r.quant = m->d.quant_type; r.cus = m->cus; r.mfma_min_nb = m->mfma_min_nb;
    r.gq = m->gq; r.gxs = m->gxs; r.q4x = m->q4x; r.q4x_bytes = m->q4x_bytes;
    r.f32_min_nb = m->f32_min_nb; r.f32x = m->f32x; r.f32x_floats = m->f32x_floats;
    return r;
}
static RouteKind kind_of(const NanoHipModel *m, GemvArgs a) { a.ordered = (m->strict || m->exact) ? 1u : 0u; a.cus = (uint32_t)m->cus; return route_kind(route_of(m), a); }

static hipError_t gemv(NanoHipModel *m, GemvArgs &a) {
    a.ordered = (m->strict || m->exact) ? 1u : 0u;                     // strict / exact mode: the reference's group order in every kernel
    a.err = m->dev_err;
    return route_projection(route_of(m), a, m->st);
}

static GemvArgs classifier_args(const NanoHipModel *m, uint32_t nb, float *dst) {
    GemvArgs a{};
    a.nseg = 1; a.seg[0] = mkseg(m->cls, dst, m->d.vocab_size, m->d.vocab_size);
    a.n = m->d.n_embd; a.gs = m->d.group_size; a.nb = nb; a.xin = m->x; a.xin_bstride = m->d.n_embd;
    a.epi = GEMV_EPI_STORE; a.norm_w = m->rms_final; a.pos = m->pos;
    return a;
}

hipError_t enqueue_classifier(NanoHipModel *m, uint32_t nb, uint32_t *ntiles_out, float *dst) {
    GemvArgs a = classifier_args(m, nb, dst ? dst : m->logits);
    a.ordered = (m->strict || m->exact) ? 1u : 0u;                     // (as gemv() sends it)
    if (ntiles_out)                                                    // per-tile arg-max partials for the sampler (route.hip: the operator's condition and count too)
        if (const uint32_t n = route_partials(route_of(m), a)) { a.tile_max = m->tile_max; *ntiles_out = n; }
    return gemv(m, a);
}
// the row statistics of `rows` rows of logits (row stride V) for targets[rows] (nullptr: each row's own arg-max) -> out[rows]  (score.hip)
hipError_t enqueue_score_rows(NanoHipModel *m, const float *logits, uint32_t rows, const uint32_t *targets, NanoHipTokenScore *out) {
    ScoreArgs a{};
    a.logits = logits; a.V = m->d.vocab_size; a.ntiles = score_tiles(a.V); a.targets = targets; a.part = m->rb.part; a.out = out;
    return launch_score_rows(a, rows, m->st);
}
// attention splits of a step: batches bring their own parallelism (nb x KV groups workgroups per split) and every
// split costs the Wo prologue nb x nsplit partial reads, so larger batches split less
static uint32_t step_nsplit(const NanoHipModel *m, uint32_t nb, uint32_t range_hint) {
    uint32_t ns = attention_nsplit(range_hint, m->hd);
    if (nb >= 4) { const uint32_t div = nb / 2; ns = (ns + div - 1) / div; }
    if (nb >= m->mfma_min_nb) ns = 1;   // the MFMA GEMM path takes plain activations only
    if (m->lora_on) ns = 1;             // the LoRA o-branch reads the combined attention output
    if (nb > 1 && (uint64_t)(m->d.n_embd / 16) * nb * m->QD > (4u << 20)) ns = 1;   // ditto the quantize-once GEMV path (route.hip ROUTE_GEMV_PREQ)
    return ns ? ns : 1;
}

// ---- the four projection launches of layer l: ONE builder each, for the fast step, the reference-order step and the routing
// questions alike.  The arguments are what differs between the callers; what a caller adds afterwards (stamps, frag_ready, the
// fused launches' ordered / cus / err) stays with that caller.  route_kind() reads only shapes, nb, epi, attn_part, resid_add and
// xq_in (route.hip), none of which depends on the layer: a question asked with layer 0's tensor is answered as for layer l's launch.
static GemvArgs proj_args(const NanoHipModel *m, uint32_t nb, uint32_t n, const float *xin, uint32_t epi) {
    GemvArgs a{};
    a.n = n; a.gs = m->d.group_size; a.nb = nb; a.xin = xin; a.xin_bstride = n; a.epi = epi; a.pos = m->pos;
    return a;
}
// q | raw k | v from xin (norm_w: the rmsnorm its prologue applies, or nullptr for an input that is normalised already); v goes where
// the cache's row description says (v's is the only position-indexed output)   reference infer.c:758-786
static GemvArgs qkv_args(const NanoHipModel *m, uint32_t l, uint32_t nb, const float *xin, const float *norm_w, const KvRows::VTarget &v) {
    GemvArgs a = proj_args(m, nb, m->d.n_embd, xin, GEMV_EPI_STORE);
    a.nseg = 3;
    a.seg[0] = mkseg(m->W[WQ][l], m->q, m->QD, m->QD);
    a.seg[1] = mkseg(m->W[WK][l], m->kraw, m->KD, m->KD);
    a.seg[2] = mkseg(m->W[WV][l], v.out, m->KD, v.bstride, v.pstride);
    a.norm_w = norm_w; a.pos = v.pos;
    return a;
}
// x += Wo . xba (+ the LoRA o-branch's o1): with the plain (combined, normalised) attention output as its input, and -- nsplit > 1 --
// with the splits' partials as its input (combined in its prologue: SLAB GEMV)   reference infer.c:885-908
static GemvArgs wo_args(const NanoHipModel *m, uint32_t l, uint32_t nb, uint32_t nsplit) {
    GemvArgs a = proj_args(m, nb, m->QD, m->xba, GEMV_EPI_RESID);
    a.nseg = 1; a.seg[0] = mkseg(m->W[WO][l], m->x, m->d.n_embd, m->d.n_embd);
    if (m->lora_on) { a.resid_add = m->lora_o1; a.resid_add_bstride = m->d.n_embd; }
    if (nsplit > 1) { a.attn_part = m->attn_part; a.attn_ml = m->attn_ml; a.attn_nsplit = nsplit; a.attn_n_head = m->d.n_head; a.attn_hd = m->hd; a.attn_table = m->ho.combine_wave ? 0u : 1u; }
    return a;
}
// W1 | W3 from xin: epi SWIGLU leaves hb = silu(W1 . xn) * (W3 . xn) (w3_out = hb), epi STORE the two products (w3_out = hb2)   infer.c:914-944
static GemvArgs w13_args(const NanoHipModel *m, uint32_t l, uint32_t nb, const float *xin, const float *norm_w, float *w3_out, uint32_t epi) {
    GemvArgs a = proj_args(m, nb, m->d.n_embd, xin, epi);
    a.nseg = 2; a.seg[0] = mkseg(m->W[W1][l], m->hb, m->d.n_hidden, m->d.n_hidden); a.seg[1] = mkseg(m->W[W3][l], w3_out, m->d.n_hidden, m->d.n_hidden);
    a.norm_w = norm_w;
    return a;
}
// what the two LoRA launches of layer l share: row b belongs to KV slot s.slot + b (a decode step) or s.slot (a chunk)
static LoraRowsArgs lora_rows_args(const NanoHipModel *m, const StepSpec &s, uint32_t l) {
    LoraRowsArgs a{};
    a.desc = m->lt.desc; a.E = m->d.n_embd; a.KD = m->KD; a.layer = l; a.slot0 = s.slot; a.slot_stride = s.one_slot() ? 0u : 1u; a.max_rank = m->lt.max_rank;
    return a;
}
// x += W2 . hb   reference infer.c:950-965
static GemvArgs w2_args(const NanoHipModel *m, uint32_t l, uint32_t nb) {
    GemvArgs a = proj_args(m, nb, m->d.n_hidden, m->hb, GEMV_EPI_RESID);
    a.nseg = 1; a.seg[0] = mkseg(m->W[W2][l], m->x, m->d.n_embd, m->d.n_embd);
    return a;
}
// does the Wo launch combine the `nsplit` partials itself?  (else: a combine kernel of its own in front of it)
static bool wo_takes_parts(const NanoHipModel *m, const StepSpec &s, uint32_t nsplit) {
    const uint32_t nb = s.nb;
    if (nsplit <= 1 || nsplit > 8 || s.rows_split_alone()) return false;
    // the plain-activation route first: a Wo launch the batched GEMM would take (Qwen3-4B at 2..8 sequences) keeps it -- the splits are
    // then combined by a kernel of its own.  (Asking only about the launch WITH the partials attached always answered "GEMV": the
    // batched routes refuse partials, and 4 sequences beyond 64 positions ran the 8-sequence SLAB GEMV: 2.6 ms against 2.0.)
    if (route_takes_fragments(kind_of(m, wo_args(m, 0, nb, 1)))) return false;
    return route_takes_attn_parts(kind_of(m, wo_args(m, 0, nb, nsplit)));
}
// the attention splits of step s: a chunk's or ragged pass's rows split as the one-sequence decode step of the step's range hint does
static uint32_t spec_nsplit(const NanoHipModel *m, const StepSpec &s) { return step_nsplit(m, s.rows_split_alone() ? 1u : s.nb, s.range_hint); }
uint32_t xba_nsplit(const NanoHipModel *m, const StepSpec &s, bool ordered) {
    if (s.rows != StepSpec::SEQS || ordered) return 1u;
    const uint32_t ns = spec_nsplit(m, s);
    return (ns > 1 && !wo_takes_parts(m, s, ns)) ? 1u : ns;
}
// paged KV cache: the table rows of the step's rows and the entries between them.  SEQS rows are slots 0 .. nb - 1 of the table, a chunk's
// rows positions of its slot's table row, a ragged pass's rows index the whole table by row_slot.  The embed kernel stages each row's pool
// row next to its RoPE row; the q | k | v launch and the attention kernel write there.
static const uint32_t *paged_rows(const NanoHipModel *m, const StepSpec &s) { return m->kv.pt + (s.one_slot() ? (size_t)s.slot * m->kv.pt_stride : 0); }
static uint32_t paged_bstride(const NanoHipModel *m, const StepSpec &s) { return s.rows_split_alone() ? 0u : m->kv.pt_stride; }
// the step's first kernel: tokens -> x, and each row's RoPE row and -- paged cache -- pool row staged at fixed addresses
static EmbedArgs embed_args(const NanoHipModel *m, const StepSpec &s) {
    EmbedArgs ea{};
    ea.tok = m->tok.w; ea.tok_s = m->tok.s; ea.tokens = m->tokens; ea.x = m->x;
    ea.E = m->d.n_embd; ea.gs = m->d.group_size; ea.quant = m->d.quant_type; ea.x_bstride = m->d.n_embd;
    ea.rope_cos = m->rope_cos; ea.rope_sin = m->rope_sin; ea.pos = m->pos; ea.rope_cur = m->rope_cos ? m->rope_cur : nullptr; ea.half = m->hd / 2;
    if (m->kv.paged) { ea.pt_rows = paged_rows(m, s); ea.kvrow = m->kv.kvrow; ea.pt_bstride = paged_bstride(m, s); ea.pt_entries = m->kv.pt_stride; }
    ea.row_slot = s.row_slot;
    return ea;
}
// every row's arg-max of logits[nb][V] -> amax (the caller adds the classifier's partials and the loop's feedback)
static ArgmaxArgs argmax_args(const NanoHipModel *m, uint32_t nb, const float *logits, uint32_t *amax) {
    ArgmaxArgs aa{};
    aa.logits = logits; aa.V = m->d.vocab_size; aa.bstride = m->d.vocab_size; aa.out = amax; aa.pos = m->pos; aa.pos0 = m->pos0; aa.nb = nb;
    return aa;
}
// layer l's attention launch over all the step's rows: qk-norm, rope, k-cache write, attention   reference infer.c:810-879
static AttnArgs attn_args(const NanoHipModel *m, const StepSpec &s, const KvRows &kv, uint32_t l, uint32_t nsplit) {
    const NanoModelDesc &d = m->d;
    AttnArgs a{};
    a.err = m->dev_err;
    a.q = m->q; a.kraw = m->kraw; kv.attention(a); a.pos = m->pos;
    a.q_norm = m->q_norm ? m->q_norm + (size_t)l * m->hd : nullptr;
    a.k_norm = m->k_norm ? m->k_norm + (size_t)l * m->hd : nullptr;
    a.rope_cos = m->rope_cos; a.rope_sin = m->rope_sin; a.rope_cur = m->rope_cos ? m->rope_cur : nullptr;
    a.out = m->attn_part; a.ml = m->attn_ml; a.xba_out = m->xba; a.nsplit = nsplit; a.range_hint = s.range_hint;
    a.layer = l; a.n_layer = d.n_layer; a.S = m->S; a.hd = m->hd; a.n_head = d.n_head; a.n_kv_head = d.n_kv_head;
    a.q_dim = m->QD; a.kv_dim = m->KD; a.rope_qwen3 = (d.arch == NANO_ARCH_QWEN3); a.is_causal = s.is_causal;
    a.kv_half = m->kv_half; a.vraw = m->kv_half ? m->vraw : nullptr;
    if (m->kv.paged) { a.pt_rows = paged_rows(m, s); a.kvrow = m->kv.kvrow; a.pt_stride = m->kv.pt_stride; a.pt_bstride = paged_bstride(m, s); a.pool_rows = m->kv.pages * 64u; }
    return a;
}
// The attention launches of one layer of a ragged pass (s.groups; `a` = the layer's arguments as attn_args built them for all nb rows).
// Pass 1 over ALL rows finishes every k row -- and the v row, from scratch, on the FP16 and the contiguous FP32 cache -- so that every
// row of the pass finds the rows of the earlier positions of its slot in the cache, whichever group they belong to.  Then one launch per
// group of rows that share a range hint, with that bucket's split count and hint -- the launch a prefill chunk of the bucket gets -- on
// the group's rows of every row-indexed array, and the combine launch where the range is split.  The groups run one after the other on
// the stream, so their partials may lie anywhere in the partial buffers.
static hipError_t enqueue_rows_attention(NanoHipModel *m, const StepSpec &s, AttnArgs a, bool wo_frag) {
    const NanoModelDesc &d = m->d;
    const uint32_t QD = m->QD, KD = m->KD;
    hipError_t e;
    a.row_slot = s.row_slot;
    a.xf_out = nullptr; a.xsf_out = nullptr; a.stamps = nullptr;
    if (!m->kv_half && !m->kv.paged) a.vraw = m->rows.vraw;
    AttnArgs p = a;
    p.prep_only = 1; p.nsplit = 1; p.range_hint = s.groups[0].hint;               // (nothing attended: the fewest workgroups, the smallest range)
    if ((e = launch_attention(p, s.nb, m->st)) != hipSuccess) return e;
    for (uint32_t gi = 0; gi < s.n_groups; gi++) {
        const RowGroup &g = s.groups[gi];
        AttnArgs b = a;
        const uint32_t ns = step_nsplit(m, 1, g.hint);
        const size_t r0 = g.row0;
        b.nsplit = ns; b.range_hint = g.hint;
        b.q += r0 * QD; b.kraw += r0 * KD; b.pos += r0; b.row_slot += r0;
        if (b.rope_cur) b.rope_cur += r0 * 2 * (m->hd / 2);
        if (b.kvrow) b.kvrow += r0;
        b.vraw = m->kv_half ? m->vraw + r0 * KD : nullptr;                          // (FP32: pass 1 stored the row, the cache has it)
        b.out += r0 * ns * QD; b.ml += r0 * d.n_head * ns * 2; b.xba_out += r0 * QD;
        if (wo_frag && ns == 1) { b.xf_out = m->gq; b.xsf_out = m->gxs; }           // (one group: row0 = 0)
        if ((e = launch_attention(b, g.n, m->st)) != hipSuccess) return e;
        if (ns > 1 && (e = launch_attn_combine_tokens(b.out, b.ml, b.xba_out, d.n_head, m->hd, ns, g.n, wo_frag ? m->gq : nullptr, wo_frag ? m->gxs : nullptr, m->st)) != hipSuccess) return e;
    }
    return hipSuccess;
}
// s.range_hint: host-side upper bound of the attended range of every sequence (a multiple of 64, <= S)
hipError_t enqueue_step(NanoHipModel *m, const StepSpec &s) {
    const NanoModelDesc &d = m->d;
    const uint32_t E = d.n_embd, L = d.n_layer, nb = s.nb, mode = s.mode;
    hipError_t e;
    // Batched prefill (CHUNK) splits every token's attention exactly as that token's own decode step would (chunks start on
    // multiples of the 64-position bucket, so one range_hint covers them) and combines with a kernel of its own: the KV
    // rows and the following logits then carry the bits of token-by-token ingestion.
    // A ragged pass (RAGGED; backend_rows.hip): rows of several slots and range buckets.  Its rows come sorted into groups
    // that share a range hint; each group gets the attention launch (and combine launch) of a prefill chunk of that bucket, so every row
    // still splits as its own decode step.  range_hint is the last group's (the largest), nsplit below the largest split count.
    const bool ragged = s.ragged(), pf = s.rows_split_alone();
    const size_t ngroups = ragged ? s.n_groups : 1u;
    const uint32_t nsplit = spec_nsplit(m, s);
    // Does this step's Wo launch go to the batched GEMM (plain activations only), or is the range split wider than the Wo
    // GEMV's prologue combines?  Then a split attention is combined by a kernel of its own (as in batched prefill) -- for
    // <= 8 splits the same arithmetic, same bits.
    const bool pf_combine = nsplit > 1 && !wo_takes_parts(m, s, nsplit);
    const uint32_t wo_nsplit = pf_combine ? 1u : nsplit;                     // splits the Wo launch combines in its prologue (SEQS: xba_nsplit(m, s))
    const bool wo_gemm = route_takes_fragments(kind_of(m, wo_args(m, 0, nb, wo_nsplit)));
    // Single-split attention (or the combine kernel) of a step whose Wo launch goes to the batched GEMM: that kernel writes
    // Wo's quantized input itself (Q80 groups of 64 inside a head, fragment order) -- one quantizer launch less per layer.
    // (a ragged pass of several groups: fragment rows are 16-token tiles of the WHOLE pass, a group starts at any row -- its launches
    // write plain xba and the Wo launch runs its quantizer, which by definition makes the same fragments)
    const bool wo_frag = wo_gemm && d.group_size == 64 && m->hd % 64 == 0 && ngroups == 1;
    EmbedArgs ea = embed_args(m, s);
    const KvRows kv = KvRows::of(m, s);
    ea.tick = m->ho.tick;                                                       // the step's first kernel opens a new hand-off epoch
    if (s.embeds() && (e = launch_embed(ea, nb, m->st)) != hipSuccess) return e;

    for (uint32_t l = 0; l < L; l++) {
        // q | raw k | v; v goes straight to its cache row; a chunk: every token of the step is a position of KV slot s.slot
        GemvArgs qa = qkv_args(m, l, nb, m->x, m->rms_attn + (size_t)l * E, kv.v_target(l));
        AttnArgs a = attn_args(m, s, kv, l, nsplit);
        if (wo_frag && nsplit == 1) { a.xf_out = m->gq; a.xsf_out = m->gxs; }
        qa.ordered = 0; qa.cus = (uint32_t)m->cus; qa.err = m->dev_err;
        // ONE launch for both (one sequence, Q80 group size 64, Qwen3 attention at head_dim 128: gemv_q80_impl.h qkv_attn_fused_kernel): the
        // attention workgroups start with the projection's, ask for their K / V rows and take q / k / v from it as write-through granules
        // tagged with the epoch of this step and layer (tick * 128 + l + 1: at most 126 layers).
        const bool fused = m->ho.fuse_qkv_attn && m->ho.hand && nb == 1 && !pf && !m->lora_on && !m->stamp.on && L <= 126u &&
                           kind_of(m, qa) == (d.quant_type == NANO_QUANT_Q4K ? ROUTE_Q4K : ROUTE_GEMV) && qkv_attn_fused_supports(d.quant_type, qa, a);
        if (fused) {
            if ((e = launch_qkv_attn_fused(d.quant_type, qa, a, m->ho.hand, m->ho.tick, l + 1u, m->st)) != hipSuccess) return e;
        } else {
            qa.stamps = next_stamps(m, 1);
            if ((e = gemv(m, qa)) != hipSuccess) return e;
            if (m->lora_on) {       // q / k / v += (alpha/rank) B (A xb), each row with the module of its slot or none   reference infer.c:792-808
                LoraRowsArgs lr = lora_rows_args(m, s, l);
                lr.x = m->x; lr.norm_w = m->rms_attn + (size_t)l * E;
                lr.q = m->q; lr.kraw = m->kraw; lr.v = kv.v_flat(l); lr.v_bstride = kv.v_flat_bstride(); lr.pos = m->pos;
                if ((e = launch_lora_qkv_rows(lr, nb, m->st)) != hipSuccess) return e;
            }
            if (ragged) {           // pass 1 over all rows, then a launch (and a combine launch) per range bucket
                if ((e = enqueue_rows_attention(m, s, a, wo_frag)) != hipSuccess) return e;
            } else {
                if (pf) {
                    // batched prefill: the nb tokens are consecutive positions of ONE sequence.  Pass 1 finishes every k row
                    // (norm + RoPE + cache write -- paged: into its page -- nothing else) so that pass 2 finds the rows of the earlier
                    // tokens of the chunk in the cache; pass 2 is the ordinary decode attention per token (it recomputes its own k row).
                    a.prep_only = 1;
                    if ((e = launch_attention(a, nb, m->st)) != hipSuccess) return e;
                    a.prep_only = 0;
                }
                a.stamps = next_stamps(m, 2);
                if ((e = launch_attention(a, nb, m->st)) != hipSuccess) return e;
            }
        }
        if (pf_combine && !ragged && (e = launch_attn_combine_tokens(m->attn_part, m->attn_ml, m->xba, d.n_head, m->hd, nsplit, nb, wo_frag ? m->gq : nullptr, wo_frag ? m->gxs : nullptr, m->st)) != hipSuccess) return e;
        {   // x += Wo . xba   reference infer.c:885-908
            if (m->lora_on) {       // o1 = (alpha/rank) B_o (A_o xba), added by the Wo epilogue: x += (Wo xba + o1); a row without a module gets -0.0f   infer.c:898-908
                LoraRowsArgs lr = lora_rows_args(m, s, l);
                lr.x = m->xba; lr.q = m->lora_o1;
                if ((e = launch_lora_o_rows(lr, nb, m->st)) != hipSuccess) return e;
            }
            GemvArgs a = wo_args(m, l, nb, wo_nsplit);
            a.frag_ready = wo_frag ? 1u : 0u;
            // hb = silu(W1 . xn) * (W3 . xn)   reference infer.c:914-944
            GemvArgs b = w13_args(m, l, nb, m->x, m->rms_ffn + (size_t)l * E, m->hb, GEMV_EPI_SWIGLU);
            // ONE launch for both (one sequence, Q80 group size 64; gemv_q80_impl.h wo_w13_fused_kernel): W1|W3's workgroups take x from Wo's as
            // granules of the same launch (epoch tags like the q | k | v + attention launch's).
            a.ordered = 0; a.cus = (uint32_t)m->cus; a.err = m->dev_err; b.ordered = 0; b.cus = (uint32_t)m->cus; b.err = m->dev_err;
            // Where it is used (round 5, same-box A/Bs, profiles/r05_wo_w13_fused.txt): with the polls backed off (workgroups that produce nothing
            // nap ~2 us before their first sweep) the fused launch wins on Qwen3-0.6B's matrices at every position (1882-1887 vs 1859-1871 tok/s at
            // positions 20..39, 1789-1795 vs 1750-1753 over 31..510).  The other forms were measured and removed: on Qwen3-4B's
            // wide matrices a 1024-thread form LOST (1.531 vs 1.473 ms per step: workgroups that spill, polls queued behind their own 207 KB of weight
            // loads) -- wo13_shape refuses those shapes; Q4K's lost 1 % over positions 31..510 (profiles/r06_q4k_fused.txt), FP32's 1.5 % at
            // positions 20..39 and 2.9 % over 31..510.
            const bool fuse13 = m->ho.fuse_wo_w13 && m->ho.hand2 && nb == 1 && !pf && !m->lora_on && !m->stamp.on && L <= 126u && d.quant_type == NANO_QUANT_Q80 &&
                                kind_of(m, a) == ROUTE_GEMV && kind_of(m, b) == ROUTE_GEMV && wo_w13_fused_supports(a, b);
            if (fuse13) {
                if ((e = launch_wo_w13_fused(a, b, m->ho.hand2, m->ho.tick, l + 1u, m->st)) != hipSuccess) return e;
            } else {
                a.stamps = next_stamps(m, 3);
                if ((e = gemv(m, a)) != hipSuccess) return e;
                b.stamps = next_stamps(m, 4);
                if ((e = gemv(m, b)) != hipSuccess) return e;
            }
        }
        {   // x += W2 . hb   reference infer.c:950-965
            GemvArgs a = w2_args(m, l, nb);
            a.stamps = next_stamps(m, 5);
            if ((e = gemv(m, a)) != hipSuccess) return e;
        }
    }
    if (mode == MODE_NOCLS) return hipSuccess;
    if (mode == MODE_SCORE) {       // a scoring prefill chunk: the classifier over all nb rows (final rmsnorm in its prologue), then their statistics
        if ((e = enqueue_classifier(m, nb, nullptr, m->rb.logits)) != hipSuccess) return e;
        return enqueue_score_rows(m, m->rb.logits, nb, s.use_targets ? m->rb.targets : nullptr, m->rb.rows);
    }
    if (mode == MODE_VERIFY) {      // a verify chunk: the classifier over all nb rows, then every row's arg-max (a scan of its logits: the partials buffer holds max_batch rows)
        if ((e = enqueue_classifier(m, nb, nullptr, m->rb.logits)) != hipSuccess) return e;
        return launch_argmax(argmax_args(m, nb, m->rb.logits, m->rb.amax), nb, m->st);
    }
    const bool sample = (mode == MODE_ARGMAX || mode == MODE_LOOP);
    uint32_t ntiles = 0;
    // probe: Q80 STREAM classifier (batch <= 8) -> the kernel's own start / stop timestamps (hipExtLaunchKernelGGL);
    // other classifiers -> events recorded around the launch (ev1..ev2 = an empty pair, the event overhead)
    bool probe_ext = s.probe_cls && d.quant_type == NANO_QUANT_Q80 && nb <= 8 && d.vocab_size >= 16384 && !route_takes_fragments(kind_of(m, classifier_args(m, nb, m->logits)));
    if (s.probe_cls && d.quant_type == NANO_QUANT_Q4K && nb == 1 && d.vocab_size >= 65536) {      // gemv_q4k_chunk.hip's looping launch
        GemvArgs ca = classifier_args(m, nb, m->logits);
        Q4kGemvPlan cp;
        probe_ext = gemv_q4k_plan(ca, &cp) && cp.kernel == Q4K_KERNEL_CHUNK && cp.loop;
    }
    if (probe_ext) { g_q80_probe_start = m->ev0; g_q80_probe_stop = m->ev1; }
    else if (s.probe_cls && (e = hipEventRecord(m->ev0, m->st)) != hipSuccess) return e;
    if ((e = enqueue_classifier(m, nb, sample ? &ntiles : nullptr)) != hipSuccess) return e;
    g_q80_probe_start = g_q80_probe_stop = nullptr;
    if (s.probe_cls) {
        if (!probe_ext && (e = hipEventRecord(m->ev1, m->st)) != hipSuccess) return e;
        if ((e = hipEventRecord(m->ev2, m->st)) != hipSuccess) return e;
    }
    m->probe_ext = probe_ext;   // final rmsnorm fused in the prologue (infer.c:999-1015)
    if (sample) {
        ArgmaxArgs aa = argmax_args(m, nb, m->logits, m->amax);
        if (ntiles) { aa.tile_max = m->tile_max; aa.ntiles = ntiles; }
        if (mode == MODE_LOOP) {
            aa.tokens = m->tokens; aa.trace = m->trace;
            if (!pf) { aa.emb = ea; aa.rope_rows = m->rope_rows; }      // ... and embeds the token it picked for the next step
        }
        if ((e = launch_argmax(aa, nb, m->st)) != hipSuccess) return e;
    }
    return hipSuccess;
}
// the reference-order step of strict mode (strict.hip) and exact mode (exact.hip): one kernel per reference operator, every float
// chain in the reference's order.  Quantizers, quantized GEMVs, embedding, RoPE, residual adds and arg-max are the fast path's own
// (bit-exact) kernels, fed with un-normalised launches (norm_w = nullptr); rmsnorm / attention / SwiGLU / the FP32 matmul are
// strict.hip's or exact.hip's.  Sequence b of the step lives in KV slot slot0 + b.
//   strict mode (exact_kernels = false): eager.  The optional phase hook fires where the reference fires its observation callback
//     (infer.c:755-949, 985-1003), after everything queued before it has finished.
//   exact mode (exact_kernels = true): the same operators and bits with no phase call in between, so that the step can be captured:
//     embed -> L x [exact rmsnorm -> q|k|v -> exact attention (q/k prep inside) -> Wo (+residual) -> exact rmsnorm -> W1|W3 -> SwiGLU ->
//     W2 (+residual)] -> exact rmsnorm -> classifier -> arg-max / loop feedback.  Every kernel reads pos[b] from device memory: one graph
//     serves every position.  Where att[max_seq_len] does not fit the one-launch attention's LDS (exact_attention_fits) the layer keeps
//     strict mode's attention launches with att in global memory.
static hipError_t strict_phase(NanoHipModel *m, int32_t layer, int32_t phase) {
    if (!m->phase_fn) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(m->st);
    if (e != hipSuccess) return e;
    m->phase_fn(m->phase_env, layer, phase);
    return hipSuccess;
}
// out = W . act for one weight tensor / a run of them, strict flavour: FP32 -> sequential matmul per segment (residual
// added in place), Q80 / Q4K -> the bit-exact GEMV kernels on the un-normalised input
static hipError_t strict_project(NanoHipModel *m, GemvArgs a) {
    if (m->d.quant_type != NANO_QUANT_F32) return gemv(m, a);
    for (uint32_t s = 0; s < a.nseg; s++) {
        const GemvSeg &g = a.seg[s];
        const hipError_t e = launch_strict_matmul_f32(g.out, a.xin, reinterpret_cast<const float *>(g.w), a.n, g.rows, a.nb, a.xin_bstride,
                                                      g.out_bstride, g.out_pstride, a.pos, a.epi == GEMV_EPI_RESID, m->st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// (the caller has asked step_served(): neither the LoRA side branches nor the FP16 / paged KV cache are on)
static hipError_t enqueue_step_ordered(NanoHipModel *m, const StepSpec &s, bool exact_kernels) {
    const NanoModelDesc &d = m->d;
    const uint32_t E = d.n_embd, H = d.n_hidden, QD = m->QD, KD = m->KD, L = d.n_layer, S = m->S;
    const uint32_t nb = s.nb, is_causal = s.is_causal, mode = s.mode, slot0 = s.slot;
    const bool one_launch = exact_kernels && exact_attention_fits(m->hd, S) && KD % 4u == 0;
    hipError_t e;
#define ST(expr) do { if ((e = (expr)) != hipSuccess) return e; } while (0)
    // the two things the modes do differently between operators.  A step that is captured makes no phase call at all, not even the
    // early-out one: nothing that could synchronise may sit in a capture.
    auto phase = [&](int32_t layer, int32_t ph) { return exact_kernels ? hipSuccess : strict_phase(m, layer, ph); };
    auto rmsnorm = [&](const float *w) { return exact_kernels ? launch_exact_rmsnorm(m->xn, m->x, w, E, nb, E, E, m->st) : launch_strict_rmsnorm(m->xn, m->x, w, E, nb, E, E, m->st); };
    ST(phase(-1, 1));                                                   // NANO_LLM_PHASE_EMBEDDING
    ST(launch_embed(embed_args(m, s), nb, m->st));
    const KvRows kv = KvRows::of(m, s);
    for (uint32_t l = 0; l < L; l++) {
        ST(phase(l, 2));                                                // ATTN_NORM   infer.c:755-758
        ST(rmsnorm(m->rms_attn + (size_t)l * E));
        ST(phase(l, 3));                                                // QKV         infer.c:768-786
        ST(strict_project(m, qkv_args(m, l, nb, m->xn, nullptr, kv.v_target(l))));
        ST(phase(l, 4));                                                // QK_ROPE     infer.c:812-835
        StrictAttnArgs sa{};
        sa.q = m->q; sa.kraw = m->kraw; sa.kcache = m->kcache; sa.vcache = m->vcache; sa.pos = m->pos;
        sa.q_norm = m->q_norm ? m->q_norm + (size_t)l * m->hd : nullptr;
        sa.k_norm = m->k_norm ? m->k_norm + (size_t)l * m->hd : nullptr;
        sa.rope_cos = m->rope_cos; sa.rope_sin = m->rope_sin; sa.att = m->att; sa.xba = m->xba;
        sa.n_head = d.n_head; sa.n_kv_head = d.n_kv_head; sa.hd = m->hd; sa.q_dim = QD; sa.kv_dim = KD;
        sa.layer = l; sa.n_layer = L; sa.S = S; sa.slot0 = slot0; sa.rope_qwen3 = (d.arch == NANO_ARCH_QWEN3); sa.is_causal = is_causal;
        if (one_launch) {                                               // exact.hip: both in one launch
            sa.fold_prep = 1;
            ST(launch_exact_attention(sa, nb, m->st));
        } else {
            ST(launch_strict_qk(sa, nb, m->st));
            ST(phase(l, 5));                                            // MHA         infer.c:839-879
            ST(launch_strict_attention(sa, nb, m->st));
        }
        ST(phase(l, 6));                                                // O           infer.c:883-908
        ST(strict_project(m, wo_args(m, l, nb, 1)));
        ST(phase(l, 7));                                                // FFN_NORM    infer.c:912-914
        ST(rmsnorm(m->rms_ffn + (size_t)l * E));
        ST(phase(l, 8));                                                // W1W3        infer.c:919-944
        ST(strict_project(m, w13_args(m, l, nb, m->xn, nullptr, m->hb2, GEMV_EPI_STORE)));
        ST(launch_strict_swiglu(m->hb, m->hb2, H, nb, H, m->st));
        ST(phase(l, 9));                                                // W2          infer.c:948-965
        ST(strict_project(m, w2_args(m, l, nb)));
    }
    if (mode == MODE_NOCLS) return hipSuccess;
    ST(phase(L, 10));                                                   // FINAL_NORM  infer.c:997-999
    ST(rmsnorm(m->rms_final));
    ST(phase(L, 11));                                                   // CLASSIFY    infer.c:1003-1015
    {
        GemvArgs a = classifier_args(m, nb, m->logits);
        a.xin = m->xn; a.norm_w = nullptr;
        ST(strict_project(m, a));
    }
    if (mode == MODE_ARGMAX || mode == MODE_LOOP) {
        ArgmaxArgs aa = argmax_args(m, nb, m->logits, m->amax);
        if (mode == MODE_LOOP) { aa.tokens = m->tokens; aa.trace = m->trace; }
        ST(launch_argmax(aa, nb, m->st));
    }
#undef ST
    return hipSuccess;
}
// scratch of the reference-order step (strict and exact mode): normalised x, the W3 output, att in global memory
static int ordered_scratch(NanoHipModel *m) {
    if (m->xn) return 0;
    const size_t Bs = m->Bs;
    if (hipMalloc(&m->xn, Bs * m->d.n_embd * 4) != hipSuccess || hipMalloc(&m->hb2, Bs * m->d.n_hidden * 4) != hipSuccess ||
        hipMalloc(&m->att, Bs * (size_t)m->d.n_head * m->S * 4) != hipSuccess)
        FAIL(NANO_HIP_ENOMEM, "hipMalloc for the scratch of strict / exact mode failed");
    return 0;
}

static int set_ordered(NanoHipModel *m, bool NanoHipModel::*mode, int on) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    HIP_TRY(hipSetDevice(m->device));
    if (on) { const int rc = ordered_scratch(m); if (rc) return rc; }
    m->*mode = on != 0;
    return NANO_HIP_OK;
}
extern "C" int nano_hip_set_strict(NanoHipModel *m, int on) { return set_ordered(m, &NanoHipModel::strict, on); }
extern "C" int nano_hip_set_exact(NanoHipModel *m, int on) { return set_ordered(m, &NanoHipModel::exact, on); }

extern "C" int nano_hip_exact_state(const NanoHipModel *m, uint32_t *on, uint32_t *graphs, uint32_t *launches_per_step) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    if (on) *on = m->exact ? 1u : 0u;
    if (graphs) *graphs = (uint32_t)m->exact_nodes.size();
    if (launches_per_step) *launches_per_step = m->exact_launches;
    return NANO_HIP_OK;
}

extern "C" int nano_hip_set_phase_hook(NanoHipModel *m, nano_hip_phase_fn fn, void *env) {
    if (!m) FAIL(NANO_HIP_EINVAL, "null model");
    m->phase_fn = fn; m->phase_env = env;
    return NANO_HIP_OK;
}

// ---- which step serves the model's switches, and which combinations none does ----
bool strict_serves(const NanoHipModel *m) { return m->strict || (m->exact && m->phase_fn); }   // strict wins; the hook needs the eager per-operator replay
bool exact_serves(const NanoHipModel *m) { return m->exact && !strict_serves(m); }
// THE place that says which combinations of (strict, exact, phase hook, LoRA, FP16 KV, paged KV) are served: asked by run_step and
// nano_hip_prefill before they queue anything.  The reference-order step has neither the LoRA side branches nor the FP16 or paged
// cache; the fast step has no LoRA side branches on a paged, FP16 or FP8 cache (they write FP32 v rows of the contiguous cache).
// That holds for decode and batched prefill alike: on the FP16 cache the fresh v row goes to vraw (KvRows::v_target) while the v branch
// would read-modify-write FP32 at a float offset into a cache of halfs -- twice the byte offset, from half of the layers on beyond the
// slot; on the FP8 cache, byte rows, from a quarter of the layers on beyond the allocation.
int step_served(const NanoHipModel *m, bool prefill) {
    if (strict_serves(m) || exact_serves(m)) {
        const char *mode = m->strict ? "strict mode" : exact_serves(m) ? "exact mode" : "exact mode with a phase hook";
        if (m->kv.paged) FAIL(NANO_HIP_EINVAL, "the paged KV cache is served by the fused path only: not with %s", mode);
        if (m->lora_on || m->kv_half) FAIL(NANO_HIP_EINVAL, "%s covers neither the LoRA side branches nor the FP16 KV cache", mode);
        return 0;
    }
    if (m->kv.paged && m->lora_on) FAIL(NANO_HIP_EINVAL, "the paged KV cache is served by the fused path only: not with the LoRA side branches");
    if (m->kv_half && m->lora_on) FAIL(NANO_HIP_EINVAL, "the LoRA side branches write FP32 v rows: not available with the FP16 KV cache");   // (FP8 too: the same message)
    (void)prefill;                      // (no combination is served for one and refused for the other any more)
    return 0;
}
// the policy of the decode steps: either failure fails the call
static int graph_step_check(const GraphRun &r) {
    if (r.step != hipSuccess) FAIL(NANO_HIP_ERUNTIME, "queueing a decode step failed: %s", hipGetErrorString(r.step));
    if (r.capture != hipSuccess) FAIL(NANO_HIP_ERUNTIME, "graph capture of a decode step failed: %s", hipGetErrorString(r.capture));
    return 0;
}
// one reference-order step of the sequences in KV slots slot0 .. slot0 + nb - 1 (the caller has asked step_served()).  Strict mode
// runs eagerly; exact mode replays one graph per (batch, mode, is_causal, slot0).
int run_step_ordered(NanoHipModel *m, uint32_t nb, uint32_t is_causal, uint32_t mode, uint32_t slot0) {
    const bool exact = exact_serves(m);
    const StepSpec s = StepSpec::seqs(nb, is_causal, mode, 0, slot0);
    const uint64_t key = (exact && m->use_graph) ? step_key(m, s, 0, true) : STEP_NO_KEY;
    m->nsplit = xba_nsplit(m, s, true);                                    // 1: xba holds final head outputs (nano_hip_read_state, also from inside the hook)
    if (key == STEP_NO_KEY) {
        HIP_TRY(enqueue_step_ordered(m, s, exact));
        if (exact) m->exact_launches = 0;
        return 0;
    }
    const GraphRun r = graph_step(m, key, [&, s] { return enqueue_step_ordered(m, s, true); });
    if (const int rc = graph_step_check(r)) return rc;
    if (r.stored) m->exact_nodes[key] = r.nodes;
    m->exact_launches = m->exact_nodes[key];
    return 0;
}
// the tokens and positions of a step's sequences: through the pinned staging rows to the device, on the model's stream (also_pos0: the
// greedy loop's first positions too).  *max_pos = the largest position among them.
int stage_batch(NanoHipModel *m, const uint32_t *tokens, const uint32_t *pos, uint32_t batch, bool also_pos0, uint32_t *max_pos) {
    if (tokens != m->h_tokens) memcpy(m->h_tokens, tokens, batch * 4);
    if (pos != m->h_pos) memcpy(m->h_pos, pos, batch * 4);
    HIP_TRY(hipMemcpyAsync(m->tokens, m->h_tokens, batch * 4, hipMemcpyHostToDevice, m->st));
    HIP_TRY(hipMemcpyAsync(m->pos, m->h_pos, batch * 4, hipMemcpyHostToDevice, m->st));
    if (also_pos0) HIP_TRY(hipMemcpyAsync(m->pos0, m->h_pos, batch * 4, hipMemcpyHostToDevice, m->st));
    uint32_t mp = 0;
    for (uint32_t i = 0; i < batch; i++) if (pos[i] > mp) mp = pos[i];
    if (max_pos) *max_pos = mp;
    return 0;
}
// Host-side upper bound of the attended range of a step of nb sequences, the largest position among them max_pos (<= S).
// The attention kernel issues its K / V loads before it knows pos (one memory round trip saved): it loads the rows below
// range_hint and masks those beyond pos.  The hint is rounded up to the 64 positions of a split's range.  Round 3 measured
// a hint rounded to 16 (the last block's rows beyond it are not fetched; four times as many graphs): 1845.9 vs 1846.0 tok/s
// at positions 20..39, 1709.6 vs 1707.8 over 31..510 -- an out-of-range load still costs its issue slot, and that, not
// the bytes, is what the kernel's load phase pays for.
// Round 4, batched steps (>= 9 sequences): the hint is rounded to 16.  At 64 sequences the K / V rows are the larger part of a
// Qwen3-0.6B step's bytes (33.5 MB per layer at a 64-row hint against 15.7 MB of weights) and the rows between the position and the
// hint are fetched for nothing: measured on one box 1.632 / 1.602 ms per step (hint step 64) vs 1.540 / 1.545 (16) at 64 sequences,
// 1.090 / 1.102 vs 1.057 / 1.044 at 16; Qwen3-4B 64 sequences 3.864 / 3.870 vs 3.811 / 3.836.  Same split count (ceil(hint / 64)),
// same bits; four times as many graphs per context.
// (batched prefill asks with nb = 1 whatever the chunk holds and so keeps the 64-position hint: a chunk's tokens must split exactly as
//  each token's own decode step does, and with head_dim > 128 -- 32 positions per workgroup and split -- ceil(round16(p + 1) / 32) is
//  not ceil(round64(p + 1) / 32))
uint32_t range_hint_of(const NanoHipModel *m, uint32_t nb, uint32_t is_causal, uint32_t max_pos) {
    const uint32_t hint_step = nb >= 9u ? 16u : 64u;
    const uint32_t hint = is_causal ? ((max_pos + hint_step) / hint_step) * hint_step : m->S;
    return hint > m->S ? m->S : hint;
}
// max_pos: largest position among the sequences of this step (host knowledge; the device reads the exact pos[b])
int run_step(NanoHipModel *m, uint32_t nb, uint32_t is_causal, uint32_t mode, uint32_t max_pos, bool skip_embed) {
    if (const int rc = step_served(m, false)) return rc;
    if (strict_serves(m) || exact_serves(m)) return run_step_ordered(m, nb, is_causal, mode, 0);
    StepSpec s = StepSpec::seqs(nb, is_causal, mode, range_hint_of(m, nb, is_causal, max_pos));
    s.skip_embed = skip_embed;
    // (measurement builds: NANO_STAMPS_GRAPH=1 captures the stamped step too -- the stamp slots are baked into a graph of its own key)
#if NANO_STAMPS
    static const bool stamps_graph = getenv("NANO_STAMPS_GRAPH") && *getenv("NANO_STAMPS_GRAPH") == '1';
#else
    constexpr bool stamps_graph = false;
#endif
    const uint64_t key = (m->use_graph && (!m->stamp.on || stamps_graph)) ? step_key(m, s) : STEP_NO_KEY;
    m->nsplit = xba_nsplit(m, s);
    if (key == STEP_NO_KEY) { HIP_TRY(enqueue_step(m, s)); return 0; }
    return graph_step_check(graph_step(m, key, [&, s] { return enqueue_step(m, s); }));
}
