// route.hip -- which kernel a projection launch (out = W . act, one weight tensor or a run of them sharing the activation) goes to.
// ONE router for the decode step (backend_step.hip), batched prefill and the operator entry points (ops.hip), so that the operator tests
// exercise exactly the launches a step issues.
//
//   FP32 / Q4K              the GEMV kernels (gemv_f32.hip, gemv_q4k.hip), more sequences than fit a launch's LDS (at most 8) in groups
//   FP32, 9..64 sequences   the activation prologue launch + the FP32 MFMA GEMM (gemm_f32.hip) where it takes the launch: same bits
//   Q4K, 9..64 sequences    the staged-group quantizer launch + the int8 MFMA GEMM (gemm_q4k.hip) where it takes the launch: same bits
//   Q80, fast path          SLAB GEMV (1..8 sequences on the small per-layer matrices; 1..2 on those of >= 8 M weights)   gemv_q80_impl.h
//                           the batched kernels, fragment-order activations: whichever gemm_q80_plan() names      gemm_q80_host.h
//                             canonical launches (group size 64, rows a multiple of 256): G7K (3..48 tokens, one row tile per CU, long
//                             rows), G7 (17..64 tokens: loader / consumer engine), G6 (2..64 tokens: MODE S staged in LDS, MODE F per item)
//                             the others (other group sizes and row lengths, the classifier): GC (the classifier, 2..64 tokens), G2
//                           STREAM GEMV for the classifier of up to 7 sequences                           gemv_q80_impl.h
//   Q80, strict mode        the kernels that keep the reference's ascending group order: SLAB, GC, G2 (a.ordered = 1)
//   what no batched kernel takes runs through the GEMV kernels in groups that fit a CU's LDS (ROUTE_GEMV_SLICED)
#include <stdlib.h>
#include "gemm_q80_host.h"

namespace nano {

// every workgroup of a multi-sequence GEMV launch re-quantizes the nb x n activations: ~ workgroups x elements of redundant work
static bool gemv_is_heavy(const GemvArgs &a) { return (uint64_t)(gemv_total_rows(a) / 16) * a.nb * a.n > (4u << 20); }
// per-layer matrices of >= 8 M weights (Qwen3-4B's): bandwidth rather than latency bound
bool route_is_wide(const GemvArgs &a) { const uint32_t rows = gemv_total_rows(a); return rows < 65536u && (uint64_t)rows * a.n >= (8u << 20); }

// the rmsnorm sum-of-squares tree the activation quantizer launch must repeat for this matrix (launch_quant_rows_frag order)
// (512 threads on the wide matrices -- the order the >= 3-sequence launches of Qwen3-4B have had since round 4; the one- and
// two-sequence SLAB launches of those matrices run the tree of their own thread count, see kernels.h "what a batch shares")
uint32_t route_norm_order(const GemvArgs &a) {
    return (q80_canonical(a) && route_is_wide(a) && a.n <= 10240u) ? 512u : 256u;
}

// The batched Q80 launch of `a`, whole, or false.  The order of preference lives here: canonical launches G7K, G7, G6 (each where its
// planner says it pays); the others GC, then G2.  (A CANONICAL launch none of the three takes does not go to G2, whose fold is the
// reference's: it would no longer be bit for bit its sequences alone.)
bool gemm_q80_plan(const GemvArgs &a, Q80GemmPlan *p) {
    using Section = bool (*)(const GemvArgs &, Q80GemmPlan &);
    static const Section canon[] = {q80_gemm_plan_g7k, q80_gemm_plan_g7, q80_gemm_plan_g6}, other[] = {q80_gemm_plan_gc, q80_gemm_plan_g2};
    const bool c = q80_canonical(a);
    for (uint32_t i = 0; i < (c ? 3u : 2u); i++) {
        *p = Q80GemmPlan{};
        if ((c ? canon : other)[i](a, *p)) { p->norm_order = route_norm_order(a); return true; }
    }
    *p = Q80GemmPlan{};
    return false;
}

RouteKind route_kind(const Q80Route &r, const GemvArgs &a, Q80GemmPlan *gp) {
    if (r.quant == NANO_QUANT_Q4K) {
        // from mfma_min_nb sequences on (9; NANO_MFMA_MIN_NB=65 restores the slices of 8: the A/B switch Q80 has) every weight byte is read
        // once per launch; what the GEMM refuses (gemm_q4k_supports()) keeps the slices
        if (a.nb >= r.mfma_min_nb && r.q4x && (uint64_t)a.nb * a.n <= r.q4x_bytes && gemm_q4k_supports(a)) return ROUTE_Q4K_GEMM;
        return ROUTE_Q4K;
    }
    if (r.quant != NANO_QUANT_Q80) {
        // FP32: from f32_min_nb sequences on every weight byte is read once per launch; what the GEMM refuses (gemm_f32_plan()) keeps the slices
        F32GemmPlan fp;
        if (r.f32_min_nb && a.nb >= r.f32_min_nb && r.f32x && gemm_f32_plan(a, &fp) && fp.xs_floats <= r.f32x_floats) return ROUTE_F32_GEMM;
        return a.nb > 8 ? ROUTE_GEMV_SLICED : ROUTE_GEMV;
    }
    const bool scratch = r.gq && r.gxs;
    const bool canon = q80_canonical(a);
    const bool wide = route_is_wide(a);
    // two sequences on wide matrices: the balanced SLAB GEMV (capacity 2) -- measured against G6 MODE P on one box, round 5: Qwen3-4B 1.833 vs
    // 1.923 ms per step (profiles/r05_wide_two_sequences.txt); from three sequences on the batched route is the faster one (four: 1.99 vs 2.80)
    if (canon && wide && a.nb == 2 && !a.xq_in) return ROUTE_GEMV;
    // the batched route: 9..64 sequences always (mfma_min_nb); 8 sequences when the matrix is large; per-layer matrices of >= 8 M weights
    // from 2 sequences on; the classifier keeps its STREAM GEMV up to 7 sequences
    const bool batched = scratch && (a.nb >= r.mfma_min_nb || (r.mfma_min_nb == 9 && ((a.nb == 8 && gemv_is_heavy(a)) || (wide && a.nb >= 2))));
    Q80GemmPlan own;
    Q80GemmPlan &p = gp ? *gp : own;
    if (batched && gemm_q80_plan(a, &p)) {
        if (p.kernel == Q80_GEMM_G7 || p.kernel == Q80_GEMM_G7K) return ROUTE_FRAG_G7;
        if (!a.attn_part && !a.resid_add) return p.kernel == Q80_GEMM_GC || p.kernel == Q80_GEMM_G2 ? ROUTE_FRAG_OLD : ROUTE_FRAG_G6;
    }
    p = Q80GemmPlan{};                                                  // (a plan leaves here only behind a ROUTE_FRAG_* answer)
    if (a.nb > 8) return ROUTE_GEMV_SLICED;
    if (a.nb > 1 && !a.attn_part && !a.xq_in && scratch && gemv_is_heavy(a)) return ROUTE_GEMV_PREQ;
    return ROUTE_GEMV;
}

// the sequences [b0, b0 + cnt) of a launch, as a launch of their own (every per-sequence pointer advanced)
static GemvArgs gemv_slice(const GemvArgs &a, uint32_t b0, uint32_t cnt) {
    GemvArgs s = a;
    s.nb = cnt;
    for (uint32_t i = 0; i < a.nseg; i++) if (s.seg[i].out) s.seg[i].out += (size_t)b0 * a.seg[i].out_bstride;
    if (a.xin) s.xin += (size_t)b0 * a.xin_bstride;
    if (a.pos) s.pos += b0;
    if (a.xq_in) s.xq_in += (size_t)b0 * ((a.n + 15) & ~15u);
    if (a.xs_in) s.xs_in += (size_t)b0 * (a.n / a.gs);
    if (a.attn_part) { s.attn_part += (size_t)b0 * a.attn_nsplit * a.n; s.attn_ml += (size_t)b0 * a.attn_n_head * a.attn_nsplit * 2; }
    if (a.resid_add) s.resid_add += (size_t)b0 * a.resid_add_bstride;
    s.tile_max = nullptr;
    return s;
}

// sequences of one launch: what the format's kernels fit in a CU's LDS (8 | 4 | 2 | 1; 0: not even one); a.nb = min(sequences, 8)
static uint32_t gemv_fit_batch(uint32_t quant, const GemvArgs &a) {
    if (quant == NANO_QUANT_Q80) return gemv_q80_fit_batch(a);
    if (quant != NANO_QUANT_Q4K) return gemv_f32_fit_batch(a);
    // the chunk form stages every sequence's activation once and shares every weight byte among up to 8 sequences (round 5); the item
    // kernel's workgroups stage the whole quantized activation of each sequence: long rows (Qwen3-4B's hidden size) take fewer per launch
    Q4kGemvPlan p;
    if (gemv_q4k_plan(a, &p) && p.kernel == Q4K_KERNEL_CHUNK) return 8u;
    return gemv_q4k_fit_batch(a);
}
bool route_gemv_slices(uint32_t quant, const GemvArgs &a, uint32_t *per, uint32_t *launches) {
    if (a.nb == 0) return false;
    GemvArgs one = a; one.nb = a.nb < 8u ? a.nb : 8u;
    const uint32_t fit = gemv_fit_batch(quant, one);
    if (fit == 0) return false;
    *per = a.nb < fit ? a.nb : fit;
    *launches = (a.nb + fit - 1) / fit;
    return true;
}
// What route_projection() writes into the arguments on every path, before it asks route_kind() or launches: the device's compute units and
// the Q4K scratch (null / 0 in the route of every other format, where the fields are null / 0 already).  The one place they are written:
// whoever must see a launch as it will be issued (route_partials() below, the plan queries of ops.hip) calls this, and mirrors nothing.
void route_fill(const Q80Route &r, GemvArgs &a) {
    a.cus = (uint32_t)r.cus;
    a.q4_scratch = r.q4x; a.q4_scratch_bytes = r.q4x_bytes;
}
// The (max, row) arg-max pairs per sequence the launch route_projection(r, a) issues is asked for (GemvArgs::tile_max) and writes; 0: it
// is not asked.  Asked: one STORE tensor of at most 8 sequences on a route that takes no fragments, and for Q4K a batch
// route_gemv_slices() leaves in one launch (gemv_slice(): a sliced launch writes none); the count is gemv_tiles() of the launch with
// the request made (the planners read tile_max as a flag).  The step's classifier (backend_step.hip enqueue_classifier) and the
// operator entry point (ops.hip nano_hip_op_fused_gemv) both ask here, a.tile_max still null, and hand the launch their buffer where
// the answer is not 0, so that an operator test runs the launch a step runs.  a.ordered as the launch will carry it.
// (A launch that is asked but writes no pairs -- FP32, the Q80 SLAB kernel, the Q4K chunk kernel's 2..8 sequences -- used to carry the
// buffer unread; it no longer does.  Only the Q4K GEMM, which refuses a launch that carries one, can tell: with NANO_MFMA_MIN_NB = 2..8
// such a classifier launch now takes the GEMM that switch asks for.  Same bits; nothing moves at the default 9.)
// FINDING, left as it was: Q80 is not asked how many launches the batch takes.  A STREAM classifier on rows of more than ~18 200 values
// at 5..8 sequences (group size 32: 18 432 values run as 4 + 1) is cut by route_gemv_slices(), its slices write no partials, and
// gemv_tiles() still reports STREAM_WGS * 4 of them.  No model has such rows; the one-launch test of Q4K would close it.
uint32_t route_partials(const Q80Route &r, GemvArgs a) {
    static float asked;                                                 // stands for the caller's buffer: compared with null, never followed
    route_fill(r, a);
    if (a.epi != GEMV_EPI_STORE || a.nseg != 1 || a.nb > 8 || route_takes_fragments(route_kind(r, a))) return 0;
    uint32_t per = 0, launches = 0;
    if (r.quant == NANO_QUANT_Q4K && !(route_gemv_slices(r.quant, a, &per, &launches) && launches == 1)) return 0;
    a.tile_max = &asked;
    return gemv_tiles(r.quant, a);
}
// the GEMV launches of a.nb sequences, cut where route_gemv_slices() says so; a shape of which not even one sequence fits is refused
// before any launch
static hipError_t launch_gemv_sliced(uint32_t quant, const GemvArgs &a, hipStream_t st) {
    uint32_t per = 0, launches = 0;
    if (!route_gemv_slices(quant, a, &per, &launches)) return hipErrorInvalidValue;
    const auto launch = quant == NANO_QUANT_Q80 ? launch_gemv_q80 : quant == NANO_QUANT_Q4K ? launch_gemv_q4k : launch_gemv_f32;
    if (launches == 1) return launch(a, st);
    for (uint32_t b0 = 0; b0 < a.nb; b0 += per) {
        const hipError_t e = launch(gemv_slice(a, b0, a.nb - b0 < per ? a.nb - b0 : per), st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t route_projection(const Q80Route &r, GemvArgs &a, hipStream_t st) {
    route_fill(r, a);
    Q80GemmPlan gp{};
    const RouteKind k = route_kind(r, a, &gp);
    if (k == ROUTE_F32_GEMM) {
        a.f32_scratch = r.f32x; a.f32_scratch_floats = r.f32x_floats;
        return launch_gemm_f32(a, st);
    }
    if (r.quant != NANO_QUANT_Q80 && r.quant != NANO_QUANT_Q4K) return launch_gemv_sliced(r.quant, a, st);      // FP32 (ROUTE_GEMV | ROUTE_GEMV_SLICED)
    switch (k) {
    case ROUTE_Q4K:
        return launch_gemv_sliced(r.quant, a, st);
    case ROUTE_Q4K_GEMM:
        return launch_gemm_q4k(a, st);
    case ROUTE_FRAG_G6:
    case ROUTE_FRAG_G7:
    case ROUTE_FRAG_OLD: {
        // quantize every sequence's activation once, straight into MFMA fragment order (unless the producing kernel already did), then
        // the GEMM the plan names
        if (!a.frag_ready) {
            const hipError_t e = launch_quant_rows_frag(a.xin, a.xin_bstride, a.norm_w, a.n, a.gs, a.nb, r.gq, r.gxs, st, gp.norm_order);
            if (e != hipSuccess) return e;
        }
        a.xq_in = r.gq; a.xs_in = r.gxs;
        switch (gp.kernel) {
        case Q80_GEMM_G6S: case Q80_GEMM_G6F: return launch_gemm_q80_g6(a, gp, st);
        case Q80_GEMM_G7: case Q80_GEMM_G7K: return launch_gemm_q80_g7(a, gp, st);
        case Q80_GEMM_GC: return launch_gemm_q80_cls(a, gp, st);
        default: return launch_gemm_q80_g2(a, gp, st);
        }
    }
    case ROUTE_GEMV_SLICED:
        // More sequences than a GEMV launch takes and a launch no batched kernel takes (row length / group size not a multiple of 4
        // groups, segment rows not multiples of 16, the LoRA o-branch addend, product tables beyond a CU's LDS): groups of 8 through the
        // GEMV kernels.  Same arithmetic per sequence, the weights are read once per group (of fewer than 8 where 8 do not fit a CU's LDS).
        return launch_gemv_sliced(r.quant, a, st);
    case ROUTE_GEMV_PREQ: {
        // when the redundant quantization outweighs a launch (~3 us) the activations are quantized once (quant_rows_kernel) and the GEMV
        // reads them back
        const hipError_t e = launch_quant_rows(a.xin, a.xin_bstride, a.norm_w, a.n, a.gs, a.nb, r.gq, r.gxs, st);
        if (e != hipSuccess) return e;
        a.xq_in = r.gq; a.xs_in = r.gxs; a.norm_w = nullptr;
        return launch_gemv_sliced(r.quant, a, st);
    }
    case ROUTE_GEMV:
    default:
        return launch_gemv_sliced(r.quant, a, st);
    }
}

}  // namespace nano
