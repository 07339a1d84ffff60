// gemv_q80.hip -- dispatcher and launch planner of the Q80 (W8A8) decode GEMVs; the kernels live in gemv_q80_impl.h, built once per
// quantization group size (gemv_q80_gs32/64/128/256.hip).
#include "gemv_q80_host.h"

namespace nano {

hipEvent_t g_q80_probe_start = nullptr, g_q80_probe_stop = nullptr;

hipError_t launch_gemv_q80_gs32(const GemvArgs &a, const Q80GemvPlan &p, hipStream_t st);
hipError_t launch_gemv_q80_gs64(const GemvArgs &a, const Q80GemvPlan &p, hipStream_t st);
hipError_t launch_gemv_q80_gs128(const GemvArgs &a, const Q80GemvPlan &p, hipStream_t st);
hipError_t launch_gemv_q80_gs256(const GemvArgs &a, const Q80GemvPlan &p, hipStream_t st);

// number of (max,row) arg-max partials a STORE launch with tile_max will write per sequence (0: none -- scan the logits)
uint32_t gemv_q80_partials(const GemvArgs &a) { return use_stream(a) ? STREAM_WGS * 4 : 0; }

// rows per workgroup / waves per workgroup of a slab launch (tuned on Qwen3-0.6B with the round-1 kernel laboratory: the chain
// time is flat within 3 % around these choices -- the kernels are latency bound)
SlabPlan q80_plan_slab(const GemvArgs &a, int B) {
    const uint32_t nchunk = (a.n + 1023) / 1024, nmat = a.epi == GEMV_EPI_SWIGLU ? 2 : 1;
    const uint32_t nseg = a.epi == GEMV_EPI_SWIGLU ? 1u : a.nseg;
    uint32_t align = 0;                                   // a workgroup's rows must lie inside one segment
    if (nseg > 1) for (uint32_t s = 0; s < nseg; s++) align |= a.seg[s].rows;
    const uint32_t rows = gemv_total_rows(a);
    // Every workgroup re-stages the activations (B x n elements), so the row slab grows until one wave of workgroups
    // covers the chip: the largest power of two with >= 256 workgroups (small matrices: ~4 units = 16 KiB of weights per
    // matrix and >= 128 workgroups, the tuned batch-1 optimum), bounded by the LDS product table.
    uint32_t rw = 4;
    while (rw < 32 && (align % (rw * 2)) == 0 && (rw * 2 / 4) * nchunk <= 4 && rows / (rw * 2) >= 128) rw *= 2;
    while (rw < 64 && (align % (rw * 2)) == 0 && rows / (rw * 2) >= 256) rw *= 2;
    {
        const uint32_t ng = a.n / a.gs, pitch = ((ng + 47) / 64) * 64 + 16;
        while (rw > 4 && (size_t)B * nmat * rw * pitch * 4 > 64 * 1024) rw /= 2;
        while (rw > 4 && (rw / 4) * nchunk * nmat > 64) rw /= 2;          // <= 16 waves x 4 units
    }
    // One workgroup per CU when the power of two leaves CUs idle (round 3, Qwen3-0.6B's W1|W3: 3072 rows as 192 slabs of 16 ->
    // 256 slabs of 12: 1871-1879 -> 1896 tok/s; the slab kernel takes any row count).  One-segment launches only.
    if (B == 1 && nseg == 1) {
        const uint32_t cus = a.cus ? a.cus : 256u, c = (rows + cus - 1) / cus;
        if (c >= 5 && c < rw && rows / rw < cus && ((c + 3) / 4) * nchunk * nmat <= 64) rw = c;
    }
    // Large matrices (Qwen3-4B's layers: 10-50 MB each) are bandwidth rather than latency bound, and a CU pulls ~25 GB/s whatever
    // it runs: the launch ends when the CU with the most rows ends.  BALANCED slabs (round 3): rw = ANY row count, chosen to
    // minimise (rounds of `cus` workgroups) x rw = the rows the busiest CU streams; a power-of-two slab left 160 of 256 CUs
    // busy on a 2560-row matrix (rw 16) where rw = 10 gives every CU one workgroup.  On a tie the larger slab (fewer
    // workgroups re-staging the activation).
    uint32_t large_nw = 0;
    // (round 5: TWO sequences on these matrices take the same balanced slabs, the product table twice as large -- Qwen3-4B at 2 sequences
    //  1.833 ms per step against 1.923 through G6 MODE P, same box; four sequences: 2.80 against 1.99 through G6, so two is where it ends)
    if (B <= 2 && (uint64_t)rows * a.n * nmat >= (8u << 20)) {
        const uint32_t cus = a.cus ? a.cus : 256u;
        uint32_t best = 0, best_cost = ~0u;
        const uint32_t ng = a.n / a.gs, pitch = (1024 / a.gs == 16) ? (((ng + 47) / 64) * 64 + 16) : (((ng + 3) & ~3u) + 4);
        for (uint32_t c = 4; c <= 64; c++) {
            const uint32_t tpw = (c + 3) / 4;
            if (tpw * nchunk * nmat > 64) break;                           // <= 16 waves x 4 units
            if ((size_t)B * nmat * tpw * 4 * pitch * 4 > 96 * 1024) break;     // product table
            uint32_t wgs = 0;
            if (nseg > 1) for (uint32_t s2 = 0; s2 < nseg; s2++) wgs += (a.seg[s2].rows + c - 1) / c; else wgs = (rows + c - 1) / c;
            // rows of the busiest CU; more than one workgroup per CU pays its prologue several times over on shared issue
            // slots (measured: QKV of Qwen3-4B, 768 workgroups of 8 rows 7.4 us vs 192 of 32 rows 6.9), so x 1.15 then
            uint32_t cost = ((wgs + cus - 1) / cus) * c * 100u;
            if (wgs > cus) cost += cost * 15u / 100u;
            if (cost <= best_cost) { best_cost = cost; best = c; }
        }
        if (best) {
            rw = best;
            const uint32_t u = ((rw + 3) / 4) * nchunk * nmat;
            large_nw = u / 2 < 8 ? 8 : (u / 2 > 16 ? 16 : u / 2);
        }
    }
    const uint32_t units = ((rw + 3) / 4) * nchunk * nmat;
    uint32_t nw = units < 4 ? units : 4;
    // (one sequence, re-swept on round 6's last day with the three-launch layer: a wave per 384 activation values -- W2 of Qwen3-0.6B on 8 waves
    //  instead of 6 -- 1994 / 1978 tok/s against 1979 / 1966 with 512, 1984 / 1972 with 448, 1952 / 1959 with 320; the five-launch form and Qwen3-4B: even)
    const uint32_t want_div = B == 1 ? 384u : 512u;
    uint32_t want = (a.n * (uint32_t)(B > 2 ? B / 2 : 1) + want_div - 1) / want_div;     // idle waves still help the activation prologue
    if (want > 16) want = 16;
    if (nw < want) nw = want;
    if (nw * 64 < rw * (uint32_t)B) nw = (rw * (uint32_t)B + 63) / 64;      // one fold thread per (row, sequence)
    if (nw < 2) nw = 2;
    uint32_t upw = (units + nw - 1) / nw;
    while (upw > 4 && nw < 16) { nw++; upw = (units + nw - 1) / nw; }
    if (large_nw) { nw = large_nw; upw = (units + nw - 1) / nw; while (upw > 4 && nw < 16) { nw++; upw = (units + nw - 1) / nw; } }
    // (Round 4 tried a raw barrier between the activation loads and the weight loads of the large slabs, so that every wave's activation
    // is asked for before any weight -- round 3 had measured the activation of Qwen3-4B's W1|W3 "arriving" with the end of the 52.9 MB
    // burst.  Measured on one box: 1.4707 ms per step with it, 1.4594 without.  The launch is bound by latency + stream + tail, not by
    // where the activation sits in the queue.  Removed.)
    SlabPlan p{rw, nw, upw, (a.n + 256 * nw - 1) / (256 * nw)};
    return p;
}

// The launch of `a`: which kernel, which instantiation, on how many waves and workgroups, with how much LDS.  Host arithmetic on shape
// fields and on pointers read as flags (norm_w, xq_in, attn_part, resid_add); nothing is dereferenced.
bool gemv_q80_plan(const GemvArgs &a, Q80GemvPlan *out) {
    if (a.nb == 0 || a.nb > 8 || !(a.gs == 32 || a.gs == 64 || a.gs == 128 || a.gs == 256) || a.n == 0 || a.n % a.gs || a.n % 16 || a.nseg == 0 || a.nseg > 3) return false;
    if (a.attn_part && (a.norm_w || a.attn_nsplit > 8 || a.attn_hd == 0 || a.attn_hd % 4)) return false;
    if (a.epi == GEMV_EPI_SWIGLU && a.nseg != 2) return false;
    if (a.epi != GEMV_EPI_SWIGLU && a.nseg > 1)
        for (uint32_t s = 0; s < a.nseg; s++) if (a.seg[s].rows % 4) return false;
    const uint32_t rows = gemv_total_rows(a);
    if (rows == 0) return false;
    const uint32_t B = a.nb <= 1 ? 1 : a.nb <= 2 ? 2 : a.nb <= 4 ? 4 : 8;
    const uint32_t f = (a.norm_w ? F_NORM : 0u) | (a.xq_in ? F_PRE : 0u) | (a.attn_part ? F_COMBINE : 0u);
    const uint32_t ng = a.n / a.gs;
    const uint64_t n16 = (a.n + 15) & ~15u, ng4 = (ng + 3) & ~3u;
    // activations [B][n16] int8 | their scales [B][ng4] | norm partials [B][16] -- what both kernels stage per sequence
    const uint64_t act = (uint64_t)B * n16 + (uint64_t)B * ng4 * 4 + (uint64_t)B * 64;
    Q80GemvPlan p{};
    p.gs = a.gs; p.B = B; p.pre = (f & F_PRE) ? 1u : 0u;
    if (use_stream(a)) {
        // STREAM: 1024 persistent workgroups of four waves, a wave owns 16-row tiles; NV float4 items of the activation per thread in
        // registers (0: the loop form); | the four waves' integer group sums [4][16][1024 / gs]
        p.kernel = Q80_KERNEL_STREAM;
        p.role = f == F_NORM ? (uint32_t)R_NORM_STORE : (uint32_t)R_GENERIC;
        const uint32_t nvr = (a.n + 1023) / 1024;
        p.nv = nvr <= 1 ? 1u : (B <= 4 && nvr <= 2) ? 2u : (B <= 2 && nvr <= 4) ? 4u : 0u;
        p.upw = 0; p.rw = 16; p.nw = 4; p.grid = STREAM_WGS;
        const uint64_t lds = act + 4ull * 16 * (1024 / a.gs) * 4;
        if (lds > GEMV_Q80_LDS_MAX) return false;
        p.lds_bytes = (uint32_t)lds;
        if (out) *out = p;
        return true;
    }
    const SlabPlan sp = q80_plan_slab(a, (int)B);
    if (sp.upw > 4) return false;
    p.kernel = Q80_KERNEL_SLAB;
    p.rw = sp.rw; p.nw = sp.nw;
    p.nv = sp.nv <= 1 ? 1u : sp.nv <= 2 ? 2u : sp.nv <= 4 ? 4u : 0u;      // float4 items a thread stages in registers; 0: the loop form
    if (B * p.nv > 8) p.nv = 0;                                           // too many staged registers: loop form
    p.upw = sp.upw <= 1 ? 1u : sp.upw <= 2 ? 2u : 4u;
    const bool sw = a.epi == GEMV_EPI_SWIGLU;
    const uint32_t nmat = sw ? 2u : 1u, nseg = sw ? 1u : a.nseg;
    // the matrices of >= 8 M weights, one or two sequences: the first unit of every wave's weights before the activation is quantized, the others
    // after (SLAB_EARLY).  Same box, interleaved (profiles/r06_slab_early_units.txt): Qwen3-4B one sequence 1.471 -> 1.427 ms per step, two
    // sequences 1.956 -> 1.825; the first TWO units early: no gain over none (one sequence), the same as one (two sequences).
    p.early = (B <= 2 && sp.upw >= 2 && (uint64_t)rows * a.n * nmat >= (8u << 20)) ? 1u : 0u;
    const uint32_t tpw = (sp.rw + 3) / 4, nchunk = (a.n + 1023) / 1024;
    p.units = tpw * nchunk * nmat;
    // workgroups per segment (a workgroup's rows lie inside one segment; the last one of a segment may be ragged)
    uint32_t wg[3] = {0, 0, 0};
    for (uint32_t s = 0; s < nseg; s++) wg[s] = (a.seg[s].rows + sp.rw - 1) / sp.rw;
    p.wg_c0 = nseg > 1 ? wg[0] : 0xffffffffu;
    p.wg_c1 = nseg > 2 ? wg[0] + wg[1] : 0xffffffffu;
    p.grid = wg[0] + wg[1] + wg[2];
    // the per-layer launches of a batch-1 step: flags resolved at compile time.  Group size 64: the role kernels carry the canonical fold
    // only, so a launch that is not canonical (strict mode; a row length that is no multiple of 256) takes the generic kernel
    p.role = R_GENERIC;
    if (B == 1 && (a.gs != 64 || q80_canonical(a))) {
        if (f == F_NORM && a.epi == GEMV_EPI_STORE) p.role = R_NORM_STORE;
        else if (f == 0 && a.epi == GEMV_EPI_RESID) p.role = R_RESID;
        else if (f == F_COMBINE && a.epi == GEMV_EPI_RESID) p.role = R_RESID_COMBINE;
        else if (f == F_NORM && a.epi == GEMV_EPI_SWIGLU) p.role = R_NORM_SWIGLU;
    }
    // | combine weights [B][n_head][8] | product table [B][nmat][4 tpw][pitch]
    const uint64_t pitch = (1024 / a.gs == 16) ? (((ng + 47) / 64) * 64 + 16) : (ng4 + 4);
    const uint64_t comb = (f & F_COMBINE) ? (uint64_t)B * a.attn_n_head * 32 : 0;
    uint64_t lds = act + comb + (uint64_t)B * nmat * (tpw * 4) * pitch * 4;
    GemvDev d = to_dev(a);
    d.early = p.early; d.tpw = tpw;
    p.variant = Q80_VAR_PLAIN;
    if (a.gs == 64 && B <= 2 && p.upw >= 2 && p.nv >= 1 && p.early) p.variant = Q80_VAR_EARLY;
    else if (a.gs == 64 && B == 1 && (p.role == R_NORM_STORE || p.role == R_NORM_SWIGLU) && (p.nv == 1 || p.nv == 2) && slab_wave_fold(d)) {
        p.variant = Q80_VAR_WF;                                            // no product table
        if (p.role == R_NORM_SWIGLU) p.units = (sp.rw + 1) / 2;            // pair units: two rows of W1 and the same two of W3
        lds = n16 + ng4 * 4 + 64;
    } else if (a.gs == 64 && B == 1 && (p.role == R_RESID || p.role == R_RESID_COMBINE) && (p.nv == 1 || p.nv == 2) && p.upw <= 2) {
        const uint32_t nch = slab_wave_fold_chunks(d);
        if (nch) {                                                         // unit sums [4 tpw][4 | 8] instead of the table
            p.variant = nch == 2u ? Q80_VAR_WFC2 : nch == 3u ? Q80_VAR_WFC3 : Q80_VAR_WFC4;
            lds = n16 + ng4 * 4 + 64 + comb + slab_unit_table(d, nch);
        }
    }
    // Behind split attention, one sequence, ONE item per thread: the splits' weights made inside each wave (SLAB_CW).  The table's bytes
    // stay in the request (a hole in the carve-up: the plan's lds_bytes do not depend on the form).  (Two items per thread -- Wo of n = 1280
    // or 2048 on the plain launch's four or six waves -- were built and are not shipped: bit-identical, but the compiler's code for the two
    // rounds of statistics loads has a wait for every load and late kernel-argument fetches inside the issue phase, which
    // tests/test_isa_hygiene.py forbids for good reason; those launches keep the table form.)
    p.cw = (a.gs == 64 && B == 1 && p.role == R_RESID_COMBINE && p.nv == 1 && p.variant != Q80_VAR_EARLY && combine_wave_shape(a)) ? 1u : 0u;
    if (lds > GEMV_Q80_LDS_MAX) return false;
    p.lds_bytes = (uint32_t)lds;
    if (out) *out = p;
    return true;
}

// sequences per launch whose LDS request a CU can meet (8 | 4 | 2 | 1; 0: not even one sequence, or a refused shape).  LDS grows with the
// capacity and nothing else of a refusal depends on it, so every smaller batch fits as well.
uint32_t gemv_q80_fit_batch(const GemvArgs &a) {
    GemvArgs t = a;
    for (uint32_t c = 8; c >= 1; c >>= 1) { t.nb = c; if (gemv_q80_plan(t, nullptr)) return c; }
    return 0;
}

hipError_t launch_gemv_q80(const GemvArgs &a, hipStream_t st) {
    Q80GemvPlan p;
    if (!gemv_q80_plan(a, &p)) return hipErrorInvalidValue;
    switch (a.gs) {
    case 32: return launch_gemv_q80_gs32(a, p, st);
    case 64: return launch_gemv_q80_gs64(a, p, st);
    case 128: return launch_gemv_q80_gs128(a, p, st);
    case 256: return launch_gemv_q80_gs256(a, p, st);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace nano
