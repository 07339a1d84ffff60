// gemv_q4k_chunk.hip -- Q4K (W4A4) fused GEMV for ONE sequence, weights read as 16-byte chunks (round 4).
//
// Same arithmetic as gemv_q4k.hip (reference infer/tensor.c:359-434 dot_two_blocks_q4k, 438-471 matmul_q4k: three integer sums
// per 32-weight group, the four-term float combine in the reference's operation order, the 8 groups of a block added in
// order, the blocks of a row added in order -> bit-identical fp32 for equal quantized inputs), another division of labour:
//
//   * gemv_q4k.hip deals (row, group) items to threads; each item costs three loads (16 nibble bytes + the block's 32 header
//     bytes, which the 8 groups of a block each fetch again) and twelve registers, a workgroup holds <= 4096 of them, and the
//     grid follows from that: 608 workgroups of 640 threads for Qwen3-4B's W1|W3, one resident per CU -> 2.4 rounds of a 7.9 us
//     workgroup (20 us per launch, `profiles/r04_stamps_q4k_before.txt`); 320 workgroups of 1024 for W2 -> two rounds, the second
//     one a quarter full, each workgroup quantizing all 9728 activations again (3.6 us).
//   * here a workgroup owns `rw` consecutive rows (any count: the grid is fitted to the chip, one round), which are ONE
//     contiguous run of 160-byte blocks.  Lane l < 60 of a wave reads chunk l of a 960-byte "wave-load" = six whole blocks:
//     one 16-byte load per lane, every byte of the matrix requested exactly once, four registers per load in flight.  Lane
//     l's role is fixed for the whole launch: c = l % 10 is the chunk inside the block (0, 1: the header; 2..9: the nibbles
//     of group c - 2), l / 10 the block of the wave-load.  The group lanes fetch the five header words they need from their
//     block's two header lanes (ds_bpermute), multiply against the staged activation group, and park the group value in a
//     wave-private LDS line; the block's first lane adds the eight in order and writes the block sum to the workgroup's
//     table [row][block]; one thread per row adds the blocks in order.  A ring of D loads per wave is in flight; the
//     classifier-like launches loop over it (persistent workgroups, the activation quantized once per workgroup).
//
// Restrictions (the router keeps gemv_q4k.hip for the rest): whole blocks (n % 256 == 0), n <= 16384.
//
// Round 5: 2 .. 8 sequences (template NB = 2 | 4 | 8).  Rounds 3-4 ran them through gemv_q4k.hip, whose workgroups each stage AND quantize
// every sequence's activation: Qwen3-4B's rows left room for one sequence per launch, i.e. no weight sharing at all (13.5 ms per 8-sequence
// step where one sequence takes 1.46).  Here the activations are normalised / combined and block-quantized ONCE, by q4k_quant_rows_kernel
// (one workgroup per sequence running exactly the one-sequence kernel's prologue: same thread count, same trees, same bits), which leaves
// the staged groups (XGroup: packed nibbles, sq, bq, nibble sum) in global memory; the projection workgroups copy them to LDS, read every
// weight byte once and multiply it against all NB sequences -- per wave-load the weight-only half once, the activation half per sequence.
#include "gemv_q4k_impl.h"
#include "gemv_q4k_host.h"
#include <hip/hip_ext.h>

namespace nano {

extern hipEvent_t g_q80_probe_start, g_q80_probe_stop;     // gemv_q80.hip: exact start / stop of the next classifier launch

namespace {

template <int ROLE, int NV, int D, bool LOOP, int NB = 1>
__global__ __launch_bounds__(1024) void gemv_q4k_chunk_kernel(const GemvDev a) {
    static_assert(NB == 1 || (ROLE == R_GENERIC && NV == 1), "several sequences: activations arrive quantized (q4k_quant_rows_kernel), generic role");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#define CHUNK_A a
#define CHUNK_BID blockIdx.x
#define CHUNK_HAND 0
#define CHUNK_HANDV (SlabHand{})
#define CHUNK_PTAG 0u
#include "gemv_q4k_chunk_body.inc"
#undef CHUNK_A
#undef CHUNK_BID
#undef CHUNK_HAND
#undef CHUNK_HANDV
#undef CHUNK_PTAG
}

}  // namespace
}  // namespace nano
#include "attn_impl.h"
namespace nano {
namespace {
// ---- q | k | v projection + attention in ONE launch (Qwen3 decode, one sequence, head_dim 128; round 6: what gemv_q80_impl.h's
//      qkv_attn_fused_kernel is for Q80) ---------------------------------------------------------------------------------------------------
// The first `ngemv` workgroups are the projection's chunk GEMV (role: rmsnorm + block quantizer + store), whose fold threads also store every
// result as an 8-byte {tag, value} granule; the LAST n_attn workgroups are the attention's (head x split): they ask for their K / V rows at
// entry, nap, then poll for q, the raw k row and the fresh v row of their KV group.  256 threads for both kinds (q4k_fused_shape).  Epoch tags, give-up and re-issue: device_common.h, backend.hip.  Reference: infer/infer.c:758-879.
template <int D>
__global__ __launch_bounds__(256) void q4k_qkv_attn_fused_kernel(const QkvAttnArgs fa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NV = 1;                                       // n <= 1024 on 256 threads: one float4 item per thread (q4k_fused_shape)
    const uint2 tk_ = hand_tick(fa.hand);                       // the step's epoch: the first load of every workgroup
    if (blockIdx.x >= fa.ngemv) {
        const uint32_t ab = blockIdx.x - fa.ngemv;
        const uint32_t split = ab / fa.head_wgs, grp = ab - split * fa.head_wgs;
        attention_body<8, 4, 1, 1, false, false, 2, false, true>(fa.a, smem, grp, 0u, split, fa.hand, hand_ctag(tk_, fa.hand), fa.wait16);
        return;
    }
    constexpr int ROLE = R_NORM_STORE, NB = 1;
    constexpr bool LOOP = false;
#define CHUNK_A fa.g
#define CHUNK_BID blockIdx.x
#define CHUNK_HAND 1
#define CHUNK_HANDV fa.hand
#define CHUNK_PTAG hand_ptag(tk_, fa.hand)
#include "gemv_q4k_chunk_body.inc"
#undef CHUNK_A
#undef CHUNK_BID
#undef CHUNK_HAND
#undef CHUNK_HANDV
#undef CHUNK_PTAG
}

// ---- the activations of a 2 .. 8-sequence launch, normalised / combined and block-quantized once -----------------------------------------
// One workgroup per sequence; its code is the one-sequence kernel's prologue (stage_issue -> stage_xn -> quantize_q4k_regs) run with the
// thread count the one-sequence launch of the same matrix would use, so every tree (rmsnorm sum of squares, split-attention combine) and
// therefore every quantized nibble is what that sequence gets when it is decoded alone.  Output: the staged groups, [sequence][GT] XGroups.
template <int ROLE, int NV>
__global__ __launch_bounds__(1024) void q4k_quant_rows_kernel(const GemvDev a, XGroup *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, nthr = a.nthr, n = a.n, GT = (n >> 8) * 8u, b = blockIdx.x;
    XGroup *xg = reinterpret_cast<XGroup *>(smem);
    float *red = reinterpret_cast<float *>(smem + (size_t)GT * sizeof(XGroup));
    GemvDev s = a;                                                  // this workgroup's sequence as a launch of its own (route.hip gemv_slice)
    s.nb = 1;
    if (a.xin) s.xin = a.xin + (size_t)b * a.xin_bstride;
    if (a.attn_part) { s.attn_part = a.attn_part + (size_t)b * a.attn_nsplit * n; s.attn_ml = a.attn_ml + (size_t)b * a.attn_n_head * a.attn_nsplit * 2u; }
    Staged<1, NV> sx;
    stage_issue<ROLE, 1, NV>(s, sx);
    stage_xn<ROLE, 1, NV>(s, sx, nullptr, red, (n + 3u) & ~3u, true);
    quantize_q4k_regs<1, NV, false>(s, sx, xg);
    __syncthreads();
    const uint4 *src = reinterpret_cast<const uint4 *>(xg);
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)b * GT);
    for (uint32_t i = tid; i < GT * 2u; i += nthr) dst[i] = src[i];
}

}  // namespace

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static size_t chunk_lds_bytes(uint32_t n, bool combine, uint32_t attn_n_head, uint32_t nmat, uint32_t rw, uint32_t nw, uint32_t sl, uint32_t nbq = 1) {
    const size_t bpl = n >> 8, GT = bpl * 8;
    return nbq * GT * sizeof(XGroup) + (16 + (combine ? (size_t)attn_n_head * 8 : 0) + (size_t)nw * sl * 64 + 2 * (size_t)nw + (size_t)nmat * nbq * rw * (bpl | 1)) * 4 + 16;
}

bool plan_chunk(const GemvArgs &a, ChunkPlan &p, uint32_t force_nw) {      // force_nw: the fused launch's 256 threads (same bits: see q4k_fused_shape)
    if (a.nb == 0 || a.nb > 8 || a.n == 0 || (a.n & 255u) || a.n > 16384u || a.nseg == 0 || a.nseg > 3) return false;
    if (a.attn_part && (a.norm_w || a.attn_nsplit > 8 || a.attn_hd % 4)) return false;
    const uint32_t nbq = a.nb <= 1 ? 1u : a.nb <= 2 ? 2u : a.nb <= 4 ? 4u : 8u;     // the kernel's NB (sequences beyond a.nb are skipped)
    if (nbq > 1 && (a.x4_in || a.xq_in)) return false;                              // (caller-quantized activations: one sequence)
    const bool sw = a.epi == GEMV_EPI_SWIGLU;
    const uint32_t nmat = sw ? 2u : 1u, nseg = sw ? 1u : a.nseg, bpl = a.n >> 8;
    const uint32_t rows = gemv_total_rows(a);
    if (rows == 0) return false;
    constexpr uint32_t want_div = 4u;
    uint32_t want = ((a.n / want_div + 63) / 64) * 64;                 // the block quantizer: four elements per thread and pass
    if (want < 256) want = 256;
    if (want > 1024) want = 1024;
    const bool cls = nseg == 1 && a.epi == GEMV_EPI_STORE && rows >= 65536u;
    const uint32_t cus = a.cus ? a.cus : 256u;
    // workgroups per CU: the per-layer matrices get one (every workgroup quantizes the activation: once per CU); the classifier's
    // activation is short next to its rows, its workgroups are persistent and small (4 x 256 threads at n = 1024)
    if (cls && want > 512) want = 1024;
    // (Measured and not taken, Qwen3-0.6B on one box: half the workgroups with twice the rows for Wo / W2, whose workgroups each bring
    // n / 4 quantizer threads: 1686 vs 1720 tok/s; the quantizer on n / 8 threads, two blocks per wave: 1661; three wave-loads per wave: 1640.)
    const uint32_t k = cls ? 1024u / want : 1u, target = cus * k;
    uint32_t best = 0, best_cost = ~0u;
    for (uint32_t c = 1; c <= 1024; c++) {
        if ((uint64_t)c * bpl >= 65536u) break;                          // the kernel's ceil(nblk / 6) and b / bpl by multiplication
        if (chunk_lds_bytes(a.n, nbq == 1 && a.attn_part != nullptr, a.attn_n_head, nmat, c, 16, 8, nbq) * k > GEMV_Q4K_CHUNK_SEARCH_LDS) break;
        uint32_t wgs = 0;
        for (uint32_t s = 0; s < nseg; s++) wgs += (a.seg[s].rows + c - 1) / c;
        // rows of the busiest CU slot; several rounds of workgroups pay the prologue (activation, norm, block quantizer) once per round
        uint32_t cost = ((wgs + target - 1) / target) * c * 100u;
        if (wgs > target) cost += cost * 15u / 100u;
        if (cost <= best_cost) { best_cost = cost; best = c; }          // ties: the larger slab (fewer workgroups staging the activation)
    }
    if (!best) return false;
    p.rw = best;
    const uint32_t TT = nmat * ((best * bpl + 5) / 6);
    uint32_t nw = want / 64;
    // one wave-load per wave where the workgroup's waves allow it (<= 16): every load at kernel entry, no serial second item
    constexpr uint32_t per_want = 2u;
    if (!cls) { uint32_t m = (TT + per_want - 1) / per_want; if (m > 16) m = 16; if (nw < m) nw = m; }
    if (force_nw) nw = force_nw;
    if (nw * 64 < best) nw = (best + 63) / 64;                           // one fold thread per row
    if (nw > 16) return false;
    uint32_t per = (TT + nw - 1) / nw;
    p.loop = per > 8;
    p.d = per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : 8;
    p.rounds = p.loop ? (per + 7) / 8 : 1;
    p.nthr = nw * 64;
    p.nv = (a.n / 4 + p.nthr - 1) / p.nthr;
    if (nbq == 1 && p.nv > 4) return false;
    p.grid = 0;
    for (uint32_t s = 0; s < 3; s++) { p.wg[s] = s < nseg ? (a.seg[s].rows + best - 1) / best : 0; p.grid += p.wg[s]; }
    p.lds = chunk_lds_bytes(a.n, nbq == 1 && a.attn_part != nullptr, a.attn_n_head, nmat, best, nw, nbq > 1 ? nbq : p.loop ? 1u : p.d, nbq);
    if (nbq > 1) p.nv = 1;                                              // (nothing staged in registers)
    return p.lds <= GEMV_Q4K_LDS_MAX;
}

namespace {

// the device block of a chunk launch (kernel: block -> (row, block of the row) by multiplication, workgroup -> tensor); no arg-max partials
GemvDev chunk_dev(const GemvArgs &a, uint32_t rw, uint32_t nthr, uint32_t rounds, const uint32_t wg[3]) {
    GemvDev d = to_dev(a);
    const uint32_t bpl = a.n >> 8, nseg = a.epi == GEMV_EPI_SWIGLU ? 1u : a.nseg;
    d.rw = rw; d.nthr = nthr; d.units = rounds;
    d.magic_nchunk = (uint32_t)(((1ull << 32) + bpl - 1) / bpl);
    d.wg_c0 = nseg > 1 ? wg[0] : 0xffffffffu;
    d.wg_c1 = nseg > 2 ? wg[0] + wg[1] : 0xffffffffu;
    d.tile_max = nullptr; d.ntiles = 0;
    return d;
}

// NB = 1: the role kernels; NB = 2 | 4 | 8: generic role, activations from q4k_quant_rows_kernel
template <int ROLE, int NV, int D, bool LOOP, int NB>
hipError_t launch_chunk_t(const GemvDev &d, const Q4kGemvPlan &p, hipStream_t st) {
    auto kern = &gemv_q4k_chunk_kernel<ROLE, NV, D, LOOP, NB>;
    if (p.lds_bytes > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    // measurement (bench.py's `best_kernel`): the classifier launch between the kernel's own start / stop timestamps, as the Q80 STREAM
    // launch is timed (gemv_q80_impl.h); the backend arms the pair for the looping launch of one decode step (one sequence) only
    hipEvent_t e0 = (LOOP && NB == 1) ? g_q80_probe_start : nullptr, e1 = (LOOP && NB == 1) ? g_q80_probe_stop : nullptr;
    if (e0 && e1) {
        g_q80_probe_start = g_q80_probe_stop = nullptr;
        hipExtLaunchKernelGGL(kern, dim3(p.grid), dim3(p.nthr), p.lds_bytes, st, e0, e1, 0, d);
    } else hipLaunchKernelGGL(kern, dim3(p.grid), dim3(p.nthr), p.lds_bytes, st, d);
    return hipGetLastError();
}
template <int ROLE, int NV, int NB>
hipError_t launch_chunk_d(const GemvDev &d, const Q4kGemvPlan &p, hipStream_t st) {
    if (p.loop) return launch_chunk_t<ROLE, NV, 8, true, NB>(d, p, st);
    if (p.d == 1) return launch_chunk_t<ROLE, NV, 1, false, NB>(d, p, st);
    if (p.d == 2) return launch_chunk_t<ROLE, NV, 2, false, NB>(d, p, st);
    if (p.d == 4) return launch_chunk_t<ROLE, NV, 4, false, NB>(d, p, st);
    return launch_chunk_t<ROLE, NV, 8, false, NB>(d, p, st);
}
template <int ROLE>
hipError_t launch_chunk_r(const GemvDev &d, const Q4kGemvPlan &p, hipStream_t st) {
    if (p.nv <= 1) return launch_chunk_d<ROLE, 1, 1>(d, p, st);
    if (p.nv <= 2) return launch_chunk_d<ROLE, 2, 1>(d, p, st);
    return launch_chunk_d<ROLE, 4, 1>(d, p, st);
}
template <int ROLE, int NV>
hipError_t launch_quant_rows_t(const GemvDev &d, XGroup *out, uint32_t nb, size_t lds, hipStream_t st) {
    auto kern = &q4k_quant_rows_kernel<ROLE, NV>;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(nb), dim3(d.nthr), lds, st, d, out);
    return hipGetLastError();
}
// (only the prologue's flags matter to the quantizer: the role kernels' registers do not spill at four float4 per thread, the generic one's do)
template <int NV>
hipError_t launch_quant_rows_r(const GemvDev &d, XGroup *out, uint32_t nb, size_t lds, hipStream_t st) {
    if (d.flags == F_NORM) return launch_quant_rows_t<R_NORM_STORE, NV>(d, out, nb, lds, st);
    if (d.flags == 0) return launch_quant_rows_t<R_RESID, NV>(d, out, nb, lds, st);
    if (d.flags == F_COMBINE) return launch_quant_rows_t<R_RESID_COMBINE, NV>(d, out, nb, lds, st);
    return launch_quant_rows_t<R_GENERIC, NV>(d, out, nb, lds, st);
}
// the quantizer launch with the threads and NV of the one-sequence chunk plan of the same matrix; refuses a missing or short scratch
hipError_t launch_quant_rows_planned(const GemvArgs &a, uint32_t nthr, uint32_t nv, hipStream_t st) {
    if (!a.q4_scratch || (size_t)a.nb * (a.n >> 5) * sizeof(XGroup) > a.q4_scratch_bytes) return hipErrorInvalidValue;
    const uint32_t bpl = a.n >> 8, GT = bpl * 8u;
    GemvDev q = to_dev(a);                                           // flags: norm / combine as the launch asks
    q.nthr = nthr; q.tile_max = nullptr;
    const size_t lds = (size_t)GT * sizeof(XGroup) + (16 + (a.attn_part ? (size_t)a.attn_n_head * 8 : 0)) * 4 + 16;
    XGroup *xg = reinterpret_cast<XGroup *>(a.q4_scratch);
    return nv <= 1 ? launch_quant_rows_r<1>(q, xg, a.nb, lds, st) : nv <= 2 ? launch_quant_rows_r<2>(q, xg, a.nb, lds, st) : launch_quant_rows_r<4>(q, xg, a.nb, lds, st);
}
// the one-sequence chunk plan behind a quantizer launch of 1 .. 64 sequences, where there is one
bool quant_rows_plan(const GemvArgs &a, ChunkPlan &p1) {
    GemvArgs one = a; one.nb = 1; one.tile_max = nullptr;
    return a.nb >= 1 && a.nb <= NANO_MAX_BATCH && !a.x4_in && !a.xq_in && plan_chunk(one, p1);
}

}  // namespace

// The quantizer launch of a several-sequence projection (2 .. 8 sequences: the chunk kernel below; 9 .. 64: gemm_q4k.hip): one workgroup
// per sequence running the prologue of the one-sequence chunk launch of the same matrix, the staged groups of sequence b left at
// a.q4_scratch + b * n bytes.  _supports: that one-sequence launch is a chunk launch (its plan gives the quantizer its thread count).
bool q4k_quant_rows_supports(const GemvArgs &a) { ChunkPlan p1; return quant_rows_plan(a, p1); }
hipError_t launch_q4k_quant_rows(const GemvArgs &a, hipStream_t st) {
    ChunkPlan p1;
    if (!quant_rows_plan(a, p1)) return hipErrorInvalidValue;
    return launch_quant_rows_planned(a, p1.nthr, p1.nv, st);
}

// one sequence; 2 .. 8 sequences: the quantizer launch, then the projection on the staged groups
hipError_t launch_q4k_chunk(const GemvArgs &a, const Q4kGemvPlan &p, hipStream_t st) {
    GemvArgs g = a;
    if (p.quant_rows) {
        const hipError_t e = launch_quant_rows_planned(a, p.quant_nthr, p.quant_nv, st);
        if (e != hipSuccess) return e;
        g.norm_w = nullptr; g.attn_part = nullptr; g.attn_ml = nullptr;
    }
    GemvDev d = chunk_dev(g, p.rw, p.nthr, p.rounds, p.wg);
    if (p.quant_rows) { d.flags = F_PRE; d.xq_in = reinterpret_cast<const int8_t *>(a.q4_scratch); }
    else if (a.x4_in) { d.flags |= F_PRE; d.xq_in = reinterpret_cast<const int8_t *>(a.x4_in); }
    if (p.partials) { d.tile_max = a.tile_max; d.ntiles = p.partials; }
    if (p.B == 2) return launch_chunk_d<R_GENERIC, 1, 2>(d, p, st);
    if (p.B == 4) return launch_chunk_d<R_GENERIC, 1, 4>(d, p, st);
    if (p.B == 8) return launch_chunk_d<R_GENERIC, 1, 8>(d, p, st);
    if (p.role == R_NORM_STORE) return launch_chunk_r<R_NORM_STORE>(d, p, st);
    if (p.role == R_RESID) return launch_chunk_r<R_RESID>(d, p, st);
    if (p.role == R_RESID_COMBINE) return launch_chunk_r<R_RESID_COMBINE>(d, p, st);
    if (p.role == R_NORM_SWIGLU) return launch_chunk_r<R_NORM_SWIGLU>(d, p, st);
    return launch_chunk_r<R_GENERIC>(d, p, st);
}

// ---- the fused q | k | v + attention launch: host side -----------------------------------------------------------------------------------
static bool q4k_fused_shape(const GemvArgs &ga, const AttnArgs &aa, QkvAttnFusedPlan &f) {
    ChunkPlan p;
    if (ga.nb != 1 || ga.nseg != 3 || ga.epi != GEMV_EPI_STORE || !ga.norm_w || ga.xq_in || ga.x4_in || ga.attn_part || ga.tile_max || ga.resid_add) return false;
    if (ga.seg[0].out_pstride || ga.seg[1].out_pstride) return false;            // (only v is position indexed: its cache row)
    // 256 threads, like the attention workgroups: the kernel needs ~200 registers (the attention body), i.e. two waves per SIMD, and a CU must
    // seat a projection workgroup AND an attention workgroup (the first build ran the projection's own 384 threads: one workgroup per CU,
    // the attention started when the projection had left -- 0.575 -> 0.626 ms per step).  Same bits as the 384-thread launch: one float4 item
    // per thread on threads 0 .. n / 4 - 1 either way, a Q4K block is one wave's, the waves beyond add +0.0 to the norm's sum.
    // n <= 1024: one float4 item per thread (NV 1); D: the chunk plan's wave-load slots, the built 1, 2, 4, 8
    if (ga.n > 1024u || !plan_chunk(ga, p, 4u) || p.loop || p.nthr != 256u || p.nv != 1u) return false;
    if (!(p.d == 1u || p.d == 2u || p.d == 4u || p.d == 8u)) return false;
    if (p.lds > FUSED_LDS_MAX) return false;
    if (!fused_attn_side_ok(aa, ga.seg[0].rows, ga.seg[1].rows, ga.seg[2].rows, false)) return false;
    f = QkvAttnFusedPlan{};
    f.kernel = FUSED_KERNEL_Q4K; f.nv = 1u; f.d = p.d;
    f.threads = p.nthr; f.rw = p.rw; f.rounds = p.rounds;
    for (uint32_t s2 = 0; s2 < 3; s2++) f.wg[s2] = p.wg[s2];
    f.ngemv = p.grid; f.n_attn = fused_attn_wgs(aa);
    const size_t lds_a = fused_attn_lds(aa.hd, false);
    f.lds_bytes = (uint32_t)(p.lds > lds_a ? p.lds : lds_a);
    return f.lds_bytes <= FUSED_LDS_MAX;
}
bool qkv_attn_fused_q4k_plan(const GemvArgs &ga, const AttnArgs &aa, QkvAttnFusedPlan *out) {
    QkvAttnFusedPlan f;
    if (!q4k_fused_shape(ga, aa, f)) return false;
    if (out) *out = f;
    return true;
}

hipError_t launch_qkv_attn_fused_q4k(const GemvArgs &ga, const AttnArgs &aa, unsigned long long *hand, uint32_t *tick, uint32_t layer1, hipStream_t st) {
    QkvAttnFusedPlan p;
    if (!hand || !tick || !layer1 || layer1 > 127u || !q4k_fused_shape(ga, aa, p)) return hipErrorInvalidValue;
    const GemvDev d = chunk_dev(ga, p.rw, p.threads, p.rounds, p.wg);
    QkvAttnArgs fa{};
    fused_attn_setup(fa, aa, hand, tick, layer1);
    const size_t lds = p.lds_bytes;
    fa.g = d; fa.ngemv = p.ngemv;
    // naps of 16 x 64 cycles between the K / V requests and the first poll.  Same box, driver's flags (profiles/r06_q4k_fused.txt): the five
    // launches per layer 1733 / 1755 tok/s; fused with 2 naps 1773 / 1818, 4: 1782 / 1779, 6: 1742 / 1739, 8: 1684 / 1688
    // (re-swept at the end of round 6, producers first in the grid: 0 / 1 / 2 / 3 naps 1789 / 1761 / 1782 / 1780 and 1784 / 1778 / 1779 / 1775 tok/s: flat; none)
    fa.wait16 = 0u;
    // the instantiations: <D> of 1, 2, 4, 8 (tests/test_fused_launch_plan.py restates the set)
#define Q4F_GO(D_) do { if (p.d == D_) { hipLaunchKernelGGL((q4k_qkv_attn_fused_kernel<D_>), dim3(p.n_attn + p.ngemv), dim3(p.threads), lds, st, fa); return hipGetLastError(); } } while (0)
    Q4F_GO(1); Q4F_GO(2); Q4F_GO(4); Q4F_GO(8);
#undef Q4F_GO
    return hipErrorInvalidValue;
}

}  // namespace nano
