// gemv_f32.hip -- FP32 decode GEMV for gfx950 (reference matmul, infer/infer.c:637-651), same latency-oriented SLAB
// structure as the Q80 kernels (gemv_q80_impl.h): a workgroup owns `rw` consecutive rows, its work units (4 rows x one
// 256-float column chunk, x2 matrices for SwiGLU) are dealt to its waves, every wave issues the activation loads and
// then ALL its weight loads at kernel entry through buffer descriptors (one memory round trip), rmsnorm / the
// split-attention combine run from registers while the weights are in flight.
// The reference adds the n products of a row sequentially; here a lane accumulates its float4 slices with fused
// multiply-adds, a DPP tree sums the 64 lanes and one thread adds the chunk partials in order -- the summation ORDER
// differs, so results match the reference to rounding (stated tolerance 1e-5 relative, DESIGN.md "Parity").
// HBM-bound byte work (2 flop / 4 bytes): no MFMA.
#include "gemv_f32_stage.h"

namespace nano {

namespace {

template <int ROLE, int B, int NV, int UPW>
__global__ __launch_bounds__(1024) void gemv_f32_slab_kernel(const GemvDev a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#define F32_A a
#define F32_BID blockIdx.x
#define F32_HAND 0
#define F32_HANDV (SlabHand{})
#define F32_PTAG 0u
#include "gemv_f32_slab_body.inc"
#undef F32_A
#undef F32_BID
#undef F32_HAND
#undef F32_HANDV
#undef F32_PTAG
}

}  // namespace
}  // namespace nano
#include "attn_impl.h"
namespace nano {
namespace {
// ---- q | k | v projection + attention in ONE launch for FP32 models (Nano: head_dim <= 64, no q / k norm, adjacent-pair RoPE; round 6: what
//      qkv_attn_fused_kernel is for Q80 and q4k_qkv_attn_fused_kernel for Q4K) ---------------------------------------------------------------
// The first `ngemv` workgroups run the projection's SLAB body (results stored as usual AND as granules), the last n_attn the attention's
// plain decode mode (attention_body MODE 2), 256 threads for both.  Epoch tags, give-up and re-issue: device_common.h, backend.hip.
// Reference: infer/infer.c:637-651, 758-879.
template <int QV>            // QV: float4 slots per lane of the attention's 8-lane sub-groups (1: head_dim <= 32, 2: <= 64 -- launch_attention's choice)
__global__ __launch_bounds__(256) void f32_qkv_attn_fused_kernel(const QkvAttnArgs fa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint2 tk_ = hand_tick(fa.hand);
    if (blockIdx.x >= fa.ngemv) {
        const uint32_t ab = blockIdx.x - fa.ngemv;
        const uint32_t split = ab / fa.head_wgs, grp = ab - split * fa.head_wgs;
        attention_body<8, QV, 1, 2, false, false, 2, false, true>(fa.a, smem, grp, 0u, split, fa.hand, hand_ctag(tk_, fa.hand), fa.wait16);
        return;
    }
    constexpr int ROLE = R_NORM_STORE, B = 1, NV = 1, UPW = 1;           // one float4 item per thread, one unit per wave (f32_fused_shape)
#define F32_A fa.g
#define F32_BID blockIdx.x
#define F32_HAND 1
#define F32_HANDV fa.hand
#define F32_PTAG hand_ptag(tk_, fa.hand)
#include "gemv_f32_slab_body.inc"
#undef F32_A
#undef F32_BID
#undef F32_HAND
#undef F32_HANDV
#undef F32_PTAG
}

struct F32Plan { uint32_t rw, nw, upw, nv; };
static F32Plan plan_f32(const GemvArgs &a, int B) {
    const uint32_t nchunk = (a.n + 255) / 256, nmat = a.epi == GEMV_EPI_SWIGLU ? 2 : 1;
    const uint32_t nseg = a.epi == GEMV_EPI_SWIGLU ? 1u : a.nseg;
    uint32_t align = 0;
    if (nseg > 1) for (uint32_t s = 0; s < nseg; s++) align |= a.seg[s].rows;
    uint32_t rows = 0;
    if (a.epi == GEMV_EPI_SWIGLU) rows = a.seg[0].rows; else for (uint32_t s = 0; s < a.nseg; s++) rows += a.seg[s].rows;
    uint32_t rw = 4;                 // 4 KiB of weights per unit: a few units per workgroup, >= 256 workgroups
    while (rw < 32 && (align % (rw * 2)) == 0 && (rw * 2 / 4) * nchunk <= 8 && rows / (rw * 2) >= 256) rw *= 2;
    const uint32_t units = (rw / 4) * nchunk * nmat;
    uint32_t nw = units < 8 ? units : 8;
    uint32_t want = (a.n * (uint32_t)(B > 2 ? B / 2 : 1) + 1023) / 1024;
    if (want > 16) want = 16;
    if (nw < want) nw = want;
    if (nw * 64 < rw * (uint32_t)B) nw = (rw * (uint32_t)B + 63) / 64;
    if (nw < 2) nw = 2;
    uint32_t upw = (units + nw - 1) / nw;
    while (upw > 4 && nw < 16) { nw++; upw = (units + nw - 1) / nw; }
    return F32Plan{rw, nw, upw, (a.n + 256 * nw - 1) / (256 * nw)};
}

template <int ROLE, int B, int NV, int UPW>
static hipError_t launch_f32_t(const GemvDev &d, const F32GemvPlan &p, hipStream_t st) {
    auto kern = &gemv_f32_slab_kernel<ROLE, B, NV, UPW>;
    if (p.lds_bytes > 64 * 1024) {          // opt-in LDS; gemv_f32_plan() has refused what a CU does not have
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
        if (e != hipSuccess) return e;
    }
    GemvDev dd = d; dd.nthr = 64 * p.nw;
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(64 * p.nw), p.lds_bytes, st, dd);
    return hipGetLastError();
}
// the instantiations: every (NV, UPW) of {0, 1, 2, 4} x {1, 2, 4} with B * NV <= 8 (tests/test_f32_gemv_plan.py restates the set)
template <int ROLE, int B>
static hipError_t launch_f32_r(const GemvDev &d, const F32GemvPlan &p, hipStream_t st) {
#define F32_GO(NV_, UPW_) do { if constexpr (B * NV_ <= 8) { if (p.nv == NV_ && p.upw == UPW_) return launch_f32_t<ROLE, B, NV_, UPW_>(d, p, st); } } while (0)
    F32_GO(1, 1); F32_GO(1, 2); F32_GO(1, 4);
    F32_GO(2, 1); F32_GO(2, 2); F32_GO(2, 4);
    F32_GO(4, 1); F32_GO(4, 2); F32_GO(4, 4);
    F32_GO(0, 1); F32_GO(0, 2); F32_GO(0, 4);
    return hipErrorInvalidValue;
#undef F32_GO
}
template <int B>
static hipError_t launch_f32_b(const GemvArgs &a, const F32GemvPlan &p, hipStream_t st) {
    GemvDev d = to_dev(a);
    d.tile_max = nullptr;
    d.nchunk = (a.n + 255) / 256;
    d.magic_nchunk = (65536 + d.nchunk - 1) / d.nchunk;
    d.rw = p.rw;
    uint32_t l2 = 0; while ((1u << l2) < p.rw / 4) l2++;
    d.log2_tiles = l2;
    d.units = (p.rw / 4) * d.nchunk * (d.epi == GEMV_EPI_SWIGLU ? 2 : 1);
    if constexpr (B == 1) {                 // the role-specialised kernels exist for one sequence only
        if (p.role == R_NORM_STORE) return launch_f32_r<R_NORM_STORE, B>(d, p, st);
        if (p.role == R_RESID) return launch_f32_r<R_RESID, B>(d, p, st);
        if (p.role == R_RESID_COMBINE) return launch_f32_r<R_RESID_COMBINE, B>(d, p, st);
        if (p.role == R_NORM_SWIGLU) return launch_f32_r<R_NORM_SWIGLU, B>(d, p, st);
    }
    if (p.role != R_GENERIC) return hipErrorInvalidValue;
    return launch_f32_r<R_GENERIC, B>(d, p, st);
}

// the fused launch's plan: the projection's own, on 256 threads (four waves like the attention's workgroups; same bits -- the float4 items sit
// on the same threads, the fourth wave adds +0.0 to the norm's sum)
static bool f32_fused_shape(const GemvArgs &ga, const AttnArgs &aa, QkvAttnFusedPlan &f) {
    if (ga.nb != 1 || ga.nseg != 3 || ga.epi != GEMV_EPI_STORE || !ga.norm_w || ga.xq_in || ga.attn_part || ga.tile_max || ga.resid_add || ga.n % 4u) return false;
    if (ga.seg[0].out_pstride || ga.seg[1].out_pstride) return false;            // (only v is position indexed: its cache row)
    for (uint32_t s2 = 0; s2 < 3; s2++) if (ga.seg[s2].rows % 4u) return false;
    const F32Plan p = plan_f32(ga, 1);
    if (p.nw > 4u || ga.n > 1024u) return false;                                 // one float4 item per thread on <= 256 threads
    const uint32_t nchunk = (ga.n + 255) / 256, units = (p.rw / 4) * nchunk;
    if (units > 4u) return false;                // one unit per wave (more than 4 make plan_f32() ask for more than 4 waves: a wave never holds a second unit)
    if (!fused_attn_side_ok(aa, ga.seg[0].rows, ga.seg[1].rows, ga.seg[2].rows, true)) return false;
    f = QkvAttnFusedPlan{};
    f.kernel = FUSED_KERNEL_F32; f.nv = 1u; f.upw = 1u; f.qv = aa.hd <= 32u ? 1u : 2u;
    f.threads = 256; f.rw = p.rw;
    uint32_t rows = 0;
    for (uint32_t s2 = 0; s2 < 3; s2++) rows += ga.seg[s2].rows;
    f.ngemv = f.wg[0] = (rows + p.rw - 1) / p.rw;                                 // (a workgroup's rows may cross tensors: multiples of 4 each)
    f.n_attn = fused_attn_wgs(aa);
    const size_t n4 = (ga.n + 3) & ~3u, pc = (nchunk + 3) & ~3u;
    const size_t lds_g = (n4 + 16 + (size_t)p.rw * pc) * 4, lds_a = fused_attn_lds(aa.hd, true), lds = lds_g > lds_a ? lds_g : lds_a;
    if (lds > FUSED_LDS_MAX) return false;
    f.lds_bytes = (uint32_t)lds;
    return true;
}

}  // namespace

bool qkv_attn_fused_f32_plan(const GemvArgs &ga, const AttnArgs &aa, QkvAttnFusedPlan *out) {
    QkvAttnFusedPlan f;
    if (!f32_fused_shape(ga, aa, f)) return false;
    if (out) *out = f;
    return true;
}

hipError_t launch_qkv_attn_fused_f32(const GemvArgs &ga, const AttnArgs &aa, unsigned long long *hand, uint32_t *tick, uint32_t layer1, hipStream_t st) {
    QkvAttnFusedPlan p;
    if (!hand || !tick || !layer1 || layer1 > 127u || !f32_fused_shape(ga, aa, p)) return hipErrorInvalidValue;
    GemvDev d = to_dev(ga);
    d.tile_max = nullptr;
    d.nchunk = (ga.n + 255) / 256;
    d.magic_nchunk = (65536 + d.nchunk - 1) / d.nchunk;
    d.rw = p.rw;
    uint32_t l2 = 0; while ((1u << l2) < p.rw / 4) l2++;
    d.log2_tiles = l2;
    d.units = (p.rw / 4) * d.nchunk;
    d.nthr = p.threads;
    QkvAttnArgs fa{};
    fused_attn_setup(fa, aa, hand, tick, layer1);
    const uint32_t grid = p.n_attn + p.ngemv;
    const size_t lds = p.lds_bytes;
    fa.g = d; fa.ngemv = p.ngemv;
    fa.wait16 = 1u;             // naps of 16 x 64 cycles before the attention's first poll: Nano-168M, one box, 0 / 1 / 2 / 3 naps: 2387 / 2384 / 2380 / 2364 and 2383 / 2381 / 2380 / 2366 tok/s
    // the instantiations: <QV> of 1, 2 (tests/test_fused_launch_plan.py restates the set)
#define F32F_GO(QV_) do { if (p.qv == QV_) { hipLaunchKernelGGL((f32_qkv_attn_fused_kernel<QV_>), dim3(grid), dim3(p.threads), lds, st, fa); return hipGetLastError(); } } while (0)
    F32F_GO(1); F32F_GO(2);
#undef F32F_GO
    return hipErrorInvalidValue;
}

// The launch of `a`: which gemv_f32_slab_kernel<ROLE, B, NV, UPW>, on how many waves and workgroups, with how much LDS.  Every choice
// launch_gemv_f32() makes is made here.  false: the arguments are refused (malformed, more than 4 units per wave -- rows beyond 16384
// floats, 8192 with SwiGLU -- or more LDS than a CU has: gemv_f32_fit_batch() tells the router how many sequences fit).
bool gemv_f32_plan(const GemvArgs &a, F32GemvPlan *out) {
    if (a.nb == 0 || a.nb > 8 || a.n == 0 || a.n % 4 || a.nseg == 0 || a.nseg > 3 || a.xq_in) return false;
    if (a.attn_part && (a.norm_w || a.attn_nsplit > 8 || a.attn_hd == 0 || a.attn_hd % 4)) return false;
    if (a.epi == GEMV_EPI_SWIGLU && a.nseg != 2) return false;
    if (a.epi != GEMV_EPI_SWIGLU && a.nseg > 1)
        for (uint32_t s = 0; s < a.nseg; s++) if (a.seg[s].rows % 4) return false;
    const uint32_t B = a.nb <= 1 ? 1 : a.nb <= 2 ? 2 : a.nb <= 4 ? 4 : 8;
    const F32Plan p = plan_f32(a, (int)B);
    if (p.upw > 4) return false;
    const uint32_t f = (a.norm_w ? F_NORM : 0u) | (a.attn_part ? F_COMBINE : 0u);
    uint32_t role = R_GENERIC;
    if (B == 1) {
        if (f == F_NORM && a.epi == GEMV_EPI_STORE) role = R_NORM_STORE;
        else if (f == 0 && a.epi == GEMV_EPI_RESID) role = R_RESID;
        else if (f == F_COMBINE && a.epi == GEMV_EPI_RESID) role = R_RESID_COMBINE;
        else if (f == F_NORM && a.epi == GEMV_EPI_SWIGLU) role = R_NORM_SWIGLU;
    }
    uint32_t nv = p.nv <= 1 ? 1 : p.nv <= 2 ? 2 : p.nv <= 4 ? 4 : 0;     // float4 items a thread stages in registers; 0: the loop form
    if (B * nv > 8) nv = 0;
    const uint32_t upw = p.upw <= 1 ? 1 : p.upw <= 2 ? 2 : 4;
    uint32_t rows = 0;
    if (a.epi == GEMV_EPI_SWIGLU) rows = a.seg[0].rows; else for (uint32_t s = 0; s < a.nseg; s++) rows += a.seg[s].rows;
    if (rows == 0) return false;
    const uint32_t nmat = a.epi == GEMV_EPI_SWIGLU ? 2 : 1, nchunk = (a.n + 255) / 256;
    const uint64_t n4 = (a.n + 3) & ~3u, pc = (nchunk + 3) & ~3u;
    // activations [B][n4] | norm partials [B][16] | combine weights [B][n_head][8] | chunk partials [B][nmat][rw][pc]
    const uint64_t lds = ((uint64_t)B * n4 + (uint64_t)B * 16 + ((f & F_COMBINE) ? (uint64_t)B * a.attn_n_head * 8 : 0) + (uint64_t)B * nmat * p.rw * pc) * 4;
    if (lds > GEMV_F32_LDS_MAX) return false;
    if (out) *out = F32GemvPlan{role, B, nv, upw, p.rw, p.nw, (rows + p.rw - 1) / p.rw, (uint32_t)lds};
    return true;
}

// sequences per launch whose LDS request a CU can meet (8 | 4 | 2 | 1; 0: not even one sequence, or a refused shape).  LDS grows
// with the capacity and nothing else of a refusal depends on it, so every smaller batch fits as well.
uint32_t gemv_f32_fit_batch(const GemvArgs &a) {
    GemvArgs t = a;
    for (uint32_t c = 8; c >= 1; c >>= 1) { t.nb = c; if (gemv_f32_plan(t, nullptr)) return c; }
    return 0;
}

hipError_t launch_gemv_f32(const GemvArgs &a, hipStream_t st) {
    F32GemvPlan p;
    if (!gemv_f32_plan(a, &p)) return hipErrorInvalidValue;
    if (p.B == 1) return launch_f32_b<1>(a, p, st);
    if (p.B == 2) return launch_f32_b<2>(a, p, st);
    if (p.B == 4) return launch_f32_b<4>(a, p, st);
    return launch_f32_b<8>(a, p, st);
}

}  // namespace nano
