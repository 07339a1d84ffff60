// gemm_f32_host.h -- the host side of the FP32 MFMA GEMM (gemm_f32.hip): the constants its kernel and its planner share, and the planner.
// The plan names the whole launch -- template value, threads, workgroups, LDS bytes and layout, token tiles, units per wave, the
// prologue launch in front -- and the launcher only consumes it (kernels.h F32GemmPlan; nano_hip_f32_gemm_plan reports it).
#pragma once
#include "kernels.h"

namespace nano {

constexpr uint32_t GF_RT = 16;                      // rows of a tile = the M of v_mfma_f32_16x16x4_f32
constexpr uint32_t GF_UNIT = 128;                   // floats of a unit: half a 256-float chunk = 32 float4 items = one level below the chunk sum
constexpr uint32_t GF_ITEMS = GF_UNIT / 4;          // float4 items of a unit
constexpr uint32_t GF_SPITCH = GF_ITEMS + 4;        // floats between the 64 operand lanes' lines of a wave's transposition buffer (16-byte reads of 16 lanes: 64 banks)
constexpr uint32_t GF_STAGE_B = 64 * GF_SPITCH * 4; // bytes of that buffer
constexpr uint32_t GF_MAX_NW = 8;                   // waves of a workgroup (two per SIMD)

// Table of unit sums: [matrix][unit][row][tp], tp = 16 * token tiles + 4 (the four row quads of an MFMA result on different banks).
static inline uint32_t gf_table_bytes(uint32_t nmat, uint32_t nu, uint32_t nt) { return nmat * nu * GF_RT * (nt * 16u + 4u) * 4u; }

static inline bool gemm_f32_plan_host(const GemvArgs &a, F32GemmPlan *out) {
    if (a.nb < 9 || a.nb > 64 || a.n == 0 || a.n % 4 || a.nseg == 0 || a.nseg > 3) return false;
    if (a.resid_add || a.attn_part || a.tile_max || a.xq_in) return false;
    if (a.epi > GEMV_EPI_SWIGLU) return false;
    if (a.epi == GEMV_EPI_SWIGLU && (a.nseg != 2 || a.seg[0].rows != a.seg[1].rows || a.seg[0].out_pstride)) return false;
    if (a.epi == GEMV_EPI_RESID && a.seg[0].out_pstride) return false;            // (the residual stream is never position indexed)
    for (uint32_t s = 0; s < a.nseg; s++) {
        if (a.seg[s].rows == 0 || a.seg[s].rows % GF_RT) return false;
        if ((uint64_t)a.seg[s].rows * a.n * 4u >= (1ull << 32)) return false;      // (32-bit byte offsets, as in the GEMV)
    }
    // the sliced route's launch of this shape: what it refuses stays refused (rows beyond 16384 floats, 8192 with SwiGLU), and its
    // thread count is the prologue's -- the rmsnorm tree of the route this one replaces
    GemvArgs t = a;
    uint32_t per = 0, launches = 0;
    if (!route_gemv_slices(NANO_QUANT_F32, t, &per, &launches)) return false;
    t.nb = per;
    F32GemvPlan gp;
    if (!gemv_f32_plan(t, &gp)) return false;
    const uint32_t nmat = a.epi == GEMV_EPI_SWIGLU ? 2u : 1u;
    const uint32_t nt = (a.nb + 15u) / 16u, nu = (a.n + GF_UNIT - 1u) / GF_UNIT;
    const uint32_t tab = gf_table_bytes(nmat, nu, nt);
    uint32_t nw = nu < GF_MAX_NW ? nu : GF_MAX_NW;                                  // the waves split the units; fewer where the table leaves less room
    while (nw > 1u && (uint64_t)nw * GF_STAGE_B + tab > GEMM_F32_LDS_MAX) nw--;
    const uint64_t lds = (uint64_t)nw * GF_STAGE_B + tab;
    if (lds > GEMM_F32_LDS_MAX) return false;
    const uint64_t pro_lds = (uint64_t)((a.n + 3u) & ~3u) * 4u + 64u;               // the prologue: one token's activation | norm partials [16]
    if (pro_lds > GEMM_F32_LDS_MAX) return false;
    if (!out) return true;
    F32GemmPlan p{};
    p.sw = nmat - 1u;
    p.nw = nw; p.threads = 64u * nw; p.grid = gemv_total_rows(a) / GF_RT; p.lds_bytes = (uint32_t)lds;
    p.rt = GF_RT; p.nt = nt; p.nu = nu; p.upw = (nu + nw - 1u) / nw; p.tp = nt * 16u + 4u;
    p.stage_bytes = GF_STAGE_B; p.tab_off = nw * GF_STAGE_B;
    p.pro_threads = 64u * gp.nw; p.pro_lds = (uint32_t)pro_lds;
    p.xs_floats = nt * 16u * nu * GF_UNIT;
    *out = p;
    return true;
}

}  // namespace nano
