// gemv_q80_host.h -- host-side routing shared by the Q80 GEMV translation units.
#pragma once
#include "kernels.h"
#include "gemv_common.h"
#include <hip/hip_ext.h>
#include <stdlib.h>

namespace nano {

constexpr uint32_t STREAM_MIN_ROWS = 16384;     // taller matrices go to the stream kernel
// workgroups of a STREAM launch: 1024 = two resident rounds of 512 (2 per CU at the kernel's register footprint)
static inline uint32_t stream_wgs() { return 1024u; }
#define STREAM_WGS (::nano::stream_wgs())

static inline bool use_stream(const GemvArgs &a) {
    return a.nseg == 1 && a.epi == GEMV_EPI_STORE && a.seg[0].rows >= STREAM_MIN_ROWS && a.seg[0].out_pstride == 0 && !a.attn_part && a.nb <= 8;
}

// rows per workgroup / waves per workgroup / work units per wave / float4 items per thread of a slab launch at capacity B: the ONE
// planner (gemv_q80.hip) behind gemv_q80_plan() and the fused one-sequence launches (fused_shape, wo13_shape: gemv_q80_impl.h)
struct SlabPlan { uint32_t rw, nw, upw, nv; };
SlabPlan q80_plan_slab(const GemvArgs &a, int B);

// a launch whose rows are one 1 KiB chunk of group size 64: the in-wave fold (SLAB_WF) takes it (the callers add: one sequence, an rmsnorm role,
// a canonical launch).  W1|W3 is never position indexed in a decode step; such a launch would keep the table.
static inline bool slab_wave_fold(const GemvDev &d) {
    return d.n == 1024u && d.ng == 16u && !d.early && (d.epi == GEMV_EPI_STORE || (d.epi == GEMV_EPI_SWIGLU && !d.out_pstride[0]));
}
// a residual launch (Wo, W2) whose rows are 2..4 WHOLE chunks of group size 64: the chunk count when the in-wave fold of a unit's chunk
// (SLAB_WFC) takes it, else 0 (the callers add: one sequence, a residual role, a canonical launch).  A LoRA addend or a position-indexed output
// keeps the table.
static inline uint32_t slab_wave_fold_chunks(const GemvDev &d) {
    if (d.nb != 1u || d.early || d.epi != GEMV_EPI_RESID || d.resid_add || d.out_pstride[0] || d.rows[1] || (d.flags & ~F_COMBINE)) return 0u;
    if (d.n % 1024u || d.n < 2048u || d.n > 4096u || d.ng * 64u != d.n) return 0u;
    return d.n / 1024u;
}
// The split-attention combine with in-wave weights and the live splits only (gemv_common.h cw_issue / cw_combine; gemv_q80_slab_body.inc
// SLAB_CW): a one-sequence launch whose input is the splits' partials, at most 8 splits, heads of 32 | 64 | 128 | 256 values that tile
// the row -- the 256 values of a wave's item round are whole heads, 8 | 4 | 2 | 1 of them.  (The callers add: the combine role, group size
// 64, the items in registers.)  GemvArgs::attn_table refuses the form -- the table form runs: a model's NANO_COMBINE_WAVE=0, read once
// when the model is created, and the operators' and queries' reading of the same variable (A/B measurements, the tests that compare the
// two forms bit for bit).  Nothing is read from the environment here.
static inline bool combine_wave_shape(const GemvArgs &a) {
    if (!a.attn_part || a.attn_table || a.nb != 1u || a.attn_nsplit == 0u || a.attn_nsplit > 8u) return false;
    const uint32_t hd = a.attn_hd;
    return (hd == 32u || hd == 64u || hd == 128u || hd == 256u) && (uint64_t)a.attn_n_head * hd == a.n;
}
static inline size_t slab_unit_table(const GemvDev &d, uint32_t nch) { return (size_t)(d.tpw * 4) * (nch <= 2u ? 4u : 8u) * 4u; }      // [rows of the tiles][unit sums] floats

// measurement hook: when both are set, the next STREAM (classifier) launch is issued with hipExtLaunchKernelGGL so that the
// two events carry the kernel's own start / stop timestamps (what rocprofv3 reports), then the hook clears itself
extern hipEvent_t g_q80_probe_start, g_q80_probe_stop;

}  // namespace nano
