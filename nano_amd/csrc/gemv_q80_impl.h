// gemv_q80_impl.h -- body of the Q80 GEMV kernels; compiled once per group size (gemv_q80_gs*.hip define
// NANO_Q80_GS and NANO_Q80_ENTRY and include this file) so that the instantiations build in parallel.
// gemv_q80.hip -- Q80 (W8A8) fused decode GEMVs for gfx950 (MI355X), up to 8 sequences per launch.
//
// Restates for the device:
//   * quantize      (reference infer/tensor.c:21-46)   per group: s = max|x|/127, q = (int8)round(x/s)
//   * matmul_quant  (reference infer/infer.c:654-679)  per row, groups in ascending order:
//                                                      val += ((float)sum_i8xi8) * ws[g] * xs[g]
// with rmsnorm (infer.c:601-614), the split-attention combine (attn.hip), the residual adds
// (infer.c:906-908,963-965) and SwiGLU (infer.c:937-944) fused in as prologue / epilogue.
// Given identical int8 inputs the fp32 outputs are BIT-IDENTICAL to the reference: the integer group
// sums are exact, every group product is formed as ((float)ival * ws) * xs and one lane adds the
// groups of a row in ascending order (no tree, no FMA contraction).
//
// A batch-1 decode step is a chain of ~140 dependent kernels whose weights (2..6 MB each, except the
// classifier) stream in well under a microsecond: every per-layer kernel is LATENCY bound, not
// bandwidth bound.  Two kernels, built for the two regimes:
//
//   SLAB   (per-layer matrices).  A workgroup owns `rw` consecutive output rows x the whole row length.
//          Its work units (4 rows x one 1 KiB column chunk, x2 matrices for SwiGLU) are dealt to its
//          waves; every wave issues ALL of its loads right at kernel entry -- first the activation, then
//          weights and weight scales through buffer descriptors (32-bit offsets, hardware bounds check,
//          no exec-masked branches, no dependent scalar loads) -- so the whole kernel costs ONE memory
//          round trip.  rmsnorm + quantization run from registers while the weights are in flight; the
//          group products land in an LDS table and one thread per (row, sequence) folds them in order.
//          (Rows of ONE chunk -- n == 1024, one sequence, the rmsnorm roles: the wave that holds a row's products folds it itself,
//          wave_fold_canon16 below; no table, no barrier behind the dots.)
//          (Rows of 2..4 whole chunks -- n == 2048 / 3072 / 4096, one sequence, the residual roles, Wo and W2: the wave of a unit folds its
//          chunk to two unit sums, wave_fold_canon16_units below; 8 floats per unit in LDS instead of 64 products, and the fold thread of a row
//          adds 2 x chunks unit sums behind the barrier instead of 16 x chunks products.)
//   STREAM (classifier: vocab x n_embd).  1024 persistent workgroups; a wave owns 16-row tiles,
//          tile = wave + k * nwaves, so the chip sweeps memory linearly; four waves per SIMD keep 16 KiB each in
//          flight while one of them is consuming.  Lane l loads bytes [16l,16l+16) of each row chunk
//          (non-temporal, fully coalesced; the row-major int8 blocks stay exactly as in the model file);
//          DPP integer group sums; the leaders park them in a wave-private LDS table; then lane l owns
//          (row l/4, groups 4(l%4)..+3): the scales of a whole tile arrive as ONE coalesced load, all 64
//          lanes form products, and a 4-stage quad chain keeps the reference's group order.
//          Measured 5.6-5.7 TB/s (cold), 95 % of what a plain read of the same bytes achieves.
//
// MFMA is not used: 2 flop/byte at batch <= 8, no tile forms.
#include <string.h>
#include <stdio.h>
#include "gemv_common.h"
#include "gemv_q80_host.h"

namespace nano {

namespace {


__device__ __forceinline__ void quant_store4(float4 v, float scale, int8_t *dst) {
    *reinterpret_cast<uint32_t *>(dst) = q80_pack4(q80_quant4(v, scale));
}

template <int ROLE, int GS, int B, int NV, int CW = 0>
__device__ __forceinline__ void stage_finish(const GemvDev &a, Staged<B, NV> &r, int8_t *xq, float *xs, float *red, uint32_t n16, uint32_t ng4) {
    const uint32_t tid = threadIdx.x, nthr = a.nthr, n = a.n, ng = a.ng;
    const uint32_t lane = tid & 63u, wid = tid >> 6, NW = nthr >> 6;
    if (has_flag<ROLE>(a, F_PRE)) { // the activations arrive quantized: xq_in[nb][n16], xs_in[nb][ng] (operator tests; large
                                    // batch x row-length products, where quant_rows_kernel quantizes ONCE instead of once per workgroup)
        for (uint32_t b = 0; b < a.nb; b++) {
            for (uint32_t i = tid * 16u; i < n; i += nthr * 16u) *reinterpret_cast<int4 *>(xq + b * n16 + i) = *reinterpret_cast<const int4 *>(a.xq_in + (size_t)b * n16 + i);
            for (uint32_t i = tid; i < ng; i += nthr) xs[b * ng4 + i] = a.xs_in[(size_t)b * ng + i];
        }
        __syncthreads();
        return;
    }
    const bool norm = has_flag<ROLE>(a, F_NORM), comb = has_flag<ROLE>(a, F_COMBINE);
    float *wgt = red + B * 16;
    if constexpr (NV == 0) {
        if (comb) combine_weights<B, false>(a, wgt, 0.0f, 0.0f);
        // generic path (large n x B): two passes over memory per sequence
        for (uint32_t b = 0; b < a.nb; b++) {
            const float *x = a.xin + (size_t)b * a.xin_bstride;
            float ss = 1.0f;
            if (norm) {
                float acc = 0.0f;
                for (uint32_t i = tid * 4u; i < n; i += nthr * 4u) {
                    const float4 v = comb ? combine4(a, b, i, wgt) : *reinterpret_cast<const float4 *>(x + i);
                    acc += v.x * v.x; acc += v.y * v.y; acc += v.z * v.z; acc += v.w * v.w;
                }
                acc = dpp_wave_sum(acc);
                __syncthreads();
                if (lane == 0) red[wid] = acc;
                __syncthreads();
                float t = 0.0f;
                for (uint32_t w = 0; w < NW; w++) t += red[w];
                t /= (float)n; t += 1e-5f;
                ss = 1.0f / sqrtf(t);
            }
            for (uint32_t i = tid * 4u; i < n; i += nthr * 4u) {       // n % GS == 0, 4*nthr % GS == 0: groups are whole
                float4 v = comb ? combine4(a, b, i, wgt) : *reinterpret_cast<const float4 *>(x + i);
                if (norm) {
                    const float4 w = *reinterpret_cast<const float4 *>(a.norm_w + i);
                    v.x = w.x * (ss * v.x); v.y = w.y * (ss * v.y); v.z = w.z * (ss * v.z); v.w = w.w * (ss * v.w);
                }
                float m = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
                m = dpp_group_max<GS / 4>(m);
                const float scale = div_const<127>(m);
                quant_store4(v, scale, xq + b * n16 + i);
                if ((tid % (GS / 4)) == 0) xs[b * ng4 + i / GS] = scale;
            }
        }
        __syncthreads();
    } else {
        if constexpr (CW != 0) {        // in-wave weights, live splits only (gemv_common.h cw_combine): no table, no barrier
            cw_combine<NV>(a, r);
        } else
        if (comb) {
            if constexpr (B == 1) {
                const bool pre_ml = a.attn_n_head * 8u <= nthr;       // every (head, split) pair has its own thread
                if (pre_ml) combine_weights<B, true>(a, wgt, r.ml_m, r.ml_l); else combine_weights<B, false>(a, wgt, 0.0f, 0.0f);
#pragma unroll
                for (int j = 0; j < NV; j++) {
                    const uint32_t i = (tid + (uint32_t)j * nthr) * 4u;
                    const float *wg = wgt + (size_t)((i < n ? i : 0u) / a.attn_hd) * 8u;
                    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int sp = 0; sp < 8; sp++) {          // splits >= nsplit: partial read as 0, weight 0
                        const float w = wg[sp];
                        acc.x += r.pv[j][sp].x * w; acc.y += r.pv[j][sp].y * w; acc.z += r.pv[j][sp].z * w; acc.w += r.pv[j][sp].w * w;
                    }
                    r.x[0][j] = acc;
                }
            } else {
                combine_weights<B, false>(a, wgt, 0.0f, 0.0f);
#pragma unroll
                for (int b = 0; b < B; b++)
#pragma unroll
                    for (int j = 0; j < NV; j++) {
                        const uint32_t i = (tid + (uint32_t)j * nthr) * 4u;
                        r.x[b][j] = (i < n && b < (int)a.nb) ? combine4(a, b, i, wgt) : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
            }
        }
        float ss[B];
#pragma unroll
        for (int b = 0; b < B; b++) ss[b] = 1.0f;
        if (norm) {                     // rmsnorm scale (infer.c:603-609); tree order, tolerance 1e-5
#pragma unroll
            for (int b = 0; b < B; b++) {
                float acc = 0.0f;
#pragma unroll
                for (int j = 0; j < NV; j++) {
                    acc += r.x[b][j].x * r.x[b][j].x; acc += r.x[b][j].y * r.x[b][j].y;
                    acc += r.x[b][j].z * r.x[b][j].z; acc += r.x[b][j].w * r.x[b][j].w;
                }
                acc = dpp_wave_sum(acc);
                if (lane == 0) red[b * 16 + wid] = acc;
            }
            __syncthreads();
#pragma unroll
            for (int b = 0; b < B; b++) {
                float t = 0.0f;
                for (uint32_t w = 0; w < NW; w++) t += red[b * 16 + w];
                t /= (float)n; t += 1e-5f;
                ss[b] = 1.0f / sqrtf(t);
            }
        }
        NANO_STAMP(a.stamps, 2, ss[0] + r.x[0][0].x);                // the activation arrived (and its norm scale is known)
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const uint32_t i = (tid + (uint32_t)j * nthr) * 4u;
#pragma unroll
            for (int b = 0; b < B; b++) {
                float4 v = r.x[b][j];
                if (norm) {
                    v.x = r.nw[j].x * (ss[b] * v.x); v.y = r.nw[j].y * (ss[b] * v.y);
                    v.z = r.nw[j].z * (ss[b] * v.z); v.w = r.nw[j].w * (ss[b] * v.w);
                }
                float m = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
                m = dpp_group_max<GS / 4>(m);
                const float scale = div_const<127>(m);
                if (i < n) {
                    quant_store4(v, scale, xq + b * n16 + i);
                    if ((tid % (GS / 4)) == 0) xs[b * ng4 + i / GS] = scale;
                }
            }
        }
        __syncthreads();
    }
}


// ordered fold of one row's group products (infer.c:668-674): NQ float4 = 4 NQ groups, all LDS reads first, then the chain
template <int NQ> __device__ __forceinline__ float fold_row(const float *p) {
    float4 t[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) t[q] = *reinterpret_cast<const float4 *>(p + 4 * q);
    float v = 0.0f;
#pragma unroll
    for (int q = 0; q < NQ; q++) { v += t[q].x; v += t[q].y; v += t[q].z; v += t[q].w; }
    return v;
}
template <int NQ> __device__ __forceinline__ void fold_row2(const float *p0, const float *p1, float &v0, float &v1) {
    float4 t[NQ], u[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) { t[q] = *reinterpret_cast<const float4 *>(p0 + 4 * q); u[q] = *reinterpret_cast<const float4 *>(p1 + 4 * q); }
    v0 = 0.0f; v1 = 0.0f;
#pragma unroll
    for (int q = 0; q < NQ; q++) { v0 += t[q].x; v1 += u[q].x; v0 += t[q].y; v1 += u[q].y; v0 += t[q].z; v1 += u[q].z; v0 += t[q].w; v1 += u[q].w; }
}

// CANONICAL fold of the fast path (kernels.h q80_canonical(); group size 64): unit sums S_u = the 8 group products of unit u added in
// ascending order, row = ((S_0 + S_1) + S_2) + ... -- the one reduction shape the batched kernels (G6, G7, G7K: gemm_q80_g6.hip, gemm_q80_g7.hip) share, so
// that a batch stays bit for bit its sequences alone whichever kernel a batch size is routed to.  NQ float4 = 4 NQ groups.
__device__ __forceinline__ float unit_sum(const float4 &t0, const float4 &t1) {
    float s = t0.x; s += t0.y; s += t0.z; s += t0.w; s += t1.x; s += t1.y; s += t1.z; s += t1.w;
    return s;
}
// One fp32 add the optimizer cannot pair: the SLP vectorizer turned two neighbouring unit sums into v_pk_add_f32 behind a shuffle of
// v_mov and let the scheduler sink the LDS reads next to them (three LDS round trips per row).  Same instruction the compiler emits for
// a + b, same rounding; not volatile, so it schedules freely.
__device__ __forceinline__ float fadd(float a, float b) { float r; asm("v_add_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// the NU = NQ / 2 unit sums of a row in lock step: NU independent add chains of depth 7 (a wave issues them back to back), then the
// NU - 1 adds of the units -- depth 7 + NU - 1 where the ordered chain has 8 NU - 1
template <int NU> __device__ __forceinline__ void unit_sums(const float4 *t, float *s) {
#pragma unroll
    for (int u = 0; u < NU; u++) s[u] = fadd(t[2 * u].x, t[2 * u].y);
#pragma unroll
    for (int u = 0; u < NU; u++) s[u] = fadd(s[u], t[2 * u].z);
#pragma unroll
    for (int u = 0; u < NU; u++) s[u] = fadd(s[u], t[2 * u].w);
#pragma unroll
    for (int u = 0; u < NU; u++) s[u] = fadd(s[u], t[2 * u + 1].x);
#pragma unroll
    for (int u = 0; u < NU; u++) s[u] = fadd(s[u], t[2 * u + 1].y);
#pragma unroll
    for (int u = 0; u < NU; u++) s[u] = fadd(s[u], t[2 * u + 1].z);
#pragma unroll
    for (int u = 0; u < NU; u++) s[u] = fadd(s[u], t[2 * u + 1].w);
}
template <int NQ> __device__ __forceinline__ float fold_row_canon(const float *p) {
    static_assert(NQ % 2 == 0, "whole units");
    float4 t[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) t[q] = *reinterpret_cast<const float4 *>(p + 4 * q);
    __builtin_amdgcn_sched_barrier(0);          // every LDS read of the row goes out before the first add (one round trip, not one per unit pair)
    float s[NQ / 2];
    unit_sums<NQ / 2>(t, s);
    float v = s[0];
#pragma unroll
    for (int u = 1; u < NQ / 2; u++) v = fadd(v, s[u]);
    return v;
}
// any group count that is a multiple of 4 (the last unit may hold 4 groups); two units per trip, their reads first
__device__ __forceinline__ float fold_row_canon_any(const float *p, uint32_t ng) {
    float v = 0.0f;
    for (uint32_t g0 = 0; g0 < ng; g0 += 16) {
        float4 t[4];
#pragma unroll
        for (int q = 0; q < 4; q++) t[q] = (g0 + 4u * (uint32_t)q < ng) ? *reinterpret_cast<const float4 *>(p + g0 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        float s = t[0].x; s += t[0].y; s += t[0].z; s += t[0].w;
        if (g0 + 4 < ng) { s += t[1].x; s += t[1].y; s += t[1].z; s += t[1].w; }
        v = g0 == 0 ? s : v + s;
        if (g0 + 8 < ng) {
            s = t[2].x; s += t[2].y; s += t[2].z; s += t[2].w;
            if (g0 + 12 < ng) { s += t[3].x; s += t[3].y; s += t[3].z; s += t[3].w; }
            v += s;
        }
    }
    return v;
}
// two rows (W1's and W3's of a SwiGLU launch): every LDS read of both goes out before the first add
template <int NQ> __device__ __forceinline__ void fold_row2_canon(const float *p0, const float *p1, float &v0, float &v1) {
    static_assert(NQ % 2 == 0, "whole units");
    float4 t[NQ], u[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) { t[q] = *reinterpret_cast<const float4 *>(p0 + 4 * q); u[q] = *reinterpret_cast<const float4 *>(p1 + 4 * q); }
    __builtin_amdgcn_sched_barrier(0);
    float s0[NQ / 2], s1[NQ / 2];
    unit_sums<NQ / 2>(t, s0); unit_sums<NQ / 2>(u, s1);
    v0 = s0[0]; v1 = s1[0];
#pragma unroll
    for (int k = 1; k < NQ / 2; k++) { v0 = fadd(v0, s0[k]); v1 = fadd(v1, s1[k]); }
}
__device__ __forceinline__ void fold_row2_canon_ng(const float *p0, const float *p1, uint32_t ng, float &v0, float &v1) {
    if (ng == 16u) { fold_row2_canon<4>(p0, p1, v0, v1); return; }
    v0 = fold_row_canon_any(p0, ng); v1 = fold_row_canon_any(p1, ng);
}
__device__ __forceinline__ float fold_row_canon_ng(const float *p, uint32_t ng) {
    if (ng == 16u) return fold_row_canon<4>(p);
    if (ng == 32u) return fold_row_canon<8>(p);
    if (ng == 48u) return fold_row_canon<12>(p);
    return fold_row_canon_any(p, ng);
}

// The same fold INSIDE a wave, for rows of one 1 KiB chunk (n == 1024, group size 64: 16 groups = two whole units).  After the integer dots
// lane 4 g + r holds the product of (row r, group g) of the wave's four-row unit; the table, the workgroup barrier and the one fold thread
// per row are a detour there.  S_0 (groups 0..7) lives in lanes 0..31, S_1 (groups 8..15) in lanes 32..63, both chains in the same
// instructions, all four rows at once (lanes r mod 4):
//   lanes r | 32 + r       ((p_0 + p_1) + p_2) + p_3          the later groups of the 16-lane row by DPP row_shl:4 / 8 / 12 (three moves that
//                                                             depend on the product only: off the chain)
//   lanes 16 + r | 48 + r  that value carried one row up (v_permlane16_swap: odd rows <- even rows), then + p_4 + p_5 + p_6 + p_7 with the
//                          SAME three moved registers (in these lanes they hold groups 5..7)
//   lanes 48 + r           S_0 from lanes 16 + r (v_permlane32_swap: upper half <- lower half), row = S_0 + S_1
// Every add is one v_add_f32 with the running value first: the float of fold_row_canon<4> for every input (tests/test_wave_fold_order.py
// restates this schedule lane by lane).  The row results are in lanes 48..51.
__device__ __forceinline__ float wave_fold_canon16(float p) {
    const float p1 = DPP_F(p, 0x104), p2 = DPP_F(p, 0x108), p3 = DPP_F(p, 0x10C);
    float s = fadd(p, p1); s = fadd(s, p2); s = fadd(s, p3);
    const uint32_t sb = __float_as_uint(s);
    const float c = __uint_as_float(__builtin_amdgcn_permlane16_swap(sb, sb, false, false)[0]);
    s = fadd(c, p); s = fadd(s, p1); s = fadd(s, p2); s = fadd(s, p3);
    const uint32_t tb = __float_as_uint(s);
    const float s0 = __uint_as_float(__builtin_amdgcn_permlane32_swap(tb, tb, false, false)[0]);
    return fadd(s0, s);
}
constexpr int WF_LANE0 = 48;          // wave_fold_canon16(): lane WF_LANE0 + r holds row r
// Its sibling for rows of SEVERAL chunks (SLAB_WFC), one chunk per wave: the same schedule up to the v_permlane32_swap, both unit sums of the
// chunk returned -- in lanes WF_LANE0 + r, s0 = S_2c and s1 = S_2c+1 of row r.  The fold thread of the row adds the units in ascending order:
// (S_0 + S_1), then (v + S_2c) + S_2c+1 per later chunk -- fold_row_canon<4 NCH>'s float for every input (tests/test_wave_fold_chunks_order.py).
__device__ __forceinline__ void wave_fold_canon16_units(float p, float &s0, float &s1) {
    const float p1 = DPP_F(p, 0x104), p2 = DPP_F(p, 0x108), p3 = DPP_F(p, 0x10C);
    float s = fadd(p, p1); s = fadd(s, p2); s = fadd(s, p3);
    const uint32_t sb = __float_as_uint(s);
    const float c = __uint_as_float(__builtin_amdgcn_permlane16_swap(sb, sb, false, false)[0]);
    s = fadd(c, p); s = fadd(s, p1); s = fadd(s, p2); s = fadd(s, p3);
    const uint32_t tb = __float_as_uint(s);
    s0 = __uint_as_float(__builtin_amdgcn_permlane32_swap(tb, tb, false, false)[0]);
    s1 = s;
}

// ------------------------------------------------------------------------------------------------------------
// SLAB kernel
// ------------------------------------------------------------------------------------------------------------
// Hand-off of a launch's results to consumers INSIDE the same launch (the fused kernels below): every result is also stored as an 8-byte
// {tag, value} granule (ONE write-through store: the data is the flag); SlabHand and the epoch tags: device_common.h.
template <int ROLE, int GS, int B, int NV, int UPW, int EARLY = 0, int WF = 0, int WFC = 0>
__global__ __launch_bounds__(1024) void gemv_q80_slab_kernel(const GemvDev a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#define SLAB_EARLY EARLY
#define SLAB_WF WF
#define SLAB_WFC WFC
#define SLAB_A a
#define SLAB_BID blockIdx.x
#define SLAB_HAND 0
#define SLAB_HANDV (SlabHand{})
#define SLAB_PTAG 0u
#define SLAB_XHAND 0
#define SLAB_XHANDV (SlabHand{})
#define SLAB_CTAG 0u
#define SLAB_PART 0
#include "gemv_q80_slab_body.inc"
#undef SLAB_A
#undef SLAB_BID
#undef SLAB_HAND
#undef SLAB_HANDV
#undef SLAB_PTAG
#undef SLAB_XHAND
#undef SLAB_XHANDV
#undef SLAB_CTAG
#undef SLAB_PART
#undef SLAB_EARLY
#undef SLAB_WF
#undef SLAB_WFC
}

#if NANO_Q80_GS == 64
}  // namespace
}  // namespace nano
#include "attn_impl.h"
namespace nano {
namespace {
// ---- q | k | v projection + attention in ONE launch (Qwen3 decode, one sequence, head_dim 128; round 5) --------------------------------------
// The LAST `n_attn` workgroups are the attention's (head x split): they ask for their K / V rows at entry, exactly as the attention kernel
// does, and then wait for q, the raw k row and the fresh v row of their KV group as granules; the first `ngemv` workgroups are the projection's
// SLAB GEMV (role: rmsnorm + quantize + store), whose fold threads also store every result as a granule.  What the boundary between the two
// kernels cost -- the gap, the attention's entry ramp and its K / V round trip -- now overlaps the projection.  Bits: the same two bodies.
// Round 6: the PRODUCERS come first in the grid (round-5 advice: with the consumers in front, a chip that other work keeps busy could seat
// the pollers and leave the projection waiting for their slots); granules carry epoch tags (device_common.h), a consumer that gives up
// skips its stores.  Reference: infer/infer.c:758-879.
template <int NV, int UPW>
__global__ __launch_bounds__(256) void qkv_attn_fused_kernel(const QkvAttnArgs fa) {
#define SLAB_WF 0
#include "qkv_attn_fused_body.inc"
#undef SLAB_WF
}
// ... its form for n == 1024 (rows of one chunk): no product table, no barrier between the dots and the granules the attention workgroups wait
// for.  One float4 item per thread, one unit per wave: the only form a shape reaches (fused_shape)
__global__ __launch_bounds__(256) void qkv_attn_fused_wf_kernel(const QkvAttnArgs fa) {
    constexpr int NV = 1, UPW = 1;
#define SLAB_WF 1
#include "qkv_attn_fused_body.inc"
#undef SLAB_WF
}

// ---- Wo + W1|W3 in ONE launch (round 5): the first all-to-all edge of the block as an in-launch all-gather -------------------------------
// Wo's epilogue produces the residual stream x; W1|W3 needs ALL of x (rmsnorm, then every row times the whole vector): an all-to-all edge,
// a kernel boundary in every earlier build.  Here the launch has W1|W3's grid; its first `wo_wgs` workgroups run Wo's body first (results
// stored as usual AND as 8-byte {tag, value} granules), then EVERY workgroup runs W1|W3's body with the activation polled from the granules
// (gemv_q80_slab_body.inc SLAB_XHAND).  W1|W3's weight and norm-weight loads go out at kernel entry (SLAB_PART 1), BEFORE Wo's body: they are
// in LDS-distance when the granules arrive, and -- younger than Wo's own loads -- do not hold up Wo's wait counts.  What the boundary cost
// (the gap, the entry ramp, the activation's round trip behind a cold launch) is traded for the polls.  Deadlock: producers are the first
// workgroups of the grid and never wait for consumers; a grid of <= one workgroup per CU is resident as a whole.  Same bodies, same bits
// (test_fused_wo_w13_launch_equals_the_two_launches).  Reference: infer/infer.c:885-944.
struct Wo13Args { GemvDev wo; GemvDev w13; SlabHand hand; uint32_t wo_wgs, wait16; };   // wait16: naps of 16 x 64 cycles before a non-producer workgroup starts polling
// Eight waves, one float4 item per thread and one unit per wave in both bodies: the one form wo13_slabs() takes
template <int ROLE_A, int WF, int WFA>      // WF: W1|W3's rows are one chunk (n == 1024): SLAB_WF; WFA: Wo's rows are that many whole chunks: SLAB_WFC
__global__ __launch_bounds__(512) void wo_w13_fused_kernel(const Wo13Args fa) {
#define WO13_CW 0
#include "wo_w13_fused_body.inc"
#undef WO13_CW
}
// The plain SLAB kernel of the combine role with the combine in the wave (SLAB_CW; one sequence, one item per thread, the table
// form's units: plain or -- WFC -- rows of 2..4 whole chunks): what a step with the fusion off, or after a hand-off gave up, launches for Wo
template <int NV, int UPW, int WFC>
__global__ __launch_bounds__(1024) void gemv_q80_slab_cw_kernel(const GemvDev a) {
    static_assert(NV == 1, "one item per thread (gemv_q80_plan)");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int ROLE = R_RESID_COMBINE, GS = 64, B = 1;
#define SLAB_CW 1
#define SLAB_WFC WFC
#define SLAB_A a
#define SLAB_BID blockIdx.x
#define SLAB_HAND 0
#define SLAB_HANDV (SlabHand{})
#define SLAB_PTAG 0u
#define SLAB_XHAND 0
#define SLAB_XHANDV (SlabHand{})
#define SLAB_CTAG 0u
#define SLAB_PART 0
#include "gemv_q80_slab_body.inc"
#undef SLAB_A
#undef SLAB_BID
#undef SLAB_HAND
#undef SLAB_HANDV
#undef SLAB_PTAG
#undef SLAB_XHAND
#undef SLAB_XHANDV
#undef SLAB_CTAG
#undef SLAB_PART
#undef SLAB_WFC
#undef SLAB_CW
}
// ... with Wo's combine in the wave (SLAB_CW): no weight table, no barrier in front of Wo's quantizer, the live splits only
template <int WF, int WFA>
__global__ __launch_bounds__(512) void wo_w13_fused_cw_kernel(const Wo13Args fa) {
    constexpr int ROLE_A = R_RESID_COMBINE;
#define WO13_CW 1
#include "wo_w13_fused_body.inc"
#undef WO13_CW
}

#endif

// ------------------------------------------------------------------------------------------------------------
// STREAM kernel (classifier)
// ------------------------------------------------------------------------------------------------------------
template <int ROLE, int GS, int B, int NV>
__global__ __launch_bounds__(256) void gemv_q80_stream_kernel(const GemvDev a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int LPG = GS / 16, GC = 1024 / GS, F = GC / 4;
    static_assert(F >= 1, "group size too large for the stream kernel");
    const uint32_t n = a.n, ng = a.ng;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n16 = (n + 15) & ~15u, ng4 = (ng + 3) & ~3u;
    int8_t *xq = reinterpret_cast<int8_t *>(smem);
    float *xs = reinterpret_cast<float *>(smem + B * n16);
    float *red = xs + B * ng4;
    int *tab = reinterpret_cast<int *>(red + B * 16) + wid * 16 * GC;

    Staged<B, NV> sx;
    stage_issue<ROLE, B, NV>(a, sx);

    const uint32_t rows = a.rows[0];
    const uint32_t nchunk = a.nchunk;
    const uint32_t ntiles = (rows + 15) >> 4;
    const uint32_t nwaves = gridDim.x * 4, wave_g = blockIdx.x * 4 + (uint32_t)wid;
    const uint32_t nunits = (wave_g < ntiles) ? ((ntiles - wave_g + nwaves - 1) / nwaves) * nchunk : 0;
    const __amdgpu_buffer_rsrc_t rw_ = mkrsrc(a.w[0], rows * n);
    const __amdgpu_buffer_rsrc_t rs_ = mkrsrc(a.ws[0], rows * ng * 4u);

    int4 wA[16];
    float sA[F];
    // unit u of this wave -> (tile, chunk); chunk fastest so a row's running value stays in the wave
    uint32_t tile_i = 0, chunk_i = 0;                      // cursor of the NEXT unit to issue
    auto issue = [&](int4 (&w)[16], float (&s)[F]) {
        const uint32_t tile = wave_g + tile_i * nwaves;
        const uint32_t row0 = tile << 4;
        const uint32_t col = (chunk_i << 10) + (uint32_t)lane * 16u;
        const uint32_t base = (col < n) ? row0 * n + col : OOB;
#pragma unroll
        for (int r = 0; r < 16; r++) w[r] = bload_w(rw_, base + (uint32_t)r * n);       // rows beyond `rows` are out of range -> 0
        const uint32_t gb = chunk_i * GC + ((uint32_t)lane & 3u) * F;
        const uint32_t so = ((row0 + ((uint32_t)lane >> 2)) * ng + gb) * 4u;
#pragma unroll
        for (int f = 0; f < F; f++) s[f] = bload_f(rs_, (gb + f < ng) ? so + 4u * f : OOB);
        if (++chunk_i == nchunk) { chunk_i = 0; tile_i++; }
    };
    if (nunits) issue(wA, sA);

    stage_finish<ROLE, GS, B, NV>(a, sx, xq, xs, red, n16, ng4);

    float val[B], best[B];
    uint32_t besti[B];
#pragma unroll
    for (int b = 0; b < B; b++) { val[b] = 0.0f; best[b] = -INFINITY; besti[b] = 0xffffffffu; }
    uint32_t ctile = 0, cchunk = 0;                        // cursor of the unit being consumed
    auto consume = [&](int4 (&w)[16], float (&s)[F]) {
        const uint32_t tile = wave_g + ctile * nwaves;
        const uint32_t col = (cchunk << 10) + (uint32_t)lane * 16u;
        const uint32_t gb = cchunk * GC + ((uint32_t)lane & 3u) * F;
        const bool last = cchunk + 1 == nchunk;
        const uint32_t row = (tile << 4) + ((uint32_t)lane >> 2);
#pragma unroll
        for (int b = 0; b < B; b++) {
            if (b < (int)a.nb) {
                const int4 xv = (col < n) ? *reinterpret_cast<const int4 *>(xq + b * n16 + col) : make_int4(0, 0, 0, 0);
                int iv[16];
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    int d = __builtin_amdgcn_sdot4(w[r].x, xv.x, 0, false);
                    d = __builtin_amdgcn_sdot4(w[r].y, xv.y, d, false);
                    d = __builtin_amdgcn_sdot4(w[r].z, xv.z, d, false);
                    d = __builtin_amdgcn_sdot4(w[r].w, xv.w, d, false);
                    iv[r] = dpp_group_sum<LPG>(d);
                }
                if ((lane % LPG) == 0) {
#pragma unroll
                    for (int r = 0; r < 16; r++) tab[r * GC + lane / LPG] = iv[r];
                }
                float p[F];
#pragma unroll
                for (int f = 0; f < F; f++) {
                    const int v = tab[(lane >> 2) * GC + (lane & 3) * F + f];
                    const float xsc = (gb + f < ng) ? xs[b * ng4 + gb + f] : 0.0f;
                    p[f] = ((float)v * s[f]) * xsc;                                          // infer.c:672
                }
                // ordered fold over the 4 lanes of a row: stage k adds lane k's products onto the running value
                float cur = val[b];
#pragma unroll
                for (int st = 0; st < 4; st++) {
                    float t = cur;
#pragma unroll
                    for (int f = 0; f < F; f++) t += p[f];                                   // groups beyond ng add +0.0f (exact)
                    cur = (st == 0) ? DPP_F(t, 0x00) : (st == 1) ? DPP_F(t, 0x55) : (st == 2) ? DPP_F(t, 0xAA) : DPP_F(t, 0xFF);
                }
                val[b] = cur;
                if (last) {
                    if ((lane & 3) == 0 && row < rows) {
                        a.out[0][(size_t)b * a.out_bstride[0] + row] = cur;
                        if (cur > best[b] || besti[b] == 0xffffffffu) { best[b] = cur; besti[b] = row; }   // rows ascend per lane: first max kept
                    }
                    val[b] = 0.0f;
                }
            }
        }
        if (++cchunk == nchunk) { cchunk = 0; ctile++; }
    };
    // single register buffer: four waves per SIMD (128 VGPRs) keep the other tiles' loads in flight while one wave
    // consumes -- measured 4-5 % faster than a two-buffer software pipeline at two waves per SIMD (round-1 kernel laboratory)
    for (uint32_t u = 0; u < nunits; u++) {
        if (u) issue(wA, sA);
        consume(wA, sA);
    }
    // per-wave arg-max partial: larger value wins, equal values -> lower row (== the reference's first maximum)
    if (a.tile_max) {
#pragma unroll
        for (int b = 0; b < B; b++) {
            if (b < (int)a.nb) {
                float bv = best[b]; uint32_t bi = besti[b];
#pragma unroll
                for (int o = 32; o >= 4; o >>= 1) {
                    const float ov = __shfl_xor(bv, o, 64);
                    const uint32_t oi = __shfl_xor(bi, o, 64);
                    if (oi != 0xffffffffu && (bi == 0xffffffffu || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
                }
                if (lane == 0) {
                    float *tm = a.tile_max + ((size_t)b * a.ntiles + wave_g) * 2;
                    tm[0] = bv; tm[1] = __uint_as_float(bi);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------

// Every choice of a launch -- kernel, role, capacity, template values, waves, rows per workgroup, grid, LDS bytes, the special form -- is
// gemv_q80_plan()'s (gemv_q80.hip, kernels.h Q80GemvPlan): the launchers below only turn a plan into the instantiation it names.
template <int ROLE, int GS, int B, int NV, int UPW>
static hipError_t launch_slab_t(const GemvDev &d, const Q80GemvPlan &p, hipStream_t st) {
    GemvDev dd = d; dd.nthr = 64 * p.nw;
    const size_t lds = p.lds_bytes;
    // the matrices of >= 8 M weights (one or two sequences, group size 64): the first unit of every wave before the activation is
    // quantized, the others after (gemv_q80_slab_body.inc SLAB_EARLY)
    if constexpr (GS == 64 && B <= 2 && UPW >= 2 && NV >= 1) if (p.variant == Q80_VAR_EARLY) {
        auto kern = &gemv_q80_slab_kernel<ROLE, GS, B, NV, UPW, 1>;
        if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(p.grid), dim3(64 * p.nw), lds, st, dd);
        return hipGetLastError();
    }
    // rows of ONE chunk (n == 1024), one sequence, the rmsnorm roles (canonical launches only at this group size): every wave
    // folds its own rows -- no product table in the LDS budget, no barrier behind the dots (gemv_q80_slab_body.inc SLAB_WF).  W1|W3: units of
    // two rows of each matrix, so that a wave holds both halves of its SwiGLU pairs (the plan's units)
    if constexpr (GS == 64 && B == 1 && (ROLE == R_NORM_STORE || ROLE == R_NORM_SWIGLU) && (NV == 1 || NV == 2)) if (p.variant == Q80_VAR_WF) {
        hipLaunchKernelGGL((gemv_q80_slab_kernel<ROLE, GS, B, NV, UPW, 0, 1>), dim3(p.grid), dim3(64 * p.nw), lds, st, dd);
        return hipGetLastError();
    }
#if NANO_Q80_GS == 64
    // the combine role with the splits' weights made inside each wave (the plan's cw; its variant is plain or WFC2..4)
    if constexpr (GS == 64 && B == 1 && ROLE == R_RESID_COMBINE && NV == 1) if (p.cw) {
        if (p.variant == Q80_VAR_PLAIN) {
            auto kern = &gemv_q80_slab_cw_kernel<NV, UPW, 0>;
            if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, dim3(p.grid), dim3(64 * p.nw), lds, st, dd); return hipGetLastError();
        }
        if constexpr (UPW <= 2) {
            if (p.variant == Q80_VAR_WFC2) { hipLaunchKernelGGL((gemv_q80_slab_cw_kernel<NV, UPW, 2>), dim3(p.grid), dim3(64 * p.nw), lds, st, dd); return hipGetLastError(); }
            if (p.variant == Q80_VAR_WFC3) { hipLaunchKernelGGL((gemv_q80_slab_cw_kernel<NV, UPW, 3>), dim3(p.grid), dim3(64 * p.nw), lds, st, dd); return hipGetLastError(); }
            if (p.variant == Q80_VAR_WFC4) { hipLaunchKernelGGL((gemv_q80_slab_cw_kernel<NV, UPW, 4>), dim3(p.grid), dim3(64 * p.nw), lds, st, dd); return hipGetLastError(); }
        }
        return hipErrorInvalidValue;
    }
#endif
    // rows of 2..4 whole chunks, one sequence, the residual roles (Wo, W2; canonical launches only at this group size): every
    // wave folds the chunk of its unit to two unit sums -- 8 floats per unit in LDS instead of the product table, 2 nch - 1 adds behind the
    // barrier (gemv_q80_slab_body.inc SLAB_WFC).  (The plans of such matrices have <= 8 units on >= 6 waves: one or two units per wave.)
    if constexpr (GS == 64 && B == 1 && (ROLE == R_RESID || ROLE == R_RESID_COMBINE) && (NV == 1 || NV == 2) && UPW <= 2) {
        if (p.variant == Q80_VAR_WFC2) { hipLaunchKernelGGL((gemv_q80_slab_kernel<ROLE, GS, B, NV, UPW, 0, 0, 2>), dim3(p.grid), dim3(64 * p.nw), lds, st, dd); return hipGetLastError(); }
        if (p.variant == Q80_VAR_WFC3) { hipLaunchKernelGGL((gemv_q80_slab_kernel<ROLE, GS, B, NV, UPW, 0, 0, 3>), dim3(p.grid), dim3(64 * p.nw), lds, st, dd); return hipGetLastError(); }
        if (p.variant == Q80_VAR_WFC4) { hipLaunchKernelGGL((gemv_q80_slab_kernel<ROLE, GS, B, NV, UPW, 0, 0, 4>), dim3(p.grid), dim3(64 * p.nw), lds, st, dd); return hipGetLastError(); }
    }
    if (p.variant != Q80_VAR_PLAIN) return hipErrorInvalidValue;          // (a form this instantiation does not have: the plan and the templates disagree)
    auto kern = &gemv_q80_slab_kernel<ROLE, GS, B, NV, UPW>;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(64 * p.nw), lds, st, dd);
    return hipGetLastError();
}
// the instantiations: every (NV, UPW) of {0, 1, 2, 4} x {1, 2, 4} with B * NV <= 8 (tests/test_q80_gemv_plan.py restates the set)
template <int ROLE, int GS, int B>
static hipError_t launch_slab_r(const GemvDev &d, const Q80GemvPlan &p, hipStream_t st) {
#define SLAB_GO(NV_, UPW_) do { if constexpr (B * NV_ <= 8) { if (p.nv == NV_ && p.upw == UPW_) return launch_slab_t<ROLE, GS, B, NV_, UPW_>(d, p, st); } } while (0)
    SLAB_GO(1, 1); SLAB_GO(1, 2); SLAB_GO(1, 4);
    SLAB_GO(2, 1); SLAB_GO(2, 2); SLAB_GO(2, 4);
    SLAB_GO(4, 1); SLAB_GO(4, 2); SLAB_GO(4, 4);
    SLAB_GO(0, 1); SLAB_GO(0, 2); SLAB_GO(0, 4);
    return hipErrorInvalidValue;
#undef SLAB_GO
}
template <int GS, int B>
static hipError_t launch_slab_b(GemvDev &d, const Q80GemvPlan &p, hipStream_t st) {
    d.rw = p.rw;
    d.early = p.early;
    d.tpw = (p.rw + 3) / 4;
    d.magic_rw = 65536u / p.rw + 1u;                                   // (tid * magic_rw) >> 16 == tid / rw for tid < 1024 <= 65536 / rw
    d.log2_tiles = 0;
    d.units = p.units;
    d.wg_c0 = p.wg_c0; d.wg_c1 = p.wg_c1;                              // workgroups up to the end of segment 0 / 1 (a workgroup's rows lie inside one segment)
    // the per-layer launches of a batch-1 step: flags resolved at compile time.  Group size 64: the role kernels carry the canonical fold
    // only, so a launch that is not canonical (strict mode; a row length that is no multiple of 256) has the generic kernel in its plan
    if constexpr (B == 1) {
        if (p.role == R_NORM_STORE) return launch_slab_r<R_NORM_STORE, GS, B>(d, p, st);
        if (p.role == R_RESID) return launch_slab_r<R_RESID, GS, B>(d, p, st);
        if (p.role == R_RESID_COMBINE) return launch_slab_r<R_RESID_COMBINE, GS, B>(d, p, st);
        if (p.role == R_NORM_SWIGLU) return launch_slab_r<R_NORM_SWIGLU, GS, B>(d, p, st);
    }
    if (p.role != R_GENERIC) return hipErrorInvalidValue;
    return launch_slab_r<R_GENERIC, GS, B>(d, p, st);
}

template <int ROLE, int GS, int B>
static hipError_t launch_stream_r(GemvDev &d, const Q80GemvPlan &p, hipStream_t st) {
    d.ntiles = p.grid * 4; d.nthr = 64 * p.nw;
    const size_t lds = p.lds_bytes;
    hipEvent_t e0 = g_q80_probe_start, e1 = g_q80_probe_stop;
    g_q80_probe_start = g_q80_probe_stop = nullptr;
#define STREAM_GO(NV_) do { auto kern = &gemv_q80_stream_kernel<ROLE, GS, B, NV_>; \
                            if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
                            if (e0 && e1) hipExtLaunchKernelGGL(kern, dim3(p.grid), dim3(64 * p.nw), (uint32_t)lds, st, e0, e1, 0, d); \
                            else hipLaunchKernelGGL(kern, dim3(p.grid), dim3(64 * p.nw), lds, st, d); return hipGetLastError(); } while (0)
    if (p.nv == 1) STREAM_GO(1);
    if constexpr (B <= 4) { if (p.nv == 2) STREAM_GO(2); }
    if constexpr (B <= 2) { if (p.nv == 4) STREAM_GO(4); }
    if (p.nv == 0) STREAM_GO(0);
#undef STREAM_GO
    return hipErrorInvalidValue;
}
template <int GS, int B>
static hipError_t launch_stream_b(GemvDev &d, const Q80GemvPlan &p, hipStream_t st) {
    if (p.role == R_NORM_STORE) return launch_stream_r<R_NORM_STORE, GS, B>(d, p, st);      // the classifier
    if (p.role != R_GENERIC) return hipErrorInvalidValue;
    return launch_stream_r<R_GENERIC, GS, B>(d, p, st);
}

#if NANO_Q80_GS == 64
// ---- the fused q | k | v + attention launch: host side -----------------------------------------------------------------------------------
// Every choice of the launch (kernels.h QkvAttnFusedPlan): the projection's own slab plan where it runs on four waves, the table or the
// in-wave fold, the attention workgroups, the larger of the two kinds' LDS.
static bool fused_shape(const GemvArgs &ga, const AttnArgs &aa, QkvAttnFusedPlan &f) {
    if (ga.gs != 64 || ga.nb != 1 || ga.nseg != 3 || ga.epi != GEMV_EPI_STORE || !ga.norm_w || ga.xq_in || ga.attn_part || ga.tile_max || ga.resid_add) return false;
    if (ga.n % 64u || ga.n > 4096u || use_stream(ga) || !q80_canonical(ga)) return false;        // (the role kernels of group size 64 carry the canonical fold only)
    if (ga.seg[0].out_pstride || ga.seg[1].out_pstride) return false;            // (only v is position indexed: its cache row)
    const SlabPlan p = q80_plan_slab(ga, 1);
    if (p.nw != 4u || p.upw > 4u) return false;                                  // 256 threads, like the attention workgroups
    const GemvDev d = to_dev(ga);
    const bool wf = slab_wave_fold(d);                    // n == 1024: the projection's waves fold their own rows, no product table
    const uint32_t upw = p.upw <= 1 ? 1u : p.upw <= 2 ? 2u : 4u;
    // The built forms and no other.  Four waves = ceil(n / 384) mean n <= 1536: two float4 items per thread at most, no NV 4.  More than 8
    // units of two chunks -- in the wave fold, more than 4 of one chunk -- need slabs of >= 20 rows, which q80_plan_slab grows only from
    // 16384 rows on: >= 8 Mi weights, and those matrices get >= 8 waves: no <2, 4>, and the wave fold holds one unit per wave.
    if (wf ? p.nv != 1u || upw != 1u : !(p.nv == 1u || (p.nv == 2u && upw <= 2u))) return false;
    if (!fused_attn_side_ok(aa, ga.seg[0].rows, ga.seg[1].rows, ga.seg[2].rows, false)) return false;   // (kernels.h)
    f = QkvAttnFusedPlan{};
    f.kernel = wf ? FUSED_KERNEL_Q80_WF : FUSED_KERNEL_Q80_TABLE;
    f.nv = p.nv; f.upw = upw;
    f.threads = 256; f.rw = p.rw;
    for (uint32_t s2 = 0; s2 < 3; s2++) { f.wg[s2] = (ga.seg[s2].rows + p.rw - 1) / p.rw; f.ngemv += f.wg[s2]; }
    f.n_attn = fused_attn_wgs(aa);
    const uint32_t tpw = (p.rw + 3) / 4;
    const size_t n16 = (d.n + 15) & ~15u, ng4 = (d.ng + 3) & ~3u, pitch = ((d.ng + 47) / 64) * 64 + 16;
    const size_t lds_g = n16 + ng4 * 4 + 64 + (wf ? 0 : (size_t)(tpw * 4) * pitch * 4), lds_a = fused_attn_lds(aa.hd, false);
    const size_t lds = lds_g > lds_a ? lds_g : lds_a;
    if (lds > FUSED_LDS_MAX) return false;
    f.lds_bytes = (uint32_t)lds;
    return true;
}

// ---- the fused Wo + W1|W3 launch: host side ----------------------------------------------------------------------------------------------
// Both bodies run on the launch's 512 threads (W1|W3's rmsnorm tree follows the thread count; Wo has no tree: any count gives its bits).
// One form: Qwen3-0.6B's shapes.  (Qwen3-4B's wide matrices had a 1024-thread form; it lost to the two plain launches -- 1.531 vs 1.473 ms
// per step -- and was removed: those shapes are refused here and take the plain launches.)
struct Wo13Plan { SlabPlan a, b; uint32_t wa, wb; };
static bool wo13_slabs(const GemvArgs &wo, const GemvArgs &w13, Wo13Plan &q) {
    if (wo.gs != 64 || w13.gs != 64 || wo.nb != 1 || w13.nb != 1 || !q80_canonical(wo) || !q80_canonical(w13)) return false;
    if (wo.nseg != 1 || wo.epi != GEMV_EPI_RESID || wo.norm_w || wo.xq_in || wo.tile_max || wo.resid_add || wo.seg[0].out_pstride) return false;
    if (wo.attn_part && (wo.attn_nsplit > 8u || wo.attn_hd % 4u)) return false;
    if (w13.nseg != 2 || w13.epi != GEMV_EPI_SWIGLU || !w13.norm_w || w13.xq_in || w13.attn_part || w13.tile_max || w13.resid_add) return false;
    if (use_stream(wo) || use_stream(w13) || w13.n != wo.seg[0].rows || w13.xin != wo.seg[0].out || w13.n % 4u) return false;
    q.a = q80_plan_slab(wo, 1); q.b = q80_plan_slab(w13, 1);
    q.wa = (wo.seg[0].rows + q.a.rw - 1) / q.a.rw; q.wb = (w13.seg[0].rows + q.b.rw - 1) / q.b.rw;
    const uint32_t cus = w13.cus ? w13.cus : 256u;
    if (q.wa > q.wb || q.wb > cus) return false;                                                // one workgroup per CU: the whole grid is resident
    // One form: EIGHT waves, one float4 item per thread and one unit per wave in both bodies.  Its shapes are the small matrices the first fused
    // build ran on W1|W3's own four waves (one item per thread and two units per wave there; Wo's threads quantized two items each and held at
    // most 4 units): every one of them has at most 512 items and 8 units a side -- 32 rows, a fold thread each (Qwen3-0.6B: Wo's 512 items, 4
    // units; W1|W3's 256 items, 6 units).  Why eight waves (round 6, last day): same bits (Wo has no tree; W1|W3's items sit on the same
    // threads), and on the same box, driver's flags | full window:
    // 1991.2 | 1894.2, 1992.5 | 1893.4, 1990.7 | 1895.2 with four waves, 2033.3 | 1919.6, 2039.2 | 1937.1, 2030.2 | 1919.2 with eight.
    const uint32_t units_a = ((q.a.rw + 3) / 4) * ((wo.n + 1023) / 1024), items_a = wo.n / 4;
    const uint32_t units_b = ((q.b.rw + 3) / 4) * ((w13.n + 1023) / 1024) * 2u, items_b = w13.n / 4;
    return q.b.nw == 4u && q.b.nv == 1u && q.b.upw == 2u && units_b <= 8u && items_b >= 1u && items_b <= 512u &&      // W1|W3
           items_a > 256u && items_a <= 512u && units_a >= 1u && units_a <= 4u;                                          // Wo
}
static void slab_dev_fill(GemvDev &d, const GemvArgs &a, const SlabPlan &p, uint32_t nthr) {
    d.tile_max = nullptr;
    d.rw = p.rw; d.tpw = (p.rw + 3) / 4; d.magic_rw = 65536u / p.rw + 1u; d.log2_tiles = 0;
    d.units = d.tpw * d.nchunk * (a.epi == GEMV_EPI_SWIGLU ? 2u : 1u);
    d.wg_c0 = 0xffffffffu; d.wg_c1 = 0xffffffffu;
    d.nthr = nthr;
}
static size_t slab_lds(const GemvDev &d, bool table = true, bool wgt = true) {      // wgt: the combine's weight table [n_head][8] (SLAB_CW has none)
    const uint32_t nmat = d.epi == GEMV_EPI_SWIGLU ? 2 : 1;
    const size_t n16 = (d.n + 15) & ~15u, ng4 = (d.ng + 3) & ~3u, pitch = ((d.ng + 47) / 64) * 64 + 16;
    return n16 + ng4 * 4 + 64 + ((d.flags & F_COMBINE) && wgt ? (size_t)d.attn_n_head * 32 : 0) + (table ? (size_t)nmat * (d.tpw * 4) * pitch * 4 : 0);
}
// Every choice of the launch (kernels.h WoW13FusedPlan), and the two device blocks it was made from
static bool wo13_shape(const GemvArgs &wo, const GemvArgs &w13, WoW13FusedPlan &f, GemvDev &da, GemvDev &db) {
    Wo13Plan q;
    if (!wo13_slabs(wo, w13, q)) return false;
    da = to_dev(wo); db = to_dev(w13);
    slab_dev_fill(da, wo, q.a, 512); slab_dev_fill(db, w13, q.b, 512);
    // W1|W3's rows of one chunk (n == 1024): pair units (two rows of W1 and the same two of W3), folded by the wave that holds them
    const bool wf = slab_wave_fold(db);
    if (wf) db.units = (db.rw + 1) / 2;
    // Wo's rows of two whole chunks (n == 2048, the widest this form takes): every wave folds its unit's chunk to two unit sums (SLAB_WFC)
    const bool wfa = slab_wave_fold_chunks(da) == 2u;
    // Wo behind split attention: the splits' weights made inside each wave where the heads tile a wave's items (SLAB_CW)
    const bool cw = (da.flags & F_COMBINE) && combine_wave_shape(wo);
    const size_t la = slab_lds(da, !wfa, !cw) + (wfa ? slab_unit_table(da, 2u) : 0), lb = slab_lds(db, !wf), lds = la > lb ? la : lb;
    if (lds > FUSED_LDS_MAX) return false;
    f = WoW13FusedPlan{};
    f.sig = 3; f.threads = 512;                                                 // (sig: the queries' word for this form; 1 was the four-wave one)
    f.role = (da.flags & F_COMBINE) ? (uint32_t)R_RESID_COMBINE : (uint32_t)R_RESID;
    f.wf = wf ? 1u : 0u; f.wfc = wfa ? 2u : 0u;
    f.nv_a = 1; f.upw_a = 1; f.nv_b = 1; f.upw_b = 1;
    f.wa = q.wa; f.wb = q.wb; f.lds_bytes = (uint32_t)lds;
    f.rw_a = q.a.rw; f.rw_b = q.b.rw;
    f.cw = cw ? 1u : 0u;
    return true;
}

#endif

template <int GS, int B>
static hipError_t launch_b(const GemvArgs &a, const Q80GemvPlan &p, hipStream_t st) {
    GemvDev d = to_dev(a);
    if (p.kernel == Q80_KERNEL_STREAM) return launch_stream_b<GS, B>(d, p, st);
    d.tile_max = nullptr;
    return launch_slab_b<GS, B>(d, p, st);
}
template <int GS>
static hipError_t launch_gs(const GemvArgs &a, const Q80GemvPlan &p, hipStream_t st) {
    if (p.gs != (uint32_t)GS) return hipErrorInvalidValue;
    if (p.B == 1) return launch_b<GS, 1>(a, p, st);
    if (p.B == 2) return launch_b<GS, 2>(a, p, st);
    if (p.B == 4) return launch_b<GS, 4>(a, p, st);
    return launch_b<GS, 8>(a, p, st);
}

}  // namespace

hipError_t NANO_Q80_ENTRY(const GemvArgs &a, const Q80GemvPlan &p, hipStream_t st) { return launch_gs<NANO_Q80_GS>(a, p, st); }

#if NANO_Q80_GS == 64
bool qkv_attn_fused_q80_plan(const GemvArgs &ga, const AttnArgs &aa, QkvAttnFusedPlan *out) {
    QkvAttnFusedPlan f;
    if (!fused_shape(ga, aa, f)) return false;
    if (out) *out = f;
    return true;
}

hipError_t launch_qkv_attn_fused_q80(const GemvArgs &ga, const AttnArgs &aa, unsigned long long *hand, uint32_t *tick, uint32_t layer1, hipStream_t st) {
    QkvAttnFusedPlan p;
    if (!hand || !tick || !layer1 || layer1 > 127u || !fused_shape(ga, aa, p)) return hipErrorInvalidValue;
    GemvDev d = to_dev(ga);
    d.tile_max = nullptr;
    d.rw = p.rw; d.tpw = (p.rw + 3) / 4; d.magic_rw = 65536u / p.rw + 1u; d.log2_tiles = 0;
    d.units = d.tpw * d.nchunk;
    d.wg_c0 = p.wg[0]; d.wg_c1 = p.wg[0] + p.wg[1];
    d.nthr = p.threads;
    QkvAttnArgs fa{};
    fused_attn_setup(fa, aa, hand, tick, layer1);
    const uint32_t grid = p.n_attn + p.ngemv;
    const size_t lds = p.lds_bytes;
    fa.g = d; fa.ngemv = p.ngemv;
    // The attention workgroups nap `wait16` x 16 x 64 cycles between asking for their K / V rows and the first poll.  Round 5 (consumers FIRST in
    // the grid: they started before the projection) tuned 3: 1881-1887 tok/s without, 1899-1901 with 3, 1851 with 5.  Round 6 put the PRODUCERS
    // first -- the attention workgroups start last and the nap is mostly dead time: same box, driver's flags, 0 / 1 / 2 / 3 naps: 1984 / 1983 /
    // 1961 / 1919, 1977 / 1986 / 1958 / 1920, 1982 / 1981 / 1960 / 1912 tok/s; positions 31..510: 1878 / 1880 / 1859 / 1821
    // (profiles/r06_handoff_naps.txt).
    fa.wait16 = 1u;
    // the instantiations: the table form's <NV, UPW> of <1, 1> <1, 2> <1, 4> <2, 1> <2, 2> and the wave-fold kernel -- what fused_shape() lets through
    // (tests/test_fused_launch_plan.py restates the set)
    if (p.kernel == FUSED_KERNEL_Q80_WF) { hipLaunchKernelGGL(qkv_attn_fused_wf_kernel, dim3(grid), dim3(p.threads), lds, st, fa); return hipGetLastError(); }
#define FUSED_GO(NV_, UPW_) do { if (p.nv == NV_ && p.upw == UPW_) { hipLaunchKernelGGL((qkv_attn_fused_kernel<NV_, UPW_>), dim3(grid), dim3(p.threads), lds, st, fa); return hipGetLastError(); } } while (0)
    FUSED_GO(1, 1); FUSED_GO(1, 2); FUSED_GO(1, 4);
    FUSED_GO(2, 1); FUSED_GO(2, 2);
#undef FUSED_GO
    return hipErrorInvalidValue;
}

bool wo_w13_fused_plan(const GemvArgs &wo, const GemvArgs &w13, WoW13FusedPlan *out) {
    WoW13FusedPlan f; GemvDev da, db;
    if (!wo13_shape(wo, w13, f, da, db)) return false;
    if (out) *out = f;
    return true;
}

hipError_t launch_wo_w13_fused(const GemvArgs &wo, const GemvArgs &w13, unsigned long long *hand, uint32_t *tick, uint32_t layer1, hipStream_t st) {
    WoW13FusedPlan q;
    Wo13Args fa{};
    if (!hand || !tick || !layer1 || layer1 > 127u || !wo13_shape(wo, w13, q, fa.wo, fa.w13)) return hipErrorInvalidValue;
    fa.wo_wgs = q.wa;
    // workgroups that produce nothing nap 4 x 16 x 64 cycles (~2 us) before their first poll, every workgroup 128 cycles between sweeps: same
    // box, driver's flags, Qwen3-0.6B: 1846-1852 tok/s without, 1855-1865 with 2, 1879-1889 with 3, 1882-1887 with 4, 1847-1852 with 5, 1806-1817 with 6
    fa.wait16 = 4u;             // (round 6, with one nap in the q|k|v + attention launch: 0 / 2 / 4 naps here 1959 / 1978 / 1982 and 1959 / 1975 / 1982 tok/s)
    SlabHand h{};
    h.buf = hand; h.tick = tick; h.layer1 = layer1;
    h.base[0] = 0; h.base[1] = 0; h.base[2] = 0;
    fa.hand = h;
    const size_t lds = q.lds_bytes;
    // the instantiations: <role, WF, WFC> of {R_RESID, R_RESID_COMBINE} x {0, 1} x {0, 2} (tests/test_fused_launch_plan.py restates the set),
    // and the in-wave combine's <WF, WFC> of {0, 1} x {0, 2} (tests/test_wo_combine_wave_order.py)
#define WO13_CW_GO(WF_, WFC_) do { if (q.cw && q.role == (uint32_t)R_RESID_COMBINE && q.wf == WF_ && q.wfc == WFC_) { \
        hipLaunchKernelGGL((wo_w13_fused_cw_kernel<WF_, WFC_>), dim3(q.wb), dim3(q.threads), lds, st, fa); return hipGetLastError(); } } while (0)
    WO13_CW_GO(0, 0); WO13_CW_GO(0, 2); WO13_CW_GO(1, 0); WO13_CW_GO(1, 2);
#undef WO13_CW_GO
    if (q.cw) return hipErrorInvalidValue;
#define WO13_GO(RA_, WF_, WFC_) do { if (q.role == (uint32_t)RA_ && q.wf == WF_ && q.wfc == WFC_) { \
        hipLaunchKernelGGL((wo_w13_fused_kernel<RA_, WF_, WFC_>), dim3(q.wb), dim3(q.threads), lds, st, fa); return hipGetLastError(); } } while (0)
    WO13_GO(R_RESID, 0, 0); WO13_GO(R_RESID, 0, 2); WO13_GO(R_RESID, 1, 0); WO13_GO(R_RESID, 1, 2);
    WO13_GO(R_RESID_COMBINE, 0, 0); WO13_GO(R_RESID_COMBINE, 0, 2); WO13_GO(R_RESID_COMBINE, 1, 0); WO13_GO(R_RESID_COMBINE, 1, 2);
#undef WO13_GO
    return hipErrorInvalidValue;
}
#endif

}  // namespace nano
