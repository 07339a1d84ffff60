// gemm_f32.hip -- FP32 skinny GEMM on the FP32 matrix cores for 9..64 tokens per weight read (large decode batches, 64-token prefill
// chunks of FP32 models): what gemm_q80*.hip is for Q80 and gemm_q4k.hip for Q4K.  out[t][r] = W[r,:] . x_t for every token t, BIT FOR BIT
// the FP32 GEMV's result (gemv_f32_slab_body.inc), whose reduction shape per row and 256-float chunk is
//     lane l:  p_l = w[4l] x[4l], then three fused multiply-adds over 4l+1 .. 4l+3
//     chunk:   the balanced pairwise tree over p_0 .. p_63 (dpp_wave_sum)
//     row:     v = 0.0f; v += chunk_0; v += chunk_1; ...; finish_epi
//   * v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain per result (one rounding per product, subnormals kept).  With C = 0 and the four
//     columns of a float4 item as its K it returns p_l for 16 rows x 16 tokens; the only difference is the sign of a zero
//     (fma(a, b, +0) against a * b), which survives the tree only as the sign of a zero chunk sum and is erased by the fold's 0.0f + ...
//   * the tree is plain fp32 adds on the MFMA results, in the tree's own association: items (0+1), (2+3), ... then pairs of pairs.  A UNIT
//     is half a chunk (32 items): its sum is one level below the chunk sum, so chunk = unit_0 + unit_1 and the waves of a workgroup can
//     split a row at unit granularity.  Unit sums go to an LDS table [matrix][unit][row][token]; after one barrier a thread per
//     (row, token) adds (unit_0 + unit_1) of every chunk in ascending order from 0.0f and runs the shared finish_epi.
//   * columns at or beyond n are zeros on both sides (out-of-range weight loads, zero-filled activation pad): +0.0f products, as the GEMV's.
//
// Data flow.  A workgroup = one 16-row tile (the W1 and the W3 tile of the same rows for SwiGLU) x all tokens; unit u belongs to wave
// u % nw.  A operand (lane i + 16 k wants W[row i][4 item + k]): the wave loads its unit coalesced and non-temporally (a row's 512 bytes
// per half wave), writes the four components of every float4 to its private LDS buffer as [k * 16 + row][item] and reads its 32 operand
// values back with eight 16-byte reads -- a 4 x 4 transpose through LDS, no barrier (a wave's LDS queue is in order).  B operand: the
// prologue launch below wrote every token's activation in operand order, [token tile][unit][item / 4][lane = k * 16 + token][item % 4]:
// one coalesced 16-byte load per four items, straight from L2, one token tile ahead.  Token columns >= nb are computed on zeros and never
// stored.
//
// The prologue (one workgroup per token) is the GEMV's own staging code (gemv_f32_stage.h: stage_issue + stage_finish_f32 of the generic
// role, one sequence, loop form) on the thread count of the sliced route's launch for the shape, so the rmsnorm sum-of-squares tree and
// therefore every normalised activation is the one of the route this replaces; it then copies the vector from LDS into operand order.
#include "gemv_f32_stage.h"
#include "gemm_f32_host.h"

namespace nano {

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

struct GemmF32Dev {
    const float *w[3]; float *out[3];
    uint32_t rows[3], out_bstride[3], out_pstride[3];
    uint32_t n, epi, nb, nt, nu, nw, tp, tab_off;
    const float *xs; const uint32_t *pos;
};

// ---- prologue: token blockIdx.x -> rmsnorm (or a copy) -> operand order -------------------------------------------------------
__global__ __launch_bounds__(1024) void gemm_f32_prologue_kernel(const GemvDev a, float *xs, const uint32_t nu) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tok = blockIdx.x, n = a.n, n4 = (n + 3) & ~3u;
    float *xf = reinterpret_cast<float *>(smem);                   // [n4]
    float *red = xf + n4;                                          // [16]
    GemvDev t = a;
    t.nb = 1; t.xin = a.xin + (size_t)tok * a.xin_bstride;
    Staged<1, 0> sx;
    stage_issue<R_GENERIC, 1, 0>(t, sx);
    stage_finish_f32<R_GENERIC, 1, 0>(t, sx, xf, red, n4);         // (ends with a workgroup barrier)
    const uint32_t tt = tok >> 4, tn = tok & 15u;
    float *dst = xs + (size_t)tt * nu * GF_UNIT * 16u;
    for (uint32_t i = threadIdx.x; i < nu * GF_ITEMS; i += a.nthr) {
        const float4 v = (i * 4u < n) ? *reinterpret_cast<const float4 *>(xf + i * 4u) : make_float4(0.f, 0.f, 0.f, 0.f);
        const uint32_t u = i / GF_ITEMS, j = i % GF_ITEMS;
        float *d = dst + ((size_t)(u * (GF_ITEMS / 4u) + (j >> 2)) * 64u + tn) * 4u + (j & 3u);      // lane k * 16 + tn: 64 floats further per k
        d[0] = v.x; d[64] = v.y; d[128] = v.z; d[192] = v.w;
    }
}

// the pairwise tree over the items [LO, LO + N) of a unit: one MFMA from a zero accumulator per item, never chained through C
template <int LO, int N>
__device__ __forceinline__ v4f item_tree(const float (&a)[GF_ITEMS], const float (&b)[GF_ITEMS]) {
    if constexpr (N == 1) return __builtin_amdgcn_mfma_f32_16x16x4f32(a[LO], b[LO], v4f{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
    else return item_tree<LO, N / 2>(a, b) + item_tree<LO + N / 2, N / 2>(a, b);
}

template <bool SW>
__global__ __launch_bounds__(64 * GF_MAX_NW) void gemm_f32_kernel(const GemmF32Dev a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t nmat = SW ? 2u : 1u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t n = a.n, NT = a.nt, NU = a.nu, TP = a.tp;
    const uint32_t b0 = a.rows[0], b1 = b0 + a.rows[1];
    const uint32_t grow0 = blockIdx.x * GF_RT;
    const int sel = SW ? 0 : (int)(grow0 >= b0) + (int)(grow0 >= b1);
    const float *w0 = sel == 0 ? a.w[0] : sel == 1 ? a.w[1] : a.w[2];
    float *out0 = sel == 0 ? a.out[0] : sel == 1 ? a.out[1] : a.out[2];
    const uint32_t obs = sel == 0 ? a.out_bstride[0] : sel == 1 ? a.out_bstride[1] : a.out_bstride[2];
    const uint32_t ops = sel == 0 ? a.out_pstride[0] : sel == 1 ? a.out_pstride[1] : a.out_pstride[2];
    const uint32_t lrow0 = grow0 - (sel == 0 ? 0u : sel == 1 ? b0 : b1);

    float *stg = reinterpret_cast<float *>(smem) + wid * (GF_STAGE_B / 4u);         // this wave's transposition buffer [64][GF_SPITCH]
    float *tab = reinterpret_cast<float *>(smem + a.tab_off);                       // [nmat][NU][16][TP]

    // the tile's 16 rows: one run of 16 * n floats (a segment's rows are a multiple of 16: the tile lies inside one tensor)
    const __amdgpu_buffer_rsrc_t rw0 = mkrsrc(w0 + (size_t)lrow0 * n, GF_RT * n * 4u);
    const __amdgpu_buffer_rsrc_t rw1 = mkrsrc(SW ? a.w[1] + (size_t)lrow0 * n : nullptr, SW ? GF_RT * n * 4u : 0u);
    const __amdgpu_buffer_rsrc_t rx = mkrsrc(a.xs, NT * 16u * NU * GF_UNIT * 4u);

    const uint32_t ln = lane & 15u, lq = lane >> 4;                                 // the MFMA lane: row / token of the tile, k
    // B side of (unit, token tile): this lane's component k of the unit's 32 items for token tt * 16 + ln; tokens >= nb: zeros
    auto load_b = [&](const uint32_t u, const uint32_t tt, float4 (&b)[GF_ITEMS / 4]) __attribute__((always_inline)) {
        const uint32_t off = (tt < NT && tt * 16u + ln < a.nb) ? ((tt * NU + u) * (GF_ITEMS / 4u) * 64u + lane) * 16u : OOB;
#pragma unroll
        for (uint32_t J = 0; J < GF_ITEMS / 4u; J++) b[J] = bload_f4(rx, off == OOB ? OOB : off + J * 1024u);
    };

    for (uint32_t u = wid; u < NU; u += a.nw) {
        // ---- the unit's weights: load i = rows 2 i and 2 i + 1, a row's 128 floats on 32 lanes ----
        float4 ld[nmat][8];
        {
            const uint32_t col = u * GF_UNIT + (lane & 31u) * 4u;
#pragma unroll
            for (uint32_t i = 0; i < 8; i++) {
                const uint32_t off = (col < n) ? ((2u * i + (lane >> 5)) * n + col) * 4u : OOB;
                ld[0][i] = bload_wf(rw0, off);
                if constexpr (SW) ld[1][i] = bload_wf(rw1, off);
            }
        }
        float4 bcur[GF_ITEMS / 4];
        load_b(u, 0u, bcur);
        // ---- 4 x 4 transpose through the wave's LDS buffer: component k of (row m, item j) -> line k * 16 + m; lane l reads line l ----
        float av[nmat][GF_ITEMS];
#pragma unroll
        for (uint32_t mt = 0; mt < nmat; mt++) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();                                        // (the reads of the previous matrix / unit are done)
#pragma unroll
            for (uint32_t i = 0; i < 8; i++) {
                float *d = stg + (2u * i + (lane >> 5)) * GF_SPITCH + (lane & 31u);
                d[0] = ld[mt][i].x; d[16 * GF_SPITCH] = ld[mt][i].y; d[32 * GF_SPITCH] = ld[mt][i].z; d[48 * GF_SPITCH] = ld[mt][i].w;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();                                        // (a wave's LDS queue is in order: the reads below see the writes above)
#pragma unroll
            for (uint32_t J = 0; J < GF_ITEMS / 4u; J++) {
                const float4 v = *reinterpret_cast<const float4 *>(stg + lane * GF_SPITCH + J * 4u);
                av[mt][J * 4 + 0] = v.x; av[mt][J * 4 + 1] = v.y; av[mt][J * 4 + 2] = v.z; av[mt][J * 4 + 3] = v.w;
            }
        }
        // ---- the unit's sums, one token tile at a time; the next tile's activations are asked for first ----
        for (uint32_t tt = 0; tt < NT; tt++) {
            float4 bnxt[GF_ITEMS / 4];
            load_b(u, tt + 1u, bnxt);                                               // (past the last tile: out of range, no traffic)
            float bv[GF_ITEMS];
#pragma unroll
            for (uint32_t J = 0; J < GF_ITEMS / 4u; J++) { bv[J * 4 + 0] = bcur[J].x; bv[J * 4 + 1] = bcur[J].y; bv[J * 4 + 2] = bcur[J].z; bv[J * 4 + 3] = bcur[J].w; }
#pragma unroll
            for (uint32_t mt = 0; mt < nmat; mt++) {
                const v4f s = item_tree<0, (int)GF_ITEMS>(av[mt], bv);
                float *to = tab + ((size_t)(mt * NU + u) * GF_RT + lq * 4u) * TP + tt * 16u + ln;       // s[e] = (row 4 lq + e, token ln)
#pragma unroll
                for (int e = 0; e < 4; e++) to[(uint32_t)e * TP] = s[e];
            }
#pragma unroll
            for (uint32_t J = 0; J < GF_ITEMS / 4u; J++) bcur[J] = bnxt[J];
        }
    }
    __syncthreads();

    // ---- one thread per (row, token): chunk = unit_0 + unit_1, chunks ascending from 0.0f, then the epilogue ----
    const uint32_t nthr = a.nw * 64u;
    for (uint32_t idx = tid; idx < GF_RT * a.nb; idx += nthr) {
        const uint32_t row = idx & 15u, tok = idx >> 4;
        const float *f = tab + (size_t)row * TP + tok;
        float v[nmat];
#pragma unroll
        for (uint32_t mt = 0; mt < nmat; mt++) {
            const float *fm = f + (size_t)mt * NU * GF_RT * TP;
            float acc = 0.0f;
            for (uint32_t u = 0; u < NU; u += 2u) {
                const float h0 = fm[(size_t)u * GF_RT * TP], h1 = (u + 1u < NU) ? fm[(size_t)(u + 1u) * GF_RT * TP] : 0.0f;
                acc += (h0 + h1);
            }
            v[mt] = acc;
        }
        float *o = out0 + (size_t)tok * obs + (ops ? (size_t)a.pos[tok] * ops : 0u) + lrow0 + row;
        const float old = a.epi == GEMV_EPI_RESID ? *o : 0.0f;
        // write-through (agent scope) store, as the GEMV's: nothing is left for the write-back at the end of the kernel
        __hip_atomic_store(o, finish_epi(a.epi, v[0], SW ? v[nmat - 1] : 0.0f, old), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool SW>
hipError_t launch_gemm_f32_t(const GemmF32Dev &d, const F32GemmPlan &p, hipStream_t st) {
    auto kern = &gemm_f32_kernel<SW>;
    if (p.lds_bytes > 64 * 1024) {          // opt-in LDS; gemm_f32_plan() has refused what a CU does not have
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(p.threads), p.lds_bytes, st, d);
    return hipGetLastError();
}

}  // namespace

bool gemm_f32_plan(const GemvArgs &a, F32GemmPlan *p) { return gemm_f32_plan_host(a, p); }

hipError_t launch_gemm_f32(const GemvArgs &a, hipStream_t st) {
    F32GemmPlan p;
    if (!gemm_f32_plan(a, &p) || !a.f32_scratch || a.f32_scratch_floats < p.xs_floats || !a.xin) return hipErrorInvalidValue;
    {   // the prologue: one workgroup per token, on the sliced route's thread count
        GemvArgs pa = a;
        pa.nseg = 0;
        GemvDev g = to_dev(pa);
        g.nthr = p.pro_threads;
        auto kern = &gemm_f32_prologue_kernel;
        if (p.pro_lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.pro_lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(a.nb), dim3(p.pro_threads), p.pro_lds, st, g, a.f32_scratch, p.nu);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const bool sw = p.sw != 0;
    GemmF32Dev d{};
    for (uint32_t s = 0; s < 3; s++) {
        const bool live = s < a.nseg;
        d.w[s] = live ? reinterpret_cast<const float *>(a.seg[s].w) : nullptr;
        d.out[s] = live ? a.seg[s].out : nullptr;
        d.rows[s] = live && !(sw && s > 0) ? a.seg[s].rows : 0u;       // SwiGLU: segment 1 is the second matrix, not more rows
        d.out_bstride[s] = live ? a.seg[s].out_bstride : 0u;
        d.out_pstride[s] = live ? a.seg[s].out_pstride : 0u;
    }
    d.n = a.n; d.epi = a.epi; d.nb = a.nb; d.nt = p.nt; d.nu = p.nu; d.nw = p.nw; d.tp = p.tp; d.tab_off = p.tab_off;
    d.xs = a.f32_scratch; d.pos = a.pos;
    return sw ? launch_gemm_f32_t<true>(d, p, st) : launch_gemm_f32_t<false>(d, p, st);
}

}  // namespace nano
