// gemm_q80_cls.hip -- GC: batched Q80 (W8A8) GEMM for TALL matrices with short rows (the classifier: vocab x n_embd), 2..64
// tokens per weight read, built like the STREAM GEMV of gemv_q80_impl.h: persistent waves sweep the matrix linearly, a wave owns
// whole 16-row tiles (the full row length), so the reference's ascending group order (infer/infer.c:668-674) is a running value
// in its own registers -- no chain between waves, no LDS product table, no barrier after the prologue.
//
//   * the activations (quant_rows_frag_kernel's MFMA B-fragment order, gemm_q80.hip) of the first LT token tiles are staged in
//     LDS ONCE per workgroup and read from there by every wave for every row tile (round 3's GEMM gave each wave its own row tile and lets
//     it fetch the fragments from L2 again: for a 151 936-row classifier that is as many L2 bytes as weight bytes per token
//     tile -- 131 us at 8 tokens and 205..290 us at 64 where the weights alone stream in ~65 us); token tiles that do not fit
//     LDS come from L2 as before;
//   * a wave keeps the next half chunk's 16 x 512 B of weights in flight (registers) while it multiplies the current one out of
//     its transposition buffer (wave-private LDS, pitch 528: conflict-free ds_read_b128 of the MFMA A fragments);
//   * one v_mfma_i32_16x16x64_i8 per (group, token tile) -> exact int32 group sums -> ((float)ival * ws) * xs (infer.c:672) added
//     to the running value of (row, token) in ascending group order: bit-identical to the GEMV path and to the reference.
// Takes: group size 64, one STORE segment of >= 16384 rows, group count a multiple of 8 or 4.  (route.hip routes the classifier
// of batched steps here.)
#include "gemv_common.h"
#include "gemm_q80_host.h"

namespace nano {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

struct GCDev {
    const int8_t *w; const float *ws; float *out;
    uint32_t rows, out_bstride, n, ng, nb, nhc, ntiles, tt, lt, nwaves;     // lt: token tiles staged in LDS
    const int8_t *xf; const float *xsf;
};

// (the LDS sizes GC_*: gemm_q80_host.h)
template <int TT>
__global__ __launch_bounds__(512, 2) void gemm_q80_cls_kernel(const GCDev a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    karg_touch(a.out); karg_touch(a.out_bstride); karg_touch(a.rows); karg_touch(a.xf); karg_touch(a.xsf);      // (late-read arguments with the first batch)
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t n = a.n, ng = a.ng, nhc = a.nhc, tt = a.tt, lt = a.lt;
    const uint32_t m = lane & 15u, kq = lane >> 4;

    // LDS: xfl[lt][ng][1024] int8 | xsl[lt][ng][16] float | per wave: wbuf[16][528] int8, wsl[8][16] float
    int8_t *xfl = reinterpret_cast<int8_t *>(smem);
    float *xsl = reinterpret_cast<float *>(smem + (size_t)lt * ng * 1024u);
    int8_t *wbuf = reinterpret_cast<int8_t *>(smem) + (size_t)lt * ng * (1024u + 64u) + (size_t)wid * GC_LDS_WAVE;
    float *wsl = reinterpret_cast<float *>(wbuf + GC_WBUF);

    const __amdgpu_buffer_rsrc_t rw = mkrsrc(a.w, a.rows * n);
    const __amdgpu_buffer_rsrc_t rs = mkrsrc(a.ws, a.rows * ng * 4u);
    const __amdgpu_buffer_rsrc_t rxf = mkrsrc(a.xf, tt * ng * 1024u);
    const __amdgpu_buffer_rsrc_t rxs = mkrsrc(a.xsf, tt * ng * 64u);

    // this wave's tiles: wave_g, wave_g + nwaves, ... -- the chip sweeps the matrix linearly
    const uint32_t wave_g = blockIdx.x * nw + wid;
    const uint32_t my_tiles = wave_g < a.ntiles ? (a.ntiles - wave_g + a.nwaves - 1u) / a.nwaves : 0u;
    const uint32_t units = my_tiles * nhc;                              // (tile, half chunk), half chunk fastest

    // ---- weight pieces of a unit: 16 rows x 512 B, two rows per load instruction (lane l: row 2r + l/32) -----------------------
    int4 wA[8];
    const uint32_t wrow = lane >> 5, wcol = (lane & 31u) * 16u;
    uint32_t it = 0, ih = 0;                                            // cursor of the NEXT unit to issue
    auto issue_w = [&]() {
        const uint32_t row0 = (wave_g + it * a.nwaves) * 16u;
        const uint32_t col = ih * 512u + wcol;
        const uint32_t base = (it < my_tiles && col < n) ? (row0 + wrow) * n + col : OOB;       // rows beyond the matrix: out of range -> 0
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(base == OOB ? OOB : base + (uint32_t)(2 * r) * n), 0, 2);
            wA[r] = make_int4(v.x, v.y, v.z, v.w);
        }
        if (++ih == nhc) { ih = 0; it++; }
    };
    issue_w();

    // ---- prologue: the first lt token tiles' fragments and scales into LDS (every wave reads them for every tile) ---------------
    {
        const uint32_t nvec = lt * ng * 64u;                            // 16-byte pieces
        for (uint32_t i = tid; i < nvec; i += blockDim.x) {
            const i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rxf, (int)(i * 16u), 0, 0);
            *reinterpret_cast<i32x4 *>(xfl + (size_t)i * 16u) = v;
        }
        const uint32_t nsc = lt * ng * 4u;                              // float4 pieces of the scales
        for (uint32_t i = tid; i < nsc; i += blockDim.x) *reinterpret_cast<float4 *>(xsl + (size_t)i * 4u) = bload_f4(rxs, i * 16u);
    }
    __syncthreads();                                                   // the only barrier

    float acc[TT][4];
    uint32_t ct = 0, ch = 0;                                            // cursor of the unit being consumed
    for (uint32_t u = 0; u < units; u++) {
        const uint32_t row0 = (wave_g + ct * a.nwaves) * 16u, g0 = ch * 8u;
        if (ch == 0) {
#pragma unroll
            for (int t = 0; t < TT; t++) { acc[t][0] = 0.f; acc[t][1] = 0.f; acc[t][2] = 0.f; acc[t][3] = 0.f; }
        }
        // 1. the unit's weight pieces: registers -> the transposition buffer; its scales (lanes 0..31: row l/2, groups g0 + 4 (l%2) .. +3)
#pragma unroll
        for (int r = 0; r < 8; r++) *reinterpret_cast<int4 *>(wbuf + (size_t)(2 * r + wrow) * GC_PITCH + wcol) = wA[r];
        const uint32_t sg = g0 + (lane & 1u) * 4u;
        const float4 wsv = bload_f4(rs, (lane < 32u && sg < ng) ? ((row0 + (lane >> 1)) * ng + sg) * 4u : OOB);     // rows beyond the matrix: 0
        // 2. fragments of the token tiles that are not staged (tiles >= lt), all of this half chunk at once
        i32x4 fbg[TT > 2 ? 2 : 1][8]; float xsg[TT > 2 ? 2 : 1][8];
        if constexpr (TT > 2) if (lt < tt) {                           // (uniform: nothing to fetch when every tile is staged)
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const uint32_t t = lt + (uint32_t)e;
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) {
                    fbg[e][j] = __builtin_amdgcn_raw_buffer_load_b128(rxf, (int)((g0 + j < ng && t < tt) ? lane * 16u : OOB), (int)((t * ng + g0 + j) * 1024u), 0);
                    xsg[e][j] = bload_f(rxs, (g0 + j < ng && t < tt) ? ((t * ng + g0 + j) * 16u + m) * 4u : OOB);
                }
            }
        }
        issue_w();                                                      // the next unit's weights (behind the fragments in the load queue)
        if (lane < 32u) {
            const uint32_t r = lane >> 1, gq = (lane & 1u) * 4u;
            wsl[(gq + 0u) * 16u + r] = wsv.x; wsl[(gq + 1u) * 16u + r] = wsv.y; wsl[(gq + 2u) * 16u + r] = wsv.z; wsl[(gq + 3u) * 16u + r] = wsv.w;
        }
        // 3. 8 groups x token tiles: A fragment from the transposition buffer, B fragment from LDS (staged) or registers, MFMA,
        //    product, running value += in ascending group order (infer.c:668-674)
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            if (g0 + j < ng) {                                          // (uniform; the last half chunk may hold 4 groups)
                const i32x4 fa = *reinterpret_cast<const i32x4 *>(wbuf + (size_t)m * GC_PITCH + j * 64u + kq * 16u);
                const float4 wv = *reinterpret_cast<const float4 *>(wsl + j * 16u + kq * 4u);
#pragma unroll
                for (int t = 0; t < TT; t++) {
                    if ((uint32_t)t < tt) {
                        i32x4 fb; float xsc;
                        if ((uint32_t)t < lt) {
                            fb = *reinterpret_cast<const i32x4 *>(xfl + ((size_t)((uint32_t)t * ng + g0 + j) * 64u + lane) * 16u);
                            xsc = xsl[((uint32_t)t * ng + g0 + j) * 16u + m];
                        } else if constexpr (TT > 2) {
                            fb = fbg[(t - 2) & 1][j]; xsc = xsg[(t - 2) & 1][j];       // (lt == 2 whenever tiles stay unstaged)
                        } else { fb = i32x4{0, 0, 0, 0}; xsc = 0.0f; }
                        const v4i cv = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa, fb, v4i{0, 0, 0, 0}, 0, 0, 0);
                        acc[t][0] += ((float)cv[0] * wv.x) * xsc; acc[t][1] += ((float)cv[1] * wv.y) * xsc;       // infer.c:672
                        acc[t][2] += ((float)cv[2] * wv.z) * xsc; acc[t][3] += ((float)cv[3] * wv.w) * xsc;
                    }
                }
            }
        }
        // 4. after the tile's last half chunk: store the 16 rows x 16 tokens of every token tile
        if (ch + 1u == nhc) {
#pragma unroll
            for (int t = 0; t < TT; t++) {
                const uint32_t tok = (uint32_t)t * 16u + m, row = row0 + kq * 4u;
                if ((uint32_t)t < tt && tok < a.nb) {
                    float *o = a.out + (size_t)tok * a.out_bstride + row;
                    if (row + 3u < a.rows) *reinterpret_cast<float4 *>(o) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
                    else {
#pragma unroll
                        for (int i = 0; i < 4; i++) if (row + i < a.rows) o[i] = acc[t][i];
                    }
                }
            }
        }
        if (++ch == nhc) { ch = 0; ct++; }
    }
}

template <int TT>
static void launch_gc_tt(const GCDev &d, const Q80GemmPlan &p, hipStream_t st) {
    constexpr auto kern = &gemm_q80_cls_kernel<TT>;
    q80_gemm_lds_limit_once<kern>();
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(p.threads), p.lds_bytes, st, d);
}

}  // namespace

// every choice is the plan's (q80_gemm_plan_gc(), gemm_q80_host.h)
hipError_t launch_gemm_q80_cls(const GemvArgs &a, const Q80GemmPlan &p, hipStream_t st) {
    GCDev d{};
    d.w = reinterpret_cast<const int8_t *>(a.seg[0].w); d.ws = a.seg[0].ws; d.out = a.seg[0].out;
    d.rows = a.seg[0].rows; d.out_bstride = a.seg[0].out_bstride;
    d.n = a.n; d.ng = p.ng; d.nb = a.nb; d.nhc = p.nhc;
    d.ntiles = p.ntiles; d.tt = p.ttl; d.lt = p.lt; d.nwaves = p.nwaves;
    d.xf = a.xq_in; d.xsf = a.xs_in;
    if (p.tt == 1u) launch_gc_tt<1>(d, p, st);
    else if (p.tt == 2u) launch_gc_tt<2>(d, p, st);
    else launch_gc_tt<4>(d, p, st);
    return hipGetLastError();
}

}  // namespace nano
