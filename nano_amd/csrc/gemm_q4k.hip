// gemm_q4k.hip -- Q4K (W4A4) skinny GEMM on the int8 matrix cores for 9..64 tokens per weight read (large decode batches, 64-token
// prefill chunks): what gemm_q80.hip is for Q80.  out[t][r] = matmul_q4k(W[r,:], x_t) for every token t, BIT-IDENTICAL to the per-token
// reference (infer/tensor.c:359-434 dot_two_blocks_q4k, 438-471 matmul_q4k) and therefore to the chunk GEMV (gemv_q4k_chunk.hip):
//
//   * a Q4K group is 32 values, which is the K of v_mfma_i32_16x16x32_i8: ONE MFMA with C = 0 returns the exact sum_pq of a 16-row x
//     16-token tile for one group.  Nibbles go in as bytes 0..15; the order of k inside a group is free as long as both operands use
//     the same one, so a packed dword w becomes the two operand dwords w & 0x0f0f0f0f and (w >> 4) & 0x0f0f0f0f -- lane (m | n, kq) takes
//     dword kq of its row's / token's 16 packed bytes, no interleave.  Lane map: gemm_q80.hip's header (A[m = l % 16][k = 8 (l / 16) ..],
//     B[k = same][n = l % 16], c[i] = C[m = 4 (l / 16) + i][n = l % 16]).
//   * everything after the integer sum is the chunk kernel's VALU expression (gemv_q4k_chunk_body.inc post_a), the same association, no
//     contraction: sp * sq * (float)sum_pq - sp * bq * (float)sum_p - sq * bp * (float)sum_q + 32 * bp * bq.  sp, bp and sum_p depend on
//     (row, group) only: computed ONCE per row tile and stage as the chunk kernel's `pre` does (q4k_unpack6, v_dot8_u32_u4 against
//     eight ones) and parked in LDS; sq, bq and sum_q come with the staged activation groups (XGroup) of q4k_quant_rows_kernel --
//     the quantizer launch of the 2..8-sequence chunk launches, one workgroup per token, the trees of that token's one-sequence launch.
//   * float order: the 8 group values of a block are added in order into a sum that starts at 0 (in registers: a lane owns its four
//     (row, token) results of a tile); the block sums of a row are added in ascending block order.  K is divided between the waves of a
//     workgroup at BLOCK granularity only: block sums go to an LDS table [block][row][token] and one thread per (row, token) adds them
//     in ascending order into its line.  The table holds one stage (GQ_KB blocks) at a time -- the row is walked in rounds.
//
// Data flow.  A workgroup = 4 waves = one 16-row tile (the W1 and the W3 tile of the same rows for SwiGLU) x all tokens; its rows are ONE
// contiguous run of 160-byte blocks.  A stage = GQ_KB blocks of each of the 16 rows: 16-byte loads, a lane's chunks consecutive inside a
// row, asked for a whole stage ahead (they stay in flight while the previous stage is multiplied), parked in LDS as [chunk][row] with a
// chunk pitch of 272 bytes: the 16-byte stores of eight consecutive chunks fall on different banks, and the A operand read of group g
// (lane l: row l % 16, dword l / 16) is one 256-byte line.  Work item (matrix, block of the stage, token tile) -> wave, round-robin; the
// item's B operands and (sq, bq, sum_q) are read straight from the staged groups in L2 (token l % 16 of the tile: the B lane and the
// result lane are the same token), one item ahead.  Token columns >= nb are computed on zeros and never stored.  No waits between
// workgroups, no give-up path.
#include "gemv_q4k_impl.h"

namespace nano {

bool q4k_quant_rows_supports(const GemvArgs &a);                       // gemv_q4k_chunk.hip
hipError_t launch_q4k_quant_rows(const GemvArgs &a, hipStream_t st);

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr uint32_t GQ_KB = 4;                              // blocks of a stage
constexpr uint32_t GQ_CH = GQ_KB * 10u;                    // 16-byte chunks of a row per stage
constexpr uint32_t GQ_PITCH = 272;                         // bytes between chunks in LDS: 16 rows x 16 bytes + 16
constexpr uint32_t GQ_STAGE_B = GQ_CH * GQ_PITCH;          // one matrix's stage
constexpr uint32_t GQ_PRE_F = GQ_KB * 8u * 3u * 16u;       // floats: [block][group][sp | bp | sum_p][row]
constexpr uint32_t GQ_NTHR = 256, GQ_NW = 4;
constexpr uint32_t GQ_LPT = (16u * GQ_CH + GQ_NTHR - 1u) / GQ_NTHR;    // chunks per thread and stage

struct GemmQ4kDev {
    const uint8_t *w[3]; float *out[3];
    uint32_t rows[3], out_bstride[3], out_pstride[3];
    uint32_t n, epi, nb, nt;                               // nt: token tiles of 16
    const uint8_t *xg; const uint32_t *pos;
};

__device__ __forceinline__ long nib_operand(uint32_t w) {
    return (long)(((unsigned long)((w >> 4) & 0x0f0f0f0fu) << 32) | (unsigned long)(w & 0x0f0f0f0fu));
}

// the B side of a work item: token l % 16 of the tile, the 8 groups of the block
struct BItem { uint32_t pk[8]; uint4 meta[8]; };           // meta = (sq, bq, sum_q, -)

template <bool SW>
__global__ __launch_bounds__(256) void gemm_q4k_kernel(const GemmQ4kDev a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t nmat = SW ? 2u : 1u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t n = a.n, bpl = n >> 8, GT = bpl * 8u, NT = a.nt, P = NT * 16u + 4u;       // P: pitch of a table row (tokens + 4: the four row quads of a tile on different banks)
    const uint32_t b0 = a.rows[0], b1 = b0 + a.rows[1];
    const uint32_t grow0 = blockIdx.x * 16u;
    const int sel = SW ? 0 : (int)(grow0 >= b0) + (int)(grow0 >= b1);
    const uint8_t *w0 = sel == 0 ? a.w[0] : sel == 1 ? a.w[1] : a.w[2];
    float *out0 = sel == 0 ? a.out[0] : sel == 1 ? a.out[1] : a.out[2];
    const uint32_t obs = sel == 0 ? a.out_bstride[0] : sel == 1 ? a.out_bstride[1] : a.out_bstride[2];
    const uint32_t ops = sel == 0 ? a.out_pstride[0] : sel == 1 ? a.out_pstride[1] : a.out_pstride[2];
    const uint32_t lrow0 = grow0 - (sel == 0 ? 0u : sel == 1 ? b0 : b1);

    // LDS: stage[nmat][GQ_CH][272] | pre[nmat][GQ_KB][8][3][16] | tab[nmat][GQ_KB][16][P]
    unsigned char *stage = smem;
    float *pre = reinterpret_cast<float *>(smem + nmat * GQ_STAGE_B);
    float *tab = pre + nmat * GQ_PRE_F;

    const size_t run0 = (size_t)lrow0 * bpl * 160u;                    // the tile's 16 rows: one run of 16 * bpl blocks
    const uint32_t run_b = 16u * bpl * 160u;
    const __amdgpu_buffer_rsrc_t rw0 = mkrsrc(w0 + run0, run_b);
    const __amdgpu_buffer_rsrc_t rw1 = mkrsrc(SW ? a.w[1] + run0 : nullptr, SW ? run_b : 0u);
    const __amdgpu_buffer_rsrc_t rx = mkrsrc(a.xg, a.nb * GT * 32u);   // (tokens >= nb: out of range, zeros)

    // this thread's chunks of a stage: chunk q = tid + 256 k of 16 rows x GQ_CH -> row q / GQ_CH, chunk j = q % GQ_CH of the row
    uint32_t lj[GQ_LPT], lgo[GQ_LPT], lso[GQ_LPT];
#pragma unroll
    for (uint32_t k = 0; k < GQ_LPT; k++) {
        const uint32_t q = tid + k * GQ_NTHR, m = q / GQ_CH, j = q - m * GQ_CH;
        const bool live = q < 16u * GQ_CH;
        lj[k] = live ? j : 0xffffu;                                    // (dead: beyond every row)
        lgo[k] = m * bpl * 160u + j * 16u;
        lso[k] = j * GQ_PITCH + m * 16u;
    }
    uint4 ring[nmat][GQ_LPT];
    auto issue = [&](const uint32_t s) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t k = 0; k < GQ_LPT; k++) {
            const uint32_t off = (s * GQ_CH + lj[k] < bpl * 10u) ? lgo[k] + s * (GQ_CH * 16u) : OOB;
            ring[0][k] = bload_u4(rw0, off, true);
            if constexpr (SW) ring[1][k] = bload_u4(rw1, off, true);
        }
    };
    const uint32_t S = (bpl + GQ_KB - 1u) / GQ_KB;
    issue(0);

    // the fold threads: thread -> row tid % 16, tokens tid / 16 + 16 k (k < NT)
    const uint32_t frow = tid & 15u, ftok = tid >> 4;
    float line[nmat][4];
#pragma unroll
    for (uint32_t mt = 0; mt < nmat; mt++)
#pragma unroll
        for (int k = 0; k < 4; k++) line[mt][k] = 0.0f;

    const uint32_t ln = lane & 15u, lq = lane >> 4;                    // the MFMA lane: row / token of the tile, quarter of K
    auto load_b = [&](const uint32_t s, const uint32_t kbv, const uint32_t i, const uint32_t items, BItem &b) __attribute__((always_inline)) {
        const uint32_t tt = i % NT, blk = (i / NT) % kbv, tok = tt * 16u + ln;
        const uint32_t off = (i < items && tok < a.nb) ? (tok * GT + (s * GQ_KB + blk) * 8u) * 32u : OOB;
#pragma unroll
        for (int g = 0; g < 8; g++) {
            b.pk[g] = __builtin_amdgcn_raw_buffer_load_b32(rx, (int)(off + (uint32_t)g * 32u + lq * 4u), 0, 0);
            const i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(off + (uint32_t)g * 32u + 16u), 0, 0);
            b.meta[g] = make_uint4((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w);
        }
    };

    for (uint32_t s = 0; s < S; s++) {
        const uint32_t kbv = bpl - s * GQ_KB < GQ_KB ? bpl - s * GQ_KB : GQ_KB;     // blocks of this stage
        const uint32_t items = nmat * kbv * NT;
        // the B side of this wave's first item is asked for before the stage is parked
        BItem cur;
        load_b(s, kbv, wid, items, cur);
        // ---- park the stage (every wave is done with the previous one: the barrier after its multiply), ask for the next ----
#pragma unroll
        for (uint32_t k = 0; k < GQ_LPT; k++) {
            if (lj[k] != 0xffffu) {
                *reinterpret_cast<uint4 *>(stage + lso[k]) = ring[0][k];
                if constexpr (SW) *reinterpret_cast<uint4 *>(stage + GQ_STAGE_B + lso[k]) = ring[1][k];
            }
        }
        issue(s + 1u);                                                 // (past the end: out of range, no traffic)
        __syncthreads();
        // ---- the weight-only half, once per (matrix, block, group, row): sp, bp, sum_p ----
        for (uint32_t it = tid; it < nmat * GQ_KB * 128u; it += GQ_NTHR) {
            const uint32_t row = it & 15u, g = (it >> 4) & 7u, blk = (it >> 7) & 3u, mt = it >> 9;
            const unsigned char *sb = stage + mt * GQ_STAGE_B + blk * 10u * GQ_PITCH + row * 16u;
            const float s_scale = *reinterpret_cast<const float *>(sb + 12);
            const uint4 h = *reinterpret_cast<const uint4 *>(sb + GQ_PITCH);          // s_bias and the 12 packed 6-bit bytes
            const uint4 v = *reinterpret_cast<const uint4 *>(sb + (2u + g) * GQ_PITCH);
            uint32_t s6, b6;
            q4k_unpack6(h.y, h.z, h.w, (int)g, s6, b6);
            const uint32_t wn[4] = { v.x, v.y, v.z, v.w };
            uint32_t sump = 0;
#pragma unroll
            for (int m = 0; m < 4; m++) sump = __builtin_amdgcn_udot8(wn[m], 0x11111111u, sump, false);
            float *po = pre + mt * GQ_PRE_F + (blk * 8u + g) * 48u + row;
            po[0] = (float)s6 * s_scale; po[16] = (float)b6 * __uint_as_float(h.x); po[32] = (float)(int)sump;
        }
        __syncthreads();
        // ---- the multiply: item (matrix, block, token tile) -> block sums of a 16 x 16 tile ----
        for (uint32_t i = wid; i < items; i += GQ_NW) {
            BItem nxt;
            load_b(s, kbv, i + GQ_NW, items, nxt);
            const uint32_t tt = i % NT, r = i / NT, blk = r % kbv, mt = r / kbv;
            const unsigned char *sa = stage + mt * GQ_STAGE_B + (blk * 10u + 2u) * GQ_PITCH + ln * 16u + lq * 4u;
            const float *pr = pre + mt * GQ_PRE_F + blk * 8u * 48u + lq * 4u;
            float dot[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int g = 0; g < 8; g++) {
                const uint32_t wa = *reinterpret_cast<const uint32_t *>(sa + (uint32_t)g * GQ_PITCH);
                const v4i c = __builtin_amdgcn_mfma_i32_16x16x32_i8(nib_operand(wa), nib_operand(cur.pk[g]), v4i{0, 0, 0, 0}, 0, 0, 0);
                const float4 sp4 = *reinterpret_cast<const float4 *>(pr + g * 48), bp4 = *reinterpret_cast<const float4 *>(pr + g * 48 + 16),
                             su4 = *reinterpret_cast<const float4 *>(pr + g * 48 + 32);
                const float spv[4] = { sp4.x, sp4.y, sp4.z, sp4.w }, bpv[4] = { bp4.x, bp4.y, bp4.z, bp4.w }, suv[4] = { su4.x, su4.y, su4.z, su4.w };
                const float sq = __uint_as_float(cur.meta[g].x), bq = __uint_as_float(cur.meta[g].y);
                const int sumq = (int)cur.meta[g].z;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float sp = spv[e], bp = bpv[e], su = suv[e];
                    // reference tensor.c:425-428, the association of gemv_q4k_chunk_body.inc post_a
                    dot[e] += sp * sq * (float)c[e] - sp * bq * su - sq * bp * (float)sumq + 32 * bp * bq;
                }
            }
            float *to = tab + ((mt * GQ_KB + blk) * 16u + lq * 4u) * P + tt * 16u + ln;
#pragma unroll
            for (int e = 0; e < 4; e++) to[(uint32_t)e * P] = dot[e];
            cur = nxt;
        }
        __syncthreads();
        // ---- one thread per (row, token): the stage's blocks in ascending order (tensor.c:438-471) ----
#pragma unroll
        for (uint32_t mt = 0; mt < nmat; mt++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if ((uint32_t)k < NT) {
                    const float *f = tab + (mt * GQ_KB * 16u + frow) * P + ftok + (uint32_t)k * 16u;
                    float l = line[mt][k];
                    for (uint32_t blk = 0; blk < kbv; blk++) l += f[blk * 16u * P];
                    line[mt][k] = l;
                }
            }
        // (the next stage's multiply writes the table after two more barriers; its park overwrites a stage every wave has left)
    }

    // ---- epilogue: store | residual add | SwiGLU; tokens >= nb are never stored ----
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t tok = ftok + (uint32_t)k * 16u;
        if ((uint32_t)k < NT && tok < a.nb) {
            float *o = out0 + (size_t)tok * obs + (ops ? (size_t)a.pos[tok] * ops : 0u) + lrow0 + frow;
            const float old = a.epi == GEMV_EPI_RESID ? *o : 0.0f;
            *o = finish_epi(a.epi, line[0][k], SW ? line[nmat - 1][k] : 0.0f, old);
        }
    }
}

}  // namespace

// shapes / features the GEMM takes (host predicate; pointers are read as flags only)
bool gemm_q4k_supports(const GemvArgs &a) {
    if (a.nb < 9 || a.nb > 64 || a.n == 0 || (a.n & 255u) || a.n > 16384u || a.nseg == 0 || a.nseg > 3) return false;
    if (a.resid_add || a.x4_in || a.xq_in || a.tile_max) return false;
    if (a.epi > GEMV_EPI_SWIGLU) return false;
    if (a.epi == GEMV_EPI_SWIGLU && (a.nseg != 2 || a.seg[0].rows != a.seg[1].rows || a.seg[0].out_pstride)) return false;
    if (a.epi == GEMV_EPI_RESID && a.seg[0].out_pstride) return false;          // (the residual stream is never position indexed)
    for (uint32_t s = 0; s < a.nseg; s++) if (a.seg[s].rows == 0 || a.seg[s].rows % 16u) return false;
    return q4k_quant_rows_supports(a);           // the quantizer launch: rmsnorm / split-attention combine exactly where the chunk launch takes them
}

hipError_t launch_gemm_q4k(const GemvArgs &a, hipStream_t st) {
    if (!gemm_q4k_supports(a)) return hipErrorInvalidValue;
    {
        const hipError_t e = launch_q4k_quant_rows(a, st);            // (refuses a missing or short scratch)
        if (e != hipSuccess) return e;
    }
    const bool sw = a.epi == GEMV_EPI_SWIGLU;
    GemmQ4kDev d{};
    uint32_t rows = 0;
    for (uint32_t s = 0; s < 3; s++) {
        const bool live = s < a.nseg;
        d.w[s] = live ? reinterpret_cast<const uint8_t *>(a.seg[s].w) : nullptr;
        d.out[s] = live ? a.seg[s].out : nullptr;
        d.rows[s] = live && !(sw && s > 0) ? a.seg[s].rows : 0u;       // SwiGLU: segment 1 is the second matrix, not more rows
        d.out_bstride[s] = live ? a.seg[s].out_bstride : 0u;
        d.out_pstride[s] = live ? a.seg[s].out_pstride : 0u;
        rows += d.rows[s];
    }
    d.n = a.n; d.epi = a.epi; d.nb = a.nb; d.nt = (a.nb + 15u) / 16u;
    d.xg = a.q4_scratch; d.pos = a.pos;
    const uint32_t nmat = sw ? 2u : 1u;
    const size_t lds = (size_t)nmat * (GQ_STAGE_B + (GQ_PRE_F + GQ_KB * 16u * (d.nt * 16u + 4u)) * 4u);
    if (sw) {
        auto kern = &gemm_q4k_kernel<true>;
        if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(rows / 16u), dim3(GQ_NTHR), lds, st, d);
    } else {
        auto kern = &gemm_q4k_kernel<false>;
        hipLaunchKernelGGL(kern, dim3(rows / 16u), dim3(GQ_NTHR), lds, st, d);
    }
    return hipGetLastError();
}

}  // namespace nano
