// score.hip -- row statistics of logits[rows][V] for given targets: one NanoHipTokenScore (include/nano_mi355x.h) per row, so that a
// prefill chunk's logits (39 MB at 64 rows of Qwen3's vocabulary) are reduced to 24 bytes per row on the device.
//
// The reduction shape depends on V only -- not on the number of rows, the row's index, the alignment of the row or the launch that
// produced the logits -- so a position's six words are the same bits however a prompt was cut into calls and chunks:
//   * a row is cut into tiles of SCORE_TILE = 4096 consecutive logits; tile t of row r is workgroup (t, r) of launch 1 (256 threads);
//   * thread i of a tile holds the 16 logits 4 i + k + 1024 j (j = 0..3 outer, k = 0..3 inner): ONE pass over memory, the values stay
//     in registers.  A 16-byte aligned full quad is one dwordx4 load, any other quad (rows of an odd V, the row's tail) four dword
//     loads of the same elements: the arithmetic below does not know which;
//   * tile maximum m_t (first index: larger value, equal values -> smaller index), then s_t = sum of expf(l - m_t): per thread over its
//     16 values in (j, k) order, the 64 lanes of a wave by the xor butterfly 32, 16, .. 1, the 4 waves added in ascending order;
//     c_t = #{j in tile : l_j > l_target} + #{j in tile, j < target : l_j == l_target};
//   * launch 2, one wave per row: M = the maximum of the m_t (first tile that holds it -> arg-max), then
//     S = sum over t ASCENDING of s_t * expf(m_t - M), added by one lane; lse = M + logf(S); rank = sum of the c_t.
// -inf logits: expf(-inf - m) = 0; a tile that holds nothing else has m_t = -inf and s_t = 0 (no -inf - -inf is formed), and
// expf(-inf - M) = 0 drops it from S.  Rows with NaN or +inf, and rows of -inf only, are unspecified.
// The partials travel through global memory between the two launches: a kernel boundary is the grid-wide dependency, no counter and no
// atomic.  The classifier kernels and their tile_max partials are not involved.
#include "device_common.h"
#include "kernels.h"

namespace nano {

namespace {
constexpr uint32_t SCORE_THREADS = 256, SCORE_QUADS = SCORE_TILE / (4 * SCORE_THREADS);      // 4 quads of 4 logits per thread
static_assert(SCORE_QUADS * 4 * SCORE_THREADS == SCORE_TILE, "a tile is a whole number of quads per thread");

// (value, index): the larger value wins, equal values -> the smaller index: the first maximum in index order whatever the visiting order
__device__ __forceinline__ void take_max(float &best, uint32_t &bi, float v, uint32_t i) {
    if (i != 0xffffffffu && (bi == 0xffffffffu || v > best || (v == best && i < bi))) { best = v; bi = i; }
}
}  // namespace

// (A two-pass form -- the row maximum first, then a second read of the cache-resident row for sum of expf(l - M), four launches -- was
// built and measured: 26.8 us against this form's 18.1 us at 64 x 151 936; profiles/prefill_score.txt, profiles/score_two_pass_dropped.patch.)
__global__ __launch_bounds__(SCORE_THREADS) void score_tiles_kernel(const ScoreArgs a) {
    __shared__ float s_val[4];
    __shared__ uint32_t s_idx[4], s_cnt[4];
    __shared__ float s_sum[4];
    const uint32_t tile = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const float *row = a.logits + (size_t)r * a.V;
    const uint32_t base = tile * SCORE_TILE;
    const uint32_t n = a.V - base < SCORE_TILE ? a.V - base : SCORE_TILE;           // logits of this tile (>= 1)
    const bool aligned = ((reinterpret_cast<uintptr_t>(row + base)) & 15u) == 0;
    const bool counted = a.targets != nullptr;
    const uint32_t tgt = counted ? a.targets[r] : 0u;
    const float tl = counted ? row[tgt] : 0.0f;

    float v[SCORE_QUADS * 4];
#pragma unroll
    for (uint32_t j = 0; j < SCORE_QUADS; j++) {
        const uint32_t e = 4u * tid + j * 4u * SCORE_THREADS;                       // first logit of the quad, inside the tile
        if (aligned && e + 3u < n) {
            const float4 q = *reinterpret_cast<const float4 *>(row + base + e);
            v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) v[4 * j + k] = e + k < n ? row[base + e + k] : -INFINITY;
        }
    }
    float best = -INFINITY;
    uint32_t bi = 0xffffffffu, cnt = 0;
#pragma unroll
    for (uint32_t j = 0; j < SCORE_QUADS; j++)
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t e = 4u * tid + j * 4u * SCORE_THREADS + k;
            if (e < n) {
                const float x = v[4 * j + k];
                if (bi == 0xffffffffu || x > best) { best = x; bi = base + e; }          // ascending indices inside a thread: strict '>'
                if (counted && (x > tl || (x == tl && base + e < tgt))) cnt++;
            }
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const uint32_t oi = __shfl_xor(bi, o, 64);
        take_max(best, bi, ov, oi);
        cnt += __shfl_xor(cnt, o, 64);
    }
    if (lane == 0) { s_val[wid] = best; s_idx[wid] = bi; s_cnt[wid] = cnt; }
    __syncthreads();
    best = s_val[0]; bi = s_idx[0]; cnt = s_cnt[0];
#pragma unroll
    for (uint32_t w = 1; w < 4; w++) { take_max(best, bi, s_val[w], s_idx[w]); cnt += s_cnt[w]; }
    const float m = best;
    float s = 0.0f;
    if (m != -INFINITY) {
#pragma unroll
        for (uint32_t i = 0; i < SCORE_QUADS * 4; i++) s += expf(v[i] - m);         // (padding and -inf logits: expf(-inf) = 0)
    }
    s = wave_sum(s);
    if (lane == 0) s_sum[wid] = s;
    __syncthreads();
    if (tid == 0) {
        ScorePartial p;
        p.m = best; p.s = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3]; p.idx = bi; p.cnt = cnt;
        a.part[(size_t)r * a.ntiles + tile] = p;
    }
}

__global__ __launch_bounds__(64) void score_combine_kernel(const ScoreArgs a) {
    __shared__ float s_e[64];
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const ScorePartial *part = a.part + (size_t)r * a.ntiles;
    float best = -INFINITY;
    uint32_t bi = 0xffffffffu, cnt = 0;
    for (uint32_t t = lane; t < a.ntiles; t += 64u) { take_max(best, bi, part[t].m, part[t].idx); cnt += part[t].cnt; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const uint32_t oi = __shfl_xor(bi, o, 64);
        take_max(best, bi, ov, oi);
        cnt += __shfl_xor(cnt, o, 64);
    }
    const float M = best;
    float S = 0.0f;
    for (uint32_t t0 = 0; t0 < a.ntiles; t0 += 64u) {                               // tiles in ascending order, 64 factors at a time
        const uint32_t t = t0 + lane;
        s_e[lane] = t < a.ntiles ? part[t].s * expf(part[t].m - M) : 0.0f;
        __syncthreads();
        if (lane == 0) { const uint32_t k = a.ntiles - t0 < 64u ? a.ntiles - t0 : 64u; for (uint32_t i = 0; i < k; i++) S += s_e[i]; }
        __syncthreads();
    }
    if (lane == 0) {
        const float *row = a.logits + (size_t)r * a.V;
        NanoHipTokenScore o;
        o.max_logit = M;
        o.lse = M + logf(S);
        o.argmax = bi == 0xffffffffu ? 0u : bi;
        o.target_logit = a.targets ? row[a.targets[r]] : M;                         // no targets: the row's own arg-max
        o.rank = a.targets ? cnt : 0u;
        o.logprob = o.target_logit - o.lse;
        a.out[r] = o;
    }
}

uint32_t score_tiles(uint32_t V) { return (V + SCORE_TILE - 1) / SCORE_TILE; }

hipError_t launch_score_rows(const ScoreArgs &a, uint32_t rows, hipStream_t st) {
    if (!rows) return hipSuccess;
    if (!a.V || a.ntiles != score_tiles(a.V) || !a.logits || !a.part || !a.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_tiles_kernel, dim3(a.ntiles, rows), dim3(SCORE_THREADS), 0, st, a);
    hipLaunchKernelGGL(score_combine_kernel, dim3(rows), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace nano
