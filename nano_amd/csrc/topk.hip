// topk.hip -- the k most probable tokens of every row of logits[rows][V], with their log-probs: k NanoHipTopEntry
// (include/nano_mi355x.h) per row, 1 <= k <= NANO_TOPK_MAX.  Runs behind score.hip's two launches on the same stream and takes the
// row's lse from the NanoHipTokenScore they wrote.
//
// The selection is exact -- a total order on (logit, index), no tolerance -- so a row's entries are the same bits whatever the row's
// index or alignment, the number of rows or the launch that produced the logits:
//   * a logit travels as a 64-bit key (ord(logit) << 32) | (0xffffffff - index).  ord is the sign-flip map of the float's bits
//     (negative: ~bits, else bits | 0x80000000) with -0.0f taken as +0.0f, compared as an integer: denormals order by value whatever
//     the float mode, -inf is a key like any other, equal floats order by index, and the LARGEST key is the first entry.  Keys of one
//     row are distinct, and none is 0 (ord(-inf) = 0x007fffff is the smallest of a row without NaN): 0 marks "no candidate";
//   * launch 1, topk_tiles_kernel, grid (score_tiles(V), rows) x 256 threads: tile t of row r is the 4096 logits of score.hip's
//     tile, thread i holds the same 16 of them (one dwordx4 load per aligned full quad, else four dword loads), ONE pass over memory.
//     The tile's best min(k, n_tile) keys go, in order, to part[row][tile][0..k) (the rest of the k slots: 0);
//   * launch 2, topk_merge_kernel, one workgroup per row: the best k of the tiles' lists (63 lists of 32 per round, the running best
//     list carried from round to round: one round up to V = 258 048), then logit = the stored float read back from the row,
//     logprob = logit - lse.
// Both launches select through select_topk() below: a threshold, then an exact sort of what passes it.
//   1. every thread's largest key -> LDS; wave 0 finds T = the k-th largest of the 256 thread maxima by a search over the key's
//      bits, most significant first (a bit stays set while >= k maxima are >= the prefix: compare, ballot, popcount);
//   2. at least k keys are >= T (k thread maxima are), and a thread whose maximum is below T holds none: the keys >= T -- the
//      survivors -- are at most k threads' keys, <= 16 k <= TOPK_CAP whatever the data (sorted rows, constant rows, the k largest in one
//      thread, one wave or one tile), typically k plus a few.  (Fewer than k candidates at all: T falls below every key, all survive.)
//   3. the survivors are compacted to LDS (an LDS counter; their order there does not matter) and every survivor counts the
//      survivors above it: that count is its place.  <= TOPK_CAP^2 / 256 comparisons per thread: the bounded worst case.
// The kernel boundary is the grid-wide dependency: no atomics on global memory, no counters, no waits between workgroups.
#include "device_common.h"
#include "kernels.h"

namespace nano {

namespace {
constexpr uint32_t TOPK_THREADS = 256, TOPK_QUADS = SCORE_TILE / (4 * TOPK_THREADS);         // score.hip's tile shape
constexpr uint32_t TOPK_CAP = 16 * NANO_TOPK_MAX;                                            // survivors: k threads x 16 keys
constexpr uint32_t MERGE_KEYS = 8;                                                           // candidates per thread of a merge round
static_assert(TOPK_QUADS * 4 * TOPK_THREADS == SCORE_TILE, "a tile is a whole number of quads per thread");
static_assert(TOPK_THREADS * MERGE_KEYS >= 2 * NANO_TOPK_MAX, "a merge round takes the running list and at least one tile's");

typedef unsigned long long u64;

__device__ __forceinline__ uint32_t topk_ord(float x) {
    uint32_t b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;                                                            // -0.0f ties with +0.0f: the index decides
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ u64 topk_key(float x, uint32_t index) { return ((u64)topk_ord(x) << 32) | (u64)(0xffffffffu - index); }

struct TopkShared {
    u64 mx[TOPK_THREADS];          // every thread's largest key
    u64 surv[TOPK_CAP];            // the keys >= T, in arrival order
    u64 T;
    uint32_t n;                    // keys that asked for a place in surv
};

// how many of wave 0's 256 thread maxima (four per lane) are >= p
__device__ __forceinline__ uint32_t maxima_at_least(const u64 (&m)[4], u64 p) {
    return (uint32_t)(__popcll(__ballot(m[0] >= p)) + __popcll(__ballot(m[1] >= p)) + __popcll(__ballot(m[2] >= p)) + __popcll(__ballot(m[3] >= p)));
}

// The best k of the workgroup's TOPK_THREADS x NC keys (0: none), in order: emit(place, key) for place = 0 .. min(k, #keys) - 1, each
// from the thread that happens to hold it.  Bits lo_bits .. 31 of every non-zero key are lo_fixed (a tile's indices share their upper
// 20 bits: the search skips them).  Ends behind a barrier only for sh: the caller orders what emit() wrote.
template <uint32_t NC, class Emit>
__device__ __forceinline__ void select_topk(const u64 (&key)[NC], uint32_t k, uint32_t lo_bits, uint32_t lo_fixed, TopkShared &sh, Emit emit) {
    static_assert(NC * NANO_TOPK_MAX <= TOPK_CAP, "k threads' keys fit the survivor list");
    const uint32_t tid = threadIdx.x;
    u64 lm = 0;
#pragma unroll
    for (uint32_t i = 0; i < NC; i++) lm = key[i] > lm ? key[i] : lm;
    sh.mx[tid] = lm;
    if (tid == 0) sh.n = 0u;
    __syncthreads();
    if (tid < 64u) {
        const u64 m[4] = { sh.mx[tid], sh.mx[tid + 64u], sh.mx[tid + 128u], sh.mx[tid + 192u] };
        u64 p = 0;
#pragma unroll 1
        for (int b = 63; b >= 32; b--) { const u64 c = p | (1ull << b); if (maxima_at_least(m, c) >= k) p = c; }
        p |= (u64)lo_fixed;        // (fewer than k maxima: p stays below every key, whose ord is never 0)
#pragma unroll 1
        for (int b = (int)lo_bits - 1; b >= 0; b--) { const u64 c = p | (1ull << b); if (maxima_at_least(m, c) >= k) p = c; }
        if (tid == 0) sh.T = p;
    }
    __syncthreads();
    const u64 T = sh.T;
#pragma unroll
    for (uint32_t i = 0; i < NC; i++)
        if (key[i] != 0 && key[i] >= T) {
            const uint32_t s = atomicAdd(&sh.n, 1u);
            if (s < TOPK_CAP) sh.surv[s] = key[i];                                           // (never more: see the header; the store stays inside LDS regardless)
        }
    __syncthreads();
    const uint32_t ns = sh.n < TOPK_CAP ? sh.n : TOPK_CAP;
    for (uint32_t s = tid; s < ns; s += TOPK_THREADS) {
        const u64 mine = sh.surv[s];
        uint32_t above = 0;
        for (uint32_t i = 0; i < ns; i++) above += sh.surv[i] > mine ? 1u : 0u;              // (one address per wave: a broadcast read)
        if (above < k) emit(above, mine);
    }
}
}  // namespace

__global__ __launch_bounds__(TOPK_THREADS) void topk_tiles_kernel(const TopkArgs a) {
    __shared__ TopkShared sh;
    const uint32_t tile = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const float *row = a.logits + (size_t)r * a.V;
    const uint32_t base = tile * SCORE_TILE;
    const uint32_t n = a.V - base < SCORE_TILE ? a.V - base : SCORE_TILE;                    // logits of this tile (>= 1)
    const bool aligned = ((reinterpret_cast<uintptr_t>(row + base)) & 15u) == 0;
    u64 key[TOPK_QUADS * 4];
#pragma unroll
    for (uint32_t j = 0; j < TOPK_QUADS; j++) {
        const uint32_t e = 4u * tid + j * 4u * TOPK_THREADS;                                 // first logit of the quad, inside the tile
        if (aligned && e + 3u < n) {
            const float4 q = *reinterpret_cast<const float4 *>(row + base + e);
            key[4 * j] = topk_key(q.x, base + e); key[4 * j + 1] = topk_key(q.y, base + e + 1u);
            key[4 * j + 2] = topk_key(q.z, base + e + 2u); key[4 * j + 3] = topk_key(q.w, base + e + 3u);
        } else {
#pragma unroll
            for (uint32_t c = 0; c < 4; c++) key[4 * j + c] = e + c < n ? topk_key(row[base + e + c], base + e + c) : 0ull;
        }
    }
    u64 *dst = a.part + ((size_t)r * a.ntiles + tile) * a.k;
    if (tid < a.k && tid >= n) dst[tid] = 0ull;                                              // a tile with fewer than k logits
    select_topk(key, a.k, 12u, ~base & 0xfffff000u, sh, [&](uint32_t place, u64 kk) { dst[place] = kk; });
}

__global__ __launch_bounds__(TOPK_THREADS) void topk_merge_kernel(const TopkArgs a) {
    __shared__ TopkShared sh;
    __shared__ u64 best[NANO_TOPK_MAX];
    const uint32_t r = blockIdx.x, tid = threadIdx.x, k = a.k;
    const u64 *part = a.part + (size_t)r * a.ntiles * k;
    if (tid < NANO_TOPK_MAX) best[tid] = 0ull;
    const uint32_t per_round = (TOPK_THREADS * MERGE_KEYS - k) / k;                          // tile lists next to the running list: >= 63
    for (uint32_t t0 = 0; t0 < a.ntiles; t0 += per_round) {
        __syncthreads();                                                                     // best[] of the round before (or the zeros)
        const uint32_t nt = a.ntiles - t0 < per_round ? a.ntiles - t0 : per_round, total = k + nt * k;
        u64 key[MERGE_KEYS];
#pragma unroll
        for (uint32_t j = 0; j < MERGE_KEYS; j++) {
            // candidate c: the running list, then place 0 of every tile of the round, place 1 of every tile, ... (the lists' heads spread
            // over the first threads, so the thread maxima are the heads and the threshold is tight)
            const uint32_t c = tid + j * TOPK_THREADS;
            key[j] = 0ull;
            if (c < k) key[j] = best[c];
            else if (c < total) { const uint32_t c2 = c - k, place = c2 / nt, t = t0 + (c2 - place * nt); key[j] = part[(size_t)t * k + place]; }
        }
        select_topk(key, k, 32u, 0u, sh, [&](uint32_t place, u64 kk) { best[place] = kk; });
    }
    __syncthreads();
    if (tid < k) {
        const u64 kk = best[tid];
        const uint32_t token = 0xffffffffu - (uint32_t)kk;
        NanoHipTopEntry o;
        o.token = token; o.logit = -INFINITY; o.logprob = -INFINITY;
        if (kk != 0 && token < a.V) {                                                        // (always: k <= V candidates exist)
            o.logit = a.logits[(size_t)r * a.V + token];                                     // the stored float: -0.0f stays -0.0f
            o.logprob = o.logit - a.scores[r].lse;
        }
        a.out[(size_t)r * k + tid] = o;
    }
}

hipError_t launch_topk_rows(const TopkArgs &a, uint32_t rows, hipStream_t st) {
    if (!rows) return hipSuccess;
    if (!a.V || a.ntiles != score_tiles(a.V) || !a.k || a.k > NANO_TOPK_MAX || a.k > a.V || rows > 65535u ||
        !a.logits || !a.part || !a.scores || !a.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_tiles_kernel, dim3(a.ntiles, rows), dim3(TOPK_THREADS), 0, st, a);
    hipLaunchKernelGGL(topk_merge_kernel, dim3(rows), dim3(TOPK_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace nano
