// lookup.hip -- greedy decode with lookup drafts: what happens between two steps of the loop, on the device next to the token and
// position buffers the steps read (tests/lookup_ref.py restates the definitions in plain Python).
//
// lookup_step_kernel, one workgroup of 256 threads behind the arg-max kernel of every step:
//   accept   the step fed f[0..nb) at positions n-1 .. n-2+nb and left row arg-maxes g[0..nb): a = the largest a <= nb-1 with
//            f[i] == g[i-1] for all 1 <= i <= a (rows behind the first mismatch do not count, whatever they hold)
//   emit     g[0 .. min(a+1, left)), cut after the first stop token; appended to the history and to the call's trace
//   lookup   for every end e in 1 .. n-1: L(e) = how many of the last ngram_max ids before e equal the history's last ids, counted
//            backwards up to the first mismatch; the match is the largest (L(e), e) with L(e) >= ngram_min.  ONE pass over e: a thread
//            takes four ends per 16-byte load (plus the 16 bytes before them), the suffix ids sit in registers, the key
//            (L << 32) | e is maximised in the wave and across the four waves through LDS.
//   draft    d[i] = h[e+i] while e+i < n, then d[e+i-n]: the periodic extension (a loop of any period is drafted in full)
//   gate     a verify chunk of K = max_draft + 1 rows only with a draft, left >= 2, the chunk inside one 64-position bucket and below
//            seq_limit; otherwise one row
//   stage    the next step's tokens and positions, the record for the host
// No waits on other workgroups, no atomics; every loop is bounded by n <= cap or by LOOKUP_MAX_ROWS.
#include "device_common.h"
#include "kernels.h"

namespace nano {

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}

__global__ __launch_bounds__(256) void lookup_step_kernel(const LookupArgs a) {
    __shared__ uint32_t s_f[LOOKUP_MAX_ROWS], s_g[LOOKUP_MAX_ROWS], s_d[LOOKUP_MAX_ROWS];
    __shared__ unsigned long long s_key[4];
    __shared__ uint32_t s_n, s_left, s_done, s_emitted, s_accepted;
    const uint32_t tid = threadIdx.x;
    const uint32_t nb = a.nb < LOOKUP_MAX_ROWS ? a.nb : LOOKUP_MAX_ROWS;
    if (tid < nb) { s_f[tid] = a.fed[tid]; s_g[tid] = a.amax[tid]; }
    __syncthreads();
    if (tid == 0) {                                           // accept, clip, stop, append
        uint32_t n = a.state[0], left = a.state[1];
        const uint32_t cur = a.state[2];
        uint32_t acc = 0, emitted = 0, done = left == 0 ? 1u : 0u;
        if (nb) {
            while (acc + 1 < nb && s_f[acc + 1] == s_g[acc]) acc++;
            const uint32_t want = acc + 1 < left ? acc + 1 : left;
            for (uint32_t i = 0; i < want && n < a.cap; i++) {
                const uint32_t tok = s_g[i];
                a.hist[n++] = tok;
                if (a.trace && cur + emitted < a.trace_cap) a.trace[cur + emitted] = tok;
                emitted++;
                if (tok == a.stop_token) { done = 1; break; }
            }
            left -= emitted;
            if (left == 0 || n >= a.cap) done = 1;
            a.state[0] = n; a.state[1] = left; a.state[2] = cur + emitted;
        }
        s_n = n; s_left = left; s_done = done; s_emitted = emitted; s_accepted = acc;
    }
    __syncthreads();                                          // (the appended ids are visible to the workgroup's loads below)
    const uint32_t n = s_n;
    const bool look = !s_done && a.max_draft >= 1 && n >= 2;
    unsigned long long best = 0;
    if (look) {
        uint32_t s0 = a.hist[n - 1], s1 = n >= 2 ? a.hist[n - 2] : 0u, s2 = n >= 3 ? a.hist[n - 3] : 0u, s3 = n >= 4 ? a.hist[n - 4] : 0u;
        const uint32_t ng = a.ngram_max < LOOKUP_MAX_NGRAM ? a.ngram_max : LOOKUP_MAX_NGRAM;
        const uint4 *h4 = reinterpret_cast<const uint4 *>(a.hist);
        // group g holds the ends e = 4g+1 .. 4g+4, whose windows h[e-4 .. e-1] lie in h[4g-3 .. 4g+3]: vectors g-1 and g
        for (uint32_t g = tid; 4 * g + 1 <= n - 1; g += 256) {
            const uint4 c = h4[g], p = g ? h4[g - 1] : make_uint4(0, 0, 0, 0);
            const uint32_t w[8] = { p.x, p.y, p.z, p.w, c.x, c.y, c.z, c.w };
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t e = 4 * g + 1 + k;
                const uint32_t lim = ng < e ? ng : e;         // the window does not run off the start
                uint32_t L = 0;
                bool run = e <= n - 1;
                run = run && lim > 0 && w[4 + k] == s0;      if (run) L = 1;
                run = run && lim > 1 && w[3 + k] == s1;      if (run) L = 2;
                run = run && lim > 2 && w[2 + k] == s2;      if (run) L = 3;
                run = run && lim > 3 && w[1 + k] == s3;      if (run) L = 4;
                const unsigned long long key = L >= a.ngram_min && L ? ((unsigned long long)L << 32) | e : 0ull;
                best = key > best ? key : best;
            }
        }
    }
    best = wave_max_u64(best);
    if ((tid & 63u) == 0) s_key[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {                                           // draft, gate, stage, record
        unsigned long long key = s_key[0];
        for (int w = 1; w < 4; w++) key = s_key[w] > key ? s_key[w] : key;
        const uint32_t mlen = (uint32_t)(key >> 32), mend = (uint32_t)key;
        const uint32_t D = a.max_draft < LOOKUP_MAX_ROWS - 1 ? a.max_draft : LOOKUP_MAX_ROWS - 1, K = D + 1;
        const uint32_t left = s_left, done = s_done;
        uint32_t nb_next = done ? 0u : 1u;
        if (!done && key && D >= 1 && left >= 2 && (n - 1) % 64u + K <= 64u && (unsigned long long)(n - 1) + K <= a.seq_limit) nb_next = K;
        if (!done) {
            a.next_tokens[0] = a.hist[n - 1]; a.next_pos[0] = n - 1;
            if (nb_next == K && K > 1) {
                for (uint32_t i = 0; i < D; i++) {
                    const uint32_t d = mend + i < n ? a.hist[mend + i] : s_d[mend + i - n];      // (mend >= 1 and mend + i >= n: the index is below i)
                    s_d[i] = d;
                    a.next_tokens[1 + i] = d; a.next_pos[1 + i] = n + i;
                }
            }
        }
        a.record[LOOKUP_REC_EMITTED] = s_emitted; a.record[LOOKUP_REC_ACCEPTED] = s_accepted; a.record[LOOKUP_REC_NB_NEXT] = nb_next;
        a.record[LOOKUP_REC_N] = n; a.record[LOOKUP_REC_MATCH_LEN] = mlen; a.record[LOOKUP_REC_MATCH_END] = mend;
        a.record[LOOKUP_REC_DONE] = done; a.record[LOOKUP_REC_LEFT] = left;
    }
}

hipError_t launch_lookup_step(const LookupArgs &a, hipStream_t st) {
    if (!a.hist || !a.state || !a.next_tokens || !a.next_pos || !a.record || !a.cap || a.cap % 4u || a.nb > LOOKUP_MAX_ROWS || (a.nb && (!a.fed || !a.amax)) ||
        (reinterpret_cast<uintptr_t>(a.hist) & 15u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lookup_step_kernel, dim3(1), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace nano
