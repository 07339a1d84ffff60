// lookup_rows.hip -- lookup drafts for several sequences: what happens between two ragged passes of nano_hip_decode_lookup_rows, on the
// device next to the token, position and row -> slot buffers the passes read (tests/lookup_rows_ref.py restates
// the round in plain Python on top of tests/lookup_ref.py).
//
// lookup_rows_seq_kernel, one workgroup of 256 threads per sequence, behind the arg-max kernel of the pass: lookup.hip's definitions
// (accept, emit, lookup, draft, gate -- the text there is the specification) on the sequence's own history and its own rows of the
// pass.  It stages nothing in the pass's buffers, which the other workgroups still read: the next rows' tokens go to stage[i][16], the
// record to record[i][8].
// lookup_rows_pack_kernel, one workgroup behind it: the live sequences (nb_next > 0) in the order of nano_hip_rows_plan -- by the range
// hint of position n - 1, stably -- each sequence's rows contiguous and ascending; the next pass's tokens, positions and row -> slot
// map, and every sequence's first row and row count for the next accept.
// Two launches because the pack needs every sequence's gate: no waits on other workgroups, no atomics; every loop is bounded by
// n <= cap, by LOOKUP_MAX_ROWS or by n_seqs.
#include "device_common.h"
#include "kernels.h"

namespace nano {

static __device__ __forceinline__ unsigned long long rows_wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}

__global__ __launch_bounds__(256) void lookup_rows_seq_kernel(const LookupRowsArgs a) {
    __shared__ uint32_t s_f[LOOKUP_MAX_ROWS], s_g[LOOKUP_MAX_ROWS], s_d[LOOKUP_MAX_ROWS];
    __shared__ unsigned long long s_key[4];
    __shared__ uint32_t s_n, s_left, s_done, s_emitted, s_accepted;
    const uint32_t tid = threadIdx.x, seq = blockIdx.x;
    if (seq >= a.n_seqs) return;
    uint32_t *hist = a.hist + (size_t)a.seq_slot[seq] * a.cap;
    uint32_t *state = a.state + (size_t)seq * LOOKUP_ST_WORDS;
    uint32_t *record = a.record + (size_t)seq * LOOKUP_REC_WORDS;
    uint32_t *stage = a.stage + (size_t)seq * LOOKUP_MAX_ROWS;
    const uint32_t was_done = state[LOOKUP_ST_DONE];
    uint32_t nb = was_done ? 0u : a.nb[seq];
    nb = nb < LOOKUP_MAX_ROWS ? nb : LOOKUP_MAX_ROWS;
    const uint32_t r0 = nb ? a.row_start[seq] : 0u;
    if (tid < nb) { s_f[tid] = a.fed[r0 + tid]; s_g[tid] = a.amax[r0 + tid]; }
    __syncthreads();
    if (tid == 0) {                                           // accept, clip, stop, append
        uint32_t n = state[LOOKUP_ST_N], left = state[LOOKUP_ST_LEFT];
        const uint32_t cur = state[LOOKUP_ST_CURSOR], base = a.trace_base ? a.trace_base[seq] : 0u;
        uint32_t acc = 0, emitted = 0, done = (was_done || left == 0) ? 1u : 0u;
        if (nb) {
            while (acc + 1 < nb && s_f[acc + 1] == s_g[acc]) acc++;
            const uint32_t want = acc + 1 < left ? acc + 1 : left;
            for (uint32_t i = 0; i < want && n < a.cap; i++) {
                const uint32_t tok = s_g[i];
                hist[n++] = tok;
                if (a.trace && (unsigned long long)base + cur + emitted < a.trace_cap) a.trace[base + cur + emitted] = tok;
                emitted++;
                if (tok == a.stop_token) { done = 1; break; }
            }
            left -= emitted;
            if (left == 0 || n >= a.cap) done = 1;
            state[LOOKUP_ST_N] = n; state[LOOKUP_ST_LEFT] = left; state[LOOKUP_ST_CURSOR] = cur + emitted;
        }
        if (done) state[LOOKUP_ST_DONE] = 1u;
        s_n = n; s_left = left; s_done = done; s_emitted = emitted; s_accepted = acc;
    }
    __syncthreads();                                          // (the appended ids are visible to the workgroup's loads below)
    const uint32_t n = s_n;
    const bool look = !s_done && a.max_draft >= 1 && n >= 2;
    unsigned long long best = 0;
    if (look) {
        uint32_t s0 = hist[n - 1], s1 = n >= 2 ? hist[n - 2] : 0u, s2 = n >= 3 ? hist[n - 3] : 0u, s3 = n >= 4 ? hist[n - 4] : 0u;
        const uint32_t ng = a.ngram_max < LOOKUP_MAX_NGRAM ? a.ngram_max : LOOKUP_MAX_NGRAM;
        const uint4 *h4 = reinterpret_cast<const uint4 *>(hist);
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
    best = rows_wave_max_u64(best);
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
            stage[0] = hist[n - 1];
            if (nb_next == K && K > 1) {
                for (uint32_t i = 0; i < D; i++) {
                    const uint32_t d = mend + i < n ? hist[mend + i] : s_d[mend + i - n];        // (mend >= 1 and mend + i >= n: the index is below i)
                    s_d[i] = d;
                    stage[1 + i] = d;
                }
            }
        }
        record[LOOKUP_REC_EMITTED] = s_emitted; record[LOOKUP_REC_ACCEPTED] = s_accepted; record[LOOKUP_REC_NB_NEXT] = nb_next;
        record[LOOKUP_REC_N] = n; record[LOOKUP_REC_MATCH_LEN] = mlen; record[LOOKUP_REC_MATCH_END] = mend;
        record[LOOKUP_REC_DONE] = done; record[LOOKUP_REC_LEFT] = left;
    }
}

// sequence i's place in the next pass: behind every live sequence with a smaller hint, and behind those with its own hint and a smaller index
__global__ __launch_bounds__(256) void lookup_rows_pack_kernel(const LookupRowsArgs a) {
    for (uint32_t i = threadIdx.x; i < a.n_seqs; i += 256) {
        const uint32_t *rec = a.record + (size_t)i * LOOKUP_REC_WORDS;
        uint32_t nbn = rec[LOOKUP_REC_NB_NEXT];
        nbn = nbn < LOOKUP_MAX_ROWS ? nbn : LOOKUP_MAX_ROWS;
        const uint32_t n = rec[LOOKUP_REC_N];
        uint32_t start = LOOKUP_ROW_NONE;
        if (nbn && n) {
            const uint32_t hint = lookup_rows_hint(n, a.max_seq_len);
            start = 0;
            for (uint32_t j = 0; j < a.n_seqs; j++) {
                const uint32_t *rj = a.record + (size_t)j * LOOKUP_REC_WORDS;
                uint32_t nj = rj[LOOKUP_REC_NB_NEXT];
                nj = nj < LOOKUP_MAX_ROWS ? nj : LOOKUP_MAX_ROWS;
                if (!nj || !rj[LOOKUP_REC_N] || j == i) continue;
                const uint32_t hj = lookup_rows_hint(rj[LOOKUP_REC_N], a.max_seq_len);
                if (hj < hint || (hj == hint && j < i)) start += nj;
            }
            const uint32_t slot = a.seq_slot[i];
            for (uint32_t k = 0; k < nbn; k++) {
                a.next_tokens[start + k] = a.stage[(size_t)i * LOOKUP_MAX_ROWS + k];
                a.next_pos[start + k] = n - 1 + k;
                a.next_slot[start + k] = slot;
            }
        }
        a.row_start[i] = start; a.nb[i] = start == LOOKUP_ROW_NONE ? 0u : nbn;
    }
}

hipError_t launch_lookup_rows_round(const LookupRowsArgs &a, hipStream_t st) {
    if (!a.n_seqs || !a.hist || !a.seq_slot || !a.state || !a.fed || !a.amax || !a.row_start || !a.nb || !a.stage || !a.record || !a.next_tokens ||
        !a.next_pos || !a.next_slot || !a.cap || a.cap % 4u || !a.max_seq_len || a.max_draft > LOOKUP_MAX_ROWS - 1 || (a.trace && !a.trace_base) ||
        (reinterpret_cast<uintptr_t>(a.hist) & 15u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lookup_rows_seq_kernel, dim3(a.n_seqs), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lookup_rows_pack_kernel, dim3(1), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace nano
