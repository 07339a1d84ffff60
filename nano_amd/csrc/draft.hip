// draft.hip -- greedy decode with a draft model: what happens between the two models' steps of a round, on the device next to the token
// and position buffers both models' steps read (tests/draft_ref.py restates the definitions in plain Python).
//
// draft_round_kernel, one workgroup of 64 threads, three roles (kernels.h DraftArgs):
//   STAGE    the draft ran D' = nb - 1 loop steps from hist[n-1]; its ids d[0..D') become rows 1 .. D' of the target's verify chunk
//            (row 0 and every position were staged by the ACCEPT launch of the round before)
//   ACCEPT   the target fed f[0..nb) at positions n-1 .. n-2+nb and left row arg-maxes g[0..nb):
//     accept   a = the largest a <= nb-1 with f[i] == g[i-1] for all 1 <= i <= a (lookup.hip's definition)
//     emit     g[0 .. min(a+1, left)), cut after the first stop token; appended to the history and to the call's trace
//     dn       the draft fed hist[n-1], d1 .. d(D'-1) at positions n-1 .. n-2+D': its rows are right up to position n-1+min(a, D'-1), so
//              it holds n + min(a, D'-1) positions -- and never more than the new history's n - 1 (a stop token cut the emitted ids).
//              A one-row round (nb <= 1) ran no draft step: dn stays
//     next     rows of the next round by the bucket rule (draft_round_rows), row 0 = hist[n-1] and positions n-1 .. for the target,
//              row 0 and the loop's first position for the draft
//   BEGIN    the draft's row 0 again, behind a catch-up chunk that used the draft's token and position rows
// No waits on other workgroups, no atomics; every loop is bounded by LOOKUP_MAX_ROWS, every history index by cap.
#include "device_common.h"
#include "kernels.h"

namespace nano {

__global__ __launch_bounds__(64) void draft_round_kernel(const DraftArgs a) {
    __shared__ uint32_t s_f[LOOKUP_MAX_ROWS], s_g[LOOKUP_MAX_ROWS];
    const uint32_t tid = threadIdx.x;
    const uint32_t nb = a.nb < LOOKUP_MAX_ROWS ? a.nb : LOOKUP_MAX_ROWS;
    if (a.role == DRAFT_ROLE_STAGE) {
        if (tid + 1 < nb) a.next_tokens[1 + tid] = a.ids[tid];
        return;
    }
    if (a.role == DRAFT_ROLE_BEGIN) {
        if (tid == 0) {
            const uint32_t n = a.state[0];
            if (n >= 1 && n <= a.cap) { a.d_tokens[0] = a.hist[n - 1]; a.d_pos[0] = n - 1; a.d_pos0[0] = n - 1; }
        }
        return;
    }
    if (tid < nb) { s_f[tid] = a.fed[tid]; s_g[tid] = a.amax[tid]; }
    __syncthreads();
    if (tid != 0) return;
    uint32_t n = a.state[0], left = a.state[1];
    const uint32_t cur = a.state[2], n_old = n;
    uint32_t acc = 0, emitted = 0, done = left == 0 ? 1u : 0u, dn = a.dn;
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
        if (nb > 1) {
            dn = n_old + (acc < nb - 2 ? acc : nb - 2);
            if (dn > n - 1) dn = n - 1;                       // (n > n_old here unless the history is full: then the call is done)
        }
    }
    const uint32_t nb_next = done ? 0u : draft_round_rows(n, left, a.max_draft, a.seq_limit);
    if (!done && n >= 1) {
        const uint32_t last = a.hist[n - 1];
        a.next_tokens[0] = last;
        for (uint32_t i = 0; i < nb_next && i < LOOKUP_MAX_ROWS; i++) a.next_pos[i] = n - 1 + i;
        if (a.d_tokens) { a.d_tokens[0] = last; a.d_pos[0] = n - 1; a.d_pos0[0] = n - 1; }
    }
    a.record[DRAFT_REC_EMITTED] = emitted; a.record[DRAFT_REC_ACCEPTED] = acc; a.record[DRAFT_REC_NB_NEXT] = nb_next; a.record[DRAFT_REC_N] = n;
    a.record[DRAFT_REC_DN] = dn; a.record[DRAFT_REC_CURSOR] = cur + emitted; a.record[DRAFT_REC_DONE] = done; a.record[DRAFT_REC_LEFT] = left;
}

hipError_t launch_draft_round(const DraftArgs &a, hipStream_t st) {
    if (a.role > DRAFT_ROLE_BEGIN || a.nb > LOOKUP_MAX_ROWS) return hipErrorInvalidValue;
    if (a.role == DRAFT_ROLE_STAGE) {
        if (a.nb < 2 || !a.ids || !a.next_tokens) return hipErrorInvalidValue;
    } else if (a.role == DRAFT_ROLE_BEGIN) {
        if (!a.hist || !a.cap || !a.state || !a.d_tokens || !a.d_pos || !a.d_pos0) return hipErrorInvalidValue;
    } else {
        if (!a.hist || !a.cap || !a.state || !a.next_tokens || !a.next_pos || !a.record || (a.nb && (!a.fed || !a.amax)) ||
            (a.d_tokens && (!a.d_pos || !a.d_pos0))) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(draft_round_kernel, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace nano
