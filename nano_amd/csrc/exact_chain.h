// exact_chain.h -- the reference's index-order float sums of NON-NEGATIVE terms (rmsnorm's sum of squares,
// infer/infer.c:601-606; the softmax denominator, infer.c:625-629), restated so that most of the chain can be evaluated
// out of order and the result is still the plain loop's float, bit for bit.  Host and device (exact mode, exact.hip;
// the CPU check is tools/exact/ssq_check.cpp).
//
// The algebra is exact_math.h's ChunkFn: while the running sum stays inside one binade, adding a chunk of terms is a
// function of the parity of the sum's mantissa alone, and that function can be computed without knowing the sum -- only
// its exponent field.  Unlike the sampler's sum (one term is exactly 1, so the sum settles in a binade at once) a sum of
// squares starts at zero and climbs through about log2(n) binades, so the exponent field at each chunk start has to be
// GUESSED from an approximate prefix (any summation order will do: a wrong guess costs time, never bits):
//
//   1. approx[c] = some float sum of chunk c's terms; its running prefix guesses the exponent field Es[c] of the exact
//      sum at the start of chunk c;
//   2. every chunk, independently: its ChunkFn for Es[c];
//   3. one walker, chunks in order: chunk_apply where the guess holds and the sum stays in its binade, else the chunk's
//      terms are added one by one.  The first chunk is always walked.
//
// With 64-term chunks a 1024-term sum of squares of Gaussian data walks at most 5 of its 16 chunks, the first included (the
// binade crossings; tools/exact/ssq_check.cpp prints the count).  chain_sum_chunked() below is that scheme with steps 1
// and 2 written as loops; exact.hip's rmsnorm and softmax currently run the plain chain on one lane out of LDS
// (chain_sum_plain's order) -- see the note there.
#pragma once
#include "exact_math.h"

namespace nano_exact {

// the reference's loop
NANO_HD float chain_sum_plain(const float *p, uint32_t n) {
    float s = 0.0f;
    for (uint32_t j = 0; j < n; j++) s += p[j];
    return s;
}

// an approximate sum of p[0..n) in an order of its own (pairs, as a wave reduction would): only ever used as a guess
NANO_HD float chain_sum_approx(const float *p, uint32_t n) {
    float a = 0.0f, b = 0.0f;
    for (uint32_t j = 0; j + 1 < n; j += 2) { a += p[j]; b += p[j + 1]; }
    if (n & 1u) a += p[n - 1];
    return a + b;
}

// the ChunkFn of p[0..n) for sums whose exponent field is Es
NANO_HD ChunkFn chain_chunk_fn(const float *p, uint32_t n, uint32_t Es) {
    ChunkFn f{0u, 0u};
    for (uint32_t j = 0; j < n; j++) chunk_push(f, f32_bits(p[j]), Es);
    return f;
}

// advance the running sum (bits sb) over one chunk: by its function where that applies, term by term otherwise.
// Returns whether the chunk had to be walked.  Es = 255 (a guess of inf / nan) is never trusted.
NANO_HD bool chain_step(uint32_t &sb, const float *p, uint32_t n, ChunkFn f, uint32_t Es) {
    if (Es < 255u && chunk_apply(sb, f, Es)) return false;
    float s = bits_f32(sb);
    for (uint32_t j = 0; j < n; j++) s += p[j];
    sb = f32_bits(s);
    return true;
}

// sum of p[0..n), every p[j] >= 0 (or nan / +inf), in index order; chunks of C terms.  *walked: chunks added term by term.
NANO_HD float chain_sum_chunked(const float *p, uint32_t n, uint32_t C, uint32_t *walked) {
    uint32_t sb = 0u, nw = 0u;
    float approx = 0.0f;
    for (uint32_t c0 = 0; c0 < n; c0 += C) {
        const uint32_t len = n - c0 < C ? n - c0 : C;
        if (c0 == 0) {
            sb = f32_bits(chain_sum_plain(p, len));
            nw++;
        } else {
            const uint32_t Es = sum_exp(f32_bits(approx));
            nw += chain_step(sb, p + c0, len, chain_chunk_fn(p + c0, len, Es), Es) ? 1u : 0u;
        }
        approx += chain_sum_approx(p + c0, len);
    }
    if (walked) *walked = nw;
    return bits_f32(sb);
}

}  // namespace nano_exact
