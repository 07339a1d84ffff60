// CPU check of exact_chain.h: the chunked evaluation of rmsnorm's sum of squares (guessed exponent fields, chunk
// functions, a walker that adds term by term where a guess fails or a binade is crossed) against the plain index-order
// float loop of the reference (infer/infer.c:601-606), bit for bit, on generated vectors.
#include "../../nano_amd/csrc/exact_chain.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>
using namespace nano_exact;

int main() {
    std::mt19937_64 rng(20240611);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    std::cauchy_distribution<float> cd(0.0f, 1.0f);
    const uint32_t ns[] = {32, 48, 128, 768, 1024, 2560, 5120, 1000 /* no multiple of any chunk */, 1, 3, 65};
    const uint32_t Cs[] = {16, 32, 64};
    const char *names[] = {"gaussian", "heavy-tailed", "zero", "denormal", "dominant-first", "dominant-last", "sixteenths", "huge", "mixed-scale"};
    long cases = 0, bad = 0, chunks = 0, walked = 0;
    uint32_t worst[3] = {0, 0, 0};                                     // most walked chunks of a gaussian n = 1024 vector, per C
    for (int rep = 0; rep < 12; rep++)
        for (uint32_t n : ns)
            for (int mode = 0; mode < 9; mode++) {
                std::vector<float> x(n), p(n);
                const float scale = ldexpf(1.0f, (int)(rng() % 13) - 6);
                for (uint32_t j = 0; j < n; j++) x[j] = scale * nd(rng);
                if (mode == 1) for (uint32_t j = 0; j < n; j++) x[j] = cd(rng);
                if (mode == 2) for (uint32_t j = 0; j < n; j++) x[j] = (rng() & 1) ? 0.0f : -0.0f;
                if (mode == 3) for (uint32_t j = 0; j < n; j++) x[j] = ldexpf(nd(rng), -70 - (int)(rng() % 10));   // squares are denormal or zero
                if (mode == 4) x[0] = 1000.0f * scale;
                if (mode == 5) x[n - 1] = 1000.0f * scale;
                if (mode == 6) for (uint32_t j = 0; j < n; j++) x[j] = roundf(nd(rng) * 16.0f) / 16.0f;             // constant ties
                if (mode == 7) for (uint32_t j = 0; j < n; j++) x[j] = ldexpf(nd(rng), 62);                         // the sum overflows to +inf
                if (mode == 8) for (uint32_t j = 0; j < n; j++) x[j] = ldexpf(nd(rng), (int)(rng() % 40) - 20);
                for (uint32_t j = 0; j < n; j++) p[j] = x[j] * x[j];
                const float a = chain_sum_plain(p.data(), n);
                for (int ci = 0; ci < 3; ci++) {
                    uint32_t w = 0;
                    const float b = chain_sum_chunked(p.data(), n, Cs[ci], &w);
                    cases++; chunks += (n + Cs[ci] - 1) / Cs[ci]; walked += w;
                    if (mode == 0 && n == 1024 && w > worst[ci]) worst[ci] = w;
                    if (f32_bits(a) != f32_bits(b)) { bad++; if (bad < 10) fprintf(stderr, "%s n=%u C=%u: plain=%a chunked=%a\n", names[mode], n, Cs[ci], a, b); }
                }
            }
    printf("%ld cases, %ld mismatches; %ld chunks, %ld walked term by term (%.1f%%); gaussian n=1024: at most %u / %u / %u chunks walked at C = 16 / 32 / 64\n",
           cases, bad, chunks, walked, 100.0 * walked / chunks, worst[0], worst[1], worst[2]);
    return bad ? 1 : 0;
}
