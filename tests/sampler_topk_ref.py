"""The restatement of the sampler with top-k truncation in front of the top-p cut (tests only; include/nano_mi355x.h "top-k truncation").

sampler_ref.parts() -- steps 1-9 of tests/sampler_ref.py, unchanged: the denominator over all V tokens, candidates p >= cutoff, the stable
descending sort -- plus the one statement behind the reference's qsort (infer/infer.c:1074-1076):

    if (top_k > 0 && (uint32_t)n0 > top_k) n0 = top_k;

and steps 10-13 on the list that is left: last = the first cdf > top_p, else the list's last entry; r = coin * cdf[last]; pick = the
first cdf > r, else last.  sample() returns sampler_ref.Sample with the same meaning of every field: n_candidates stays the count of
p >= cutoff, top[i] is 0 for i >= min(n0, top_k), sum_bits and crossings do not depend on top_k, temperature 0 ignores top_k.
tests/test_sampler_topk_ref.py holds it equal to sampler_ref.sample for top_k = 0 and top_k >= n0 on every case of
tests/sampler_path_cases.py."""
import numpy as np

import sampler_ref as sr


def sample(logits, history, penalty, temperature, top_p, coin, top_k=0):
    if temperature == 0.0:
        return sr.Sample(int(np.argmax(sr.penalised(logits, history, penalty, temperature))), 0, argmax=True)
    d, n = sr.parts(logits, history, penalty, temperature, top_p)
    if n.n0 == 0:
        return sr.Sample(0, 0, none=True, sum_bits=d.sum_bits, crossings=d.crossings)
    nk = min(n.n0, int(top_k)) if top_k > 0 else n.n0
    order, cdf = n.order[:nk], n.cdf[:nk]                     # (a prefix of a sequential running sum is the running sum of the prefix)
    above = np.nonzero(cdf > np.float32(top_p))[0]
    cut, last = bool(above.size), int(above[0]) if above.size else nk - 1
    r = np.float32(coin) * cdf[last]
    above = np.nonzero(cdf[:last + 1] > r)[0]
    pick = int(above[0]) if above.size else last
    top = tuple(int(t) for t in order[:6]) + (0,) * max(0, 6 - nk)
    return sr.Sample(int(order[pick]), n.n0, sum_bits=d.sum_bits, nucleus=last + 1, top=top, cut=cut, last=last, pick=pick,
                     r=float(r), crossings=d.crossings)
