"""The restatement of the sampler with a logit edit in front of the pick (tests only; include/nano_mi355x.h "logit edits").

Let V be the vocabulary and W = ceil(V / 32).  A row may carry
  * a mask: W uint32 words; token j is allowed when bit (j & 31) of word (j >> 5) is set; bits of tokens >= V in the last word are ignored;
  * a bias list: (tokens, values), distinct tokens in any order, at most NANO_BIAS_MAX = 1024 of them.
The edited row is

    x_j  = l_j + b_j                      one float32 add, only for a token that has an entry; a token without one keeps its stored bits
    l'_j = allowed(j) ? x_j : -inf

and the result is sampler_topk_ref.sample on l' -- sampler_ref.penalised / distribution unchanged: the penalty, the temperature, the
softmax over all V -- with ONE difference: a disallowed token is never a candidate.  The candidate test is

    allowed(j) and p_j >= cutoff.

For top_p < 1 that changes nothing (p = 0 < cutoff); for top_p >= 1 the cutoff is <= 0, the unfiltered sampler on l' counts the p = 0 tokens
as candidates, lists them in top[] and returns the sorted list's last entry when coin * sum is not below the sum.  With the filter
n_candidates and top[] hold allowed tokens only, and a returned token is always an allowed one.  Temperature 0 is the first maximum of the
penalised l'.  tests/test_logit_edit_ref.py holds this equal to sampler_topk_ref.sample where the two must agree and shows the case where
they must not."""
import hashlib

import numpy as np

import sampler_ref as sr

BIAS_MAX = 1024
NINF = np.float32(-np.inf)


def words(allowed, V):
    """mask words from a boolean array [V] or a list of allowed ids; bits of tokens >= V are left 0"""
    a = np.asarray(allowed)
    on = np.zeros(-(-V // 32) * 32, bool)
    if a.dtype == bool:
        on[:V] = a.reshape(-1)
    else:
        on[a.astype(np.int64).reshape(-1)] = True
    return np.packbits(on.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def allowed(allow, V):
    """bool[V] of a mask's words (None: every token)"""
    if allow is None:
        return np.ones(V, bool)
    w = np.ascontiguousarray(allow, np.uint32).reshape(-1)
    assert w.size == -(-V // 32), (w.size, V)
    return np.unpackbits(w.astype("<u4").view(np.uint8), bitorder="little")[:V].astype(bool)


def edited(logits, allow=None, bias=None):
    """l': float32[V]"""
    x = np.array(logits, np.float32).reshape(-1)
    if bias is not None and len(bias[0]):
        t = np.asarray(bias[0], np.int64).reshape(-1)
        v = np.asarray(bias[1], np.float32).reshape(-1)
        assert t.size == v.size <= BIAS_MAX and np.unique(t).size == t.size and t.min() >= 0 and t.max() < x.size
        with np.errstate(invalid="ignore"):
            x[t] = x[t] + v
    x[~allowed(allow, x.size)] = NINF
    return x


_nucleus_cache = {}


def nucleus(d, key, top_p, on):
    """sampler_ref.nucleus with the allowed filter in the candidate test"""
    V = d.p.size
    tp = np.float32(top_p)
    k = (key, tp.tobytes(), hashlib.blake2b(np.packbits(on).tobytes(), digest_size=16).digest())
    n = _nucleus_cache.get(k)
    if n is None:
        with np.errstate(divide="ignore"):
            cutoff = np.float32((np.float32(1.0) - tp) / np.float32(V - 1))
        idx = np.nonzero(on & (d.p >= cutoff))[0]
        order = idx[np.argsort(-d.p[idx], kind="stable")]
        cdf = np.cumsum(d.p[order], dtype=np.float32)
        above = np.nonzero(cdf > tp)[0]
        n = sr.Nucleus(int(idx.size), order, cdf, int(above[0]) if above.size else int(idx.size) - 1, bool(above.size))
        _nucleus_cache[k] = n
    return n


def sample(logits, history, penalty, temperature, top_p, coin, top_k=0, allow=None, bias=None):
    """sampler_ref.Sample of the edited row, every field with the meaning it has in sampler_topk_ref.sample"""
    lp = edited(logits, allow, bias)
    y = sr.penalised(lp, history, penalty, temperature)
    if temperature == 0.0:
        return sr.Sample(int(np.argmax(y)), 0, argmax=True)
    d, key = sr.distribution(y)
    n = nucleus(d, key, top_p, allowed(allow, lp.size))
    if n.n0 == 0:
        return sr.Sample(0, 0, none=True, sum_bits=d.sum_bits, crossings=d.crossings)
    nk = min(n.n0, int(top_k)) if top_k > 0 else n.n0
    order, cdf = n.order[:nk], n.cdf[:nk]
    above = np.nonzero(cdf > np.float32(top_p))[0]
    cut, last = bool(above.size), int(above[0]) if above.size else nk - 1
    r = np.float32(coin) * cdf[last]
    above = np.nonzero(cdf[:last + 1] > r)[0]
    pick = int(above[0]) if above.size else last
    top = tuple(int(t) for t in order[:6]) + (0,) * max(0, 6 - nk)
    return sr.Sample(int(order[pick]), n.n0, sum_bits=d.sum_bits, nucleus=last + 1, top=top, cut=cut, last=last, pick=pick,
                     r=float(r), crossings=d.crossings)
