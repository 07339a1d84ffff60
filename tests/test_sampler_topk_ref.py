"""CPU tests of the top-k restatement (tests/sampler_topk_ref.py) and of the case table of tests/test_gpu_sample_topk.py.

The restatement is sampler_ref.parts() plus one truncation, so it is pinned to sampler_ref.sample (itself pinned to the compiled
reference's golden and the oracle by tests/test_sampler_ref.py): equal field by field for top_k = 0 and for every top_k >= n0, on every
case and coin of tests/sampler_path_cases.py.  For 1 <= top_k < n0 it is held to the one statement it adds, spelled out as the plain loops
of sample_top_p over the first top_k sorted entries.  The closing test holds the top-k case table to the classes and tags it states."""
import dataclasses

import numpy as np
import pytest

import sampler_path_cases as pc
import sampler_ref as sr
import sampler_topk_cases as tc
import sampler_topk_ref as tr


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_top_k_off_and_top_k_beyond_the_candidates_change_nothing(name):
    c = pc.BY_NAME[name]
    for coin in c.coins:
        want = dataclasses.asdict(c.ref(coin))
        n0 = want["n_candidates"]
        for k in (0, max(n0, 1), n0 + 1, c.V, 0xFFFFFFFF):
            got = dataclasses.asdict(tr.sample(c.logits, c.history, c.penalty, c.temperature, c.top_p, coin, k))
            assert got == want, (name, coin, k, {f: (got[f], want[f]) for f in got if got[f] != want[f]})


def loops(p_sorted, top_p, coin):
    """the two sequential loops of sample_top_p (infer/infer.c:1078-1108) over a sorted list, in float32"""
    tp, cum, last = np.float32(top_p), np.float32(0.0), len(p_sorted) - 1
    for i, v in enumerate(p_sorted):
        cum = np.float32(cum + v)
        if cum > tp:
            last = i
            break
    r, cdf = np.float32(np.float32(coin) * cum), np.float32(0.0)
    for i in range(last + 1):
        cdf = np.float32(cdf + p_sorted[i])
        if r < cdf:
            return i, last
    return last, last


@pytest.mark.parametrize("name", [c.name for c in tc.CASES])
def test_truncation_is_the_loops_over_the_first_k(name):
    c = tc.BY_NAME[name]
    if c.temperature == 0.0:
        assert c.ref(0.0) == sr.sample(c.logits, c.history, c.penalty, 0.0, c.top_p, 0.0)
        return
    d, n = sr.parts(c.logits, c.history, c.penalty, c.temperature, c.top_p)
    for coin in c.coins:
        s = c.ref(coin)
        if n.n0 == 0:
            assert s.none and s.sum_bits == d.sum_bits
            continue
        nk = min(n.n0, c.top_k)
        pick, last = loops(d.p[n.order[:nk]], c.top_p, coin)
        assert (s.token, s.pick, s.last, s.nucleus, s.n_candidates, s.sum_bits) == (int(n.order[pick]), pick, last, last + 1, n.n0, d.sum_bits), (name, coin)
        assert s.nucleus <= c.top_k and s.top == tuple(int(t) for t in n.order[:min(6, nk)]) + (0,) * (6 - min(6, nk))
        assert s.crossings == d.crossings


def test_cases_reach_what_they_state():
    """From the restatement and the bins alone: each case reaches its class and its tags; the union reaches every class and every tag of
    REQUIRED.  No case may sit between SUPERSET and WIDE (BIG): the GPU test asserts the class each case states."""
    classes, union = set(), set()
    for c in tc.CASES:
        cls, tags = tc.observe(c)
        assert cls == c.cls, (c.name, c.cls, cls, sorted(tags))
        assert c.tags <= tags, (c.name, "the input no longer reaches", sorted(c.tags - tags))
        classes.add(c.cls)
        union |= c.tags
    assert classes == {tc.ALL, tc.SUPERSET, tc.WIDE, tc.ARGMAX, tc.NONE}
    assert not tc.REQUIRED - union, ("tags no case states: give them an input", sorted(tc.REQUIRED - union))
    assert union <= tc.REQUIRED, sorted(union - tc.REQUIRED)
    assert sum(c.V == tc.VQ for c in tc.CASES) == 1


def test_the_issue_table_of_nuclei():
    """rnd, rnd(sigma = 1), ties, flat and spaced(64) at k in {1, 20, 64, 1000}: nucleus == min(k, n0) with no cut, except spaced(64) at
    k >= 64, where the cut falls at 58 (the behaviour the GPU case table relies on)"""
    V = tc.VB
    for make in (lambda: pc.rnd(V, 16, sigma=1.0), lambda: pc.rnd(V, 17, "ties", 1.0), lambda: np.zeros(V, np.float32)):
        l = make()
        for k in (1, 20, 64, 1000):
            s = tr.sample(l, [], 1.0, 1.0, 0.99, 0.37, k)
            assert not s.cut and s.nucleus == min(k, s.n_candidates), (k, s)
    l = pc.spaced(tc.VT, 64)
    for k in (1, 20, 64, 1000):
        s = tr.sample(l, [], 1.0, 1.0, 0.9, 0.37, k)
        assert (s.cut, s.nucleus) == ((False, k) if k < 64 else (True, 58)), (k, s)
