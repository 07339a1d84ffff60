"""CPU tests of the sampler's restatement (tests/sampler_ref.py) and of the case table of tests/test_gpu_sampler_paths.py.

The restatement returns fields no other reference here returns (nucleus, the six most probable tokens, the denominator's bits at any
vocabulary, the chunks in which the denominator changes binade).  It is pinned from three sides: the compiled reference's golden, the
oracle's sampler on every case of the table, and the oracle's softmax bit for bit (the libm called through ctypes is the oracle's).
The closing test holds the table to what it states: every case reaches the class and the tags it names, and together the cases reach
every tag of sampler_path_cases.REQUIRED and every class."""
import os

import numpy as np
import pytest

from conftest import GOLD
import sampler_cases as sc
import sampler_path_cases as pc
import sampler_ref as sr

NAMES = [c.name for c in pc.CASES]


def test_restatement_vs_reference_golden():
    """tests/golden/sampler_logits.npz (the compiled reference, 12 vectors x 4 coins at V = 151 936): token, candidates, denominator bits"""
    g = np.load(os.path.join(GOLD, "sampler_logits.npz"))
    assert [repr(c) for c in sc.CASES] == [str(c) for c in g["cases"]]
    for ci, (seed, sigma, mode, rp, temp, top_p, nh) in enumerate(sc.CASES):
        l, h = sc.logits_of(seed, sigma, mode), sc.history_of(seed, nh)
        for ki, coin in enumerate(sc.COINS):
            s = sr.sample(l, h, rp, temp, top_p, coin)
            assert s.token == int(g["tokens"][ci, ki]), (ci, ki)
            if temp != 0.0:
                assert s.n_candidates == int(g["n_candidates"][ci]) and s.sum_bits == int(g["denominator_bits"][ci]), (ci, ki)


def test_sequential_sum_is_sequential():
    """step 5 rests on np.cumsum adding in index order in float32: against a plain loop, on addends of very different sizes"""
    e = (np.random.default_rng(2).random(5000) ** 8).astype(np.float32)
    s = np.float32(0.0)
    for v in e:
        s = np.float32(s + v)
    assert np.cumsum(e, dtype=np.float32)[-1].tobytes() == s.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_vs_oracle(oracle, name):
    """every case of the table: the probabilities equal the oracle's softmax bit for bit, token and candidate count equal the oracle's
    sampler for every coin.  (Without a candidate the reference and the oracle index probindex[-1]: only the count is compared, through
    the oracle's probabilities.)"""
    c = pc.BY_NAME[name]
    if c.temperature != 0.0:
        d, n = sr.parts(c.logits, c.history, c.penalty, c.temperature, c.top_p)
        p = oracle.softmax(d.y)
        assert np.array_equal(p.view(np.uint32), d.p.view(np.uint32))
        if n.n0 == 0:
            cutoff = np.float32((np.float32(1.0) - np.float32(c.top_p)) / np.float32(c.V - 1))
            assert not np.any(p >= cutoff) and all(c.ref(coin).none for coin in c.coins)
            return
    for coin in c.coins:
        tok, cnt = oracle.sample_logits(c.logits, c.history, c.penalty, c.temperature, c.top_p, coin)
        s = c.ref(coin)
        assert (s.token, s.n_candidates) == (tok, cnt), (coin, s.token, s.n_candidates, tok, cnt)
        if not s.argmax:
            d, n = sr.parts(c.logits, c.history, c.penalty, c.temperature, c.top_p)
            assert s.token == int(n.order[s.pick]) and s.pick <= s.last == s.nucleus - 1 < s.n_candidates
            assert s.top[:min(6, n.n0)] == tuple(int(t) for t in n.order[:6]) and all(t == 0 for t in s.top[n.n0:])


def test_cases_reach_what_they_state():
    """From the restatement alone: each case reaches its class and its tags; the union reaches every class and every tag of REQUIRED.
    (SUPERSET against WIDE with a nucleus that fits the sorter is the device's decision: BIG here, settled by the GPU test.)"""
    classes, union = set(), set()
    for c in pc.CASES:
        cls, tags = pc.observe(c)
        assert cls == c.cls or (cls == pc.BIG and c.cls in (pc.SUPERSET, pc.WIDE)), (c.name, c.cls, cls)
        assert c.tags <= tags, (c.name, "the input no longer reaches", sorted(c.tags - tags))
        classes.add(c.cls)
        union |= c.tags
    assert classes == {pc.ALL, pc.SUPERSET, pc.WIDE, pc.ARGMAX, pc.NONE}
    assert not pc.REQUIRED - union, ("tags no case states: give them an input", sorted(pc.REQUIRED - union))
    assert union <= pc.REQUIRED, sorted(union - pc.REQUIRED)
    # the V = 151 936 cases feed the mixed batch and the call-order test: every class must be there
    assert {c.cls for c in pc.CASES if c.V == pc.VQ} == classes
