"""CPU tests of the restatement of the sampler with logit edits (tests/logit_edit_ref.py): equal to sampler_topk_ref.sample without an edit
on every constructed case, equal to it on the edited logits for top_p < 1 over the overlays of tests/logit_edit_cases.py, and different
from it in the one stated way -- a disallowed token is never a candidate -- at top_p = 1."""
import numpy as np
import pytest

import logit_edit_cases as ec
import logit_edit_ref as er
import sampler_path_cases as pc
import sampler_topk_cases as tc
import sampler_topk_ref as tr


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_no_edit_equals_the_sampler_on_path_cases(name):
    c = pc.BY_NAME[name]
    for coin in c.coins:
        assert er.sample(c.logits, c.history, c.penalty, c.temperature, c.top_p, coin) == \
            tr.sample(c.logits, c.history, c.penalty, c.temperature, c.top_p, coin), (name, coin)


@pytest.mark.parametrize("name", [c.name for c in tc.CASES])
def test_no_edit_equals_the_sampler_on_topk_cases(name):
    c = tc.BY_NAME[name]
    for coin in c.coins:
        assert er.sample(c.logits, c.history, c.penalty, c.temperature, c.top_p, coin, c.top_k) == c.ref(coin), (name, coin)


@pytest.mark.parametrize("name", [o.name for o in ec.OVERLAYS if o.top_p < 1.0])
def test_top_p_below_1_equals_the_sampler_on_the_edited_logits(name):
    o = ec.BY_NAME[name]
    on = o.on()
    for coin in o.coins:
        s = o.ref(coin)
        assert s == tr.sample(o.edited(), o.history, o.penalty, o.temperature, o.top_p, coin, o.top_k), (name, coin)
        assert on[s.token], (name, coin, s.token)
        if not s.argmax:
            assert all(on[t] for t in s.top[:min(6, s.n_candidates, o.top_k or 6)]), (name, coin, s.top)


def test_edited_keeps_bits_without_an_entry_and_adds_once_with_one():
    l = np.array([-0.0, 1.5, np.float32(1e-8), 3.0, 2.0], np.float32)
    x = er.edited(l, er.words(np.array([0, 1, 2, 3]), 5), (np.array([3, 1]), np.array([0.25, np.float32(1e-8)], np.float32)))
    want = np.array([-0.0, np.float32(1.5) + np.float32(1e-8), np.float32(1e-8), 3.25, -np.inf], np.float32)
    assert np.array_equal(x.view(np.uint32), want.view(np.uint32))                # -0.0 stays -0.0: no add without an entry
    assert np.array_equal(er.edited(l).view(np.uint32), l.view(np.uint32))
    # dead bits of the last word are ignored
    w = er.words(np.array([4]), 5)
    w[0] |= 0xFFFFFFE0
    assert er.allowed(w, 5).tolist() == [False, False, False, False, True]


def test_words_and_allowed_round_trip():
    for V in (5, 32, 33, 1024, 9000):
        on = np.random.default_rng(V).random(V) < 0.3
        w = er.words(on, V)
        assert w.size == -(-V // 32) and np.array_equal(er.allowed(w, V), on)
        assert np.array_equal(er.words(np.nonzero(on)[0], V), w)
        j = int(np.nonzero(on)[0][-1])
        assert (int(w[j >> 5]) >> (j & 31)) & 1


def test_top_p_1_four_allowed_the_filter_bites():
    """the one stated difference: at top_p = 1 the unfiltered sampler on the edited logits counts every token a candidate and can return a
    disallowed one; the restatement cannot"""
    V = 1000
    l, ids, w = ec.four_allowed(V)
    lp = er.edited(l, w)
    on = er.allowed(w, V)
    # the unfiltered reference: all V tokens are candidates (p >= 0), the p = 0 ones follow the four in index order
    u = tr.sample(lp, [], 1.0, 1.0, 1.0, 1.0)
    assert u.n_candidates == V and not on[u.top[4]] and not on[u.top[5]]
    assert not on[u.token] and u.token == V - 1, u.token                         # coin 1: r == the sum, the sorted list's last entry
    # the restatement: four candidates, the last allowed token of the sorted order
    s = er.sample(l, [], 1.0, 1.0, 1.0, 1.0, allow=w)
    order = ids[np.argsort(-l[ids], kind="stable")]
    assert s.n_candidates == 4 and s.top[4:6] == (0, 0) and s.top[:4] == tuple(int(t) for t in order)
    assert s.token == int(order[-1]) and on[s.token]
    for coin in (0.0, 0.37, pc.ALMOST1):
        assert on[er.sample(l, [], 1.0, 1.0, 1.0, coin, allow=w).token]
