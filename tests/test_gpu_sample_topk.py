"""GPU tests of the device sampler's top-k truncation (nano_hip_op_sample_batch_ex) against the restatement, field by field.

tests/sampler_topk_cases.py holds the inputs and what each reaches; tests/sampler_topk_ref.py is the reference (pinned on the CPU by
tests/test_sampler_topk_ref.py).  Per case and coin (0, 0.37, the largest float below 1) the device's token, status, n_candidates, nucleus,
top[6] and sum_bits equal the restatement's -- integers, no tolerance; walked_chunks and sum_bits equal those of the top_k = 0 call; then
the result shows the class the case states, so a row cannot pass by declining: only the constructed no-candidate case may end in
NANO_SAMPLE_FALLBACK.  Then what the table of the cases promises per tag, and rows of different top_k in one call."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import synth_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf
import sampler_path_cases as pc
import sampler_ref as sr
import sampler_topk_cases as tc
import sampler_topk_ref as tr

pytestmark = pytest.mark.gpu
OK, FALLBACK = 0, 1
CAP = tc.CAP


def model_file(model_dir, V):
    """tiny-qwen3 serves its own vocabulary; bigvocab-qwen3 (one layer, E = 64) the others, under a vocabulary of V"""
    if V == tc.VT:
        return synth_model(model_dir, "tiny-qwen3", "f32", 0)[0]
    if V == tc.VQ:
        return synth_model(model_dir, "bigvocab-qwen3", "f32", 0)[0]
    path = os.path.join(model_dir, f"bigvocab-qwen3-V{V}.bin")
    if not os.path.exists(path):
        mf.write_model(path, dataclasses.replace(mf.preset("bigvocab-qwen3"), vocab_size=V))
    return path


@pytest.fixture(scope="module")
def models(model_dir):
    opened = {}

    def open_(V, max_batch=1):
        if (V, max_batch) not in opened:
            opened[V, max_batch] = nb.load_model_file(model_file(model_dir, V), max_seq_len=64, max_batch=max_batch)
        return opened[V, max_batch]
    yield open_
    for m in opened.values():
        m.close()


def values(r):
    return (r.token, r.status, r.n_candidates, r.nucleus, tuple(r.top), r.sum_bits)


def fields(r):
    """everything the device reports that is defined for the row's status"""
    if r.status == FALLBACK:
        return (r.status, r.n_candidates, r.sum_bits, r.walked_chunks)
    return values(r) + (r.walked_chunks,)


def reached(r):
    return (tc.ALL if r.n_sorted == r.n_candidates <= CAP else tc.WIDE if r.n_sorted == r.n_candidates else
            tc.SUPERSET if r.n_candidates > CAP and r.nucleus <= r.n_sorted < r.n_candidates else "?")


def check(c, coin, r, where=()):
    """one device result against the restatement: values first, then the class"""
    s = c.ref(coin)
    at = (c.name, coin) + tuple(where)
    if s.argmax:
        assert (r.token, r.status) == (s.token, OK), (at, r.token, s.token)
        assert c.cls == tc.ARGMAX, at
        return s
    if s.none:
        assert (r.status, r.n_candidates, r.sum_bits) == (FALLBACK, 0, s.sum_bits), (at, values(r))
        assert c.cls == tc.NONE, at
        return s
    assert values(r) == (s.token, OK, s.n_candidates, s.nucleus, s.top, s.sum_bits), (at, values(r), s)
    assert r.n_sorted >= r.nucleus and r.nucleus <= max(c.top_k, 1), (at, r.n_sorted, r.nucleus)
    assert reached(r) == c.cls, (at, f"reached {reached(r)} (n_sorted {r.n_sorted}, n_candidates {r.n_candidates}, nucleus {r.nucleus}), not {c.cls}")
    return s


def one(m, c, coin, top_k=None):
    return m.op_sample(c.logits, c.history, *c.row(coin)[:4], top_k=c.top_k if top_k is None else top_k)


@pytest.mark.parametrize("name", [c.name for c in tc.CASES])
def test_case(models, name):
    c = tc.BY_NAME[name]
    m = models(c.V)
    for coin in c.coins:
        r = one(m, c, coin)
        s = check(c, coin, r)
        off = m.op_sample(c.logits, c.history, *c.row(coin)[:4])                     # the entry point without top_k
        if c.cls != tc.ARGMAX:
            assert (r.sum_bits, r.walked_chunks, r.n_candidates) == (off.sum_bits, off.walked_chunks, off.n_candidates), (name, coin)
        if "k>=n0" in c.tags:
            assert fields(r) == fields(off) and r.n_sorted == off.n_sorted, (name, coin, "k >= n_candidates must change nothing")
        if "p-binds" in c.tags:
            assert s.cut and r.nucleus < c.top_k and values(r) == values(off), (name, coin, "the cut in front of entry k - 1: the top_k = 0 result")
        if "k-binds" in c.tags:
            d, n = sr.parts(c.logits, c.history, c.penalty, c.temperature, c.top_p)
            assert not s.cut and r.nucleus == c.top_k < r.n_candidates, (name, coin)
            assert np.float32(s.r) == np.float32(coin) * n.cdf[c.top_k - 1], (name, coin, "r = coin * cdf[k - 1]")
            assert r.token == int(n.order[s.pick]) and s.pick < c.top_k and r.token in set(int(t) for t in n.order[:c.top_k])
        if "k=1" in c.tags:
            d, n = sr.parts(c.logits, c.history, c.penalty, c.temperature, c.top_p)
            assert r.token == int(n.order[0]) == int(np.argmax(d.p)), (name, coin, "the first maximum")
        if "k<6" in c.tags:
            assert all(t == 0 for t in r.top[c.top_k:]) and tuple(r.top[:c.top_k]) == s.top[:c.top_k], (name, coin, tuple(r.top))
        if "tie@k" in c.tags:
            d, n = sr.parts(c.logits, c.history, c.penalty, c.temperature, c.top_p)
            inside, outside = int(n.order[c.top_k - 1]), int(n.order[c.top_k])
            assert d.p[inside] == d.p[outside] and inside < outside, (name, "equal probabilities: the lower index is inside")
        if "penalised" in c.tags:
            assert tuple(r.top) != tr.sample(c.logits, [], 1.0, c.temperature, c.top_p, coin, c.top_k).top, (name, "the penalty moved the list")
        if c.cls == tc.ARGMAX:
            assert r.token == off.token == one(m, c, coin, top_k=1).token, (name, "temperature 0 ignores top_k")


def test_equal_maxima_lower_index(models):
    c = tc.BY_NAME["k1-tied-maxima"]
    for coin in c.coins:
        assert one(models(c.V), c, coin).token == 300


def test_last_draw_of_a_k_bound_list(models):
    """coin ~ 1 draws the list's last entry, entry k - 1 of the stable order; coin 0 the first"""
    for name in ("k-binds-k20", "big-rnd-k1000", "flat-k20", "tie@k-spaced"):
        c = tc.BY_NAME[name]
        d, n = sr.parts(c.logits, c.history, c.penalty, c.temperature, c.top_p)
        m = models(c.V)
        assert one(m, c, 1.0).token == int(n.order[c.top_k - 1]), name
        assert one(m, c, 0.0).token == int(n.order[0]), name


def test_rows_with_different_top_k_in_one_call(models):
    """rows of top_k 0, 1, 20 and V (and the wide, certified-superset and no-candidate classes) in one call: each row equals the one-row call
    and the restatement"""
    m = models(tc.VB, 8)
    rows = [("big-rnd-k20", 0.37, 0), ("big-rnd-k20", 0.37, 1), ("big-rnd-k20", 0.37, 20), ("big-rnd-k20", 0.37, tc.VB),
            ("flat-k20", tc.ALMOST1, 20), ("bin-end-k20", 0.0, 20), ("none-flat-k20", 0.37, 20), ("penalty-big-k20", 0.37, 20)]
    cs = [tc.BY_NAME[n] for n, _, _ in rows]
    got = m.op_sample_batch(np.stack([c.logits for c in cs]), [c.row(coin) for c, (_, coin, _) in zip(cs, rows)], top_k=[k for _, _, k in rows])
    for i, (c, (name, coin, k)) in enumerate(zip(cs, rows)):
        s = c.ref(coin, top_k=k)
        alone = m.op_sample_batch(c.logits.reshape(1, -1), [c.row(coin)], top_k=[k])[0]
        assert fields(got[i]) == fields(alone), (i, name, k)
        if s.none:
            assert (got[i].status, got[i].n_candidates) == (FALLBACK, 0), (i, name)
        else:
            assert values(got[i]) == (s.token, OK, s.n_candidates, s.nucleus, s.top, s.sum_bits), (i, name, k, values(got[i]), s)
    # the first row (top_k = 0) is the entry point without top_k, record for record
    off = m.op_sample(cs[0].logits, cs[0].history, *cs[0].row(0.37)[:4])
    assert fields(got[0]) + (got[0].n_sorted,) == fields(off) + (off.n_sorted,)
    # a reversed call: every slot sees another class than before
    back = m.op_sample_batch(np.stack([c.logits for c in cs[::-1]]), [c.row(coin) for c, (_, coin, _) in zip(cs[::-1], rows[::-1])],
                             top_k=[k for _, _, k in rows[::-1]])
    assert [fields(r) for r in back[::-1]] == [fields(r) for r in got]


def test_reserved_words_are_refused(models):
    m = models(tc.VT)
    arr, _keep = nb.sample_params_ex([(1.0, 1.0, 0.9, 0.5, [])], 5)
    out = (nb.NanoHipSample * 1)()
    l = np.zeros(tc.VT, np.float32)
    for w in range(3):
        arr[0].reserved[w] = 1
        assert nb.lib().nano_hip_op_sample_batch_ex(m.h, l, 1, arr, out) == -1 and "reserved" in nb.last_error()
        arr[0].reserved[w] = 0
    assert nb.lib().nano_hip_op_sample_batch_ex(m.h, l, 1, arr, out) == 0 and out[0].status == OK and out[0].nucleus == 5
