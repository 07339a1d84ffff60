"""GPU tests of the device sampler's logit edits (nano_hip_op_sample_batch_edit) against the restatement, field by field.

tests/logit_edit_cases.py holds the overlays, tests/logit_edit_ref.py the reference (pinned on the CPU by tests/test_logit_edit_ref.py).
Per overlay and coin (0, 0.37, the largest float below 1) the device's token, status, n_candidates, nucleus, top[6] and sum_bits equal the
restatement's -- integers, no tolerance -- and for top_p < 1 every field, n_sorted and walked_chunks included, equals the device's own
_ex call on host-edited logits.  Rows without an edit equal _ex rows in every field.  Then the top_p = 1 difference, the mask table,
rows of different edits in one call, a random sweep (every OK token is allowed) and the refusals."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import synth_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf
import logit_edit_cases as ec
import logit_edit_ref as er
import sampler_path_cases as pc
import sampler_topk_cases as tc

pytestmark = pytest.mark.gpu
OK, FALLBACK = 0, 1
CAP = tc.CAP
VT, VB = ec.VT, ec.VB


def model_file(model_dir, V):
    """tiny-qwen3 serves its own vocabulary; bigvocab-qwen3 (one layer, E = 64) the others, under a vocabulary of V"""
    if V == VT:
        return synth_model(model_dir, "tiny-qwen3", "f32", 0)[0]
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


def every(r):
    """every field of a result that is defined for its status (a temperature-0 row reports its token and zeros; a declined row leaves
    token, nucleus and top[] unspecified)"""
    if r.status == FALLBACK:
        return (r.status, r.n_candidates, r.sum_bits, r.n_sorted, r.walked_chunks)
    return values(r) + (r.n_sorted, r.walked_chunks)


def reached(r):
    return (tc.ALL if r.n_sorted == r.n_candidates <= CAP else tc.WIDE if r.n_sorted == r.n_candidates else
            tc.SUPERSET if r.n_candidates > CAP and r.nucleus <= r.n_sorted < r.n_candidates else "?")


def run(m, o, coin, edit="own"):
    e = o.edit() if edit == "own" else edit
    return m.op_sample_batch(o.logits.reshape(1, -1), [o.row(coin)], top_k=[o.top_k], edits=[e])[0]


def against_ref(o, coin, r):
    s = o.ref(coin)
    if s.argmax:
        assert (r.token, r.status) == (s.token, OK), (o.name, coin, r.token, s.token)
    else:
        assert not s.none, o.name
        assert values(r) == (s.token, OK, s.n_candidates, s.nucleus, s.top, s.sum_bits), (o.name, coin, values(r), s)
    assert o.on()[r.token], (o.name, coin, r.token)
    return s


# ---- 1. rows without an edit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k-binds-k20", "big-rnd-k20", "flat-k20", "argmax-k7", "none-flat-k20"])     # ALL, SUPERSET, WIDE, ARGMAX, NONE
def test_rows_without_an_edit_are_ex_rows(models, name):
    c = tc.BY_NAME[name]
    m = models(c.V)
    some = ec.BY_NAME[f"mask-and-bias-V{VB if c.V == VB else VT}"]
    for coin in c.coins:
        ex = m.op_sample_batch(c.logits.reshape(1, -1), [c.row(coin)], top_k=[c.top_k])[0]
        for edits in ([None], [{}], [{"allow": None, "bias": None}]):
            r = m.op_sample_batch(c.logits.reshape(1, -1), [c.row(coin)], top_k=[c.top_k], edits=edits)[0]
            assert every(r) == every(ex), (name, coin, edits)
        if c.cls not in (tc.ARGMAX, tc.NONE):
            assert reached(ex) == c.cls, (name, reached(ex))
        # ... and behind an edited call on the same slot (the staging has changed hands by then)
        run(m, some, 0.37)
        r = m.op_sample_batch(c.logits.reshape(1, -1), [c.row(coin)], top_k=[c.top_k], edits=[None])[0]
        assert every(r) == every(ex), (name, coin, "after an edited call")
        assert every(m.op_sample_batch(c.logits.reshape(1, -1), [c.row(coin)], top_k=[c.top_k])[0]) == every(ex), (name, coin)


# ---- 2. edited rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [o.name for o in ec.OVERLAYS])
def test_overlay(models, name):
    o = ec.BY_NAME[name]
    m = models(o.V)
    lp = o.edited()
    for coin in o.coins:
        r = run(m, o, coin)
        against_ref(o, coin, r)
        if o.top_p < 1.0:
            ex = m.op_sample_batch(lp.reshape(1, -1), [o.row(coin)], top_k=[o.top_k])[0]
            assert every(r) == every(ex), (name, coin, every(r), every(ex))


def test_what_the_overlays_reach(models):
    """the classes the issue names: five allowed of a flat row are sorted in LDS; 8437 allowed run the wide phase with the filter; a mask
    over random logits at V = 9000 stays a certified superset"""
    m = models(VB)
    r = run(m, ec.BY_NAME["flat-five-allowed-V9000"], 0.37)
    assert reached(r) == tc.ALL and r.n_candidates == 5 and sorted(r.top[:5]) == [3, 1000, 4095, 4096, 8999] and r.top[5] == 0
    assert reached(m.op_sample_batch(np.zeros((1, VB), np.float32), [(1.0, 1.0, 0.9, 0.37, [])])[0]) == tc.WIDE      # the same row unedited
    o = ec.BY_NAME["flat-16th-banned-top_p1-V9000"]
    for coin in o.coins + (1.0,):
        r = run(m, o, coin)
        against_ref(o, coin, r)
        assert reached(r) == tc.WIDE and r.n_candidates == 8437 and r.status == OK and r.token % 16 != 0, (coin, every(r))
        assert all(t % 16 for t in r.top), tuple(r.top)
    r = run(m, ec.BY_NAME["mask-0x55555555-V9000"], 0.37)
    assert r.n_candidates > 4000 and r.status == OK


# ---- 3. top_p = 1 with four allowed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [VT, VB])
def test_top_p_1_four_allowed(models, V):
    m = models(V)
    l, ids, w = ec.four_allowed(V)
    order = ids[np.argsort(-l[ids], kind="stable")]
    for coin in (0.0, 0.37, pc.ALMOST1, 1.0):
        r = m.op_sample_batch(l.reshape(1, -1), [(1.0, 1.0, 1.0, coin, [])], edits=[{"allow": w}])[0]
        s = er.sample(l, [], 1.0, 1.0, 1.0, coin, allow=w)
        assert values(r) == (s.token, OK, 4, s.nucleus, s.top, s.sum_bits), (V, coin, values(r), s)
        assert r.n_candidates == 4 and tuple(r.top[4:6]) == (0, 0) and tuple(r.top[:4]) == tuple(int(t) for t in order)
        assert r.token in ids
    assert m.op_sample_batch(l.reshape(1, -1), [(1.0, 1.0, 1.0, 1.0, [])], edits=[{"allow": w}])[0].token == int(order[-1])
    # the unfiltered sampler on the edited logits does return a disallowed token here: the filter is what keeps it out
    u = m.op_sample_batch(er.edited(l, w).reshape(1, -1), [(1.0, 1.0, 1.0, 1.0, [])])[0]
    assert u.status == OK and u.token not in ids and u.n_candidates == V


# ---- 4. the table and batching --------------------------------------------------------------------------------------------------------
def test_mask_table_and_per_call_masks_agree(models):
    m = models(VB)
    names = ["mask-nibbles-V9000", "mask-tail-word-V9000", "mask-all-but-argmax-V9000"]
    os_ = [ec.BY_NAME[n] for n in names]
    m.set_mask_table(np.stack([o.allow for o in os_]))
    try:
        for k, o in enumerate(os_):
            for coin in o.coins:
                assert every(run(m, o, coin, {"mask_id": k + 1})) == every(run(m, o, coin)), (o.name, coin)
        # a table mask with a per-call bias list
        o = ec.BY_NAME["mask-and-bias-V9000"]
        m.set_mask_table(np.stack([os_[0].allow, o.allow]))
        assert every(run(m, o, 0.37, {"mask_id": 2, "bias": o.bias})) == every(run(m, o, 0.37))
        # replacing the table changes the next call: id 1 was the nibble pattern, now it is the tail word
        o = os_[0]
        before = run(m, o, 0.37, {"mask_id": 1})
        m.set_mask_table(os_[1].allow.reshape(1, -1))
        after = run(m, o, 0.37, {"mask_id": 1})
        assert every(after) == every(run(m, os_[1], 0.37)) and 8992 <= after.token < 9000 and every(after) != every(before)
    finally:
        m.set_mask_table(None)
    with pytest.raises(nb.NanoHipError):
        run(m, os_[0], 0.37, {"mask_id": 1})                                       # the table is gone


def test_rows_with_different_edits_in_one_call(models):
    m = models(VB, 4)
    names = ["mask-and-bias-V9000", "bias-max-shuffled-V9000", "flat-five-allowed-V9000", "mask-t0-all-but-argmax-V9000"]
    sets = [names, names[::-1], ["mask-tail-word-V9000", None, "flat-16th-banned-top_p1-V9000", "bias-edges-V9000"]]
    plain = tc.BY_NAME["big-rnd-k20"]
    m.set_mask_table(ec.BY_NAME["mask-nibbles-V9000"].allow.reshape(1, -1))
    try:
        for rows in sets:
            os_ = [ec.BY_NAME[n] if n else None for n in rows]
            logits = np.stack([o.logits if o else plain.logits for o in os_])
            prm = [o.row(0.37) if o else plain.row(0.37) for o in os_]
            ks = [o.top_k if o else plain.top_k for o in os_]
            edits = [o.edit() if o else None for o in os_]
            got = m.op_sample_batch(logits, prm, top_k=ks, edits=edits)
            for i, o in enumerate(os_):
                alone = m.op_sample_batch(logits[i:i + 1], [prm[i]], top_k=[ks[i]], edits=[edits[i]])[0]
                assert every(got[i]) == every(alone), (rows, i)
                if o:
                    against_ref(o, 0.37, got[i])
                else:
                    assert every(got[i]) == every(m.op_sample_batch(logits[i:i + 1], [prm[i]], top_k=[ks[i]])[0]), (rows, i)
        # table ids and per-call masks side by side
        o = ec.BY_NAME["mask-nibbles-V9000"]
        got = m.op_sample_batch(np.stack([o.logits] * 3), [o.row(0.37)] * 3, edits=[{"mask_id": 1}, o.edit(), None])
        assert every(got[0]) == every(got[1]) != every(got[2])
    finally:
        m.set_mask_table(None)


# ---- 5. a random sweep: every OK token is allowed --------------------------------------------------------------------------------------
def test_random_edits_never_return_a_disallowed_token(models):
    m = models(VT, 4)
    rng = np.random.default_rng(2024)
    n_ok = 0
    for call in range(50):
        logits, prm, ks, edits, ons = [], [], [], [], []
        for _ in range(4):
            l = (rng.normal(0.0, rng.choice([0.3, 1.0, 3.0]), VT)).astype(np.float32)
            kind = rng.integers(4)
            on = np.ones(VT, bool)
            if kind != 3:
                on = rng.random(VT) < rng.choice([0.004, 0.1, 0.5, 0.97])
                on[rng.integers(VT)] = True
            nb_ = int(rng.choice([0, 1, 17, 300, 1024]))
            toks = rng.permutation(VT)[:nb_]
            vals = rng.normal(0.0, 4.0, nb_).astype(np.float32)
            if nb_ and rng.random() < 0.3:
                vals[0] = -np.inf
                on[toks[-1]] = True                                               # (keep one allowed token finite)
            logits.append(l)
            prm.append((float(rng.choice([1.0, 1.1])), float(rng.choice([0.0, 0.7, 1.0])), float(rng.choice([0.0, 0.9, 1.0])),
                        float(rng.choice([0.0, rng.random(), pc.ALMOST1, 1.0])), rng.integers(0, VT, 12).astype(np.uint32)))
            ks.append(int(rng.choice([0, 3])))
            edits.append({"allow": er.words(on, VT) if kind != 3 else None, "bias": (toks, vals)})
            ons.append(on)
        got = m.op_sample_batch(np.stack(logits), prm, top_k=ks, edits=edits)
        for i, r in enumerate(got):
            if r.status == OK:
                n_ok += 1
                assert ons[i][r.token], (call, i, r.token, prm[i][:4], ks[i])
                s = er.sample(logits[i], prm[i][4], prm[i][0], prm[i][1], prm[i][2], prm[i][3], ks[i], edits[i]["allow"], edits[i]["bias"])
                assert r.token == s.token, (call, i, r.token, s.token)
    assert n_ok >= 190, n_ok                                                       # (top_p = 0 over a near-flat row may leave no candidate)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause(models):
    m = models(VB)
    o = ec.BY_NAME["mask-and-bias-V9000"]
    l, row = o.logits.reshape(1, -1), [o.row(0.37)]
    W = -(-VB // 32)
    m.set_mask_table(np.stack([o.allow, o.allow]))
    dead = np.zeros(W, np.uint32)
    dead[-1] = 0xFFFFFF00                                                          # only bits of tokens >= V
    toks = np.arange(nb.NANO_BIAS_MAX + 1)

    def refused(edit, word):
        with pytest.raises(nb.NanoHipError) as e:
            m.op_sample_batch(l, row, edits=[edit])
        assert "error -1:" in str(e.value) and word in str(e.value), (edit.keys(), str(e.value))

    try:
        refused({"allow": o.allow, "mask_id": 1}, "both")
        refused({"mask_id": 3}, "beyond the mask table")
        refused({"allow": np.zeros(W, np.uint32)}, "allows no token")
        refused({"allow": dead}, "allows no token")
        refused({"bias": (toks, np.zeros(toks.size, np.float32))}, "NANO_BIAS_MAX")
        refused({"bias": ([VB], [1.0])}, "out of vocabulary")
        refused({"bias": ([5, 9, 5], [1.0, 2.0, 3.0])}, "listed twice")
        refused({"bias": ([5], [np.nan])}, "NaN or +inf")
        refused({"bias": ([5], [np.inf])}, "NaN or +inf")
        # n_bias > 0 with a null list: only the raw call can say that
        arr, _keep = nb.sample_params_edit(row, 0, [None])
        arr[0].n_bias = 4
        out = (nb.NanoHipSample * 1)()
        assert nb.lib().nano_hip_op_sample_batch_edit(m.h, l.reshape(-1), 1, arr, out) == -1 and "null bias list" in nb.last_error()
        # a failed table call leaves the old table in place
        with pytest.raises(nb.NanoHipError) as e:
            m.set_mask_table(np.stack([o.allow, dead]))
        assert "allows no token" in str(e.value)
        with pytest.raises(nb.NanoHipError):
            m.set_mask_table(np.zeros((1, W), np.uint32))
        assert every(run(m, o, 0.37, {"mask_id": 2, "bias": o.bias})) == every(run(m, o, 0.37))
        # a following valid call works, and a -inf bias is no refusal
        r = run(m, o, 0.37, {"allow": o.allow, "bias": ([int(np.argmax(o.edited()))], [-np.inf])})
        assert r.status == OK and o.on()[r.token]
    finally:
        m.set_mask_table(None)
