"""GPU tests of every path of the device sampler (sampler.hip, sampler_wide.hip, backend_sampler.hip) at constructed edges, field by field.

tests/sampler_path_cases.py holds the inputs and what each means to reach; tests/sampler_ref.py is the reference (pinned on the CPU by
tests/test_sampler_ref.py).  Per case and coin the device's token, status, n_candidates, nucleus, top[6] and sum_bits equal the
restatement's -- integers, no tolerance -- then walked_chunks is at least the number of chunks in which the denominator changes binade
(such a chunk cannot be jumped; no upper bound, that would be a speed claim), then the result shows the class the case states.  Values
come first so that a path mismatch cannot hide a wrong token.  Then: the call after a call without a candidate, every ordered pair of
classes on one slot, histories interleaved with penalty-free calls, all five classes in one batch (and shuffled), a 64-coin ladder over a
radix-sorted list, and the vocabulary one past the declared limit."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import synth_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf
import sampler_path_cases as pc
import sampler_ref as sr

pytestmark = pytest.mark.gpu
OK, FALLBACK = 0, 1                  # NANO_SAMPLE_OK, NANO_SAMPLE_FALLBACK
CAP = pc.CAP


def model_file(model_dir, V):
    """bigvocab-qwen3 (one layer, E = 64) under a vocabulary of V: V * 256 bytes + the tokenizer section, written once"""
    if V == pc.VQ:
        return synth_model(model_dir, "bigvocab-qwen3", "f32", 0)[0]
    path = os.path.join(model_dir, f"bigvocab-qwen3-V{V}.bin")
    if not os.path.exists(path):
        mf.write_model(path, dataclasses.replace(mf.preset("bigvocab-qwen3"), vocab_size=V))
    return path


@pytest.fixture(scope="module")
def models(model_dir):
    """open(V, max_batch) -> the model of that vocabulary, opened once for the module"""
    opened = {}

    def open_(V, max_batch=1):
        if (V, max_batch) not in opened:
            opened[V, max_batch] = nb.load_model_file(model_file(model_dir, V), max_seq_len=512, max_batch=max_batch)
        return opened[V, max_batch]
    yield open_
    for m in opened.values():
        m.close()


def values(r):
    return (r.token, r.status, r.n_candidates, r.nucleus, tuple(r.top), r.sum_bits)


def fields(r):
    """everything the device reports that is defined for the row's status (without a candidate: no token, nucleus or top)"""
    if r.status == FALLBACK:
        return (r.status, r.n_candidates, r.n_sorted, r.sum_bits, r.walked_chunks)
    return values(r) + (r.n_sorted, r.walked_chunks)


def check(c, coin, r, where=()):
    """one device result against the restatement: values, then the walk, then the class"""
    s = c.ref(coin)
    at = (c.name, coin) + tuple(where)
    if s.argmax:
        assert (r.token, r.status) == (s.token, OK), (at, r.token, s.token)
        assert c.cls == pc.ARGMAX, at
        return
    if s.none:
        assert (r.status, r.n_candidates, r.sum_bits) == (FALLBACK, 0, s.sum_bits), (at, values(r))
        assert r.walked_chunks >= len(s.crossings), (at, r.walked_chunks, sorted(s.crossings))
        assert c.cls == pc.NONE, at
        return
    assert values(r) == (s.token, OK, s.n_candidates, s.nucleus, s.top, s.sum_bits), (at, values(r), s)
    assert r.walked_chunks >= len(s.crossings), (at, r.walked_chunks, sorted(s.crossings))
    got = (pc.ALL if r.n_sorted == r.n_candidates <= CAP else pc.WIDE if r.n_sorted == r.n_candidates else
           pc.SUPERSET if r.n_candidates > CAP and r.nucleus <= r.n_sorted < r.n_candidates else "?")
    assert got == c.cls, (at, f"reached {got} (n_sorted {r.n_sorted}, n_candidates {r.n_candidates}, nucleus {r.nucleus}), not {c.cls}: "
                              "the case needs a new input that reaches its class, not a weaker assertion")


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_case(models, name):
    c = pc.BY_NAME[name]
    m = models(c.V)
    for coin in c.coins:
        check(c, coin, m.op_sample(c.logits, c.history, *c.row(coin)[:4]))


def one(m, c, coin):
    return m.op_sample(c.logits, c.history, *c.row(coin)[:4])


@pytest.mark.parametrize("none,then", [("none-flat", "top_p=0"), ("none-flat", "cap-K8192"), ("none-V2", "vocab-2-ties")])
def test_call_after_no_candidate(models, none, then):
    """NANO_SAMPLE_FALLBACK with n_candidates == 0 (nano_mi355x.h), and the next call on the slot -- every candidate sorted in LDS, through the
    cells the declined call re-armed on its early return -- is right"""
    a, b = pc.BY_NAME[none], pc.BY_NAME[then]
    assert a.cls == pc.NONE and b.cls == pc.ALL and a.V == b.V
    m = models(a.V)
    for coin in b.coins:
        check(a, a.coins[0], one(m, a, a.coins[0]))
        check(b, coin, one(m, b, coin), ("after", none))


# (two supersets: the largest dropped probability of one call must not survive into the next one's check of its cut)
REPS = [(pc.ALL, "cap-K8191"), (pc.SUPERSET, "levels-superset"), (pc.SUPERSET, "masked-6/7"), (pc.WIDE, "wide-16384-cut8191"),
        (pc.ARGMAX, "argmax-tie-pos-pen>1"), (pc.NONE, "none-flat")]


def test_every_order_of_two_classes_on_one_slot(models):
    """samp_pick re-arms ncand / ndrop / dropmax and the bins (on its early returns too), the wide cut re-arms ncand, the radix sort's totals
    are cleared per call: one representative of each class after each class (itself included), both calls against the restatement"""
    m = models(pc.VQ)
    reps = [pc.BY_NAME[v] for _, v in REPS]
    assert all(c.cls == k and c.V == pc.VQ for (k, _), c in zip(REPS, reps))
    for first in reps:
        for second in reps:
            check(first, first.coins[-1], one(m, first, first.coins[-1]), ("before", second.name))
            check(second, second.coins[1 % len(second.coins)], one(m, second, second.coins[1 % len(second.coins)]), ("after", first.name))


def test_histories_interleaved_with_penalty_free_calls(models):
    """the slot's record of marked ids: a penalty call, a penalty-free call with an unrelated history (its history is not read and must not
    disturb the record), a penalty call whose history extends the first, one whose history is a prefix of it (the set starts over)"""
    m = models(pc.VQ)
    V = pc.VQ
    la, lb = pc.rnd(V, 31), pc.rnd(V, 32, "ties")
    A = pc.hist(V, 77, 40)
    A2 = np.concatenate([A, pc.hist(V, 78, 5)]).astype(np.uint32)
    # make sure the histories matter: the most probable tokens are in them
    A[:3] = np.argsort(-la)[:3]
    A2[:3] = A[:3]; A2[-2:] = np.argsort(-lb)[:2]
    B = pc.hist(V, 79, 25)
    calls = [(la, A, 1.5, 0.8, 0.9, 0.4), (lb, B, 1.0, 1.0, 0.9, 0.6), (lb, A2, 1.5, 0.8, 0.9, 0.2), (la, A2, 1.0, 0.0, 0.9, 0.0),
             (la, A[:7], 1.5, 0.8, 0.9, 0.7), (lb, A, 0.7, 0.0, 0.9, 0.0), (la, A2, 0.7, 1.2, 0.5, 0.9)]
    for k, (l, h, rp, temp, top_p, coin) in enumerate(calls):
        s = sr.sample(l, h, rp, temp, top_p, coin)
        r = m.op_sample(l, h, rp, temp, top_p, coin)
        if s.argmax:
            assert (r.token, r.status) == (s.token, OK), k
        else:
            assert values(r) == (s.token, OK, s.n_candidates, s.nucleus, s.top, s.sum_bits), (k, values(r), s)
    assert sr.sample(la, A, 1.5, 0.8, 0.9, 0.4).top != sr.sample(la, [], 1.0, 0.8, 0.9, 0.4).top


def batch_rows():
    """(case, coin) of every V = 151 936 case, then further coins of the cases beyond the LDS sorter, 64 rows"""
    cs = [c for c in pc.CASES if c.V == pc.VQ]
    rows = [(c, c.coins[i % len(c.coins)]) for i, c in enumerate(cs)]
    more = [(c, coin) for c in cs if c.cls in (pc.WIDE, pc.SUPERSET) for coin in c.coins[::-1]]
    rows += [rc for rc in more if rc not in rows][:64 - len(rows)]
    return rows[:64]


def test_mixed_batch(models):
    """all five classes in one op_sample_batch call of 64 rows and in a shuffled order: each row equals the restatement, and the one-row
    call, field by field"""
    m = models(pc.VQ, 64)
    rows = batch_rows()
    assert len(rows) == 64 and {c.cls for c, _ in rows} == {pc.ALL, pc.SUPERSET, pc.WIDE, pc.ARGMAX, pc.NONE}
    L = np.stack([c.logits for c, _ in rows])
    got = m.op_sample_batch(L, [c.row(coin) for c, coin in rows])
    for i, ((c, coin), r) in enumerate(zip(rows, got)):
        check(c, coin, r, ("row", i))
    perm = np.random.default_rng(1).permutation(len(rows))
    shuffled = m.op_sample_batch(L[perm], [rows[i][0].row(rows[i][1]) for i in perm])
    for j, i in enumerate(perm):
        check(rows[i][0], rows[i][1], shuffled[j], ("shuffled row", j))
        assert fields(shuffled[j]) == fields(got[i]), (rows[i][0].name, i, j)
    for i, (c, coin) in enumerate(rows):
        assert fields(one(m, c, coin)) == fields(got[i]), (c.name, i)


def test_coin_ladder_over_the_radix_sort(models):
    """a noisy near-flat vector (every token a candidate, 127 k in the nucleus) under 64 coins in one batch: each token is entry `pick` of
    the restatement's sorted list -- 64 positions of the radix sort's output, draws in front of and inside the cut's chunk"""
    m = models(pc.VQ, 64)
    c = pc.BY_NAME["wide-noisy"]
    coins = [float(np.float32((k + 0.5) / 64.0)) for k in range(62)] + [pc.ALMOST1, 1.0]      # (the last two draw the cut's own entry)
    d, n = sr.parts(c.logits, c.history, c.penalty, c.temperature, c.top_p)
    got = m.op_sample_batch(np.broadcast_to(c.logits, (64, c.V)), [c.row(coin) for coin in coins])
    picks = set()
    for coin, r in zip(coins, got):
        s = c.ref(coin)
        check(c, coin, r)
        assert r.token == int(n.order[s.pick]), (coin, s.pick)
        picks.add(s.pick // pc.CHUNK)
    assert len(picks) == 63 and n.last // pc.CHUNK in picks and min(picks) < n.last // pc.CHUNK


def test_vocabulary_past_the_limit_is_refused(models):
    """V = SAMPLE_MAX_CHUNKS * 256 + 1: the sampler declines with an error, the model goes on serving forwards"""
    m = models(pc.VMAX + 1)
    l = np.zeros(pc.VMAX + 1, np.float32)
    with pytest.raises(nb.NanoHipError, match="too large for the device sampler"):
        m.op_sample(l, [], 1.0, 1.0, 0.9, 0.5)
    logits, _ = m.forward([1], [0])
    assert logits.shape == (1, pc.VMAX + 1) and np.all(np.isfinite(logits)) and float(np.abs(logits).max()) > 0.0
    with pytest.raises(nb.NanoHipError, match="too large for the device sampler"):
        m.op_sample(l, [], 1.0, 0.0, 0.9, 0.0)
