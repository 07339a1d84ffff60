"""GPU tests of the two between-rounds launches of lookup drafts for several sequences (nano_amd/csrc/lookup_rows.hip) through
nano_hip_op_lookup_rows_round, against tests/lookup_rows_ref.py: record for record, history for history and row for row."""
import random

import numpy as np
import pytest

import lookup_ref as lr
import lookup_rows_ref as rr
from nano_amd import binding as nb

pytestmark = pytest.mark.gpu

S = 128


def check(histories, left, slots, fed=(), amax=(), row_start=None, nb_rows=None, D=7, stop=None, ngram_min=1, ngram_max=3, seq_limit=S, max_seq_len=S):
    B = len(histories)
    rs = [rr.NONE] * B if row_start is None else list(row_start)
    cnt = [0] * B if nb_rows is None else list(nb_rows)
    want = rr.round_step(histories, left, slots, list(fed), list(amax), rs, cnt, D, ngram_min, ngram_max, lr.NO_STOP if stop is None else stop, seq_limit, max_seq_len)
    got = nb.op_lookup_rows_round(histories, left, slots, fed, amax, row_start, nb_rows, max_draft=D, ngram_max=ngram_max, ngram_min=ngram_min, stop_token=stop,
                                  seq_limit=seq_limit, max_seq_len=max_seq_len)
    w_recs, w_hs, w_tok, w_pos, w_slot, w_start = want
    g_recs, g_hs, g_tok, g_pos, g_slot, g_start = got
    assert g_recs == w_recs
    assert [h.tolist() for h in g_hs] == w_hs
    assert g_start == w_start
    rows = len(w_tok)
    assert rows == sum(r["nb_next"] for r in w_recs)
    for g, w in ((g_tok, w_tok), (g_pos, w_pos), (g_slot, w_slot)):
        assert g[:rows].tolist() == w and np.all(g[rows:] == rr.NONE)
    return want


def history(seed, n, vocab=6):
    rng = random.Random(seed)
    return [rng.randrange(vocab) for _ in range(n)]


@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_first_round_of_several_sequences(B):
    """no pass has run yet: lookup, gate and packing only; history lengths that are no multiples of 4"""
    lens = [5, 9, 22, 3, 31][:B]
    hs = [history(10 + i, n) for i, n in enumerate(lens)]
    recs = check(hs, [20] * B, list(range(B)))[0]
    assert any(r["nb_next"] == 8 for r in check(hs + [[1, 2, 3, 1, 2, 3, 1]], [20] * (B + 1), list(range(B + 1)))[0])
    assert all(r["emitted"] == 0 and r["done"] == 0 for r in recs)


def test_two_buckets_and_the_chunk_that_falls_back_at_the_bucket_end():
    hs = [[1, 2, 3] * 21, [4, 5, 4, 5, 4, 5], [6] * 65]                     # n - 1 = 62, 5, 64
    recs, _h, _t, pos, slots, start = check(hs, [10, 10, 10], [0, 1, 2])
    assert [r["nb_next"] for r in recs] == [1, 8, 8] and start == [0, 1, 9]
    assert pos == [62] + list(range(5, 13)) + list(range(64, 72)) and slots == [0] + [1] * 8 + [2] * 8


def test_behind_a_pass_first_round_beside_accepted_and_rejected_chunks():
    """sequence 0 has had no rows yet, sequence 1 comes from a 16-row chunk whose rows were all accepted, sequence 2 from one rejected at row 1"""
    h0 = history(1, 7)
    h1 = [1, 2, 3, 4] * 5 + [1, 2, 3]                                       # 23 ids
    h2 = [5, 6] * 6 + [5]                                                   # 13 ids
    fed1 = [h1[-1]] + [[4, 1, 2, 3][k % 4] for k in range(15)]
    amax1 = fed1[1:] + [9]                                                  # every drafted id confirmed; the last row's arg-max is new
    fed2 = [h2[-1]] + [[6, 5][k % 2] for k in range(15)]
    amax2 = [7] + [0] * 15                                                  # row 0 answers 7, the draft said 6
    recs = check([h0, h1, h2], [40, 40, 40], [0, 1, 2], fed1 + fed2, amax1 + amax2, [rr.NONE, 0, 16], [0, 16, 16], D=15)[0]
    assert [r["accepted"] for r in recs] == [0, 15, 0] and [r["emitted"] for r in recs] == [0, 16, 1]
    # the same pass with the two chunks the other way round in it
    check([h0, h1, h2], [40, 40, 40], [0, 1, 2], fed2 + fed1, amax2 + amax1, [rr.NONE, 16, 0], [0, 16, 16], D=15)


def test_left_one_stop_token_and_a_dead_sequence_in_the_middle():
    h1 = [1, 2, 3, 4] * 5 + [1, 2, 3]
    fed = [3, 4, 1, 2, 3, 4, 1, 2]
    amax = [4, 1, 2, 3, 4, 1, 2, 8]
    hs = [h1, history(2, 11), h1, h1]
    # sequence 0: one id left of an accepted run; sequence 1: dead (nothing left, no rows); sequence 2: the stop token inside the accepted
    # run; sequence 3: the whole run
    recs = check(hs, [1, 0, 30, 30], [0, 1, 2, 3], fed * 3, amax * 3, [0, rr.NONE, 8, 16], [8, 0, 8, 8], stop=2)[0]
    assert [r["emitted"] for r in recs] == [1, 0, 3, 3] and [r["done"] for r in recs] == [1, 1, 1, 1]
    recs = check(hs, [1, 0, 30, 30], [0, 1, 2, 3], fed * 3, amax * 3, [0, rr.NONE, 8, 16], [8, 0, 8, 8], stop=None)[0]
    assert [r["emitted"] for r in recs] == [1, 0, 8, 8] and [r["nb_next"] for r in recs] == [0, 0, 1, 1]      # (the new last id 8 has no match)
    assert check(hs, [2, 0, 1, 30], [0, 1, 2, 3])[0][2]["nb_next"] == 1     # left = 1: no chunk


def test_slots_out_of_order_and_the_periodic_extension():
    hs = [[1, 2, 3, 1, 2, 3], history(3, 70), [9, 9]]                       # sequence 0: the draft runs past the history's end
    recs, _h, toks, _p, slots, start = check(hs, [30, 30, 30], [3, 0, 2])
    assert recs[0]["nb_next"] == 8 and toks[start[0]:start[0] + 8] == [3, 1, 2, 3, 1, 2, 3, 1]
    assert slots[start[0]] == 3 and slots[start[1]] == 0 and slots[start[2]] == 2
    assert start[1] > start[0] and start[1] > start[2]                      # position 69 lies in the second bucket


def test_random_rounds():
    rng = random.Random(7)
    for _ in range(6):
        B = rng.randrange(1, 9)
        D = rng.choice([1, 3, 7, 15])
        hs = [history(rng.random(), rng.choice([2, 5, 9, 30, 61, 62, 63, 64, 65, 100]), vocab=4) for _ in range(B)]
        nb_rows = [rng.choice([0, 1, D + 1]) for _ in range(B)]
        fed, amax, rs = [], [], []
        for i in range(B):
            rs.append(len(fed) if nb_rows[i] else rr.NONE)
            f = [hs[i][-1]] + [rng.randrange(4) for _ in range(nb_rows[i] - 1)] if nb_rows[i] else []
            a = [f[k + 1] if k + 1 < len(f) and rng.random() < 0.8 else rng.randrange(4) for k in range(len(f))]
            fed += f; amax += a
        left = [rng.choice([0, 1, 2, 5, 40]) if nb_rows[i] == 0 else rng.choice([1, 2, 5, 40]) for i in range(B)]
        slots = rng.sample(range(16), B)
        check(hs, left, slots, fed, amax, rs, nb_rows, D=D, stop=rng.choice([None, 2]))
