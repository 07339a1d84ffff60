"""CPU tests of tests/lookup_rows_ref.py: the round of lookup drafts for several sequences, restated in plain Python.

The property everything else rests on: a sequence's ids, stats and steps do not depend on what shares its pass -- simulate_rows per
sequence is lookup_ref.simulate.  And the planner's shape: stable order by hint, contiguous rows, groups = runs of equal hints."""
import random

import pytest

import lookup_ref as lr
import lookup_rows_ref as rr


def sequences(seed, B, vocab=7, n_truth=140):
    """B (history, truth) pairs; a small vocabulary makes n-gram matches (right and wrong drafts) frequent; sequence 1 is periodic"""
    rng = random.Random(seed)
    hs, ts = [], []
    for i in range(B):
        n = rng.choice([1, 2, 3, 5, 6, 7, 9, 62, 63])
        if i == 1:
            period = [rng.randrange(vocab) for _ in range(3)]
            full = [period[k % 3] for k in range(n + n_truth)]
        else:
            full = [rng.randrange(vocab) for _ in range(n + n_truth)]
        hs.append(full[:n]); ts.append(full[n:])
    return hs, ts


@pytest.mark.parametrize("B", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("D", [0, 1, 3, 7, 15])
def test_simulate_rows_is_simulate_per_sequence(B, D):
    for seed in range(6):
        hs, ts = sequences(seed, B)
        max_new = [[100, 37, 5, 64, 1, 2, 0, 90][i] for i in range(B)]
        ids, stats, rounds = rr.simulate_rows(hs, ts, max_new, D, 1, 3, seq_limit=128, max_seq_len=128)
        want_rounds = 0
        for i in range(B):
            want_ids, want_stats = lr.simulate(hs[i], ts[i], max_new[i], D, 1, 3, seq_limit=128)
            assert ids[i] == want_ids and stats[i] == want_stats, (seed, i)
            want_rounds = max(want_rounds, want_stats["steps_plain"] + want_stats["steps_verify"])
        assert rounds == want_rounds


def test_simulate_rows_stop_token_and_max_steps():
    hs, ts = sequences(3, 3)
    stop = ts[0][20]
    ids, stats, _ = rr.simulate_rows(hs, ts, [60, 60, 60], 7, 1, 3, stop_token=stop, seq_limit=128, max_seq_len=128)
    for i in range(3):
        want_ids, want_stats = lr.simulate(hs[i], ts[i], 60, 7, 1, 3, stop_token=stop, seq_limit=128)
        assert ids[i] == want_ids and stats[i] == want_stats
    assert ids[0][-1] == stop and len(ids[0]) <= 21
    ids, stats, rounds = rr.simulate_rows(hs, ts, [60, 60, 60], 7, 1, 3, seq_limit=128, max_seq_len=128, max_steps=2)
    assert rounds == 2
    for i in range(3):
        assert (ids[i], stats[i]) == lr.simulate(hs[i], ts[i], 60, 7, 1, 3, seq_limit=128, max_steps=2)


def planner_cases():
    rng = random.Random(11)
    edge = [1, 5, 62, 63, 64, 65, 120, 126, 127, 128]
    for B in range(1, 9):
        for K in (1, 2, 4, 8, 16):
            for _ in range(6):
                n, nb = [], []
                for _i in range(B):
                    nb_i = rng.choice([0, 1, K])
                    n_i = rng.choice(edge)
                    while nb_i and n_i - 1 + nb_i > 128:
                        n_i = rng.choice(edge)
                    n.append(n_i); nb.append(nb_i)
                yield n, nb


def test_planner_shape():
    for n, nb in planner_cases():
        order, start, groups = rr.plan(n, nb, 128)
        live = [i for i in range(len(n)) if nb[i]]
        assert sorted(order) == live
        hints = [rr.hint(n[i], 128) for i in order]
        assert hints == sorted(hints)
        for k in range(1, len(order)):                                      # stable: equal hints keep the caller's order
            assert hints[k - 1] < hints[k] or order[k - 1] < order[k]
        row = 0
        for i in order:                                                     # contiguous rows, in pass order, no gaps
            assert start[i] == row
            row += nb[i]
        assert all(start[i] == rr.NONE for i in range(len(n)) if not nb[i])
        # groups: the runs of equal hints
        assert [g[0] for g in groups] == sorted(set(hints)) and sum(g[1] for g in groups) == row
        for h, rows in groups:
            assert rows == sum(nb[i] for i in order if rr.hint(n[i], 128) == h)


def test_hint_is_the_bucket_end():
    assert [rr.hint(n, 128) for n in (1, 64, 65, 128)] == [64, 64, 128, 128]
    assert rr.hint(65, 100) == 100 and rr.hint(129, 1 << 30) == 192


def test_round_step_packs_by_hint():
    hs = [[1, 2, 3] * 21, [4, 5, 4, 5, 4, 5], [6] * 65]                     # n - 1 = 62, 5, 64
    recs, _h, toks, pos, sl, start = rr.round_step(hs, [10, 10, 10], [3, 0, 2], [], [], [rr.NONE] * 3, [0] * 3, 7, seq_limit=128, max_seq_len=128)
    assert [r["nb_next"] for r in recs] == [1, 8, 8]                        # the chunk at 62 would leave its bucket: one row
    assert start == [0, 1, 9] and sl == [3] + [0] * 8 + [2] * 8
    assert pos == [62] + list(range(5, 13)) + list(range(64, 72))
    assert toks[0] == 3 and toks[1:9] == [5, 4, 5, 4, 5, 4, 5, 4]
