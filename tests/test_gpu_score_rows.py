"""The row-statistics kernel alone (nano_amd/csrc/score.hip through nano_hip_op_score_rows) against numpy on the same float32 logits:
selections and rank equal, lse within 1e-5 * max(1, |ref|) of float64, logprob the float32 difference of what was returned
(tests/score_ref.py).  Sizes: one logit, fewer than a quad, a fraction of a tile, one logit past a tile (odd: rows are not 16-byte
aligned), several tiles, Qwen3's vocabulary; 1, 3 and 64 rows."""
import numpy as np
import pytest

from nano_amd import binding as nb
from score_ref import check_scores

pytestmark = pytest.mark.gpu

SHAPES = [(V, rows) for V in (1, 5, 512, 4097, 20000) for rows in (1, 3, 64)] + [(151936, 1), (151936, 3)]


def random_logits(rows, V, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, V)) * 4.0).astype(np.float32)


def targets_for(rows, V, seed):
    t = np.random.default_rng(seed + 1).integers(0, V, rows).astype(np.uint32)
    t[0] = 0                                                  # the first and the last index, then random ones
    if rows > 1:
        t[1] = V - 1
    return t


@pytest.mark.parametrize("V,rows", SHAPES)
def test_random_rows(V, rows):
    lg = random_logits(rows, V, 1000 + V + rows)
    t = targets_for(rows, V, V + rows)
    worst = check_scores(nb.op_score_rows(lg, t), lg, t, f"V={V} rows={rows}")
    worst = max(worst, check_scores(nb.op_score_rows(lg, None), lg, None, f"V={V} rows={rows}, own arg-max"))
    print(f"V={V} rows={rows}: worst lse error = {worst:.3f} of the bound")


def test_full_vocabulary_64_rows():
    """39 MB of logits, the shape of a full prefill chunk of Qwen3: one case."""
    V, rows = 151936, 64
    lg = random_logits(rows, V, 7)
    t = targets_for(rows, V, 8)
    worst = check_scores(nb.op_score_rows(lg, t), lg, t, "64 x 151936")
    print(f"64 x 151936: worst lse error = {worst:.3f} of the bound")


@pytest.mark.parametrize("V", [5, 4097, 20000])
def test_all_logits_equal(V):
    lg = np.full((3, V), 1.25, np.float32)
    t = np.array([0, V - 1, V // 2], np.uint32)
    got = nb.op_score_rows(lg, t)
    check_scores(got, lg, t, f"all equal, V={V}")
    assert not got["argmax"].any()
    assert np.array_equal(got["rank"], t)                     # every earlier index ties and counts
    assert np.all(np.abs(got["lse"].astype(np.float64) - (1.25 + np.log(V))) <= 1e-5 * (1.25 + np.log(V)))


@pytest.mark.parametrize("V,first,second", [(5, 1, 3), (4097, 100, 4096), (20000, 4095, 4096), (20000, 3, 19999)])
def test_the_maximum_twice(V, first, second):
    """Inside one tile, across two tiles, across a tile boundary: the first wins; the second as target has rank 1, the first rank 0."""
    lg = random_logits(2, V, V + first)
    lg[:, first] = 50.0; lg[:, second] = 50.0
    t = np.array([second, first], np.uint32)
    got = nb.op_score_rows(lg, t)
    check_scores(got, lg, t, f"two maxima, V={V}")
    assert got["argmax"].tolist() == [first, first]
    assert got["rank"].tolist() == [1, 0]


@pytest.mark.parametrize("offset", [1e4, -1e4])
def test_large_offsets_do_not_overflow(offset):
    V = 20000
    lg = (random_logits(3, V, 5) + np.float32(offset)).astype(np.float32)
    t = targets_for(3, V, 6)
    got = nb.op_score_rows(lg, t)
    check_scores(got, lg, t, f"offset {offset:g}")
    assert np.all(np.isfinite(got["lse"])) and np.all(np.isfinite(got["logprob"]))


def test_minus_infinity_entries_and_target():
    V = 20000
    lg = random_logits(3, V, 11)
    lg[0, ::3] = -np.inf                                      # scattered
    lg[1, 4096:3 * 4096] = -np.inf                            # two whole tiles hold nothing else
    lg[2, :100] = -np.inf
    t = np.array([3, 5000, 7], np.uint32)                     # every target is a -inf logit
    assert np.all(np.isneginf(lg[np.arange(3), t]))
    got = nb.op_score_rows(lg, t)
    check_scores(got, lg, t, "-inf entries")
    assert np.all(np.isneginf(got["logprob"])) and np.all(np.isfinite(got["lse"]))
    # a -inf target ranks behind every finite logit and behind the -inf logits in front of it
    assert got["rank"][2] == (V - 100) + 7
    t2 = np.array([1, 100, 5000], np.uint32)                  # finite targets of the same rows
    check_scores(nb.op_score_rows(lg, t2), lg, t2, "-inf entries, finite targets")


def test_denormals():
    V = 4097
    rng = np.random.default_rng(3)
    lg = (rng.integers(1, 1 << 22, (3, V)).astype(np.uint32)).view(np.float32).copy()      # positive denormals
    lg[1] = -lg[1]
    lg[2, ::2] = 0.0
    assert np.all(np.abs(lg) < np.finfo(np.float32).tiny)
    t = targets_for(3, V, 4)
    check_scores(nb.op_score_rows(lg, t), lg, t, "denormals")


@pytest.mark.parametrize("V", [4097, 20000])
def test_a_row_scores_the_same_wherever_it_sits(V):
    """The reduction shape depends on V only: row 0 of 1, row 2 of 3 and row 63 of 64 return the same 24 bytes (V = 4097: the three
    placements differ in alignment too)."""
    row = random_logits(1, V, 21 + V)[0]
    tgt = V // 3
    seen = []
    for rows, at in ((1, 0), (3, 2), (64, 63)):
        lg = random_logits(rows, V, 33 + rows)
        lg[at] = row
        t = targets_for(rows, V, rows); t[at] = tgt
        seen.append(nb.op_score_rows(lg, t)[at].tobytes())
    assert seen[0] == seen[1] == seen[2]
