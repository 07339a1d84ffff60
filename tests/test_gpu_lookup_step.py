"""GPU tests of lookup_step_kernel (nano_amd/csrc/lookup.hip) through nano_hip_op_lookup_step against tests/lookup_ref.py: every output
word equal -- the record, the history with the emitted ids appended, and all 16 words of the next step's tokens and positions."""
import random

import numpy as np
import pytest

import lookup_ref as lr
from nano_amd import binding as nb

pytestmark = pytest.mark.gpu

OP_CAPACITY = 65536                  # the largest history nano_hip_op_lookup_step takes


def check(h, fed=(), amax=(), *, left, D=7, lo=1, hi=3, stop=None, limit=1 << 30, what=""):
    stop_r = lr.NO_STOP if stop is None else stop
    rec, h2, toks, pos = lr.step(h, list(fed), list(amax), left, D, lo, hi, stop_r, limit)
    got, gh, gt, gp = nb.op_lookup_step(h, fed, amax, left=left, max_draft=D, ngram_max=hi, ngram_min=lo, stop_token=stop, seq_limit=limit)
    tag = f"{what}: n {len(h)}, fed {list(fed)}, amax {list(amax)}, left {left}, D {D}, ngram {lo}..{hi}, stop {stop}, limit {limit}"
    assert got == rec, (tag, got, rec)
    assert gh.tolist() == h2, tag
    pad = [lr.NONE] * (16 - len(toks))
    assert gt.tolist() == toks + pad and gp.tolist() == pos + pad, (tag, gt.tolist(), toks, gp.tolist(), pos)
    return rec, toks


def test_lookup_edges():
    assert check([5], left=9, what="n = 1")[0]["nb_next"] == 1
    rec, toks = check([5, 5], left=9, what="n = 2, period 1")
    assert rec["nb_next"] == 8 and toks == [5] * 8 and (rec["match_len"], rec["match_end"]) == (1, 1)
    assert check([1, 2, 3, 4, 4], left=9, what="only match at e = n-1")[0]["match_end"] == 4
    rec, _ = check([7, 1, 2, 3, 7], left=9, hi=4, what="e = 1 with ngram_max 4: the window runs off the start")
    assert (rec["match_len"], rec["match_end"]) == (1, 1)
    assert check([1, 2, 9, 1, 2, 8, 2], left=9, what="two equal-length matches: the later")[0]["match_end"] == 5
    rec, _ = check([7, 1, 2, 9, 2, 8, 1, 2], left=9, what="longer earlier against shorter later: the longer")
    assert (rec["match_len"], rec["match_end"]) == (2, 3)
    rec, _ = check([1, 2, 3, 4, 1, 2, 3, 4], left=9, hi=2, what="four matching ids, ngram_max 2")
    assert (rec["match_len"], rec["match_end"]) == (2, 4)
    rec, _ = check([1, 2, 9, 1, 2], left=9, lo=3, hi=4, what="ngram_min above the best match")
    assert rec["nb_next"] == 1 and rec["match_len"] == 0
    assert check([1, 2, 1], left=9, D=0, what="D = 0")[0]["nb_next"] == 1
    for D in (1, 15):
        assert check([1, 2, 1], left=9, D=D, what="D")[0]["nb_next"] == D + 1


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1025, OP_CAPACITY])
def test_lookup_long_histories(n):
    """the match at e = 1 and at e = n-1: the first and the last end of the strided scan, around whole multiples of the 256 threads' reach"""
    for where in ("first", "last"):
        h = list(range(10, 10 + n))                            # all different: no match
        if where == "first":
            h[0] = h[n - 1]                                    # e = 1
        else:
            h[n - 2] = h[n - 1]                                # e = n-1
        rec, toks = check(h, left=20, D=3, limit=1 << 20, what=f"{where} end")
        assert rec["match_end"] == (1 if where == "first" else n - 1) and rec["match_len"] == 1
        assert rec["nb_next"] == (4 if (n - 1) % 64 + 4 <= 64 else 1)
    h = [3, 4, 5, 6] + list(range(10, 10 + n - 8)) + [3, 4, 5, 6]
    rec, _ = check(h, left=20, D=3, hi=4, limit=1 << 20, what="length 4 at e = 4")
    assert (rec["match_len"], rec["match_end"]) == (4, 4)


def test_accept_clip_and_stop():
    h = [1, 2, 3, 1]
    fed = [1, 2, 3, 1]                                          # positions 3 .. 6
    assert check(h, fed, [9, 3, 1, 2], left=50, D=3, what="a = 0")[0]["emitted"] == 1
    rec, _ = check(h, fed, [2, 3, 1, 2], left=50, D=3, what="a = nb-1")
    assert (rec["accepted"], rec["emitted"]) == (3, 4)
    rec, _ = check(h, fed, [2, 7, 1, 2], left=50, D=3, what="a mismatch in the middle, the rows behind it match again")
    assert (rec["accepted"], rec["emitted"]) == (1, 2)
    rec, _ = check(h, fed, [2, 3, 1, 2], left=2, D=3, what="left < a+1")
    assert (rec["accepted"], rec["emitted"], rec["done"], rec["nb_next"]) == (3, 2, 1, 0)
    rec, _ = check(h, fed, [2, 3, 1, 2], left=5, D=3, what="left == 1 at the gate")
    assert (rec["emitted"], rec["left"], rec["nb_next"], rec["done"]) == (4, 1, 1, 0)
    rec, _ = check(h, fed, [2, 3, 1, 2], left=50, D=3, stop=2, what="the stop token first")
    assert (rec["emitted"], rec["done"]) == (1, 1)
    rec, _ = check(h, fed, [2, 3, 1, 2], left=50, D=3, stop=1, what="the stop token inside the accepted run")
    assert (rec["emitted"], rec["done"], rec["accepted"]) == (3, 1, 3)
    assert check(h, [1], [2], left=50, D=3, what="a plain step")[0]["nb_next"] == 4
    assert check(h, [1], [2], left=1, D=3, what="the last id")[0]["done"] == 1
    assert check(h, left=0, D=3, what="nothing to emit")[0]["done"] == 1


def test_gates():
    K = 8
    for n, want in ((64 - K + 1, K), (64 - K + 2, 1), (128 - K + 1, K), (128 - K + 2, 1)):     # (n-1) % 64 + K = 64 | 65
        h = [1, 2] * (n // 2) + [1] * (n % 2)
        assert check(h, left=50, D=K - 1, what="bucket end")[0]["nb_next"] == want
    h = [1, 2] * 10                                             # n = 20: n-1+K = 27
    assert check(h, left=50, D=K - 1, limit=27, what="n-1+K = S")[0]["nb_next"] == K
    assert check(h, left=50, D=K - 1, limit=26, what="n-1+K = S+1")[0]["nb_next"] == 1


def test_random_cases():
    rng = random.Random(39)
    for case in range(200):
        n = rng.choice([1, 2, 3, 5, 8, 13, 40, 63, 64, 65, 130, 300])
        h = [rng.randrange(4) for _ in range(n)]
        hi = rng.randint(1, 4); lo = rng.randint(1, hi)
        D = rng.randint(0, 15)
        nb_ = rng.choice([0, 1, D + 1])
        fed, amax = [], []
        if nb_:
            fed = [h[-1]] + [rng.randrange(4) for _ in range(nb_ - 1)]
            amax = [rng.randrange(4) for _ in range(nb_)]
            if rng.random() < 0.5:                              # a run of accepted rows
                for i in range(rng.randint(0, nb_ - 1)):
                    amax[i] = fed[i + 1]
        check(h, fed, amax, left=rng.choice([0, 1, 2, 3, 20]), D=D, lo=lo, hi=hi, stop=rng.choice([None, None, 0, 3]),
              limit=rng.choice([1 << 30, n + 3, n + 16]), what=f"random case {case}")
