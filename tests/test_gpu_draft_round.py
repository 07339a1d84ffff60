"""GPU tests of draft_round_kernel alone (nano_hip_op_draft_round: its STAGE role, then its ACCEPT role), held to tests/draft_ref.py field
for field: the record, the history, row 0 and the positions of the next round."""
import numpy as np
import pytest

import draft_ref as dr
from nano_amd import binding as nb

pytestmark = pytest.mark.gpu

NONE = dr.NONE


def hist(n, seed=3):
    return np.random.default_rng(seed).integers(0, 1000, n).astype(np.uint32).tolist()


def check(h, fed, amax, left, D, dn, stop=None, seq_limit=1 << 30):
    stop_token = dr.NO_STOP if stop is None else stop
    want, wh, tok0, pos = dr.step(h, fed, amax, left, D, stop_token, seq_limit, dn, cap=dr.history_cap(len(h), seq_limit))
    rec, gh, nt, npos = nb.op_draft_round(h, fed, amax, left=left, dn=dn, max_draft=D, stop_token=stop, seq_limit=seq_limit)
    assert rec == want, (rec, want)
    assert gh.tolist() == wh
    toks = [NONE] * 16
    toks[:len(fed)] = fed                                  # row 0 as the round before staged it, rows 1 .. as STAGE put them
    if tok0 is not None:
        toks[0] = tok0
    assert nt.tolist() == toks
    assert npos.tolist() == pos + [NONE] * (16 - len(pos))
    return rec


def truth_rows(h, nb_rows, wrong_at=None):
    """a round of nb_rows rows behind history h: fed ids and arg-maxes of a target whose continuation is 5000, 5001, ..; the draft is
    wrong at fed row wrong_at (1-based among the drafted rows)"""
    cont = [5000 + i for i in range(nb_rows)]
    fed = [h[-1]] + cont[:nb_rows - 1]
    if wrong_at is not None:
        fed[wrong_at] = 7777
    amax = [cont[i] if (wrong_at is None or i < wrong_at) else 9000 + i for i in range(nb_rows)]
    return fed, amax


@pytest.mark.parametrize("rows", [0, 1, 2, 16])
def test_row_counts(rows):
    h = hist(20)
    fed, amax = truth_rows(h, rows) if rows else ([], [])
    rec = check(h, fed, amax, 50, 15, 7)
    assert rec["emitted"] == rows and rec["accepted"] == max(rows - 1, 0)
    assert rec["dn"] == (7 if rows <= 1 else 20 + rows - 2)


@pytest.mark.parametrize("wrong_at", [1, 4, None], ids=["row1", "middle", "none"])
def test_first_mismatch(wrong_at):
    h = hist(20)
    fed, amax = truth_rows(h, 8, wrong_at)
    rec = check(h, fed, amax, 50, 7, 19)
    a = 7 if wrong_at is None else wrong_at - 1
    assert (rec["accepted"], rec["emitted"], rec["n"], rec["dn"]) == (a, a + 1, 20 + a + 1, 20 + min(a, 6))


def test_left_smaller_than_the_accepted_rows():
    h = hist(20)
    fed, amax = truth_rows(h, 8)
    rec = check(h, fed, amax, 3, 7, 19)
    assert (rec["accepted"], rec["emitted"], rec["done"], rec["left"], rec["nb_next"]) == (7, 3, 1, 0, 0)


@pytest.mark.parametrize("at", [0, 3, 7], ids=["first", "middle", "last"])
def test_stop_token(at):
    h = hist(20)
    fed, amax = truth_rows(h, 8)
    rec = check(h, fed, amax, 50, 7, 19, stop=amax[at])
    assert (rec["emitted"], rec["done"], rec["nb_next"]) == (at + 1, 1, 0) and rec["dn"] == min(26, 20 + at)


@pytest.mark.parametrize("n,rows_next", [(59, 5), (62, 2), (63, 1), (64, 5), (126, 2), (127, 1)])
def test_bucket_end_and_sequence_limit(n, rows_next):
    """a one-row round takes the history from n to n + 1 ids: at 63 the next round feeds position 62 first (one draft fits the bucket),
    at 64 position 63 (none), 65 opens the next bucket; seq_limit = 128: 127 ids leave room for one drafted row, 128 for none"""
    h = hist(n)
    rec = check(h, [h[-1]], [4242], 50, 4, 3, seq_limit=128)
    assert rec["n"] == n + 1 and rec["nb_next"] == dr.round_rows(n + 1, 49, 4, 128) == rows_next


def test_history_capacity_reached():
    h = hist(127)                                          # seq_limit 127: the device history holds 128 ids
    fed, amax = truth_rows(h, 1)
    rec = check(h, fed, amax, 5, 4, 100, seq_limit=127)
    assert (rec["emitted"], rec["n"], rec["done"], rec["left"], rec["nb_next"]) == (1, 128, 1, 4, 0)
    h = hist(126)                                          # two accepted rows, room for both and not one more
    fed, amax = truth_rows(h, 3, wrong_at=2)
    rec = check(h, fed, amax, 5, 4, 100, seq_limit=127)
    assert (rec["accepted"], rec["emitted"], rec["n"], rec["done"]) == (1, 2, 128, 1)
