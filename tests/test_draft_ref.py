"""CPU tests of the definitions of greedy decode with a draft model (tests/draft_ref.py): the bucket rule, clipping, the stop token,
what the draft holds after a round, and the catch-up rows -- and that the loop is lossless for any draft."""
import random

import pytest

import draft_ref as dr
import lookup_ref as lr


def truth(n_prompt, n):
    rng = random.Random(5)
    return [rng.randrange(1000) for _ in range(n_prompt)], [rng.randrange(1000) for _ in range(n)]


def perfect(full):
    return lambda prefix, k: full[len(prefix): len(prefix) + k]


def useless(prefix, k):
    return [2000 + i for i in range(k)]                   # ids the truth never holds


def test_accepted_is_the_lookup_loops():
    assert dr.accepted is lr.accepted
    assert dr.accepted([5, 6, 7], [6, 7, 8]) == 2 and dr.accepted([5, 6, 7], [6, 9, 8]) == 1 and dr.accepted([5, 6, 7], [0, 7, 8]) == 0
    assert dr.accepted([5], [6]) == 0


@pytest.mark.parametrize("n,want", [(1, 5), (60, 5), (61, 4), (62, 3), (63, 2), (64, 1), (65, 5), (128, 1), (129, 5)])
def test_bucket_ends_at_positions_63_64(n, want):
    """a history of n ids feeds position n-1 first: the chunk's last position n-1+D' stays at or below the bucket's 63"""
    assert dr.round_rows(n, 100, 4, 1 << 30) == want
    assert (n - 1) // 64 == (n - 1 + want - 1) // 64


def test_round_rows_clips_to_left_the_limit_and_max_draft():
    assert dr.round_rows(10, 0, 4, 1 << 30) == 0
    assert [dr.round_rows(10, left, 4, 1 << 30) for left in (1, 2, 3, 5, 6)] == [1, 2, 3, 5, 5]
    assert [dr.round_rows(n, 50, 4, 128) for n in (120, 124, 125, 126, 127, 128)] == [5, 5, 4, 3, 2, 1]   # last position n-1+D' <= 127
    assert dr.round_rows(10, 100, 0, 1 << 30) == 1 and dr.round_rows(1, 100, 15, 1 << 30) == 16 and dr.round_rows(1, 100, 40, 1 << 30) == 16


def test_left_clips_the_emitted_ids():
    rec, h, tok0, pos = dr.step([1, 2, 3], [3, 10, 11, 12], [10, 11, 12, 13], 2, 4, dr.NO_STOP, 1 << 30, 2)
    assert (rec["accepted"], rec["emitted"], rec["left"], rec["done"], rec["nb_next"]) == (3, 2, 0, 1, 0)
    assert h == [1, 2, 3, 10, 11] and tok0 is None and pos == []


@pytest.mark.parametrize("at", [0, 1, 3])
def test_stop_token_inside_a_chunk(at):
    amax = [10, 11, 12, 13]
    rec, h, _, _ = dr.step([1, 2, 3], [3, 10, 11, 12], amax, 50, 4, amax[at], 1 << 30, 2)
    assert rec["accepted"] == 3 and rec["emitted"] == at + 1 and rec["done"] == 1 and h == [1, 2, 3] + amax[:at + 1]
    assert rec["dn"] == min(3 + 2, len(h) - 1)            # never the last id's position: it has not been fed to anybody


def test_dn_after_full_partial_and_zero_acceptance():
    h0, fed = [1, 2, 3], [3, 10, 11, 12]                  # n = 3, D' = 3: the draft fed 3, 10, 11 at positions 2, 3, 4
    full = dr.step(h0, fed, [10, 11, 12, 13], 50, 3, dr.NO_STOP, 1 << 30, 2)[0]
    part = dr.step(h0, fed, [10, 77, 12, 13], 50, 3, dr.NO_STOP, 1 << 30, 2)[0]
    zero = dr.step(h0, fed, [99, 11, 12, 13], 50, 3, dr.NO_STOP, 1 << 30, 2)[0]
    assert (full["accepted"], full["n"], full["dn"]) == (3, 7, 5)       # positions 0 .. 4; h[5] = 12 was drafted but never fed to the draft
    assert (part["accepted"], part["n"], part["dn"]) == (1, 5, 4)       # position 3 held the right id 10, position 4 a wrong one
    assert (zero["accepted"], zero["n"], zero["dn"]) == (0, 4, 3)       # position 2 held h[2]
    assert [dr.catch_up_rows(r["n"], r["dn"]) for r in (full, part, zero)] == [1, 0, 0]
    plain = dr.step(h0, [3], [10], 50, 3, dr.NO_STOP, 1 << 30, 1)[0]    # a one-row round ran no draft step: the draft falls behind
    assert (plain["n"], plain["dn"]) == (4, 1) and dr.catch_up_rows(plain["n"], plain["dn"]) == 2


def test_catch_up_row_counts_over_a_run():
    prompt, want = truth(40, 100)
    full = prompt + want
    ids, st = dr.simulate(prompt, want, 100, 4, perfect(full), seq_limit=160)
    assert ids == want and st["accepted"] == st["drafted"]
    # the prompt (39 rows), then one row after every fully accepted round but the last, plus the rows a plain round left behind
    _, one = dr.simulate(prompt, want, 100, 4, perfect(full), seq_limit=160, max_rounds=1)
    assert one["draft_rows_fed"] == 39 and one["rounds_verify"] == 1 and one["draft_held"] == 40 + 3
    ids, bad = dr.simulate(prompt, want, 100, 4, useless, seq_limit=160)
    assert ids == want and bad["accepted"] == 0 and bad["emitted"] == 100
    # a rejected round needs no catch-up, a plain round one row -- fed by the next drafted round, which the call's last round (left = 1,
    # so plain) does not have
    assert bad["rounds_plain"] == 3 and bad["draft_rows_fed"] == 39 + bad["rounds_plain"] - 1


def test_history_capacity_ends_the_call():
    cap = dr.history_cap(127, 127)
    assert cap == 128
    rec, h, _, _ = dr.step(list(range(127)), [126], [7], 5, 4, dr.NO_STOP, 127, 100, cap=cap)
    assert rec["emitted"] == 1 and rec["n"] == 128 and rec["done"] == 1 and rec["left"] == 4


@pytest.mark.parametrize("D", [0, 1, 4, 15])
@pytest.mark.parametrize("kind", ["perfect", "useless", "half"])
def test_lossless_for_any_draft(D, kind):
    prompt, want = truth(5, 123)
    full = prompt + want
    rng = random.Random(D)
    half = lambda prefix, k: [t if rng.random() < 0.7 else 3000 for t in full[len(prefix): len(prefix) + k]]
    fn = {"perfect": perfect(full), "useless": useless, "half": half}[kind]
    ids, st = dr.simulate(prompt, want, 123, D, fn, seq_limit=128)
    assert ids == want and st["emitted"] == 123 and st["draft_held"] <= 5 + 123 - 1
    assert st["rounds_plain"] + st["rounds_verify"] <= 123
    if D == 0:
        assert st["rounds_verify"] == 0 and st["draft_rows_fed"] == 0
    # continued call after call, one round each, the ids and the summed stats are the single call's
    if kind != "half":
        h, held, acc = list(prompt), 0, {k: 0 for k in st}
        while len(h) < 5 + 123:
            got, s1 = dr.simulate(h, full[len(h):], 5 + 123 - len(h), D, fn, seq_limit=128, draft_held=held, max_rounds=1)
            h += got
            held = s1["draft_held"]
            for k in acc:
                acc[k] += s1[k]
        acc["draft_held"] = held
        assert h == full and acc == st
