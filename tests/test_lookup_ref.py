"""CPU tests of the definitions of greedy decode with lookup drafts (tests/lookup_ref.py): the single-pass key form
the kernel computes against the two-loop definition, and the lossless property of the loop."""
import itertools
import random

import pytest

import lookup_ref as lr


def test_key_form_equals_definition_exhaustively():
    """every history over a 3-letter alphabet up to length 9, every legal (ngram_min, ngram_max)"""
    pairs = [(lo, hi) for hi in range(1, 5) for lo in range(1, hi + 1)]
    checked = 0
    for n in range(1, 10):
        for h in itertools.product(range(3), repeat=n):
            for lo, hi in pairs:
                assert lr.find_match_key(h, lo, hi) == lr.find_match(h, lo, hi), (h, lo, hi)
                checked += 1
    assert checked == sum(3 ** n for n in range(1, 10)) * len(pairs)


def test_match_prefers_length_then_recency():
    assert lr.find_match([1, 2, 9, 1, 2, 8, 2], 1, 3) == (1, 5)            # two matches of length 1 (ends 2 and 5): the later
    assert lr.find_match([7, 1, 2, 9, 2, 8, 1, 2], 1, 3) == (2, 3)         # length 2 at end 3 beats length 1 at end 5
    assert lr.find_match([1, 2, 3], 1, 3) is None
    assert lr.find_match([5], 1, 4) is None
    assert lr.find_match([5, 5], 1, 4) == (1, 1)
    assert lr.find_match([1, 2, 3, 4, 1, 2, 3, 4], 1, 2) == (2, 4)         # four matching ids, ngram_max = 2
    assert lr.find_match([1, 2, 9, 1, 2], 3, 4) is None                     # ngram_min above the best match


def test_draft_is_the_periodic_extension():
    assert lr.draft([1, 2, 3, 1], 1, 7) == [2, 3, 1, 2, 3, 1, 2]
    assert lr.draft([5, 5], 1, 4) == [5, 5, 5, 5]
    assert lr.draft([1, 2, 3, 4, 1], 1, 2) == [2, 3]
    assert lr.draft([1, 2], 1, 0) == []


def test_accept_stops_at_the_first_mismatch():
    assert lr.accepted([1], [9]) == 0
    assert lr.accepted([1, 2, 3], [2, 3, 4]) == 2
    assert lr.accepted([1, 2, 7, 4], [2, 3, 4, 5]) == 1                     # rows behind the mismatch match again: they do not count
    assert lr.accepted([1, 7, 3], [2, 3, 4]) == 0


def _truths():
    rng = random.Random(39)
    yield "period 3", [1, 2, 3] * 70
    yield "period 1", [4] * 200
    yield "random over 4 letters", [rng.randrange(4) for _ in range(200)]
    yield "random over 50 letters", [rng.randrange(50) for _ in range(200)]
    yield "period 5 with a defect every 17", [(i % 5) if i % 17 else 9 for i in range(200)]


@pytest.mark.parametrize("name,seq", list(_truths()), ids=[n for n, _ in _truths()])
def test_simulate_is_lossless(name, seq):
    """whatever is drafted, gated or clipped, the loop emits exactly the truth"""
    for D in range(0, 16):
        for n0, max_new, limit in ((1, 100, 1 << 30), (5, 100, 128), (5, 123, 128), (60, 20, 1 << 30), (3, 1, 1 << 30), (3, 2, 1 << 30)):
            hist, truth = seq[:n0], seq[n0:]
            ids, st = lr.simulate(hist, truth, max_new, D, 1, 3, seq_limit=limit)
            assert ids == truth[:max_new], (name, D, n0, max_new)
            assert st["emitted"] == max_new and st["drafted"] == st["steps_verify"] * D
            assert st["steps_plain"] + st["steps_verify"] <= max_new
            if D == 0:
                assert st["steps_verify"] == 0 and st["steps_plain"] == max_new


def test_simulate_gate_and_stop():
    seq = [1, 2, 3] * 70
    # a chunk stays inside one 64-position bucket: with K = 16 the positions 49 .. 63 of every bucket take plain steps
    ids, st = lr.simulate(seq[:4], seq[4:], 150, 15, 1, 3)
    assert ids == seq[4:154] and st["steps_plain"] > 0 and st["steps_verify"] > 0
    # the stop token ends the loop after it is emitted, also inside an accepted run
    ids, st = lr.simulate(seq[:4], seq[4:], 150, 7, 1, 3, stop_token=3)
    assert ids == [2, 3]
    ids, st = lr.simulate(seq[:4], seq[4:], 150, 7, 1, 3, max_steps=1)
    assert ids == seq[4:12] and st["steps_verify"] == 1 and st["accepted"] == 7
    # nothing to draft from: plain steps only
    ids, st = lr.simulate([0], list(range(1, 60)), 50, 7)
    assert ids == list(range(1, 51)) and st["steps_verify"] == 0
