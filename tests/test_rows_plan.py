"""CPU sweep of the ragged step's planner (nano_hip_rows_plan, include/nano_mi355x.h): how nano_hip_step_rows cuts the rows of its
segments -- each a run of positions of one KV slot -- into passes of at most `cap` rows, and in what order a pass holds them.  Device-free:
host arithmetic only.  Also every refusal of the device call that needs no device, and the addressing predicate."""
import ctypes as C

import numpy as np
import pytest

from nano_amd import binding as nb

EINVAL = -1


def lib():
    return nb.lib()


def rows_of(segs):
    """caller-order rows as (slot, position)"""
    return [(s[0], s[1] + k) for s in segs for k in range(s[2])]


def check_plan(segs, cap, S):
    rp, ri, rh, n_passes = nb.rows_plan(segs, cap, S)
    rows = rows_of(segs)
    assert len(rp) == len(ri) == len(rh) == len(rows)
    assert len(set(rows)) == len(rows)                                       # no (slot, position) twice
    # the hint of a row is that of its own one-sequence decode step
    for (slot, pos), h in zip(rows, rh):
        assert h == min(((pos + 64) // 64) * 64, S), (slot, pos, h)
    # every row is in exactly one pass, at one row of its own; at most cap rows per pass; no gaps
    assert n_passes == -(-len(rows) // cap)                                   # nothing forces a cut: ceil(rows / cap)
    seen = set()
    for p, i in zip(rp, ri):
        assert p < n_passes and i < cap and (p, i) not in seen
        seen.add((int(p), int(i)))
    for p in range(n_passes):
        idx = sorted(i for (q, i) in seen if q == p)
        assert idx == list(range(len(idx))) and 1 <= len(idx) <= cap
        assert len(idx) == cap or p == n_passes - 1                           # greedy fill: only the last pass is partly filled
    # a slot's rows ascend over (pass, position): a later position never sits in an earlier pass
    last = {}
    for (slot, pos), p in zip(rows, rp):
        if slot in last:
            assert (int(p), pos) > last[slot], (slot, pos)
        last[slot] = (int(p), pos)
    # rows of a pass are sorted by hint, stably (caller order among equal hints)
    for p in range(n_passes):
        mine = [r for r in range(len(rows)) if rp[r] == p]
        want = sorted(mine, key=lambda r: int(rh[r]))                         # (sorted() is stable)
        got = sorted(mine, key=lambda r: int(ri[r]))
        assert got == want, p
    return rp, ri, rh, n_passes


COUNTS = (0, 1, 63, 64, 65, 200)
POS0 = (0, 63, 64, 127)


@pytest.mark.parametrize("S", [256, 4096])
@pytest.mark.parametrize("cap", [8, 64])
def test_constructed_lists(cap, S):
    for count in COUNTS:
        for pos0 in POS0:
            if pos0 + count > S:
                continue
            check_plan([(0, pos0, count)], cap, S)
            check_plan([(5, 3, 2), (0, pos0, count), (9, 70, 1)], cap, S)
            check_plan([(s, pos0, count) for s in range(4)], cap, S)
    # the GPU test's lists
    check_plan([(2, 0, 15), (0, 0, 70), (3, 0, 1), (1, 0, 150)], cap, S)
    check_plan([(1, 150, 20), (2, 15, 60)], cap, S)
    check_plan([(s, 0, 4) for s in range(16)], cap, S)
    check_plan([], cap, S)
    check_plan([(1, 0, 0), (2, 9, 0)], cap, S)


@pytest.mark.parametrize("S", [256, 4096])
@pytest.mark.parametrize("cap", [8, 64])
def test_random_lists(cap, S):
    rng = np.random.default_rng(1000 * cap + S)
    for _ in range(60):
        n = int(rng.integers(1, 9))
        slots = rng.permutation(64)[:n]
        segs = []
        for s in slots:
            count = int(rng.choice(COUNTS + (2, 17)))
            pos0 = int(rng.choice(POS0 + (1, 200)))
            if pos0 + count > S:
                pos0 = S - count
            segs.append((int(s), pos0, count))
        check_plan(segs, cap, S)


def test_one_pass_holds_three_buckets_in_hint_order():
    """rows of buckets 0, 1 and 2 in one pass of 64: slot 1's two buckets, another slot's bucket-0 rows behind them in caller order"""
    segs = [(1, 60, 10), (0, 0, 5), (2, 120, 12)]
    rp, ri, rh, n = check_plan(segs, 64, 256)
    assert n == 1
    assert rh.tolist() == [64] * 4 + [128] * 6 + [64] * 5 + [128] * 8 + [192] * 4
    assert ri[:4].tolist() == [0, 1, 2, 3] and ri[10:15].tolist() == [4, 5, 6, 7, 8]      # the bucket-0 rows first, caller order
    assert rh[np.argsort(ri)].tolist() == sorted(rh.tolist())
    # the hint is clipped to max_seq_len
    assert nb.rows_plan([(0, 190, 10)], 64, 200)[2].tolist() == [192] * 2 + [200] * 8


def plan_rc(segs, n, cap, S):
    return lib().nano_hip_rows_plan(segs, n, cap, S, None, None, None, None)


def test_plan_refusals():
    ok = nb.row_segs([(0, 0, 4), (1, 8, 4)])
    assert plan_rc(ok.ctypes.data, 2, 64, 256) == 0
    assert plan_rc(None, 2, 64, 256) == EINVAL                                # null segs
    assert plan_rc(None, 0, 64, 256) == 0                                     # ... but an empty list needs none
    assert plan_rc(ok.ctypes.data, 2, 0, 256) == EINVAL and plan_rc(ok.ctypes.data, 2, 64, 0) == EINVAL
    for bad in ([(0, 0, 4, 1)],                                               # reserved != 0
                [(3, 0, 4), (1, 0, 2), (3, 10, 1)],                           # two segments with the same slot
                [(3, 0, 0), (3, 10, 1)],                                      # ... an empty one counts
                [(0, 250, 7)], [(0, 256, 1)], [(0, 0xffffffff, 2)], [(0, 1, 0xffffffff)], [(0, 257, 0)]):     # beyond max_seq_len
        s = nb.row_segs(bad)
        assert plan_rc(s.ctypes.data, len(bad), 64, 256) == EINVAL, bad
        assert b"" != lib().nano_hip_last_error()
    s = nb.row_segs([(0, 250, 6), (7, 256, 0)])                               # up to the last position: fine
    assert plan_rc(s.ctypes.data, 2, 64, 256) == 0


def test_device_call_refusals_that_need_no_device():
    L = lib()
    s = nb.row_segs([(0, 0, 2)])
    t = np.zeros(2, np.uint32)
    assert L.nano_hip_step_rows(None, s.ctypes.data, 1, t.ctypes.data, None) == EINVAL      # null model
    assert L.nano_prefill_batch(None, None, t, 1, None) == EINVAL                            # null context


def test_addressing_predicate():
    A = lib().nano_hip_rows_addressable
    assert A(28, 4096, 1024, 4) == 1 and A(36, 32768, 1024, 4) == 1           # Qwen3-0.6B / 4B shapes: 64 slots are no obstacle
    assert A(36, 32768, 1024, 2) == 1
    assert A(4, 1 << 20, 1024, 4) == 0                                        # a layer of one slot beyond a 32-bit byte offset
    assert A(4, 1 << 20, 1024, 2) == 1 and A(4, 1 << 21, 1024, 2) == 0
    assert A(1 << 16, 1 << 16, 8, 4) == 0                                     # a slot's rows beyond a 32-bit count
    assert A(0, 256, 64, 4) == 0 and A(2, 256, 64, 0) == 0
