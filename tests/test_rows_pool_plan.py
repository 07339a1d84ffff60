"""CPU sweep of the pooled ragged step's row map (nano_hip_rows_pool_plan, include/nano_mi355x.h): per fed row its segment and its
ordinal among the segment's pooled rows, from the function nano_hip_step_rows_pool builds its kernel's map with.  Device-free."""
import numpy as np
import pytest

from nano_amd import binding as nb

EINVAL = -1
NONE = 0xFFFFFFFF
S = 256


def random_segs(rng):
    n = int(rng.integers(1, 71))
    slots = rng.permutation(128)[:n]
    segs = []
    for s in slots:
        count = int(rng.integers(0, 131))
        pos0 = int(rng.integers(0, S - count + 1)) if rng.integers(0, 2) else 0
        segs.append((int(s), pos0, count))
    return segs


def check_map(segs, cap, pooling):
    rp, ri, _rh, n_passes = nb.rows_plan(segs, cap, S)
    row_seg, row_ord = nb.rows_pool_plan(segs, cap, S, pooling)
    total = sum(c for _, _, c in segs)
    assert len(row_seg) == len(row_ord) == total
    # the placement is nano_hip_rows_plan's: caller row r is fed as row pass_start[pass] + index
    per_pass = np.bincount(rp, minlength=n_passes) if total else np.zeros(0, int)
    pass_start = np.concatenate([[0], np.cumsum(per_pass)]).astype(int)
    fed = [None] * total                                                      # fed row -> (segment, position, pass, pass row)
    r = 0
    for i, (_slot, pos0, count) in enumerate(segs):
        for j in range(count):
            w = int(pass_start[rp[r]] + ri[r])
            assert fed[w] is None
            fed[w] = (i, pos0 + j, int(rp[r]), int(ri[r]))
            r += 1
    assert all(f is not None for f in fed)
    assert [f[0] for f in fed] == row_seg.tolist()
    by_seg = [[] for _ in segs]
    for w in range(total):
        by_seg[fed[w][0]].append((fed[w][2], fed[w][3], fed[w][1], int(row_ord[w])))
    for i, (_slot, pos0, count) in enumerate(segs):
        mine = by_seg[i]
        assert len(mine) == count
        pooled = sorted(m for m in mine if m[3] != NONE)                      # by (pass, pass row)
        # pooled rows ascend in position over (pass, pass row), and their ordinals count up from 0
        assert [m[2] for m in pooled] == sorted(m[2] for m in pooled)
        assert [m[3] for m in pooled] == list(range(len(pooled)))
        if pooling == "last":
            assert len(pooled) == (1 if count else 0)
            if count:
                assert pooled[0][2] == pos0 + count - 1                       # the segment's highest position
        else:
            assert len(pooled) == count
            assert [m[2] for m in pooled] == list(range(pos0, pos0 + count))


@pytest.mark.parametrize("pooling", ["last", "mean"])
def test_random_lists(pooling):
    rng = np.random.default_rng(20261020)
    for k in range(200):
        check_map(random_segs(rng), (1, 8, 64)[k % 3], pooling)


@pytest.mark.parametrize("pooling", ["last", "mean"])
@pytest.mark.parametrize("cap", [1, 8, 64])
def test_constructed_lists(cap, pooling):
    check_map([], cap, pooling)
    check_map([(3, 0, 0), (1, 7, 0)], cap, pooling)
    check_map([(0, 0, 40), (1, 0, 40), (2, 0, 40)], cap, pooling)             # the second segment straddles a pass of 64
    check_map([(s, 0, 1) for s in range(64)], cap, pooling)
    check_map([(0, 0, 0), (1, 0, 5), (2, 0, 0)], cap, pooling)
    check_map([(1, 60, 10), (0, 0, 5), (2, 120, 12)], cap, pooling)           # one pass of three range buckets: the rows are re-ordered
    check_map([(s, 0, n) for s, n in enumerate((1, 2, 15, 63, 64, 65, 100, 3, 1))], cap, pooling)


def test_refusals():
    L = nb.lib()
    ok = nb.row_segs([(0, 0, 4), (1, 8, 4)])
    assert L.nano_hip_rows_pool_plan(ok.ctypes.data, 2, 64, S, 0, None, None) == 0
    assert L.nano_hip_rows_pool_plan(ok.ctypes.data, 2, 64, S, 1, None, None) == 0
    assert L.nano_hip_rows_pool_plan(ok.ctypes.data, 2, 64, S, 2, None, None) == EINVAL and "pooling" in nb.last_error()
    assert L.nano_hip_rows_pool_plan(None, 2, 64, S, 0, None, None) == EINVAL
    assert L.nano_hip_rows_pool_plan(None, 0, 64, S, 0, None, None) == 0
    assert L.nano_hip_rows_pool_plan(ok.ctypes.data, 2, 0, S, 0, None, None) == EINVAL
    for bad in ([(0, 0, 4, 1)], [(3, 0, 4), (3, 10, 1)], [(0, 250, 7)]):      # what nano_hip_rows_plan refuses
        s = nb.row_segs(bad)
        assert L.nano_hip_rows_pool_plan(s.ctypes.data, len(bad), 64, S, 1, None, None) == EINVAL, bad
