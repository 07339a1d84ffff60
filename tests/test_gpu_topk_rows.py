"""GPU tests of the top-k selection alone (nano_hip_op_topk_rows: score.hip's two launches, then topk.hip's two) against the numpy
reference of tests/topk_ref.py: tokens equal, logit and logprob bit for bit, consistent with the row's score record."""
import numpy as np
import pytest

from nano_amd import binding as nb
from topk_ref import bits, check_topk, ref_topk

pytestmark = pytest.mark.gpu

TILE = 4096
KS = (1, 5, 20, 32)


def random_rows(rows, V, seed):
    return (np.random.default_rng(seed).standard_normal((rows, V)) * 4.0).astype(np.float32)


def targets_for(l, k, seed):
    """half of the rows: one of the row's own best k (so the target is among the entries), the others: any token"""
    rows, V = l.shape
    rng = np.random.default_rng(seed)
    t = rng.integers(0, V, rows).astype(np.uint32)
    best = ref_topk(l, k)
    for r in range(0, rows, 2):
        t[r] = best[r, rng.integers(0, k)]
    return t


@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("V", [1, 5, 512, 4097, 20000])
def test_random_rows(V, rows):
    """4097: the last tile holds one logit (fewer than k candidates) and the rows are not 16-byte aligned"""
    l = random_rows(rows, V, 1000 * rows + V)
    for k in sorted({min(k, V) for k in KS}):
        sc, top = nb.op_topk_rows(l, k)
        check_topk(top, sc, l, k, None, f"V={V} rows={rows} k={k}")
        t = targets_for(l, k, k)
        sc, top = nb.op_topk_rows(l, k, t)
        check_topk(top, sc, l, k, t, f"V={V} rows={rows} k={k} with targets")


@pytest.mark.parametrize("rows,k", [(3, 32), (64, 20)])
def test_full_vocabulary(rows, k):
    V = 151936
    l = random_rows(rows, V, rows)
    t = targets_for(l, k, 5)
    sc, top = nb.op_topk_rows(l, k, t)
    check_topk(top, sc, l, k, t, f"V={V} rows={rows} k={k}")


# ---- planted rows: V = 3 tiles + 37 logits (an odd V: every second row is not 16-byte aligned; the last tile can hold k = 32) ----
PV = 3 * TILE + 37


def planted_rows():
    rng = np.random.default_rng(2024)
    base = lambda: rng.uniform(-1.0, 1.0, PV).astype(np.float32)
    rows, names = [], []

    def add(name, x):
        names.append(name); rows.append(np.ascontiguousarray(x, np.float32))

    add("all equal", np.full(PV, 0.5, np.float32))
    x = base(); x[100] = x[2000] = 9.0; add("the maximum twice inside a tile", x)
    x = base(); x[TILE - 1] = x[TILE] = 9.0; add("the maximum twice across a tile boundary", x)
    x = base(); x[3 * TILE:] = 10.0 + rng.permutation(37); add("the k largest in the last tile", x)
    x = base()
    for t in range(4):
        x[t * TILE + 11 * t + 3] = 9.0 - t
    add("one per tile", x)
    x = base(); i = 37
    x[[TILE + 4 * i + c + 1024 * j for j in range(4) for c in range(4)]] = 20.0 + rng.permutation(16); add("16 held by one thread", x)
    x = base(); x[2 * TILE + 4 * 128:2 * TILE + 4 * 128 + 32] = 30.0 + rng.permutation(32); add("32 in one wave's quarter of a tile", x)
    x = base(); x[2 * TILE + 4 * 128:2 * TILE + 4 * 192] += 50.0; add("one wave's whole quarter above the rest", x)
    add("sorted ascending", np.sort(base()))
    add("sorted descending", np.sort(base())[::-1])
    x = np.zeros(PV, np.float32); x[1::2] = -0.0; add("alternating +0.0 / -0.0", x)
    d = rng.integers(1, 0x00800000, PV).astype(np.uint32)
    d[::3] |= 0x80000000
    add("denormals of both signs", d.view(np.float32))
    x = base(); x[rng.random(PV) < 0.3] = -np.inf; add("-inf scattered", x)
    x = base(); x[:2 * TILE] = -np.inf; add("two whole tiles of -inf", x)
    x = np.full(PV, -np.inf, np.float32); x[[5, TILE + 1, TILE + 2, 3 * TILE - 1, 3 * TILE, PV - 1, 77]] = [1.0, -3.0, 2.5, 2.5, 0.0, -0.0, 1e-40]
    add("fewer than k finite logits", x)
    add("offset +1e4", base() + np.float32(1e4))
    add("offset -1e4", base() - np.float32(1e4))
    return names, np.stack(rows)


_planted = {}


def planted_run(k):
    if k not in _planted:
        names, l = planted_rows()
        sc, top = nb.op_topk_rows(l, k)
        _planted[k] = (names, l, sc, top)
    return _planted[k]


@pytest.mark.parametrize("k", [1, 5, 16, 20, 32])
def test_planted_rows(k):
    names, l, sc, top = planted_run(k)
    for r, name in enumerate(names):
        check_topk(top[r:r + 1], sc[r:r + 1], l[r:r + 1], k, None, f"{name}, k={k}")
    r = names.index("all equal")
    assert np.array_equal(top["token"][r], np.arange(k))
    r = names.index("alternating +0.0 / -0.0")
    assert np.array_equal(top["token"][r], np.arange(k)) and np.array_equal(bits(top["logit"][r]) >> 31, np.arange(k) & 1)
    r = names.index("fewer than k finite logits")
    if k > 7:
        assert np.all(np.isneginf(top["logit"][r, 7:])) and np.all(np.isneginf(top["logprob"][r, 7:]))
        assert np.array_equal(top["token"][r, 7:], np.setdiff1d(np.arange(PV), [5, TILE + 1, TILE + 2, 3 * TILE - 1, 3 * TILE, PV - 1, 77])[:k - 7])
    # with targets: the row's own j-th best and a token that is not among the entries
    want = ref_topk(l, k)
    for t in (want[:, k - 1], want[:, 0], np.full(l.shape[0], PV - 2, np.uint32)):
        sc_t, top_t = nb.op_topk_rows(l, k, t)
        check_topk(top_t, sc_t, l, k, t, f"planted rows with targets, k={k}")
        assert top_t.tobytes() == top.tobytes()


def test_a_rows_entries_do_not_depend_on_where_the_row_is():
    """the same row as row 0 of 1, row 2 of 3 and row 63 of 64 (an odd V: the alignments differ): the same bytes"""
    k = 20
    row = random_rows(1, PV, 77)[0]
    out = []
    for rows, at in ((1, 0), (3, 2), (64, 63)):
        l = random_rows(rows, PV, 78 + rows)
        l[at] = row
        sc, top = nb.op_topk_rows(l, k)
        out.append((sc[at].tobytes(), top[at].tobytes()))
    assert out[0] == out[1] == out[2]
