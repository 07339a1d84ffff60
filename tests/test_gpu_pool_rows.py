"""GPU tests of the pool kernel alone (pool.hip through nano_hip_op_pool_rows): the per-row final norm, LAST / MEAN pooling over segments
that straddle passes, truncation, normalisation.  Most of it needs no tolerance: the kernel's chains are fixed, so MEAN must be the
float32 ascending sum of the kernel's own per-row vectors divided by the count, whatever the pass cut.  Against float64 the bounds are
derived below from the summation orders pool.hip documents."""
import numpy as np
import pytest

import pool_ref as pr
from fused_ref import bits
from nano_amd import binding as nb

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                                               # unit roundoff of float32
EMBD = [128, 192, 1024, 2560, 130]                                           # (130: rows that are not 16-byte aligned -- the predicated dword path)
COUNTS = {"1": [1], "2": [2], "63": [63], "64": [64], "65": [65], "130": [130], "40x3": [40, 40, 40], "1x64": [1] * 64, "0-5-0": [0, 5, 0]}
CAPS = [1, 7, 64]
ROWS = 130


def gamma(k):
    return k * U / (1 - k * U)


def norm_bound(E):
    """Relative bound per component of the fast form's y[i] = w[i] * (x[i] * inv) against float64, from pool.hip's order.
    Sum of squares: a lane squares (1 rounding per term) and adds its 4 * ceil(E / 256) terms one at a time (one rounding per add; all
    terms >= 0, so the relative errors do not amplify), then the 6 levels of the xor butterfly: <= 4 * ceil(E / 256) + 1 + 6 roundings
    on any term's path.  Then sum / E and + 1e-5f (2 roundings; both summands >= 0); sqrtf halves the relative error accumulated so far
    and rounds once; 1 / . rounds once; x * inv and w * (.) round once each."""
    k_sum = 4 * -(-E // 256) + 1 + 6
    return gamma((k_sum + 2) / 2 + 4)


def unit_bound(dim):
    """Relative bound per component of out = v * (1 / sqrtf(sum v^2)) against the float64 normalisation of the same float32 v.
    Sum: a thread squares (1 rounding) and adds its 4 * ceil(dim / 1024) terms one at a time, the butterfly's 6 levels, then the 4 wave
    sums added in order (<= 4 roundings); sqrtf halves that and rounds once, the division rounds once, the product rounds once."""
    k_sum = 4 * -(-dim // 1024) + 1 + 6 + 4
    return gamma(k_sum / 2 + 3)


_base = {}


def base(E):
    """seeded rows and weights as test_rmsnorm draws them, and the kernel's own per-row vectors: every row fed as a one-row segment"""
    if E not in _base:
        rng = np.random.default_rng(E)
        x = (rng.standard_normal((ROWS, E)) * 3).astype(np.float32)
        w = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
        y = nb.op_pool_rows(x, w, [1] * ROWS, "last", False, 0, pass_cap=64)
        _base[E] = (x, w, y)
    return _base[E]


def ordered_mean(y, counts):
    """(((y_0 + y_1) + y_2) + ...) / count per segment, in float32; a segment without rows: zeros"""
    out, at = np.zeros((len(counts), y.shape[1]), np.float32), 0
    for i, c in enumerate(counts):
        if c:
            acc = y[at].copy()
            for r in range(at + 1, at + c):
                acc = acc + y[r]
            out[i] = acc / np.float32(c)
        at += c
    return out


def test_bounds_are_no_looser_than_the_existing_rmsnorm_tolerance():
    assert all(norm_bound(E) < 1e-5 for E in EMBD) and all(unit_bound(E) < 1e-5 for E in EMBD)


@pytest.mark.parametrize("E", EMBD)
def test_row_norm_against_float64(E):
    x, w, y = base(E)
    ref = pr.norm_rows_f64(x, w)
    d = np.abs(y.astype(np.float64) - ref)
    bound = norm_bound(E) * np.abs(ref)
    print(f"n_embd {E}: max relative error {float((d / np.abs(ref)).max()):.3e}, bound {norm_bound(E):.3e}")
    assert np.all(d <= bound), (float((d / np.abs(ref)).max()), norm_bound(E))


@pytest.mark.parametrize("name", list(COUNTS))
@pytest.mark.parametrize("E", EMBD)
def test_pooling_is_exact_whatever_the_cut(E, name):
    counts = COUNTS[name]
    rows = sum(counts)
    x, w, y = base(E)
    ends = np.cumsum(counts) - 1
    want_last = np.stack([y[e] if c else np.zeros(E, np.float32) for e, c in zip(ends, counts)])
    want_mean = ordered_mean(y[:rows], counts)
    for cap in CAPS:
        last = nb.op_pool_rows(x[:rows], w, counts, "last", False, 0, pass_cap=cap)
        mean = nb.op_pool_rows(x[:rows], w, counts, "mean", False, 0, pass_cap=cap)
        assert np.array_equal(bits(last), bits(want_last)), ("last", cap)
        assert np.array_equal(bits(mean), bits(want_mean)), ("mean", cap)


@pytest.mark.parametrize("E", EMBD)
def test_mean_of_one_row_is_last(E):
    x, w, _y = base(E)
    for normalize in (False, True):
        for dim in (0, 33):
            a = nb.op_pool_rows(x[:64], w, [1] * 64, "mean", normalize, dim)
            b = nb.op_pool_rows(x[:64], w, [1] * 64, "last", normalize, dim)
            assert np.array_equal(bits(a), bits(b)), (normalize, dim)


@pytest.mark.parametrize("pooling", ["last", "mean"])
@pytest.mark.parametrize("E", EMBD)
def test_truncation_normalisation_and_the_guard(E, pooling):
    x, w, _y = base(E)
    counts = [40, 40, 40]
    full = nb.op_pool_rows(x[:120], w, counts, pooling, False, 0)
    for dim in (0, 1, 33, E - 1, E):
        d = dim or E
        raw, tail = nb.op_pool_rows(x[:120], w, counts, pooling, False, dim, guard=64)
        assert np.array_equal(bits(raw), bits(full[:, :d])), dim             # dim = k is the first k components of dim = 0
        assert np.all(tail == 0xA5A5A5A5), dim
        unit, tail = nb.op_pool_rows(x[:120], w, counts, pooling, True, dim, guard=64)
        assert np.all(tail == 0xA5A5A5A5), dim
        for i in range(len(counts)):                                         # truncation first: unit length over the kept components
            ref = pr.normalize_f64(raw[i])
            err = np.abs(unit[i].astype(np.float64) - ref)
            assert np.all(err <= unit_bound(d) * np.abs(ref)), (dim, i, float((err / np.abs(ref)).max()), unit_bound(d))


@pytest.mark.parametrize("E", EMBD)
def test_zero_rows_and_empty_segments_give_zeros(E):
    _x, w, _y = base(E)
    z = np.zeros((6, E), np.float32)
    for pooling in ("last", "mean"):
        for dim in (0, 33):
            out = nb.op_pool_rows(z, w, [0, 5, 0, 1], pooling, True, dim, pass_cap=7)
            assert not np.isnan(out).any() and not out.any(), (pooling, dim)
    x, w, y = base(E)
    out = nb.op_pool_rows(x[:5], w, [0, 5, 0], "last", True, 0)              # rows only in the middle segment
    assert not out[0].any() and not out[2].any() and out[1].any()
    ref = pr.normalize_f64(y[4])
    assert np.all(np.abs(out[1].astype(np.float64) - ref) <= unit_bound(E) * np.abs(ref))
