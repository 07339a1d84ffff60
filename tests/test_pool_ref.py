"""CPU tests of tests/pool_ref.py, the numpy statement of the pooled final-norm vector the GPU tests compare against."""
import numpy as np

import pool_ref as pr
from fused_ref import bits


def rows(seed, count, E):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((count, E)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    return x, w


def test_mean_of_one_row_is_last(oracle):
    x, w = rows(1, 1, 96)
    y = pr.norm_rows_ordered(oracle, x, w)
    for normalize in (False, True):
        for dim in (0, 33):
            a, b = pr.pool_ordered(y, "mean", normalize, dim), pr.pool_ordered(y, "last", normalize, dim)
            assert np.array_equal(bits(a), bits(b)), (normalize, dim)


def test_last_is_the_last_rows_norm(oracle):
    x, w = rows(2, 5, 64)
    y = pr.norm_rows_ordered(oracle, x, w)
    assert np.array_equal(bits(pr.pool_ordered(y, "last", False)), bits(oracle.rmsnorm(x[4], w)))
    assert np.allclose(y, pr.norm_rows_f64(x, w), rtol=1e-5, atol=0)


def test_truncation_happens_before_normalisation(oracle):
    x, w = rows(3, 7, 128)
    y = pr.norm_rows_ordered(oracle, x, w)
    for pooling in ("last", "mean"):
        full, cut = pr.pool_ordered(y, pooling, True, 0), pr.pool_ordered(y, pooling, True, 40)
        raw = pr.pool_ordered(y, pooling, False, 0)
        assert np.array_equal(bits(pr.pool_ordered(y, pooling, False, 40)), bits(raw[:40]))
        assert abs(float(np.linalg.norm(cut.astype(np.float64))) - 1.0) < 1e-6         # unit length over the kept components ...
        assert float(np.linalg.norm(full[:40].astype(np.float64))) < 0.99             # ... which a cut of the normalised full vector is not
        assert np.allclose(cut, pr.pool_f64(y, pooling, True, 40), rtol=1e-5, atol=1e-7)


def test_zero_vector_gives_zeros():
    y = np.zeros((3, 32), np.float32)
    for pooling in ("last", "mean"):
        out = pr.pool_ordered(y, pooling, True, 0)
        assert not np.isnan(out).any() and not out.any()
        assert not pr.pool_f64(y, pooling, True, 5).any()
    assert not pr.pool_ordered(np.zeros((0, 32), np.float32), "mean", True, 8).any()   # a segment without rows


def test_ordered_mean_does_not_depend_on_the_pass_cut(oracle):
    x, w = rows(4, 70, 64)
    y = pr.norm_rows_ordered(oracle, x, w)
    whole = pr.pool_ordered(y, "mean", True, 0)
    acc = y[0].copy()
    for r in range(1, 70):
        acc = acc + y[r]
    assert np.array_equal(bits(pr.pool_ordered(y, "mean", False, 0)), bits(acc / np.float32(70)))
    for cuts in ((1,), (64,), (7, 8, 69), tuple(range(1, 70))):
        assert np.array_equal(bits(pr.pool_ordered(y, "mean", True, 0, cuts=cuts)), bits(whole)), cuts


def test_embed_ordered_walks_the_segments(oracle):
    x, w = rows(5, 9, 48)
    out = pr.embed_ordered(oracle, x, w, [0, 5, 0, 4], "mean", True, 0)
    assert out.shape == (4, 48) and not out[0].any() and not out[2].any()
    assert np.array_equal(bits(out[3]), bits(pr.pool_ordered(pr.norm_rows_ordered(oracle, x[5:], w), "mean", True, 0)))
