"""CPU test: the 64-bit key topk.hip selects by -- (ord(logit) << 32) | (0xffffffff - index), restated in numpy (topk_ref.keys) --
orders planted floats exactly as the reference order does (float comparison descending, equal floats by index)."""
import numpy as np

from topk_ref import key_ord, keys, ref_topk

FLT_MIN = np.float32(1.17549435e-38)
FLT_MAX = np.float32(3.40282347e38)
DEN_MIN = np.uint32(1).view(np.float32)                      # the smallest positive denormal
DEN_MAX = np.uint32(0x007FFFFF).view(np.float32)             # the largest


def planted():
    v = [0.0, -0.0, DEN_MIN, -DEN_MIN, DEN_MAX, -DEN_MAX, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX, -np.inf,
         1.5, 1.5, -0.0, 0.0, -np.inf, DEN_MIN, -DEN_MAX, -2.25, -2.25, FLT_MAX, 1e-30, -1e-30]
    return np.array(v, np.float32)


def test_key_orders_planted_floats_as_the_reference():
    x = planted()
    want = ref_topk(x[None, :], x.size)[0]
    got = np.argsort(keys(x))[::-1].astype(np.uint32)        # the largest key first (keys are distinct: any sort is the order)
    assert len(set(keys(x).tolist())) == x.size
    assert np.array_equal(got, want)
    for seed in range(4):                                    # and in every arrangement of the same values
        p = np.random.default_rng(seed).permutation(x.size)
        y = x[p]
        assert np.array_equal(np.argsort(keys(y))[::-1].astype(np.uint32), ref_topk(y[None, :], y.size)[0])


def test_key_properties():
    x = planted()
    o = key_ord(x)
    assert o[0] == o[1] == 0x80000000                        # +-0 tie: the index decides
    assert key_ord(np.float32(-np.inf)) == 0x007FFFFF and o.min() == 0x007FFFFF      # no key of a row without NaN is 0 ("no candidate")
    assert key_ord(DEN_MIN) == 0x80000001 and key_ord(-DEN_MIN) == 0x7FFFFFFE        # denormals order as integers: nothing to flush
    r = np.random.default_rng(7).standard_normal(4096).astype(np.float32) * np.float32(50)
    order = np.argsort(r, kind="stable")
    assert np.all(np.diff(key_ord(r[order]).astype(np.int64)) >= 0)                  # monotone in the float
    # a tile's indices share their upper 20 bits: the low words of its keys do too (the threshold search skips them)
    base = 5 * 4096
    lo = np.uint32(0xFFFFFFFF) - (base + np.arange(4096, dtype=np.uint32))
    assert np.all((lo & np.uint32(0xFFFFF000)) == (~np.uint32(base) & np.uint32(0xFFFFF000)))
