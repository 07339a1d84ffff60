"""The Q80 activation quantizer's shared-reciprocal form (device_common.h q80_quant4), restated in numpy with float32 operations
exactly as on the device, against roundf of the float32 quotient (q80_quant1, reference infer/tensor.c:21-46).

    ri = rcp(scale) once per group;  t = x * ri;  a = |t|;  f = fract(a)
    safe  <=>  |f - 0.5| > 2^-14  and  a < 128          (both false for NaN)
    safe:     q = (int) trunc(t + copysign(0.5, t))      (float32 add)
    not safe: q = q80_quant1(x, scale)                   (the exact division; trivially equal)

v_rcp_f32 is good to 1 ulp, so the reciprocal is tried as RN(1/s) and as each of its 1-ulp neighbours (the neighbours are up to 1.5 ulp
from 1/s: more than the hardware may err).  A denormal scale is tried both with its true reciprocal and flushed (ri = inf), which is
what the hardware does.  No GPU: tests/test_gpu_q80_quant_fast.py runs the kernels on the same groups."""
import numpy as np
import pytest

F = np.float32
DELTA = F(2.0 ** -14)
GS = 64
TINY = np.finfo(F).tiny            # the smallest normal number


def div127(m):
    """device_common.h div_const<127>: the correctly rounded m / 127 (checked exhaustively by tools/div_const_check.c)"""
    return (np.asarray(m, F) / F(127.0)).astype(F)


def exact(x, scale):
    """q80_quant1 for finite quotients: roundf (half away from zero) of the float32 quotient; NaN -> 0.  float64 holds every float32 +- 0.5 exactly."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = (x.astype(F) / scale.astype(F)).astype(F).astype(np.float64)
    r = np.trunc(q + np.copysign(0.5, q))
    return np.where(np.isnan(r), 0.0, r)


def fast(x, scale, ri):
    """-> (integers of the fast path as float64, safe mask)"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = (x.astype(F) * ri.astype(F)).astype(F)
        a = np.abs(t)
        f = (a - np.floor(a)).astype(F)                  # v_fract_f32: exact for finite a; inf - inf = NaN
        safe = (np.abs((f - F(0.5)).astype(F)) > DELTA) & (a < F(128.0))
        q = np.trunc((t + np.copysign(F(0.5), t)).astype(F)).astype(np.float64)
    return q, safe


def reciprocals(scale):
    """RN(1/s), its two 1-ulp neighbours, and the flushed form of a denormal (or zero) scale"""
    with np.errstate(divide="ignore", over="ignore"):
        r = (F(1.0) / scale.astype(F)).astype(F)
    lo = np.where(np.isinf(r), r, np.nextafter(r, F(0)))         # (1/s beyond the largest float is inf in every model, not FLT_MAX)
    out = [("rn", r), ("rn-1ulp", lo.astype(F)), ("rn+1ulp", np.nextafter(r, F(np.inf)))]
    out.append(("flushed", np.where(np.abs(scale) < TINY, F(np.inf), r).astype(F)))
    return out


def check(x, want_rejected=None, max_rejected_share=None):
    """x: [groups, group size].  Zero mismatches among the accepted values, for every modelled reciprocal."""
    x = np.ascontiguousarray(x, F)
    scale = np.repeat(div127(np.abs(x).max(axis=1))[:, None], x.shape[1], axis=1)
    want = exact(x, scale)
    shares = []
    for name, ri in reciprocals(scale):
        q, safe = fast(x, scale, ri)
        bad = safe & (q != want)
        assert not bad.any(), (name, int(bad.sum()), x[bad][:4], scale[bad][:4], q[bad][:4], want[bad][:4])
        # (a rejected value takes q80_quant1 itself: equal to `want` by construction)
        if want_rejected is not None:
            missed = want_rejected & safe
            assert not missed.any(), (name, int(missed.sum()), x[missed][:4], scale[missed][:4])
        shares.append(1.0 - float(safe.mean()))
    if max_rejected_share is not None:
        assert max(shares) <= max_rejected_share, shares
    return shares


def nudge(v, k):
    """v moved by k ulp (k in -3..3)"""
    v = np.asarray(v, F).copy()
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf))
    return v


def planted_groups(group_max, gs=GS):
    """For every group maximum M: scale s = M / 127; groups that hold RN((k + 0.5) s) for k = 0..126, each nudged by -3..+3 ulp, both
    signs, next to M itself in the group's last place (so the scale stays s).
    -> (x [groups, gs], mask of the NORMAL values within 3 ulp of the real tie (k + 0.5) s)"""
    rows, near = [], []
    ks = np.arange(127, dtype=np.float64) + 0.5
    R = -(-127 // (gs - 1))                                       # groups per set of 127 ties
    for M in np.asarray(group_max, F):
        tie = ks * np.float64(div127(M))                          # exact in float64
        for sign in (1.0, -1.0):
            for d in range(-3, 4):
                v = np.zeros(R * (gs - 1), F); t = np.zeros(R * (gs - 1)); planted = np.zeros(R * (gs - 1), bool)
                v[:127] = nudge((sign * tie).astype(F), d); t[:127] = sign * tie; planted[:127] = True
                g = np.concatenate([v.reshape(R, gs - 1), np.full((R, 1), M, F)], axis=1)
                t = np.concatenate([t.reshape(R, gs - 1), np.zeros((R, 1))], axis=1)
                planted = np.concatenate([planted.reshape(R, gs - 1), np.zeros((R, 1), bool)], axis=1)
                ulp = np.spacing(np.abs(g)).astype(np.float64)
                rows.append(g)
                # (a NORMAL x only: 3 ulp of a denormal are not 3 * 2^-23 of it, and the quotient may move by more than delta)
                near.append(planted & (np.abs(g.astype(np.float64) - t) <= 3.0 * ulp) & (np.abs(g) >= TINY))
    return np.concatenate(rows), np.concatenate(near)


def test_random_groups_over_many_decades():
    """group magnitudes over 36 decades (1e-18 .. 1e18), normal and uniform values: no mismatch, and the fallback stays rare -- at most
    1e-3 of the values, so the test cannot pass by rejecting everything (the bound's own estimate: 4 delta = 2.4e-4 for evenly spread
    fractional parts, less on bell-shaped data)"""
    rng = np.random.default_rng(80)
    G = 1 << 14
    mag = (10.0 ** rng.uniform(-18, 18, size=(G, 1)))
    x = np.concatenate([(rng.standard_normal((G, GS)) * mag).astype(F), (rng.uniform(-1, 1, size=(G, GS)) * mag).astype(F)])
    assert np.log10(np.abs(x).max(axis=1).max() / np.abs(x).max(axis=1).min()) >= 12
    shares = check(x, max_rejected_share=1e-3)
    assert min(shares[:3]) > 0                   # (some value of 2 M does lie next to a tie: the fallback is exercised)


def test_planted_ties_take_the_fallback():
    """(k + 0.5) * scale for k = 0..126, nudged by -3..+3 ulp, both signs, under scales with mantissas across the binade and from 1e-30
    to 1e30: every value within 3 ulp of a tie is rejected (3 ulp of x are at most 3 * 126.5 * 2^-23 of the quotient, t adds its
    own error: inside delta), and whatever is accepted is right"""
    rng = np.random.default_rng(81)
    M = np.concatenate([rng.uniform(1, 2, 24) * 10.0 ** rng.integers(-30, 31, 24), [127.0, 1.0, 254.0, 126.99999, 3.0e-5]]).astype(F)
    for gs in (64, 32):
        x, near = planted_groups(M, gs)
        assert x.shape[1] == gs and near.sum() >= 127 * 2 * 5 * M.size            # (nudges of -2..+2 ulp always stay within 3 ulp of the real tie)
        check(x, want_rejected=near)


def test_zero_denormal_tiny_and_huge_groups():
    rng = np.random.default_rng(82)
    zero = np.zeros((1, GS), F)                                              # scale 0: 0 * inf = NaN -> fallback -> 0
    den = (rng.integers(-8000, 8001, size=(64, GS)) * 1.4e-45).astype(F)     # groups of denormals, denormal or zero scales
    den_small = (rng.integers(-40, 41, size=(8, GS)) * 1.4e-45).astype(F)    # ... whose scale rounds to zero or one unit
    tiny = (rng.uniform(-1, 1, size=(8, GS)) * TINY).astype(F); tiny[:, 0] = TINY        # the maximum is the smallest normal number
    huge = (rng.uniform(-1, 1, size=(8, GS)) * 1e38).astype(F); huge[:, 0] = F(1e38)
    top = (rng.uniform(-1, 1, size=(4, GS)) * 3.4e38).astype(F); top[:, 0] = np.finfo(F).max
    for x in (zero, den, den_small, tiny, huge, top):
        check(x)
    x, near = planted_groups(np.asarray([TINY, 1e38, 4096 * 1.4e-45, 2.0e-36], F))
    check(x, want_rejected=near)
    # the all-zero group: every value rejected, every integer 0
    s0 = np.zeros((1, GS), F)
    for _, ri in reciprocals(s0):
        _, safe = fast(zero, s0, ri)
        assert not safe.any()
    assert not exact(zero, s0).any()
