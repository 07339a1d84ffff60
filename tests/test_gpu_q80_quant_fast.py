"""The Q80 activation quantizer's shared-reciprocal form on the device (device_common.h q80_quant4): one v_rcp_f32 per group, a
multiply per value, and the exact division (q80_quant1) only for a value whose scaled form lies within 2^-14 of a half-integer or is
not below 128.  The integers must be those of round(x / scale) (reference infer/tensor.c:21-46) BIT FOR BIT -- so the inputs here are
what that shortcut could get wrong: (k + 0.5) * scale for every k, nudged by -3..+3 ulp, both signs; an all-zero group (scale 0);
groups of denormals (denormal scales: the hardware reciprocal flushes them); a group whose maximum is the smallest normal number;
groups near 1e38 and FLT_MAX.  Finite values with quotients inside int8 only: the reference's cast of anything else is undefined.

  * nano_hip_op_quantize_q80 (misc.hip) against the oracle's quantizer, integers and scales;
  * the decode launches' own prologue (gemv_q80_impl.h stage_finish) through nano_hip_op_fused_gemv: residual roles take the
    activation as it is (no rmsnorm in front), so the planted values reach the quantizer; n = 3072 is the launch whose upper waves hold
    a dead second item (skipped as a whole wave), n = 1088 leaves one wave partly live behind the row's end (it runs everything and
    guards the store);
  * the rmsnorm roles at n = 1024 (q|k|v: store; W1|W3: SwiGLU), order-free inputs as in test_gpu_wave_fold.py.
tests/test_q80_quant_fast_order.py restates the arithmetic on the CPU and owns the group builders used here."""
import numpy as np
import pytest

from canon import matmul_q80_canon
from nano_amd import binding as nb
from test_q80_quant_fast_order import F, TINY, planted_groups
from fused_ref import bits, order_free

pytestmark = pytest.mark.gpu

Q80 = 0x80


def weights(rng, rows, n, gs=64):
    wq = rng.integers(-127, 128, size=rows * n, dtype=np.int8)
    ws = rng.uniform(1e-4, 2e-3, size=rows * n // gs).astype(F)
    return wq, ws


def special_groups(rng, gs):
    """zero, denormal, tiny and huge groups whose quotients the reference's cast defines (finite, |x / scale| <= 127)"""
    unit = np.float64(1.4012984643e-45)                       # the smallest denormal
    out = [np.zeros((1, gs), F)]                              # scale 0, 0 / 0: the reference's NaN cast gives 0 on x86-64, q80_quant1 returns 0
    for m in (1, 2, 5, 64, 1000, 60000):                      # max = 127 m units -> scale = m units exactly; j / m has exact ties for even m
        g = (rng.integers(-127 * m, 127 * m + 1, size=(1, gs)) * unit).astype(F); g[0, -1] = F(127 * m * unit)
        out.append(g)
    g = (rng.uniform(-1, 1, size=(2, gs)) * TINY).astype(F); g[:, -1] = TINY; out.append(g)          # the maximum is the smallest normal number
    g = (rng.uniform(-1, 1, size=(2, gs)) * 1e38).astype(F); g[:, -1] = F(1e38); out.append(g)
    g = (rng.uniform(-1, 1, size=(1, gs)) * 3.4e38).astype(F); g[0, -1] = np.finfo(F).max; out.append(g)
    return np.concatenate(out)


def planted_vector(rng, n, gs, maxima, special=False):
    """n values = n / gs whole groups drawn from the planted pool of `maxima` (the un-nudged ties and the +-1 ulp ones always among
    them), the special groups in front where asked"""
    pool, _ = planted_groups(np.asarray(maxima, F), gs)
    R = -(-127 // (gs - 1))
    sets = pool.reshape(len(maxima), 2, 7, R, gs)             # [maximum, sign, nudge -3..3, group of the set, gs]
    first = sets[:, :, 2:5].reshape(-1, gs)                   # nudges -1, 0, +1
    rest = np.concatenate([sets[:, :, :2].reshape(-1, gs), sets[:, :, 5:].reshape(-1, gs)])
    groups = [special_groups(rng, gs)] if special else []
    groups += [first, rest[rng.permutation(len(rest))]]
    x = np.concatenate(groups)[: n // gs]
    assert x.shape == (n // gs, gs), x.shape
    return x.reshape(-1).astype(F)


@pytest.mark.parametrize("gs", [64, 32])
def test_quantize_operator_matches_the_oracle(oracle, gs):
    rng = np.random.default_rng(gs)
    n = 4096
    cases = [planted_vector(rng, n, gs, [1.0, 0.37], special=True),             # the special groups, then ties under two scales
             planted_vector(rng, n, gs, [3.0e-5, 254.0, 1.7e30, 6.1e-31]),      # ties only, scales over sixty decades
             (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(F)]
    for x in cases:
        assert np.all(np.isfinite(x))
        wq, ws = oracle.quantize_q80(x, gs)
        gq, gscale = nb.op_quantize_q80(x, gs)
        assert np.array_equal(bits(gscale), bits(ws))
        bad = np.flatnonzero(gq != wq)
        assert bad.size == 0, (gs, bad.size, bad[:8], x[bad[:8]], gq[bad[:8]], wq[bad[:8]])


def ascending(oracle, xq, xs, wq, ws, n, rows, gs):
    """the reference's own fold, groups ascending (infer.c:668-674): what a row length that is no multiple of 256 gets on every route
    (kernels.h q80_canonical(); tests/canon.py restates the canonical fold of the other lengths only)"""
    return oracle.matmul_q80(xq, xs, wq, ws, n, rows, gs)


# Wo's shape of Qwen3-0.6B (one live item per thread), W2's (3072 on 512 threads: the second item of waves 4..7 is dead) and a row that
# ends inside a wave (1088 = 272 float4 items on 256 threads: the second item of wave 0 has 16 live lanes, of waves 1..3 none)
@pytest.mark.parametrize("n,rows", [(2048, 64), (3072, 64), (1088, 8)], ids=str)
def test_residual_roles_quantize_planted_ties_exactly(oracle, n, rows):
    gs = 64
    rng = np.random.default_rng(n)
    x = planted_vector(rng, n, gs, [1.0, 0.37, 254.0, 3.0e-5])
    old = rng.standard_normal(rows).astype(F)
    wq, ws = weights(rng, rows, n)
    xq, xs = oracle.quantize_q80(x, gs)
    fold = matmul_q80_canon if n % 256 == 0 else (lambda *a: ascending(oracle, *a))
    want = (old + fold(xq, xs, wq, ws, n, rows, gs)).astype(F)
    one, route = nb.op_fused_gemv(Q80, 1, n, [(wq, ws, rows)], x[None], None, gs=gs, resid=old[None], want_route=True)
    assert route == "gemv", route
    bad = np.flatnonzero(bits(one[0]) != bits(want))
    assert bad.size == 0, (n, rows, bad.size, bad[:8], one[0][bad[:8]], want[bad[:8]])
    two = nb.op_fused_gemv(Q80, 1, n, [(wq, ws, rows)], np.stack([x, x]), None, gs=gs, nb=2, resid=np.stack([old, old]))
    assert np.array_equal(bits(two[0]), bits(one[0])) and np.array_equal(bits(two[1]), bits(one[0]))


@pytest.mark.parametrize("kind", [0, 2], ids=["store", "swiglu"])
def test_norm_roles_are_canon(oracle, kind):
    """q|k|v's and W1|W3's shape, 64 rows: rmsnorm + quantize + projection.  Random ORDER-FREE inputs (sums of squares exact in any
    order: the rmsnorm tree's own order cannot move the quantized activation, test_gpu_fused_roles.py); the store form pins both
    projections bit for bit, the SwiGLU form carries the same bits on the one- and the two-sequence route"""
    n, gs, rows = 1024, 64, 64
    rng = np.random.default_rng(7 + kind)
    x = order_free(rng, n)
    nw = (1 + 0.1 * rng.standard_normal(n)).astype(F)
    segs = [(*weights(rng, rows, n), rows), (*weights(rng, rows, n), rows)]
    xq, xs = oracle.quantize_q80(oracle.rmsnorm(x, nw), gs)
    want = np.concatenate([matmul_q80_canon(xq, xs, wq, ws, n, r, gs) for wq, ws, r in segs])
    store = nb.op_fused_gemv(Q80, 0, n, segs, x[None], nw, gs=gs)[0]
    bad = np.flatnonzero(bits(store) != bits(want))
    assert bad.size == 0, (bad.size, bad[:8], store[bad[:8]], want[bad[:8]])
    if kind == 2:
        one, route = nb.op_fused_gemv(Q80, 2, n, segs, x[None], nw, gs=gs, want_route=True)
        assert route == "gemv", route
        two = nb.op_fused_gemv(Q80, 2, n, segs, np.stack([x, x]), nw, gs=gs, nb=2)
        assert np.array_equal(bits(two[0]), bits(one[0])) and np.array_equal(bits(two[1]), bits(one[0]))
        h1, h3 = want[:rows].astype(F), want[rows:].astype(F)
        sw = (h1 * (F(1) / (F(1) + np.exp(-h1.astype(np.float64)).astype(F))) * h3).astype(F)
        assert np.allclose(one[0], sw, rtol=3e-6, atol=1e-9)              # (the epilogue's expf is the device's: <= 2 ulp of libm)
