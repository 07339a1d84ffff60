"""GPU tests of the FP32 MFMA GEMM (nano_amd/csrc/gemm_f32.hip): 9..64 tokens per weight read of FP32 models, through the step's own
router (nb.op_fused_gemv(0x00, ..., use_gemm=True)); nb.f32_gemm_plan reports the plan the launcher follows.

The contract is the FP32 GEMV's bits.  The GEMV's row is, per 256-float chunk, a lane's float4 (one multiply, three fused multiply-adds),
a balanced pairwise tree over the 64 lanes, and the chunk sums added in ascending order from 0.0f (gemv_f32_slab_body.inc).  The GEMM
takes the lane's chain from v_mfma_f32_16x16x4_f32 with a zero accumulator, adds the same tree with plain fp32 adds and folds the same
way -- so every token's rows must be, BIT FOR BIT,
    (a) the same launch of that token alone (nb = 1: the GEMV), and
    (b) the same nb through the sliced route (use_gemm=False: the GEMV in groups of 8).
test_order_* is the verification of the MFMA claim: general random weights and activations, where every association of the sum rounds
differently.  The norm cases use order-free activations (sums of squares exact in any order: the rmsnorm scale does not depend on a
launch's thread count) and are also held against float64 within tests/test_gpu_f32_gemv.py's derived per-row bound
    |d| <= (10 + nchunk) 2^-24 sum|w_i a_i| + 2^-24 |ref|
and the project's 1e-5 bar; that bound is derived there and is not loosened here.  The exact cases (integer multiples of powers of two:
every partial sum of any association is exact) are bit for bit float64: a dropped, doubled or misplaced item, unit, row or token
cannot pass.  Every launch runs in a guarded buffer: one guard float behind every token's rows, 8 guard slots behind the last token.
Helpers are copies of tests/test_gpu_f32_gemv.py's."""
import numpy as np
import pytest

from nano_amd import binding as nb
from fused_ref import bits, order_free, silu_mul, rows_total

F32 = 0x00
U = 2.0 ** -24
SENTINEL = np.float32(-12345.678)


def exact_weights(rng, rows, n):
    """multiples of 2^-4 in [-1, 1]"""
    return (rng.integers(-16, 17, size=(rows, n), dtype=np.int8).astype(np.float32) / np.float32(16.0)).astype(np.float32)


def dot64(W, a):
    a = a.astype(np.float64)
    w = W.astype(np.float64)
    return w @ a, np.abs(w) @ np.abs(a)


def row_bound(ref, S, n):
    return (10 + (n + 255) // 256) * U * S + U * np.abs(ref)


def swiglu_bound(h1, S1, h3, S3, n):
    e1, e3 = row_bound(h1, S1, n), row_bound(h3, S3, n)
    silu = h1 / (1.0 + np.exp(-h1))
    return silu * h3, 1.1 * e1 * np.abs(h3) + np.abs(silu) * e3 + 1.1 * e1 * e3 + 3e-6 * np.abs(silu * h3)


def run(kind, n, W, x, nw, old, use_gemm, want_route):
    """the launch of all tokens in a guarded buffer; returns out[nb, rows_total] after checking the route and the guards"""
    nb_, rt = x.shape[0], rows_total(kind, [w.shape[0] for w in W])
    g = np.full((nb_ + 8, rt + 1), SENTINEL, np.float32)
    if old is not None:
        g[:nb_, :rt] = old
    _, route = nb.op_fused_gemv(F32, kind, n, [(w, None, w.shape[0]) for w in W], x, nw, nb=nb_, guard=g, use_gemm=use_gemm, want_route=True)
    assert route == want_route, (route, want_route)
    assert np.all(bits(g[:, rt]) == bits(SENTINEL)), "a guard element behind a token's rows changed"
    assert np.all(bits(g[nb_:]) == bits(SENTINEL)), "slots beyond the batch were written"
    return g[:nb_, :rt].copy()


def alone(kind, n, W, x, nw, old, b):
    return nb.op_fused_gemv(F32, kind, n, [(w, None, w.shape[0]) for w in W], x[b:b + 1], nw, nb=1,
                            resid=old[b:b + 1] if old is not None else None)[0]


def hold_against_gemv(kind, n, W, x, nw, old, tokens=None, sliced=True):
    """the GEMM launch, bit for bit (a) every token alone and (b) the sliced route; returns the GEMM's output"""
    out = run(kind, n, W, x, nw, old, True, "f32_gemm")
    for b in (range(x.shape[0]) if tokens is None else tokens):
        one = alone(kind, n, W, x, nw, old, b)
        bad = np.flatnonzero(bits(out[b]) != bits(one))
        assert not bad.size, ("token", b, "differs from its launch alone in rows", bad[:8], float(np.abs(out[b] - one).max()))
    if sliced:
        ref = run(kind, n, W, x, nw, old, False, "gemv_sliced")
        bad = np.argwhere(bits(out) != bits(ref))
        assert not bad.size, ("differs from the sliced route at (token, row)", bad[:8])
    return out


_weights = {}


def general_weights(n, rows):
    key = (n, rows)
    if key not in _weights:
        rng = np.random.default_rng(n * 13 + sum(rows) + len(rows))
        _weights[key] = [(0.02 * rng.standard_normal((r, n), dtype=np.float32)).astype(np.float32) for r in rows]
    return _weights[key]


# what the cases reach, from the reported plans (the closing coverage test)
SEEN = []


def note(kind, n, rows, nb_, norm=False):
    p = nb.f32_gemm_plan(kind, n, rows, nb_, norm=norm)
    assert nb.ROUTE_NAMES[p["route"]] == "f32_gemm", (kind, n, rows, nb_, p)
    SEEN.append(p)
    return p


ORDER_N = [256, 352, 768, 1408, 2048]           # one chunk, a partial chunk, three, 5 1/2, eight
ORDER_NB = [9, 16, 17, 33, 64]                  # a ragged first tile, a whole one, one over, a third tile begun, all four


# ---- 1. the order test: the verification of the MFMA claim ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rows", [(16,), (48,), (128, 64, 64)], ids=lambda r: "x".join(map(str, r)))
@pytest.mark.parametrize("n", ORDER_N)
def test_order_store_and_residual(n, rows):
    """kinds 0 and 1 on general random floats without a norm, every token count; kind 1 on general old residual values"""
    W = general_weights(n, rows)
    for nb_ in ORDER_NB:
        rng = np.random.default_rng(n + 7 * nb_ + sum(rows))
        x = rng.standard_normal((nb_, n)).astype(np.float32)
        for kind in (0, 1):
            if kind == 1 and len(rows) > 1:
                continue
            old = rng.standard_normal((nb_, sum(rows))).astype(np.float32) if kind == 1 else None
            note(kind, n, rows, nb_)
            # every token alone at the edges of the token tiles, all of them at the smallest and the largest count
            tokens = None if nb_ in (9, 64) and rows == (16,) else sorted({0, 8, 15, 16, 31, 32, nb_ - 1} & set(range(nb_)))
            hold_against_gemv(kind, n, W, x, None, old, tokens=tokens)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ORDER_N)
def test_order_swiglu(n):
    """kind 2: the W1 and the W3 tile of the same rows in one workgroup, two accumulator sets"""
    rows = (48, 48)
    W = general_weights(n, rows)
    for nb_ in ORDER_NB:
        rng = np.random.default_rng(n + 11 * nb_)
        x = rng.standard_normal((nb_, n)).astype(np.float32)
        note(2, n, rows, nb_)
        hold_against_gemv(2, n, W, x, None, None, tokens=sorted({0, 15, 16, nb_ - 1} & set(range(nb_))))


# ---- 2. norm cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,rows,nb_", [(0, 768, (128, 64, 64), 17), (0, 352, (48,), 9), (2, 768, (48, 48), 33), (0, 2048, (16,), 64),
                                             (2, 1408, (32, 32), 16)])
def test_norm_cases(oracle, kind, n, rows, nb_):
    rng = np.random.default_rng(n + nb_ + kind)
    W = general_weights(n, rows)
    x = order_free(rng, (nb_, n))
    nw = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    note(kind, n, rows, nb_, norm=True)
    out = hold_against_gemv(kind, n, W, x, nw, None)
    worst = 0.0
    for b in range(nb_):
        a = oracle.rmsnorm(x[b], nw)
        refs = [dot64(w, a) for w in W]
        if kind == 2:
            ref, bound = swiglu_bound(refs[0][0], refs[0][1], refs[1][0], refs[1][1], n)
        else:
            ref = np.concatenate([r for r, _ in refs]); S = np.concatenate([s for _, s in refs])
            bound = row_bound(ref, S, n)
        d = np.abs(out[b].astype(np.float64) - ref)
        worst = max(worst, float((d / bound).max()))
        assert not np.any(d > bound), (b, "rows beyond the per-row bound", np.flatnonzero(d > bound)[:6], float((d / bound).max()))
        assert float(d.max() / np.abs(ref).max()) <= 1e-5, (b, float(d.max() / np.abs(ref).max()))
    print(f"norm case kind {kind} n {n} rows {rows} nb {nb_}: worst |d| / bound {worst:.3f}")


# ---- 3. exact cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,rows,nb_", [(0, 352, (48, 16, 16), 17), (1, 1408, (48,), 33), (0, 2048, (32,), 64), (1, 260, (16,), 9),
                                             (0, 4, (16,), 16), (2, 768, (32, 32), 48)])
def test_exact_cases(kind, n, rows, nb_):
    rng = np.random.default_rng(n * 3 + nb_ + kind)
    W = [exact_weights(rng, r, n) for r in rows]
    x = order_free(rng, (nb_, n))
    old = (rng.integers(-1024, 1025, size=(nb_, sum(rows))).astype(np.float32) / np.float32(256.0)) if kind == 1 else None
    assert (n * 2.0 + 4.0) / 2.0 ** -8 <= 2 ** 24, "inputs are not exact in fp32"
    note(kind, n, rows, nb_)
    out = run(kind, n, W, x, None, old, True, "f32_gemm")
    for b in range(nb_):
        refs = [dot64(w, x[b])[0] for w in W]
        if kind == 2:
            h1, h3 = refs[0].astype(np.float32), refs[1].astype(np.float32)
            assert np.array_equal(h1.astype(np.float64), refs[0]) and np.array_equal(h3.astype(np.float64), refs[1])
            assert np.allclose(out[b], silu_mul(h1, h3), rtol=3e-6, atol=1e-9), b
            assert np.array_equal(bits(out[b]), bits(alone(kind, n, W, x, None, None, b))), ("alone", b)
            continue
        ref = np.concatenate(refs) + (old[b].astype(np.float64) if kind == 1 else 0.0)
        want = ref.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), ref), "the reference itself is not exact in fp32"
        bad = np.flatnonzero(bits(out[b]) != bits(want))
        assert not bad.size, (b, "rows differ from the exact result", bad[:8], float(np.abs(out[b] - want).max()))


# ---- 4. zeros and subnormals ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_zeros_and_subnormals():
    n, rows, nb_ = 352, 32, 17
    rng = np.random.default_rng(5)
    # an all-zero weight row (and a zero tail of another) against negative activations: products -0.0 in the GEMV, +0.0 from the MFMA
    W = (0.02 * rng.standard_normal((rows, n))).astype(np.float32)
    W[3] = 0.0
    W[7, 100:] = 0.0
    x = -np.abs(rng.standard_normal((nb_, n))).astype(np.float32)
    for kind in (0, 1):
        old = np.zeros((nb_, rows), np.float32) if kind == 1 else None
        if old is not None:
            old[:, 3] = -0.0
        out = hold_against_gemv(kind, n, [W], x, None, old)
        assert np.all(bits(out[:, 3]) == 0), "0.0f + a zero chunk sum is +0.0 (kind 1: -0.0 + +0.0)"
    # zero activations (one whole token, one token's tail) against negative weights
    Wn = -np.abs(W) - np.float32(0.01)
    x0 = rng.standard_normal((nb_, n)).astype(np.float32)
    x0[4] = 0.0
    x0[9, 128:] = 0.0
    hold_against_gemv(0, n, [Wn], x0, None, None)
    # subnormal products: 2^-100 x 2^-40 = 2^-140, signs mixed, sums stay subnormal
    sgn = np.where(rng.integers(0, 2, (rows, n)) == 1, 1.0, -1.0)
    Ws = (sgn * 2.0 ** -100).astype(np.float32)
    xs = (np.where(rng.integers(0, 2, (nb_, n)) == 1, 1.0, -1.0) * 2.0 ** -40 * rng.integers(1, 4, (nb_, n))).astype(np.float32)
    out = hold_against_gemv(0, n, [Ws], xs, None, None)
    ref = Ws.astype(np.float64) @ xs.astype(np.float64).T                      # exact: small integer multiples of 2^-140
    assert np.array_equal(out.astype(np.float64), ref.T.astype(np.float32).astype(np.float64)) and np.any(out != 0), "subnormals were flushed"


# ---- 5. refused shapes keep the sliced route ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_shapes_keep_the_sliced_route():
    rng = np.random.default_rng(77)
    n, nb_ = 768, 17
    # rows = 20: no multiple of 16
    W = [exact_weights(rng, 20, n)]
    x = order_free(rng, (nb_, n))
    assert nb.ROUTE_NAMES[nb.f32_gemm_plan(0, n, (20,), nb_)["route"]] == "gemv_sliced"
    out = run(0, n, W, x, None, None, True, "gemv_sliced")
    want = (W[0].astype(np.float64) @ x.astype(np.float64).T).T.astype(np.float32)
    assert np.array_equal(bits(out), bits(want))
    # split-attention partials (at most 8 sequences reach the FP32 GEMV with them; the GEMM starts at 9): the router keeps the GEMV
    assert nb.ROUTE_NAMES[nb.f32_gemm_plan(1, n, (16,), 8, attn=(16, 48, 4))["route"]] == "gemv"
    n_head, hd, ls = 16, 48, (1, 3, 2, 2)
    part = order_free(rng, (8, len(ls), n))
    ml = np.zeros((8, n_head, len(ls), 2), np.float32); ml[..., 0] = 0.25; ml[..., 1] = np.asarray(ls, np.float32)
    xa = (part.astype(np.float64).sum(axis=1) / sum(ls)).astype(np.float32)
    Wa = exact_weights(rng, 16, n)
    old = (rng.integers(-1024, 1025, size=(8, 16)).astype(np.float32) / np.float32(256.0))
    out, route = nb.op_fused_gemv(F32, 1, n, [(Wa, None, 16)], None, None, nb=8, resid=old, attn=(part, ml, n_head, hd), use_gemm=True, want_route=True)
    assert route == "gemv", route
    want = (old.astype(np.float64) + (Wa.astype(np.float64) @ xa.astype(np.float64).T).T).astype(np.float32)
    assert np.array_equal(bits(out), bits(want))


# ---- 6. coverage --------------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_template_value_and_plan_axis():
    """from the reported plans (CPU): the cases above reach both template values of gemm_f32_kernel<SW>, every token-tile count, one and
    several units per wave, fewer waves than 8 and all 8, a ragged last unit and an odd unit count"""
    T = []
    for n in ORDER_N:
        for nb_ in ORDER_NB:
            for rows in ((16,), (48,), (128, 64, 64)):
                T.append(dict(nb.f32_gemm_plan(0, n, rows, nb_), n=n))
            T.append(dict(nb.f32_gemm_plan(1, n, (48,), nb_), n=n))
            T.append(dict(nb.f32_gemm_plan(2, n, (48, 48), nb_), n=n))
    assert all(nb.ROUTE_NAMES[t["route"]] == "f32_gemm" for t in T)
    for sw in (0, 1):
        assert any(t["sw"] == sw for t in T), sw
        for nt in (1, 2, 3, 4):
            assert any(t["sw"] == sw and t["nt"] == nt for t in T), (sw, nt)
    assert any(t["upw"] == 1 for t in T) and any(t["upw"] == 2 for t in T)
    assert any(t["nw"] == 2 for t in T) and any(t["nw"] == 8 for t in T) and any(2 < t["nw"] < 8 for t in T)
    assert any(t["nu"] % 2 for t in T) and any(t["n"] % 128 for t in T)
    assert any(t["grid"] == 1 for t in T) and any(t["grid"] == 16 for t in T)
    assert any(t["lds_bytes"] > 65536 for t in T)
