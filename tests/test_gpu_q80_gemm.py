"""Every batched Q80 launch plan (G6 gemm_q80_g6.hip, G7 / G7K gemm_q80_g7.hip, GC gemm_q80_cls.hip, G2 gemm_q80.hip) on the device.

The launches go through nb.op_fused_gemv(0x80, ..., use_gemm=True), i.e. the step's own router (route.hip), and nb.q80_gemm_plan reports
the plan the launchers consume.  Each case names the (kernel, template values) it is meant to reach at the smallest shape the CPU sweep
found for it; the closing coverage test checks that the cases here and GEMM_CASES of tests/test_gpu_fused_roles.py together reach every
tuple the sweep (tests/test_q80_gemm_plan.py UNIVERSE) finds reachable.  Values are checked first (a plan mismatch must not hide a wrong
result).

BARS, none of them new (inputs and helpers of tests/test_gpu_fused_roles.py: order-free activations, check_q80 / ref_q80).
  * The canonical kernels (G6, G7, G7K): the fast path == tests/canon.py bit for bit and within 1e-5 of max|ref| of the reference's
    order; strict mode of the same launch == the oracle bit for bit (check_q80).
  * GC and G2: both modes bit for bit the oracle's.
  * SwiGLU: the fused form under rtol = 3e-6, atol = 1e-9 (the device's expf against libm: test_k4_norm_swiglu_q80's bar); the store form
    of the same two matrices pins the projections bit for bit as above.
SECTION 3 (tests/test_q80_gemm_plan.py SECTION3): two launches whose G2 plan asks for more than a CU's LDS run through the GEMV kernels in
slices (route gemv_sliced), bit for bit the oracle's in both modes; the parent commit returned an error for both."""
import numpy as np
import pytest

from nano_amd import binding as nb
from test_q80_gemm_plan import UNIVERSE, ROUTE_OF, tuple_of, canonical
from test_gpu_fused_roles import GEMM_CASES, Q80, bits, check_q80, order_free, q80_weights, ref_q80, silu_mul


def case(gs, kind, n, rows, nb_, want, ordered=False):
    cid = "-".join(str(v) for v in want) + f"-gs{gs}-k{kind}-n{n}-r{sum(rows[:1] if kind == 2 else rows)}-t{nb_}" + ("-strict" if ordered else "")
    return pytest.param(dict(gs=gs, kind=kind, n=n, rows=tuple(rows), nb=nb_, ordered=ordered, want=tuple(want)), id=cid)


# (kernel, template values) -- G6 MODE S (NV, R, MS), MODE F (R, MS, TT), G7 (TP, PP, MS), GC (TT), G2 (GS, SW, TT) -- at the smallest
# shape (by weight bytes, then tokens) the CPU sweep meets it at: ragged last tiles and tensor ends inside a tile wherever the tuple allows
CASES = [
    # G2 at the group sizes and token tiles GEMM_CASES (group size 64, strict mode) does not reach
    case(32, 0, 64, (16,), 3, ("g2", 32, 0, 1)), case(32, 0, 64, (16,), 17, ("g2", 32, 0, 2)), case(32, 0, 64, (16,), 33, ("g2", 32, 0, 4)),
    case(32, 2, 64, (16, 16), 3, ("g2", 32, 1, 1)),
    case(64, 2, 192, (16, 16), 3, ("g2", 64, 1, 1)), case(64, 2, 192, (16, 16), 17, ("g2", 64, 1, 2)), case(64, 2, 192, (16, 16), 33, ("g2", 64, 1, 4)),
    case(128, 0, 384, (16,), 3, ("g2", 128, 0, 1)), case(128, 0, 384, (16,), 17, ("g2", 128, 0, 2)), case(128, 0, 384, (16,), 33, ("g2", 128, 0, 4)),
    case(128, 2, 384, (16, 16), 3, ("g2", 128, 1, 1)), case(128, 2, 384, (16, 16), 17, ("g2", 128, 1, 2)), case(128, 2, 384, (16, 16), 33, ("g2", 128, 1, 4)),
    case(256, 0, 768, (16,), 3, ("g2", 256, 0, 1)), case(256, 0, 768, (16,), 17, ("g2", 256, 0, 2)), case(256, 0, 768, (16,), 33, ("g2", 256, 0, 4)),
    case(256, 2, 768, (16, 16), 3, ("g2", 256, 1, 1)), case(256, 2, 768, (16, 16), 17, ("g2", 256, 1, 2)), case(256, 2, 768, (16, 16), 33, ("g2", 256, 1, 4)),
    # G6 MODE F: rounds x several tensors x token tiles
    case(64, 0, 256, (8,), 3, ("g6f", 1, 0, 1)), case(64, 2, 4096, (8, 8), 17, ("g6f", 1, 0, 2)),
    case(64, 0, 4096, (16, 16, 8), 17, ("g6f", 1, 1, 2)), case(64, 0, 2048, (16, 16, 8), 33, ("g6f", 1, 1, 4)),
    case(64, 0, 1280, (8,), 3, ("g6f", 2, 0, 1)), case(64, 2, 4352, (8, 8), 17, ("g6f", 2, 0, 2)), case(64, 0, 1280, (16, 16, 8), 3, ("g6f", 2, 1, 1)),
    case(64, 2, 9984, (8, 8), 3, ("g6f", 3, 0, 1)), case(64, 2, 9984, (8, 8), 17, ("g6f", 3, 0, 2)), case(64, 0, 9984, (16, 16, 8), 3, ("g6f", 3, 1, 1)),
    case(64, 0, 9984, (16, 16, 8), 17, ("g6f", 3, 1, 2)), case(64, 0, 9984, (16, 16, 8), 33, ("g6f", 3, 1, 4)),
    case(64, 2, 12800, (8, 8), 3, ("g6f", 4, 0, 1)), case(64, 2, 12800, (8, 8), 17, ("g6f", 4, 0, 2)), case(64, 0, 12800, (16, 16, 8), 3, ("g6f", 4, 1, 1)),
    case(64, 0, 12800, (16, 16, 8), 17, ("g6f", 4, 1, 2)),
    # G6 MODE S: eight waves at work, so at least eight (tile, unit) items per workgroup
    case(64, 0, 2048, (4100,), 3, ("g6s", 5, 1, 0)), case(64, 0, 2048, (4112, 16, 8), 3, ("g6s", 5, 1, 1)), case(64, 1, 256, (28700,), 3, ("g6s", 5, 2, 0)),
    case(64, 1, 768, (28700,), 3, ("g6s", 5, 4, 0)), case(64, 0, 768, (16400, 8192, 4100), 3, ("g6s", 5, 4, 1)),
    case(64, 2, 4096, (8, 8), 3, ("g6s", 8, 1, 0)), case(64, 0, 4096, (16, 16, 8), 3, ("g6s", 8, 1, 1)), case(64, 0, 2816, (4100,), 3, ("g6s", 8, 2, 0)),
    case(64, 0, 2816, (4112, 16, 8), 3, ("g6s", 8, 2, 1)),
    case(64, 0, 2816, (8200,), 3, ("g6s", 8, 4, 0)), case(64, 0, 2816, (4112, 1024, 1000), 3, ("g6s", 8, 4, 1)),
    # G7: three and six to eight row tiles per workgroup (8200 .. 20500 rows at 256 CUs), two token tiles per wave
    case(64, 0, 256, (8200,), 17, ("g7", 3, 1, 0)), case(64, 0, 256, (8208, 16, 8), 17, ("g7", 3, 1, 1)), case(64, 1, 256, (16392,), 33, ("g7", 5, 2, 0)),
    case(64, 1, 256, (20500,), 17, ("g7", 8, 1, 0)), case(64, 0, 256, (8208, 8192, 4100), 17, ("g7", 8, 1, 1)), case(64, 1, 256, (20500,), 33, ("g7", 8, 2, 0)), case(64, 0, 256, (8208, 8192, 4100), 33, ("g7", 8, 2, 1)),
    # GC at two token tiles
    case(64, 0, 256, (16392,), 17, ("gc", 2)),
]


def inputs(c):
    rng = np.random.default_rng(sum(c["rows"]) + c["n"] + c["nb"] + c["gs"])
    n, nb_, gs, kind = c["n"], c["nb"], c["gs"], c["kind"]
    x = order_free(rng, (nb_, n))
    nw = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32) if kind != 1 else None
    segs = [(*q80_weights(rng, r, n, gs), r) for r in c["rows"]]
    old = rng.standard_normal((nb_, sum(c["rows"]))).astype(np.float32) if kind == 1 else None
    return x, nw, segs, old


def check_ordered(oracle, c, x, nw, segs, old, kind, ordered, route, use_gemm=True):
    """one launch in the reference's order (GC, G2, the GEMV slices) against the oracle, bit for bit"""
    out, r = nb.op_fused_gemv(Q80, kind, c["n"], segs, x, nw, gs=c["gs"], nb=c["nb"], resid=old, use_gemm=use_gemm, ordered=ordered, want_route=True)
    for b in range(c["nb"]):
        ref = ref_q80(oracle, oracle.rmsnorm(x[b], nw) if nw is not None else x[b], segs, c["n"], c["gs"])
        if kind == 1:
            ref = (old[b] + ref).astype(np.float32)
        assert np.array_equal(bits(out[b]), bits(ref)), (ordered, r, b, float(np.abs(out[b] - ref).max()))
    assert r == route, (r, route)


def check_swiglu(oracle, c, x, nw, segs, ordered, canon, route, use_gemm=True):
    out, r = nb.op_fused_gemv(Q80, 2, c["n"], segs, x, nw, gs=c["gs"], nb=c["nb"], use_gemm=use_gemm, ordered=ordered, want_route=True)
    for b in range(c["nb"]):
        xn = oracle.rmsnorm(x[b], nw)
        want = silu_mul(ref_q80(oracle, xn, segs[:1], c["n"], c["gs"], canon=canon), ref_q80(oracle, xn, segs[1:], c["n"], c["gs"], canon=canon))
        assert np.allclose(out[b], want, rtol=3e-6, atol=1e-9), (ordered, r, b, float(np.abs(out[b] - want).max()))
    assert r == route, (r, route)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES)
def test_q80_gemm_plan_case(oracle, c):
    gs, kind, n, rows, nb_, ordered = c["gs"], c["kind"], c["n"], c["rows"], c["nb"], c["ordered"]
    p = nb.q80_gemm_plan(kind, n, rows, nb_, gs=gs, ordered=ordered, use_gemm=True)
    x, nw, segs, old = inputs(c)
    canon = canonical(gs, n, kind, rows, ordered)
    route = nb.ROUTE_NAMES[p["route"]]
    # 1. values; SwiGLU: the store form of the two matrices pins the projections, the fused form (the case's plan) the epilogue
    store = 0 if kind == 2 else kind
    if canon:
        # (strict mode of the same launch goes to G2 / GC; where those refuse it -- interior tensors that are no multiple of 16 rows --
        #  the strict launch has no batched route to ask for)
        strict = nb.q80_gemm_plan(store, n, rows, nb_, gs=gs, ordered=True, use_gemm=True)["kernel"] != 0
        check_q80(oracle, store, n, segs, x, nw, old, nb_, use_gemm=True, routes=None if kind == 2 else (route,), strict_too=strict)
    else:
        for o in (True, False) if not ordered else (True,):
            check_ordered(oracle, c, x, nw, segs, old, store, o, nb.ROUTE_NAMES[nb.q80_gemm_plan(store, n, rows, nb_, gs=gs, ordered=o, use_gemm=True)["route"]])
    if kind == 2:
        check_swiglu(oracle, c, x, nw, segs, ordered, canon, route)
    # 2. the plan, last
    assert p["kernel"] and tuple_of(p) == c["want"] and route == ROUTE_OF[c["want"][0]], \
        f"the launcher's plan is {tuple_of(p) if p['kernel'] else route}, the case means {c['want']}: a retune moved this case -- pick a new shape for this tuple"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,rows", [(2, 256, (64, 64)), (0, 8192, (32,))], ids=["swiglu-n256", "store-n8192"])
def test_section3_runs_in_gemv_slices(oracle, kind, n, rows):
    """group size 32 at 64 tokens: G2's product tables do not fit a CU's LDS -- 64 sequences through the GEMV kernels, 8 per launch"""
    c = dict(gs=32, kind=kind, n=n, rows=rows, nb=64)
    x, nw, segs, old = inputs(c)
    for ordered in (True, False):
        p = nb.q80_gemm_plan(kind, n, rows, 64, gs=32, ordered=ordered)
        assert p["kernel"] == 0 and nb.ROUTE_NAMES[p["route"]] == "gemv_sliced", p
        if kind != 2:
            check_ordered(oracle, c, x, nw, segs, old, kind, ordered, "gemv_sliced", use_gemm=False)
            continue
        out = check_swiglu(oracle, c, x, nw, segs, ordered, False, "gemv_sliced", use_gemm=False)
        # the epilogue's expf is the device's: every sequence of the batch bit for bit the same launch of that sequence alone, whose two
        # projections (the one-sequence store form, a GEMV launch as well) are the oracle's bit for bit
        for b in range(64):
            alone = nb.op_fused_gemv(Q80, 2, n, segs, x[b:b + 1], nw, gs=32, nb=1, ordered=ordered)
            assert np.array_equal(bits(out[b]), bits(alone[0])), (ordered, b)
            proj, r = nb.op_fused_gemv(Q80, 0, n, segs, x[b:b + 1], nw, gs=32, nb=1, ordered=ordered, want_route=True)
            assert r == "gemv" and np.array_equal(bits(proj[0]), bits(ref_q80(oracle, oracle.rmsnorm(x[b], nw), segs, n, 32))), (ordered, b)


def plans_run():
    """(kernel, template values) of the launches the cases here and GEMM_CASES issue, from the plans the query reports"""
    got = {}
    for prm in CASES:
        c = prm.values[0]
        p = nb.q80_gemm_plan(c["kind"], c["n"], c["rows"], c["nb"], gs=c["gs"], ordered=c["ordered"], use_gemm=True)
        got[tuple_of(p) if p["kernel"] else None] = prm.id
    for nb_, kind, n, rows in GEMM_CASES:
        tall = len(rows) == 1 and rows[0] >= 16384                   # (gemm_route_case: the tall matrices run the fast path only)
        for ordered in (False,) if tall else (False, True):
            p = nb.q80_gemm_plan(kind, n, rows, nb_, ordered=ordered, use_gemm=True)
            if p["kernel"]:
                got.setdefault(tuple_of(p), ("GEMM_CASES", nb_, kind, n, rows, ordered))
    return got


def test_cases_cover_every_reachable_plan():
    """CPU arithmetic only: the plans come from the query, which each case's own test also holds against the tuple the case states"""
    got = plans_run()
    for prm in CASES:
        c = prm.values[0]
        p = nb.q80_gemm_plan(c["kind"], c["n"], c["rows"], c["nb"], gs=c["gs"], ordered=c["ordered"], use_gemm=True)
        assert p["kernel"] and tuple_of(p) == c["want"], (prm.id, p)
    assert None not in got and set(got) <= UNIVERSE, sorted(set(got) - UNIVERSE)
    assert not UNIVERSE - set(got), ("a reachable (kernel, template tuple) without a GPU case", sorted(UNIVERSE - set(got)))
