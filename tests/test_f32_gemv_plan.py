"""CPU sweep of the FP32 GEMV launch plan (nano_hip_f32_gemv_plan: gemv_f32_plan() + route_f32_slices(), the functions the launcher
and the router themselves follow -- nano_amd/csrc/gemv_f32.hip, route.hip).  No GPU: the query is host arithmetic on a shape.

For every descriptor of the grid either the router refuses the shape (takes == 0) for one of the documented reasons
  * more than 4 work units per wave, which 16 waves reach beyond 64 units: a row of more than 16384 floats (8192 with SwiGLU, whose
    units come in pairs),
  * one sequence alone asks for more LDS than a CU has (163840 bytes),
  * several weight tensors whose row counts are no multiples of 4,
or the launch is one gemv_f32_slab_kernel<ROLE, B, NV, UPW> that exists, with a thread for every row of the fold, a wave slot for every
work unit, a workgroup for every row, and an LDS request a CU can meet -- the batch cut into as many launches as that takes.
The kernels behind the plans run in tests/test_gpu_f32_gemv.py."""
import numpy as np
import pytest

from nano_amd import binding as nb

LDS_MAX = 163840            # bytes of LDS a gfx950 CU has
ROLE = {n: i for i, n in enumerate(nb.F32_ROLES)}

NAMED_N = [192, 352, 768, 1408, 2048, 2560, 3072, 4096, 9728, 12288, 16384, 16388]
ROWS = [1, 3, 4, 36, 333, 768, 16384, 151936]
ROWS4 = [r for r in ROWS if r % 4 == 0]
NBS = [1, 2, 3, 4, 5, 6, 7, 8, 11, 64]


def capacity(nb_):
    return 1 if nb_ <= 1 else 2 if nb_ <= 2 else 4 if nb_ <= 4 else 8


def heads_of(n):
    hd = next(h for h in (128, 64, 48, 32, 4) if n % h == 0)
    return n // hd, hd, 4


def check(kind, n, rows, nb_, norm, attn):
    """one descriptor: a documented refusal, or every invariant of a launch; returns the plan"""
    p = nb.f32_gemv_plan(kind, n, rows, nb_, norm=norm, attn=attn)
    ctx = (kind, n, rows, nb_, norm, attn, p)
    nmat = 2 if kind == 2 else 1
    nchunk = (n + 255) // 256
    total = rows[0] if kind == 2 else sum(rows)
    ragged_segments = kind != 2 and len(rows) > 1 and any(r % 4 for r in rows)
    # one sequence's LDS at the smallest plan (rw = 4): activations, norm partials, combine weights, chunk partials
    one = (n + 16 + (attn[0] * 8 if attn else 0) + nmat * 4 * ((nchunk + 3) & ~3)) * 4
    refused = nchunk * nmat > 64 or ragged_segments or one > LDS_MAX
    if not p["takes"]:
        assert refused, ("refused without a documented reason", ctx)
        assert not any(p.values()), ctx
        return p
    assert not refused, ("taken against a documented limit", ctx)
    B, nv, upw, rw, nw = p["B"], p["nv"], p["upw"], p["rw"], p["nw"]
    # the template is one launch_f32_r instantiates: NV x UPW of {0, 1, 2, 4} x {1, 2, 4} with B * NV <= 8, roles only for one sequence
    assert B == capacity(p["seqs_per_launch"]) and B in (1, 2, 4, 8), ctx
    assert nv in (0, 1, 2, 4) and upw in (1, 2, 4) and B * nv <= 8, ctx
    want_role = "generic"
    if B == 1:
        want_role = {(0, True, False): "norm_store", (1, False, False): "resid", (1, False, True): "resid_combine",
                     (2, True, False): "norm_swiglu"}.get((kind, norm, attn is not None), "generic")
    assert p["role"] == ROLE[want_role], ctx
    assert rw in (4, 8, 16, 32), ctx
    units = (rw // 4) * nchunk * nmat
    assert 2 <= nw and 64 * nw <= 1024, ctx
    assert 64 * nw >= rw * B, ("a fold row without a thread", ctx)
    assert nw * upw >= units, ("a work unit without a wave slot", ctx)
    assert nv == 0 or nv * 256 * nw >= n, ("an activation float4 without a register", ctx)
    assert p["grid"] * rw >= total and (p["grid"] - 1) * rw < total, ctx
    assert p["lds_bytes"] <= LDS_MAX, ctx
    # what the kernel lays out: [B][n] activations | [B][16] norm partials | [B][n_head][8] combine weights | [B][nmat][rw][nchunk, padded to 4]
    assert p["lds_bytes"] == B * (n + 16 + (attn[0] * 8 if attn else 0) + nmat * rw * ((nchunk + 3) & ~3)) * 4, ctx
    assert 1 <= p["seqs_per_launch"] <= min(nb_, 8) and p["launches"] * p["seqs_per_launch"] >= nb_, ctx
    assert (p["launches"] - 1) * p["seqs_per_launch"] < nb_, ctx
    if nb_ <= 8 and p["launches"] > 1:                       # cut only where the whole batch does not fit
        whole = capacity(nb_) * (p["lds_bytes"] // B)
        assert whole > LDS_MAX, ("a batch that fits was cut", ctx)
    if kind != 2 and len(rows) > 1:
        assert all(r % rw == 0 for r in rows), ("a workgroup across two weight tensors", ctx)
    return p


def segment_sets(i):
    """one, two and three weight tensors of a STORE / residual launch, the several-tensor ones in multiples of 4"""
    r = ROWS[i % len(ROWS)]
    a, b, c = (ROWS4[(i + k) % len(ROWS4)] for k in range(3))
    return [(r,), (a, b), (a, b, c)]


def test_named_shapes_full_cross():
    seen = 0
    for n in NAMED_N + [4, 64, 256, 8192, 8196, 20480]:
        for i, r in enumerate(ROWS):
            for nb_ in NBS:
                for norm in (False, True):
                    for segs in segment_sets(i):
                        check(0, n, segs, nb_, norm, None); seen += 1
                    check(2, n, (r, r), nb_, norm, None); seen += 1
                for segs in segment_sets(i):
                    check(1, n, segs, nb_, False, None); seen += 1
                    if nb_ <= 8:
                        check(1, n, segs, nb_, False, heads_of(n)); seen += 1
    assert seen > 15000


def test_every_row_length():
    """every multiple of 4 up to 20480, the other axes rotating"""
    takes = 0
    for j, n in enumerate(range(4, 20481, 4)):
        r = ROWS[j % len(ROWS)]
        for nb_ in NBS:
            kind = (j + nb_) % 3
            if kind == 0:
                p = check(0, n, segment_sets(j + nb_)[(j // 3) % 3], nb_, bool(j & 1), None)
            elif kind == 1:
                p = check(1, n, (r,), nb_, False, heads_of(n) if (j & 1 and nb_ <= 8) else None)
            else:
                p = check(2, n, (r, r), nb_, bool(j & 2), None)
            takes += p["takes"]
    assert takes > 30000


def test_documented_refusals():
    P = nb.f32_gemv_plan
    assert P(1, 16384, (16,))["takes"] == 1 and P(1, 16388, (16,))["takes"] == 0          # 64 | 65 units: upw 4 | 5 on 16 waves
    assert P(2, 8192, (16, 16))["takes"] == 1 and P(2, 8196, (16, 16))["takes"] == 0
    assert P(0, 20480, (768,), 3, norm=True)["takes"] == 0
    assert P(0, 256, (8, 4))["takes"] == 1 and P(0, 256, (8, 3))["takes"] == 0 and P(0, 256, (3,))["takes"] == 1
    # one sequence that does not fit: 16384 floats + the combine weights of 4096 heads
    assert P(1, 16384, (16,), attn=(2048, 8, 4))["takes"] == 1
    assert check(1, 16384, (16,), 1, False, (4096, 4, 4))["takes"] == 0
    # a malformed descriptor is an error, not a plan
    for bad in (dict(kind=3, n=256, rows=(4,)), dict(kind=0, n=258, rows=(4,)), dict(kind=2, n=256, rows=(4, 8)), dict(kind=0, n=256, rows=(4,), nb=65),
                dict(kind=0, n=256, rows=(4,), attn=(2, 128, 4)), dict(kind=1, n=256, rows=(4,), nb=9, attn=(2, 128, 4))):
        with pytest.raises(nb.NanoHipError):
            P(**bad)


def test_qwen3_4b_w2_fits_in_slices():
    """Qwen3-4B's W2 (n = 9728, 2560 rows): 8 sequences in one launch would ask for 316928 bytes of LDS, 4 for 158464 -- the router
    issues two launches of 4.  n = 12288: 4 sequences would ask for 199936."""
    p = check(1, 9728, (2560,), 8, False, None)
    assert (p["takes"], p["B"], p["nv"], p["upw"], p["nw"], p["lds_bytes"], p["launches"], p["seqs_per_launch"]) == (1, 4, 0, 4, 16, 158464, 2, 4)
    for nb_, launches, per in ((3, 1, 3), (4, 1, 4), (5, 2, 4), (7, 2, 4), (11, 3, 4), (64, 16, 4)):
        p = check(1, 9728, (2560,), nb_, False, None)
        assert (p["launches"], p["seqs_per_launch"], p["lds_bytes"]) == (launches, per, 158464), (nb_, p)
    p = check(1, 12288, (512,), 4, False, None)
    assert (p["B"], p["launches"], p["seqs_per_launch"], p["lds_bytes"]) == (2, 2, 2, 99968)
    # where 8 fit, a batch beyond 8 runs in the groups of 8 it always has
    p = check(0, 768, (768, 384, 384), 64, True, None)
    assert (p["B"], p["launches"], p["seqs_per_launch"]) == (8, 8, 8)
    p = check(0, 768, (768, 384, 384), 11, True, None)
    assert (p["B"], p["launches"], p["seqs_per_launch"]) == (8, 2, 8)


# (rw, nw, UPW, NV) at capacities 1, 2, 4, 8 of the per-layer and classifier launches of Nano-168M and Nano-56M, copied from the
# planner before the plan became a function of its own: the launches of models that ran before must not move
NANO_PLANS = {
    (0, 768, (768, 384, 384)): [(4, 3, 1, 1)] * 4,
    (1, 768, (768,)): [(4, 3, 1, 1)] * 4,
    (2, 768, (2048, 2048)): [(8, 8, 2, 1)] * 4,
    (1, 2048, (768,)): [(4, 8, 1, 1)] * 4,
    (0, 768, (16384,)): [(8, 6, 1, 1)] * 4,
    (0, 512, (512, 256, 256)): [(4, 2, 1, 1)] * 4,
    (1, 512, (512,)): [(4, 2, 1, 1)] * 4,
    (2, 512, (1408, 1408)): [(4, 4, 1, 1)] * 4,
    (1, 1408, (512,)): [(4, 6, 1, 1)] * 4,
    (0, 512, (16384,)): [(16, 8, 1, 1)] * 4,
}


@pytest.mark.parametrize("shape", list(NANO_PLANS), ids=lambda s: f"k{s[0]}-{s[1]}x{sum(s[2])}")
def test_nano_model_plans_unchanged(shape):
    kind, n, rows = shape
    for nb_, want in zip((1, 2, 4, 8), NANO_PLANS[shape]):
        p = check(kind, n, rows, nb_, kind != 1, None)
        assert (p["rw"], p["nw"], p["upw"], p["nv"]) == want and p["launches"] == 1, (shape, nb_, p)
        if kind == 1 and nb_ == 1:                           # Wo behind split attention
            q = check(kind, n, rows, 1, False, heads_of(n))
            assert q["role"] == ROLE["resid_combine"] and (q["rw"], q["nw"], q["upw"], q["nv"]) == want


def test_query_needs_no_device_and_follows_no_pointer():
    """shape fields only: the descriptor of the binding's query holds no weight, activation or output pointer at all"""
    p = nb.f32_gemv_plan(0, 768, (768, 384, 384), 1, norm=True)
    assert p == dict(role=ROLE["norm_store"], B=1, nv=1, upw=1, rw=4, nw=3, grid=384, lds_bytes=3200, launches=1, seqs_per_launch=1, takes=1)
    assert np.all([nb.f32_gemv_plan(0, 768, (768, 384, 384), 1, norm=True, cus=c) == p for c in (0, 1, 304)])
