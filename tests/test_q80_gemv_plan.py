"""CPU sweep of the Q80 GEMV launch plan (nano_hip_q80_gemv_plan: route_kind() + gemv_q80_plan() + route_q80_slices(), the functions the
router and the launchers themselves follow -- nano_amd/csrc/route.hip, gemv_q80.hip, gemv_q80_impl.h).  No GPU: the query is host
arithmetic on a shape.

For every descriptor of the grid one of three things holds.
  * The router sends it to a batched kernel (G6 / G7 / G2 / GC, which have their own files): the route, and zeros for the kernel fields.
  * The router refuses it (takes == 0, every other field 0) for one of the documented reasons
      - several weight tensors of a STORE / residual launch whose row counts are no multiples of 4 (a SLAB work unit is four rows
        of one tensor),
      - more than 4 work units per wave, which 16 waves reach beyond 64 units: a SLAB row of more than 65536 values (32768 with
        SwiGLU, whose units come in pairs),
      - one sequence alone asks for more LDS than a CU has (163840 bytes).
  * The launch is one gemv_q80_slab_kernel<ROLE, GS, B, NV, UPW, EARLY, WF, WFC> or gemv_q80_stream_kernel<ROLE, GS, B, NV> that exists,
    with a thread for every row of the fold, a wave slot for every work unit, a workgroup for every row and none across two weight
    tensors, the LDS layout the kernels address and a request a CU can meet -- the batch cut into as many launches as that takes.
The special forms appear exactly where gemv_q80_impl.h says: EARLY on matrices of >= 8 Mi weights at one or two sequences (group size
64, at least two units per wave, the activation in registers); WF on one-sequence rmsnorm-role launches of n == 1024; WFC2..4 on
one-sequence residual-role launches of one tensor with n == 2048 / 3072 / 4096 (role kernels: group size 64, canonical launches only).
The kernels behind the plans run in tests/test_gpu_q80_gemv.py, whose coverage test reads UNIVERSE below."""
import numpy as np
import pytest

from nano_amd import binding as nb

LDS_MAX = 163840            # bytes of LDS a gfx950 CU has
ROLE = {n: i for i, n in enumerate(nb.Q80_ROLES)}
VAR = {n: i for i, n in enumerate(nb.Q80_VARIANTS)}
SLAB, STREAM = nb.Q80_KERNELS.index("slab"), nb.Q80_KERNELS.index("stream")
GEMV_ROUTES = ("gemv", "gemv_preq", "gemv_sliced")

GSS = [32, 64, 128, 256]
NAMED_N = [64, 256, 768, 1024, 1408, 2048, 2304, 2560, 3072, 4096, 8192, 9728, 12288, 16384, 20480]
ROWS = [1, 3, 4, 7, 36, 333, 768, 2560, 9728, 16384, 16391, 151936]
ROWS4 = [r for r in ROWS if r % 4 == 0]
NBS = [1, 2, 3, 4, 5, 6, 7, 8, 11, 64]

SEEN = set()                # (kernel, B, NV, UPW, variant) of every launch the sweeps below met
DONE = set()                # ... the sweeps that ran


def capacity(nb_):
    return 1 if nb_ <= 1 else 2 if nb_ <= 2 else 4 if nb_ <= 4 else 8


def heads_of(n):
    hd = next(h for h in (128, 64, 48, 32, 16) if n % h == 0)
    return n // hd, hd, 4


def canonical(gs, n, kind, rows, ordered):
    """kernels.h q80_canonical()"""
    return not ordered and gs == 64 and n % 256 == 0 and not (kind == 0 and len(rows) == 1 and rows[0] >= 16384)


def slab_lds(gs, n, B, nmat, rw, heads, variant):
    """what gemv_q80_slab_body.inc lays out: [B][n16] int8 activations | [B][ng4] scales | [B][16] norm partials |
    [B][n_head][8] combine weights | the product table [B][nmat][4 tpw][pitch] (wf: none; wfcN: unit sums [4 tpw][4 | 8])"""
    ng = n // gs
    n16, ng4, tpw = (n + 15) & ~15, (ng + 3) & ~3, (rw + 3) // 4
    pitch = ((ng + 47) // 64) * 64 + 16 if gs == 64 else ng4 + 4
    if variant == VAR["wf"]:
        return n16 + ng4 * 4 + 64
    if variant in (VAR["wfc2"], VAR["wfc3"], VAR["wfc4"]):
        return n16 + ng4 * 4 + 64 + heads * 32 + tpw * 4 * (4 if variant == VAR["wfc2"] else 8) * 4
    return B * (n16 + ng4 * 4 + 64 + heads * 32) + B * nmat * tpw * 4 * pitch * 4


def check(gs, kind, n, rows, nb_, norm, attn, ordered=False):
    """one descriptor: a batched route, a documented refusal, or every invariant of a launch; returns the plan"""
    p = nb.q80_gemv_plan(kind, n, rows, nb_, gs=gs, norm=norm, attn=attn, ordered=ordered)
    ctx = (gs, kind, n, rows, nb_, norm, attn, ordered, p)
    nmat = 2 if kind == 2 else 1
    nchunk = (n + 1023) // 1024
    ng = n // gs
    total = rows[0] if kind == 2 else sum(rows)
    heads = attn[0] if attn else 0
    stream = kind == 0 and len(rows) == 1 and rows[0] >= 16384 and not attn            # use_stream(): every slice has <= 8 sequences
    ragged_segments = kind != 2 and len(rows) > 1 and any(r % 4 for r in rows)
    route = nb.ROUTE_NAMES[p["route"]]
    if p["takes"] and route not in GEMV_ROUTES:
        assert route in ("frag_g6", "frag_old", "frag_g7") and nb_ >= 2, ctx
        assert (p["launches"], p["seqs_per_launch"]) == (1, nb_), ctx
        assert not any(p[k] for k in nb.Q80_PLAN_FIELDS[1:13]), ctx
        return p
    # one sequence's LDS at the smallest plan (rw = 4) / of the stream kernel
    one = ((n + 15) & ~15) + ((ng + 3) & ~3) * 4 + 64 + 4 * 16 * (1024 // gs) * 4 if stream else slab_lds(gs, n, 1, nmat, 4, heads, 0)
    refused = ragged_segments or (not stream and nchunk * nmat > 64) or one > LDS_MAX
    if not p["takes"]:
        assert refused, ("refused without a documented reason", ctx)
        assert not any(p.values()), ctx
        return p
    assert not refused, ("taken against a documented limit", ctx)
    per, B, nv, upw, rw, nw, variant = p["seqs_per_launch"], p["B"], p["nv"], p["upw"], p["rw"], p["nw"], p["variant"]
    assert route == ("gemv_sliced" if nb_ > 8 else route) and (route != "gemv_preq" or (2 <= nb_ <= 8 and not attn)), ctx
    pre = route == "gemv_preq"
    assert p["pre"] == int(pre) and p["gs"] == gs, ctx
    # slices: every sequence in one, the last one not empty, a batch cut only where its capacity does not fit
    assert 1 <= per <= min(nb_, 8) and p["launches"] * per >= nb_ and (p["launches"] - 1) * per < nb_, ctx
    assert B == capacity(per) and B in (1, 2, 4, 8), ctx
    assert p["lds_bytes"] <= LDS_MAX, ctx
    SEEN.add((p["kernel"], B, nv, upw, variant))
    if stream:
        # 1024 persistent workgroups of four waves, a wave owns 16-row tiles; the norm role only for a plain normed launch
        assert (p["kernel"], p["grid"], nw, rw, upw, variant) == (STREAM, 1024, 4, 16, 0, 0), ctx
        assert p["role"] == ROLE["norm_store" if norm and not pre else "generic"], ctx
        nvr = (n + 1023) // 1024
        assert nv == (1 if nvr <= 1 else 2 if nvr <= 2 and B <= 4 else 4 if nvr <= 4 and B <= 2 else 0), ctx
        assert nv == 0 or nv * 256 * nw >= n, ctx
        # [B][n16] | [B][ng4] | [B][16] | the four waves' integer group sums [4][16][1024 / gs]
        assert p["lds_bytes"] == B * (((n + 15) & ~15) + ((ng + 3) & ~3) * 4 + 64) + 4 * 16 * (1024 // gs) * 4, ctx
        if min(nb_, 8) > per:
            assert capacity(min(nb_, 8)) * (p["lds_bytes"] // B) > LDS_MAX, ("a batch that fits was cut", ctx)
        return p
    assert p["kernel"] == SLAB, ctx
    # the template is one launch_slab_r instantiates: NV x UPW of {0, 1, 2, 4} x {1, 2, 4} with B * NV <= 8
    assert nv in (0, 1, 2, 4) and upw in (1, 2, 4) and B * nv <= 8, ctx
    # roles: one sequence only; group size 64: canonical launches only (the role kernels there carry the canonical fold alone)
    want_role = "generic"
    if B == 1 and not pre and (gs != 64 or canonical(gs, n, kind, rows, ordered)):
        want_role = {(0, True, False): "norm_store", (1, False, False): "resid", (1, False, True): "resid_combine",
                     (2, True, False): "norm_swiglu"}.get((kind, norm, attn is not None), "generic")
    assert p["role"] == ROLE[want_role], ctx
    units = ((rw + 3) // 4) * nchunk * nmat
    assert 4 <= rw <= 64 and 2 <= nw <= 16, ctx
    assert 64 * nw >= rw * B, ("a fold row without a thread", ctx)
    assert nw * upw >= units, ("a work unit without a wave slot", ctx)
    assert nv == 0 or nv * 256 * nw >= n, ("an activation float4 without a register", ctx)
    # the grid: every tensor's rows in workgroups of its own, at most the last one of a tensor ragged
    segs = rows[:1] if kind == 2 else rows
    assert p["grid"] == sum((r + rw - 1) // rw for r in segs), ctx
    assert p["grid"] * rw >= total and all(((r + rw - 1) // rw - 1) * rw < r for r in segs), ctx
    # the special forms, exactly where the launcher's comments put them
    big = total * n * nmat >= 8 << 20
    role_n = nb.Q80_ROLES[p["role"]]
    want_var = "plain"
    if gs == 64 and B <= 2 and upw >= 2 and nv >= 1 and big:
        want_var = "early"
    elif gs == 64 and B == 1 and role_n in ("norm_store", "norm_swiglu") and n == 1024 and nv in (1, 2):
        want_var = "wf"
    elif gs == 64 and B == 1 and role_n in ("resid", "resid_combine") and n in (2048, 3072, 4096) and len(rows) == 1 and nv in (1, 2) and upw <= 2 \
            and not (upw >= 2 and big):
        want_var = "wfc%d" % (n // 1024)
    assert variant == VAR[want_var], (want_var, ctx)
    assert p["lds_bytes"] == slab_lds(gs, n, B, nmat, rw, heads, variant), ctx
    if min(nb_, 8) > per:
        # capacities 4 and 8 take the same or fewer rows per workgroup the larger they are (the planner shrinks rw to bound the table),
        # and never more than 64: the whole batch at these rows is the most its own plan could have asked for
        whole = slab_lds(gs, n, capacity(min(nb_, 8)), nmat, rw if B >= 4 else 64, heads, 0)
        assert whole > LDS_MAX, ("a batch that fits was cut", ctx)
    return p


def segment_sets(i):
    """one, two and three weight tensors of a STORE / residual launch; the several-tensor ones in multiples of 4, every fourth ragged"""
    r = ROWS[i % len(ROWS)]
    a, b, c = (ROWS4[(i + k) % len(ROWS4)] for k in range(3))
    return [(r,), (a, b + (3 if i % 4 == 3 else 0)), (a, b, c)]


def test_named_shapes_full_cross():
    seen = 0
    for gs in GSS:
        for n in (n for n in NAMED_N if n % gs == 0):
            for i, r in enumerate(ROWS):
                for nb_ in NBS:
                    ordered = bool((i + nb_) & 1)
                    for norm in (False, True):
                        for segs in segment_sets(i):
                            check(gs, 0, n, segs, nb_, norm, None, ordered); seen += 1
                        check(gs, 2, n, (r, r), nb_, norm, None, not ordered); seen += 1
                    for segs in segment_sets(i):
                        check(gs, 1, n, segs, nb_, False, None, ordered); seen += 1
                        if nb_ <= 8:
                            check(gs, 1, n, segs, nb_, False, heads_of(n), not ordered); seen += 1
    assert seen > 80000
    DONE.add("named")


def test_every_row_length():
    """every multiple of 16 and of the group size up to 20480, the other axes rotating"""
    takes = 0
    for gs in GSS:
        for j, n in enumerate(range(gs, 20481, gs)):
            if n % 16:
                continue
            r = ROWS[j % len(ROWS)]
            for nb_ in NBS:
                kind = (j + nb_) % 3
                ordered = bool((j // 3 + nb_) & 1)
                if kind == 0:
                    p = check(gs, 0, n, segment_sets(j + nb_)[(j // 3) % 3], nb_, bool(j & 1), None, ordered)
                elif kind == 1:
                    p = check(gs, 1, n, (r,), nb_, False, heads_of(n) if (j & 1 and nb_ <= 8) else None, ordered)
                else:
                    p = check(gs, 2, n, (r, r), nb_, bool(j & 2), None, ordered)
                takes += p["takes"]
    assert takes > 10000
    DONE.add("lengths")


# What the two sweeps above reach of the template space, as (kernel, B, NV, UPW, variant); tests/test_gpu_q80_gemv.py runs a case for every
# (kernel, B, NV, UPW) and every variant here.  Instantiated and reached by no descriptor: the slab kernel's loop form (NV = 0)
# on one unit per wave at one and two sequences, and most of the special forms' (NV, UPW) pairs.
def K(kernel, B, nv, upw, variant="plain"):
    return (kernel, B, nv, upw, VAR[variant])


UNIVERSE = {
    K(SLAB, 1, 0, 2), K(SLAB, 1, 0, 4), K(SLAB, 1, 1, 1), K(SLAB, 1, 1, 1, "wf"), K(SLAB, 1, 1, 1, "wfc2"), K(SLAB, 1, 1, 2),
    K(SLAB, 1, 1, 2, "early"), K(SLAB, 1, 1, 4), K(SLAB, 1, 1, 4, "early"), K(SLAB, 1, 2, 1), K(SLAB, 1, 2, 1, "wf"),
    K(SLAB, 1, 2, 1, "wfc2"), K(SLAB, 1, 2, 1, "wfc3"), K(SLAB, 1, 2, 1, "wfc4"), K(SLAB, 1, 2, 2), K(SLAB, 1, 2, 2, "early"),
    K(SLAB, 1, 2, 4), K(SLAB, 1, 2, 4, "early"), K(SLAB, 1, 4, 1), K(SLAB, 1, 4, 2), K(SLAB, 1, 4, 2, "early"), K(SLAB, 1, 4, 4),
    K(SLAB, 1, 4, 4, "early"),
    K(SLAB, 2, 0, 2), K(SLAB, 2, 0, 4), K(SLAB, 2, 1, 1), K(SLAB, 2, 1, 2), K(SLAB, 2, 1, 2, "early"), K(SLAB, 2, 1, 4),
    K(SLAB, 2, 1, 4, "early"), K(SLAB, 2, 2, 1), K(SLAB, 2, 2, 2), K(SLAB, 2, 2, 2, "early"), K(SLAB, 2, 2, 4), K(SLAB, 2, 2, 4, "early"),
    K(SLAB, 2, 4, 1), K(SLAB, 2, 4, 2), K(SLAB, 2, 4, 2, "early"), K(SLAB, 2, 4, 4), K(SLAB, 2, 4, 4, "early"),
    K(SLAB, 4, 0, 1), K(SLAB, 4, 0, 2), K(SLAB, 4, 0, 4), K(SLAB, 4, 1, 1), K(SLAB, 4, 1, 2), K(SLAB, 4, 1, 4), K(SLAB, 4, 2, 1),
    K(SLAB, 4, 2, 2), K(SLAB, 4, 2, 4),
    K(SLAB, 8, 0, 1), K(SLAB, 8, 0, 2), K(SLAB, 8, 0, 4), K(SLAB, 8, 1, 1), K(SLAB, 8, 1, 2), K(SLAB, 8, 1, 4),
    K(STREAM, 1, 0, 0), K(STREAM, 1, 1, 0), K(STREAM, 1, 2, 0), K(STREAM, 1, 4, 0),
    K(STREAM, 2, 0, 0), K(STREAM, 2, 1, 0), K(STREAM, 2, 2, 0), K(STREAM, 2, 4, 0),
    K(STREAM, 4, 0, 0), K(STREAM, 4, 1, 0), K(STREAM, 4, 2, 0),
    K(STREAM, 8, 0, 0), K(STREAM, 8, 1, 0),
}


def test_universe_is_what_the_sweeps_reach():
    if "named" not in DONE:
        test_named_shapes_full_cross()
    if "lengths" not in DONE:
        test_every_row_length()
    print(sorted(SEEN))
    assert SEEN == UNIVERSE, (sorted(SEEN - UNIVERSE), sorted(UNIVERSE - SEEN))


def test_documented_refusals():
    P = nb.q80_gemv_plan
    # 64 | 65 chunks of 1 KiB: upw 4 | 5 on 16 waves (SwiGLU: 32 | 33 chunks of both matrices)
    assert P(1, 65536, (16,))["takes"] == 1 and check(64, 1, 66560, (16,), 1, False, None)["takes"] == 0
    assert P(2, 32768, (16, 16))["takes"] == 1 and check(64, 2, 33792, (16, 16), 1, False, None)["takes"] == 0
    assert P(0, 256, (8, 4))["takes"] == 1 and P(0, 256, (8, 3))["takes"] == 0 and P(0, 256, (3,))["takes"] == 1
    # one sequence that does not fit: the combine weights of 16384 heads
    assert P(1, 65536, (16,), attn=(2048, 32, 4))["takes"] == 1
    assert check(64, 1, 65536, (16,), 1, False, (16384, 4, 4))["takes"] == 0
    # a malformed descriptor is an error, not a plan
    for bad in (dict(kind=3, n=256, rows=(4,)), dict(kind=0, n=264, rows=(4,)), dict(kind=0, n=256, rows=(4,), gs=48), dict(kind=0, n=288, rows=(4,), gs=32 * 3),
                dict(kind=2, n=256, rows=(4, 8)), dict(kind=0, n=256, rows=(4,), nb=65), dict(kind=0, n=256, rows=(4,), attn=(2, 128, 4)),
                dict(kind=1, n=256, rows=(4,), nb=9, attn=(2, 128, 4))):
        with pytest.raises(nb.NanoHipError):
            P(**bad)


def test_long_rows_fit_in_slices():
    """The launches that asked for more LDS than a CU has before the router knew the limit: 5..8 sequences on rows of 9728 values with
    SwiGLU at group size 32 (166912 bytes at capacity 8), on rows of 16384 at group sizes 32 and 64 (174592 bytes at 64) and with SwiGLU at
    128, on rows of 20480 everywhere -- now run in slices of 4 (of 2: SwiGLU on 20480 values at group size 32); no launch of the grid
    asks for more than 163840 bytes (check() asserts it for every descriptor)."""
    for nb_, launches, per in ((4, 1, 4), (5, 2, 4), (7, 2, 4), (8, 2, 4), (11, 3, 4), (64, 16, 4)):
        p = check(32, 2, 9728, (4, 4), nb_, True, None)
        assert (p["launches"], p["seqs_per_launch"], p["B"]) == (launches, per, 4), (nb_, p)
    assert slab_lds(32, 9728, 8, 2, 4, 0, 0) == 166912
    assert slab_lds(64, 16384, 8, 1, 4, 0, 0) == 174592
    for gs in GSS:
        for kind, rows in ((0, (4,)), (1, (4,)), (2, (4, 4))):
            p = check(gs, kind, 16384, rows, 8, kind != 1, None)
            cut = gs <= 64 or (gs == 128 and kind == 2)          # group size 256: 142336 bytes (SwiGLU 151040) at capacity 8 -- they fit
            assert (p["launches"], p["seqs_per_launch"], p["B"]) == ((2, 4, 4) if cut else (1, 8, 8)), (gs, kind, p)
            assert (slab_lds(gs, 16384, 8, len(rows), 4, 0, 0) > LDS_MAX) == cut and p["lds_bytes"] <= LDS_MAX
            p = check(gs, kind, 20480, rows, 8, kind != 1, None)
            assert (p["launches"], p["seqs_per_launch"]) == ((4, 2) if (gs, kind) == (32, 2) else (2, 4)), (gs, kind, p)
    # where 8 fit, a batch beyond 8 runs in the groups of 8 it always has
    p = check(32, 0, 192, (36, 4, 12), 64, True, None)
    assert (nb.ROUTE_NAMES[p["route"]], p["B"], p["launches"], p["seqs_per_launch"]) == ("gemv_sliced", 8, 8, 8), p
    p = check(32, 0, 192, (36, 4, 12), 11, True, None)
    assert (p["B"], p["launches"], p["seqs_per_launch"]) == (8, 2, 8), p


# (rw, nw, UPW, NV) at capacities 1, 2, 4, 8 of the per-layer and classifier launches of Qwen3-0.6B, Qwen3-4B and the tiny presets -- keyed
# (group size, kind, n, rows) --, copied from the planner before the plan became a function of its own: the launches of models that ran
# before must not move.  "stream": the classifier's kernel, which has no such choices.
MODEL_PLANS = {
    # Qwen3-0.6B, group size 64
    (64, 0, 1024, (2048, 1024, 1024)): [(16, 4, 1, 1), (16, 4, 1, 1), (16, 4, 1, 1), (16, 8, 1, 1)],
    (64, 1, 2048, (1024,)): [(8, 6, 1, 2), (8, 4, 1, 2), (8, 8, 1, 1), (8, 16, 1, 1)],
    (64, 2, 1024, (3072, 3072)): [(12, 4, 2, 1), (16, 4, 2, 1), (16, 4, 2, 1), (16, 8, 1, 1)],
    (64, 1, 3072, (1024,)): [(4, 8, 1, 2), (4, 6, 1, 2), (4, 12, 1, 1), (4, 16, 1, 1)],
    (64, 0, 1024, (151936,)): ["stream", "stream", "stream", "stream"],
    # Qwen3-4B, group size 64
    (64, 0, 2560, (4096, 1024, 1024)): [(25, 10, 4, 1), (25, 10, 4, 1), (16, 10, 2, 1), (16, 16, 1, 1)],
    (64, 1, 4096, (2560,)): [(10, 8, 2, 2), (10, 8, 2, 2), (8, 16, 1, 1), (8, 16, 1, 1)],
    (64, 2, 2560, (9728, 9728)): [(38, 16, 4, 1), (38, 16, 4, 1), (16, 10, 4, 1), (8, 16, 1, 1)],
    (64, 1, 9728, (2560,)): [(10, 15, 2, 4), (10, 15, 2, 4), (8, 16, 2, 0), (8, 16, 2, 0)],
    (64, 0, 2560, (151936,)): ["stream", "stream", "stream", "stream"],
    # tiny-qwen3, group size 32
    (32, 0, 256, (256, 128, 128)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (32, 1, 256, (256,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (32, 2, 256, (768, 768)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (32, 1, 768, (256,)): [(4, 2, 1, 2), (4, 2, 1, 2), (4, 3, 1, 1), (4, 6, 1, 1)],
    (32, 0, 256, (1024,)): [(8, 2, 1, 1), (8, 2, 1, 1), (8, 2, 1, 1), (8, 2, 1, 1)],
    # tiny-nano, group size 32
    (32, 0, 128, (128, 64, 64)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (32, 1, 128, (128,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (32, 2, 128, (384, 384)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (32, 1, 384, (128,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 3, 1, 1)],
    (32, 0, 128, (512,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    # tiny-qwen3, group size 64
    (64, 0, 256, (256, 128, 128)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (64, 1, 256, (256,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (64, 2, 256, (768, 768)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (64, 1, 768, (256,)): [(4, 2, 1, 2), (4, 2, 1, 2), (4, 3, 1, 1), (4, 6, 1, 1)],
    (64, 0, 256, (1024,)): [(8, 2, 1, 1), (8, 2, 1, 1), (8, 2, 1, 1), (8, 2, 1, 1)],
    # tiny-nano, group size 64
    (64, 0, 128, (128, 64, 64)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (64, 1, 128, (128,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (64, 2, 128, (384, 384)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (64, 1, 384, (128,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 3, 1, 1)],
    (64, 0, 128, (512,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    # tiny-qwen3, group size 128
    (128, 0, 256, (256, 128, 128)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (128, 1, 256, (256,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (128, 2, 256, (768, 768)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (128, 1, 768, (256,)): [(4, 2, 1, 2), (4, 2, 1, 2), (4, 3, 1, 1), (4, 6, 1, 1)],
    (128, 0, 256, (1024,)): [(8, 2, 1, 1), (8, 2, 1, 1), (8, 2, 1, 1), (8, 2, 1, 1)],
    # tiny-nano, group size 128
    (128, 0, 128, (128, 64, 64)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (128, 1, 128, (128,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (128, 2, 128, (384, 384)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (128, 1, 384, (128,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 3, 1, 1)],
    (128, 0, 128, (512,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    # tiny-nano-odd, group size 32
    (32, 0, 192, (192, 96, 96)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (32, 1, 192, (192,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (32, 2, 192, (352, 352)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
    (32, 1, 352, (192,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 3, 1, 1)],
    (32, 0, 192, (512,)): [(4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1), (4, 2, 1, 1)],
}


@pytest.mark.parametrize("shape", list(MODEL_PLANS), ids=lambda s: f"gs{s[0]}-k{s[1]}-{s[2]}x{sum(s[3][:1] if s[1] == 2 else s[3])}")
def test_model_plans_unchanged(shape):
    gs, kind, n, rows = shape
    for nb_, want in zip((1, 2, 4, 8), MODEL_PLANS[shape]):
        # strict mode too: the planner does not look at the fold's order (the router does: wide matrices leave the GEMV at other sizes)
        for ordered in (False, True):
            p = check(gs, kind, n, rows, nb_, kind != 1, None, ordered)
            if nb.ROUTE_NAMES[p["route"]] not in GEMV_ROUTES:
                assert nb_ >= 2, (shape, nb_, p)
                continue
            assert p["launches"] == 1, (shape, nb_, p)
            if want == "stream":
                assert p["kernel"] == STREAM, (shape, nb_, p)
            else:
                assert (p["kernel"], p["rw"], p["nw"], p["upw"], p["nv"]) == (SLAB,) + want, (shape, nb_, ordered, p)
        if kind == 1 and nb_ == 1:                           # Wo behind split attention
            q = check(gs, kind, n, rows, 1, False, heads_of(n))
            assert q["role"] == ROLE["resid_combine" if gs != 64 or n % 256 == 0 else "generic"] and (q["rw"], q["nw"], q["upw"], q["nv"]) == want


def test_model_plans_reach_the_special_forms():
    """the forms the models' one-sequence steps run: Qwen3-0.6B wf (q|k|v, W1|W3), wfc2 (Wo), wfc3 (W2); Qwen3-4B early everywhere but
    Wo (wfc4: 10 M weights, but on two units per wave... of which the first is early)"""
    V = lambda *a, **k: nb.Q80_VARIANTS[check(64, *a, **k)["variant"]]
    assert V(0, 1024, (2048, 1024, 1024), 1, True, None) == "wf" and V(2, 1024, (3072, 3072), 1, True, None) == "wf"
    assert V(1, 2048, (1024,), 1, False, None) == "wfc2" and V(1, 3072, (1024,), 1, False, None) == "wfc3"
    assert V(0, 2560, (4096, 1024, 1024), 1, True, None) == "early" and V(2, 2560, (9728, 9728), 2, True, None) == "early"
    assert V(1, 9728, (2560,), 1, False, None) == "early" and V(1, 4096, (2560,), 1, False, None) == "early"
    # strict mode keeps the generic kernel and the product table on the small matrices
    assert V(0, 1024, (2048, 1024, 1024), 1, True, None, ordered=True) == "plain"


def test_query_needs_no_device_and_follows_no_pointer():
    """shape fields only: the descriptor of the binding's query holds no weight, activation or output pointer at all"""
    p = nb.q80_gemv_plan(0, 1024, (2048, 1024, 1024), 1, norm=True)
    assert p == dict(route=0, kernel=SLAB, role=ROLE["norm_store"], gs=64, B=1, nv=1, upw=1, rw=16, nw=4, grid=256, lds_bytes=1152, variant=VAR["wf"], pre=0,
                     launches=1, seqs_per_launch=1, takes=1)
    assert np.all([nb.q80_gemv_plan(0, 1024, (2048, 1024, 1024), 1, norm=True, cus=c) == p for c in (0, 256)])

