"""CPU sweep of the Q4K GEMV launch plan (nano_hip_q4k_gemv_plan: route_kind() + gemv_q4k_plan() + route_gemv_slices(), the functions the
router and the launchers themselves follow -- nano_amd/csrc/route.hip, gemv_q4k.hip, gemv_q4k_chunk.hip).  No GPU: the query is host
arithmetic on a shape.

For every descriptor of the grid one of three things holds.
  * The router sends it to the int8 MFMA GEMM (gemm_q4k.hip: 9..64 tokens of whole 256-value blocks): the route, and zeros for the
    kernel fields.
  * The router refuses it (takes == 0, every other field 0) for one of the documented reasons, all of them the item kernel's (the chunk
    kernel takes the whole-block shapes its search finds a slab for; 2..4 sequences of such a shape that stay on the item kernel meet its
    limits)
      - several weight tensors of a STORE / residual launch whose row counts are no multiples of 4 (a workgroup's rows lie in one tensor),
      - more than 4 (row, group) items per thread at the smallest workgroup (4 rows),
      - one sequence alone asks for more LDS than a CU has (163840 bytes).
  * The launch is one gemv_q4k_slab_kernel<ROLE, B, NV, IPT> or gemv_q4k_chunk_kernel<ROLE, NV, D, LOOP, NB> that exists, with a thread
    for every row of the fold, a slot for every item / wave-load, a workgroup for every row and none across two weight tensors, the LDS
    layout the kernels address and a request a CU can meet -- the batch cut into as many launches as that takes.
Which kernel: the chunk kernel takes whole-block rows (n % 256 == 0, n <= 16384) of one sequence; of 2..8 sequences (behind its quantizer
launch) from 5 sequences on, on matrices of >= 8 Mi weights, and where the item kernel cannot hold the sequences; the item kernel the rest."""
import numpy as np
import pytest

from nano_amd import binding as nb

LDS_MAX = 163840            # bytes of LDS a gfx950 CU has
ROLE = {n: i for i, n in enumerate(nb.Q80_ROLES)}
SLAB, CHUNK = nb.Q4K_KERNELS.index("slab"), nb.Q4K_KERNELS.index("chunk")
KERNEL_FIELDS = nb.Q4K_PLAN_FIELDS[1:21]

# whole-block and partial-block row lengths
NAMED_N = [64, 192, 256, 352, 768, 1024, 1408, 2048, 2304, 2560, 3072, 4096, 4100, 8192, 9728, 9732, 12288, 16384, 16388, 20480]
ROWS = [1, 3, 4, 7, 36, 333, 768, 2560, 9728, 16384, 16391, 151936]          # the row lists of tests/test_q80_gemv_plan.py
ROWS4 = [r for r in ROWS if r % 4 == 0]
NBS = [1, 2, 3, 4, 5, 6, 7, 8, 11, 64]

SEEN = set()                # plan_tuple() of every GEMV launch the two sweeps below met
DONE = set()                # ... the sweeps that ran


def plan_tuple(p):
    """the kernel instantiation a taken GEMV plan names: ("slab", role, B, nv, ipt) of gemv_q4k_slab_kernel<ROLE, B, NV, IPT> or
    ("chunk", role, NB, nv, d, loop) of gemv_q4k_chunk_kernel<ROLE, NV, D, LOOP, NB> (tests/test_gpu_q4k_gemv.py names its cases by it)"""
    if p["kernel"] == SLAB:
        return ("slab", p["role"], p["B"], p["nv"], p["ipt"])
    assert p["kernel"] == CHUNK, p
    return ("chunk", p["role"], p["B"], p["nv"], p["d"], p["loop"])


def sweep(grid):
    """check() over a grid, the GEMV launches it meets noted in SEEN"""
    for c in grid:
        p = check(*c)
        if p["takes"] and nb.ROUTE_NAMES[p["route"]] == "q4k":
            SEEN.add(plan_tuple(p))
        yield p


def capacity(nb_):
    return 1 if nb_ <= 1 else 2 if nb_ <= 2 else 4 if nb_ <= 4 else 8


def heads_of(n):
    hd = next(h for h in (128, 64, 48, 32, 16, 4) if n % h == 0)
    return n // hd, hd, 4


def whole_blocks(n):
    """the rows the chunk kernel reads: whole 256-value blocks, at most 64 of them"""
    return n % 256 == 0 and n <= 16384


def wide(n, total):
    """route.hip route_is_wide(): per-layer matrices of >= 8 Mi weights"""
    return total < 65536 and total * n >= 8 << 20


def slab_lds(n, B, nmat, rw, heads):
    """what gemv_q4k_slab_kernel lays out: xg[B][GT] 32-byte groups | xn[B][n4] | tmp[B][bpl][16] | red[B][16] | [B][n_head][8] combine
    weights | the product table P[B][nmat][rw][GT + 4] (+ 16 bytes of alignment slack)"""
    n4, bpl = (n + 3) & ~3, (n + 255) // 256
    GT = bpl * 8
    return B * GT * 32 + (B * n4 + B * bpl * 16 + B * 16 + B * heads * 8 + B * nmat * rw * (GT + 4)) * 4 + 16


def chunk_lds(n, NB, nmat, rw, nw, lines, heads):
    """what gemv_q4k_chunk_body.inc lays out: xg[NB][GT] | red[16 (+ [n_head][8] combine weights)] | scr[nw][lines][64] | am[2 nw] |
    the block sums Dt[nmat][NB][rw][bpl | 1] (+ 16 bytes of alignment slack)"""
    bpl = n // 256
    return NB * bpl * 8 * 32 + (16 + heads * 8 + nw * lines * 64 + 2 * nw + nmat * NB * rw * (bpl | 1)) * 4 + 16


def chunk_refuses(kind, n, segs, NB, nmat, heads):
    """the chunk planner's search bound: its smallest slab (1 row, at the search's 16 waves x 8 lines) asks for more than 150 KiB per CU --
    a classifier launch (one STORE tensor of >= 65536 rows) seats 1024 / quantizer threads workgroups on a CU"""
    want = min(1024, max(256, (n // 4 + 63) // 64 * 64))
    cls = kind == 0 and len(segs) == 1 and segs[0] >= 65536
    if cls and want > 512:
        want = 1024
    return chunk_lds(n, NB, nmat, 1, 16, 8, heads if NB == 1 else 0) * (1024 // want if cls else 1) > 150 * 1024


def slab_items_over(n, nmat):
    """more than 4 items per thread at 4 rows per workgroup: 4 rows x 8 groups per block x matrices, on 256..512 threads or -- long rows --
    the block quantizer's n / 4 (at most 1024)"""
    items = 4 * ((n + 255) // 256) * 8 * nmat
    nthr = max(256, min(512, (items + 63) // 64 * 64), min(1024, (n // 4 + 63) // 64 * 64))
    return (items + nthr - 1) // nthr > 4


def check(kind, n, rows, nb_, norm, attn):
    """one descriptor: the GEMM route, a documented refusal, or every invariant of a launch; returns the plan"""
    p = nb.q4k_gemv_plan(kind, n, rows, nb_, norm=norm, attn=attn)
    ctx = (kind, n, rows, nb_, norm, attn, p)
    nmat = 2 if kind == 2 else 1
    bpl = (n + 255) // 256
    GT = bpl * 8
    segs = rows[:1] if kind == 2 else rows
    total = sum(segs)
    heads = attn[0] if attn else 0
    route = nb.ROUTE_NAMES[p["route"]]
    if p["takes"] and route == "q4k_gemm":
        assert nb_ >= 9 and whole_blocks(n) and all(r % 16 == 0 for r in rows), ctx
        assert (p["launches"], p["seqs_per_launch"]) == (1, nb_), ctx
        assert not any(p[k] for k in KERNEL_FIELDS), ctx
        return p
    ragged_segments = kind != 2 and len(rows) > 1 and any(r % 4 for r in rows)
    # Refusals are the item kernel's: its limits where the (first) launch is its own.  Its rows per workgroup are 4..64 and the planner does
    # not trade them for LDS: what fits at 64 rows fits, what does not fit at 4 does not; in between the test takes either answer.
    B0 = capacity(min(nb_, 8))
    limits = ragged_segments or slab_items_over(n, nmat)
    fits = lambda B_, rw_: slab_lds(n, B_, nmat, rw_, heads) <= LDS_MAX
    chunk_one = whole_blocks(n) and not chunk_refuses(kind, n, segs, 1, nmat, heads)
    chunk_can = chunk_one and not chunk_refuses(kind, n, segs, B0, nmat, heads)
    one_must, one_may = not chunk_one and (limits or not fits(1, 4)), not chunk_one and (limits or not fits(1, 64))
    if nb_ == 1:
        must_refuse, may_refuse = one_must, one_may
    elif chunk_can and (min(nb_, 8) >= 5 or wide(n, total)):
        must_refuse = may_refuse = False
    elif chunk_can:
        # 2..4 sequences on matrices that are not wide stay on the item kernel where it holds them -- with its limits (FINDING: such a
        # launch is refused although the chunk kernel takes the same tensors at 1 and at 5..8 sequences)
        must_refuse, may_refuse = limits and fits(B0, 64), limits and fits(B0, 4)
    else:
        # the item kernel in slices of what fits; slices of one sequence are one-sequence launches (the chunk kernel's where it takes them)
        must_refuse = limits if fits(2, 64) else one_must if not fits(2, 4) else limits and one_must
        may_refuse = limits if fits(2, 64) else one_may if not fits(2, 4) else limits or one_may
    if not p["takes"]:
        assert may_refuse, ("refused without a documented reason", ctx)
        assert not any(p.values()), ctx
        return p
    assert not must_refuse, ("taken against a documented limit", ctx)
    assert route == "q4k", ctx
    per, B, nv, rw, nthr = p["seqs_per_launch"], p["B"], p["nv"], p["rw"], p["nthr"]
    # slices: every sequence in one, the last one not empty
    assert 1 <= per <= min(nb_, 8) and p["launches"] * per >= nb_ and (p["launches"] - 1) * per < nb_, ctx
    assert B == capacity(per) and B in (1, 2, 4, 8), ctx
    assert p["lds_bytes"] <= LDS_MAX, ctx
    assert p["pre"] == 0, ctx
    # the grid: every tensor's rows in workgroups of its own
    assert p["grid"] == sum((r + rw - 1) // rw for r in segs), ctx
    want_role = "generic"
    if B == 1:
        want_role = {(0, True, False): "norm_store", (1, False, False): "resid", (1, False, True): "resid_combine",
                     (2, True, False): "norm_swiglu"}.get((kind, norm, attn is not None), "generic")
    # arg-max partials: the query asks for them wherever one STORE tensor is planned as ONE launch; one pair per workgroup
    asked = kind == 0 and len(rows) == 1 and p["launches"] == 1
    if p["kernel"] == CHUNK:
        assert whole_blocks(n) and not chunk_refuses(kind, n, segs, B, nmat, heads) and not chunk_refuses(kind, n, segs, 1, nmat, heads), ctx
        nw = nthr // 64
        assert nthr % 64 == 0 and 1 <= nw <= 16 and nthr >= rw, ctx
        assert p["d"] in (1, 2, 4, 8) and (not p["loop"] or p["d"] == 8) and p["ipt"] == 0, ctx
        loads = nmat * ((rw * bpl + 5) // 6)                        # wave-loads of six blocks per workgroup
        assert (p["rounds"] * 8 if p["loop"] else p["d"]) * nw >= loads and (p["loop"] or p["rounds"] == 1), ("a wave-load without a slot", ctx)
        assert (p["wg0"], p["wg1"], p["wg2"]) == tuple((r + rw - 1) // rw for r in segs) + (0,) * (3 - len(segs)), ctx
        assert p["quant_rows"] == int(per > 1), ctx
        if per == 1:
            assert nv in (1, 2, 4) and nv * 4 * nthr >= n, ("an activation float4 without a register", ctx)
            assert p["role"] == ROLE[want_role] and (p["quant_nthr"], p["quant_nv"]) == (0, 0), ctx
            assert p["partials"] == (p["grid"] if asked else 0), ctx
            assert p["lds_bytes"] == chunk_lds(n, 1, nmat, rw, nw, 1 if p["loop"] else p["d"], heads), ctx
        else:
            # behind the quantizer launch: generic role, nothing staged in registers, no partials; the quantizer runs the one-sequence plan
            one = nb.q4k_gemv_plan(kind, n, rows, 1, norm=norm, attn=attn)
            assert (p["role"], nv, p["partials"]) == (ROLE["generic"], 1, 0), ctx
            assert one["kernel"] == CHUNK and (p["quant_nthr"], p["quant_nv"]) == (one["nthr"], one["nv"]), (one, ctx)
            assert p["lds_bytes"] == chunk_lds(n, B, nmat, rw, nw, B, 0), ctx
            # 2..4 sequences leave the item kernel only on wide matrices or where it cannot hold them (at any rows per workgroup <= 64)
            assert per >= 5 or wide(n, total) or slab_lds(n, capacity(per), nmat, 64, heads) > LDS_MAX, ctx
    else:
        assert p["kernel"] == SLAB, ctx
        assert not chunk_can or (2 <= per <= 4 and not wide(n, total)), ("a whole-block launch the chunk kernel should take", ctx)
        assert not ragged_segments, ctx
        # the template is one launch_q4k_r instantiates: NV x IPT of {0, 1, 2, 4} x {1, 2, 4} with B * NV <= 8
        assert nv in (0, 1, 2, 4) and p["ipt"] in (1, 2, 4) and B * nv <= 8, ctx
        assert nthr % 64 == 0 and nthr <= 1024 and nthr >= rw * B, ("a fold row without a thread", ctx)
        assert p["ipt"] * nthr >= rw * GT * nmat, ("an item without a thread slot", ctx)
        assert nv == 0 or nv * 4 * nthr >= n, ("an activation float4 without a register", ctx)
        assert rw in (4, 8, 16, 32, 64) and (len(segs) == 1 or all(r % rw == 0 for r in segs)), ctx
        if want_role == "norm_swiglu" and (rw * GT) % 64:
            want_role = "generic"                                   # whole waves per matrix, or the matrix of an item is a per-lane choice
        assert p["role"] == ROLE[want_role], ctx
        assert (p["d"], p["loop"], p["rounds"], p["wg0"], p["wg1"], p["wg2"], p["quant_rows"], p["quant_nthr"], p["quant_nv"]) == (0,) * 9, ctx
        assert p["partials"] == (p["grid"] if asked else 0), ctx
        assert p["lds_bytes"] == slab_lds(n, B, nmat, rw, heads), ctx
    if min(nb_, 8) > per:
        # a batch is cut only where the chunk form does not take it and its capacity does not fit the item kernel: larger capacities take
        # the same or more rows per workgroup (more fold threads), so the whole batch at these rows is the least its own plan could ask for
        # (one-sequence slices may be the chunk kernel's: then at the item kernel's 4 rows)
        assert not chunk_can and (p["kernel"] == SLAB or per == 1), ("a batch the chunk form takes was cut", ctx)
        assert slab_lds(n, B0, nmat, rw if p["kernel"] == SLAB else 4, heads) > LDS_MAX, ("a batch that fits was cut", ctx)
    return p


def segment_sets(i):
    """one, two and three weight tensors of a STORE / residual launch; the several-tensor ones in multiples of 4, every fourth ragged"""
    r = ROWS[i % len(ROWS)]
    a, b, c = (ROWS4[(i + k) % len(ROWS4)] for k in range(3))
    return [(r,), (a, b + (3 if i % 4 == 3 else 0)), (a, b, c)]


def named_grid():
    for n in NAMED_N:
        for i, r in enumerate(ROWS):
            for nb_ in NBS:
                for norm in (False, True):
                    for segs in segment_sets(i):
                        yield 0, n, segs, nb_, norm, None
                    yield 2, n, (r, r), nb_, norm, None
                for segs in segment_sets(i):
                    yield 1, n, segs, nb_, False, None
                    yield 1, n, segs, nb_, False, heads_of(n)


def length_grid():
    """every multiple of 4 up to 20480, the other axes rotating"""
    for j, n in enumerate(range(4, 20481, 4)):
        r = ROWS[j % len(ROWS)]
        for nb_ in NBS:
            kind = (j + nb_) % 3
            if kind == 0:
                yield 0, n, segment_sets(j + nb_)[(j // 3) % 3], nb_, bool(j & 1), None
            elif kind == 1:
                yield 1, n, (r,), nb_, False, heads_of(n) if j & 1 else None
            else:
                yield 2, n, (r, r), nb_, bool(j & 2), None


def test_named_shapes_full_cross():
    seen = sum(1 for p in sweep(named_grid()) if p is not None)
    assert seen > 30000
    DONE.add("named")


def test_every_row_length():
    takes = sum(p["takes"] for p in sweep(length_grid()))
    assert takes > 40000
    DONE.add("lengths")


# What the two sweeps above reach of the template space with the default 256 CUs: 55 instantiations of gemv_q4k_slab_kernel as
# role -> (B, NV, IPT) and 90 of gemv_q4k_chunk_kernel as role -> (NB, NV, D, LOOP).  tests/test_gpu_q4k_gemv.py runs a case for every one
# of them on the device.  The launchers instantiate more (the slab kernel every (NV, IPT) of {0, 1, 2, 4} x {1, 2, 4} with B * NV <= 8
# per role and capacity): no descriptor of the sweeps reaches the rest, e.g. the LDS-staged activation (NV = 0) on fewer than 4 items.
SLAB_TUPLES = {
    "generic": [(1, 0, 4), (1, 1, 1), (1, 1, 2), (1, 1, 4), (1, 2, 1), (1, 2, 2), (1, 2, 4), (1, 4, 2), (1, 4, 4), (2, 1, 1), (2, 1, 2),
        (2, 1, 4), (2, 2, 1), (2, 2, 2), (2, 2, 4), (2, 4, 2), (2, 4, 4), (4, 1, 1), (4, 1, 2), (4, 1, 4), (4, 2, 1), (4, 2, 2),
        (4, 2, 4), (8, 1, 1), (8, 1, 2), (8, 1, 4)],
    "norm_store": [(1, 0, 4), (1, 1, 1), (1, 1, 2), (1, 1, 4), (1, 2, 1), (1, 2, 4), (1, 4, 2), (1, 4, 4)],
    "resid": [(1, 0, 4), (1, 1, 1), (1, 1, 2), (1, 1, 4), (1, 2, 1), (1, 2, 4), (1, 4, 2), (1, 4, 4)],
    "resid_combine": [(1, 0, 4), (1, 1, 1), (1, 1, 2), (1, 1, 4), (1, 2, 1), (1, 2, 4), (1, 4, 2), (1, 4, 4)],
    "norm_swiglu": [(1, 1, 1), (1, 1, 2), (1, 1, 4), (1, 2, 4), (1, 4, 4)],
}
CHUNK_TUPLES = {
    "generic": [(1, 1, 1, 0), (1, 1, 2, 0), (1, 1, 4, 0), (1, 1, 8, 0), (1, 1, 8, 1), (1, 2, 1, 0), (1, 2, 2, 0), (1, 2, 4, 0),
        (1, 2, 8, 0), (1, 2, 8, 1), (1, 4, 1, 0), (1, 4, 2, 0), (1, 4, 4, 0), (1, 4, 8, 0), (1, 4, 8, 1), (2, 1, 1, 0), (2, 1, 2, 0),
        (2, 1, 4, 0), (2, 1, 8, 0), (2, 1, 8, 1), (4, 1, 1, 0), (4, 1, 2, 0), (4, 1, 4, 0), (4, 1, 8, 0), (4, 1, 8, 1), (8, 1, 1, 0),
        (8, 1, 2, 0), (8, 1, 4, 0), (8, 1, 8, 0), (8, 1, 8, 1)],
    "norm_store": [(1, 1, 1, 0), (1, 1, 2, 0), (1, 1, 4, 0), (1, 1, 8, 0), (1, 1, 8, 1), (1, 2, 1, 0), (1, 2, 2, 0), (1, 2, 4, 0),
        (1, 2, 8, 0), (1, 2, 8, 1), (1, 4, 1, 0), (1, 4, 2, 0), (1, 4, 4, 0), (1, 4, 8, 0), (1, 4, 8, 1)],
    "resid": [(1, 1, 1, 0), (1, 1, 2, 0), (1, 1, 4, 0), (1, 1, 8, 0), (1, 1, 8, 1), (1, 2, 1, 0), (1, 2, 2, 0), (1, 2, 4, 0),
        (1, 2, 8, 0), (1, 2, 8, 1), (1, 4, 1, 0), (1, 4, 2, 0), (1, 4, 4, 0), (1, 4, 8, 0), (1, 4, 8, 1)],
    "resid_combine": [(1, 1, 1, 0), (1, 1, 2, 0), (1, 1, 4, 0), (1, 1, 8, 0), (1, 1, 8, 1), (1, 2, 1, 0), (1, 2, 2, 0), (1, 2, 4, 0),
        (1, 2, 8, 0), (1, 2, 8, 1), (1, 4, 1, 0), (1, 4, 2, 0), (1, 4, 4, 0), (1, 4, 8, 0), (1, 4, 8, 1)],
    "norm_swiglu": [(1, 1, 1, 0), (1, 1, 2, 0), (1, 1, 4, 0), (1, 1, 8, 0), (1, 1, 8, 1), (1, 2, 1, 0), (1, 2, 2, 0), (1, 2, 4, 0),
        (1, 2, 8, 0), (1, 2, 8, 1), (1, 4, 1, 0), (1, 4, 2, 0), (1, 4, 4, 0), (1, 4, 8, 0), (1, 4, 8, 1)],
}
UNIVERSE = {("slab", ROLE[r]) + t for r, ts in SLAB_TUPLES.items() for t in ts} | {("chunk", ROLE[r]) + t for r, ts in CHUNK_TUPLES.items() for t in ts}


def test_universe_is_what_the_sweeps_reach():
    """a retune that adds or drops a reachable instantiation fails here: move UNIVERSE, and the cases of tests/test_gpu_q4k_gemv.py with it"""
    if "named" not in DONE:
        test_named_shapes_full_cross()
    if "lengths" not in DONE:
        test_every_row_length()
    print(sorted(SEEN))
    assert len(UNIVERSE) == 145
    assert SEEN == UNIVERSE, (sorted(SEEN - UNIVERSE), sorted(UNIVERSE - SEEN))


def test_documented_refusals():
    P = nb.q4k_gemv_plan
    # tensors of 8 | 3 rows: the item kernel refuses them, the chunk kernel's workgroups take any count
    assert P(0, 192, (8, 4))["takes"] == 1 and check(0, 192, (8, 3), 1, True, None)["takes"] == 0 and P(0, 192, (3,))["takes"] == 1
    assert P(0, 256, (8, 3))["kernel"] == CHUNK
    # 4 rows of 16388 values with SwiGLU: 4168 items on 1024 threads
    assert P(2, 16388, (16, 16))["takes"] == 0 and P(2, 16384, (16, 16))["kernel"] == CHUNK and P(1, 16388, (16,))["takes"] == 1
    # a malformed descriptor is an error, not a plan
    for bad in (dict(kind=3, n=256, rows=(4,)), dict(kind=0, n=258, rows=(4,)), dict(kind=2, n=256, rows=(4, 8)), dict(kind=0, n=256, rows=(4,), nb=65),
                dict(kind=0, n=256, rows=(4,), attn=(2, 128, 4)), dict(kind=1, n=256, rows=(4,), attn=(2, 64, 4))):
        with pytest.raises(nb.NanoHipError):
            P(**bad)


def test_long_partial_block_rows_run_in_slices():
    """the item kernel's LDS-fit slicing, which only partial-block rows reach: 56.5 KB per sequence at 9732 values, 24.1 KB at 4100"""
    for nb_, launches, per in ((1, 1, 1), (2, 1, 2), (3, 2, 2), (5, 3, 2), (8, 4, 2), (11, 6, 2), (64, 32, 2)):
        p = check(1, 9732, (64,), nb_, False, None)
        assert (p["kernel"], p["launches"], p["seqs_per_launch"]) == (SLAB, launches, per), (nb_, p)
    for nb_, launches, per in ((4, 1, 4), (5, 2, 4), (7, 2, 4), (8, 2, 4), (11, 3, 4)):
        p = check(0, 4100, (64, 32, 32), nb_, True, None)
        assert (p["kernel"], p["launches"], p["seqs_per_launch"], p["B"]) == (SLAB, launches, per, 4), (nb_, p)
    # whole blocks of the same lengths: the chunk form shares the weights among all 8
    p = check(1, 9728, (64,), 8, False, None)
    assert (p["kernel"], p["launches"], p["seqs_per_launch"], p["quant_rows"]) == (CHUNK, 1, 8, 1), p
    # where 8 fit, a batch beyond 8 runs in groups of 8
    p = check(0, 192, (36, 4, 12), 11, True, None)
    assert (p["kernel"], p["B"], p["launches"], p["seqs_per_launch"]) == (SLAB, 8, 2, 8), p


# The launches of every projection of Qwen3-0.6B, Qwen3-4B and the tiny presets -- keyed (kind, n, rows, split-attention partials) -- at
# 1, 2, 3, 4, 5, 8, 11 and 64 sequences, copied from the planners and predicates before the plan became a function of its own: the
# launches of models that ran before must not move.  "gemm": the int8 MFMA GEMM's route.  Slab launches: ("slab", role, B, nv, ipt, rw,
# nthr, grid, lds_bytes, partials, launches, seqs_per_launch); chunk launches: ("chunk", role, B, nv, d, loop, rounds, rw, nthr, grid,
# lds_bytes, quant_nthr, quant_nv, partials, launches, seqs_per_launch).
PIN_NBS = (1, 2, 3, 4, 5, 8, 11, 64)
MODEL_PLANS = {
    (0, 1024, (2048, 1024, 1024), None): [
        ('chunk', 1, 1, 1, 2, 0, 1, 16, 384, 256, 4544, 0, 0, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 16, 512, 256, 15504, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 16, 512, 256, 30992, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 16, 512, 256, 30992, 0, 1, 4),
        ('chunk', 0, 8, 1, 2, 0, 1, 16, 384, 256, 23168, 384, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 2, 0, 1, 16, 384, 256, 23168, 384, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (1, 2048, (1024,), None): [
        ('chunk', 2, 1, 1, 1, 0, 1, 4, 512, 256, 4384, 0, 0, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 8, 512, 128, 26000, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 8, 512, 128, 51984, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 8, 512, 128, 51984, 0, 1, 4),
        ('chunk', 0, 8, 1, 1, 0, 1, 4, 512, 256, 34064, 512, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 1, 0, 1, 4, 512, 256, 34064, 512, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (1, 2048, (1024,), (16, 128, 4)): [
        ('chunk', 3, 1, 1, 1, 0, 1, 4, 512, 256, 4896, 0, 0, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 8, 512, 128, 27024, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 8, 512, 128, 54032, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 8, 512, 128, 54032, 0, 1, 4),
        ('chunk', 0, 8, 1, 1, 0, 1, 4, 512, 256, 34064, 512, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 1, 0, 1, 4, 512, 256, 34064, 512, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (2, 1024, (3072, 3072), None): [
        ('chunk', 4, 1, 1, 2, 0, 1, 12, 512, 256, 5744, 0, 0, 0, 1, 1),
        ('slab', 0, 2, 1, 2, 16, 512, 192, 20112, 0, 1, 2),
        ('slab', 0, 4, 1, 2, 16, 512, 192, 40208, 0, 1, 3),
        ('slab', 0, 4, 1, 2, 16, 512, 192, 40208, 0, 1, 4),
        ('chunk', 0, 8, 1, 2, 0, 1, 12, 512, 256, 28560, 512, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 2, 0, 1, 12, 512, 256, 28560, 512, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (1, 3072, (1024,), None): [
        ('chunk', 2, 1, 1, 1, 0, 1, 4, 768, 256, 6528, 0, 0, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 768, 256, 35600, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 768, 256, 71184, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 768, 256, 71184, 0, 1, 4),
        ('chunk', 0, 8, 1, 1, 0, 1, 4, 768, 256, 50992, 768, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 1, 0, 1, 4, 768, 256, 50992, 768, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (0, 1024, (151936,), None): [
        ('chunk', 1, 1, 1, 8, 1, 4, 149, 256, 1020, 5140, 0, 0, 1020, 1, 1),
        ('slab', 0, 2, 1, 4, 64, 512, 2374, 29328, 2374, 1, 2),
        ('slab', 0, 4, 1, 4, 64, 512, 2374, 58640, 2374, 1, 3),
        ('slab', 0, 4, 1, 4, 64, 512, 2374, 58640, 2374, 1, 4),
        ('slab', 0, 8, 1, 4, 64, 512, 2374, 117264, 2374, 1, 5),
        ('slab', 0, 8, 1, 4, 64, 512, 2374, 117264, 2374, 1, 8),
        ('slab', 0, 8, 1, 4, 64, 512, 2374, 117264, 0, 2, 8),
        ('slab', 0, 8, 1, 4, 64, 512, 2374, 117264, 0, 8, 8),
    ],
    (0, 2560, (4096, 1024, 1024), None): [
        ('chunk', 1, 1, 1, 4, 0, 1, 25, 1024, 246, 20252, 0, 0, 0, 1, 1),
        ('chunk', 0, 2, 1, 4, 0, 1, 25, 1024, 246, 15720, 1024, 1, 0, 1, 2),
        ('chunk', 0, 4, 1, 4, 0, 1, 25, 1024, 246, 31232, 1024, 1, 0, 1, 3),
        ('chunk', 0, 4, 1, 4, 0, 1, 25, 1024, 246, 31232, 1024, 1, 0, 1, 4),
        ('chunk', 0, 8, 1, 4, 0, 1, 25, 1024, 246, 62256, 1024, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 4, 0, 1, 25, 1024, 246, 62256, 1024, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (1, 4096, (2560,), None): [
        ('chunk', 2, 1, 1, 2, 0, 1, 10, 1024, 256, 13176, 0, 0, 0, 1, 1),
        ('chunk', 0, 2, 1, 2, 0, 1, 10, 1024, 256, 17952, 1024, 1, 0, 1, 2),
        ('chunk', 0, 4, 1, 2, 0, 1, 10, 1024, 256, 35696, 1024, 1, 0, 1, 3),
        ('chunk', 0, 4, 1, 2, 0, 1, 10, 1024, 256, 35696, 1024, 1, 0, 1, 4),
        ('chunk', 0, 8, 1, 2, 0, 1, 10, 1024, 256, 71184, 1024, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 2, 0, 1, 10, 1024, 256, 71184, 1024, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (1, 4096, (2560,), (32, 128, 4)): [
        ('chunk', 3, 1, 1, 2, 0, 1, 10, 1024, 256, 14200, 0, 0, 0, 1, 1),
        ('chunk', 0, 2, 1, 2, 0, 1, 10, 1024, 256, 17952, 1024, 1, 0, 1, 2),
        ('chunk', 0, 4, 1, 2, 0, 1, 10, 1024, 256, 35696, 1024, 1, 0, 1, 3),
        ('chunk', 0, 4, 1, 2, 0, 1, 10, 1024, 256, 35696, 1024, 1, 0, 1, 4),
        ('chunk', 0, 8, 1, 2, 0, 1, 10, 1024, 256, 71184, 1024, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 2, 0, 1, 10, 1024, 256, 71184, 1024, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (2, 2560, (9728, 9728), None): [
        ('chunk', 4, 1, 1, 8, 0, 1, 38, 1024, 256, 38880, 0, 0, 0, 1, 1),
        ('chunk', 0, 2, 1, 8, 0, 1, 38, 1024, 256, 20208, 1024, 1, 0, 1, 2),
        ('chunk', 0, 4, 1, 8, 0, 1, 38, 1024, 256, 40208, 1024, 1, 0, 1, 3),
        ('chunk', 0, 4, 1, 8, 0, 1, 38, 1024, 256, 40208, 1024, 1, 0, 1, 4),
        ('chunk', 0, 8, 1, 8, 0, 1, 38, 1024, 256, 80208, 1024, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 8, 0, 1, 38, 1024, 256, 80208, 1024, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (1, 9728, (2560,), None): [
        ('chunk', 2, 1, 4, 4, 0, 1, 10, 1024, 256, 27880, 0, 0, 0, 1, 1),
        ('chunk', 0, 2, 1, 4, 0, 1, 10, 1024, 256, 30976, 1024, 4, 0, 1, 2),
        ('chunk', 0, 4, 1, 4, 0, 1, 10, 1024, 256, 61744, 1024, 4, 0, 1, 3),
        ('chunk', 0, 4, 1, 4, 0, 1, 10, 1024, 256, 61744, 1024, 4, 0, 1, 4),
        ('chunk', 0, 8, 1, 4, 0, 1, 10, 1024, 256, 123280, 1024, 4, 0, 1, 5),
        ('chunk', 0, 8, 1, 4, 0, 1, 10, 1024, 256, 123280, 1024, 4, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (0, 2560, (151936,), None): [
        ('chunk', 1, 1, 1, 8, 1, 8, 594, 1024, 256, 33000, 0, 0, 256, 1, 1),
        ('slab', 0, 2, 1, 4, 32, 640, 4748, 48528, 4748, 1, 2),
        ('slab', 0, 4, 1, 4, 32, 640, 4748, 97040, 4748, 1, 3),
        ('slab', 0, 4, 1, 4, 32, 640, 4748, 97040, 4748, 1, 4),
        ('chunk', 0, 8, 1, 8, 1, 3, 198, 1024, 768, 123152, 1024, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 8, 1, 3, 198, 1024, 768, 123152, 1024, 1, 0, 1, 8),
        ('chunk', 0, 8, 1, 8, 1, 3, 198, 1024, 768, 123152, 1024, 1, 0, 2, 8),
        ('chunk', 0, 8, 1, 8, 1, 3, 198, 1024, 768, 123152, 1024, 1, 0, 8, 8),
    ],
    (0, 256, (256, 128, 128), None): [
        ('chunk', 1, 1, 1, 1, 0, 1, 2, 256, 256, 1400, 0, 0, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 128, 3216, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 128, 6416, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 128, 6416, 0, 1, 4),
        ('chunk', 0, 8, 1, 1, 0, 1, 2, 256, 256, 10416, 256, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 1, 0, 1, 2, 256, 256, 10416, 256, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (1, 256, (256,), None): [
        ('chunk', 2, 1, 1, 1, 0, 1, 1, 256, 256, 1396, 0, 0, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 64, 3216, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 64, 6416, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 64, 6416, 0, 1, 4),
        ('chunk', 0, 8, 1, 1, 0, 1, 1, 256, 256, 10384, 256, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 1, 0, 1, 1, 256, 256, 10384, 256, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (1, 256, (256,), (4, 64, 4)): [
        ('chunk', 3, 1, 1, 1, 0, 1, 1, 256, 256, 1524, 0, 0, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 64, 3472, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 64, 6928, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 64, 6928, 0, 1, 4),
        ('chunk', 0, 8, 1, 1, 0, 1, 1, 256, 256, 10384, 256, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 1, 0, 1, 1, 256, 256, 10384, 256, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (2, 256, (768, 768), None): [
        ('chunk', 4, 1, 1, 1, 0, 1, 3, 256, 256, 1416, 0, 0, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 192, 3600, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 192, 7184, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 192, 7184, 0, 1, 4),
        ('chunk', 0, 8, 1, 1, 0, 1, 3, 256, 256, 10544, 256, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 1, 0, 1, 3, 256, 256, 10544, 256, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (1, 768, (256,), None): [
        ('chunk', 2, 1, 1, 1, 0, 1, 1, 256, 256, 1916, 0, 0, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 64, 9104, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 64, 18192, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 64, 18192, 0, 1, 4),
        ('chunk', 0, 8, 1, 1, 0, 1, 1, 256, 256, 14544, 256, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 1, 0, 1, 1, 256, 256, 14544, 256, 1, 0, 1, 8),
        'gemm',
        'gemm',
    ],
    (0, 256, (1024,), None): [
        ('chunk', 1, 1, 1, 1, 0, 1, 4, 256, 256, 1408, 0, 0, 256, 1, 1),
        ('slab', 0, 2, 1, 1, 8, 256, 128, 3600, 128, 1, 2),
        ('slab', 0, 4, 1, 1, 8, 256, 128, 7184, 128, 1, 3),
        ('slab', 0, 4, 1, 1, 8, 256, 128, 7184, 128, 1, 4),
        ('chunk', 0, 8, 1, 1, 0, 1, 4, 256, 256, 10480, 256, 1, 0, 1, 5),
        ('chunk', 0, 8, 1, 1, 0, 1, 4, 256, 256, 10480, 256, 1, 0, 1, 8),
        ('chunk', 0, 8, 1, 1, 0, 1, 4, 256, 256, 10480, 256, 1, 0, 2, 8),
        ('chunk', 0, 8, 1, 1, 0, 1, 4, 256, 256, 10480, 256, 1, 0, 8, 8),
    ],
    (0, 128, (128, 64, 64), None): [
        ('slab', 1, 1, 1, 1, 4, 256, 64, 1104, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 64, 2192, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 64, 4368, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 64, 4368, 0, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 64, 8720, 0, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 64, 8720, 0, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 64, 8720, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 64, 8720, 0, 8, 8),
    ],
    (1, 128, (128,), None): [
        ('slab', 2, 1, 1, 1, 4, 256, 32, 1104, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 32, 2192, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 32, 4368, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 32, 4368, 0, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 8720, 0, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 8720, 0, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 8720, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 8720, 0, 8, 8),
    ],
    (1, 128, (128,), (4, 32, 4)): [
        ('slab', 3, 1, 1, 1, 4, 256, 32, 1232, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 32, 2448, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 32, 4880, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 32, 4880, 0, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 9744, 0, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 9744, 0, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 9744, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 9744, 0, 8, 8),
    ],
    (2, 128, (384, 384), None): [
        ('slab', 0, 1, 1, 1, 4, 256, 96, 1296, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 96, 2576, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 96, 5136, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 96, 5136, 0, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 96, 10256, 0, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 96, 10256, 0, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 96, 10256, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 96, 10256, 0, 8, 8),
    ],
    (1, 384, (128,), None): [
        ('slab', 2, 1, 1, 1, 4, 256, 32, 2576, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 32, 5136, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 32, 10256, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 32, 10256, 0, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 20496, 0, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 20496, 0, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 20496, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 32, 20496, 0, 8, 8),
    ],
    (0, 128, (512,), None): [
        ('slab', 1, 1, 1, 1, 4, 256, 128, 1104, 128, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 128, 2192, 128, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 128, 4368, 128, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 128, 4368, 128, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 128, 8720, 128, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 128, 8720, 128, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 128, 8720, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 128, 8720, 0, 8, 8),
    ],
    (0, 192, (192, 96, 96), None): [
        ('slab', 1, 1, 1, 1, 4, 256, 96, 1360, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 96, 2704, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 96, 5392, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 96, 5392, 0, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 96, 10768, 0, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 96, 10768, 0, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 96, 10768, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 96, 10768, 0, 8, 8),
    ],
    (1, 192, (192,), None): [
        ('slab', 2, 1, 1, 1, 4, 256, 48, 1360, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 48, 2704, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 48, 5392, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 48, 5392, 0, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 10768, 0, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 10768, 0, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 10768, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 10768, 0, 8, 8),
    ],
    (1, 192, (192,), (4, 48, 4)): [
        ('slab', 3, 1, 1, 1, 4, 256, 48, 1488, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 48, 2960, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 48, 5904, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 48, 5904, 0, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 11792, 0, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 11792, 0, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 11792, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 11792, 0, 8, 8),
    ],
    (2, 192, (352, 352), None): [
        ('slab', 0, 1, 1, 1, 4, 256, 88, 1552, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 88, 3088, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 88, 6160, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 88, 6160, 0, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 88, 12304, 0, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 88, 12304, 0, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 88, 12304, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 88, 12304, 0, 8, 8),
    ],
    (1, 352, (192,), None): [
        ('slab', 2, 1, 1, 1, 4, 256, 48, 2448, 0, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 48, 4880, 0, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 48, 9744, 0, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 48, 9744, 0, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 19472, 0, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 19472, 0, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 19472, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 48, 19472, 0, 8, 8),
    ],
    (0, 192, (512,), None): [
        ('slab', 1, 1, 1, 1, 4, 256, 128, 1360, 128, 1, 1),
        ('slab', 0, 2, 1, 1, 4, 256, 128, 2704, 128, 1, 2),
        ('slab', 0, 4, 1, 1, 4, 256, 128, 5392, 128, 1, 3),
        ('slab', 0, 4, 1, 1, 4, 256, 128, 5392, 128, 1, 4),
        ('slab', 0, 8, 1, 1, 4, 256, 128, 10768, 128, 1, 5),
        ('slab', 0, 8, 1, 1, 4, 256, 128, 10768, 128, 1, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 128, 10768, 0, 2, 8),
        ('slab', 0, 8, 1, 1, 4, 256, 128, 10768, 0, 8, 8),
    ],
}


def pin_of(p):
    if nb.ROUTE_NAMES[p["route"]] == "q4k_gemm":
        return "gemm"
    if p["kernel"] == SLAB:
        return ("slab",) + tuple(p[k] for k in ("role", "B", "nv", "ipt", "rw", "nthr", "grid", "lds_bytes", "partials", "launches", "seqs_per_launch"))
    return ("chunk",) + tuple(p[k] for k in ("role", "B", "nv", "d", "loop", "rounds", "rw", "nthr", "grid", "lds_bytes", "quant_nthr", "quant_nv", "partials",
                                            "launches", "seqs_per_launch"))


@pytest.mark.parametrize("shape", list(MODEL_PLANS), ids=lambda s: f"k{s[0]}-{s[1]}x{sum(s[2][:1] if s[0] == 2 else s[2])}{'-attn' if s[3] else ''}")
def test_model_plans_unchanged(shape):
    kind, n, rows, attn = shape
    assert len(MODEL_PLANS[shape]) == len(PIN_NBS)
    for nb_, want in zip(PIN_NBS, MODEL_PLANS[shape]):
        p = check(kind, n, rows, nb_, kind != 1, attn)
        assert p["takes"] == 1 and pin_of(p) == want, (shape, nb_, p)


def test_query_needs_no_device_and_follows_no_pointer():
    """shape fields only: the descriptor of the binding's query holds no weight, activation or output pointer at all"""
    p = nb.q4k_gemv_plan(0, 1024, (2048, 1024, 1024), 1, norm=True)
    assert p["takes"] == 1 and p["kernel"] == CHUNK and p["role"] == ROLE["norm_store"] and p["grid"] == p["wg0"] + p["wg1"] + p["wg2"]
    assert np.all([nb.q4k_gemv_plan(0, 1024, (2048, 1024, 1024), 1, norm=True, cus=c) == p for c in (0, 256)])
    # the chunk kernel fits its grid to the chip
    assert nb.q4k_gemv_plan(0, 1024, (2048, 1024, 1024), 1, norm=True, cus=64)["grid"] < p["grid"]
