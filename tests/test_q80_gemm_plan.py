"""CPU sweep of the batched Q80 launch plan (nano_hip_q80_gemm_plan: route_kind() + gemm_q80_plan(), the functions the router and the
launchers themselves follow -- nano_amd/csrc/route.hip, gemm_q80_host.h).  No GPU: the query is host arithmetic on a shape.

For every descriptor of the grid exactly one of three things holds.
  * The router keeps it with the GEMV kernels for a reason of its own (fewer than 9 sequences on a matrix that is neither heavy nor
    wide; two sequences on a wide canonical matrix): a GEMV route and zeros.  tests/test_q80_gemv_plan.py holds those launches.
  * The router asks for a batched kernel and gemm_q80_plan() refuses (a GEMV route and zeros) for one of the documented reasons
      - split-attention partials as the input (the batched kernels read fragment-order activations),
      - canonical launches (group size 64, n % 256 == 0, not ordered, not a tall STORE matrix): a weight tensor of 2^32 - 2^20 bytes or
        more (32-bit buffer offsets), 65536 rows or more in all, or a launch that fits neither G6 (its unit-sum table [tiles per
        workgroup][units][token tiles] KiB next to the waves' buffers within a CU's LDS, at most 4 items per wave -- 3 at four token
        tiles) nor G7 (17..64 tokens, at most 8 row tiles per workgroup and 14 (row tile, token tile) pairs over its consumer waves),
      - the others: interior weight tensors whose rows are no multiple of G2's 16-row tile, a group count whose magic division is
        not exact over G2's index range, or G2's stages and product tables beyond a CU's LDS (SECTION3 below: launches the parent
        commit sent to G2, whose launcher returned an error after the quantizer launch had gone out).
  * The plan is a launch of a kernel that exists -- the template tuple is one the launch ladders instantiate -- with the LDS bytes of
    the layout the kernel addresses and no more than a CU has, a workgroup for every row tile, no tile across two weight tensors, and
    the kernel's own limits (restated below from the kernels' comments).
The kernels behind the plans run in tests/test_gpu_q80_gemm.py, whose coverage test reads UNIVERSE below."""
import numpy as np
import pytest

from nano_amd import binding as nb
from test_q80_gemv_plan import ROWS, NBS, NAMED_N, GSS, segment_sets, heads_of, canonical

LDS_MAX = 163840            # bytes of LDS a gfx950 CU has
KERN = {n: i for i, n in enumerate(nb.Q80_GEMM_KERNELS)}
GEMV_ROUTES = ("gemv", "gemv_preq", "gemv_sliced")
ROUTE_OF = {"g6s": "frag_g6", "g6f": "frag_g6", "g7": "frag_g7", "g7k": "frag_g7", "gc": "frag_old", "g2": "frag_old"}
TOKENS = sorted(set(NBS) | {9, 16, 17, 32, 33, 48, 49})
F = nb.Q80_GEMM_PLAN_FIELDS
# the fields each kernel's launch is made of; every other field of its plan is 0
COMMON = ("route", "kernel", "threads", "grid", "lds_bytes", "norm_order", "takes")
TILES = ("hh", "ntiles", "tc0", "tc1", "tpw", "full", "ms")
OWN = {
    "g6s": TILES + ("tt", "nv", "r", "nu", "nw", "rounds", "tts", "magic"),
    "g6f": TILES + ("tt", "nv", "r", "nu", "nw", "rounds", "tts", "magic"),
    "g7": TILES + ("tp", "pp", "nk", "ttl", "nsa", "pre", "a_stage", "a_ws", "b_base", "b_stage", "b_xs"),
    "g7k": ("hh", "ntiles", "nk", "nu", "ttl", "ks", "ncw", "nss", "tab", "ring", "nl"),
    "gc": ("tt", "ntiles", "ttl", "waves", "lt", "nhc", "nwaves", "ng"),
    "g2": ("tt", "gs", "sw", "magic", "ng", "npass"),
}

SEEN = set()                # (kernel, template tuple) of every launch the sweeps below met at 256 CUs (the device's)
DONE = set()


def ceil_div(a, b):
    return (a + b - 1) // b


def tuple_of(p):
    """(kernel, its template values): G6 MODE S (NV, R, MS), MODE F (R, MS, TT); G7 (TP, PP, MS); G7K (); GC (TT); G2 (GS, SW, TT)"""
    k = nb.Q80_GEMM_KERNELS[p["kernel"]]
    return (k,) + {"g6s": (p["nv"], p["r"], p["ms"]), "g6f": (p["r"], p["ms"], p["tt"]), "g7": (p["tp"], p["pp"], p["ms"]), "g7k": (),
                   "gc": (p["tt"],), "g2": (p["gs"], p["sw"], p["tt"])}[k]


_MAGIC = {}


def magic_exact(div, bits, upto):
    """(e * ceil(2^bits / div)) >> bits == e // div for every e < upto, in the kernels' 32-bit arithmetic"""
    key = (div, bits, upto)
    if key not in _MAGIC:
        e = np.arange(upto, dtype=np.uint64)
        prod = (e * np.uint64(((1 << bits) + div - 1) // div)) & np.uint64(0xffffffff)
        _MAGIC[key] = bool(np.all(prod >> np.uint64(bits) == e // np.uint64(div)))
    return _MAGIC[key]


def g2_lds(gs, n, sw, tt):
    """gemm_q80.hip: two weight stages [matrices][16 rows][528] | weight scales [matrices][16][ng | 1] floats | product tables
    [matrices][512 / gs groups of a pass][16 rows][16 TT + 1 tokens] floats, two of them except SwiGLU at four token tiles"""
    nmat = 2 if sw else 1
    return 2 * nmat * 16 * 528 + nmat * 16 * ((n // gs) | 1) * 4 + (1 if (tt == 4 and sw) else 2) * nmat * (512 // gs) * 16 * (16 * tt + 1) * 4


def gc_takes(gs, kind, n, rows, nb_):
    """gemm_q80_cls.hip: group size 64, one STORE tensor of >= 16384 rows, 2..64 tokens, a group count that is a multiple of 4, rows of at most
    8192 values, 32-bit buffer offsets, and min(token tiles, 2) tiles of fragments [ng][1024 + 64] staged next to four waves' buffers"""
    ng = n // 64
    return gs == 64 and kind == 0 and len(rows) == 1 and rows[0] >= 16384 and 2 <= nb_ <= 64 and n % 256 == 0 and n <= 8192 and \
        rows[0] * n < (1 << 32) - (1 << 20) and min(ceil_div(nb_, 16), 2) * ng * 1088 + 4 * 8960 + 256 <= LDS_MAX


def row_tiles(p, segs, sw, cus):
    """G6 / G7: a tile is two halves of hh <= 8 rows (SwiGLU: W1's rows and the same rows of W3) inside one weight tensor; workgroup b
    owns tiles b, b + grid, ...: every tile has a workgroup, `full` of them own tpw tiles and the others tpw - 1"""
    assert 1 <= p["hh"] <= 8, p
    trw = p["hh"] if sw else 2 * p["hh"]
    ends = np.cumsum([ceil_div(r, trw) for r in segs]).tolist()
    assert p["ntiles"] == ends[-1]
    assert p["tc0"] == (ends[0] if len(segs) > 1 else 0xffffffff) and p["tc1"] == (ends[1] if len(segs) > 2 else 0xffffffff)
    assert p["grid"] == min(p["ntiles"], cus) and p["tpw"] == ceil_div(p["ntiles"], p["grid"])
    assert 1 <= p["full"] <= p["grid"] and p["full"] * p["tpw"] + (p["grid"] - p["full"]) * (p["tpw"] - 1) == p["ntiles"]
    assert p["ms"] == int(not sw and len(segs) > 1)


def g6_fits(segs, n, sw, tt, cus):
    """G6 at its own choice of tile height (the rows the busiest workgroup streams + 2 per tile, ties to the taller tile): the unit-sum
    table fits next to the waves' buffers, and a wave owns at most 4 items (3 at four token tiles)"""
    nu = ceil_div(n // 64, 8)
    best = None
    for hh in range(1, 9):
        trw = hh if sw else 2 * hh
        tiles = sum(ceil_div(r, trw) for r in segs)
        tpw = ceil_div(tiles, min(tiles, cus))
        cost = tpw * (trw * (2 if sw else 1) + 2)
        if best is None or cost <= best[0]:
            best = (cost, tpw)
    tpw = best[1]
    tts = tt if (tt == 2 and tpw * nu < 8 and tpw * nu * tt <= 32) else 1
    items = tpw * nu * tts
    nw = 8
    while nw > items:
        nw >>= 1
    rounds = ceil_div(items, nw)
    return rounds <= (3 if tt == 4 else 4) and nw * 9472 + tpw * nu * tt * 1024 + ((tpw + 3) & ~3) * 4 + 64 <= LDS_MAX


def g7_fits(segs, n, sw, ttl, cus):
    """G7 at its own choice of tile height (tiles per workgroup x max(6 per token tile, a tile's rows + 2), ties to the taller tile): at most 8
    row tiles per workgroup, 14 (row tile, token tile or pair of them) items over the consumer waves, two weight and two fragment stages in LDS,
    and where it pays: row tiles per workgroup x token tiles >= 8, or at most four 256-byte steps"""
    best = None
    for hh in range(1, 9):
        trw = hh if sw else 2 * hh
        tiles = sum(ceil_div(r, trw) for r in segs)
        tpw = ceil_div(tiles, min(tiles, cus))
        cost = tpw * max(6 * ttl, trw * (2 if sw else 1) + 2)
        if best is None or cost <= best[0]:
            best = (cost, tpw)
    tpw = best[1]
    if tpw > 8 or tpw * ceil_div(ttl, 2) > 14:
        return False
    pp = 1 if tpw * ttl <= 14 else 2
    a_stage, b_stage = tpw * 4096 + ceil_div(tpw, 4) * 1024, ceil_div(ttl, pp) * pp * 4096 + 1024
    return 2 * b_stage + 1024 + 2 * a_stage <= LDS_MAX and (tpw * ttl >= 8 or n // 256 <= 4)


def check(gs, kind, n, rows, nb_, ordered=False, *, attn=None, cus=256, use_gemm=False):
    """one descriptor: a GEMV route of the router's, a documented refusal, or every invariant of a launch; returns the plan"""
    p = nb.q80_gemm_plan(kind, n, rows, nb_, gs=gs, attn=attn, ordered=ordered, use_gemm=use_gemm, cus=cus)
    ctx = (gs, kind, n, rows, nb_, ordered, attn, cus, use_gemm, p)
    c = cus or 256
    sw = kind == 2
    segs = rows[:1] if sw else rows
    total = sum(segs)
    ng, ttl = n // gs, ceil_div(nb_, 16)
    tt = 1 if ttl <= 1 else 2 if ttl == 2 else 4
    canon = canonical(gs, n, kind, rows, ordered)
    route = nb.ROUTE_NAMES[p["route"]]
    assert p["takes"] == 1, ctx
    # route.hip's own conditions: the batched route from 9 sequences on (use_gemm: from one), at 8 on heavy matrices, from 2 on wide ones --
    # but two sequences on a wide canonical matrix stay with the balanced SLAB GEMV
    wide = total < 65536 and total * n >= 8 << 20
    heavy = (total // 16) * nb_ * n > 4 << 20
    batched = (use_gemm or nb_ >= 9 or (nb_ == 8 and heavy) or (wide and nb_ >= 2)) and not (canon and wide and nb_ == 2)
    if route in GEMV_ROUTES:
        assert not any(p[f] for f in F[1:-1]), ctx
        assert route == "gemv_sliced" or nb_ <= 8, ctx
        if not batched:
            return p
        if attn is not None:
            why = "attention partials"
        elif canon:
            big = any(r * n >= (1 << 32) - (1 << 20) for r in segs) or total >= 65536
            g7k = 3 <= nb_ <= 48 and len(rows) == 1 and n // 256 >= 8 and ceil_div(rows[0], 16) <= c
            why = "oversize" if big else None if (g7k or g6_fits(segs, n, sw, tt, c) or (nb_ >= 17 and g7_fits(segs, n, sw, ttl, c))) else "fits neither G6 nor G7"
        else:
            ragged = not sw and any(r % 16 for r in rows[:-1])
            why = "ragged interior tensors" if ragged else "magic" if not magic_exact(ng, 20, 16 * ng + 4096) else \
                  "section 3" if g2_lds(gs, n, sw, tt) > LDS_MAX else None
            assert not gc_takes(gs, kind, n, rows, nb_), ("GC's shape refused", ctx)
        assert why, ("refused without a documented reason", ctx)
        return p
    assert batched, ("a batched launch the router's own conditions do not ask for", ctx)
    k = nb.Q80_GEMM_KERNELS[p["kernel"]]
    assert route == ROUTE_OF[k] and attn is None, ctx
    assert not any(p[f] for f in F if f not in COMMON + OWN[k]), ("a field of another kernel", ctx)
    assert p["lds_bytes"] <= LDS_MAX and p["threads"] % 64 == 0 and 64 <= p["threads"] <= 1024 and p["grid"] >= 1, ctx
    assert p["norm_order"] == (512 if canon and wide and n <= 10240 else 256), ctx
    # the order of preference: canonical launches never leave the canonical kernels, the others never enter them
    assert (k in ("g6s", "g6f", "g7", "g7k")) == canon, ctx
    if cus == 256:
        SEEN.add(tuple_of(p))
    if k in ("g6s", "g6f"):
        row_tiles(p, segs, sw, c)
        nu, nw, tts, tpw = p["nu"], p["nw"], p["tts"], p["tpw"]
        assert nu == ceil_div(ng, 8) and n % 256 == 0 and gs == 64, ctx
        assert nw in (1, 2, 4, 8) and p["threads"] == 64 * nw, ctx
        items = tpw * nu * tts
        assert p["rounds"] == ceil_div(items, nw) and (nw == 8 or nw <= items < 2 * nw), ctx
        assert p["magic"] == (65536 + nu * tts - 1) // (nu * tts) and magic_exact(nu * tts, 16, items + 64), ctx
        assert tts in (1, 2) and (tts == 1 or tts == tt), ctx
        common = nw * 9472 + tpw * nu * tt * 1024 + ((tpw + 3) & ~3) * 4      # waves' buffers | unit sums [tpw][nu][token tiles][256] | counters
        if k == "g6s":
            # MODE S: 16 tokens at most, eight waves, NV 16-byte units per thread hold the row; the activation [ng'][1024] + scales in LDS
            assert nb_ <= 16 and nw == 8 and p["tt"] == 1 and n <= 4096 and p["nv"] == (5 if n <= 2560 else 8) and p["nv"] * 512 >= n, ctx
            assert p["r"] in (1, 2, 4) and p["rounds"] <= p["r"] and (p["r"] == 1 or p["rounds"] > p["r"] // 2), ctx
            assert p["lds_bytes"] == common + nu * 8 * 1024 + 64 + nu * 8 * 64 + 64, ctx
        else:
            assert p["nv"] == 1 and p["tt"] == (1 if tts > 1 else tt), ctx
            assert p["r"] == p["rounds"] and 1 <= p["r"] <= (3 if p["tt"] == 4 else 4), ctx
            assert p["lds_bytes"] == common + 64, ctx
            # MODE S wherever it fits
            assert not (tt == 1 and nw == 8 and n <= 4096 and common + nu * 8 * 1088 + 128 <= LDS_MAX), ctx
    elif k == "g7":
        row_tiles(p, segs, sw, c)
        tpw, pp, nsa, nk = p["tpw"], p["pp"], p["nsa"], p["nk"]
        assert 17 <= nb_ <= 64 and nk == n // 256 and n % 256 == 0 and p["ttl"] == ttl and p["threads"] == 1024, ctx
        assert p["tp"] in (1, 2, 3, 5, 8) and tpw <= p["tp"] and (p["tp"] == 1 or tpw > {2: 1, 3: 2, 5: 3, 8: 5}[p["tp"]]), ctx
        assert pp in (1, 2) and tpw * ceil_div(ttl, pp) <= 14 and (pp == 1 or tpw * ttl > 14), ctx
        assert p["a_ws"] == tpw * 4096 and p["a_stage"] == p["a_ws"] + ceil_div(tpw, 4) * 1024, ctx
        assert p["b_xs"] == ceil_div(ttl, pp) * pp * 4096 and p["b_stage"] == p["b_xs"] + 1024, ctx
        assert 2 <= nsa <= min(32, nk + 1) and p["b_base"] == nsa * p["a_stage"] and p["lds_bytes"] == p["b_base"] + 2 * p["b_stage"] + 1024, ctx
        # a loader's DMA instructions in flight -- every second step is its own, 4 per tile + 1 per four tiles of scales -- fit vmcnt's 6 bits
        assert ((nsa - 1) // 2) * (4 * tpw + ceil_div(tpw, 4)) <= 63, ctx
        assert p["pre"] == min(nsa - 1, nk, 3), ctx
        assert tpw * ttl >= 8 or nk <= 4, ("where it pays", ctx)
    elif k == "g7k":
        hh, ks, nu, nl, ring = p["hh"], p["ks"], p["nu"], p["nl"], p["ring"]
        assert 3 <= nb_ <= 48 and len(rows) == 1 and not sw and p["ttl"] == ttl <= 3, ctx
        assert p["nk"] == n // 256 >= 8 and nu == ceil_div(p["nk"], 2), ctx
        assert 1 <= hh <= 8 and p["ntiles"] == p["grid"] == ceil_div(rows[0], 2 * hh) <= c and (hh == 1 or ceil_div(rows[0], 2 * hh - 2) > c), ctx
        assert 2 <= ks <= min(nu, 6) and p["ncw"] == ks * ttl <= 14 and p["nss"] == ceil_div(nu, ks), ctx
        assert nl == min(16 - p["ncw"], 6) and nl >= 2 and p["threads"] == (p["ncw"] + nl) * 64, ctx
        assert ring in (2, 3) and p["tab"] == ring * 2 * ks * 4352 and p["lds_bytes"] == p["tab"] + nu * ttl * 1024, ctx
        assert ring * ceil_div(2 * ks, nl) * 5 <= 60, ("vmcnt", ctx)
    elif k == "gc":
        assert gc_takes(gs, kind, n, rows, nb_), ctx
        assert p["ng"] == ng and p["nhc"] == ceil_div(ng, 8) and p["ntiles"] == ceil_div(rows[0], 16) and p["ttl"] == ttl and p["tt"] == tt, ctx
        assert p["waves"] in (4, 6, 8) and p["threads"] == 64 * p["waves"] and p["grid"] == c and p["nwaves"] == c * p["waves"], ctx
        assert p["lt"] == ttl or (p["lt"] == 2 and ttl <= 4), ctx
        assert p["lds_bytes"] == p["lt"] * ng * 1088 + p["waves"] * 8960 + 64, ctx       # staged tiles [lt][ng][1024 + 64] | the waves' buffers
        # as many waves as leave room for the staged tiles: two more would not fit with them
        assert p["waves"] == 8 or p["lt"] * ng * 1088 + (p["waves"] + 2) * 8960 + 256 > LDS_MAX, ctx
    else:
        assert k == "g2" and (p["gs"], p["sw"], p["tt"]) == (gs, int(sw), tt) and p["threads"] == 512, ctx
        assert not gc_takes(gs, kind, n, rows, nb_), ("GC comes first", ctx)
        assert p["ng"] == ng and p["npass"] == ceil_div(n, 512) and p["grid"] == ceil_div(total, 16), ctx
        assert sw or all(r % 16 == 0 for r in rows[:-1]), ctx
        assert p["magic"] == ((1 << 20) + ng - 1) // ng and magic_exact(ng, 20, 16 * ng + 4096), ctx
        assert p["lds_bytes"] == g2_lds(gs, n, sw, tt), ctx
    return p


def test_named_shapes_full_cross():
    seen = 0
    for gs in GSS:
        for n in (n for n in NAMED_N if n % gs == 0):
            for i, r in enumerate(ROWS):
                for nb_ in TOKENS:
                    ordered = bool((i + nb_) & 1)
                    for cus in ((256,) if nb_ % 3 else (256, 64, 0, 304)):
                        for segs in segment_sets(i):
                            check(gs, 0, n, segs, nb_, ordered, cus=cus); seen += 1
                            check(gs, 1, n, segs, nb_, not ordered, cus=cus); seen += 1
                        check(gs, 2, n, (r, r), nb_, ordered, cus=cus); seen += 1
                    check(gs, 0, n, segment_sets(i)[2], nb_, False, use_gemm=True); seen += 1
                    check(gs, 1, n, (r,), nb_, True, use_gemm=True); seen += 1
                    if nb_ <= 8:
                        check(gs, 1, n, (r,), nb_, False, attn=heads_of(n), use_gemm=True); seen += 1
    assert seen > 80000
    DONE.add("named")


def test_every_row_length():
    """every multiple of 16 and of the group size up to 20480, the other axes rotating"""
    launches = 0
    for gs in GSS:
        for j, n in enumerate(range(gs, 20481, gs)):
            if n % 16:
                continue
            r = ROWS[j % len(ROWS)]
            for nb_ in TOKENS:
                kind = (j + nb_) % 3
                ordered = bool((j // 3 + nb_) & 1)
                rows = segment_sets(j + nb_)[(j // 3) % 3] if kind == 0 else (r,) if kind == 1 else (r, r)
                launches += check(gs, kind, n, rows, nb_, ordered)["kernel"] != 0
    assert launches > 5000
    DONE.add("lengths")


def test_tall_and_many_tiled_shapes():
    """the classifier's kernel on every row length it takes, and the launches with 4..8 row tiles per workgroup (20000..65000 rows)"""
    for n in range(256, 8192 + 512, 256):
        for nb_ in TOKENS:
            for rows in (16384, 16391, 151936):
                p = check(64, 0, n, (rows,), nb_, bool(nb_ & 1))
                batched = nb_ >= 9 or p["kernel"] != 0          # (8 sequences on a heavy matrix: check() holds the router's rule)
                want = "none" if not batched else "gc" if gc_takes(64, 0, n, (rows,), nb_) else "g2"
                assert nb.Q80_GEMM_KERNELS[p["kernel"]] == want, (n, nb_, rows, p)
    for n in (256, 512, 768, 1024, 1280, 2048, 2560, 2816, 4096):
        for segs in [(r,) for r in range(4100, 65000, 2050)] + [(4112, 16, 8), (4112, 1024, 1000), (8208, 16, 8), (8192, 8192, 8192), (8208, 8192, 4100),
                                                                 (16000, 16000, 16000), (30000, 30016)]:
            for nb_ in (3, 8, 9, 16, 17, 32, 33, 48, 49, 64):
                check(64, 0, n, segs, nb_, use_gemm=True)
                check(64, 1, n, segs, nb_, use_gemm=True)
                if segs[0] <= 16400:
                    check(64, 2, n, (segs[0], segs[0]), nb_, use_gemm=True)
    DONE.add("tall")


def test_model_shapes_every_token_count():
    """the projections of Qwen3-0.6B, Qwen3-4B and the tiny presets (the keys of PINS below) at 1..64 tokens"""
    for gs, kind, n, rows in PINS:
        for nb_ in range(1, 65):
            for cus in ((256,) if nb_ % 5 else (256, 64, 0, 304)):
                for ordered in (False, True):
                    check(gs, kind, n, rows, nb_, ordered, cus=cus)
                    check(gs, kind, n, rows, nb_, ordered, cus=cus, use_gemm=True)
    DONE.add("models")


# What the sweeps above reach of the template space at the device's 256 CUs, as (kernel, template values) -- G6 MODE S (NV, R, MS), MODE F
# (R, MS, TT), G7 (TP, PP, MS), G7K (), GC (TT), G2 (GS, SW, TT); tests/test_gpu_q80_gemm.py runs a case for every one.  Of what the launch
# ladders instantiate the planner reaches everything but G7 at one to three row tiles per workgroup with two token tiles per wave (PP = 2
# is the answer to more than 14 (row tile, token tile) pairs: at least four row tiles), and of G2's 24 tuples those of SECTION3_FROM
# that never fit (group size 32 with SwiGLU beyond one token tile).  G6 MODE F at four rounds of four token tiles is not instantiated.
UNIVERSE = {("g2", gs, sw, tt) for gs in GSS for sw in (0, 1) for tt in (1, 2, 4) if not (gs == 32 and sw and tt > 1)} | \
    {("g6f", r, ms, tt) for r in (1, 2, 3, 4) for ms in (0, 1) for tt in (1, 2, 4) if not (r == 4 and tt == 4)} | \
    {("g6s", nv, r, ms) for nv in (5, 8) for r in (1, 2, 4) for ms in (0, 1)} | \
    {("g7", tp, pp, ms) for tp in (1, 2, 3, 5, 8) for pp in (1, 2) for ms in (0, 1) if not (pp == 2 and tp <= 3)} | \
    {("g7k",), ("gc", 1), ("gc", 2), ("gc", 4)}


def test_universe_is_what_the_sweeps_reach():
    for name, sweep in (("named", test_named_shapes_full_cross), ("lengths", test_every_row_length), ("tall", test_tall_and_many_tiled_shapes),
                        ("models", test_model_shapes_every_token_count)):
        if name not in DONE:
            sweep()
    print(sorted(SEEN))
    assert SEEN == UNIVERSE, (sorted(SEEN - UNIVERSE), sorted(UNIVERSE - SEEN))


# Launches the parent commit routed to G2 whose launcher then returned hipErrorInvalidValue -- after the activation quantizer launch had
# gone out -- because its two weight stages, weight scales and product tables ask for more than a CU's 163840 bytes of LDS (g2_lds()).
# SECTION3_FROM: (group size, SwiGLU, TT) -> the first row length that does not fit; every class not listed fits up to the 65536 values
# (SwiGLU: 32768) the GEMV kernels take.  Group size 32 with SwiGLU at 17..64 tokens never fits (two matrices x 16 groups of a pass x 16
# rows x 33 | 65 tokens); the other classes grow with the weight scales [matrices][16][ng | 1].
# gemm_q80_plan() refuses them; they run through the GEMV kernels in slices that fit (up to 8 sequences in one launch).  No GC shape has
# the property (its two late exits are unreachable behind its shape checks: the sweep over every row length it takes finds none).
SECTION3_FROM = {(32, 0, 1): 56064, (32, 0, 2): 39680, (32, 0, 4): 6912, (32, 1, 1): 15104, (32, 1, 2): 32, (32, 1, 4): 32,
                 (64, 1, 1): 47616, (64, 1, 2): 31232, (64, 1, 4): 31744}
SECTION3 = [(2, 256, (64, 64), 64), (0, 8192, (32,), 64), (2, 256, (768, 768), 17), (2, 128, (384, 384), 49), (2, 192, (352, 352), 64),
            (2, 2560, (9728, 9728), 33), (1, 9728, (2560,), 33), (1, 6912, (16,), 48), (0, 20480, (4, 4, 12), 64), (2, 15136, (16, 16), 9)]


@pytest.mark.parametrize("kind,n,rows,nb_", SECTION3)
def test_section3_shapes_are_refused_and_sliced(kind, n, rows, nb_):
    for ordered in (False, True):
        p = check(32, kind, n, rows, nb_, ordered)
        assert nb.ROUTE_NAMES[p["route"]] == "gemv_sliced" and p["kernel"] == 0, p
        assert g2_lds(32, n, kind == 2, 1 if nb_ <= 16 else 2 if nb_ <= 32 else 4) > LDS_MAX
        q = nb.q80_gemv_plan(kind, n, rows, nb_, gs=32, ordered=ordered)                 # ... and the slices are launches the GEMV kernels take
        assert q["takes"] == 1 and nb.ROUTE_NAMES[q["route"]] == "gemv_sliced" and q["launches"] * q["seqs_per_launch"] >= nb_ and q["lds_bytes"] <= LDS_MAX, q


def test_section3_neighbours_keep_the_matrix_cores():
    """one token tile fewer, the next group size, a row just short of the limit"""
    assert g2_lds(32, 256, True, 4) == 166912 + 2 * 16 * 9 * 4                # (the issue's figure + the weight scales)
    assert g2_lds(32, 256, True, 1) <= LDS_MAX and check(32, 2, 256, (64, 64), 16)["kernel"] == KERN["g2"]
    assert check(64, 2, 256, (64, 64), 64, True)["kernel"] == KERN["g2"] and check(128, 2, 256, (64, 64), 64)["kernel"] == KERN["g2"]
    assert g2_lds(32, 6848, False, 4) <= LDS_MAX < g2_lds(32, 6912, False, 4) and check(32, 1, 6848, (16,), 64)["kernel"] == KERN["g2"]
    assert check(32, 0, 8192, (32,), 32)["kernel"] == KERN["g2"]
    for gs in GSS:
        for sw in (0, 1):
            for tt in (1, 2, 4):
                first = next((n for n in range(gs, 65536 + 1, gs) if n % 16 == 0 and g2_lds(gs, n, sw, tt) > LDS_MAX), None)
                assert SECTION3_FROM.get((gs, sw, tt)) == first, (gs, sw, tt, first)
    for (gs, sw, tt), n in SECTION3_FROM.items():
        if n <= (32768 if sw else 65536):
            assert check(gs, 2 if sw else 1, n, (16, 16) if sw else (16,), 16 * tt, True)["kernel"] == 0


def test_documented_refusals():
    Q = lambda *a, **k: nb.Q80_GEMM_KERNELS[check(*a, **k)["kernel"]]
    # interior tensors in multiples of G2's 16-row tile (the last one may be ragged); the canonical kernels cut their tiles at tensor ends
    assert Q(32, 0, 256, (32, 16, 7), 9) == "g2" and Q(32, 0, 256, (32, 8, 16), 9) == "none" and Q(64, 0, 256, (32, 8, 16), 9) == "g6f"
    assert Q(64, 0, 256, (32, 8, 16), 9, True) == "none"
    # one group per row: G2's magic division overflows 32 bits inside its index range
    assert Q(32, 0, 32, (64,), 9) == "none" and Q(32, 0, 64, (64,), 9) == "g2"
    # canonical launches: 65536 rows, a tensor of 4 GiB - 1 MiB, and what fits neither G6 nor G7 (9..16 tokens: G7 does not start before 17)
    assert Q(64, 0, 256, (32768, 32768), 16) == "none" and Q(64, 0, 256, (32768, 32752), 16) != "none"
    assert Q(64, 1, 65536, (65535,), 9) == "none"
    assert Q(64, 2, 16384, (9728, 9728), 16) == "none" and Q(64, 2, 16384, (9728, 9728), 17) == "g7"
    # split-attention partials never reach a batched kernel
    assert Q(64, 1, 2048, (1024,), 8, attn=heads_of(2048), use_gemm=True) == "none" and Q(64, 1, 2048, (1024,), 8, use_gemm=True) == "g7k"
    # a malformed descriptor is an error, not a plan
    for bad in (dict(kind=3, n=256, rows=(4,)), dict(kind=0, n=264, rows=(4,)), dict(kind=0, n=256, rows=(4,), gs=48), dict(kind=2, n=256, rows=(4, 8)),
                dict(kind=0, n=256, rows=(4,), nb=65)):
        with pytest.raises(nb.NanoHipError):
            nb.q80_gemm_plan(**bad)


# The plans of every per-layer projection and the classifier of Qwen3-0.6B and Qwen3-4B and of the tiny presets at 256 CUs, as
# "kernel tt,nv,r,ms,tp,pp,gs,sw grid*threads lds_bytes o<norm_order>" or the GEMV route's name -- the answers of the parent commit's
# route_kind(), *_supports(), g6_plan() / g7_plan() / g7k_plan() and launcher arithmetic (compiled from that commit, not from the code
# under test): the launches of models that ran before must not move.  S3: the parent's launcher returned an error (SECTION3).
S3 = "gemv_sliced"
PIN_TOKENS_MODELS = (3, 8, 9, 16, 17, 32, 33, 48, 49, 64)
PIN_TOKENS_TINY = (9, 16, 17, 49, 64)
# (group size, kind, n, rows) -> [fast path, strict mode] x token counts
PINS = {
    # Qwen3-0.6B, group size 64
    (64, 0, 1024, (2048, 1024, 1024)): [
        ['gemv', 'gemv', 'g6f 1,1,1,1,0,0,0,0 256*128 21072 o256', 'g6f 1,1,1,1,0,0,0,0 256*128 21072 o256', 'g7 0,0,0,1,1,1,0,0 256*1024 45056 o256', 'g7 0,0,0,1,1,1,0,0 256*1024 45056 o256', 'g7 0,0,0,1,1,1,0,0 256*1024 53248 o256', 'g7 0,0,0,1,1,1,0,0 256*1024 53248 o256', 'g7 0,0,0,1,1,1,0,0 256*1024 61440 o256', 'g7 0,0,0,1,1,1,0,0 256*1024 61440 o256'],
        ['gemv', 'gemv', 'g2 1,0,0,0,0,0,64,0 256*512 35392 o256', 'g2 1,0,0,0,0,0,64,0 256*512 35392 o256', 'g2 2,0,0,0,0,0,64,0 256*512 51776 o256', 'g2 2,0,0,0,0,0,64,0 256*512 51776 o256', 'g2 4,0,0,0,0,0,64,0 256*512 84544 o256', 'g2 4,0,0,0,0,0,64,0 256*512 84544 o256', 'g2 4,0,0,0,0,0,64,0 256*512 84544 o256', 'g2 4,0,0,0,0,0,64,0 256*512 84544 o256'],
    ],
    (64, 1, 2048, (1024,)): [
        ['gemv', 'gemv', 'g7k 0,0,0,0,0,0,0,0 256*640 108544 o256', 'g7k 0,0,0,0,0,0,0,0 256*640 108544 o256', 'g7k 0,0,0,0,0,0,0,0 256*896 112640 o256', 'g7k 0,0,0,0,0,0,0,0 256*896 112640 o256', 'g7k 0,0,0,0,0,0,0,0 256*1024 116736 o256', 'g7k 0,0,0,0,0,0,0,0 256*1024 116736 o256', 'g6f 4,1,1,0,0,0,0,0 256*256 54352 o256', 'g6f 4,1,1,0,0,0,0,0 256*256 54352 o256'],
        ['gemv', 'gemv', 'g2 1,0,0,0,0,0,64,0 64*512 36416 o256', 'g2 1,0,0,0,0,0,64,0 64*512 36416 o256', 'g2 2,0,0,0,0,0,64,0 64*512 52800 o256', 'g2 2,0,0,0,0,0,64,0 64*512 52800 o256', 'g2 4,0,0,0,0,0,64,0 64*512 85568 o256', 'g2 4,0,0,0,0,0,64,0 64*512 85568 o256', 'g2 4,0,0,0,0,0,64,0 64*512 85568 o256', 'g2 4,0,0,0,0,0,64,0 64*512 85568 o256'],
    ],
    (64, 2, 1024, (3072, 3072)): [
        ['gemv', 'gemv', 'g6f 1,1,1,0,0,0,0,0 256*256 42064 o256', 'g6f 1,1,1,0,0,0,0,0 256*256 42064 o256', 'g7 0,0,0,0,2,1,0,0 256*1024 65536 o256', 'g7 0,0,0,0,2,1,0,0 256*1024 65536 o256', 'g7 0,0,0,0,2,1,0,0 256*1024 73728 o256', 'g7 0,0,0,0,2,1,0,0 256*1024 73728 o256', 'g7 0,0,0,0,2,1,0,0 256*1024 81920 o256', 'g7 0,0,0,0,2,1,0,0 256*1024 81920 o256'],
        ['gemv', 'gemv', 'g2 1,0,0,0,0,0,64,1 192*512 70784 o256', 'g2 1,0,0,0,0,0,64,1 192*512 70784 o256', 'g2 2,0,0,0,0,0,64,1 192*512 103552 o256', 'g2 2,0,0,0,0,0,64,1 192*512 103552 o256', 'g2 4,0,0,0,0,0,64,1 192*512 102528 o256', 'g2 4,0,0,0,0,0,64,1 192*512 102528 o256', 'g2 4,0,0,0,0,0,64,1 192*512 102528 o256', 'g2 4,0,0,0,0,0,64,1 192*512 102528 o256'],
    ],
    (64, 1, 3072, (1024,)): [
        ['gemv', 'gemv', 'g7k 0,0,0,0,0,0,0,0 256*768 162816 o256', 'g7k 0,0,0,0,0,0,0,0 256*768 162816 o256', 'g7k 0,0,0,0,0,0,0,0 256*1024 142848 o256', 'g7k 0,0,0,0,0,0,0,0 256*1024 142848 o256', 'g7k 0,0,0,0,0,0,0,0 256*1024 122880 o256', 'g7k 0,0,0,0,0,0,0,0 256*1024 122880 o256', 'g6f 4,1,2,0,0,0,0,0 256*256 62544 o256', 'g6f 4,1,2,0,0,0,0,0 256*256 62544 o256'],
        ['gemv', 'gemv', 'g2 1,0,0,0,0,0,64,0 64*512 37440 o256', 'g2 1,0,0,0,0,0,64,0 64*512 37440 o256', 'g2 2,0,0,0,0,0,64,0 64*512 53824 o256', 'g2 2,0,0,0,0,0,64,0 64*512 53824 o256', 'g2 4,0,0,0,0,0,64,0 64*512 86592 o256', 'g2 4,0,0,0,0,0,64,0 64*512 86592 o256', 'g2 4,0,0,0,0,0,64,0 64*512 86592 o256', 'g2 4,0,0,0,0,0,64,0 64*512 86592 o256'],
    ],
    (64, 0, 1024, (151936,)): [
        ['gemv_preq', 'gc 1,0,0,0,0,0,0,0 256*512 89152 o256', 'gc 1,0,0,0,0,0,0,0 256*512 89152 o256', 'gc 1,0,0,0,0,0,0,0 256*512 89152 o256', 'gc 2,0,0,0,0,0,0,0 256*512 106560 o256', 'gc 2,0,0,0,0,0,0,0 256*512 106560 o256', 'gc 4,0,0,0,0,0,0,0 256*512 123968 o256', 'gc 4,0,0,0,0,0,0,0 256*512 123968 o256', 'gc 4,0,0,0,0,0,0,0 256*512 141376 o256', 'gc 4,0,0,0,0,0,0,0 256*512 141376 o256'],
        ['gemv_preq', 'gc 1,0,0,0,0,0,0,0 256*512 89152 o256', 'gc 1,0,0,0,0,0,0,0 256*512 89152 o256', 'gc 1,0,0,0,0,0,0,0 256*512 89152 o256', 'gc 2,0,0,0,0,0,0,0 256*512 106560 o256', 'gc 2,0,0,0,0,0,0,0 256*512 106560 o256', 'gc 4,0,0,0,0,0,0,0 256*512 123968 o256', 'gc 4,0,0,0,0,0,0,0 256*512 123968 o256', 'gc 4,0,0,0,0,0,0,0 256*512 141376 o256', 'gc 4,0,0,0,0,0,0,0 256*512 141376 o256'],
    ],
    # Qwen3-4B, group size 64
    (64, 0, 2560, (4096, 1024, 1024)): [
        ['g6s 1,5,2,1,0,0,0,0 256*512 134800 o512', 'g6s 1,5,2,1,0,0,0,0 256*512 134800 o512', 'g6s 1,5,2,1,0,0,0,0 256*512 134800 o512', 'g6s 1,5,2,1,0,0,0,0 256*512 134800 o512', 'g6f 2,1,2,1,0,0,0,0 256*512 106576 o512', 'g6f 2,1,2,1,0,0,0,0 256*512 106576 o512', 'g6f 4,1,2,1,0,0,0,0 256*512 137296 o512', 'g6f 4,1,2,1,0,0,0,0 256*512 137296 o512', 'g7 0,0,0,1,2,1,0,0 256*1024 137216 o512', 'g7 0,0,0,1,2,1,0,0 256*1024 137216 o512'],
        ['g2 1,0,0,0,0,0,64,0 384*512 36928 o256', 'g2 1,0,0,0,0,0,64,0 384*512 36928 o256', 'g2 1,0,0,0,0,0,64,0 384*512 36928 o256', 'g2 1,0,0,0,0,0,64,0 384*512 36928 o256', 'g2 2,0,0,0,0,0,64,0 384*512 53312 o256', 'g2 2,0,0,0,0,0,64,0 384*512 53312 o256', 'g2 4,0,0,0,0,0,64,0 384*512 86080 o256', 'g2 4,0,0,0,0,0,64,0 384*512 86080 o256', 'g2 4,0,0,0,0,0,64,0 384*512 86080 o256', 'g2 4,0,0,0,0,0,64,0 384*512 86080 o256'],
    ],
    (64, 1, 4096, (2560,)): [
        ['g7k 0,0,0,0,0,0,0,0 256*704 138752 o512', 'g7k 0,0,0,0,0,0,0,0 256*704 138752 o512', 'g7k 0,0,0,0,0,0,0,0 256*704 138752 o512', 'g7k 0,0,0,0,0,0,0,0 256*704 138752 o512', 'g7k 0,0,0,0,0,0,0,0 256*1024 146944 o512', 'g7k 0,0,0,0,0,0,0,0 256*1024 146944 o512', 'g7k 0,0,0,0,0,0,0,0 256*1024 129024 o512', 'g7k 0,0,0,0,0,0,0,0 256*1024 129024 o512', 'g6f 4,1,1,0,0,0,0,0 256*512 108624 o512', 'g6f 4,1,1,0,0,0,0,0 256*512 108624 o512'],
        ['g2 1,0,0,0,0,0,64,0 160*512 38464 o256', 'g2 1,0,0,0,0,0,64,0 160*512 38464 o256', 'g2 1,0,0,0,0,0,64,0 160*512 38464 o256', 'g2 1,0,0,0,0,0,64,0 160*512 38464 o256', 'g2 2,0,0,0,0,0,64,0 160*512 54848 o256', 'g2 2,0,0,0,0,0,64,0 160*512 54848 o256', 'g2 4,0,0,0,0,0,64,0 160*512 87616 o256', 'g2 4,0,0,0,0,0,64,0 160*512 87616 o256', 'g2 4,0,0,0,0,0,64,0 160*512 87616 o256', 'g2 4,0,0,0,0,0,64,0 160*512 87616 o256'],
    ],
    (64, 2, 2560, (9728, 9728)): [
        ['g6s 1,5,4,0,0,0,0,0 256*512 145056 o512', 'g6s 1,5,4,0,0,0,0,0 256*512 145056 o512', 'g6s 1,5,4,0,0,0,0,0 256*512 145056 o512', 'g6s 1,5,4,0,0,0,0,0 256*512 145056 o512', 'g7 0,0,0,0,5,1,0,0 256*1024 132096 o512', 'g7 0,0,0,0,5,1,0,0 256*1024 132096 o512', 'g7 0,0,0,0,5,2,0,0 256*1024 148480 o512', 'g7 0,0,0,0,5,2,0,0 256*1024 148480 o512', 'g7 0,0,0,0,5,2,0,0 256*1024 148480 o512', 'g7 0,0,0,0,5,2,0,0 256*1024 148480 o512'],
        ['g2 1,0,0,0,0,0,64,1 608*512 73856 o256', 'g2 1,0,0,0,0,0,64,1 608*512 73856 o256', 'g2 1,0,0,0,0,0,64,1 608*512 73856 o256', 'g2 1,0,0,0,0,0,64,1 608*512 73856 o256', 'g2 2,0,0,0,0,0,64,1 608*512 106624 o256', 'g2 2,0,0,0,0,0,64,1 608*512 106624 o256', 'g2 4,0,0,0,0,0,64,1 608*512 105600 o256', 'g2 4,0,0,0,0,0,64,1 608*512 105600 o256', 'g2 4,0,0,0,0,0,64,1 608*512 105600 o256', 'g2 4,0,0,0,0,0,64,1 608*512 105600 o256'],
    ],
    (64, 1, 9728, (2560,)): [
        ['g7k 0,0,0,0,0,0,0,0 256*704 150016 o512', 'g7k 0,0,0,0,0,0,0,0 256*704 150016 o512', 'g7k 0,0,0,0,0,0,0,0 256*704 150016 o512', 'g7k 0,0,0,0,0,0,0,0 256*704 150016 o512', 'g7k 0,0,0,0,0,0,0,0 256*896 143360 o512', 'g7k 0,0,0,0,0,0,0,0 256*896 143360 o512', 'g7k 0,0,0,0,0,0,0,0 256*1024 162816 o512', 'g7k 0,0,0,0,0,0,0,0 256*1024 162816 o512', 'g6f 4,1,3,0,0,0,0,0 256*512 153680 o512', 'g6f 4,1,3,0,0,0,0,0 256*512 153680 o512'],
        ['g2 1,0,0,0,0,0,64,0 160*512 44096 o256', 'g2 1,0,0,0,0,0,64,0 160*512 44096 o256', 'g2 1,0,0,0,0,0,64,0 160*512 44096 o256', 'g2 1,0,0,0,0,0,64,0 160*512 44096 o256', 'g2 2,0,0,0,0,0,64,0 160*512 60480 o256', 'g2 2,0,0,0,0,0,64,0 160*512 60480 o256', 'g2 4,0,0,0,0,0,64,0 160*512 93248 o256', 'g2 4,0,0,0,0,0,64,0 160*512 93248 o256', 'g2 4,0,0,0,0,0,64,0 160*512 93248 o256', 'g2 4,0,0,0,0,0,64,0 160*512 93248 o256'],
    ],
    (64, 0, 2560, (151936,)): [
        ['gemv_preq', 'gc 1,0,0,0,0,0,0,0 256*512 115264 o256', 'gc 1,0,0,0,0,0,0,0 256*512 115264 o256', 'gc 1,0,0,0,0,0,0,0 256*512 115264 o256', 'gc 2,0,0,0,0,0,0,0 256*512 158784 o256', 'gc 2,0,0,0,0,0,0,0 256*512 158784 o256', 'gc 4,0,0,0,0,0,0,0 256*512 158784 o256', 'gc 4,0,0,0,0,0,0,0 256*512 158784 o256', 'gc 4,0,0,0,0,0,0,0 256*512 158784 o256', 'gc 4,0,0,0,0,0,0,0 256*512 158784 o256'],
        ['gemv_preq', 'gc 1,0,0,0,0,0,0,0 256*512 115264 o256', 'gc 1,0,0,0,0,0,0,0 256*512 115264 o256', 'gc 1,0,0,0,0,0,0,0 256*512 115264 o256', 'gc 2,0,0,0,0,0,0,0 256*512 158784 o256', 'gc 2,0,0,0,0,0,0,0 256*512 158784 o256', 'gc 4,0,0,0,0,0,0,0 256*512 158784 o256', 'gc 4,0,0,0,0,0,0,0 256*512 158784 o256', 'gc 4,0,0,0,0,0,0,0 256*512 158784 o256', 'gc 4,0,0,0,0,0,0,0 256*512 158784 o256'],
    ],
    # tiny-qwen3, group size 32
    (32, 0, 256, (256, 128, 128)): [
        ['g2 1,0,0,0,0,0,32,0 32*512 52288 o256', 'g2 1,0,0,0,0,0,32,0 32*512 52288 o256', 'g2 2,0,0,0,0,0,32,0 32*512 85056 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150592 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150592 o256'],
        ['g2 1,0,0,0,0,0,32,0 32*512 52288 o256', 'g2 1,0,0,0,0,0,32,0 32*512 52288 o256', 'g2 2,0,0,0,0,0,32,0 32*512 85056 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150592 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150592 o256'],
    ],
    (32, 1, 256, (256,)): [
        ['g2 1,0,0,0,0,0,32,0 16*512 52288 o256', 'g2 1,0,0,0,0,0,32,0 16*512 52288 o256', 'g2 2,0,0,0,0,0,32,0 16*512 85056 o256', 'g2 4,0,0,0,0,0,32,0 16*512 150592 o256', 'g2 4,0,0,0,0,0,32,0 16*512 150592 o256'],
        ['g2 1,0,0,0,0,0,32,0 16*512 52288 o256', 'g2 1,0,0,0,0,0,32,0 16*512 52288 o256', 'g2 2,0,0,0,0,0,32,0 16*512 85056 o256', 'g2 4,0,0,0,0,0,32,0 16*512 150592 o256', 'g2 4,0,0,0,0,0,32,0 16*512 150592 o256'],
    ],
    (32, 2, 256, (768, 768)): [
        ['g2 1,0,0,0,0,0,32,1 48*512 104576 o256', 'g2 1,0,0,0,0,0,32,1 48*512 104576 o256', S3, S3, S3],
        ['g2 1,0,0,0,0,0,32,1 48*512 104576 o256', 'g2 1,0,0,0,0,0,32,1 48*512 104576 o256', S3, S3, S3],
    ],
    (32, 1, 768, (256,)): [
        ['g2 1,0,0,0,0,0,32,0 16*512 53312 o256', 'g2 1,0,0,0,0,0,32,0 16*512 53312 o256', 'g2 2,0,0,0,0,0,32,0 16*512 86080 o256', 'g2 4,0,0,0,0,0,32,0 16*512 151616 o256', 'g2 4,0,0,0,0,0,32,0 16*512 151616 o256'],
        ['g2 1,0,0,0,0,0,32,0 16*512 53312 o256', 'g2 1,0,0,0,0,0,32,0 16*512 53312 o256', 'g2 2,0,0,0,0,0,32,0 16*512 86080 o256', 'g2 4,0,0,0,0,0,32,0 16*512 151616 o256', 'g2 4,0,0,0,0,0,32,0 16*512 151616 o256'],
    ],
    (32, 0, 256, (1024,)): [
        ['g2 1,0,0,0,0,0,32,0 64*512 52288 o256', 'g2 1,0,0,0,0,0,32,0 64*512 52288 o256', 'g2 2,0,0,0,0,0,32,0 64*512 85056 o256', 'g2 4,0,0,0,0,0,32,0 64*512 150592 o256', 'g2 4,0,0,0,0,0,32,0 64*512 150592 o256'],
        ['g2 1,0,0,0,0,0,32,0 64*512 52288 o256', 'g2 1,0,0,0,0,0,32,0 64*512 52288 o256', 'g2 2,0,0,0,0,0,32,0 64*512 85056 o256', 'g2 4,0,0,0,0,0,32,0 64*512 150592 o256', 'g2 4,0,0,0,0,0,32,0 64*512 150592 o256'],
    ],
    # tiny-qwen3, group size 64
    (64, 0, 256, (256, 128, 128)): [
        ['g6f 1,1,1,1,0,0,0,0 256*64 10576 o256', 'g6f 1,1,1,1,0,0,0,0 256*64 10576 o256', 'g7 0,0,0,1,1,1,0,0 52*1024 29696 o256', 'g7 0,0,0,1,1,1,0,0 32*1024 46080 o256', 'g7 0,0,0,1,1,1,0,0 32*1024 46080 o256'],
        ['g2 1,0,0,0,0,0,64,0 32*512 34624 o256', 'g2 1,0,0,0,0,0,64,0 32*512 34624 o256', 'g2 2,0,0,0,0,0,64,0 32*512 51008 o256', 'g2 4,0,0,0,0,0,64,0 32*512 83776 o256', 'g2 4,0,0,0,0,0,64,0 32*512 83776 o256'],
    ],
    (64, 1, 256, (256,)): [
        ['g6f 1,1,1,0,0,0,0,0 128*64 10576 o256', 'g6f 1,1,1,0,0,0,0,0 128*64 10576 o256', 'g7 0,0,0,0,1,1,0,0 26*1024 29696 o256', 'g7 0,0,0,0,1,1,0,0 16*1024 46080 o256', 'g7 0,0,0,0,1,1,0,0 16*1024 46080 o256'],
        ['g2 1,0,0,0,0,0,64,0 16*512 34624 o256', 'g2 1,0,0,0,0,0,64,0 16*512 34624 o256', 'g2 2,0,0,0,0,0,64,0 16*512 51008 o256', 'g2 4,0,0,0,0,0,64,0 16*512 83776 o256', 'g2 4,0,0,0,0,0,64,0 16*512 83776 o256'],
    ],
    (64, 2, 256, (768, 768)): [
        ['g6f 1,1,1,0,0,0,0,0 256*64 10576 o256', 'g6f 1,1,1,0,0,0,0,0 256*64 10576 o256', 'g7 0,0,0,0,1,1,0,0 154*1024 29696 o256', 'g7 0,0,0,0,1,1,0,0 96*1024 46080 o256', 'g7 0,0,0,0,1,1,0,0 96*1024 46080 o256'],
        ['g2 1,0,0,0,0,0,64,1 48*512 69248 o256', 'g2 1,0,0,0,0,0,64,1 48*512 69248 o256', 'g2 2,0,0,0,0,0,64,1 48*512 102016 o256', 'g2 4,0,0,0,0,0,64,1 48*512 100992 o256', 'g2 4,0,0,0,0,0,64,1 48*512 100992 o256'],
    ],
    (64, 1, 768, (256,)): [
        ['g6f 1,1,1,0,0,0,0,0 128*128 21072 o256', 'g6f 1,1,1,0,0,0,0,0 128*128 21072 o256', 'g7 0,0,0,0,1,1,0,0 26*1024 39936 o256', 'g7 0,0,0,0,1,1,0,0 16*1024 56320 o256', 'g7 0,0,0,0,1,1,0,0 16*1024 56320 o256'],
        ['g2 1,0,0,0,0,0,64,0 16*512 35136 o256', 'g2 1,0,0,0,0,0,64,0 16*512 35136 o256', 'g2 2,0,0,0,0,0,64,0 16*512 51520 o256', 'g2 4,0,0,0,0,0,64,0 16*512 84288 o256', 'g2 4,0,0,0,0,0,64,0 16*512 84288 o256'],
    ],
    (64, 0, 256, (1024,)): [
        ['g6f 1,1,1,0,0,0,0,0 256*64 10576 o256', 'g6f 1,1,1,0,0,0,0,0 256*64 10576 o256', 'g7 0,0,0,0,1,1,0,0 103*1024 29696 o256', 'g7 0,0,0,0,1,1,0,0 64*1024 46080 o256', 'g7 0,0,0,0,1,1,0,0 64*1024 46080 o256'],
        ['g2 1,0,0,0,0,0,64,0 64*512 34624 o256', 'g2 1,0,0,0,0,0,64,0 64*512 34624 o256', 'g2 2,0,0,0,0,0,64,0 64*512 51008 o256', 'g2 4,0,0,0,0,0,64,0 64*512 83776 o256', 'g2 4,0,0,0,0,0,64,0 64*512 83776 o256'],
    ],
    # tiny-qwen3, group size 128
    (128, 0, 256, (256, 128, 128)): [
        ['g2 1,0,0,0,0,0,128,0 32*512 25792 o256', 'g2 1,0,0,0,0,0,128,0 32*512 25792 o256', 'g2 2,0,0,0,0,0,128,0 32*512 33984 o256', 'g2 4,0,0,0,0,0,128,0 32*512 50368 o256', 'g2 4,0,0,0,0,0,128,0 32*512 50368 o256'],
        ['g2 1,0,0,0,0,0,128,0 32*512 25792 o256', 'g2 1,0,0,0,0,0,128,0 32*512 25792 o256', 'g2 2,0,0,0,0,0,128,0 32*512 33984 o256', 'g2 4,0,0,0,0,0,128,0 32*512 50368 o256', 'g2 4,0,0,0,0,0,128,0 32*512 50368 o256'],
    ],
    (128, 1, 256, (256,)): [
        ['g2 1,0,0,0,0,0,128,0 16*512 25792 o256', 'g2 1,0,0,0,0,0,128,0 16*512 25792 o256', 'g2 2,0,0,0,0,0,128,0 16*512 33984 o256', 'g2 4,0,0,0,0,0,128,0 16*512 50368 o256', 'g2 4,0,0,0,0,0,128,0 16*512 50368 o256'],
        ['g2 1,0,0,0,0,0,128,0 16*512 25792 o256', 'g2 1,0,0,0,0,0,128,0 16*512 25792 o256', 'g2 2,0,0,0,0,0,128,0 16*512 33984 o256', 'g2 4,0,0,0,0,0,128,0 16*512 50368 o256', 'g2 4,0,0,0,0,0,128,0 16*512 50368 o256'],
    ],
    (128, 2, 256, (768, 768)): [
        ['g2 1,0,0,0,0,0,128,1 48*512 51584 o256', 'g2 1,0,0,0,0,0,128,1 48*512 51584 o256', 'g2 2,0,0,0,0,0,128,1 48*512 67968 o256', 'g2 4,0,0,0,0,0,128,1 48*512 67456 o256', 'g2 4,0,0,0,0,0,128,1 48*512 67456 o256'],
        ['g2 1,0,0,0,0,0,128,1 48*512 51584 o256', 'g2 1,0,0,0,0,0,128,1 48*512 51584 o256', 'g2 2,0,0,0,0,0,128,1 48*512 67968 o256', 'g2 4,0,0,0,0,0,128,1 48*512 67456 o256', 'g2 4,0,0,0,0,0,128,1 48*512 67456 o256'],
    ],
    (128, 1, 768, (256,)): [
        ['g2 1,0,0,0,0,0,128,0 16*512 26048 o256', 'g2 1,0,0,0,0,0,128,0 16*512 26048 o256', 'g2 2,0,0,0,0,0,128,0 16*512 34240 o256', 'g2 4,0,0,0,0,0,128,0 16*512 50624 o256', 'g2 4,0,0,0,0,0,128,0 16*512 50624 o256'],
        ['g2 1,0,0,0,0,0,128,0 16*512 26048 o256', 'g2 1,0,0,0,0,0,128,0 16*512 26048 o256', 'g2 2,0,0,0,0,0,128,0 16*512 34240 o256', 'g2 4,0,0,0,0,0,128,0 16*512 50624 o256', 'g2 4,0,0,0,0,0,128,0 16*512 50624 o256'],
    ],
    (128, 0, 256, (1024,)): [
        ['g2 1,0,0,0,0,0,128,0 64*512 25792 o256', 'g2 1,0,0,0,0,0,128,0 64*512 25792 o256', 'g2 2,0,0,0,0,0,128,0 64*512 33984 o256', 'g2 4,0,0,0,0,0,128,0 64*512 50368 o256', 'g2 4,0,0,0,0,0,128,0 64*512 50368 o256'],
        ['g2 1,0,0,0,0,0,128,0 64*512 25792 o256', 'g2 1,0,0,0,0,0,128,0 64*512 25792 o256', 'g2 2,0,0,0,0,0,128,0 64*512 33984 o256', 'g2 4,0,0,0,0,0,128,0 64*512 50368 o256', 'g2 4,0,0,0,0,0,128,0 64*512 50368 o256'],
    ],
    # tiny-nano, group size 32
    (32, 0, 128, (128, 64, 64)): [
        ['g2 1,0,0,0,0,0,32,0 16*512 52032 o256', 'g2 1,0,0,0,0,0,32,0 16*512 52032 o256', 'g2 2,0,0,0,0,0,32,0 16*512 84800 o256', 'g2 4,0,0,0,0,0,32,0 16*512 150336 o256', 'g2 4,0,0,0,0,0,32,0 16*512 150336 o256'],
        ['g2 1,0,0,0,0,0,32,0 16*512 52032 o256', 'g2 1,0,0,0,0,0,32,0 16*512 52032 o256', 'g2 2,0,0,0,0,0,32,0 16*512 84800 o256', 'g2 4,0,0,0,0,0,32,0 16*512 150336 o256', 'g2 4,0,0,0,0,0,32,0 16*512 150336 o256'],
    ],
    (32, 1, 128, (128,)): [
        ['g2 1,0,0,0,0,0,32,0 8*512 52032 o256', 'g2 1,0,0,0,0,0,32,0 8*512 52032 o256', 'g2 2,0,0,0,0,0,32,0 8*512 84800 o256', 'g2 4,0,0,0,0,0,32,0 8*512 150336 o256', 'g2 4,0,0,0,0,0,32,0 8*512 150336 o256'],
        ['g2 1,0,0,0,0,0,32,0 8*512 52032 o256', 'g2 1,0,0,0,0,0,32,0 8*512 52032 o256', 'g2 2,0,0,0,0,0,32,0 8*512 84800 o256', 'g2 4,0,0,0,0,0,32,0 8*512 150336 o256', 'g2 4,0,0,0,0,0,32,0 8*512 150336 o256'],
    ],
    (32, 2, 128, (384, 384)): [
        ['g2 1,0,0,0,0,0,32,1 24*512 104064 o256', 'g2 1,0,0,0,0,0,32,1 24*512 104064 o256', S3, S3, S3],
        ['g2 1,0,0,0,0,0,32,1 24*512 104064 o256', 'g2 1,0,0,0,0,0,32,1 24*512 104064 o256', S3, S3, S3],
    ],
    (32, 1, 384, (128,)): [
        ['g2 1,0,0,0,0,0,32,0 8*512 52544 o256', 'g2 1,0,0,0,0,0,32,0 8*512 52544 o256', 'g2 2,0,0,0,0,0,32,0 8*512 85312 o256', 'g2 4,0,0,0,0,0,32,0 8*512 150848 o256', 'g2 4,0,0,0,0,0,32,0 8*512 150848 o256'],
        ['g2 1,0,0,0,0,0,32,0 8*512 52544 o256', 'g2 1,0,0,0,0,0,32,0 8*512 52544 o256', 'g2 2,0,0,0,0,0,32,0 8*512 85312 o256', 'g2 4,0,0,0,0,0,32,0 8*512 150848 o256', 'g2 4,0,0,0,0,0,32,0 8*512 150848 o256'],
    ],
    (32, 0, 128, (512,)): [
        ['g2 1,0,0,0,0,0,32,0 32*512 52032 o256', 'g2 1,0,0,0,0,0,32,0 32*512 52032 o256', 'g2 2,0,0,0,0,0,32,0 32*512 84800 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150336 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150336 o256'],
        ['g2 1,0,0,0,0,0,32,0 32*512 52032 o256', 'g2 1,0,0,0,0,0,32,0 32*512 52032 o256', 'g2 2,0,0,0,0,0,32,0 32*512 84800 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150336 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150336 o256'],
    ],
    # tiny-nano, group size 64
    (64, 0, 128, (128, 64, 64)): [
        ['g2 1,0,0,0,0,0,64,0 16*512 34496 o256', 'g2 1,0,0,0,0,0,64,0 16*512 34496 o256', 'g2 2,0,0,0,0,0,64,0 16*512 50880 o256', 'g2 4,0,0,0,0,0,64,0 16*512 83648 o256', 'g2 4,0,0,0,0,0,64,0 16*512 83648 o256'],
        ['g2 1,0,0,0,0,0,64,0 16*512 34496 o256', 'g2 1,0,0,0,0,0,64,0 16*512 34496 o256', 'g2 2,0,0,0,0,0,64,0 16*512 50880 o256', 'g2 4,0,0,0,0,0,64,0 16*512 83648 o256', 'g2 4,0,0,0,0,0,64,0 16*512 83648 o256'],
    ],
    (64, 1, 128, (128,)): [
        ['g2 1,0,0,0,0,0,64,0 8*512 34496 o256', 'g2 1,0,0,0,0,0,64,0 8*512 34496 o256', 'g2 2,0,0,0,0,0,64,0 8*512 50880 o256', 'g2 4,0,0,0,0,0,64,0 8*512 83648 o256', 'g2 4,0,0,0,0,0,64,0 8*512 83648 o256'],
        ['g2 1,0,0,0,0,0,64,0 8*512 34496 o256', 'g2 1,0,0,0,0,0,64,0 8*512 34496 o256', 'g2 2,0,0,0,0,0,64,0 8*512 50880 o256', 'g2 4,0,0,0,0,0,64,0 8*512 83648 o256', 'g2 4,0,0,0,0,0,64,0 8*512 83648 o256'],
    ],
    (64, 2, 128, (384, 384)): [
        ['g2 1,0,0,0,0,0,64,1 24*512 68992 o256', 'g2 1,0,0,0,0,0,64,1 24*512 68992 o256', 'g2 2,0,0,0,0,0,64,1 24*512 101760 o256', 'g2 4,0,0,0,0,0,64,1 24*512 100736 o256', 'g2 4,0,0,0,0,0,64,1 24*512 100736 o256'],
        ['g2 1,0,0,0,0,0,64,1 24*512 68992 o256', 'g2 1,0,0,0,0,0,64,1 24*512 68992 o256', 'g2 2,0,0,0,0,0,64,1 24*512 101760 o256', 'g2 4,0,0,0,0,0,64,1 24*512 100736 o256', 'g2 4,0,0,0,0,0,64,1 24*512 100736 o256'],
    ],
    (64, 1, 384, (128,)): [
        ['g2 1,0,0,0,0,0,64,0 8*512 34752 o256', 'g2 1,0,0,0,0,0,64,0 8*512 34752 o256', 'g2 2,0,0,0,0,0,64,0 8*512 51136 o256', 'g2 4,0,0,0,0,0,64,0 8*512 83904 o256', 'g2 4,0,0,0,0,0,64,0 8*512 83904 o256'],
        ['g2 1,0,0,0,0,0,64,0 8*512 34752 o256', 'g2 1,0,0,0,0,0,64,0 8*512 34752 o256', 'g2 2,0,0,0,0,0,64,0 8*512 51136 o256', 'g2 4,0,0,0,0,0,64,0 8*512 83904 o256', 'g2 4,0,0,0,0,0,64,0 8*512 83904 o256'],
    ],
    (64, 0, 128, (512,)): [
        ['g2 1,0,0,0,0,0,64,0 32*512 34496 o256', 'g2 1,0,0,0,0,0,64,0 32*512 34496 o256', 'g2 2,0,0,0,0,0,64,0 32*512 50880 o256', 'g2 4,0,0,0,0,0,64,0 32*512 83648 o256', 'g2 4,0,0,0,0,0,64,0 32*512 83648 o256'],
        ['g2 1,0,0,0,0,0,64,0 32*512 34496 o256', 'g2 1,0,0,0,0,0,64,0 32*512 34496 o256', 'g2 2,0,0,0,0,0,64,0 32*512 50880 o256', 'g2 4,0,0,0,0,0,64,0 32*512 83648 o256', 'g2 4,0,0,0,0,0,64,0 32*512 83648 o256'],
    ],
    # tiny-nano, group size 128
    (128, 0, 128, (128, 64, 64)): [
        ['gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced'],
        ['gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced'],
    ],
    (128, 1, 128, (128,)): [
        ['gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced'],
        ['gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced'],
    ],
    (128, 2, 128, (384, 384)): [
        ['gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced'],
        ['gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced'],
    ],
    (128, 1, 384, (128,)): [
        ['g2 1,0,0,0,0,0,128,0 8*512 25792 o256', 'g2 1,0,0,0,0,0,128,0 8*512 25792 o256', 'g2 2,0,0,0,0,0,128,0 8*512 33984 o256', 'g2 4,0,0,0,0,0,128,0 8*512 50368 o256', 'g2 4,0,0,0,0,0,128,0 8*512 50368 o256'],
        ['g2 1,0,0,0,0,0,128,0 8*512 25792 o256', 'g2 1,0,0,0,0,0,128,0 8*512 25792 o256', 'g2 2,0,0,0,0,0,128,0 8*512 33984 o256', 'g2 4,0,0,0,0,0,128,0 8*512 50368 o256', 'g2 4,0,0,0,0,0,128,0 8*512 50368 o256'],
    ],
    (128, 0, 128, (512,)): [
        ['gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced'],
        ['gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced', 'gemv_sliced'],
    ],
    # tiny-nano-odd, group size 32
    (32, 0, 192, (192, 96, 96)): [
        ['g2 1,0,0,0,0,0,32,0 24*512 52160 o256', 'g2 1,0,0,0,0,0,32,0 24*512 52160 o256', 'g2 2,0,0,0,0,0,32,0 24*512 84928 o256', 'g2 4,0,0,0,0,0,32,0 24*512 150464 o256', 'g2 4,0,0,0,0,0,32,0 24*512 150464 o256'],
        ['g2 1,0,0,0,0,0,32,0 24*512 52160 o256', 'g2 1,0,0,0,0,0,32,0 24*512 52160 o256', 'g2 2,0,0,0,0,0,32,0 24*512 84928 o256', 'g2 4,0,0,0,0,0,32,0 24*512 150464 o256', 'g2 4,0,0,0,0,0,32,0 24*512 150464 o256'],
    ],
    (32, 1, 192, (192,)): [
        ['g2 1,0,0,0,0,0,32,0 12*512 52160 o256', 'g2 1,0,0,0,0,0,32,0 12*512 52160 o256', 'g2 2,0,0,0,0,0,32,0 12*512 84928 o256', 'g2 4,0,0,0,0,0,32,0 12*512 150464 o256', 'g2 4,0,0,0,0,0,32,0 12*512 150464 o256'],
        ['g2 1,0,0,0,0,0,32,0 12*512 52160 o256', 'g2 1,0,0,0,0,0,32,0 12*512 52160 o256', 'g2 2,0,0,0,0,0,32,0 12*512 84928 o256', 'g2 4,0,0,0,0,0,32,0 12*512 150464 o256', 'g2 4,0,0,0,0,0,32,0 12*512 150464 o256'],
    ],
    (32, 2, 192, (352, 352)): [
        ['g2 1,0,0,0,0,0,32,1 22*512 104320 o256', 'g2 1,0,0,0,0,0,32,1 22*512 104320 o256', S3, S3, S3],
        ['g2 1,0,0,0,0,0,32,1 22*512 104320 o256', 'g2 1,0,0,0,0,0,32,1 22*512 104320 o256', S3, S3, S3],
    ],
    (32, 1, 352, (192,)): [
        ['g2 1,0,0,0,0,0,32,0 12*512 52416 o256', 'g2 1,0,0,0,0,0,32,0 12*512 52416 o256', 'g2 2,0,0,0,0,0,32,0 12*512 85184 o256', 'g2 4,0,0,0,0,0,32,0 12*512 150720 o256', 'g2 4,0,0,0,0,0,32,0 12*512 150720 o256'],
        ['g2 1,0,0,0,0,0,32,0 12*512 52416 o256', 'g2 1,0,0,0,0,0,32,0 12*512 52416 o256', 'g2 2,0,0,0,0,0,32,0 12*512 85184 o256', 'g2 4,0,0,0,0,0,32,0 12*512 150720 o256', 'g2 4,0,0,0,0,0,32,0 12*512 150720 o256'],
    ],
    (32, 0, 192, (512,)): [
        ['g2 1,0,0,0,0,0,32,0 32*512 52160 o256', 'g2 1,0,0,0,0,0,32,0 32*512 52160 o256', 'g2 2,0,0,0,0,0,32,0 32*512 84928 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150464 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150464 o256'],
        ['g2 1,0,0,0,0,0,32,0 32*512 52160 o256', 'g2 1,0,0,0,0,0,32,0 32*512 52160 o256', 'g2 2,0,0,0,0,0,32,0 32*512 84928 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150464 o256', 'g2 4,0,0,0,0,0,32,0 32*512 150464 o256'],
    ],
}


def pin_of(p):
    if not p["kernel"]:
        return nb.ROUTE_NAMES[p["route"]]
    return "%s %d,%d,%d,%d,%d,%d,%d,%d %d*%d %d o%d" % (nb.Q80_GEMM_KERNELS[p["kernel"]], p["tt"], p["nv"], p["r"], p["ms"], p["tp"], p["pp"], p["gs"], p["sw"],
                                                    p["grid"], p["threads"], p["lds_bytes"], p["norm_order"])


@pytest.mark.parametrize("shape", list(PINS), ids=lambda s: f"gs{s[0]}-k{s[1]}-{s[2]}x{sum(s[3][:1] if s[1] == 2 else s[3])}")
def test_model_plans_unchanged(shape):
    gs, kind, n, rows = shape
    toks = PIN_TOKENS_MODELS if len(PINS[shape][0]) == len(PIN_TOKENS_MODELS) else PIN_TOKENS_TINY
    for ordered, want in zip((False, True), PINS[shape]):
        assert len(want) == len(toks)
        got = [pin_of(check(gs, kind, n, rows, t, ordered)) for t in toks]
        assert got == want, (shape, ordered, [(t, g, w) for t, g, w in zip(toks, got, want) if g != w])


def test_query_needs_no_device_and_follows_no_pointer():
    """shape fields only: the descriptor of the binding's query holds no weight, activation or output pointer at all"""
    p = nb.q80_gemm_plan(1, 4096, (2560,), 16)
    want = dict.fromkeys(F, 0)
    want.update(route=nb.ROUTE_NAMES.index("frag_g7"), kernel=KERN["g7k"], threads=704, grid=256, lds_bytes=138752, norm_order=512, hh=5, ntiles=256,
                nu=8, nk=16, ttl=1, ks=5, ncw=5, nss=2, tab=130560, ring=3, nl=6, takes=1)
    assert p == want, {f: (p[f], want[f]) for f in F if p[f] != want[f]}
    assert nb.q80_gemm_plan(1, 4096, (2560,), 16, cus=0) == p and nb.q80_gemm_plan(1, 4096, (2560,), 16, cus=64)["kernel"] == KERN["g6f"]
    # the GEMV query's answer for a batched route is what it was: the route, one launch of nb sequences, zeros
    g = nb.q80_gemv_plan(1, 4096, (2560,), 16)
    assert g == dict(dict.fromkeys(nb.Q80_PLAN_FIELDS, 0), route=p["route"], launches=1, seqs_per_launch=16, takes=1)
