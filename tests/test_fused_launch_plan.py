"""CPU sweep of the two fused one-sequence launch plans (nano_hip_qkv_attn_fused_plan: qkv_attn_fused_plan(), nano_hip_wo_w13_fused_plan:
wo_w13_fused_plan() -- nano_amd/csrc/kernels.h; the functions launch_qkv_attn_fused() and launch_wo_w13_fused() take every choice from, behind
the conditions backend_step.hip puts in front of them).  No GPU: the queries are host arithmetic on shapes.

A FORM is the kernel and the template values of a launch:
    ("q80_table", NV, UPW)   qkv_attn_fused_kernel<NV, UPW>          Q80 group size 64, the product table and the barrier behind the dots
    ("q80_wf", 1, 1)         qkv_attn_fused_wf_kernel                Q80, rows of one chunk (n == 1024): every wave folds its own rows
    ("q4k", 1, D)            q4k_qkv_attn_fused_kernel<D>
    ("f32", 1, QV)           f32_qkv_attn_fused_kernel<QV>           QV 1: head_dim <= 32, 2: above
    ("wo_w13", 3, role, WF, WFC)     wo_w13_fused_kernel<role, WF, WFC>: 512 threads, one item per thread and one unit per wave (the queries' sig 3)
The sweeps below run the shape space the models can bring -- row lengths in multiples of 64 up to 4096; 1 .. 64 heads, the KV head count
and the head ratio powers of two; head_dim 128 (Q80, Q4K: Qwen3's attention) or 4 .. 64 in steps of 4 (FP32: Nano's); 1 .. 8 splits;
range_hint up to nsplit * 64; 256 compute units; Wo rows of up to 4096, W1|W3 rows of up to 2048 values, hidden sizes in steps of 256 (the
planner's slabs move with rows / 256) up to 16384 -- and check that
  * the forms met are exactly UNIVERSE, and SMALLEST names the smallest shape of each (weight bytes, then range_hint, then the shape);
  * the instantiations the launchers (the wave-fold kernel and the macros FUSED_GO, Q4F_GO, F32F_GO, WO13_GO) name are exactly UNIVERSE;
  * no plan asks for more than 64 KiB of LDS, runs other than 256 threads next to the attention workgroups, or -- Wo + W1|W3, whose waits
    rely on the whole grid being resident -- more workgroups than compute units;
  * the attention side (kernels.h fused_attn_side_ok()) decides independently of the projection: nsplit 1 .. 8, a power-of-two KV head
    count and ratio, n_head * nsplit <= 256, range_hint <= nsplit * 64;
  * the presets take the forms PRESETS records.
The kernels behind the forms run in tests/test_gpu_fused_launches.py, whose cases and coverage test read UNIVERSE and SMALLEST."""
import ctypes as C

import numpy as np
import pytest

from nano_amd import binding as nb
from nano_amd import modelfile as mf

F32, Q80, Q4K = 0x00, 0x80, 0x42
LDS_MAX = 64 * 1024
CUS = 256
R_RESID, R_COMBINE = nb.Q80_ROLES.index("resid"), nb.Q80_ROLES.index("resid_combine")

# ---- the reachable forms, and the smallest shape the sweep meets each at ----------------------------------------------------------------
# q | k | v + attention: (n, n_head, n_kv_head, head_dim); Wo + W1|W3: (Wo n, n_embd, n_hidden, splits Wo combines -- 1: none)
SMALLEST = {
    ("q80_table", 1, 1): (256, 8, 4, 128),
    ("q80_table", 1, 2): (256, 32, 16, 128),
    ("q80_table", 1, 4): (256, 64, 32, 128),
    ("q80_table", 2, 1): (1280, 1, 1, 128),
    ("q80_table", 2, 2): (1280, 16, 8, 128),
    ("q80_wf", 1, 1): (1024, 8, 4, 128),
    ("q4k", 1, 1): (256, 1, 1, 128),
    ("q4k", 1, 2): (256, 16, 16, 128),
    ("q4k", 1, 4): (256, 32, 32, 128),
    ("q4k", 1, 8): (256, 64, 64, 128),
    ("f32", 1, 1): (64, 1, 1, 4),
    ("f32", 1, 2): (64, 1, 1, 36),
    ("wo_w13", 3, R_RESID, 0, 0): (1280, 256, 2304, 1),
    ("wo_w13", 3, R_RESID, 0, 2): (2048, 256, 2304, 1),
    ("wo_w13", 3, R_RESID, 1, 0): (1280, 1024, 2304, 1),
    ("wo_w13", 3, R_RESID, 1, 2): (2048, 1024, 2304, 1),
    ("wo_w13", 3, R_COMBINE, 0, 0): (1280, 256, 2304, 2),
    ("wo_w13", 3, R_COMBINE, 0, 2): (2048, 256, 2304, 2),
    ("wo_w13", 3, R_COMBINE, 1, 0): (1280, 1024, 2304, 2),
    ("wo_w13", 3, R_COMBINE, 1, 2): (2048, 1024, 2304, 2),
}
UNIVERSE = frozenset(SMALLEST)

# ---- every instantiation the launchers name (gemv_q80_impl.h FUSED_GO / the wave-fold kernel / WO13_GO, gemv_q4k_chunk.hip Q4F_GO, gemv_f32.hip F32F_GO) ----
NAMED = frozenset(
    [("q80_table", nv, upw) for nv, upw in ((1, 1), (1, 2), (1, 4), (2, 1), (2, 2))] + [("q80_wf", 1, 1)] +
    [("q4k", 1, d) for d in (1, 2, 4, 8)] +
    [("f32", 1, qv) for qv in (1, 2)] +
    [("wo_w13", 3, role, wf, wfc) for role in (R_RESID, R_COMBINE) for wf in (0, 1) for wfc in (0, 2)])

# ---- the presets: which form each takes (None: the step issues the plain launches) -------------------------------------------------------
# (preset, quant) -> (q | k | v + attention, Wo + W1|W3 at one split, ... at two)
PRESETS = {
    ("qwen3-0.6b", "q80"): (("q80_wf", 1, 1), ("wo_w13", 3, R_RESID, 1, 2), ("wo_w13", 3, R_COMBINE, 1, 2)),
    ("qwen3-0.6b-3l", "q80"): (("q80_wf", 1, 1), ("wo_w13", 3, R_RESID, 1, 2), ("wo_w13", 3, R_COMBINE, 1, 2)),
    ("qwen3-0.6b", "q4k"): (("q4k", 1, 4), None, None),
    ("qwen3-0.6b-3l", "q4k"): (("q4k", 1, 4), None, None),
    ("nano-56m", "f32"): (("f32", 1, 1), None, None),
    ("nano-168m", "f32"): (("f32", 1, 2), None, None),
    ("wide-qwen3-2l", "q80"): (None, None, None),       # n = 2560: seven waves, and >= 8 Mi weights -- both launches refuse Qwen3-4B's shapes
    ("qwen3-4b", "q80"): (None, None, None),
}

HEADS = [(kv * r, kv) for kv in (1, 2, 4, 8, 16, 32, 64) for r in (1, 2, 4, 8, 16, 32, 64) if kv * r <= 64]
NS = list(range(64, 4097, 64))


def qkv_form(p):
    """the form a q | k | v + attention plan names, None: the plain launches"""
    if not p["takes"]:
        assert not any(p.values()), p
        return None
    k = nb.FUSED_KERNELS[p["kernel"]]
    return (k, p["nv"], p["d"]) if k == "q4k" else (k, p["upw"], p["qv"]) if k == "f32" else (k, p["nv"], p["upw"])


def wo13_form(p):
    if not p["takes"]:
        assert not any(p.values()), p
        return None
    return ("wo_w13", p["sig"], p["role"], p["wf"], p["wfc"])


def qkv_weight_bytes(quant, n, n_head, n_kv, hd):
    rows = (n_head + 2 * n_kv) * hd
    return rows * n * 4 if quant == F32 else rows * (n + n // 64 * 4) if quant == Q80 else rows * (n // 256) * 160


def preset_forms(preset, quant):
    """the forms a model of the preset takes, from its ModelSpec alone"""
    s = mf.preset(preset, quant, group_size=64 if quant == "q80" else 0)
    hd = s.head_dim if s.arch == 3 else s.n_embd // s.n_head
    q = {"f32": F32, "q80": Q80, "q4k": Q4K}[quant]
    a = qkv_form(nb.qkv_attn_fused_plan(q, s.n_embd, s.n_head, s.n_kv_head, hd, gs=s.group_size))
    if quant != "q80":
        return a, None, None
    return (a, wo13_form(nb.wo_w13_fused_plan(s.n_head * hd, s.n_embd, s.n_hidden)),
            wo13_form(nb.wo_w13_fused_plan(s.n_head * hd, s.n_embd, s.n_hidden, attn=(s.n_head, hd, 2))))


def attn_lds(hd, plain):
    """gemv_common.h fused_attn_lds(): q | k | maxima | sums | 4 waves' partials | the fresh v row, Qwen3's body: | 4 give-up words | 4 x 8 weighted rows"""
    hd4 = (hd + 3) & ~3
    return (hd4 + hd4 + 4 + 4 + 4 * hd4 + hd4 + (0 if plain else 4 + 4 * 8 * hd4)) * 4


def check_qkv_plan(quant, n, n_head, n_kv, hd, nsplit, p):
    """what every taken plan promises, whatever its form"""
    ctx = (quant, n, n_head, n_kv, hd, nsplit, p)
    rows = ((n_head * hd), n_kv * hd, n_kv * hd)
    assert p["threads"] == 256 and p["lds_bytes"] <= LDS_MAX and p["_zero"] == 0, ctx
    assert p["n_attn"] == n_head * nsplit, ctx
    rw = p["rw"]
    if quant == F32:
        assert rw % 4 == 0 and p["ngemv"] == p["wg0"] == (sum(rows) + rw - 1) // rw and p["wg1"] == p["wg2"] == 0, ctx
        units = rw // 4 * ((n + 255) // 256)
        assert p["nv"] == 1 and n <= 1024 and units <= 4 * p["upw"] and p["qv"] == (1 if hd <= 32 else 2), ctx
        assert p["lds_bytes"] == max((((n + 3) & ~3) + 16 + rw * ((((n + 255) // 256) + 3) & ~3)) * 4, attn_lds(hd, True)), ctx
    else:
        assert [p["wg0"], p["wg1"], p["wg2"]] == [(r + rw - 1) // rw for r in rows] and p["ngemv"] == p["wg0"] + p["wg1"] + p["wg2"], ctx
        assert rw <= 256, ("a fold row without a thread", ctx)
        if quant == Q80:
            nchunk = (n + 1023) // 1024
            assert p["nv"] * 1024 >= n and (rw + 3) // 4 * nchunk <= 4 * p["upw"], ctx
            assert (nb.FUSED_KERNELS[p["kernel"]] == "q80_wf") == (n == 1024), ctx
            ng = n // 64
            table = 0 if n == 1024 else (rw + 3) // 4 * 4 * (((ng + 47) // 64) * 64 + 16) * 4
            # the larger of the two kinds' workgroups: activations | scales | norm partials | product table, or the attention's
            assert p["lds_bytes"] == max(((n + 15) & ~15) + ((ng + 3) & ~3) * 4 + 64 + table, attn_lds(hd, False)), ctx
        else:
            assert p["nv"] == 1 and n <= 1024 and n % 256 == 0 and p["rounds"] == 1, ctx
            assert ((rw * (n // 256) + 5) // 6 + 3) // 4 <= p["d"], ("a wave-load without a slot", ctx)
            assert p["lds_bytes"] >= attn_lds(hd, False), ctx           # (the chunk plan's own bytes are test_q4k_gemv_plan.py's; the 64 KiB cap above is what protects)


def test_qkv_attn_sweep_meets_exactly_the_universe():
    seen = {}
    for n in NS:
        for n_head, n_kv in HEADS:
            for quant, hds in ((Q80, (128,)), (Q4K, (128,)), (F32, range(4, 65, 4))):
                for hd in hds:
                    p = nb.qkv_attn_fused_plan(quant, n, n_head, n_kv, hd, range_hint=64, nsplit=1, cus=CUS)
                    f = qkv_form(p)
                    if f is None:
                        continue
                    check_qkv_plan(quant, n, n_head, n_kv, hd, 1, p)
                    key = (qkv_weight_bytes(quant, n, n_head, n_kv, hd), 64, n, n_head, n_kv, hd)
                    if f not in seen or key < seen[f]:
                        seen[f] = key
    want = {f for f in UNIVERSE if f[0] != "wo_w13"}
    assert set(seen) == want, ("reachable without a case / listed but not reached", sorted(set(seen) ^ want))
    for f, key in seen.items():
        assert SMALLEST[f] == key[2:], (f, "the smallest shape of this form is", key[2:])


def attn_side_ok(n_head, n_kv, nsplit, range_hint):
    """kernels.h fused_attn_side_ok(), the part the descriptor's shape decides"""
    r = n_head // n_kv if n_kv and n_head % n_kv == 0 else 0
    return (1 <= nsplit <= 8 and n_kv & (n_kv - 1) == 0 and r > 0 and r & (r - 1) == 0 and n_head * nsplit <= 256 and range_hint <= nsplit * 64)


@pytest.mark.parametrize("quant,n,hd", [(Q80, 1024, 128), (Q80, 256, 128), (Q4K, 512, 128), (F32, 256, 32), (F32, 64, 36)])
def test_attention_side_decides_alone(quant, n, hd):
    """every KV head count 1 .. 64 with power-of-two ratios, every split count 0 .. 9 (0 here: an explicit 9 stands for the step's own
    choice being out of range), range_hint at 1, at the bound and one beyond it: taken where the projection takes the heads and the
    attention side allows the rest -- and then the projection's side of the plan does not move"""
    met = set()
    for n_kv in range(1, 65):
        for r in (1, 2, 4, 8, 16, 32, 64):
            n_head = n_kv * r
            if n_head > 64:
                continue
            base = nb.qkv_attn_fused_plan(quant, n, n_head, n_kv, hd, range_hint=64, nsplit=1, cus=CUS)
            for nsplit in range(1, 10):
                for rh in (1, nsplit * 64, nsplit * 64 + 1):
                    p = nb.qkv_attn_fused_plan(quant, n, n_head, n_kv, hd, range_hint=rh, nsplit=nsplit, cus=CUS)
                    ok = bool(base["takes"]) and attn_side_ok(n_head, n_kv, nsplit, rh)
                    assert bool(p["takes"]) == ok, (quant, n, n_head, n_kv, hd, nsplit, rh, p)
                    if ok:
                        check_qkv_plan(quant, n, n_head, n_kv, hd, nsplit, p)
                        assert {k: v for k, v in p.items() if k != "n_attn"} == {k: v for k, v in base.items() if k != "n_attn"}
                        met.add((nsplit, n_kv >= 8, r))
    assert {m[0] for m in met} == set(range(1, 9)) and {m[1] for m in met} == {False, True} and {1, 2, 4, 8} <= {m[2] for m in met}, met


def test_attention_side_limits():
    """one shape just outside each predicate of the attention side, and the neighbours inside"""
    take = lambda *a, **k: nb.qkv_attn_fused_plan(*a, **k)["takes"]
    assert take(Q80, 256, 64, 32, 128, nsplit=4, range_hint=256) == 1                     # n_head * nsplit = 256
    assert take(Q80, 256, 64, 32, 128, nsplit=5, range_hint=320) == 0                     # ... 320
    assert take(F32, 256, 64, 64, 32, nsplit=4, range_hint=256) == 1
    assert take(F32, 64, 33, 1, 4, nsplit=8, range_hint=512) == 0                          # (33 heads: no power-of-two ratio)
    assert take(F32, 264, 66, 2, 4, nsplit=4, range_hint=256) == 0                         # n_head * nsplit = 264
    assert take(F32, 256, 4, 4, 64) == 1 and take(F32, 272, 4, 4, 68) == 0                 # head_dim 68
    assert take(F32, 256, 8, 8, 32, qk_norm=True) == 0 and take(F32, 256, 8, 8, 32, rope_qwen3=True) == 0    # Nano's plain attention only
    assert take(Q80, 1024, 16, 8, 128, qk_norm=False) == 0 and take(Q80, 1024, 32, 16, 64) == 0              # Qwen3's at head_dim 128 only
    assert take(Q80, 1024, 16, 8, 128, nsplit=2, range_hint=128) == 1 and take(Q80, 1024, 16, 8, 128, nsplit=2, range_hint=129) == 0
    assert take(Q80, 1024, 16, 8, 128, nsplit=0, range_hint=512) == 1                     # the step's own choice: 8 splits of 64
    assert take(Q80, 1024, 12, 4, 128) == 0 and take(Q80, 1024, 12, 3, 128) == 0


def test_projection_side_limits():
    """the refusals the planners' arithmetic sets, from both sides"""
    take = lambda *a, **k: nb.qkv_attn_fused_plan(*a, **k)["takes"]
    assert take(Q80, 1536, 16, 8, 128) == 1 and take(Q80, 1792, 16, 8, 128) == 0           # ceil(n / 384) == 4 waves
    assert take(Q80, 1024, 16, 8, 128, gs=128) == 0 and take(Q80, 1024, 16, 8, 128, ordered=True) == 0 and take(Q80, 1024, 16, 8, 128, use_gemm=True) == 0
    assert take(Q80, 320, 16, 8, 128) == 0                                                 # (not canonical: n % 256)
    assert take(Q4K, 1024, 16, 8, 128) == 1 and take(Q4K, 1280, 16, 8, 128) == 0
    assert take(F32, 1024, 4, 4, 64) == 1 and take(F32, 1088, 4, 4, 64) == 0 and take(F32, 1024, 16, 16, 64) == 0     # one float4 per thread; <= 4 units
    w = lambda *a, **k: nb.wo_w13_fused_plan(*a, **k)["takes"]
    assert w(2048, 1024, 3072) == 1 and w(2304, 1024, 3072) == 0                           # Wo n = 2304: three float4 items per thread on 256 threads
    assert w(2048, 1024, 3072, gs=128) == 0 and w(2048, 1024, 3072, ordered=True) == 0
    assert w(2048, 1024, 3072, attn=(16, 128, 8)) == 1
    assert w(4096, 2560, 9728) == 0                                                        # Qwen3-4B's


def test_wo_w13_sweep_meets_exactly_the_universe():
    seen = {}
    for n_wo in NS:
        for E in range(64, 2049, 64):
            for hidden in range(256, 16385, 256):
                for splits in (1, 2):
                    if splits > 1 and n_wo % 128:
                        continue
                    attn = (n_wo // 128, 128, splits) if splits > 1 else None
                    p = nb.wo_w13_fused_plan(n_wo, E, hidden, attn=attn, cus=CUS)
                    f = wo13_form(p)
                    if f is None:
                        continue
                    ctx = (n_wo, E, hidden, splits, p)
                    assert p["lds_bytes"] <= LDS_MAX and p["_zero"] == 0, ctx
                    assert p["wb"] <= CUS and p["wa"] <= p["wb"], ("the whole grid must be resident, Wo's workgroups among W1|W3's", ctx)
                    assert p["wa"] == (E + p["rw_a"] - 1) // p["rw_a"] and p["wb"] == (hidden + p["rw_b"] - 1) // p["rw_b"], ctx
                    assert p["sig"] == 3 and p["threads"] == 512 and max(p["rw_a"], p["rw_b"]) <= p["threads"], ctx
                    assert (p["nv_a"], p["upw_a"], p["nv_b"], p["upw_b"]) == (1, 1, 1, 1), ctx
                    assert p["nv_a"] * p["threads"] * 4 >= n_wo and p["nv_b"] * p["threads"] * 4 >= E, ("an activation float4 without a register", ctx)
                    waves = p["threads"] // 64
                    assert (p["rw_a"] + 3) // 4 * ((n_wo + 1023) // 1024) <= waves * p["upw_a"], ("a Wo unit without a wave slot", ctx)
                    units_b = (p["rw_b"] + 1) // 2 if p["wf"] else (p["rw_b"] + 3) // 4 * ((E + 1023) // 1024) * 2
                    assert units_b <= waves * p["upw_b"], ("a W1|W3 unit without a wave slot", ctx)
                    assert p["role"] == (R_COMBINE if splits > 1 else R_RESID) and p["wf"] == int(E == 1024) and p["wfc"] == (2 if n_wo == 2048 else 0), ctx
                    key = (n_wo * E + 2 * E * hidden, n_wo, E, hidden, splits)
                    if f not in seen or key < seen[f]:
                        seen[f] = key
    want = {f for f in UNIVERSE if f[0] == "wo_w13"}
    assert set(seen) == want, ("reachable without a case / listed but not reached", sorted(set(seen) ^ want))
    for f, key in seen.items():
        assert SMALLEST[f] == key[1:], (f, "the smallest shape of this form is", key[1:])


def test_universe_and_dead_account_for_every_named_instantiation():
    assert NAMED == UNIVERSE, ("named by a launcher and reached by no shape, or reachable and not built", sorted(NAMED ^ UNIVERSE))
    assert len(NAMED) == 5 + 1 + 4 + 2 + 8 == 20


def test_a_smaller_chip_changes_no_form_but_may_refuse():
    """Wo + W1|W3 needs a compute unit per workgroup: on fewer than the grid it is refused, never cut"""
    assert nb.wo_w13_fused_plan(2048, 1024, 3072, cus=256)["wb"] == 256
    for cus in (64, 128, 255):
        p = nb.wo_w13_fused_plan(2048, 1024, 3072, cus=cus)
        assert p["takes"] == 0 or p["wb"] <= cus, (cus, p)


@pytest.mark.parametrize("preset,quant", sorted(PRESETS))
def test_presets_take_the_recorded_forms(preset, quant):
    got = preset_forms(preset, quant)
    assert got == PRESETS[(preset, quant)], (preset, quant, got)
    assert all(f is None or f in UNIVERSE for f in got)


def test_wide_qwen3_takes_neither_fused_launch():
    """Qwen3-4B's shapes (n = 2560): q80_plan_slab asks for at least ceil(2560 / 384) = 7 waves (8 or more on matrices of >= 8 Mi weights),
    fused_shape() takes four -- the steps of wide-qwen3-2l issue the plain launches whatever NANO_FUSE_LAUNCHES says"""
    assert preset_forms("wide-qwen3-2l", "q80") == (None, None, None)
    assert nb.q80_gemv_plan(0, 2560, [4096, 1024, 1024], 1, norm=True)["nw"] >= 7


def test_queries_need_no_device_and_follow_no_pointer():
    """descriptors whose pointers are all null but the flags: the answer is the shape's"""
    g = nb._fused_shape(Q80, 0, 1024, [2048, 1024, 1024], 1, gs=64, norm=True)
    a = nb._attn_shape(16, 8, 128, range_hint=64, nsplit=1)
    out = np.zeros(len(nb.QKV_ATTN_FUSED_PLAN_FIELDS), np.uint32)
    assert nb.lib().nano_hip_qkv_attn_fused_plan(C.byref(g), C.byref(a), 256, out.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert out[-1] == 1 and nb.FUSED_KERNELS[out[0]] == "q80_wf"
    a.kv_half = 1
    assert nb.lib().nano_hip_qkv_attn_fused_plan(C.byref(g), C.byref(a), 256, out.ctypes.data_as(C.POINTER(C.c_uint32))) == 0 and not out.any()
    assert nb.lib().nano_hip_qkv_attn_fused_plan(None, C.byref(a), 256, out.ctypes.data_as(C.POINTER(C.c_uint32))) != 0
    assert nb.lib().nano_hip_wo_w13_fused_plan(C.byref(g), None, 256, out.ctypes.data_as(C.POINTER(C.c_uint32))) != 0
