"""CPU tests (no device) of the FP32 MFMA GEMM's launch planner: nano_hip_f32_gemm_plan reports route_kind() and the F32GemmPlan the
launcher consumes (nano_amd/csrc/gemm_f32_host.h).  Swept over kinds, row lengths, row sets, every token count 1..65, norm on / off and
split-attention partials: the documented refusals, and for every accepted plan the invariants the kernel relies on -- the grid covers
all rows, the token tiles cover all tokens, every unit of a row is owned by exactly one wave, the LDS request is what the kernel lays
out and fits a CU.  nano_hip_f32_gemv_plan, which describes the sliced route, keeps answering as tests/test_f32_gemv_plan.py pins it."""
import numpy as np
import pytest

from nano_amd import binding as nb

LDS_MAX = 163840
NS = [4, 128, 256, 260, 352, 768, 1408, 2048, 2560, 9728, 16384, 16388]
ROW_SETS = [(16,), (48,), (768, 384, 384), (20,), (151936,), (32, 16), (16, 20, 16)]
STAGE = 64 * (32 + 4) * 4          # a wave's transposition buffer: 64 operand lines of 32 items + 4 floats of padding


def heads_of(n):
    hd = next(h for h in (128, 64, 48, 32, 4) if n % h == 0)
    return n // hd, hd, 4


def sliced_plan_takes(kind, n, rows, nb_, norm):
    return nb.f32_gemv_plan(kind, n, rows, nb_, norm=norm)["takes"] == 1


def check(kind, n, rows, nb_, norm, attn=None):
    if attn is not None and nb_ > 8:                       # the descriptor itself is malformed: FP32 partials reach at most 8 sequences
        with pytest.raises(nb.NanoHipError):
            nb.f32_gemm_plan(kind, n, rows, nb_, norm=norm, attn=attn)
        return None
    p = nb.f32_gemm_plan(kind, n, rows, nb_, norm=norm, attn=attn)
    ctx = (kind, n, rows, nb_, norm, attn, p)
    assert p["takes"] == 1, ctx
    nmat = 2 if kind == 2 else 1
    total = rows[0] if kind == 2 else sum(rows)
    nt, nu = (nb_ + 15) // 16, (n + 127) // 128
    tab = nmat * nu * 16 * (nt * 16 + 4) * 4                # the unit-sum table [matrix][unit][row][16 * token tiles + 4]
    refused = (nb_ < 9 or nb_ > 64 or attn is not None or any(r % 16 for r in rows) or any(r * n * 4 >= 2 ** 32 for r in rows)
               or not sliced_plan_takes(kind, n, rows, nb_, norm)          # rows beyond 16384 floats, 8192 with SwiGLU
               or STAGE + tab > LDS_MAX or n * 4 + 64 > LDS_MAX)
    route = nb.ROUTE_NAMES[p["route"]]
    if refused:
        assert route == ("gemv_sliced" if nb_ > 8 else "gemv"), ("taken against a documented refusal", ctx)
        assert not any(v for k, v in p.items() if k not in ("route", "takes")), ctx
        return p
    assert route == "f32_gemm", ("refused without a documented reason", ctx)
    assert p["sw"] == nmat - 1 and p["rt"] == 16, ctx
    assert p["grid"] * p["rt"] == total, ("the grid does not cover the rows", ctx)
    assert p["nt"] == nt and p["nt"] * 16 >= nb_ > (p["nt"] - 1) * 16, ctx
    assert p["nu"] == nu and p["nu"] * 128 >= n > (p["nu"] - 1) * 128, ctx
    nw = p["nw"]
    assert 1 <= nw <= 8 and p["threads"] == 64 * nw, ctx
    owners = np.zeros(nu, np.int64)                         # unit u belongs to wave u % nw, which walks u, u + nw, ...
    for w in range(nw):
        mine = list(range(w, nu, nw))
        assert len(mine) <= p["upw"], ctx
        owners[mine] += 1
    assert np.all(owners == 1), ("a unit without a wave, or with two", ctx)
    assert p["upw"] == -(-nu // nw), ctx
    assert p["tp"] == nt * 16 + 4 and p["stage_bytes"] == STAGE and p["tab_off"] == nw * STAGE, ctx
    assert p["lds_bytes"] == nw * STAGE + tab and p["lds_bytes"] <= LDS_MAX, ctx
    assert nw == min(8, nu) or (nw + 1) * STAGE + tab > LDS_MAX, ("fewer waves than the table leaves room for", ctx)
    # the prologue runs the sliced route's rmsnorm tree: the thread count of that route's launch for the shape
    g = nb.f32_gemv_plan(kind, n, rows, nb_, norm=norm)
    assert p["pro_threads"] == 64 * g["nw"] and p["pro_lds"] == n * 4 + 64, ctx
    assert p["xs_floats"] == nt * 16 * nu * 128, ctx
    return p


def test_sweep():
    taken = refused = 0
    for n in NS:
        for rows in ROW_SETS:
            for nb_ in range(1, 66):
                if nb_ == 65:
                    with pytest.raises(nb.NanoHipError):
                        nb.f32_gemm_plan(0, n, rows, nb_)
                    continue
                for norm in (False, True):
                    cases = [(0, rows)]
                    if len(rows) == 1:
                        cases += [(1, rows), (2, rows * 2)]
                    for kind, rs in cases:
                        if kind == 1 and norm:
                            continue
                        p = check(kind, n, rs, nb_, norm)
                        if nb.ROUTE_NAMES[p["route"]] == "f32_gemm":
                            taken += 1
                        else:
                            refused += 1
                if len(rows) == 1 and nb_ in (1, 8, 9, 33):
                    check(1, n, rows, nb_, False, attn=heads_of(n))
    assert taken > 3000 and refused > 3000, (taken, refused)


def test_documented_refusals_and_named_plans():
    P = lambda *a, **k: nb.ROUTE_NAMES[nb.f32_gemm_plan(*a, **k)["route"]]
    assert P(0, 768, (768, 384, 384), 8) == "gemv" and P(0, 768, (768, 384, 384), 9) == "f32_gemm" and P(0, 768, (768, 384, 384), 64) == "f32_gemm"
    assert P(0, 768, (20,), 16) == "gemv_sliced" and P(0, 768, (32, 20), 16) == "gemv_sliced"
    assert P(1, 768, (16,), 8, attn=(16, 48, 4)) == "gemv"
    assert P(0, 16384, (16,), 9) == "gemv_sliced" and P(0, 16388, (16,), 9) == "gemv_sliced"        # the table beyond a CU's LDS; a row the GEMV plan refuses
    assert P(2, 8196, (16, 16), 9) == "gemv_sliced"
    assert P(0, 2560, (151936,), 9) == "f32_gemm" and P(0, 9728, (151936,), 9) == "gemv_sliced"      # 5.9 GB: 32-bit byte offsets
    # Nano-168M's per-layer launches at 64 tokens, and its classifier
    for kind, n, rows, nw, upw in ((0, 768, (768, 384, 384), 6, 1), (1, 768, (768,), 6, 1), (2, 768, (2048, 2048), 6, 1), (1, 2048, (768,), 8, 2)):
        p = check(kind, n, rows, 64, kind != 1)
        assert (p["nw"], p["upw"], p["nt"]) == (nw, upw, 4), p
    with pytest.raises(nb.NanoHipError):
        nb.f32_gemm_plan(0, 258, (16,), 9)


def test_the_sliced_route_plan_is_unchanged():
    """nano_hip_f32_gemv_plan describes the sliced route and answers as before (the pins of tests/test_f32_gemv_plan.py at nb = 11, 64)"""
    p = nb.f32_gemv_plan(0, 768, (768, 384, 384), 64, norm=True)
    assert (p["takes"], p["B"], p["launches"], p["seqs_per_launch"], p["rw"], p["nw"], p["upw"], p["nv"]) == (1, 8, 8, 8, 4, 3, 1, 1)
    p = nb.f32_gemv_plan(0, 768, (768, 384, 384), 11, norm=True)
    assert (p["takes"], p["B"], p["launches"], p["seqs_per_launch"]) == (1, 8, 2, 8)
    for nb_, launches, per in ((11, 3, 4), (64, 16, 4)):
        p = nb.f32_gemv_plan(1, 9728, (2560,), nb_)
        assert (p["launches"], p["seqs_per_launch"], p["lds_bytes"]) == (launches, per, 158464), (nb_, p)
    p = nb.f32_gemv_plan(0, 64, (151936,), 11)
    assert (p["B"], p["rw"], p["nw"], p["launches"], p["seqs_per_launch"]) == (8, 32, 8, 2, 8)


def test_query_needs_no_device_and_ignores_cus():
    p = nb.f32_gemm_plan(2, 768, (2048, 2048), 64, norm=True)
    assert all(nb.f32_gemm_plan(2, 768, (2048, 2048), 64, norm=True, cus=c) == p for c in (0, 1, 304))
