"""CPU tests of the LoRA operator surface: the descriptors' layouts, the exported symbols, and every refusal -- all of them happen
before a device is asked for.  The operators have no host path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from nano_amd import binding as nb

EINVAL, ENODEV = -1, -3
HEADER = open(os.path.join(ROOT, "include", "nano_mi355x.h")).read()


def test_descriptor_layouts():
    D = nb.NanoLoraOpDesc
    assert C.sizeof(D) == 8 * 4 + 2 * 8 + 6 * 8 + 8 + 3 * 8 + 3 * 8 == 152
    assert (D.E.offset, D.nb.offset, D.S.offset, D.v_bstride.offset, D.x.offset, D.a.offset, D.b.offset, D.pos.offset, D.q.offset,
            D.q_floats.offset, D.v_floats.offset) == (0, 16, 20, 24, 32, 48, 72, 96, 104, 128, 144)
    assert re.search(r"uint32_t E, KD, rank, alpha, nb, S;\s*uint32_t v_bstride, _pad;", HEADER)
    G = nb.NanoFusedGemvDesc
    # the addend is APPENDED: every earlier field keeps its place
    assert G.argmax_out.offset == 192 and G.resid_add.offset == 200 and G.resid_add_stride.offset == 208 and C.sizeof(G) == 216
    assert re.search(r"uint32_t \*argmax_out;.*?const float \*resid_add;.*?uint32_t resid_add_stride;[^;]*\} NanoFusedGemvDesc;", HEADER, re.S)


def test_symbols_are_exported():
    for name in ("nano_hip_op_lora_qkv", "nano_hip_op_lora_o", "nano_hip_lora_attach", "nano_hip_lora_enable"):
        assert hasattr(nb.lib(), name) and re.search(r"\bint %s\(" % name, HEADER), name
    assert callable(nb.op_lora_qkv) and callable(nb.op_lora_o)


def desc(qkv=True, E=128, KD=64, rank=4, nb_=2, S=4, pos=(1, 3), v_slots=2, v_bstride=None, null=None, q_floats=None, k_floats=None, v_floats=None):
    keep = {n: np.zeros(sz, np.float32) for n, sz in (("x", nb_ * max(E, 1)), ("norm_w", max(E, 1)), ("A", min(max(rank, 1), 64) * max(E, 1)),
                                                     ("B", max(E, KD, 1) * min(max(rank, 1), 64)), ("q", nb_ * max(E, 1)), ("kraw", nb_ * max(KD, 1)),
                                                     ("v", v_slots * S * max(KD, 1)))}
    keep["pos"] = np.ascontiguousarray(pos, np.uint32)
    d = nb.NanoLoraOpDesc()
    d.E, d.KD, d.rank, d.alpha, d.nb, d.S = E, KD, rank, 16, nb_, S
    d.v_bstride = S * KD if v_bstride is None else v_bstride
    d.x, d.norm_w, d.pos = keep["x"].ctypes.data, keep["norm_w"].ctypes.data, keep["pos"].ctypes.data
    for i in range(3 if qkv else 1):
        d.a[i], d.b[i] = keep["A"].ctypes.data, keep["B"].ctypes.data
    d.q, d.kraw, d.v = keep["q"].ctypes.data, keep["kraw"].ctypes.data, keep["v"].ctypes.data
    d.q_floats = nb_ * E if q_floats is None else q_floats
    d.k_floats = nb_ * KD if k_floats is None else k_floats
    d.v_floats = v_slots * S * KD if v_floats is None else v_floats
    if null in ("a1", "b2"):
        getattr(d, null[0])[int(null[1])] = None
    elif null:
        setattr(d, null, None)
    return d, keep


def call(qkv=True, **kw):
    d, keep = desc(qkv, **kw)
    return (nb.lib().nano_hip_op_lora_qkv if qkv else nb.lib().nano_hip_op_lora_o)(0, C.byref(d))


def test_operators_refuse_before_they_ask_for_a_device():
    L = nb.lib()
    assert L.nano_hip_op_lora_qkv(0, None) == EINVAL and L.nano_hip_op_lora_o(0, None) == EINVAL
    for null in ("x", "norm_w", "pos", "q", "kraw", "v", "a1", "b2"):
        assert call(null=null) == EINVAL and "null" in nb.last_error(), null
    for null in ("x", "q"):
        assert call(qkv=False, null=null) == EINVAL, null
    for qkv in (True, False):
        assert call(qkv, E=130) == EINVAL and "% 4" in nb.last_error()
        assert call(qkv, rank=0) == EINVAL and "rank" in nb.last_error()
        assert call(qkv, E=8192, rank=2721) == EINVAL and "LDS" in nb.last_error()          # (8192 + 3 * 2721 + 32) * 4 = 65548 > 65536
        assert call(qkv, nb_=0, pos=()) == EINVAL and call(qkv, nb_=65, pos=(0,) * 65) == EINVAL
        assert call(qkv, q_floats=2 * 128 - 1) == EINVAL
    assert call(KD=0) == EINVAL and call(k_floats=127) == EINVAL
    assert call(pos=(1, 4)) == EINVAL and "beyond S" in nb.last_error()
    assert call(v_slots=1) == EINVAL and "v_floats" in nb.last_error()                      # sequence 1's slot is not in the buffer
    assert call(v_slots=1, v_bstride=0) != EINVAL                                           # ... as a chunk of one slot it is


def test_attach_refuses_a_null_model_and_what_the_launches_cannot_run():
    L = nb.lib()
    p = np.zeros(16, np.float32)
    assert L.nano_hip_lora_attach(None, 4, 8, p, p.size) == EINVAL and L.nano_hip_lora_enable(None, 1) == EINVAL
    src = open(os.path.join(ROOT, "nano_amd", "csrc", "backend.hip")).read()
    attach = src[src.index('extern "C" int nano_hip_lora_attach'):src.index('extern "C" int nano_hip_lora_enable')]
    assert attach.index("lora_shape_error(m->d.n_embd, rank)") < attach.index("hipSetDevice")   # the operators' own check, before any device work


def test_fused_gemv_addend_is_a_flag_of_the_plan_queries():
    """the descriptor's shape check refuses an addend outside kind 1 or narrower than the rows; the queries read it as a flag: Q80's
    batched routes refuse a launch with an addend (route.hip), so the flag moves a 16-sequence step's Wo from the fragment route to slices"""
    out = (C.c_uint32 * 32)()
    for kind, stride in ((0, 256), (2, 256), (1, 255)):
        d = nb._fused_shape(0x80, kind, 256, [256, 256] if kind == 2 else [256], 1, gs=64, resid_add=(nb._FLAG.ctypes.data, stride))
        assert nb.lib().nano_hip_q80_gemv_plan(C.byref(d), 256, out) == EINVAL and "addend" in nb.last_error()
    plain = nb.q80_gemv_plan(1, 1024, [1024], 16, gs=64, use_gemm=True)
    added = nb.q80_gemv_plan(1, 1024, [1024], 16, gs=64, use_gemm=True, resid_add=True)
    assert plain["takes"] == 1 and added["takes"] == 1
    assert nb.ROUTE_NAMES[plain["route"]].startswith("frag") and nb.ROUTE_NAMES[added["route"]].startswith("gemv"), (plain, added)
    assert added["launches"] * added["seqs_per_launch"] >= 16 and added["launches"] > 1
    for q in (nb.f32_gemv_plan, nb.q4k_gemv_plan):
        assert q(1, 1024, [1024], 3, resid_add=True)["takes"] == 1


def test_operators_have_no_host_path():
    """valid arguments: without a device no result (and no quiet host computation); with one, the launch runs"""
    if nb.device_count() > 0:
        assert call() == 0 and call(qkv=False) == 0
        return
    assert call() == ENODEV and call(qkv=False) == ENODEV
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(nb.NanoHipError):
        nb.op_lora_o(z(1, 128), (z(4, 128), z(128, 4)), z(1, 128), rank=4, alpha=8)
    with pytest.raises(nb.NanoHipError):
        nb.op_lora_qkv(z(1, 128), z(128), ((z(4, 128), z(128, 4)), (z(4, 128), z(64, 4)), (z(4, 128), z(64, 4))), z(1, 128), z(1, 64), z(1, 4, 64),
                       [2], KD=64, rank=4, alpha=8, S=4, v_bstride=256)
    with pytest.raises(nb.NanoHipError):
        nb.op_fused_gemv(0x00, 1, 128, [(z(128, 128), None, 128)], z(1, 128), resid=z(1, 128), resid_add=z(1, 128))
