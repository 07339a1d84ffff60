"""CPU tests: the C-ABI library loads without a GPU and exports every symbol the headers declare; the
model writer / layout helpers agree with each other; the product refuses to run without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from nano_amd import binding as nb
from nano_amd import modelfile as mf


def declared_symbols(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b([a-z_][a-z0-9_]*)\s*\([^;{}]*\)\s*;", src)
    return sorted({n for n in names if n not in ("defined", "sizeof", "void", "int", "char", "float") and not n.startswith("on_")})


@pytest.mark.parametrize("header", ["nano_mi355x.h", "nano_infer_abi.h"])
def test_library_exports_every_declared_symbol(header):
    L = nb.lib()
    syms = declared_symbols(header)
    assert len(syms) >= 15
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing


def test_fused_launch_entry_points_are_declared_and_exported():
    """the two plan queries and the two operators of the fused one-sequence launches: in the header, in the library, and the queries'
    word counts and the descriptor layouts of the binding are the header's"""
    syms = declared_symbols("nano_mi355x.h")
    for name in ("nano_hip_qkv_attn_fused_plan", "nano_hip_wo_w13_fused_plan", "nano_hip_op_qkv_attn_fused", "nano_hip_op_wo_w13_fused"):
        assert name in syms and hasattr(nb.lib(), name), name
    src = open(os.path.join(ROOT, "include", "nano_mi355x.h")).read()
    assert int(re.search(r"#define NANO_QKV_ATTN_FUSED_PLAN_WORDS (\d+)", src).group(1)) == len(nb.QKV_ATTN_FUSED_PLAN_FIELDS)
    assert int(re.search(r"#define NANO_WO_W13_FUSED_PLAN_WORDS (\d+)", src).group(1)) == len(nb.WO_W13_FUSED_PLAN_FIELDS)
    assert C.sizeof(nb.NanoQkvAttnFusedDesc) == 2 * 8 + 2 * 4 + 5 * 8 and C.sizeof(nb.NanoWoW13FusedDesc) == 2 * 8 + 2 * 4 + 3 * 8
    # the queries answer without a device, and refuse a null descriptor
    assert nb.qkv_attn_fused_plan(0x80, 1024, 16, 8, 128)["takes"] == 1 and nb.wo_w13_fused_plan(2048, 1024, 3072)["takes"] == 1
    out = (C.c_uint32 * 16)()
    assert nb.lib().nano_hip_qkv_attn_fused_plan(None, None, 256, out) == -1 and nb.lib().nano_hip_wo_w13_fused_plan(None, None, 256, out) == -1


def test_no_cpu_fallback():
    """Without a GPU the create call must fail loudly (no silent host path)."""
    if nb.device_count() > 0:
        pytest.skip("a GPU is visible here")
    spec = mf.preset("tiny-nano", "f32")
    blob = np.zeros(nb.lib().nano_hip_params_bytes(nb.desc_from_spec(spec)), np.uint8)
    with pytest.raises(nb.NanoHipError):
        nb.DeviceModel(nb.desc_from_spec(spec), blob, blob.size)
    with pytest.raises(nb.NanoHipError):
        nb.op_quantize_q80(np.zeros(64, np.float32), 64)
    z = np.zeros(64, np.float32)
    with pytest.raises(nb.NanoHipError):                # the fused-launch operators too: no device, no result
        nb.op_wo_w13_fused(64, (np.zeros(64 * 64, np.int8), z, 64), (np.zeros(64 * 64, np.int8), z, 64), (np.zeros(64 * 64, np.int8), z, 64), z, z, x=z)


@pytest.mark.parametrize("preset,quant,gs", [("tiny-nano", "f32", 0), ("tiny-qwen3", "q80", 64), ("tiny-nano-odd", "q4k", 0),
                                             ("qwen3-0.6b", "q80", 64), ("nano-168m", "f32", 0)])
def test_layout_and_backend_agree_on_blob_size(preset, quant, gs):
    spec = mf.preset(preset, quant, group_size=gs)
    lay = mf.param_layout(spec)
    want = lay.total_bytes - lay.params_offset
    got = nb.lib().nano_hip_params_bytes(nb.desc_from_spec(spec))
    if quant == "q4k":
        assert got == 0            # Q4K frames carry their own sizes
    else:
        assert got == want


def test_algorithmic_bytes_match_survey():
    """SURVEY 8d figures."""
    assert mf.preset("qwen3-0.6b", "q80", 64).algorithmic_bytes_per_token() == 633233408
    assert mf.preset("qwen3-0.6b", "q80", 128).algorithmic_bytes_per_token() == 614608896
    assert mf.preset("qwen3-0.6b", "q4k").algorithmic_bytes_per_token() == 372490240
    assert mf.preset("nano-168m", "f32").algorithmic_bytes_per_token() == 673185792
    assert mf.preset("nano-56m", "q80", 128).algorithmic_bytes_per_token() == 57311232
    assert mf.preset("qwen3-4b", "q80", 64).algorithmic_bytes_per_token() == 4273664000


def test_header_roundtrip(tmp_path):
    spec = mf.preset("tiny-qwen3", "q80", group_size=64)
    p = str(tmp_path / "m.bin")
    lay = mf.write_model(p, spec)
    assert os.path.getsize(p) == lay.total_bytes
    back = mf.read_header(p)
    assert back == spec
