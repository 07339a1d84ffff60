"""CPU tests of the LoRA table's surface: the new symbols in the header and in the library, the per-row operators' descriptor layout, the
device-free size query against the module files mf.write_lora writes, and every refusal that can be asked for without a device -- with
a null model, or, for the two operators, before a device is asked for.  The operators have no host path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from nano_amd import binding as nb
from nano_amd import modelfile as mf

EINVAL, ENODEV = -1, -3
HEADER = open(os.path.join(ROOT, "include", "nano_mi355x.h")).read()
ENGINE_HEADER = open(os.path.join(ROOT, "include", "nano_infer_abi.h")).read()
NONE = nb.NANO_LORA_NONE


def test_symbols_are_declared_and_exported():
    L = nb.lib()
    for name in ("nano_hip_lora_table_set", "nano_hip_lora_table_clear", "nano_hip_lora_bind", "nano_hip_lora_binding",
                 "nano_hip_op_lora_qkv_rows", "nano_hip_op_lora_o_rows"):
        assert hasattr(L, name) and re.search(r"\bint %s\(" % name, HEADER), name
    assert hasattr(L, "nano_hip_lora_param_floats") and re.search(r"\bsize_t nano_hip_lora_param_floats\(", HEADER)
    for name in ("nano_lora_table_load", "nano_lora_table_load_from_buffer", "nano_lora_table_free", "nano_lora_bind"):
        assert hasattr(L, name) and re.search(r"\bint %s\(" % name, ENGINE_HEADER), name
    assert re.search(r"#define NANO_LORA_TABLE_MAX\s+64u", HEADER) and re.search(r"#define NANO_LORA_NONE\s+0xffffffffu", HEADER)
    assert nb.NANO_LORA_TABLE_MAX == 64 and NONE == 0xffffffff
    for f in (nb.op_lora_qkv_rows, nb.op_lora_o_rows, nb.lora_param_floats, nb.DeviceModel.lora_table_set_file, nb.DeviceModel.lora_table_clear,
              nb.DeviceModel.lora_bind, nb.DeviceModel.lora_binding, nb.Engine.lora_table_load, nb.Engine.lora_table_free, nb.Engine.lora_bind):
        assert callable(f)
    for phrase in ("Not offered", "Qwen", "FP16, FP8 or paged", "strict or exact", "ragged steps or pooling", "more than one attention split",
                   "quantized form", "bindings inside KV"):
        assert phrase in HEADER, phrase                     # the "not offered" list, stated where the calls are declared


def test_descriptor_layouts():
    A = nb.NanoLoraAdapter
    assert C.sizeof(A) == 8 + 6 * 8 == 56 and (A.rank.offset, A.alpha.offset, A.a.offset, A.b.offset) == (0, 4, 8, 32)
    assert re.search(r"uint32_t rank, alpha;\s*const float \*a\[3\], \*b\[3\];\s*\} NanoLoraAdapter;", HEADER)
    D = nb.NanoLoraRowsOpDesc
    assert C.sizeof(D) == 6 * 4 + 8 * 8 + 3 * 8 == 112
    assert (D.E.offset, D.KD.offset, D.nb.offset, D.S.offset, D.v_bstride.offset, D.n_adapters.offset, D.x.offset, D.norm_w.offset, D.adapters.offset,
            D.row_adapter.offset, D.pos.offset, D.q.offset, D.kraw.offset, D.v.offset, D.q_floats.offset, D.k_floats.offset, D.v_floats.offset) == \
        (0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104)
    assert re.search(r"uint32_t E, KD, nb, S;\s*uint32_t v_bstride, n_adapters;\s*const float \*x;.*?const float \*norm_w;.*?const NanoLoraAdapter \*adapters;.*?"
                     r"const uint32_t \*row_adapter;.*?const uint32_t \*pos;.*?float \*q, \*kraw, \*v;.*?uint64_t q_floats, k_floats, v_floats;\s*\} NanoLoraRowsOpDesc;",
                     HEADER, re.S)


@pytest.mark.parametrize("preset", ["tiny-nano", "tiny-nano-odd"])
@pytest.mark.parametrize("rank", [1, 5, 8])
def test_param_floats_is_the_payload_of_a_module_file(tmp_path, preset, rank):
    spec = mf.preset(preset, "f32")
    path = str(tmp_path / "m.lora")
    mf.write_lora(path, spec, rank=rank, alpha=16, seed=3)
    payload = os.path.getsize(path) - 256
    assert payload % 4 == 0 and payload > 0
    assert nb.lora_param_floats(spec.n_layer, spec.n_embd, spec.kv_dim, rank) == payload // 4


def test_model_calls_refuse_a_null_model_and_null_arrays():
    L = nb.lib()
    p = np.zeros(16, np.float32)
    one = np.zeros(1, np.uint32)
    out = C.c_uint32(7)
    assert L.nano_hip_lora_table_set(None, 0, 4, 8, p.ctypes.data, p.size) == EINVAL
    assert L.nano_hip_lora_table_clear(None, 0) == EINVAL
    assert L.nano_hip_lora_bind(None, one.ctypes.data, one.ctypes.data, 1) == EINVAL
    assert L.nano_hip_lora_binding(None, 0, C.byref(out)) == EINVAL and out.value == 7
    for name in ("nano_lora_table_load_from_buffer", "nano_lora_table_free", "nano_lora_bind"):
        assert hasattr(L, name)
    assert L.nano_lora_table_load(None, 0, b"/nonexistent") == EINVAL
    assert L.nano_lora_table_load_from_buffer(None, 0, p.ctypes.data, 64) == EINVAL
    assert L.nano_lora_table_free(None, 0) == EINVAL
    assert L.nano_lora_bind(None, one.ctypes.data, one.ctypes.data, 1) == EINVAL


def test_model_calls_check_before_any_device_work():
    """the refusals of table_set and bind that need a model stand in front of the first device call, in the order the header lists them"""
    src = open(os.path.join(ROOT, "nano_amd", "csrc", "backend.hip")).read()
    end = src.index('extern "C" int nano_hip_lora_binding')
    set_ = src[src.index('extern "C" int nano_hip_lora_table_set'):src.index('extern "C" int nano_hip_lora_table_clear')]
    clear = src[src.index('extern "C" int nano_hip_lora_table_clear'):src.index('extern "C" int nano_hip_lora_bind(')]
    bind = src[src.index('extern "C" int nano_hip_lora_bind('):end]
    for needle in ("!params", "id >= NANO_LORA_TABLE_MAX", "NANO_ARCH_NANO", "m->lt.at.buf", "lora_shape_error(m->d.n_embd, rank)", "n_floats < total", "lora_entry_bound(m, id)"):
        assert set_.index(needle) < set_.index("hipSetDevice"), needle
    for needle in ("id >= NANO_LORA_TABLE_MAX", "lora_entry_bound(m, id)"):
        assert clear.index(needle) < clear.index("hipSetDevice"), needle
    for needle in ("!slots || !ids", "slots[i] >= m->maxB", "listed[slots[i]]", "ids[i] >= NANO_LORA_TABLE_MAX", "is empty", "NANO_ARCH_NANO"):
        assert bind.index(needle) < bind.index("hipSetDevice"), needle
    attach = src[src.index('extern "C" int nano_hip_lora_attach'):src.index('extern "C" int nano_hip_lora_enable')]
    assert attach.index("m->lt.n") < attach.index("hipSetDevice")          # a module after a table: refused before any device work


def desc(qkv=True, E=128, KD=64, ranks=(5, 8, 1), nb_=3, S=4, pos=(1, 3, 0), rows=(0, NONE, 2), v_slots=3, v_bstride=None, null=None,
         q_floats=None, k_floats=None, v_floats=None, n_adapters=None):
    rmax = min(max(max(ranks), 1), 64)
    keep = {n: np.zeros(sz, np.float32) for n, sz in (("x", nb_ * max(E, 1)), ("norm_w", max(E, 1)), ("A", rmax * max(E, 1)), ("B", max(E, KD, 1) * rmax),
                                                     ("q", nb_ * max(E, 1)), ("kraw", nb_ * max(KD, 1)), ("v", v_slots * S * max(KD, 1)))}
    keep["pos"] = np.ascontiguousarray(pos, np.uint32)
    keep["rows"] = np.ascontiguousarray(rows, np.uint32)
    ad = (nb.NanoLoraAdapter * len(ranks))()
    for i, r in enumerate(ranks):
        ad[i].rank, ad[i].alpha = r, 16
        for j in range(3 if qkv else 1):
            ad[i].a[j], ad[i].b[j] = keep["A"].ctypes.data, keep["B"].ctypes.data
    keep["ad"] = ad
    d = nb.NanoLoraRowsOpDesc()
    d.E, d.KD, d.nb, d.S = E, KD, nb_, S
    d.n_adapters = len(ranks) if n_adapters is None else n_adapters
    d.v_bstride = S * KD if v_bstride is None else v_bstride
    d.x, d.norm_w, d.pos, d.row_adapter = keep["x"].ctypes.data, keep["norm_w"].ctypes.data, keep["pos"].ctypes.data, keep["rows"].ctypes.data
    d.adapters = ad
    d.q, d.kraw, d.v = keep["q"].ctypes.data, keep["kraw"].ctypes.data, keep["v"].ctypes.data
    d.q_floats = nb_ * E if q_floats is None else q_floats
    d.k_floats = nb_ * KD if k_floats is None else k_floats
    d.v_floats = v_slots * S * KD if v_floats is None else v_floats
    if null in ("a1", "b2", "a0"):
        getattr(ad[1], null[0])[int(null[1])] = None
    elif null == "adapters":
        d.adapters = None
    elif null:
        setattr(d, null, None)
    return d, keep


def call(qkv=True, **kw):
    d, keep = desc(qkv, **kw)
    return (nb.lib().nano_hip_op_lora_qkv_rows if qkv else nb.lib().nano_hip_op_lora_o_rows)(0, C.byref(d))


def test_operators_refuse_before_they_ask_for_a_device():
    L = nb.lib()
    assert L.nano_hip_op_lora_qkv_rows(0, None) == EINVAL and L.nano_hip_op_lora_o_rows(0, None) == EINVAL
    for null in ("x", "norm_w", "pos", "q", "kraw", "v", "adapters", "row_adapter", "a1", "b2"):
        assert call(null=null) == EINVAL and "null" in nb.last_error(), null
    for null in ("x", "q", "adapters", "row_adapter", "a0"):
        assert call(qkv=False, null=null) == EINVAL, null
    for qkv in (True, False):
        assert call(qkv, E=130) == EINVAL and "% 4" in nb.last_error()
        assert call(qkv, ranks=(5, 0, 1)) == EINVAL and "rank" in nb.last_error()              # each adapter's rank, not only a used one
        assert call(qkv, E=8192, ranks=(1, 2721)) == EINVAL and "LDS" in nb.last_error()       # (8192 + 3 * 2721 + 32) * 4 = 65548 > 65536
        assert call(qkv, nb_=0, pos=(), rows=()) == EINVAL and call(qkv, nb_=65, pos=(0,) * 65, rows=(0,) * 65) == EINVAL
        assert call(qkv, n_adapters=0) == EINVAL and call(qkv, n_adapters=65) == EINVAL
        assert call(qkv, rows=(0, 3, 2)) == EINVAL and "adapter" in nb.last_error()            # neither an adapter nor NANO_LORA_NONE
        assert call(qkv, q_floats=3 * 128 - 1) == EINVAL
    assert call(KD=0) == EINVAL and call(k_floats=3 * 64 - 1) == EINVAL
    assert call(pos=(1, 4, 0)) == EINVAL and "beyond S" in nb.last_error()
    assert call(v_slots=2) == EINVAL and "v_floats" in nb.last_error()                         # row 2's slot is not in the buffer
    assert call(v_slots=1, v_bstride=0) != EINVAL                                              # ... as a chunk of one slot it is


def test_operators_have_no_host_path():
    """valid arguments: without a device no result (and no quiet host computation); with one, the launch runs"""
    if nb.device_count() > 0:
        assert call() == 0 and call(qkv=False) == 0
        return
    assert call() == ENODEV and call(qkv=False) == ENODEV
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(nb.NanoHipError):
        nb.op_lora_o_rows(z(2, 128), [(4, 8, ((z(4, 128), z(128, 4)),))], [0, None], z(2, 128))
    with pytest.raises(nb.NanoHipError):
        nb.op_lora_qkv_rows(z(1, 128), z(128), [(4, 8, ((z(4, 128), z(128, 4)), (z(4, 128), z(64, 4)), (z(4, 128), z(64, 4))))], [0], z(1, 128), z(1, 64),
                            z(1, 4, 64), [2], KD=64, S=4, v_bstride=256)
