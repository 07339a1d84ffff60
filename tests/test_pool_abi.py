"""CPU tests of the text-embedding surface: the parameter block's layout, the exported symbols, and every refusal -- all of them happen
before a device is asked for (the operator) or need no device at all (a null model / context).  The operator has no host path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from nano_amd import binding as nb

EINVAL = -1


def test_params_layout():
    P = nb.NanoHipPoolParams
    assert C.sizeof(P) == 16
    assert (P.pooling.offset, P.normalize.offset, P.dim.offset, P.reserved.offset) == (0, 4, 8, 12)
    src = open(os.path.join(ROOT, "include", "nano_mi355x.h")).read()
    assert int(re.search(r"#define NANO_POOL_LAST (\d+)u", src).group(1)) == nb.POOL_LAST == 0
    assert int(re.search(r"#define NANO_POOL_MEAN (\d+)u", src).group(1)) == nb.POOL_MEAN == 1
    assert re.search(r"typedef struct NanoHipPoolParams \{ uint32_t pooling, normalize, dim, reserved; \}", src)


def test_symbols_are_exported():
    L = nb.lib()
    for name in ("nano_hip_step_rows_pool", "nano_hip_rows_pool_plan", "nano_hip_op_pool_rows", "nano_embed_batch"):
        assert hasattr(L, name), name
    assert callable(nb.DeviceModel.step_rows_pool) and callable(nb.op_pool_rows) and callable(nb.rows_pool_plan)
    src = open(os.path.join(ROOT, "include", "nano_infer_abi.h")).read()
    assert "int nano_embed_batch(Nano_Context *ctx" in src


def op(x=True, w=True, counts=(2, 1), rows=3, n_embd=8, p=(0, 1, 0, 0), pass_cap=64, out=True, n_segs=None, params=True):
    xv, wv = np.zeros((max(rows, 1), max(n_embd, 1)), np.float32), np.ones(max(n_embd, 1), np.float32)
    c = np.ascontiguousarray(counts, np.uint32)
    o = np.zeros((len(counts) + 1) * max(n_embd, 1), np.float32)
    pp = nb.NanoHipPoolParams(*p)
    return nb.lib().nano_hip_op_pool_rows(0, xv.ctypes.data if x else None, rows, n_embd, wv.ctypes.data if w else None,
                                          c.ctypes.data if counts is not None else None, len(counts) if n_segs is None else n_segs,
                                          C.byref(pp) if params else None, pass_cap, o.ctypes.data if out else None)


def test_operator_refuses_before_it_asks_for_a_device():
    assert op(x=False) == EINVAL and op(w=False) == EINVAL and op(out=False) == EINVAL and op(params=False) == EINVAL
    assert op(n_segs=0) == EINVAL and op(n_embd=0) == EINVAL
    assert op(rows=4) == EINVAL and "sum" in nb.last_error()                  # rows is not the sum of the counts
    assert op(p=(2, 1, 0, 0)) == EINVAL                                       # pooling > 1
    assert op(p=(0, 2, 0, 0)) == EINVAL                                       # normalize > 1
    assert op(p=(0, 1, 9, 0)) == EINVAL                                       # dim > n_embd
    assert op(p=(0, 1, 0, 1)) == EINVAL                                       # reserved != 0
    assert op(pass_cap=0) == EINVAL and op(pass_cap=257) == EINVAL


def test_operator_has_no_host_path():
    if nb.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(nb.NanoHipError):
        nb.op_pool_rows(np.zeros((3, 8), np.float32), np.ones(8, np.float32), [2, 1])
    assert op() == -3                                                         # valid arguments: no device, no result
    assert op(p=(1, 0, 8, 0), pass_cap=1) == -3


def test_model_entry_points_refuse_a_null_model():
    L = nb.lib()
    tok = np.zeros(4, np.uint32)
    seg = nb.row_segs([(0, 0, 4)])
    out = np.zeros(64, np.float32)
    for p in ((0, 1, 0, 0), (2, 1, 0, 0), (0, 2, 0, 0), (0, 1, 0, 1), (1, 0, 0xffffffff, 0)):
        pp = nb.NanoHipPoolParams(*p)
        assert L.nano_hip_step_rows_pool(None, seg.ctypes.data, 1, tok.ctypes.data, C.byref(pp), out.ctypes.data) == EINVAL, p
    pp = nb.NanoHipPoolParams(0, 1, 0, 0)
    assert L.nano_hip_step_rows_pool(None, seg.ctypes.data, 1, tok.ctypes.data, None, out.ctypes.data) == EINVAL
    assert L.nano_hip_step_rows_pool(None, seg.ctypes.data, 1, tok.ctypes.data, C.byref(pp), None) == EINVAL
    assert L.nano_hip_step_rows_pool(None, None, 0, None, C.byref(pp), out.ctypes.data) == EINVAL
    ptrs = (C.c_void_p * 1)(tok.ctypes.data)
    n = np.array([4], np.uint32)
    assert L.nano_embed_batch(None, ptrs, n.ctypes.data, 1, 0, 1, 0, out.ctypes.data) == EINVAL      # null context
