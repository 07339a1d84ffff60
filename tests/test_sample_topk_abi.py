"""CPU tests of the sampler's top-k surface (include/nano_mi355x.h "top-k truncation"): the two entry points are exported, the row
struct's layout is pinned, and null arguments are refused -- with a null model that happens before a device is asked for."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from nano_amd import binding as nb

EINVAL = -1


def test_symbols_are_exported():
    L = nb.lib()
    for name in ("nano_hip_forward_sample_batch_ex", "nano_hip_op_sample_batch_ex"):
        assert hasattr(L, name), name


def test_row_layout():
    P, X = nb.NanoHipSampleParams, nb.NanoHipSampleParamsEx
    assert C.sizeof(P) == 32                                                 # unchanged: four floats, a pointer, a word, padding
    assert C.sizeof(X) == 48 and (X.p.offset, X.top_k.offset, X.reserved.offset) == (0, 32, 36) and X.reserved.size == 12
    src = open(os.path.join(ROOT, "include", "nano_mi355x.h")).read()
    body = re.search(r"typedef struct NanoHipSampleParamsEx \{(.*?)\} NanoHipSampleParamsEx;", src, re.S).group(1)
    assert [w for w in re.findall(r"(\w+)(?:\[\d+\])?;", body)] == ["p", "top_k", "reserved"]


def test_null_arguments_are_refused():
    L = nb.lib()
    prm, _keep = nb.sample_params_ex([(1.0, 1.0, 0.9, 0.5, [])], 20)
    out = (nb.NanoHipSample * 1)()
    tok = np.zeros(1, np.uint32)
    logits = np.zeros(8, np.float32)
    assert L.nano_hip_forward_sample_batch_ex(None, tok, tok, 1, prm, out) == EINVAL and "null" in nb.last_error()
    assert L.nano_hip_op_sample_batch_ex(None, logits, 1, prm, out) == EINVAL and "null" in nb.last_error()
    assert L.nano_hip_forward_sample_batch_ex(None, tok, tok, 1, None, None) == EINVAL
    assert L.nano_hip_op_sample_batch_ex(None, logits, 1, None, None) == EINVAL
    # the entry points without top_k are callers of these: the same refusals
    old, _keep2 = nb.sample_params([(1.0, 1.0, 0.9, 0.5, [])])
    assert L.nano_hip_forward_sample_batch(None, tok, tok, 1, old, out) == EINVAL and "null" in nb.last_error()
    assert L.nano_hip_op_sample_batch(None, logits, 1, old, out) == EINVAL
    assert L.nano_hip_op_sample_batch(None, logits, 1, None, out) == EINVAL
    assert L.nano_hip_op_sample_batch(None, logits, 1000, old, out) == EINVAL


def test_helpers_default_to_top_k_off():
    arr, _keep = nb.sample_params_ex([(1.1, 0.7, 0.8, 0.25, [3, 4]), (1.0, 1.0, 0.9, 0.5, [])], [0, 20])
    assert [(a.top_k, tuple(a.reserved), a.p.n_history) for a in arr] == [(0, (0, 0, 0), 2), (20, (0, 0, 0), 0)]
    one, _keep = nb.sample_params_ex([(1.0, 1.0, 0.9, 0.5, [])] * 3, 7)
    assert [a.top_k for a in one] == [7, 7, 7]
    import inspect
    for f in (nb.DeviceModel.forward_sample, nb.DeviceModel.op_sample, nb.DeviceModel.forward_sample_batch, nb.DeviceModel.op_sample_batch):
        assert inspect.signature(f).parameters["top_k"].default == 0, f.__name__
