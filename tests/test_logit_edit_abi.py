"""CPU tests of the logit-edit surface (include/nano_mi355x.h "logit edits", include/nano_infer_abi.h): the binding's structs and constant
are the headers', the entry points are exported, and a null model is refused before a device is asked for."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from nano_amd import binding as nb

EINVAL = -1


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_symbols_are_exported():
    L = nb.lib()
    for name in ("nano_hip_forward_sample_batch_edit", "nano_hip_op_sample_batch_edit", "nano_hip_mask_table_set", "nano_set_logit_edit",
                 "nano_forward_batch_sample_edit"):
        assert hasattr(L, name), name


def test_struct_layouts_are_the_headers():
    src = header("nano_mi355x.h")
    assert int(re.search(r"#define NANO_BIAS_MAX (\d+)u", src).group(1)) == nb.NANO_BIAS_MAX == 1024
    B, E, X = nb.NanoHipLogitBias, nb.NanoHipSampleParamsEdit, nb.NanoHipSampleParamsEx
    assert C.sizeof(B) == 8 and (B.token.offset, B.bias.offset) == (0, 4)
    assert C.sizeof(X) == 48                                                 # unchanged
    assert C.sizeof(E) == 72 and (E.ex.offset, E.allow.offset, E.bias.offset, E.mask_id.offset, E.n_bias.offset) == (0, 48, 56, 64, 68)
    body = re.search(r"typedef struct NanoHipSampleParamsEdit \{(.*?)\} NanoHipSampleParamsEdit;", re.sub(r"/\*.*?\*/", "", src, flags=re.S), re.S).group(1)
    assert re.findall(r"(\w+);", body) == ["ex", "allow", "bias", "mask_id", "n_bias"] == [f for f, _ in E._fields_]
    body = re.search(r"typedef struct NanoHipLogitBias \{(.*?)\} NanoHipLogitBias;", src, re.S).group(1)
    assert re.findall(r"(\w+);", body) == ["token", "bias"] == [f for f, _ in B._fields_]
    eng = header("nano_infer_abi.h")
    body = re.search(r"typedef struct NanoLogitEdit \{(.*?)\} NanoLogitEdit;", eng, re.S).group(1)
    N = nb.NanoLogitEdit
    assert re.findall(r"(\w+);", body) == ["allow", "bias_tokens", "bias_values", "n_bias"] == [f for f, _ in N._fields_]
    assert C.sizeof(N) == 32 and (N.allow.offset, N.bias_tokens.offset, N.bias_values.offset, N.n_bias.offset) == (0, 8, 16, 24)


def test_a_null_model_is_refused_without_a_device():
    L = nb.lib()
    prm, _keep = nb.sample_params_edit([(1.0, 1.0, 0.9, 0.5, [])], 0, [{"allow": np.full(1, 0xF, np.uint32), "bias": ([1], [0.5])}])
    out = (nb.NanoHipSample * 1)()
    tok = np.zeros(1, np.uint32)
    logits = np.zeros(8, np.float32)
    assert L.nano_hip_forward_sample_batch_edit(None, tok, tok, 1, prm, out) == EINVAL and "null" in nb.last_error()
    assert L.nano_hip_op_sample_batch_edit(None, logits, 1, prm, out) == EINVAL and "null" in nb.last_error()
    assert L.nano_hip_op_sample_batch_edit(None, logits, 1, None, None) == EINVAL
    w = np.full(1, 1, np.uint32)
    assert L.nano_hip_mask_table_set(None, w.ctypes.data, 1) == EINVAL and "null" in nb.last_error()
    L.nano_set_logit_edit.restype = C.c_int
    L.nano_set_logit_edit.argtypes = [C.c_void_p, C.c_void_p]
    assert L.nano_set_logit_edit(None, None) == EINVAL


def test_helper_builds_rows():
    w = nb.mask_words([0, 33], 40)
    assert w.tolist() == [1, 2]
    assert nb.mask_words(np.arange(40) == 39, 40).tolist() == [0, 1 << 7]
    arr, _keep = nb.sample_params_edit([(1.1, 0.7, 0.8, 0.25, [3, 4]), (1.0, 1.0, 0.9, 0.5, []), (1.0, 1.0, 0.9, 0.5, [])], [0, 20, 0],
                                       [None, {"allow": w, "bias": ([5, 2], [1.0, -2.0])}, {"mask_id": 2}])
    assert [(a.ex.top_k, a.mask_id, a.n_bias, bool(a.allow), bool(a.bias)) for a in arr] == [(0, 0, 0, False, False), (20, 0, 2, True, True), (0, 2, 0, False, False)]
    assert (arr[1].bias[0].token, arr[1].bias[0].bias, arr[1].bias[1].token, arr[1].bias[1].bias) == (5, 1.0, 2, -2.0)
    assert arr[1].allow[1] == 2 and arr[0].ex.p.n_history == 2
    import inspect
    for f in (nb.DeviceModel.forward_sample_batch, nb.DeviceModel.op_sample_batch):
        assert inspect.signature(f).parameters["edits"].default is None, f.__name__
