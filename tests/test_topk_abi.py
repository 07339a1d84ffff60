"""CPU tests of the top-k surface: the record's layout, and every entry point's refusals -- all of them happen before a device is
asked for (the operator) or need no device at all (a null model).  The operator has no host path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from nano_amd import binding as nb

EINVAL = -1


def test_record_layout():
    E = nb.NanoHipTopEntry
    assert C.sizeof(E) == 12 and (E.token.offset, E.logit.offset, E.logprob.offset) == (0, 4, 8)
    d = nb.TOP_ENTRY_DTYPE
    assert d.itemsize == 12 and [d.fields[n][1] for n in ("token", "logit", "logprob")] == [0, 4, 8]
    assert [d.fields[n][0] for n in ("token", "logit", "logprob")] == [np.dtype("<u4"), np.dtype("<f4"), np.dtype("<f4")]
    src = open(os.path.join(ROOT, "include", "nano_mi355x.h")).read()
    assert int(re.search(r"#define NANO_TOPK_MAX (\d+)u", src).group(1)) == nb.TOPK_MAX == 32


def test_symbols_are_exported():
    L = nb.lib()
    for name in ("nano_hip_op_topk_rows", "nano_hip_prefill_score_topk", "nano_hip_forward_topk", "nano_hip_step_rows_score",
                 "nano_score_ids_topk", "nano_forward_batch_topk"):
        assert hasattr(L, name), name


def op(logits, rows, V, k, targets=None, scores=True, top=True):
    l = np.ascontiguousarray(logits, np.float32)
    sc = np.zeros(max(rows, 1), nb.TOKEN_SCORE_DTYPE)
    tp = np.zeros(max(rows, 1) * max(k, 1), nb.TOP_ENTRY_DTYPE)
    t = None if targets is None else np.ascontiguousarray(targets, np.uint32)
    return nb.lib().nano_hip_op_topk_rows(0, l.ctypes.data if logits is not None else None, rows, V, k, None if t is None else t.ctypes.data,
                                          sc.ctypes.data if scores else None, tp.ctypes.data if top else None)


def test_operator_refuses_before_it_asks_for_a_device():
    l = np.zeros((2, 40), np.float32)
    assert op(None, 2, 40, 5) == EINVAL
    assert op(l, 2, 40, 5, top=False) == EINVAL
    assert op(l, 0, 40, 5) == EINVAL and op(l, 2, 0, 5) == EINVAL and op(l, 2, 40, 0) == EINVAL
    assert op(l, 2, 40, 33) == EINVAL and "NANO_TOPK_MAX" in nb.last_error()
    assert op(l[:, :5], 2, 5, 6) == EINVAL                                  # k > V
    assert op(l, 2, 40, 5, targets=[3, 40]) == EINVAL and "target" in nb.last_error()


def test_operator_has_no_host_path():
    if nb.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(nb.NanoHipError):
        nb.op_topk_rows(np.zeros((1, 8), np.float32), 3)
    assert op(np.zeros((2, 40), np.float32), 2, 40, 5, scores=False) == -3  # valid arguments (scores_out may be NULL): no device, no result


def test_model_entry_points_refuse_a_null_model():
    L = nb.lib()
    tok = np.zeros(4, np.uint32)
    sc = np.zeros(4, nb.TOKEN_SCORE_DTYPE)
    tp = np.zeros(4 * 32, nb.TOP_ENTRY_DTYPE)
    seg = nb.row_segs([(0, 0, 4)])
    assert L.nano_hip_prefill_score_topk(None, 0, tok.ctypes.data, 0, 4, None, 5, sc.ctypes.data, tp.ctypes.data) == EINVAL
    assert L.nano_hip_forward_topk(None, tok.ctypes.data, tok.ctypes.data, 4, None, 5, sc.ctypes.data, tp.ctypes.data) == EINVAL
    assert L.nano_hip_step_rows_score(None, seg.ctypes.data, 1, tok.ctypes.data, None, 5, sc.ctypes.data, tp.ctypes.data) == EINVAL
    nll = C.c_double(0.0)
    ti, tl = np.zeros(4 * 32, np.uint32), np.zeros(4 * 32, np.float32)
    assert L.nano_score_ids_topk(None, tok.ctypes.data, 4, 5, None, None, ti.ctypes.data, tl.ctypes.data, C.byref(nll)) == EINVAL
    assert L.nano_forward_batch_topk(None, tok.ctypes.data, tok.ctypes.data, 4, 5, ti.ctypes.data, tl.ctypes.data, None) == EINVAL
