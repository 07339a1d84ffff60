"""The C-ABI of greedy decode with lookup drafts, without a device: struct sizes, the symbols in header and library, and the
NANO_HIP_EINVAL cases that are decided before a device is asked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from nano_amd import binding as nb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nano_hip_decode_lookup", "nano_hip_verify_draft", "nano_hip_op_lookup_step")
EINVAL = -1


def test_struct_sizes_and_fields():
    assert C.sizeof(nb.NanoHipLookupParams) == 20 and C.sizeof(nb.NanoHipLookupStats) == 20
    assert [n for n, _ in nb.NanoHipLookupParams._fields_] == ["max_draft", "ngram_max", "ngram_min", "stop_token", "max_steps"]
    assert [n for n, _ in nb.NanoHipLookupStats._fields_] == ["steps_plain", "steps_verify", "drafted", "accepted", "emitted"]
    assert len(nb.LOOKUP_RECORD_FIELDS) == 8


def test_symbols_in_header_and_library():
    text = open(os.path.join(ROOT, "include", "nano_mi355x.h")).read()
    lib = nb.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", text), s
        assert hasattr(lib, s), s
    for t in ("NanoHipLookupParams", "NanoHipLookupStats"):
        assert re.search(r"typedef struct " + t + r" \{[^}]*\} " + t + ";", text), t
    m = re.search(r"typedef struct NanoHipLookupParams \{([^}]*)\}", text)
    assert re.findall(r"uint32_t\s+(\w+);", m.group(1)) == [n for n, _ in nb.NanoHipLookupParams._fields_]


def _params(**kw):
    d = dict(max_draft=7, ngram_max=3, ngram_min=1, stop_token=0xFFFFFFFF, max_steps=0)
    d.update(kw)
    return nb.NanoHipLookupParams(*(d[n] for n, _ in nb.NanoHipLookupParams._fields_))


def test_null_model_is_refused():
    lib = nb.lib()
    h = np.array([1, 2, 3], np.uint32)
    out, n = np.zeros(8, np.uint32), C.c_uint32(0)
    p = _params()
    assert lib.nano_hip_decode_lookup(None, h.ctypes.data, 3, 4, C.byref(p), out.ctypes.data, C.byref(n), None) == EINVAL
    assert lib.nano_hip_verify_draft(None, 0, h.ctypes.data, 0, 3, out.ctypes.data, None) == EINVAL
    assert "null" in nb.last_error()


@pytest.mark.parametrize("kw", [dict(max_draft=16), dict(ngram_max=0), dict(ngram_max=5), dict(ngram_min=0), dict(ngram_min=3, ngram_max=2)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_op_refuses_parameters_before_any_device(kw):
    with pytest.raises(nb.NanoHipError, match="error -1"):
        nb.op_lookup_step([1, 2, 3], left=4, **{"max_draft": 7, "ngram_max": 3, "ngram_min": 1, **kw})


def test_op_refuses_shapes_before_any_device():
    lib = nb.lib()
    h = np.zeros(64, np.uint32)
    rec, nt, npos = np.zeros(8, np.uint32), np.zeros(16, np.uint32), np.zeros(16, np.uint32)
    p = _params()
    args = lambda hist, n, fed, amax, nrows, pp, r: (0, hist, n, fed, amax, nrows, pp, 4, 1 << 20, r, nt.ctypes.data, npos.ctypes.data)
    ok = (h.ctypes.data, 3, None, None, 0, C.byref(p), rec.ctypes.data)
    for bad in ((None,) + ok[1:], ok[:5] + (None,) + ok[6:], ok[:6] + (None,), (ok[0], 0) + ok[2:], (ok[0], 65537) + ok[2:],
                ok[:2] + (None, None, 2) + ok[5:], ok[:2] + (h.ctypes.data, h.ctypes.data, 17) + ok[5:]):
        assert lib.nano_hip_op_lookup_step(*args(*bad)) == EINVAL, bad
    with pytest.raises(ValueError):
        nb.op_lookup_step([1, 2, 3], [1, 2], [1], left=4)
