"""The C-ABI of greedy decode with a draft model, without a device: struct sizes, the symbols in header and library with the stated
signatures, and the NANO_HIP_EINVAL cases that are decided before a device is asked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from nano_amd import binding as nb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def header():
    return open(os.path.join(ROOT, "include", "nano_mi355x.h")).read()


def test_struct_sizes_and_fields():
    assert C.sizeof(nb.NanoHipDraftParams) == 16 and C.sizeof(nb.NanoHipDraftStats) == 28
    assert [n for n, _ in nb.NanoHipDraftParams._fields_] == ["max_draft", "stop_token", "max_rounds", "draft_held"]
    assert [n for n, _ in nb.NanoHipDraftStats._fields_] == ["rounds_plain", "rounds_verify", "drafted", "accepted", "emitted", "draft_rows_fed", "draft_held"]
    assert len(nb.DRAFT_RECORD_FIELDS) == 8
    text = header()
    for cls in (nb.NanoHipDraftParams, nb.NanoHipDraftStats):
        m = re.search(r"typedef struct " + cls.__name__ + r" \{(.*?)\} " + cls.__name__ + ";", text, re.S)
        assert m, cls.__name__
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        names = [n.strip() for decl in re.findall(r"uint32_t\s+([^;]+);", body) for n in decl.split(",")]
        assert names == [n for n, _ in cls._fields_]


def test_symbols_and_signatures():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = nb.lib()
    want = {
        "nano_hip_decode_draft": ["NanoHipModel *target", "NanoHipModel *draft", "const uint32_t *history", "uint32_t n_history", "uint32_t max_new",
                                  "const NanoHipDraftParams *p", "uint32_t *out_ids", "uint32_t *n_out", "NanoHipDraftStats *stats"],
        "nano_hip_op_draft_round": ["int device", "uint32_t *history", "uint32_t n", "const uint32_t *fed", "const uint32_t *amax", "uint32_t nb",
                                    "const NanoHipDraftParams *params", "uint32_t left", "uint32_t seq_limit", "uint32_t dn", "uint32_t *record_out",
                                    "uint32_t *next_tokens_out", "uint32_t *next_pos_out"],
    }
    for name, args in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == args
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == len(args)
    assert hasattr(nb.DeviceModel, "decode_draft") and hasattr(nb, "op_draft_round")
    abi = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nano_infer_abi.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+nano_set_draft_model\s*\(\s*const char \*path\s*,\s*int max_draft\s*\)\s*;", abi) and hasattr(lib, "nano_set_draft_model")


def test_null_arguments_are_refused_before_any_device():
    lib = nb.lib()
    h = np.array([1, 2, 3], np.uint32)
    out, n = np.zeros(8, np.uint32), C.c_uint32(7)
    p = nb.NanoHipDraftParams(4, 0xFFFFFFFF, 0, 0)
    st = nb.NanoHipDraftStats()
    fake = C.c_void_p(0)
    assert lib.nano_hip_decode_draft(None, None, h.ctypes.data, 3, 4, C.byref(p), out.ctypes.data, C.byref(n), C.byref(st)) == EINVAL
    assert "null" in nb.last_error()
    assert lib.nano_hip_decode_draft(fake, fake, None, 3, 4, None, None, None, None) == EINVAL
    assert n.value == 7                                                      # nothing was written


def test_op_refuses_before_any_device():
    lib = nb.lib()
    h = np.zeros(64, np.uint32)
    rec, nt, npos = np.zeros(8, np.uint32), np.zeros(16, np.uint32), np.zeros(16, np.uint32)
    p = nb.NanoHipDraftParams(4, 0xFFFFFFFF, 0, 0)
    p16 = nb.NanoHipDraftParams(16, 0xFFFFFFFF, 0, 0)
    call = lambda hist, n, fed, amax, rows, pp, dn, r: lib.nano_hip_op_draft_round(0, hist, n, fed, amax, rows, pp, 4, 1 << 20, dn, r, nt.ctypes.data, npos.ctypes.data)
    ok = (h.ctypes.data, 3, None, None, 0, C.byref(p), 0, rec.ctypes.data)
    for bad in ((None,) + ok[1:], ok[:5] + (None,) + ok[6:], ok[:7] + (None,), (ok[0], 0) + ok[2:], (ok[0], 65537) + ok[2:],
                ok[:2] + (None, None, 2) + ok[5:], ok[:2] + (h.ctypes.data, h.ctypes.data, 17) + ok[5:], ok[:5] + (C.byref(p16),) + ok[6:],
                ok[:6] + (3,) + ok[7:]):
        assert call(*bad) == EINVAL, bad
    with pytest.raises(ValueError):
        nb.op_draft_round([1, 2, 3], [1, 2], [1], left=4)
    with pytest.raises(nb.NanoHipError, match="error -1"):
        nb.op_draft_round([1, 2, 3], left=4, max_draft=16)
    with pytest.raises(nb.NanoHipError, match="error -1"):
        nb.op_draft_round([1, 2, 3], left=4, dn=3)
