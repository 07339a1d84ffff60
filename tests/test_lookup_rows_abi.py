"""The C-ABI of lookup drafts for several sequences, without a device: the struct's layout, the symbols in the headers and the library,
the device-free planner against tests/lookup_rows_ref.py, and the NANO_HIP_EINVAL cases that are decided before a device is asked for."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import lookup_rows_ref as rr
from nano_amd import binding as nb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
S = 128


def test_struct_size_and_fields():
    Q = nb.NanoHipLookupSeq
    assert C.sizeof(Q) == 16
    assert [n for n, _ in Q._fields_] == ["slot", "n_history", "max_new", "reserved"]
    assert (Q.slot.offset, Q.n_history.offset, Q.max_new.offset, Q.reserved.offset) == (0, 4, 8, 12)


def test_symbols_in_headers_and_library():
    text = open(os.path.join(ROOT, "include", "nano_mi355x.h")).read()
    lib = nb.lib()
    for s in ("nano_hip_decode_lookup_rows", "nano_hip_lookup_rows_plan", "nano_hip_op_lookup_rows_round"):
        assert re.search(r"\bint\s+" + s + r"\s*\(", text), s
        assert hasattr(lib, s), s
    m = re.search(r"typedef struct NanoHipLookupSeq \{([^}]*)\} NanoHipLookupSeq;", text)
    assert m and re.findall(r"\w+", m.group(1).replace("uint32_t", "")) == [n for n, _ in nb.NanoHipLookupSeq._fields_]
    engine = open(os.path.join(ROOT, "include", "nano_infer_abi.h")).read()
    assert re.search(r"\bint\s+nano_decode_batch_lookup\s*\(", engine) and hasattr(lib, "nano_decode_batch_lookup")


def sweep():
    """n_seqs 1 .. 8, positions straddling 63 / 64 / 127, dead sequences, nb_next 1 and K"""
    rng = random.Random(5)
    edge = [1, 2, 5, 57, 62, 63, 64, 65, 66, 113, 120, 126, 127, 128]      # n: position n - 1 = 62 / 63 / 64 / 126 / 127 among them
    for B in range(1, 9):
        for K in (1, 2, 4, 8, 16):
            for _ in range(12):
                n, nb_next = [], []
                for _i in range(B):
                    rows = rng.choice([0, 1, K])
                    at = rng.choice(edge)
                    while rows and at - 1 + rows > S:
                        at = rng.choice(edge)
                    n.append(at); nb_next.append(rows)
                yield n, nb_next
    yield [64, 64, 65, 64], [1, 0, 1, 1]                                    # a dead sequence between equal hints
    yield [5, 5, 5], [0, 0, 0]                                              # nobody lives


def test_planner_agrees_with_the_python_planner():
    cases = 0
    for n, nb_next in sweep():
        fits_100 = all(a - 1 + b <= 100 for a, b in zip(n, nb_next) if b)     # (a clipped hint: max_seq_len no multiple of 64)
        for max_seq_len in ((S, 100) if fits_100 else (S,)):
            order, start, groups = nb.lookup_rows_plan(n, nb_next, max_seq_len)
            assert (order, start, groups) == rr.plan(n, nb_next, max_seq_len), (n, nb_next, max_seq_len)
            cases += 1
    assert cases >= 8 * 5 * 12 + 2                                          # (every case of the sweep at max_seq_len = S at least)


def test_planner_accepts_null_outputs_and_no_sequences():
    lib = nb.lib()
    n, b = np.array([64, 3], np.uint32), np.array([1, 8], np.uint32)
    ng = C.c_uint32(9)
    assert lib.nano_hip_lookup_rows_plan(n.ctypes.data, b.ctypes.data, 2, S, None, None, None, None, C.byref(ng)) == 0 and ng.value == 1
    assert lib.nano_hip_lookup_rows_plan(n.ctypes.data, b.ctypes.data, 2, S, None, None, None, None, None) == 0
    assert lib.nano_hip_lookup_rows_plan(None, None, 0, S, None, None, None, None, C.byref(ng)) == 0 and ng.value == 0


def test_planner_refusals():
    lib = nb.lib()
    n, b = np.array([64, 3], np.uint32), np.array([1, 8], np.uint32)
    ng = C.c_uint32(0)
    plan = lambda pn, pb, count, s: lib.nano_hip_lookup_rows_plan(pn, pb, count, s, None, None, None, None, C.byref(ng))
    assert plan(None, b.ctypes.data, 2, S) == EINVAL and plan(n.ctypes.data, None, 2, S) == EINVAL
    assert plan(n.ctypes.data, b.ctypes.data, 2, 0) == EINVAL
    for bad_n, bad_b in (([64, 3], [1, 17]), ([0, 3], [1, 8]), ([128, 3], [2, 8]), ([64, 122], [1, 8])):
        with pytest.raises(nb.NanoHipError, match="error -1"):
            nb.lookup_rows_plan(bad_n, bad_b, S)
    assert nb.lookup_rows_plan([0, 3], [0, 8], S)[0] == [1]                 # (a dead sequence's n is not looked at)
    with pytest.raises(ValueError):
        nb.lookup_rows_plan([1, 2], [1], S)


def _call(m, seqs, n_seqs, hist, p, out, n_out):
    return nb.lib().nano_hip_decode_lookup_rows(m, seqs, n_seqs, hist, p, out, n_out, None, None)


def test_null_model_and_null_arrays_are_refused():
    seqs = (nb.NanoHipLookupSeq * 1)(nb.NanoHipLookupSeq(0, 3, 4, 0))
    h, out, n = np.array([1, 2, 3], np.uint32), np.zeros(4, np.uint32), np.zeros(1, np.uint32)
    hp, op = (C.c_void_p * 1)(h.ctypes.data), (C.c_void_p * 1)(out.ctypes.data)
    p = nb.NanoHipLookupParams(7, 3, 1, 0xFFFFFFFF, 0)
    assert _call(None, seqs, 1, hp, C.byref(p), op, n.ctypes.data) == EINVAL
    assert "null" in nb.last_error()
    assert _call(None, None, 0, None, None, None, None) == EINVAL           # (a null model is refused whatever the count)


@pytest.mark.parametrize("kw", [dict(max_draft=16), dict(ngram_max=0), dict(ngram_max=5), dict(ngram_min=0), dict(ngram_min=3, ngram_max=2)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_op_refuses_parameters_before_any_device(kw):
    with pytest.raises(nb.NanoHipError, match="error -1"):
        nb.op_lookup_rows_round([[1, 2, 3]], [4], [0], **{"max_draft": 7, "ngram_max": 3, "ngram_min": 1, **kw})


def test_op_refuses_shapes_before_any_device():
    ok = dict(histories=[[1, 2, 3], [4, 5]], left=[4, 4], slots=[0, 1])
    for bad in (dict(slots=[1, 1]), dict(slots=[0, 64]), dict(histories=[[1, 2, 3], []]), dict(histories=[[1, 2, 3], [0] * 65537]),
                dict(fed=[1, 2], amax=[1, 2], row_start=[0, 1], nb=[1, 2]), dict(fed=[1] * 20, amax=[1] * 20, row_start=[0, 1], nb=[1, 17]),
                dict(max_seq_len=0)):
        with pytest.raises(nb.NanoHipError, match="error -1"):
            nb.op_lookup_rows_round(**{**ok, **bad})
    with pytest.raises(nb.NanoHipError, match="error -1"):
        nb.op_lookup_rows_round([], [], [])
    with pytest.raises(ValueError):
        nb.op_lookup_rows_round([[1, 2, 3]], [4], [0], fed=[1, 2], amax=[1])
    with pytest.raises(ValueError):
        nb.op_lookup_rows_round([[1, 2, 3]], [4, 4], [0])
