"""The scoring prefill's C-ABI surface, without a device: the record's layout, the argument checks that need no GPU, and the absence of a
host path."""
import ctypes as C

import numpy as np
import pytest

from nano_amd import binding as nb

NANO_HIP_EINVAL = -1


def test_token_score_layout():
    assert C.sizeof(nb.NanoHipTokenScore) == 24
    offsets = [getattr(nb.NanoHipTokenScore, n).offset for n in ("logprob", "target_logit", "max_logit", "lse", "argmax", "rank")]
    assert offsets == [0, 4, 8, 12, 16, 20]
    assert nb.TOKEN_SCORE_DTYPE.itemsize == 24
    assert [nb.TOKEN_SCORE_DTYPE.fields[n][1] for n in ("logprob", "target_logit", "max_logit", "lse", "argmax", "rank")] == offsets


def test_null_arguments_are_refused_without_a_device():
    L = nb.lib()
    tok = np.zeros(4, np.uint32); out = np.zeros(4, nb.TOKEN_SCORE_DTYPE); lg = np.zeros((4, 8), np.float32)
    assert L.nano_hip_prefill_score(None, 0, tok.ctypes.data, 0, 4, None, out.ctypes.data) == NANO_HIP_EINVAL
    assert L.nano_hip_op_score_rows(0, None, 4, 8, None, out.ctypes.data) == NANO_HIP_EINVAL
    assert L.nano_hip_op_score_rows(0, lg.ctypes.data, 4, 8, None, None) == NANO_HIP_EINVAL
    assert L.nano_hip_op_score_rows(0, lg.ctypes.data, 0, 8, None, out.ctypes.data) == NANO_HIP_EINVAL
    assert L.nano_hip_op_score_rows(0, lg.ctypes.data, 4, 0, None, out.ctypes.data) == NANO_HIP_EINVAL
    bad = np.array([0, 1, 8, 2], np.uint32)                   # a target >= V
    assert L.nano_hip_op_score_rows(0, lg.ctypes.data, 4, 8, bad.ctypes.data, out.ctypes.data) == NANO_HIP_EINVAL
    assert nb.last_error()


def test_score_rows_has_no_host_path():
    if nb.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(nb.NanoHipError):
        nb.op_score_rows(np.zeros((2, 16), np.float32), [1, 2])
