"""CPU tests of the shared-prefix surface: the library exports nano_hip_kv_fork, nano_hip_kv_sharing (include/nano_mi355x.h) and
nano_prefill_shared (include/nano_infer_abi.h), and each refuses a null model with NANO_HIP_EINVAL before it touches a device."""
import ctypes as C

import numpy as np

from nano_amd import binding as nb

NANO_HIP_EINVAL = -1


def raw(name, argtypes):
    f = getattr(C.CDLL(nb.LIB_PATH), name)                     # a prototype of its own: the binding's array types refuse None
    f.restype, f.argtypes = C.c_int, argtypes
    return f


def test_library_exports_the_shared_prefix_entries():
    L = nb.lib()
    for name in ("nano_hip_kv_fork", "nano_hip_kv_sharing", "nano_prefill_shared"):
        assert hasattr(L, name), name
    assert callable(nb.DeviceModel.kv_fork) and callable(nb.DeviceModel.kv_sharing) and callable(nb.Engine.prefill_shared)


def test_null_model_is_einval_without_a_device():
    dst = np.array([1], np.uint32)
    fork = raw("nano_hip_kv_fork", [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32])
    assert fork(None, 0, 1, dst.ctypes.data, 1) == NANO_HIP_EINVAL
    assert "null" in nb.last_error()
    assert fork(None, 0, 1, None, 0) == NANO_HIP_EINVAL
    shared, cows = C.c_uint32(7), C.c_uint64(7)
    sharing = raw("nano_hip_kv_sharing", [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)])
    assert sharing(None, C.byref(shared), C.byref(cows)) == NANO_HIP_EINVAL
    assert (shared.value, cows.value) == (7, 7)                # nothing written
    prefill = raw("nano_prefill_shared", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32])
    assert prefill(None, dst.ctypes.data, 1, 4) == NANO_HIP_EINVAL
