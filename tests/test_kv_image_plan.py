"""CPU tests of the KV image's host side (include/nano_mi355x.h "KV images"): nano_hip_kv_image_plan and nano_hip_kv_image_check use no
device, and their arithmetic is tests/kv_image_ref.py's plain restatement of the layout.  A missing symbol fails these tests."""
import ctypes as C
import struct

import numpy as np
import pytest

import kv_image_ref as kr
from nano_amd import binding as nb

N_POS = [0, 1, 63, 64, 65, 128, 129, 255, 256]
KV_DIMS = [4, 8, 12, 16, 36, 64, 128]


def test_entry_points_are_exported_and_bound():
    for name in ("nano_hip_kv_image_plan", "nano_hip_kv_image_bytes", "nano_hip_kv_image_check", "nano_hip_kv_save", "nano_hip_kv_restore",
                 "nano_kv_image_bytes", "nano_kv_save", "nano_kv_restore"):
        assert hasattr(nb.lib(), name), name
    for cls in (nb.DeviceModel, nb.Engine):
        assert callable(cls.kv_save) and callable(cls.kv_restore) and callable(cls.kv_image_bytes)
    assert C.sizeof(nb.NanoKvImageHeader) == kr.HEADER_BYTES == 64


def test_plan_query_equals_the_restated_layout():
    widths = set()
    for n_layer in range(1, 5):
        for kv_dim in KV_DIMS:
            for eb in (4, 2, 1):
                for n_pos in N_POS:
                    got, want = nb.kv_image_plan(n_layer, kv_dim, eb, n_pos), kr.plan(n_layer, kv_dim, eb, n_pos)
                    assert got == want, (n_layer, kv_dim, eb, n_pos)
                    widths.add(got["vec_bytes"])
                    # the blocks tile the payload: block b starts where the formula says, the last row of the last run ends the image
                    rb = kv_dim * eb
                    if n_pos:
                        last = got["blocks"] - 1
                        assert kr.offset(n_layer, rb, n_pos, last, 0, 0, 0) == 64 + last * got["block_stride"]
                        assert kr.offset(n_layer, rb, n_pos, last, n_layer - 1, 1, got["last_rows"] - 1) + rb == got["total_bytes"]
    assert widths == {16, 8, 4}


def test_plan_query_refuses_what_is_no_cache():
    out = (C.c_uint64 * 8)()
    L = nb.lib()
    assert L.nano_hip_kv_image_plan(2, 16, 4, 10, None) == -1
    for n_layer, kv_dim, eb in ((0, 16, 4), (2, 0, 4), (2, 6, 4), (2, 16, 3), (2, 16, 0), (2, 16, 8)):
        assert L.nano_hip_kv_image_plan(n_layer, kv_dim, eb, 10, out) == -1, (n_layer, kv_dim, eb)
        assert "KV image plan" in nb.last_error()


def random_image(rng, fmt, n_layer, kv_dim, n_pos, tag=0x1234):
    rb = kv_dim * kr.FMT_BYTES[fmt]
    k = rng.integers(0, 256, (n_layer, n_pos, rb), dtype=np.uint8)
    v = rng.integers(0, 256, (n_layer, n_pos, rb), dtype=np.uint8)
    return k, v, kr.write(k, v, fmt, tag)


@pytest.mark.parametrize("fmt,kv_dim", [(0, 16), (1, 36), (2, 12)])
@pytest.mark.parametrize("n_pos", [0, 1, 64, 129])
def test_check_accepts_the_reference_writers_image(fmt, kv_dim, n_pos):
    k, v, img = random_image(np.random.default_rng(n_pos + kv_dim), fmt, 3, kv_dim, n_pos)
    h = nb.kv_image_check(img)
    assert (h["magic"], h["version"], h["header_bytes"], h["block_rows"]) == (struct.unpack("<I", kr.MAGIC)[0], 1, 64, 64)
    assert (h["format"], h["n_layer"], h["kv_dim"], h["n_pos"], h["row_bytes"]) == (fmt, 3, kv_dim, n_pos, kv_dim * kr.FMT_BYTES[fmt])
    assert h["payload_bytes"] == img.size - 64 and h["model_tag"] == 0x1234 and h["reserved0"] == 0 and h["reserved1"] == [0, 0]
    assert nb.kv_image_check(img.tobytes())["n_pos"] == n_pos             # bytes as well as arrays
    hh, k2, v2 = kr.read(img)
    assert np.array_equal(k, k2) and np.array_equal(v, v2) and hh["n_pos"] == n_pos


def patched(img, word, value, fmt="<I"):
    out = img.copy()
    out[4 * word:4 * word + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), np.uint8)
    return out


def test_check_refuses_each_corruption():
    _, _, img = random_image(np.random.default_rng(5), 1, 2, 36, 70)
    nb.kv_image_check(img)
    bad = {
        "short: less than the header": img[:63],
        "short: less than header and payload": img[:-1],
        "bad magic": patched(img, 0, 0x3256_4B4E),
        "bad version": patched(img, 1, 2),
        "bad header size": patched(img, 2, 128),
        "block rows": patched(img, 7, 32),
        "row_bytes": patched(img, 8, 36 * 4),
        "format unknown": patched(img, 3, 3),
        "payload bytes": patched(img, 10, img.size - 64 - 72, "<Q"),
        "reserved word 9": patched(img, 9, 1),
        "reserved word 14": patched(img, 14, 1),
        "reserved word 15": patched(img, 15, 7),
    }
    for what, b in bad.items():
        with pytest.raises(nb.NanoHipError, match="KV image"):
            nb.kv_image_check(b)
        assert nb.lib().nano_hip_kv_image_check(b.ctypes.data, b.size, None) == -1, what
    # a format change alone breaks row_bytes; with row_bytes and the payload following it the image is well-formed (and another cache's)
    assert nb.lib().nano_hip_kv_image_check(patched(img, 3, 0).ctypes.data, img.size, None) == -1
    assert nb.lib().nano_hip_kv_image_check(None, 64, None) == -1
    # longer buffers are fine: the header says where the image ends
    assert nb.kv_image_check(np.concatenate([img, np.zeros(5, np.uint8)]))["n_pos"] == 70


@pytest.mark.parametrize("fmt,kv_dim", [(0, 8), (1, 36), (2, 12)])
def test_prefix_image_is_the_byte_prefix_plus_the_row_cut(fmt, kv_dim):
    k, v, img = random_image(np.random.default_rng(11), fmt, 3, kv_dim, 129)
    stride = nb.kv_image_plan(3, kv_dim, kr.FMT_BYTES[fmt], 129)["block_stride"]
    for n in (0, 1, 63, 64, 65, 70, 128, 129):
        want = kr.write(k[:, :n], v[:, :n], fmt, 0x1234)
        cut = kr.prefix(img, n)
        assert np.array_equal(cut, want), n
        nb.kv_image_check(cut)
        full = n // 64
        assert np.array_equal(want[64:64 + full * stride], img[64:64 + full * stride])        # whole blocks: the same bytes at the same place
