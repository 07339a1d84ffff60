"""tests/kv8_ref.py (the FP8 KV cache's e4m3fn write and read rules in numpy) against torch.float8_e4m3fn on the CPU, and the option's
public surface.  torch rounds to nearest even with subnormals, but turns values beyond the format's range into NaN (500.0 -> NaN), so
the contract's clamp comes first on that side as well."""
import os

import numpy as np
import torch

import kv8_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_encode(x):
    t = torch.from_numpy(np.asarray(x, np.float32).copy()).clamp(-448.0, 448.0)
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_decode_matches_torch_on_all_256_codes():
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    got = kv8_ref.e4m3_decode(codes)
    assert np.isnan(got[[0x7F, 0xFF]]).all() and np.isnan(want[[0x7F, 0xFF]]).all()
    fin = kv8_ref.finite_codes()
    assert len(fin) == 254
    assert np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32))
    assert got[0x7E] == 448.0 and got[0xFE] == -448.0 and got[0x01] == 2.0 ** -9 and got[0x08] == 2.0 ** -6
    assert got[0x00] == 0.0 and not np.signbit(got[0x00]) and np.signbit(got[0x80])


def test_encode_matches_torch_on_every_edge():
    x = kv8_ref.edge_values()
    assert len(x) == 2 * (127 + 3 * 126 + 3 + 3) + 2
    got, want = kv8_ref.e4m3_encode(x), torch_encode(x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(x[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    assert not np.isin(got, kv8_ref.NAN_CODES).any()                   # nothing finite becomes a NaN code


def test_encode_contract_points():
    enc = kv8_ref.e4m3_encode
    f = np.float32
    assert list(enc(f([0.0, -0.0]))) == [0x00, 0x80]                    # the sign of zero is kept
    assert list(enc(f([448, -448, 464, -464, 1e4, -1e4, np.inf, -np.inf]))) == [0x7E, 0xFE] * 4      # saturation, Inf included
    t = f(2.0 ** -10)                                                   # the tie between 0 and the smallest subnormal: to even = 0
    assert list(enc(f([t, -t]))) == [0x00, 0x80]
    assert list(enc(f([t * f(1 + 2.0 ** -23), -t * f(1 + 2.0 ** -23)]))) == [0x01, 0x81]
    assert list(enc(f([t * f(1 - 2.0 ** -23), -t * f(1 - 2.0 ** -23)]))) == [0x00, 0x80]
    assert list(enc(f([3 * 2.0 ** -10, 5 * 2.0 ** -10]))) == [0x02, 0x02]                            # subnormal ties go to the even code
    assert list(enc(f([1.0625, 1.1875, 7.5 * 2.0 ** -9]))) == [0x38, 0x3A, 0x08]                      # normal ties; the subnormals' carry into 2^-6
    fin = kv8_ref.finite_codes()
    assert np.array_equal(enc(kv8_ref.e4m3_decode(fin)), fin)           # every finite value is a fixed point
    x = np.random.default_rng(8).standard_normal(4096).astype(np.float32) * f(3.0)
    assert np.array_equal(enc(x), torch_encode(x))


def test_fp8_kv_cache_is_declared_bound_and_documented():
    """The public surface of the option: the flag in the C header, the environment switch in INTEGRATION.md's knob table, the keyword
    in the Python binding."""
    hdr = open(os.path.join(ROOT, "include", "nano_mi355x.h")).read()
    assert "#define NANO_HIP_KV_FP8 4u" in hdr
    assert "#define NANO_HIP_KV_F16 1u" in hdr and "#define NANO_HIP_KV_PAGED 2u" in hdr      # (the existing flags keep their values)
    knobs = [ln for ln in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if ln.startswith("| `NANO_KV_FP8=1`")]
    assert len(knobs) == 1, "NANO_KV_FP8 has no row in INTEGRATION.md's knob table"
    for doc in ("DESIGN.md", "README.md"):
        assert "NANO_KV_FP8" in open(os.path.join(ROOT, doc)).read(), doc
    import inspect

    from nano_amd import binding as nb
    for fn in (nb.DeviceModel.__init__, nb.load_model_file):
        p = inspect.signature(fn).parameters
        assert "kv_fp8" in p and p["kv_fp8"].default is None, fn
        assert "kv_f16" in p and "kv_paged" in p
