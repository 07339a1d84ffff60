"""The FP8 KV cache's element format in numpy (include/nano_mi355x.h NANO_HIP_KV_FP8): OCP e4m3fn, one byte, scale 1.

  sign | 4 exponent bits (bias 7) | 3 mantissa bits; exponent 0: subnormals m * 2^-9; 0x7F / 0xFF: NaN; no infinities;
  largest finite +-448 (0x7E / 0xFE).
  write: byte = e4m3_rne(clamp(x, -448, 448)) -- round to nearest even, subnormals included, the sign of zero kept; out-of-range
  values and +-Inf saturate and never become a NaN code.  NaN inputs are outside the contract (here: 0x7F | sign).

tests/test_kv8_ref.py holds these two functions to torch.float8_e4m3fn on the CPU; the GPU tests hold the kernels to them."""
import numpy as np

E4M3_MAX = 448.0
NAN_CODES = (0x7F, 0xFF)


def _table():
    c = np.arange(256)
    ex, mt = (c >> 3) & 15, c & 7
    mag = np.where(ex == 0, mt * 2.0 ** -9, (8 + mt) * 2.0 ** (ex.astype(np.float64) - 10))
    mag = np.where((ex == 15) & (mt == 7), np.nan, mag)
    return np.where(c & 0x80, -mag, mag).astype(np.float32)


E4M3_TABLE = _table()                                                   # code -> value (float32, exact)


def e4m3_decode(codes):
    """uint8 codes -> float32 values (0x7F / 0xFF -> NaN)"""
    return E4M3_TABLE[np.asarray(codes, np.uint8)]


def e4m3_encode(x):
    """float32 -> uint8, the contract's write rule.  Every step below is exact in float64: a float32 scaled by a power of two."""
    x = np.asarray(x, np.float32)
    sign = np.signbit(x).astype(np.uint8) << 7
    a = np.minimum(np.abs(x.astype(np.float64)), E4M3_MAX)             # the clamp (Inf included); NaN stays NaN
    nan = np.isnan(a)
    a = np.where(nan, 0.0, a)
    _, ex = np.frexp(a)                                                 # a = m * 2^ex, m in [0.5, 1)
    e = np.where(a < 2.0 ** -6, -6, ex - 1)                             # binade of a; below 2^-6 (0 included): the subnormals' fixed step
    q = np.rint(np.ldexp(a, 3 - e)).astype(np.int64)                    # a in units of 2^(e - 3), to nearest EVEN: 0..8 (subnormal), 8..16
    code = ((e + 7) << 3) + (q - 8)                                     # q = 16 carries into the next exponent by itself; e = -6: the code IS q
    code = np.where(nan, 0x7F, code)                                    # (subnormals 0..7, and 8 = 2^-6, the first normal)
    return (code.astype(np.uint8) | sign).astype(np.uint8)


def finite_codes():
    return np.array([c for c in range(256) if c not in NAN_CODES], np.uint8)


def edge_values():
    """The contract's edges as float32: all 254 finite values, every midpoint between neighbours and one float32 step either side of
    each, +-0, +-448, +-464 (the first value e4m3 rounding alone would turn into NaN), +-1e4, 2^-10 (the tie between 0 and the smallest
    subnormal) and +-2^-10 (1 +- 2^-23)."""
    pos = np.sort(e4m3_decode(np.arange(0, 0x7F, dtype=np.uint8)).astype(np.float64))      # 0 .. 448, ascending
    mid = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)                 # (4 mantissa bits: exact in float32)
    assert np.array_equal(mid.astype(np.float64), (pos[:-1] + pos[1:]) / 2)
    lo, hi = np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))
    t = np.float32(2.0 ** -10)
    near = np.array([t, t * np.float32(1 + 2.0 ** -23), t * np.float32(1 - 2.0 ** -23)], np.float32)
    half = np.concatenate([pos.astype(np.float32), mid, lo, hi, np.array([448.0, 464.0, 1e4], np.float32), near])
    both = np.concatenate([half, -half, np.array([0.0, -0.0], np.float32)])
    return both.astype(np.float32)
