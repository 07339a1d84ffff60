"""The in-wave canonical fold of one-chunk Q80 rows (nano_amd/csrc/gemv_q80_impl.h wave_fold_canon16), restated lane by lane in numpy
with the kernel's own add order, against tests/canon.py.  No GPU needed.

A wave holds one unit of four rows: lane 4 g + r has the product of (row r, group g), g = 0..15.  The kernel's schedule:

    p1, p2, p3 = p moved by DPP row_shl:4 / 8 / 12        lane l reads lane l + 4 k of its own 16-lane row (0.0 beyond the row)
    s = ((p + p1) + p2) + p3                               lanes r | 32 + r: groups 0..3 | 8..11
    c = s of the even 16-lane rows carried to the odd rows (v_permlane16_swap), s = (((c + p) + p1) + p2) + p3
                                                           lanes 16 + r | 48 + r: S_0 | S_1
    s0 = s of lanes 0..31 carried to lanes 32..63 (v_permlane32_swap), row = s0 + s        lanes 48 + r

Every step is ONE fp32 add with the running value as the first operand, so the float in lane 48 + r must be canon.py's
(S_0 + S_1) of row r for every input: random rows, signed zeros, denormals, cancellation, infinities."""
import numpy as np

from canon import matmul_q80_canon

F = np.float32


def row_shl(v, k):
    """DPP row_shl:k with bound_ctrl: lane l of a 16-lane row reads lane l + k of the same row, 0.0 beyond it"""
    out = np.zeros(64, F)
    for lane in range(64):
        if (lane % 16) + k < 16:
            out[lane] = v[lane + k]
    return out


def permlane16_swap_first(a, b):
    """v_permlane16_swap a, b -> a: its odd 16-lane rows are replaced by b's even rows (row 1 <- row 0, row 3 <- row 2)"""
    out = a.copy()
    out[16:32] = b[0:16]
    out[48:64] = b[32:48]
    return out


def permlane32_swap_first(a, b):
    """v_permlane32_swap a, b -> a: its upper 32 lanes are replaced by b's lower 32"""
    out = a.copy()
    out[32:64] = b[0:32]
    return out


def fadd(a, b):
    with np.errstate(all="ignore"):
        return (a.astype(F) + b.astype(F)).astype(F)


def wave_fold(p):
    """p[64]: lane 4 g + r = product (row r, group g) -> the four row values (lanes 48..51)"""
    p = np.asarray(p, F)
    p1, p2, p3 = row_shl(p, 4), row_shl(p, 8), row_shl(p, 12)
    s = fadd(fadd(fadd(p, p1), p2), p3)
    c = permlane16_swap_first(s, s)
    s = fadd(fadd(fadd(fadd(c, p), p1), p2), p3)
    s0 = permlane32_swap_first(s, s)
    return fadd(s0, s)[48:52]


def canon_rows(prod):
    """prod[4, 16] fp32 group products -> canon.py's fold of them (its loop, on products given directly: canon.py forms its own from
    int8 inputs, which cannot produce infinities or chosen signed zeros; test_canon_rows_is_canon_py ties the two together)"""
    out = None
    for u in range(2):
        s = prod[:, 8 * u].copy()
        for k in range(1, 8):
            s = fadd(s, prod[:, 8 * u + k])
        out = s if out is None else fadd(out, s)
    return out


def lanes_of(prod):
    p = np.zeros(64, F)
    for g in range(16):
        for r in range(4):
            p[4 * g + r] = prod[r, g]
    return p


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | nan))


def test_canon_rows_is_canon_py():
    """the helper above is tests/canon.py: the same rows through matmul_q80_canon (integer sums x weight scales x activation scales)"""
    rng = np.random.default_rng(1)
    rows, n = 4, 1024
    wq = rng.integers(-127, 128, size=rows * n, dtype=np.int8)
    ws = rng.uniform(1e-4, 2e-3, size=rows * 16).astype(F)
    xq = rng.integers(-127, 128, size=n, dtype=np.int8)
    xs = rng.uniform(1e-3, 1e-1, size=16).astype(F)
    ival = np.einsum("rgk,gk->rg", wq.reshape(rows, 16, 64).astype(np.int32), xq.reshape(16, 64).astype(np.int32))
    prod = ((ival.astype(F) * ws.reshape(rows, 16)).astype(F) * xs[None, :]).astype(F)
    want = matmul_q80_canon(xq, xs, wq, ws, n, rows)
    assert same_bits(canon_rows(prod), want)
    assert same_bits(wave_fold(lanes_of(prod)), want)


def test_wave_fold_random_rows():
    rng = np.random.default_rng(2)
    for trial in range(400):
        scale = F(10.0) ** rng.integers(-30, 30)
        prod = (rng.standard_normal((4, 16)) * scale).astype(F)
        assert same_bits(wave_fold(lanes_of(prod)), canon_rows(prod)), trial


def test_wave_fold_adversarial_rows():
    tiny = np.nextafter(F(0), F(1))                        # the smallest denormal
    big = F(3.0e38)
    cases = []
    z = np.zeros((4, 16), F)
    cases.append(z.copy())                                 # +0 everywhere
    cases.append((-z).copy())                              # -0 everywhere: the sum of -0s is -0, a chain started from +0.0 would give +0
    m = z.copy(); m[:, ::2] = -0.0; cases.append(m)        # mixed signed zeros
    d = z.copy(); d[:, :] = tiny; d[1] = -tiny; d[2, ::2] = -tiny; cases.append(d)          # denormals, exact cancellation of denormals
    c = z.copy(); c[:, 0] = 1.0; c[:, 1:] = F(2.0) ** -24; cases.append(c)                # every add is a tie: association shows
    c2 = z.copy(); c2[:, 7] = 1.0; c2[:, :7] = F(2.0) ** -24; c2[:, 8:] = F(2.0) ** -25; cases.append(c2)
    o = z.copy(); o[:, 0] = big; o[:, 1] = big; o[:, 2] = -big; cases.append(o)            # overflow inside a unit: inf, then inf - big
    o2 = z.copy(); o2[:, 0] = big; o2[:, 8] = big; cases.append(o2)                        # overflow only in S_0 + S_1
    i = z.copy(); i[0, 3] = np.inf; i[1, 3] = np.inf; i[1, 12] = -np.inf; cases.append(i)  # inf; inf - inf across the units -> NaN
    a = z.copy()
    for r in range(4):
        a[r] = [(-1.0) ** g * (1.0 + g * 2.0 ** -20) * 10.0 ** (r - 1) for g in range(16)]  # alternating signs: cancellation
    cases.append(a.astype(F))
    one = z.copy(); one[:, :] = np.arange(64, dtype=F).reshape(16, 4).T + 1.0; cases.append(one)   # lane order: a wrong lane map shows as a wrong sum
    w = z.copy(); w[:, :] = (F(2.0) ** np.arange(16, dtype=F))[None, :] * np.arange(1, 5, dtype=F)[:, None]; cases.append(w)
    for k, prod in enumerate(cases):
        with np.errstate(all="ignore"):
            assert same_bits(wave_fold(lanes_of(prod.astype(F))), canon_rows(prod.astype(F))), k


def test_wave_fold_orders_differ_from_other_shapes():
    """the inputs above can tell the canonical shape from the reference's single ascending chain (so the comparison is not vacuous)"""
    prod = np.zeros((4, 16), F); prod[:, 7] = 1.0; prod[:, :7] = F(2.0) ** -24; prod[:, 8:] = F(2.0) ** -25
    chain = prod[:, 0].copy()
    for g in range(1, 16):
        chain = fadd(chain, prod[:, g])
    assert not same_bits(chain, canon_rows(prod))
    assert same_bits(wave_fold(lanes_of(prod)), canon_rows(prod))
