"""The in-wave fold of the chunks of Q80 rows of 2, 3 and 4 chunks (nano_amd/csrc/gemv_q80_impl.h wave_fold_canon16_units and the
unit-sum fold of gemv_q80_slab_body.inc SLAB_WFC), restated lane by lane in numpy with the kernel's own add order, against
tests/canon.py.  No GPU needed.

The wave of a unit holds four rows x one chunk: for chunk c, lane 4 g + r has the product of (row r, group 16 c + g).  It runs the
one-chunk schedule (tests/test_wave_fold_order.py) up to the v_permlane32_swap, which leaves S_2c beside S_2c+1 in lanes 48 + r; those
lanes park the two sums, and the fold thread of the row adds

    chunk 0        v = S_0 + S_1
    chunk c > 0    v = (v + S_2c) + S_2c+1

Every step is ONE fp32 add with the running value as the first operand, so the row value must be canon.py's
((S_0 + S_1) + S_2) + ... of row r for every input: random rows, signed zeros and denormals in every lane position."""
import numpy as np
import pytest

from canon import matmul_q80_canon
from test_wave_fold_order import F, fadd, permlane16_swap_first, permlane32_swap_first, row_shl, same_bits

CHUNKS = [2, 3, 4]


def wave_fold_units(p):
    """p[64] of one chunk -> (s0[64], s1[64]): in lanes 48 + r the two unit sums of row r"""
    p = np.asarray(p, F)
    p1, p2, p3 = row_shl(p, 4), row_shl(p, 8), row_shl(p, 12)
    s = fadd(fadd(fadd(p, p1), p2), p3)
    c = permlane16_swap_first(s, s)
    s = fadd(fadd(fadd(fadd(c, p), p1), p2), p3)
    return permlane32_swap_first(s, s), s


def wave_fold_chunks(prod):
    """prod[4, 16 nch] -> the four row values: per chunk the two unit sums of lanes 48..51, added as the fold thread adds them"""
    nch = prod.shape[1] // 16
    v = None
    for c in range(nch):
        p = np.zeros(64, F)
        for g in range(16):
            for r in range(4):
                p[4 * g + r] = prod[r, 16 * c + g]
        s0, s1 = wave_fold_units(p)
        v = fadd(s0, s1) if c == 0 else fadd(fadd(v, s0), s1)
    return v[48:52]


def canon_rows(prod):
    """canon.py's fold on products given directly (test_canon_rows_is_canon_py ties the two together)"""
    out = None
    for u in range(prod.shape[1] // 8):
        s = prod[:, 8 * u].copy()
        for k in range(1, 8):
            s = fadd(s, prod[:, 8 * u + k])
        out = s if out is None else fadd(out, s)
    return out


@pytest.mark.parametrize("nch", CHUNKS)
def test_canon_rows_is_canon_py(nch):
    rng = np.random.default_rng(nch)
    rows, n = 4, 1024 * nch
    ng = n // 64
    wq = rng.integers(-127, 128, size=rows * n, dtype=np.int8)
    ws = rng.uniform(1e-4, 2e-3, size=rows * ng).astype(F)
    xq = rng.integers(-127, 128, size=n, dtype=np.int8)
    xs = rng.uniform(1e-3, 1e-1, size=ng).astype(F)
    ival = np.einsum("rgk,gk->rg", wq.reshape(rows, ng, 64).astype(np.int32), xq.reshape(ng, 64).astype(np.int32))
    prod = ((ival.astype(F) * ws.reshape(rows, ng)).astype(F) * xs[None, :]).astype(F)
    want = matmul_q80_canon(xq, xs, wq, ws, n, rows)
    assert same_bits(canon_rows(prod), want)
    assert same_bits(wave_fold_chunks(prod), want)


@pytest.mark.parametrize("nch", CHUNKS)
def test_wave_fold_chunks_random_rows(nch):
    rng = np.random.default_rng(20 + nch)
    for trial in range(300):
        scale = F(10.0) ** rng.integers(-30, 30)
        prod = (rng.standard_normal((4, 16 * nch)) * scale).astype(F)
        assert same_bits(wave_fold_chunks(prod), canon_rows(prod)), trial


@pytest.mark.parametrize("nch", CHUNKS)
def test_wave_fold_chunks_zeros_and_denormals_in_every_lane_position(nch):
    """one special product (-0, +0, the smallest denormal of either sign, a larger denormal) at every (row, group) of the tile, among
    ordinary products, among denormal products, and alone among -0s"""
    rng = np.random.default_rng(40 + nch)
    tiny = np.nextafter(F(0), F(1))
    specials = [F(-0.0), F(0.0), tiny, -tiny, F(3e-40), F(-3e-40)]
    ng = 16 * nch
    grounds = [(rng.standard_normal((4, ng)) * 1e-3).astype(F), (rng.integers(-40, 41, size=(4, ng)).astype(F) * tiny).astype(F),
               np.full((4, ng), -0.0, F)]
    for gi, ground in enumerate(grounds):
        for g in range(ng):
            for r in range(4):
                for sp in specials:
                    prod = ground.copy()
                    prod[r, g] = sp
                    assert same_bits(wave_fold_chunks(prod), canon_rows(prod)), (gi, g, r, float(sp))


@pytest.mark.parametrize("nch", CHUNKS)
def test_wave_fold_chunks_adversarial_rows(nch):
    ng = 16 * nch
    tiny = np.nextafter(F(0), F(1))
    z = np.zeros((4, ng), F)
    cases = [z.copy(), (-z).copy()]                          # +0 everywhere; -0 everywhere: the row is -0 (no chain starts from +0.0)
    for c in range(nch):                                     # a whole unit / a whole chunk of -0 next to ordinary ones, and the reverse
        m = np.ones((4, ng), F); m[:, 16 * c: 16 * c + 8] = -0.0; cases.append(m)
        m = np.ones((4, ng), F); m[:, 16 * c: 16 * c + 16] = -0.0; cases.append(m)
        m = np.full((4, ng), -0.0, F); m[:, 16 * c + 8: 16 * c + 16] = tiny; cases.append(m)
    d = np.full((4, ng), tiny, F); d[1] = -tiny; d[2, ::2] = -tiny; cases.append(d)      # denormals, exact cancellation of denormals
    t = z.copy(); t[:, 0] = 1.0; t[:, 1:] = F(2.0) ** -24; cases.append(t)                 # every add is a tie: association shows
    t2 = z.copy(); t2[:, ng - 1] = 1.0; t2[:, :ng - 1] = F(2.0) ** -25; cases.append(t2)
    one = (np.arange(4 * ng, dtype=F).reshape(ng, 4).T + 1.0).astype(F); cases.append(one)   # a wrong lane map shows as a wrong sum
    w = ((F(1.5) ** np.arange(ng, dtype=F))[None, :] * np.arange(1, 5, dtype=F)[:, None]).astype(F); cases.append(w)
    for k, prod in enumerate(cases):
        assert same_bits(wave_fold_chunks(prod), canon_rows(prod)), k
    assert np.all(wave_fold_chunks(cases[1]).view(np.uint32) == 0x80000000)


@pytest.mark.parametrize("nch", CHUNKS)
def test_orders_differ_from_other_shapes(nch):
    """the inputs can tell the canonical shape from a single ascending chain and from a pairwise tree of the chunks' sums"""
    ng = 16 * nch
    prod = np.zeros((4, ng), F); prod[:, 7] = 1.0; prod[:, :7] = F(2.0) ** -24; prod[:, 8:] = F(2.0) ** -25
    chain = prod[:, 0].copy()
    for g in range(1, ng):
        chain = fadd(chain, prod[:, g])
    assert not same_bits(chain, canon_rows(prod))
    # (S_0 + S_1) + (S_2 + S_3) is not ((S_0 + S_1) + S_2) + S_3
    p2 = np.zeros((4, ng), F); p2[:, 0] = 1.0; p2[:, 16] = F(2.0) ** -24; p2[:, 24] = F(2.0) ** -24
    tree = fadd(fadd(p2[:, 0], p2[:, 8]), fadd(p2[:, 16], p2[:, 24]))
    assert not same_bits(tree, canon_rows(p2)[:4])
    assert same_bits(wave_fold_chunks(prod), canon_rows(prod)) and same_bits(wave_fold_chunks(p2), canon_rows(p2))
