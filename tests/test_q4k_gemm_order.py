"""CPU test: the arithmetic of the Q4K MFMA GEMM (nano_amd/csrc/gemm_q4k.hip), restated in numpy, against the oracle's matmul_q4k
(reference infer/tensor.c:359-434 dot_two_blocks_q4k, 438-471 matmul_q4k) -- and why K may be divided between the waves of a workgroup
at BLOCK granularity only.

The kernel's model:
  * the three integer sums of a 32-value group are taken over the PERMUTED nibble order the MFMA operands use (a packed dword w goes
    in as w & 0x0f0f0f0f, then (w >> 4) & 0x0f0f0f0f: the low nibbles of four bytes, then their high nibbles) -- integer sums are
    exact in any order;
  * the four-term expression sp*sq*(float)sum_pq - sp*bq*(float)sum_p - sq*bp*(float)sum_q + 32*bp*bq in float32, one operation at a
    time, in the association of gemv_q4k_chunk_body.inc;
  * the 8 group values of a block added in order into a sum that starts at 0; the block sums FILED in a table and folded in
    ascending block order, the row walked in rounds of R blocks (the table holds one round).
That is bit for bit the oracle for every R.  A second model that lets two waves each pre-add the lines of half a row and adds the two
lines is NOT: float addition does not associate, so lines must not be pre-added per wave."""
import numpy as np
import pytest
from fused_ref import bits

f32 = np.float32
NS = (256, 768, 2560)
ROWS, ACTS, SEED = 16, 3, 5


def unpack6(sb):
    """the 8 six-bit scales and biases of a block from its 12 packed bytes (tensor.c:120-135)"""
    sb = sb.astype(np.uint32)
    s6, b6 = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    for i in range(4):
        s6[i] = sb[i] & 0x3f
        s6[i + 4] = (((sb[i] >> 6) << 4) | (sb[8 + i] & 0x0f)) & 0x3f
        b6[i] = sb[4 + i] & 0x3f
        b6[i + 4] = (((sb[4 + i] >> 6) << 4) | ((sb[8 + i] & 0xf0) >> 4)) & 0x3f
    return s6, b6


def parse(T, rows, n):
    """framed Q4K tensor -> per (row, group): scale, bias (float32) and the 32 nibbles in the MFMA operand's k order"""
    bpl = n // 256
    blocks = T[44:].reshape(rows, bpl, 160)
    sc = np.zeros((rows, bpl * 8), f32); bi = np.zeros((rows, bpl * 8), f32)
    nib = np.zeros((rows, bpl * 8, 32), np.int64)
    for r in range(rows):
        for j in range(bpl):
            blk = blocks[r, j]
            s_scale, s_bias = blk[12:16].view(f32)[0], blk[16:20].view(f32)[0]
            s6, b6 = unpack6(blk[20:32])
            for g in range(8):
                sc[r, j * 8 + g] = f32(s6[g]) * s_scale
                bi[r, j * 8 + g] = f32(b6[g]) * s_bias
                w = blk[32 + 16 * g:48 + 16 * g].view(np.uint32)            # the group's four packed dwords
                k = []
                for d in w:                                                 # lane quarter kq takes dword kq: low nibbles, then high nibbles
                    k += [(int(d) >> (8 * i)) & 0x0f for i in range(4)] + [(int(d) >> (8 * i + 4)) & 0x0f for i in range(4)]
                nib[r, j * 8 + g] = k
    return sc, bi, nib


def block_sums(W, X, n):
    """[row][block] block sums of one activation: every float32 operation on its own"""
    wsc, wbi, wn = W
    xsc, xbi, xn = X
    bpl = n // 256
    out = np.zeros((wsc.shape[0], bpl), f32)
    for r in range(wsc.shape[0]):
        for j in range(bpl):
            dot = f32(0)
            for g in range(8):
                G = j * 8 + g
                sp, bp, sq, bq = wsc[r, G], wbi[r, G], xsc[0, G], xbi[0, G]
                spq, su, sumq = int((wn[r, G] * xn[0, G]).sum()), int(wn[r, G].sum()), int(xn[0, G].sum())
                t0 = f32(f32(sp * sq) * f32(spq))
                t1 = f32(f32(sp * bq) * f32(su))
                t2 = f32(f32(sq * bp) * f32(sumq))
                t3 = f32(f32(f32(32) * bp) * bq)
                dot = f32(dot + f32(f32(f32(t0 - t1) - t2) + t3))
            out[r, j] = dot
    return out


def fold_rounds(D, R):
    """the kernel: rounds of R blocks, each round's block sums folded ascending into the line"""
    rows, bpl = D.shape
    line = np.zeros(rows, f32)
    for j0 in range(0, bpl, R):
        table = D[:, j0:j0 + R].copy()                                      # what the round files in LDS
        for j in range(table.shape[1]):
            line = (line + table[:, j]).astype(f32)
    return line


def fold_half_lines(D):
    """NOT the kernel: two waves pre-add the lines of half a row each, the halves are added"""
    rows, bpl = D.shape
    h = (bpl + 1) // 2
    a, b = np.zeros(rows, f32), np.zeros(rows, f32)
    for j in range(h):
        a = (a + D[:, j]).astype(f32)
    for j in range(h, bpl):
        b = (b + D[:, j]).astype(f32)
    return (a + b).astype(f32)


@pytest.fixture(scope="module")
def cases(oracle):
    out = []
    for n in NS:
        rng = np.random.default_rng(SEED + n)
        WT = oracle.quantize_q4k((0.02 * rng.standard_normal(ROWS * n)).astype(f32), [ROWS, n])
        W = parse(WT, ROWS, n)
        for t in range(ACTS):
            x = (rng.standard_normal(n) * 2).astype(f32)
            XT = oracle.quantize_q4k(x, [n])
            out.append((n, t, oracle.matmul_q4k(XT, WT, 0, ROWS), block_sums(W, parse(XT, 1, n), n)))
    return out


@pytest.mark.parametrize("R", [1, 3, 8])
def test_block_granular_rounds_are_the_reference_bits(cases, R):
    for n, t, ref, D in cases:
        got = fold_rounds(D, R)
        assert np.array_equal(bits(got), bits(ref)), (n, t, R, float(np.abs(got - ref).max()))


def test_pre_added_half_row_lines_are_not(cases):
    """seed pinned on the CPU: at least one of these inputs moves when lines are pre-added per wave (one block: nothing to split)"""
    moved = [(n, t) for n, t, ref, D in cases if not np.array_equal(bits(fold_half_lines(D)), bits(ref))]
    assert moved, "pre-added half-row lines matched the reference on every input: pick another seed"
    assert all(n > 256 for n, t in moved)
