"""The in-wave fold of the chunks of Q80 rows of 2, 3 and 4 chunks on the device (gemv_q80_slab_body.inc SLAB_WFC, gemv_q80_impl.h
wave_fold_canon16_units): at n = 2048 / 3072 / 4096, group size 64, one sequence, the residual roles (Wo, W2; Wo also behind the
split-attention combine) the wave of a unit (four rows x one chunk) folds its chunk to the chunk's two unit sums and leaves 8 floats in
LDS -- no product table -- and the fold thread of a row adds the row's unit sums in ascending order behind the barrier.  The bits must
be those of tests/canon.py, which the table route (two sequences and more) is held to as well.

Through the operator C-ABI (nano_hip_op_fused_gemv, the step's own router) and, for the residual stream of a whole step, through a
model run with plain and with fused launches.  tests/test_wave_fold_chunks_order.py restates the lane schedule itself on the CPU.
Reference lines: quantize tensor.c:21-46, matmul_quant infer.c:654-679, residual adds infer.c:906-908 / 963-965."""
import numpy as np
import pytest

from canon import matmul_q80_canon
from nano_amd import binding as nb
from nano_amd import modelfile as mf
from fused_ref import bits, order_free

pytestmark = pytest.mark.gpu

Q80, GS = 0x80, 64
F = np.float32


def weights(rng, rows, n):
    wq = rng.integers(-127, 128, size=rows * n, dtype=np.int8)
    ws = rng.uniform(1e-4, 2e-3, size=rows * n // GS).astype(F)
    return wq, ws


def resid_case(oracle, n, seg, x, old, attn=None, act=None):
    """one residual launch, one sequence: old + canon.py bit for bit in EVERY row, route "gemv"; the same inputs as two sequences (the
    product table's route; plain activations) carry the same bits in both sequences"""
    rows = seg[2]
    xq, xs = oracle.quantize_q80(x if act is None else act, GS)
    want = (old + matmul_q80_canon(xq, xs, seg[0], seg[1], n, rows, GS)).astype(F)
    one, route = nb.op_fused_gemv(Q80, 1, n, [seg], None if attn is not None else x[None], None, gs=GS, resid=old[None], attn=attn, want_route=True)
    assert route == "gemv", route
    assert one.shape == (1, rows)
    bad = np.flatnonzero(bits(one[0]) != bits(want))
    assert bad.size == 0, (n, rows, bad.size, bad[:8], one[0][bad[:8]], want[bad[:8]])
    if attn is None:
        two = nb.op_fused_gemv(Q80, 1, n, [seg], np.stack([x, x]), None, gs=GS, nb=2, resid=np.stack([old, old]))
        assert np.array_equal(bits(two[0]), bits(one[0])) and np.array_equal(bits(two[1]), bits(one[0]))
    return one[0]


# Wo of Qwen3-0.6B (8 rows per workgroup: two tiles x two chunks = four units); W2 (4 rows: one tile, three chunks); four chunks (still
# below the 8 M weights of the wide plans); 1030 rows -> 5 rows per workgroup (the second tile has three dead rows); 2050 rows -> a ragged
# last workgroup; 7 rows: a last workgroup with a dead row
@pytest.mark.parametrize("n,rows", [(2048, 1024), (3072, 1024), (4096, 1024), (2048, 1030), (3072, 7), (2048, 2050)], ids=str)
def test_residual_role_is_canon(oracle, n, rows):
    rng = np.random.default_rng(n + rows)
    x = (order_free(rng, n) * F(3)).astype(F)                 # (no norm in front of these launches: any values would do)
    old = rng.standard_normal(rows).astype(F)
    resid_case(oracle, n, (*weights(rng, rows, n), rows), x, old)


@pytest.mark.parametrize("nch", [2, 3])
def test_signed_zero_and_denormal_products(oracle, nch):
    """the rows of test_gpu_wave_fold.py's test of the same name at 2 and 3 chunks: the special groups in chunk 0 only (rows 0..63) and in
    the last chunk only (rows 64..127), whole rows of zeros and of denormals, and a whole unit of -0 in every unit position (rows 128...).
    old = -0.0, so the stored bits show the row's own sign: an all-(-0) row must come out 0x80000000 (no chain may start from +0.0)"""
    rng = np.random.default_rng(50 + nch)
    n, ng = 1024 * nch, 16 * nch
    rows = 128 + 2 * nch
    wq, ws = weights(rng, rows, n)
    wq = wq.reshape(rows, ng, GS).copy(); ws = ws.reshape(rows, ng).copy()
    for base, c0 in ((0, 0), (64, nch - 1)):
        g0 = 16 * c0
        R = lambda r: base + r
        wq[R(0)] = 0; ws[R(0)] = -ws[R(0)]                                   # every product of the row -0
        wq[R(1)] = 0                                                         # every product +0
        wq[R(2)] = 0; ws[R(2), ::2] = -ws[R(2), ::2]                         # alternating -0 / +0
        wq[R(3), g0:g0 + 8] = 0; ws[R(3), g0:g0 + 8] = -ws[R(3), g0:g0 + 8]                  # the chunk's first unit -0, the rest ordinary
        wq[R(4), g0 + 8:g0 + 16] = 0; ws[R(4), g0 + 8:g0 + 16] = -ws[R(4), g0 + 8:g0 + 16]   # its second unit -0
        ws[R(5)] = F(1e-43)                                                  # denormal scales: denormal products and sums, the whole row
        ws[R(6)] = F(3e-44); ws[R(6), ::3] = -F(3e-44)                       # ... of both signs, cancelling
        ws[R(7), :] = F(1e-43); ws[R(7), g0] = F(1e-3)                       # one ordinary group in the chunk, the others denormal
        ws[R(8), g0:g0 + 16] = F(1e-36)                                      # the chunk's products near the smallest normal number
        wq[R(9), g0 + 5] = 0; ws[R(9), g0 + 5] = -ws[R(9), g0 + 5]           # one -0 among ordinary groups
        wq[R(10)] = 0; ws[R(10)] = -ws[R(10)]                                # all -0 but the chunk, which is all +0
        ws[R(10), g0:g0 + 16] = -ws[R(10), g0:g0 + 16]
        wq[R(11)] = 0; ws[R(11), g0:g0 + 16] = -ws[R(11), g0:g0 + 16]        # all +0 but the chunk, which is all -0
        for r in range(16, 32):                                              # a -0 / denormal group in every lane position of the chunk
            g = r - 16
            wq[R(r), g0 + g] = 0; ws[R(r), g0 + g] = -ws[R(r), g0 + g]
            ws[R(r), g0 + (g + 5) % 16] = F(2e-43)
        for r in range(32, 48):                                              # the chunk denormal in every lane position, the others zero
            g = r - 32
            wq[R(r)] = 0; wq[R(r), g0 + g] = rng.integers(1, 128, size=GS); ws[R(r), g0 + g] = F(2e-43)
    for u in range(2 * nch):                                                 # a whole unit of -0, every unit position
        wq[128 + u, 8 * u:8 * u + 8] = 0; ws[128 + u, 8 * u:8 * u + 8] = -ws[128 + u, 8 * u:8 * u + 8]
    x = (order_free(rng, n) * F(3)).astype(F)
    x[::GS] = F(6.0)                                                         # (every activation group has a scale > 0: the zeros above are the weights')
    old = np.full(rows, -0.0, F)
    out = resid_case(oracle, n, (wq.reshape(-1), ws.reshape(-1), rows), x, old)
    for base in (0, 64):
        assert bits(out)[base] == 0x80000000 and bits(out)[base + 1] == 0 and bits(out)[base + 2] == 0, [hex(v) for v in bits(out)[base:base + 3]]
        assert bits(out)[base + 10] == 0 and bits(out)[base + 11] == 0
        assert 0 < abs(float(out[base + 5])) < 1.2e-38                       # (the denormal rows are denormal on the device too: nothing flushed)
        assert all(0 < abs(float(out[base + r])) < 1.2e-38 for r in range(32, 48))


@pytest.mark.parametrize("nsplit,ls", [(2, (3, 5)), (8, (1, 1, 2, 4, 2, 2, 1, 3))])
def test_split_combine_role_is_canon(oracle, nsplit, ls):
    """Wo behind the split-attention combine (R_RESID_COMBINE), test_gpu_fused_roles.py's construction: equal split maxima make every
    exp() an exact 1, the split sums add up to a power of two, the partials are order-free -> the combined activation is exact"""
    n, n_head, hd, rows = 2048, 16, 128, 1024
    rng = np.random.default_rng(nsplit + n)
    part = order_free(rng, (1, nsplit, n))
    ml = np.zeros((1, n_head, nsplit, 2), F)
    ml[..., 0] = 0.25
    ml[..., 1] = np.asarray(ls, F)
    w = F(1.0) / F(sum(ls))
    assert float(w) * sum(ls) == 1.0 and (sum(ls) & (sum(ls) - 1)) == 0
    x = np.zeros(n, F)
    for s in range(nsplit):
        x = (x + part[0, s] * w).astype(F)
    old = rng.standard_normal(rows).astype(F)
    resid_case(oracle, n, (*weights(rng, rows, n), rows), None, old, attn=(part, ml, n_head, hd), act=x)


def test_residual_stream_of_a_model_is_the_same_with_plain_and_fused_launches(tmp_path):
    """Qwen3-0.6B's layer shapes, three layers, six steps: Wo (inside the fused Wo + W1|W3 launch with fusion 3, a launch of its own with
    fusion 0) and W2 write the residual stream -- it and the logits must be the same bits after every step, and no hand-off gives up"""
    spec = mf.preset("qwen3-0.6b-3l", "q80", group_size=GS)
    path = str(tmp_path / "wfc.bin")
    mf.write_model(path, spec, seed=13)
    toks = [5, 977, 19999, 5, 4242, 63]
    m = nb.load_model_file(path, max_seq_len=64, max_batch=1, kv_f16=False)
    try:
        seen = {}
        for fusion in (0, 3):
            m.set_fusion(fusion)
            xs, lgs = [], []
            for pos, t in enumerate(toks):
                lg = m.forward([t], [pos], want_logits=True)[0]
                lgs.append(np.array(lg[0], F, copy=True))
                xs.append(m.read_state("x", spec.n_embd))
            assert m.handoff_state()[1] == 0                   # no hand-off gave up
            seen[fusion] = (xs, lgs)
        for pos in range(len(toks)):
            for k, name in enumerate(("x", "logits")):
                a, b = seen[0][k][pos], seen[3][k][pos]
                assert np.all(np.isfinite(a)) and float(np.abs(a).max()) > 0
                assert np.array_equal(bits(a), bits(b)), (name, pos, int((bits(a) != bits(b)).sum()))
    finally:
        m.close()
