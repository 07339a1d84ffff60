"""The in-wave canonical fold of one-chunk Q80 rows on the device (gemv_q80_slab_body.inc SLAB_WF, gemv_q80_impl.h wave_fold_canon16):
at n = 1024, group size 64, one sequence, the rmsnorm roles (q|k|v: store; W1|W3: SwiGLU) keep every group product in the lane that
formed it, fold a row inside its wave and store from there -- no LDS product table, no workgroup barrier behind the dots.  The bits
must be those of tests/canon.py, which the table route (every other shape, two sequences and more) is held to as well.

Through the operator C-ABI (nano_hip_op_fused_gemv, the step's own router) and, for the position-indexed v row, through a model
whose first layer sees order-free activations.  Inputs are ORDER-FREE where a norm is in front (test_gpu_fused_roles.py explains
why that pins the quantized activation exactly).  tests/test_wave_fold_order.py restates the lane schedule itself on the CPU.
Reference lines: rmsnorm infer.c:601-614, quantize tensor.c:21-46, matmul_quant infer.c:654-679, SwiGLU infer.c:937-944."""
import numpy as np
import pytest

from canon import matmul_q80_canon
from nano_amd import binding as nb
from nano_amd import modelfile as mf
from fused_ref import bits, order_free, silu_mul

pytestmark = pytest.mark.gpu

Q80, N, GS = 0x80, 1024, 64
F = np.float32


def weights(rng, rows):
    wq = rng.integers(-127, 128, size=rows * N, dtype=np.int8)
    ws = rng.uniform(1e-4, 2e-3, size=rows * N // GS).astype(F)
    return wq, ws


def canon_of(oracle, x, nw, segs):
    xq, xs = oracle.quantize_q80(oracle.rmsnorm(x, nw), GS)
    return np.concatenate([matmul_q80_canon(xq, xs, wq, ws, N, rows, GS) for wq, ws, rows in segs])


def store_case(oracle, rng, rows, segs=None):
    """one q|k|v-like launch (kind 0: rmsnorm + quantize + store): canon.py bit for bit; the same inputs as two sequences (the product
    table's route) give sequence 0 the same bits"""
    x = order_free(rng, N)
    nw = (1 + 0.1 * rng.standard_normal(N)).astype(F)
    segs = segs if segs is not None else [(*weights(rng, r), r) for r in rows]
    want = canon_of(oracle, x, nw, segs)
    one, route = nb.op_fused_gemv(Q80, 0, N, segs, x[None], nw, gs=GS, want_route=True)
    assert route == "gemv", route
    bad = np.flatnonzero(bits(one[0]) != bits(want))
    assert bad.size == 0, (rows, bad[:8], one[0][bad[:8]], want[bad[:8]])
    two = nb.op_fused_gemv(Q80, 0, N, segs, np.stack([x, x]), nw, gs=GS, nb=2)
    assert np.array_equal(bits(two[0]), bits(one[0])) and np.array_equal(bits(two[1]), bits(one[0]))
    return one[0]


# q|k|v of Qwen3-0.6B (16 rows per workgroup, one unit per wave); 2560 rows -> 10 rows per workgroup (rw % 4 != 0: the third tile has two
# dead rows); 2050 rows -> 9 rows per workgroup and a last workgroup of 7; three short segments of odd tile counts (4 rows per workgroup; the
# segments of a launch are multiples of 4 rows); 4096 + 2 x 1024 -> 32 rows per workgroup (two units per wave)
@pytest.mark.parametrize("rows", [(2048, 1024, 1024), (2560,), (2050,), (1004, 44, 36), (4096, 1024, 1024), (7,)], ids=str)
def test_store_role_is_canon(oracle, rows):
    store_case(oracle, np.random.default_rng(sum(rows)), rows)


# W1|W3 of Qwen3-0.6B (12 rows per workgroup: 6 pair units of 2 + 2 rows); 2560 -> 10 rows (5 pair units); 2050 -> 9 rows (the fifth pair
# unit has a dead row) and a last workgroup of 7; 1030 -> 5 rows
@pytest.mark.parametrize("rows", [3072, 2560, 2050, 1030, 3], ids=str)
def test_swiglu_role_is_canon(oracle, rows):
    rng = np.random.default_rng(rows)
    x = order_free(rng, N)
    nw = (1 + 0.1 * rng.standard_normal(N)).astype(F)
    w1, w3 = (*weights(rng, rows), rows), (*weights(rng, rows), rows)
    h1, h3 = canon_of(oracle, x, nw, [w1]), canon_of(oracle, x, nw, [w3])
    one, route = nb.op_fused_gemv(Q80, 2, N, [w1, w3], x[None], nw, gs=GS, want_route=True)
    assert route == "gemv", route
    # the two projections inside are canon.py's; the epilogue's expf is the device's (<= 2 ulp of libm) ...
    assert np.allclose(one[0], silu_mul(h1, h3), rtol=3e-6, atol=1e-9), float(np.abs(one[0] - silu_mul(h1, h3)).max())
    # ... and the same device epilogue on the table route's projections (two sequences) gives the same bits: same v0, same v1
    two = nb.op_fused_gemv(Q80, 2, N, [w1, w3], np.stack([x, x]), nw, gs=GS, nb=2)
    assert np.array_equal(bits(two[0]), bits(one[0])) and np.array_equal(bits(two[1]), bits(one[0]))
    # the store form of the same pair pins the projections themselves bit for bit (the segments of a store launch are multiples of 4 rows)
    if rows % 4 == 0:
        both = nb.op_fused_gemv(Q80, 0, N, [w1, w3], x[None], nw, gs=GS)[0]
        assert np.array_equal(bits(both), bits(np.concatenate([h1, h3])))


def test_signed_zero_and_denormal_products(oracle):
    """group products that are +0, -0 and denormal: weight groups of zeros under scales of either sign (an all-(-0) row must come out
    -0: no chain may start from +0.0), scales so small that products and partial sums are denormal, and both next to ordinary groups"""
    rng = np.random.default_rng(5)
    rows = 64
    wq, ws = weights(rng, rows)
    wq = wq.reshape(rows, 16, GS).copy(); ws = ws.reshape(rows, 16).copy()
    wq[0] = 0; ws[0] = -ws[0]                                  # row 0: every product -0
    wq[1] = 0                                                  # row 1: every product +0
    wq[2] = 0; ws[2, ::2] = -ws[2, ::2]                        # row 2: alternating -0 / +0
    wq[3, :8] = 0; ws[3, :8] = -ws[3, :8]                      # row 3: S_0 = -0, S_1 ordinary
    wq[4, 8:] = 0; ws[4, 8:] = -ws[4, 8:]                      # row 4: S_0 ordinary, S_1 = -0
    ws[5] = F(1e-42)                                           # row 5: denormal scales: denormal products and sums
    ws[6] = F(3e-44); ws[6, ::3] = -F(3e-44)                   # row 6: ... of both signs, cancelling
    ws[7, 1:] = F(1e-43)                                       # row 7: one ordinary group, fifteen denormal ones
    ws[8] = F(1e-36)                                           # row 8: products near the smallest normal number
    wq[9, 5] = 0; ws[9, 5] = -ws[9, 5]                         # row 9: one -0 among ordinary groups
    for r in range(16, 32):                                    # a -0 / denormal group in every lane position of a wave's unit
        g = r - 16
        wq[r, g] = 0; ws[r, g] = -ws[r, g]
        ws[r, (g + 5) % 16] = F(2e-43)
    seg = (wq.reshape(-1), ws.reshape(-1), rows)
    out = store_case(oracle, rng, (rows,), segs=[seg])
    assert bits(out[0])[0] == 0x80000000 and bits(out[1])[0] == 0 and bits(out[2])[0] == 0
    assert 0 < abs(float(out[5])) < 1.2e-38                    # (the denormal rows are denormal on the device too: nothing flushed)
    # the same matrix as W1 of a SwiGLU pair (W3 ordinary): the pair units keep zeros and denormals too
    w3 = (*weights(rng, rows), rows)
    x = order_free(rng, N)
    nw = (1 + 0.1 * rng.standard_normal(N)).astype(F)
    both = nb.op_fused_gemv(Q80, 0, N, [seg, w3], x[None], nw, gs=GS)[0]
    assert np.array_equal(bits(both), bits(canon_of(oracle, x, nw, [seg, w3])))
    one = nb.op_fused_gemv(Q80, 2, N, [seg, w3], x[None], nw, gs=GS)
    two = nb.op_fused_gemv(Q80, 2, N, [seg, w3], np.stack([x, x]), nw, gs=GS, nb=2)
    assert np.array_equal(bits(two[0]), bits(one[0]))
    two = nb.op_fused_gemv(Q80, 2, N, [w3, seg], np.stack([x, x]), nw, gs=GS, nb=2)
    one = nb.op_fused_gemv(Q80, 2, N, [w3, seg], x[None], nw, gs=GS)
    assert np.array_equal(bits(two[0]), bits(one[0]))


@pytest.mark.parametrize("fusion", [0, 3], ids=["plain-launches", "fused-launches"])
def test_position_indexed_v_row_is_canon(oracle, tmp_path, fusion):
    """q | k | v as a decode step launches it: three segments, the v segment stored at the row of the step's position in the KV cache.
    Qwen3-0.6B's layer shapes; the embedding rows of the tokens used are rewritten as order-free values (int8 in [-32, 32] under the
    scale 2^-4), so layer 0's rmsnorm and quantizer are pinned and its v rows must be canon.py's bit for bit -- through the plain role
    kernel (fusion 0) and through the fused q | k | v + attention launch (fusion 3), at several positions, each row where it belongs."""
    spec = mf.preset("qwen3-0.6b-3l", "q80", group_size=GS)
    assert spec.n_embd == N
    path = str(tmp_path / "wf.bin")
    lay = mf.write_model(path, spec, seed=11)
    raw = np.memmap(path, dtype=np.uint8, mode="r+")
    base = lay.params_offset

    def ent(name, dtype):
        off, nbytes = lay.entries[name]
        return raw[base + off: base + off + nbytes].view(dtype)

    rng = np.random.default_rng(17)
    toks = [5, 977, 19999, 5, 4242, 63]
    eq, es = ent("tok_emb.0.q", np.int8).reshape(spec.vocab_size, N), ent("tok_emb.0.s", F).reshape(spec.vocab_size, N // GS)
    for t in set(toks):
        eq[t] = rng.integers(-32, 33, size=N, dtype=np.int8)
        es[t] = F(1.0 / 16.0)
    raw.flush()
    nw = np.array(ent("rms_attn", F)[:N])
    wv = (np.array(ent("wv.0.q", np.int8)), np.array(ent("wv.0.s", F)), spec.kv_dim)
    xs_of = {t: (eq[t].astype(F) * F(1.0 / 16.0)).astype(F) for t in set(toks)}
    del eq, es, raw
    m = nb.load_model_file(path, max_seq_len=64, max_batch=1, kv_f16=False)
    try:
        m.set_fusion(fusion)
        for pos, t in enumerate(toks):
            m.forward([t], [pos], want_logits=False)
        assert m.handoff_state()[1] == 0                       # no hand-off gave up
        for pos, t in enumerate(toks):
            got = m.read_state("v", spec.kv_dim, layer=0, pos=pos)
            want = canon_of(oracle, xs_of[t], nw, [wv])
            assert np.array_equal(bits(got), bits(want)), (fusion, pos, int((bits(got) != bits(want)).sum()))
    finally:
        m.close()
