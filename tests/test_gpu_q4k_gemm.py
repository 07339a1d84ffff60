"""GPU tests of the Q4K int8 MFMA GEMM (nano_amd/csrc/gemm_q4k.hip): 9..64 tokens per weight read -- batched decode steps and
64-token prefill chunks of Q4K models -- through the step's own router (nano_hip_op_fused_gemv), the prefill entry point and batched
forwards.  The bar is the Q4K path's own: projections BIT FOR BIT the oracle's restatement of the reference (infer/tensor.c:359-434,
438-471), a batch row bit for bit the sequence alone, and every result equal to what the sliced GEMV route (NANO_MFMA_MIN_NB=65)
computes.  Helpers are copies of tests/test_gpu_fused_roles.py's."""
import os

import numpy as np
import pytest

from conftest import synth_model
from nano_amd import binding as nb
from fused_ref import bits, order_free, silu_mul

pytestmark = pytest.mark.gpu

Q4K = 0x42


def q4k_weights(oracle, rng, rows, n):
    w = (0.02 * rng.standard_normal(rows * n)).astype(np.float32)
    return oracle.quantize_q4k(w, [rows, n])                # framed tensor (44-byte prefix)


def ref_q4k(oracle, act, WTs, n):
    XT = oracle.quantize_q4k(np.ascontiguousarray(act, np.float32), [n])
    return np.concatenate([oracle.matmul_q4k(XT, WT, 0, rows) for WT, rows in WTs])


class min_nb:
    """NANO_MFMA_MIN_NB for the models created inside (read at model creation): 65 = the sliced GEMV route, the A/B switch"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.old = os.environ.get("NANO_MFMA_MIN_NB")
        if self.v is not None:
            os.environ["NANO_MFMA_MIN_NB"] = str(self.v)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("NANO_MFMA_MIN_NB", None)
        else:
            os.environ["NANO_MFMA_MIN_NB"] = self.old


# ---- 1. operator parity -----------------------------------------------------------------------------------------------------------
# (kind, rows): q|k|v-like three segments sharing the activation; 37 row tiles (ragged against any rows-per-workgroup); the residual
# add; W1|W3 with SwiGLU
SHAPES = [(0, (48, 16, 16)), (0, (592,)), (1, (32,)), (2, (64, 64))]
_weights = {}


def case_weights(oracle, n, kind, rows):
    """weights (and their oracle form) of a (n, shape) case: made once, shared by every token count"""
    key = (n, kind, rows)
    if key not in _weights:
        rng = np.random.default_rng(n * 7 + kind * 3 + len(rows) + rows[0])
        _weights[key] = [(q4k_weights(oracle, rng, r, n), r) for r in rows]
    return _weights[key]


@pytest.mark.parametrize("kind,rows", SHAPES)
@pytest.mark.parametrize("n", [256, 768, 2560])             # one block, an odd count, more than one K round
@pytest.mark.parametrize("nb_", [9, 16, 17, 31, 48, 64])    # a ragged last token tile, an exact tile, one over
def test_gemm_roles_q4k_bit_exact(oracle, nb_, n, kind, rows):
    WTs = case_weights(oracle, n, kind, rows)
    segs = [(WT[44:], None, r) for WT, r in WTs]
    rng = np.random.default_rng(nb_ * 31 + n + kind)
    x = order_free(rng, (nb_, n))
    nw = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32) if kind != 1 else None
    old = rng.standard_normal((nb_, sum(rows))).astype(np.float32) if kind == 1 else None
    out, route = nb.op_fused_gemv(Q4K, kind, n, segs, x, nw, nb=nb_, resid=old, want_route=True)
    assert route == "q4k_gemm", route
    for b in range(nb_):
        act = oracle.rmsnorm(x[b], nw) if nw is not None else x[b]
        if kind == 2:
            h1, h3 = ref_q4k(oracle, act, WTs[:1], n), ref_q4k(oracle, act, WTs[1:], n)
            assert np.allclose(out[b], silu_mul(h1, h3), rtol=3e-6, atol=1e-9), b
            alone = nb.op_fused_gemv(Q4K, kind, n, segs, x[b:b + 1], nw, nb=1)[0]
            assert np.array_equal(bits(out[b]), bits(alone)), ("alone", b)
        else:
            ref = ref_q4k(oracle, act, WTs, n)
            if kind == 1:
                ref = (old[b] + ref).astype(np.float32)
            assert np.array_equal(bits(out[b]), bits(ref)), (b, float(np.abs(out[b] - ref).max()))


# ---- 2. saturated nibbles ---------------------------------------------------------------------------------------------------------
def test_saturated_nibbles_bit_exact(oracle):
    """two-valued weights and activations: every group holds codes 0 and 15 only -- a missing mask or a signed read of the high nibble
    moves every integer sum"""
    n, rows, nb_ = 512, 32, 16
    rng = np.random.default_rng(41)
    w = np.where(rng.integers(0, 2, rows * n) == 1, np.float32(0.07), np.float32(-0.05)).astype(np.float32)
    WT = oracle.quantize_q4k(w, [rows, n])
    x = np.where(rng.integers(0, 2, (nb_, n)) == 1, np.float32(2.0), np.float32(-1.5)).astype(np.float32)
    assert set(np.unique(WT[44:].reshape(rows * (n // 256), 160)[:, 32:] & 0x0f)) == {0, 15}
    out, route = nb.op_fused_gemv(Q4K, 0, n, [(WT[44:], None, rows)], x, None, nb=nb_, want_route=True)
    assert route == "q4k_gemm", route
    for b in range(nb_):
        ref = ref_q4k(oracle, x[b], [(WT, rows)], n)
        assert np.array_equal(bits(out[b]), bits(ref)), (b, float(np.abs(out[b] - ref).max()))


# ---- 3. guard elements ------------------------------------------------------------------------------------------------------------
def test_token_columns_beyond_nb_and_guard_floats_are_never_written(oracle):
    n, rows, nb_, slots, pad = 256, (48, 16, 16), 17, 24, 8
    WTs = case_weights(oracle, n, 0, rows)
    rng = np.random.default_rng(17)
    x = order_free(rng, (nb_, n))
    nw = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    fill = np.float32(-12345.5)
    guard = np.full((slots, sum(rows) + pad), fill, np.float32)
    out, route = nb.op_fused_gemv(Q4K, 0, n, [(WT[44:], None, r) for WT, r in WTs], x, nw, nb=nb_, guard=guard, want_route=True)
    assert route == "q4k_gemm", route
    for b in range(nb_):
        ref = ref_q4k(oracle, oracle.rmsnorm(x[b], nw), WTs, n)
        assert np.array_equal(bits(out[b, :sum(rows)]), bits(ref)), b
    assert np.all(out[:nb_, sum(rows):] == fill), "guard floats behind a slot's rows were written"
    assert np.all(out[nb_:] == fill), "slots >= nb were written (token columns of the ragged last tile)"


# ---- 4. split-attention combine in the quantizer launch -----------------------------------------------------------------------------
def test_combine_in_the_prologue_equals_each_sequence_alone(oracle):
    n_head, hd, n, rows, nsplit, nb_ = 4, 64, 256, 32, 2, 16
    WT = case_weights(oracle, n, 1, (rows,))[0][0]
    rng = np.random.default_rng(29)
    part = rng.standard_normal((nb_, nsplit, n)).astype(np.float32)
    ml = np.zeros((nb_, n_head, nsplit, 2), np.float32)
    ml[..., 0] = rng.standard_normal((nb_, n_head, nsplit)).astype(np.float32)
    ml[..., 1] = rng.uniform(0.5, 4.0, (nb_, n_head, nsplit)).astype(np.float32)
    old = rng.standard_normal((nb_, rows)).astype(np.float32)
    seg = [(WT[44:], None, rows)]
    out, route = nb.op_fused_gemv(Q4K, 1, n, seg, None, None, nb=nb_, resid=old, attn=(part, ml, n_head, hd), want_route=True)
    assert route == "q4k_gemm", route
    for b in range(nb_):
        alone = nb.op_fused_gemv(Q4K, 1, n, seg, None, None, nb=1, resid=old[b:b + 1], attn=(part[b:b + 1], ml[b:b + 1], n_head, hd))[0]
        assert np.array_equal(bits(out[b]), bits(alone)), b


# ---- 5. refused shapes keep the sliced route ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rows", [(1024, (1000, 40, 36)), (192, (64, 32, 32))])
def test_refused_shapes_keep_the_sliced_route(oracle, n, rows):
    """segment rows that are no multiple of 16; a row length that is no whole block (tiny-nano-odd's): the slices of 8, same bits"""
    nb_ = 16
    rng = np.random.default_rng(n + 5)
    WTs = [(q4k_weights(oracle, rng, r, n), r) for r in rows]
    x = order_free(rng, (nb_, n))
    nw = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    out, route = nb.op_fused_gemv(Q4K, 0, n, [(WT[44:], None, r) for WT, r in WTs], x, nw, nb=nb_, want_route=True)
    assert route == "q4k", route
    for b in range(nb_):
        ref = ref_q4k(oracle, oracle.rmsnorm(x[b], nw), WTs, n)
        assert np.array_equal(bits(out[b]), bits(ref)), (b, float(np.abs(out[b] - ref).max()))


# ---- 6. prefill ---------------------------------------------------------------------------------------------------------------------
def test_prefill_chunk_tokens(model_dir):
    path, _ = synth_model(model_dir, "tiny-qwen3", "q4k", 0)
    m = nb.load_model_file(path, max_seq_len=128, max_batch=1)
    assert m.prefill_chunk_tokens() == 64
    m.set_strict(True)
    assert m.prefill_chunk_tokens() == 1
    m.set_strict(False)
    assert m.prefill_chunk_tokens() == 64
    m.close()
    path, _ = synth_model(model_dir, "tiny-nano-odd", "q4k", 0)         # n_embd 192: no whole blocks, the GEMM refuses
    m = nb.load_model_file(path, max_seq_len=64, max_batch=1)
    assert m.prefill_chunk_tokens() == 8
    m.close()
    with min_nb(65):
        path, _ = synth_model(model_dir, "tiny-qwen3", "q4k", 0)
        m = nb.load_model_file(path, max_seq_len=128, max_batch=1)
        assert m.prefill_chunk_tokens() == 8
        m.close()


def test_prefill_of_64_token_chunks_equals_token_by_token(model_dir):
    """100 prompt tokens = chunks of 64 + 36 through the GEMM: K and V rows of every layer at the chunks' edges and the next logits are
    those of one forward per token, and those of the sliced route (NANO_MFMA_MIN_NB=65: chunks of 8)"""
    from nano_amd import modelfile as mf
    path, spec = synth_model(model_dir, "tiny-qwen3", "q4k", 0)
    T, S, kv_dim = 100, 128, spec.kv_dim
    ids = mf.prompt_ids(611, T + 1, spec.vocab_size)
    probes = [(l, p) for l in range(spec.n_layer) for p in (0, 63, 64, 99)]

    def state(m):
        rows = [m.read_state(w, kv_dim, layer=l, pos=p).copy() for l, p in probes for w in ("k", "v")]
        return rows, m.forward([int(ids[T])], [T])[0][0].copy()

    ma = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    for p in range(T):
        ma.forward([int(ids[p])], [p], want_logits=False)
    ref_rows, ref_lg = state(ma)
    ma.close()
    for v in (None, 65):
        with min_nb(v):
            mb = nb.load_model_file(path, max_seq_len=S, max_batch=1)
        assert mb.prefill_chunk_tokens() == (64 if v is None else 8)
        mb.prefill(ids[:T], 0)
        rows, lg = state(mb)
        mb.close()
        for (l, p), i in zip(probes, range(0, len(rows), 2)):
            assert np.array_equal(bits(rows[i]), bits(ref_rows[i])), ("k", v, l, p)
            assert np.array_equal(bits(rows[i + 1]), bits(ref_rows[i + 1])), ("v", v, l, p)
        assert np.array_equal(bits(lg), bits(ref_lg)), v


# ---- 7. batched decode A/B ----------------------------------------------------------------------------------------------------------
def test_batched_decode_equals_the_sliced_route(model_dir):
    from nano_amd import modelfile as mf
    path, spec = synth_model(model_dir, "tiny-qwen3", "q4k", 0)
    B, T = 33, 6
    seqs = [mf.prompt_ids(900 + b, T, spec.vocab_size) for b in range(B)]

    def run(v):
        with min_nb(v):
            m = nb.load_model_file(path, max_seq_len=16, max_batch=B)
        out = [m.forward([int(s[pos]) for s in seqs], [pos] * B)[0].copy() for pos in range(T)]
        m.close()
        return out
    gemm, sliced = run(None), run(65)
    for pos in range(T):
        assert np.array_equal(bits(gemm[pos]), bits(sliced[pos])), pos
