"""GPU tests of text embeddings through a model (nano_hip_step_rows_pool / nano_embed_batch, include/nano_mi355x.h,
include/nano_infer_abi.h) on the tiny presets with synthetic weights.  Strict and exact mode must return the oracle's final-norm states
and tests/pool_ref.py's ordered form on them BIT FOR BIT; the fast path must not depend on how a call's rows are packed, must leave
nano_hip_step_rows' K / V rows, and is tied to the forward that is already verified through the classifier's logits."""
import ctypes as C
import os

import numpy as np
import pytest

import pool_ref as pr
from conftest import E2E_CASES
from fused_ref import bits
from nano_amd import binding as nb
from nano_amd import modelfile as mf
from oracle import binding as ob
from test_gpu_pool_rows import U, norm_bound

pytestmark = pytest.mark.gpu

S = 256
FAST_CASES = [("tiny-qwen3", "q80", 64), ("tiny-nano", "f32", 0), ("tiny-nano-odd", "q4k", 0)]
LENGTHS = (1, 2, 15, 63, 64, 65, 100, 3, 1)                                  # nine texts: their rows span several passes and range buckets
CACHES = {"paged": dict(kv_f16=False, kv_paged=True), "fp16": dict(kv_f16=True, kv_paged=False), "fp8": dict(kv_f16=False, kv_paged=False, kv_fp8=True)}

_models = {}


def synth(model_dir, preset, quant, gs):
    """the tiny presets with a RoPE table (block_size) long enough for the texts here; returns (path, spec, layout)"""
    key = (preset, quant, gs)
    if key not in _models:
        spec = mf.preset(preset, quant, group_size=gs, block_size=S)
        path = os.path.join(model_dir, f"pool-{preset}-{quant}-{gs}.bin")
        _models[key] = (path, spec, mf.write_model(path, spec, seed=39))
    return _models[key]


def texts_of(spec, lengths, seed=500):
    return [np.ascontiguousarray(mf.prompt_ids(seed + i, n, spec.vocab_size), np.uint32) for i, n in enumerate(lengths)]


def call_of(texts):
    """text i in slot i from position 0: (segments, tokens)"""
    return [(i, 0, len(t)) for i, t in enumerate(texts)], np.concatenate(texts).astype(np.uint32)


# ---- 1. strict and exact mode: the oracle's states, and the ordered form on them, bit for bit -------------------------------------
_oracle_states = {}


def oracle_states(oracle, path, spec, texts):
    """per text the oracle's final-norm state after each of its tokens: [len, n_embd] (computed once per model file)"""
    if path not in _oracle_states:
        o = ob.OracleCtx(oracle, path, max_seq_len=S)
        out = []
        for t in texts:
            rows = []
            for pos, tok in enumerate(t):
                o.forward(int(tok), pos)
                rows.append(o.state("x", spec.n_embd))
            out.append(np.stack(rows))
        o.close()
        _oracle_states[path] = out
    return _oracle_states[path]


@pytest.mark.parametrize("mode", ["strict", "exact"])
@pytest.mark.parametrize("preset,quant,gs", E2E_CASES)
def test_ordered_modes_return_the_oracles_bits(oracle, model_dir, preset, quant, gs, mode):
    path, spec, _ = synth(model_dir, preset, quant, gs)
    texts = texts_of(spec, (1, 5, 70))
    states = oracle_states(oracle, path, spec, texts)
    segs, toks = call_of(texts)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=4)
    m.set_strict(True) if mode == "strict" else m.set_exact(True)
    last = m.step_rows_pool(segs, toks, "last", False, 0)
    for i, st in enumerate(states):
        assert np.array_equal(last[i], st[-1]), ("last", i)
        assert np.array_equal(bits(last[i]), bits(pr.pool_ordered(st, "last", False, 0))), ("last", i)
    for pooling, normalize, dim in (("mean", False, 0), ("last", True, 0), ("mean", True, 0), ("mean", True, 33)):
        got = m.step_rows_pool(segs, toks, pooling, normalize, dim)
        for i, st in enumerate(states):
            assert np.array_equal(bits(got[i]), bits(pr.pool_ordered(st, pooling, normalize, dim))), (pooling, normalize, dim, i)
    m.close()


# ---- 2. the fast path: packing does not matter, and the cache is nano_hip_step_rows' ----------------------------------------------
def one_call_equals_nine(path, spec, **cache):
    texts = texts_of(spec, LENGTHS)
    segs, toks = call_of(texts)
    a = nb.load_model_file(path, max_seq_len=S, max_batch=len(texts), **cache)
    b = nb.load_model_file(path, max_seq_len=S, max_batch=len(texts), **cache)
    for pooling in ("last", "mean"):
        for normalize, dim in ((True, 0), (False, 33)):
            whole = a.step_rows_pool(segs, toks, pooling, normalize, dim)
            for i, t in enumerate(texts):
                alone = b.step_rows_pool([(i, 0, len(t))], t, pooling, normalize, dim)
                assert np.array_equal(bits(whole[i]), bits(alone[0])), (pooling, normalize, dim, i)
            assert np.isfinite(whole).all() and whole.any(axis=1).all()
    return a, b, texts, segs, toks


def bucket_positions(length):
    ps = set()
    for lo in range(0, length, 64):
        hi = min(lo + 63, length - 1)
        ps |= {lo, (lo + hi) // 2, hi}
    return sorted(ps)


@pytest.mark.parametrize("preset,quant,gs", FAST_CASES)
def test_one_call_equals_one_call_per_text(model_dir, preset, quant, gs):
    path, spec, _ = synth(model_dir, preset, quant, gs)
    a, b, texts, segs, toks = one_call_equals_nine(path, spec, kv_f16=False, kv_paged=False)
    c = nb.load_model_file(path, max_seq_len=S, max_batch=len(texts), kv_f16=False, kv_paged=False)
    c.step_rows(segs, toks)
    for i, t in enumerate(texts):                                            # the K / V rows are those nano_hip_step_rows leaves
        for layer in range(spec.n_layer):
            for pos in bucket_positions(len(t)):
                for which in ("k", "v"):
                    ra, rc = a.read_state(which, spec.kv_dim, i, layer, pos), c.read_state(which, spec.kv_dim, i, layer, pos)
                    assert np.array_equal(bits(ra), bits(rc)), (which, "slot", i, "layer", layer, "pos", pos)
    # ... and the slots go on decoding as nano_hip_step_rows' do
    nxt, pos = [int(t[-1]) for t in texts], [len(t) for t in texts]
    la, lc = a.forward(nxt, pos)[0], c.forward(nxt, pos)[0]
    assert np.array_equal(bits(la), bits(lc))
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("cache", list(CACHES))
def test_one_call_equals_one_call_per_text_on_the_other_caches(model_dir, cache):
    path, spec, _ = synth(model_dir, "tiny-qwen3", "q80", 64)
    a, b, *_ = one_call_equals_nine(path, spec, **CACHES[cache])
    a.close(); b.close()


# ---- 3. the fast path tied to the verified forward: logit = W_cls[token] . e ------------------------------------------------------
def test_last_vector_reproduces_the_classifiers_logits(model_dir):
    path, spec, lay = synth(model_dir, "tiny-nano", "f32", 0)
    V, E = spec.vocab_size, spec.n_embd
    off, nbytes = lay.entries["tok_emb"]
    assert spec.shared_classifier and nbytes == 4 * V * E
    W = np.fromfile(path, np.float32, V * E, offset=lay.params_offset + off).reshape(V, E).astype(np.float64)
    texts = texts_of(spec, LENGTHS)
    segs, toks = call_of(texts)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=len(texts))
    e = m.step_rows_pool(segs, toks, "last", False, 0).astype(np.float64)
    _sc, top = m.step_rows_score(segs, toks, 32)
    ends = np.cumsum([len(t) for t in texts]) - 1
    worst = 0.0
    for i, r in enumerate(ends):
        tok, logit = top[r]["token"].astype(np.int64), top[r]["logit"].astype(np.float64)
        ref = W[tok] @ e[i]
        Sabs = np.abs(W[tok]) @ np.abs(e[i])
        # test_gpu_ops.py's FP32 matmul bound (n = n_embd) plus the pool kernel's per-row norm bound times S: the classifier's prologue
        # norms the row in an order of its own
        bound = (10 + (E + 255) // 256) * U * Sabs + U * np.abs(ref) + norm_bound(E) * Sabs
        d = np.abs(logit - ref)
        worst = max(worst, float((d / bound).max()))
        assert np.all(d <= bound), (i, float((d / bound).max()))
    print(f"largest |logit - W.e| / bound over {len(ends)} texts x 32 tokens: {worst:.3f}")
    m.close()


# ---- 4. refusals with a model ------------------------------------------------------------------------------------------------------
def test_refusals(model_dir):
    path, spec, _ = synth(model_dir, "tiny-nano", "f32", 0)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=4)
    L = nb.lib()
    tok = np.arange(4, dtype=np.uint32)
    seg = nb.row_segs([(0, 0, 4)])
    out = np.full(4 * spec.n_embd, 7.0, np.float32)

    def rc(p, segs=seg, n=1, t=tok, o=out):
        pp = None if p is None else nb.NanoHipPoolParams(*p)
        return L.nano_hip_step_rows_pool(m.h, segs.ctypes.data, n, t.ctypes.data, None if pp is None else C.byref(pp), None if o is None else o.ctypes.data)

    assert rc(None) == -1 and rc((0, 1, 0, 0), o=None) == -1
    assert rc((2, 1, 0, 0)) == -1 and rc((0, 2, 0, 0)) == -1 and rc((0, 1, spec.n_embd + 1, 0)) == -1 and rc((0, 1, 0, 1)) == -1
    assert rc((0, 1, 0, 0), segs=nb.row_segs([(4, 0, 4)])) == -1              # what nano_hip_step_rows refuses: a slot beyond max_batch
    assert rc((0, 1, 0, 0), t=np.full(4, spec.vocab_size, np.uint32)) == -1  # ... a token beyond the vocabulary
    assert np.all(out == 7.0)                                                 # a refused call writes nothing
    assert rc((0, 1, 0, 0), n=0) == 0 and np.all(out == 7.0)                  # no segments: nothing happens
    lpath = os.path.join(model_dir, "pool-tiny-nano.lora")
    mf.write_lora(lpath, spec, rank=4, alpha=8, seed=3)
    m.lora_attach_file(lpath)
    with pytest.raises(nb.NanoHipError, match="LoRA"):
        m.step_rows_pool([(0, 0, 4)], tok)
    m.lora_enable(False)
    got = m.step_rows_pool([(1, 0, 0), (0, 0, 4), (2, 0, 0)], tok, "mean", True, 5)
    assert got.shape == (3, 5) and not got[0].any() and not got[2].any() and abs(float(np.linalg.norm(got[1].astype(np.float64))) - 1) < 1e-6
    assert not m.step_rows_pool([(1, 0, 0), (2, 0, 0)], [], "last", True, 0).any()       # all counts 0: zeros, nothing fed
    m.close()


# ---- 5. the engine -----------------------------------------------------------------------------------------------------------------
def test_engine_embed_batch(model_dir):
    path, spec, _ = synth(model_dir, "tiny-qwen3", "q80", 64)
    texts = texts_of(spec, (5, 70, 1, 33), seed=900)
    segs, toks = call_of(texts)
    lens = [len(t) for t in texts]
    e = nb.Engine(path, max_seq_len=S, max_batch=4)                          # what nano_prefill_batch gives for the same texts
    first = e.prefill_batch(texts)
    second = e.forward_batch(first, lens, want_logits=False)
    e.close()
    e = nb.Engine(path, max_seq_len=S, max_batch=4)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=4)
    for pooling, normalize, dim in (("mean", False, 40), ("last", True, 0)):
        got = e.embed_batch(texts, spec.n_embd, pooling, normalize, dim)
        assert np.array_equal(bits(got), bits(m.step_rows_pool(segs, toks, pooling, normalize, dim))), (pooling, normalize, dim)
    # the sequences are left ingested: each text's last row once more gives the arg-max nano_prefill_batch's first_ids gives ...
    assert np.array_equal(e.forward_batch([int(t[-1]) for t in texts], [n - 1 for n in lens], want_logits=False), first)
    assert np.array_equal(e.forward_batch(first, lens, want_logits=False), second)       # ... and the sequences decode on as the prefilled ones do
    with pytest.raises(nb.NanoHipError):
        e.embed_batch(texts, spec.n_embd, 2)                                 # pooling > 1
    e.close(); m.close()


def test_engine_refuses_lora(model_dir):
    path, spec, _ = synth(model_dir, "tiny-nano", "f32", 0)
    lpath = os.path.join(model_dir, "pool-engine-tiny-nano.lora")
    mf.write_lora(lpath, spec, rank=4, alpha=8, seed=3)
    e = nb.Engine(path, max_seq_len=S, lora_path=lpath)
    t = texts_of(spec, (6,))[0]
    ptrs = (C.c_void_p * 1)(t.ctypes.data)
    n = np.array([6], np.uint32)
    out = np.zeros(spec.n_embd, np.float32)
    assert e.L.nano_embed_batch(e.ctx, ptrs, n.ctypes.data, 1, 0, 1, 0, out.ctypes.data) == -1 and "LoRA" in nb.last_error()
    with pytest.raises(nb.NanoHipError):
        e.embed_batch([t], spec.n_embd)
    e.close()
