"""GPU tests of the top-k entry points of a model (nano_hip_prefill_score_topk, nano_hip_forward_topk, nano_hip_step_rows_score) and of
the engine (nano_score_ids_topk, nano_forward_batch_topk).

The reference of every entry is numpy (tests/topk_ref.py) on the logits that one nano_hip_forward per token returns, on the presets
where batched prefill is asserted bit-identical to token-by-token feeding: tokens equal, logit and logprob bit for bit."""
import os

import numpy as np
import pytest

from nano_amd import binding as nb
from nano_amd import modelfile as mf
from topk_ref import bits, check_topk

pytestmark = pytest.mark.gpu

S = 160
MODELS = [("tiny-qwen3", "q80", 64), ("tiny-qwen3", "f32", 0), ("tiny-nano", "f32", 0), ("tiny-nano-odd", "q4k", 0),
          ("qwen3-0.6b-3l", "q80", 64)]              # the last: a vocabulary of five tiles

_models, _logits = {}, {}


def synth_model(model_dir, preset, quant, gs, block=256):
    """the presets with a RoPE table (block_size) long enough for three 64-position buckets"""
    key = (preset, quant, gs, block)
    if key not in _models:
        spec = mf.preset(preset, quant, group_size=gs, block_size=block)
        path = os.path.join(model_dir, f"topk-{preset}-{quant}-{gs}-{block}.bin")
        mf.write_model(path, spec, seed=39)
        _models[key] = (path, spec)
    return _models[key]


def prepare(m, mode):
    if mode == "strict":
        m.set_strict(True)
    if mode == "exact":
        m.set_exact(True)
    return m


def token_logits(path, ids, T, mode=None, **kw):
    """[T, V] logits of feeding ids[:T] one nano_hip_forward at a time (computed once per case, never modified)"""
    key = (path, ids[:T].tobytes(), mode, tuple(sorted(kw.items())))
    if key not in _logits:
        m = prepare(nb.load_model_file(path, max_seq_len=S, max_batch=1, **kw), mode)
        out = np.stack([m.forward([int(ids[p])], [p])[0][0] for p in range(T)])
        m.close()
        out.setflags(write=False)
        _logits[key] = out
    return _logits[key]


# ---- 1. the scoring prefill ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [5, 70])
@pytest.mark.parametrize("preset,quant,gs", MODELS)
def test_prefill_score_topk(model_dir, preset, quant, gs, T):
    """T = 70 crosses a chunk boundary (and the 64-position bucket)"""
    path, spec = synth_model(model_dir, preset, quant, gs)
    ids = mf.prompt_ids(900 + T, T + 2, spec.vocab_size)
    tg = ids[1:T + 1]
    ref = token_logits(path, ids, T)
    m, twin = (nb.load_model_file(path, max_seq_len=S, max_batch=1) for _ in range(2))
    want_sc = twin.prefill_score(ids[:T], tg)
    for k in (1, 20):
        sc, top = m.prefill_score_topk(ids[:T], k, tg)
        check_topk(top, sc, ref, k, tg, f"{preset}/{quant} T={T} k={k}")
        assert sc.tobytes() == want_sc.tobytes()                            # the records are nano_hip_prefill_score's
        cut = 3 if T == 5 else 33                                           # the same prompt in two calls
        s1, t1 = m.prefill_score_topk(ids[:cut], k, tg[:cut])
        s2, t2 = m.prefill_score_topk(ids[cut:T], k, tg[cut:], pos0=cut)
        assert np.concatenate([t1, t2]).tobytes() == top.tobytes() and np.concatenate([s1, s2]).tobytes() == sc.tobytes()
        own_sc, own_top = m.prefill_score_topk(ids[:T], k)                  # no targets: each row's own arg-max
        assert own_top.tobytes() == top.tobytes() and not own_sc["rank"].any()
    only, none = m.prefill_score_topk(ids[:T], 0, tg)                       # k = 0: scores only
    assert none is None and only.tobytes() == want_sc.tobytes()
    twin.prefill(ids[:T])                                                   # what follows is what follows a plain prefill
    a, b = m.forward([int(ids[T])], [T])[0], twin.forward([int(ids[T])], [T])[0]
    assert np.array_equal(bits(a), bits(b))
    m.close(); twin.close()


@pytest.mark.parametrize("mode", ["strict", "exact"])
def test_prefill_score_topk_in_reference_order_modes(model_dir, mode):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    T, k = 9, 20
    ids = mf.prompt_ids(41, T + 1, spec.vocab_size)
    ref = token_logits(path, ids, T, mode=mode)
    m = prepare(nb.load_model_file(path, max_seq_len=S, max_batch=1), mode)
    sc, top = m.prefill_score_topk(ids[:T], k, ids[1:T + 1])
    check_topk(top, sc, ref, k, ids[1:T + 1], mode)
    assert sc.tobytes() == m.prefill_score(ids[:T], ids[1:T + 1]).tobytes()
    m.close()


# ---- 2. a decode step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,quant,gs,batch", [m + (b,) for m in MODELS[:4] for b in (1, 3, 9)] + [MODELS[4] + (9,)])
def test_forward_topk(model_dir, preset, quant, gs, batch):
    """two steps of slots 0 .. batch-1 at different positions (the second replays the first one's graph where the positions share a
    bucket); 9 rows on a model whose prefill chunk holds 8: the step's own partial rows"""
    path, spec = synth_model(model_dir, preset, quant, gs)
    k = min(20, spec.vocab_size)
    m, twin = (nb.load_model_file(path, max_seq_len=S, max_batch=batch) for _ in range(2))
    lens = [3 + 2 * s for s in range(batch)]
    for s in range(batch):
        for x in (m, twin):
            x.prefill(mf.prompt_ids(60 + s, lens[s], spec.vocab_size), 0, s)
    rng = np.random.default_rng(batch)
    for step in range(2):
        toks = rng.integers(0, spec.vocab_size, batch).astype(np.uint32)
        pos = np.array([n + step for n in lens], np.uint32)
        tg = rng.integers(0, spec.vocab_size, batch).astype(np.uint32)
        logits, amax = twin.forward(toks, pos, want_argmax=True)
        sc, top = m.forward_topk(toks, pos, k, tg)
        check_topk(top, sc, logits, k, tg, f"{preset}/{quant} batch {batch} step {step}")
        assert np.array_equal(sc["argmax"], amax)
        for s in range(batch):                                              # m->logits is left as nano_hip_forward leaves it
            assert np.array_equal(bits(m.read_state("logits", spec.vocab_size, slot=s)), bits(logits[s]))
    sc0, none = m.forward_topk(toks, pos, 0)                                # k = 0: scores only (the same step again: the same rows)
    assert none is None and np.array_equal(sc0["argmax"], amax) and np.array_equal(bits(sc0["lse"]), bits(sc["lse"]))
    m.close(); twin.close()


@pytest.mark.parametrize("mode", ["strict", "exact"])
def test_forward_topk_in_reference_order_modes(model_dir, mode):
    path, spec = synth_model(model_dir, "tiny-nano", "f32", 0)
    m, twin = (prepare(nb.load_model_file(path, max_seq_len=S, max_batch=3), mode) for _ in range(2))
    for step in range(2):
        toks, pos = np.array([5, 9, 2], np.uint32) + step, np.full(3, step, np.uint32)
        logits = twin.forward(toks, pos)[0]
        sc, top = m.forward_topk(toks, pos, 20)
        check_topk(top, sc, logits, 20, None, f"{mode} step {step}")
    m.close(); twin.close()


# ---- 3. the scoring form of a ragged step ------------------------------------------------------------------------------------------
# three slots at different positions: a count-1 decode row, a segment that crosses the 64-position bucket, 76 rows = two passes of 64
SEGS = [(0, 40, 1), (1, 50, 30), (2, 0, 45)]
ROWS_CASES = {"fast": ("tiny-qwen3", "q80", 64, None, {}), "chunks of 8": ("tiny-nano", "f32", 0, None, {}),
              "strict": ("tiny-qwen3", "q80", 64, "strict", {}), "exact": ("tiny-qwen3", "q80", 64, "exact", {}),
              "fp16 paged": ("tiny-qwen3", "q80", 64, None, dict(kv_f16=True, kv_paged=True))}


@pytest.mark.parametrize("case", list(ROWS_CASES))
def test_step_rows_score(model_dir, case):
    preset, quant, gs, mode, kw = ROWS_CASES[case]
    path, spec = synth_model(model_dir, preset, quant, gs)
    k = 20
    seq = [mf.prompt_ids(300 + s, S, spec.vocab_size) for s in range(3)]
    a, b, c = (prepare(nb.load_model_file(path, max_seq_len=S, max_batch=3, **kw), mode) for _ in range(3))
    for m in (a, b, c):
        for s, p0, _ in SEGS:
            if p0:
                m.prefill(seq[s][:p0], 0, s)
    toks = np.concatenate([seq[s][p0:p0 + n] for s, p0, n in SEGS])
    tg = np.concatenate([seq[s][p0 + 1:p0 + n + 1] for s, p0, n in SEGS])
    want = [a.prefill_score_topk(seq[s][p0:p0 + n], k, seq[s][p0 + 1:p0 + n + 1], pos0=p0, slot=s) for s, p0, n in SEGS]
    want_sc, want_top = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    sc, top = b.step_rows_score(SEGS, toks, k, tg)
    assert sc.tobytes() == want_sc.tobytes() and top.tobytes() == want_top.tobytes()
    amax = c.step_rows(SEGS, toks, want_argmax=True)
    assert np.array_equal(sc["argmax"], amax) and np.array_equal(top["token"][:, 0], amax)
    only, none = c.step_rows_score(SEGS, toks, 0, tg)                       # k = 0: scores only (the same rows fed again)
    assert none is None and only.tobytes() == sc.tobytes()
    own_sc, own_top = c.step_rows_score(SEGS, toks, k)                      # no targets
    assert own_top.tobytes() == top.tobytes() and not own_sc["rank"].any()
    # the caches are what nano_hip_prefill per segment leaves: the next step of all three slots
    nxt, pos = [int(seq[s][p0 + n]) for s, p0, n in SEGS], [p0 + n for s, p0, n in SEGS]
    la, lb = a.forward(nxt, pos)[0], b.forward(nxt, pos)[0]
    assert np.array_equal(bits(la), bits(lb))
    for m in (a, b, c):
        m.close()


def test_refusals(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    V = spec.vocab_size
    m = nb.load_model_file(path, max_seq_len=S, max_batch=2)
    L = nb.lib()
    tok, pos = np.array([1, 2], np.uint32), np.zeros(2, np.uint32)
    bad = np.array([1, V], np.uint32)
    sc, tp = np.zeros(2, nb.TOKEN_SCORE_DTYPE), np.zeros(2 * 64, nb.TOP_ENTRY_DTYPE)
    seg = nb.row_segs([(0, 0, 2)])
    P, T_ = tok.ctypes.data, tp.ctypes.data
    for k, tgt, scores, top in ((33, None, sc.ctypes.data, T_), (V + 1, None, sc.ctypes.data, T_), (5, bad.ctypes.data, sc.ctypes.data, T_),
                                (5, None, sc.ctypes.data, None), (0, None, None, None)):
        assert L.nano_hip_prefill_score_topk(m.h, 0, P, 0, 2, tgt, k, scores, top) == -1
        assert L.nano_hip_forward_topk(m.h, P, pos.ctypes.data, 2, tgt, k, scores, top) == -1
        assert L.nano_hip_step_rows_score(m.h, seg.ctypes.data, 1, P, tgt, k, scores, top) == -1
    assert L.nano_hip_prefill_score_topk(m.h, 0, None, 0, 2, None, 5, sc.ctypes.data, T_) == -1
    assert L.nano_hip_forward_topk(m.h, None, pos.ctypes.data, 2, None, 5, sc.ctypes.data, T_) == -1
    assert L.nano_hip_step_rows_score(m.h, seg.ctypes.data, 1, None, None, 5, sc.ctypes.data, T_) == -1
    assert not tp.view(np.uint8).any() and not sc.view(np.uint8).any()
    s2, t2 = m.prefill_score_topk(tok, 5)                                   # scores_out may be NULL with k >= 1; the model is usable
    assert L.nano_hip_prefill_score_topk(m.h, 0, P, 0, 2, None, 5, None, T_) == 0 and tp[:10].tobytes() == t2.tobytes()
    m.close()


# ---- 4. the engine --------------------------------------------------------------------------------------------------------------------
def test_engine_score_ids_topk(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    n, k = 71, 20
    ids = mf.prompt_ids(42, n, spec.vocab_size)
    ref = token_logits(path, ids, n - 1)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    sc, top = m.prefill_score_topk(ids[:-1], k, ids[1:])
    m.close()
    check_topk(top, sc, ref, k, ids[1:], "engine reference")
    e = nb.Engine(path, max_seq_len=S)
    lp0, am0, nll0 = e.score_ids(ids)
    lp, am, nll, ti, tl = e.score_ids_topk(ids, k)
    e.close()
    assert np.array_equal(bits(lp), bits(lp0)) and np.array_equal(am, am0) and nll == nll0
    assert np.array_equal(ti, top["token"]) and np.array_equal(bits(tl), bits(top["logprob"]))


def test_engine_forward_batch_topk(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    k = 20
    m = nb.load_model_file(path, max_seq_len=S, max_batch=2)
    e = nb.Engine(path, max_seq_len=S, max_batch=2)
    for step in range(2):
        toks, pos = [7 + step, 11 + step], [step, step]
        sc, top = m.forward_topk(toks, pos, k)
        ti, tl, am = e.forward_batch_topk(toks, pos, k)
        assert np.array_equal(ti, top["token"]) and np.array_equal(bits(tl), bits(top["logprob"])) and np.array_equal(am, sc["argmax"])
    assert e.L.nano_forward_batch_topk(e.ctx, None, None, 2, k, ti.ctypes.data, tl.ctypes.data, None) == -1
    assert e.L.nano_forward_batch_topk(e.ctx, ti.ctypes.data, ti.ctypes.data, 2, 33, ti.ctypes.data, tl.ctypes.data, None) == -1
    e.close(); m.close()
