"""GPU tests of the scoring prefill (nano_hip_prefill_score, nano_score_ids): batched prefill that also runs the classifier over every
fed row and reduces the logits to one NanoHipTokenScore per position on the device.

The reference of every score is numpy on the logits one nano_hip_forward per token returns (tests/score_ref.py): on the shapes where
batched prefill is asserted bit-identical to token-by-token ingestion (test_gpu_e2e.py test_batched_prefill_equals_token_by_token) the
selections and rank must be equal and lse within 1e-5 * max(1, |ref|)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import synth_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf
from score_ref import check_scores, ref_scores
from fused_ref import bits

pytestmark = pytest.mark.gpu

S = 96
TOL_Q80 = 2e-2                       # test_gpu_e2e.py TOL["q80"]: Q80 logits, relative to the row's largest |logit|


_logits = {}


def token_logits(path, ids, T, max_seq_len=S, mode=None, lora=None, **kw):
    """[T, V] logits of feeding ids[:T] one nano_hip_forward at a time (computed once per case, never modified)"""
    key = (path, ids[:T].tobytes(), max_seq_len, mode, lora, tuple(sorted(kw.items())))
    if key not in _logits:
        m = nb.load_model_file(path, max_seq_len=max_seq_len, max_batch=1, **kw)
        prepare(m, mode, lora)
        out = np.stack([m.forward([int(ids[p])], [p])[0][0] for p in range(T)])
        m.close()
        out.setflags(write=False)
        _logits[key] = out
    return _logits[key]


def prepare(m, mode=None, lora=None):
    if lora:
        m.lora_attach_file(lora)
    if mode == "strict":
        m.set_strict(True)
    if mode == "exact":
        m.set_exact(True)


def score_both_ways(m, ids, T, ref_logits, what, slot=0, **tol):
    """prefill_score of ids[:T] for the next tokens, then (the slot starts over) for each row's own arg-max"""
    got = m.prefill_score(ids[:T], ids[1:T + 1], 0, slot)
    worst = check_scores(got, ref_logits, ids[1:T + 1], what, **tol)
    own = m.prefill_score(ids[:T], None, 0, slot)
    worst = max(worst, check_scores(own, ref_logits, None, what + ", own arg-max", **tol))
    assert np.array_equal(own["argmax"], got["argmax"]) and np.array_equal(bits(own["lse"]), bits(got["lse"]))
    return got, worst


PREFILL_CASES = [("tiny-qwen3", "q80", 64, 5), ("tiny-qwen3", "q80", 64, 23), ("tiny-qwen3", "q80", 64, 70), ("tiny-qwen3", "q80", 64, 93),
                 ("hd256-qwen3", "q80", 64, 64), ("tiny-nano", "f32", 0, 11), ("tiny-nano-odd", "q4k", 0, 13), ("tiny-qwen3", "f32", 0, 9)]


@pytest.mark.parametrize("preset,quant,gs,T", PREFILL_CASES)
def test_scores_equal_token_by_token_logits(model_dir, preset, quant, gs, T):
    path, spec = synth_model(model_dir, preset, quant, gs)
    ids = mf.prompt_ids(500 + T, T + 3, spec.vocab_size)
    ref = token_logits(path, ids, T)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=2)
    _, worst = score_both_ways(m, ids, T, ref, f"{preset}/{quant} T={T}", slot=1)
    m.close()
    print(f"prefill_score {preset}/{quant} T={T}: worst lse error {worst:.3f} of the bound")


# wide-qwen3: the rmsnorm tree may differ in the last ulp between batch sizes, so a chunk's logits are not the
# token-by-token bits.  lse and target_logit within TOL_Q80 of the row's largest |logit|; argmax only where the reference's top two
# logits differ by more than that, which may leave out at most one position in ten: WIDE_SEED was picked so that the token-by-token
# logits alone stay within that limit (asserted below before anything is compared).
WIDE_T, WIDE_SEED = 20, 55


def test_scores_on_wide_rows(model_dir):
    path, spec = synth_model(model_dir, "wide-qwen3", "q80", 64)
    T = WIDE_T
    ids = mf.prompt_ids(WIDE_SEED, T + 1, spec.vocab_size)
    ref = token_logits(path, ids, T)
    r = ref_scores(ref, ids[1:T + 1])
    bound = TOL_Q80 * np.abs(ref).max(axis=1).astype(np.float64)
    top2 = np.sort(ref, axis=1)[:, -2:].astype(np.float64)
    clear = (top2[:, 1] - top2[:, 0]) > bound
    print(f"wide-qwen3: {int((~clear).sum())} of {T} positions have their top two logits within the tolerance")
    assert (~clear).sum() * 10 <= T, "the seed leaves out more than one position in ten"
    m = nb.load_model_file(path, max_seq_len=S, max_batch=2)
    got = m.prefill_score(ids[:T], ids[1:T + 1], 0, 1)
    own = m.prefill_score(ids[:T], None, 0, 1)
    m.close()
    ref_tl = ref[np.arange(T), ids[1:T + 1]].astype(np.float64)
    e_lse, e_tl = np.abs(got["lse"] - r["lse"]) / bound, np.abs(got["target_logit"] - ref_tl) / bound
    print(f"wide-qwen3 T={T}: lse {e_lse.max():.3e}, target_logit {e_tl.max():.3e} of the bound")
    assert np.all(e_lse <= 1.0) and np.all(e_tl <= 1.0)
    assert np.array_equal(got["argmax"][clear], r["argmax"][clear])
    assert np.array_equal(own["argmax"], got["argmax"]) and not own["rank"].any()
    assert np.array_equal(bits(got["logprob"]), bits(got["target_logit"] - got["lse"]))


@pytest.mark.parametrize("preset,quant,gs,T", [("tiny-qwen3", "q80", 64, 93), ("tiny-nano", "f32", 0, 11), ("tiny-nano-odd", "q4k", 0, 13)])
def test_side_effects_are_those_of_prefill(model_dir, preset, quant, gs, T):
    """after prefill_score into slot 1: the K row (last layer, pos T - 1), the V row (layer 0, pos T // 2) and the next three logits are
    a second model's after prefill"""
    path, spec = synth_model(model_dir, preset, quant, gs)
    ids = mf.prompt_ids(500 + T, T + 3, spec.vocab_size)
    out = []
    for scoring in (False, True):
        m = nb.load_model_file(path, max_seq_len=S, max_batch=2)
        if scoring:
            m.prefill_score(ids[:T], ids[1:T + 1], 0, 1)
        else:
            m.prefill(ids[:T], 0, 1)
        k = m.read_state("k", spec.kv_dim, slot=1, layer=spec.n_layer - 1, pos=T - 1)
        v = m.read_state("v", spec.kv_dim, slot=1, layer=0, pos=T // 2)
        nxt = [m.forward([0, int(ids[T + i])], [0, T + i])[0][1].copy() for i in range(3)]
        m.close()
        out.append([k, v] + nxt)
    for a, b in zip(*out):
        assert np.array_equal(bits(a), bits(b))


def test_chunking_does_not_change_a_byte(model_dir):
    """T = 93 in one call = calls of 1 + 7 + 64 + 21 tokens at increasing pos0 (the 64 cross a 64-position bucket: two chunks)"""
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    T = 93
    ids = mf.prompt_ids(593, T + 1, spec.vocab_size)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    whole = m.prefill_score(ids[:T], ids[1:T + 1])
    parts, at = [], 0
    for n in (1, 7, 64, 21):
        parts.append(m.prefill_score(ids[at:at + n], ids[at + 1:at + n + 1], pos0=at))
        at += n
    m.close()
    assert at == T and np.concatenate(parts).tobytes() == whole.tobytes()


def test_scoring_and_plain_chunk_graphs_do_not_cross(model_dir):
    """two full 64-token chunks per call; plain, plain (replayed), scored, scored (replayed), plain on one slot"""
    spec = mf.preset("tiny-qwen3", "q80", group_size=64, block_size=128)
    path = os.path.join(model_dir, "score-tiny-qwen3-q80-bs128.bin")
    mf.write_model(path, spec, seed=39)
    T = 128
    ids = mf.prompt_ids(77, T + 1, spec.vocab_size)
    tg = np.concatenate([ids[1:T], ids[:1]])                  # (position T - 1 has no next token in the context: any id)
    ref = token_logits(path, ids, T, max_seq_len=T)
    m = nb.load_model_file(path, max_seq_len=T, max_batch=1)
    rows = lambda: [m.read_state(w, spec.kv_dim, 0, layer, pos).copy() for w in ("k", "v") for layer in (0, spec.n_layer - 1) for pos in (0, 63, 64, 127)]
    m.prefill(ids[:T]); first = rows()
    m.prefill(ids[:T])
    a = m.prefill_score(ids[:T], tg)
    b = m.prefill_score(ids[:T], tg)
    c = m.prefill_score(ids[:T], None)                        # a third kind of chunk: no targets
    m.prefill(ids[:T]); last = rows()
    d = m.prefill_score(ids[:T], None)
    m.close()
    check_scores(a, ref, tg, "first scoring call")
    assert a.tobytes() == b.tobytes()
    check_scores(c, ref, None, "own arg-max")
    assert c.tobytes() == d.tobytes()
    for x, y in zip(first, last):
        assert np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_scoring_behind_a_fork(model_dir, paged):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    ids = mf.prompt_ids(311, 51, spec.vocab_size)
    fresh = nb.load_model_file(path, max_seq_len=S, max_batch=1, kv_paged=paged)
    want = fresh.prefill_score(ids[:50], ids[1:51])
    fresh.close()
    m = nb.load_model_file(path, max_seq_len=S, max_batch=3, kv_paged=paged)
    m.prefill(ids[:40], 0, 0)
    m.kv_fork(0, 40, [1, 2])
    got = m.prefill_score(ids[40:50], ids[41:51], pos0=40, slot=2)
    m.close()
    assert got.tobytes() == want[40:50].tobytes()


@pytest.mark.parametrize("mode", ["strict", "exact"])
@pytest.mark.parametrize("preset,quant,gs", [("tiny-qwen3", "q80", 64), ("tiny-nano", "f32", 0)])
def test_reference_order_modes(model_dir, preset, quant, gs, mode):
    """strict / exact mode feed token by token: the selections are the bits of the same mode's forward logits"""
    path, spec = synth_model(model_dir, preset, quant, gs)
    T = 12
    ids = mf.prompt_ids(700, T + 1, spec.vocab_size)
    ref = token_logits(path, ids, T, mode=mode)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=2)
    prepare(m, mode)
    assert m.prefill_chunk_tokens() == 1
    score_both_ways(m, ids, T, ref, f"{mode} {preset}/{quant}", slot=1)
    m.close()


def test_fp16_rows(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    T = 70
    ids = mf.prompt_ids(570, T + 1, spec.vocab_size)
    ref = token_logits(path, ids, T, kv_f16=True)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1, kv_f16=True)
    score_both_ways(m, ids, T, ref, "FP16 rows")
    m.close()


def test_lora(model_dir):
    path, spec = synth_model(model_dir, "tiny-nano", "f32", 0)
    lpath = os.path.join(model_dir, "score-tiny-nano.lora")
    mf.write_lora(lpath, spec, rank=4, alpha=8, seed=3)
    T = 11
    ids = mf.prompt_ids(511, T + 1, spec.vocab_size)
    ref = token_logits(path, ids, T, lora=lpath)
    plain = token_logits(path, ids, T)
    assert not np.array_equal(ref, plain)                     # the module does something
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    prepare(m, lora=lpath)
    score_both_ways(m, ids, T, ref, "LoRA")
    m.lora_enable(False)
    score_both_ways(m, ids, T, plain, "LoRA switched off")
    m.close()


@pytest.mark.parametrize("quant,gs", [("f32", 0), ("q80", 64)])
def test_full_vocabulary(model_dir, quant, gs):
    path, spec = synth_model(model_dir, "bigvocab-qwen3", quant, gs)
    T = 9
    ids = mf.prompt_ids(909, T + 1, spec.vocab_size)
    ref = token_logits(path, ids, T, max_seq_len=32)
    m = nb.load_model_file(path, max_seq_len=32, max_batch=1)
    _, worst = score_both_ways(m, ids, T, ref, f"bigvocab {quant}")
    m.close()
    print(f"bigvocab-qwen3/{quant}: worst lse error {worst:.3f} of the bound")


def test_refusals_feed_nothing(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    V = spec.vocab_size
    known, other = mf.prompt_ids(1, 8, V), mf.prompt_ids(2, 8, V)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=2)
    m.prefill(known, 0, 1)
    before = [m.read_state(w, spec.kv_dim, 1, spec.n_layer - 1, 0).copy() for w in ("k", "v")]
    L = nb.lib()
    out = np.zeros(8, nb.TOKEN_SCORE_DTYPE)
    bad_t, bad_k = other.copy(), other.copy()
    bad_t[5] = V; bad_k[0] = V + 7
    args = lambda tok, tgt, n=8, slot=1, pos0=0: (m.h, slot, tok.ctypes.data, pos0, n, None if tgt is None else tgt.ctypes.data, out.ctypes.data)
    assert L.nano_hip_prefill_score(*args(other, bad_t)) == -1 and "target" in nb.last_error()
    assert L.nano_hip_prefill_score(*args(bad_k, other)) == -1
    assert L.nano_hip_prefill_score(*args(other, other, slot=2)) == -1
    assert L.nano_hip_prefill_score(*args(other, other, pos0=S - 7)) == -1
    assert L.nano_hip_prefill_score(m.h, 1, None, 0, 8, None, out.ctypes.data) == -1
    assert L.nano_hip_prefill_score(m.h, 1, other.ctypes.data, 0, 8, None, None) == -1
    assert L.nano_hip_prefill_score(*args(other, bad_t, n=0)) == 0                # count == 0: nothing is looked at, nothing is touched
    assert not out.view(np.uint8).any()
    after = [m.read_state(w, spec.kv_dim, 1, spec.n_layer - 1, 0) for w in ("k", "v")]
    for a, b in zip(before, after):
        assert np.array_equal(bits(a), bits(b))
    assert m.prefill_score(other[:0], other[:0]).size == 0
    m.close()


def test_engine_score_ids(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    n = 71
    ids = mf.prompt_ids(42, n, spec.vocab_size)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    want = m.prefill_score(ids[:-1], ids[1:])
    m.close()
    e = nb.Engine(path, max_seq_len=S)
    lp, am, nll = e.score_ids(ids)
    assert np.array_equal(bits(lp), bits(want["logprob"])) and np.array_equal(am, want["argmax"])
    total = 0.0
    for x in want["logprob"]:
        total -= float(x)
    assert nll == total
    nll_only = C.c_double(-1.0)
    assert e.L.nano_score_ids(e.ctx, ids, n, None, None, C.byref(nll_only)) == 0 and nll_only.value == total
    assert e.score_ids(ids[:1])[2] == 0.0 and e.score_ids(ids[:1])[0].size == 0
    e.close()
