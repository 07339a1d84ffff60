"""GPU test of the step's callers taken together: one script of calls that reaches the fast step every way there is -- prefill chunks
(plain, scored for targets, scored for the arg-max, verify), a ragged pass, the greedy loop, a batched decode step with logits and with
top-k -- run twice on one model (the second run replays every graph the first one captured, on rewritten positions) and once on a model
created with NANO_HIP_NO_GRAPH=1 (every step eager).  Everything the calls return must be equal BIT FOR BIT between the three runs: ids,
score records field by field, top-k entries, logits and the attention output read back after the batched step.  A step that replayed
another step's graph, or a caller that left something of its step behind for the next one, shows here as a difference.

The model is the suite's tiny-qwen3 Q80 group-size-64 preset, with a RoPE table (block_size) long enough for max_seq_len 192 as
test_gpu_rows.py writes it; batched prefill then feeds 64 tokens per weight read."""
import os

import numpy as np
import pytest

from nano_amd import binding as nb
from nano_amd import modelfile as mf

pytestmark = pytest.mark.gpu

S, B = 192, 4


def u32(a):
    """an array's bytes as uint32 words: floats compare by their bits, records field by field"""
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        return {n: u32(a[n]) for n in a.dtype.names}
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def script(m, spec):
    """the calls, in order; returns [(what, array or dict of field arrays)]"""
    V = spec.vocab_size
    ids = mf.prompt_ids(51, 131, V)
    out = []
    assert m.prefill(ids[:130], 0, 0) is None                                              # 1: chunks of 64, 64 (replayed) and 2 rows
    out.append(("prefill_score targets", u32(m.prefill_score(ids[:130], ids[1:131], 0, 1))))     # 2
    out.append(("prefill_score argmax", u32(m.prefill_score(ids[:130], None, 0, 1))))            # 3: the same chunks, another kind of graph
    draft = mf.prompt_ids(52, 6, V)
    am, acc = m.verify_draft(draft, pos0=130, slot=0)                                       # 4
    out.append(("verify_draft", am.copy())); out.append(("verify_draft accepted", np.array([acc], np.uint32)))
    segs = [(0, 130, 1), (2, 0, 70), (3, 60, 9)]                                            # 5: slot 3 crosses the bucket end at 64: 80 rows, two passes
    out.append(("step_rows", m.step_rows(segs, mf.prompt_ids(53, 80, V), want_argmax=True).copy()))
    out.append(("decode_greedy", m.decode_greedy([int(ids[130]), int(ids[129])], [131, 130], 5).copy()))      # 6: slots 0 and 1
    toks, pos = mf.prompt_ids(54, B, V), [136, 135, 70, 69]                                 # 7: every slot at its current position
    logits, _ = m.forward(toks, pos)
    out.append(("forward logits", u32(logits)))
    out.append(("xba", u32(np.stack([m.read_state("xba", spec.n_head * spec.hd, s) for s in range(B)]))))
    sc, top = m.forward_topk(toks, pos, 4)                                                  # 8
    out.append(("forward_topk scores", u32(sc))); out.append(("forward_topk top", u32(top)))
    return out


def same(a, b, what):
    assert [w for w, _ in a] == [w for w, _ in b]
    for (w, x), (_, y) in zip(a, b):
        for f in (x if isinstance(x, dict) else {None: x}):
            xa, ya = (x[f], y[f]) if f else (x, y)
            assert xa.shape == ya.shape and np.array_equal(xa, ya), (what, w, f, int(np.count_nonzero(xa != ya)))


def test_mixed_calls_equal_replayed_and_eager(model_dir, monkeypatch):
    spec = mf.preset("tiny-qwen3", "q80", group_size=64, block_size=256)
    path = os.path.join(model_dir, "step-mix-tiny-qwen3-q80-64.bin")
    mf.write_model(path, spec, seed=39)
    monkeypatch.delenv("NANO_HIP_NO_GRAPH", raising=False)
    a = nb.load_model_file(path, max_seq_len=S, max_batch=B, kv_f16=False, kv_paged=False)
    assert a.prefill_chunk_tokens() == 64
    first = script(a, spec)
    second = script(a, spec)
    with monkeypatch.context() as mp:
        mp.setenv("NANO_HIP_NO_GRAPH", "1")                      # (read when the model is created)
        b = nb.load_model_file(path, max_seq_len=S, max_batch=B, kv_f16=False, kv_paged=False)
    eager = script(b, spec)
    for w, x in first:
        print(w, {k: v.shape for k, v in x.items()} if isinstance(x, dict) else x.shape)
    same(first, second, "first run vs the same script again (replays)")
    same(first, eager, "graphs vs NANO_HIP_NO_GRAPH=1")
    a.close(); b.close()
