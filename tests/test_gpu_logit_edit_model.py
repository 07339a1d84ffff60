"""GPU tests of logit edits behind a decode step and through the engine (tiny-qwen3 F32 and Q80).

nano_hip_forward_sample_batch_edit equals nano_hip_forward followed by the operator on those logits; temperature-0 rows are numpy's first
arg-max of the edited logits; the step's logits stay unedited, bit for bit; an unedited call behind an edited one is the call on a fresh
model.  Through the engine: a session with nano_set_logit_edit gives the same ids on the device and through the host loops
(NANO_HOST_SAMPLER=1, read once per process: child processes), all of them allowed; clearing the edit restores the unconstrained ids; the
same for nano_forward_batch_sample_edit with per-sequence edits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import synth_model
from nano_amd import binding as nb
import logit_edit_engine_child as ch
import logit_edit_ref as er

pytestmark = pytest.mark.gpu
MODELS = [("tiny-qwen3", "f32", 0), ("tiny-qwen3", "q80", 64)]
HERE = os.path.dirname(os.path.abspath(__file__))


def record(r):
    return (r.token, r.status, r.n_candidates, r.n_sorted, r.nucleus, tuple(r.top), r.sum_bits, r.walked_chunks)


def row_edits(V, rng):
    """four rows: a mask and a bias list, a bias list, none, a mask (a temperature-0 row)"""
    on0, on3 = rng.random(V) < 0.05, rng.random(V) < 0.5
    t = rng.permutation(V)[:40]
    return ([{"allow": er.words(on0, V), "bias": (t, rng.normal(0.0, 3.0, 40).astype(np.float32))},
             {"bias": (t[:5], np.array([8.0, -np.inf, 2.0, 1.0, -1.0], np.float32))}, None, {"allow": er.words(on3, V)}],
            [on0, np.ones(V, bool), np.ones(V, bool), on3])


@pytest.mark.parametrize("preset,quant,gs", MODELS)
def test_step_then_edited_sample_equals_the_operator(model_dir, preset, quant, gs):
    path, spec = synth_model(model_dir, preset, quant, gs)
    V, B = spec.vocab_size, 4
    a = nb.load_model_file(path, max_seq_len=32, max_batch=B)
    b = nb.load_model_file(path, max_seq_len=32, max_batch=B)
    fresh = nb.load_model_file(path, max_seq_len=32, max_batch=B)
    try:
        rng = np.random.default_rng(18)
        ids = rng.integers(0, V, size=(B, 8)).astype(np.uint32)
        cfg = [(1.1, 1.0, 0.9), (1.0, 0.7, 1.0), (1.2, 1.0, 0.9), (1.1, 0.0, 0.9)]
        ks = [0, 3, 0, 0]
        for p in range(3):
            edits, ons = row_edits(V, rng)
            hists = [ids[s, :p] for s in range(B)]
            rows = [(rp, t, tp, float(np.float32(rng.random() * 0.999)), hists[s]) for s, (rp, t, tp) in enumerate(cfg)]
            got = a.forward_sample_batch(ids[:, p], [p] * B, rows, top_k=ks, edits=edits)
            # the step's logits are not modified: what an unedited step of another model leaves, bit for bit
            lg, _ = b.forward(ids[:, p], [p] * B)
            for s in range(B):
                kept = a.read_state("logits", V, slot=s)
                assert np.array_equal(np.asarray(kept, np.float32).view(np.uint32), lg[s].view(np.uint32)), (p, s)
            want = b.op_sample_batch(lg, rows, top_k=ks, edits=edits)
            for s in range(B):
                assert record(got[s]) == record(want[s]), (p, s)
                e = edits[s] or {}
                ref = er.sample(lg[s], hists[s], *rows[s][:4], ks[s], e.get("allow"), e.get("bias"))
                assert got[s].status == 0 and got[s].token == ref.token and ons[s][got[s].token], (p, s)
                if not ref.argmax:
                    assert (got[s].n_candidates, got[s].nucleus, tuple(got[s].top), got[s].sum_bits) == (ref.n_candidates, ref.nucleus, ref.top, ref.sum_bits)
            # temperature 0 (penalty 1.1 over the history): numpy's first arg-max of the penalised edited logits; with penalty 1 of the edited logits
            y = er.edited(lg[3], edits[3]["allow"])
            flat = a.op_sample_batch(lg[3:4], [(1.0, 0.0, 0.9, 0.0, [])], edits=[edits[3]])[0]
            assert flat.token == int(np.argmax(y)) and ons[3][flat.token]
            # an unedited call behind an edited one: the same call on a model that never saw an edit
            plain = a.forward_sample_batch(ids[:, p], [p] * B, rows, top_k=ks)
            assert [record(r) for r in plain] == [record(r) for r in fresh.forward_sample_batch(ids[:, p], [p] * B, rows, top_k=ks)], p
    finally:
        a.close(); b.close(); fresh.close()


def child(path, V, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("NANO_SAMPLE_TOP_K", "NANO_HOST_SAMPLER", "NANO_LOOKUP_DRAFT")}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "logit_edit_engine_child.py"), path, str(V)], env=e, capture_output=True, text=True,
                       timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("preset,quant,gs", MODELS)
def test_engine_edit(model_dir, preset, quant, gs):
    path, spec = synth_model(model_dir, preset, quant, gs)
    V = spec.vocab_size
    dev = child(path, V)
    host = child(path, V, NANO_HOST_SAMPLER="1")
    assert len(dev["sess_edit"]) == 24 and len(dev["sess_plain"]) == 24 and len(dev["greedy_edit"]) == 12
    # device and host loops agree id for id, with the edit and without
    assert dev == host
    # every id is allowed
    assert set(dev["sess_edit"]) <= set(ch.ALLOWED) and set(dev["greedy_edit"]) <= set(ch.ALLOWED)
    assert len(set(dev["sess_edit"])) > 1
    # clearing the edit restores the unconstrained ids; and the edit did something
    assert dev["sess_cleared"] == dev["sess_plain"] and not set(dev["sess_plain"]) <= set(ch.ALLOWED)
    assert dev["greedy_edit"] != dev["greedy_plain"]
    # per-sequence edits at batch 3: sequences 0 and 2 stay inside their sets, sequence 1 (bias only) is free
    for s, allowed in enumerate(ch.SEQ_ALLOWED):
        if allowed:
            assert set(dev["batch_edit"][s]) <= set(allowed), (s, dev["batch_edit"][s])
    assert dev["batch_edit"] != dev["batch_plain"] and len(dev["batch_edit"][0]) == 8
