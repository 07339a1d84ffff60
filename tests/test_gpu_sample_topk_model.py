"""GPU tests of top-k sampling behind a decode step and through the engine (tiny-qwen3, tiny-nano).

nano_hip_forward_sample_batch_ex equals the operator on the logits nano_hip_forward returns from a second model, rows of mixed top_k;
the entry point without top_k and the _ex one with top_k = 0 return identical records; with NANO_SAMPLE_TOP_K=1 the engine's
generate_next_token and nano_forward_batch_sample pass Sampler.top_k to the device and give the ids of the host loops
(NANO_HOST_SAMPLER=1), and without the knob top_k stays ignored.  The engine reads its knobs once per process: child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import synth_model
from nano_amd import binding as nb
import sampler_topk_ref as tr

pytestmark = pytest.mark.gpu
MODELS = [("tiny-qwen3", "q80", 64), ("tiny-nano", "f32", 0)]
HERE = os.path.dirname(os.path.abspath(__file__))


def record(r):
    return (r.token, r.status, r.n_candidates, r.n_sorted, r.nucleus, tuple(r.top), r.sum_bits, r.walked_chunks)


@pytest.mark.parametrize("preset,quant,gs", MODELS)
def test_step_then_sample_equals_the_operator(model_dir, preset, quant, gs):
    path, spec = synth_model(model_dir, preset, quant, gs)
    V, B = spec.vocab_size, 6
    a = nb.load_model_file(path, max_seq_len=32, max_batch=B)
    b = nb.load_model_file(path, max_seq_len=32, max_batch=B)
    try:
        rng = np.random.default_rng(8)
        ids = rng.integers(0, V, size=(B, 12)).astype(np.uint32)
        ks = [0, 1, 5, 20, V, 3]
        cfg = [(1.1, 1.0, 0.9), (1.0, 1.0, 0.9), (1.2, 0.7, 0.95), (1.0, 1.3, 0.8), (1.1, 1.0, 0.9), (1.3, 0.0, 0.9)]
        bound = 0
        for p in range(4):
            hists = [ids[s, :p] for s in range(B)]
            rows = [(rp, t, tp, float(np.float32(rng.random() * 0.999)), hists[s]) for s, (rp, t, tp) in enumerate(cfg)]
            got = a.forward_sample_batch(ids[:, p], [p] * B, rows, top_k=ks)
            lg, _ = b.forward(ids[:, p], [p] * B)
            want = b.op_sample_batch(lg, rows, top_k=ks)
            for s in range(B):
                assert record(got[s]) == record(want[s]), (p, s, ks[s])
                ref = tr.sample(lg[s], hists[s], *rows[s][:4], ks[s])
                assert got[s].status == 0 and got[s].token == ref.token, (p, s, ks[s])
                if not ref.argmax:
                    assert (got[s].n_candidates, got[s].nucleus, tuple(got[s].top), got[s].sum_bits) == (ref.n_candidates, ref.nucleus, ref.top, ref.sum_bits)
                    bound += ks[s] != 0 and got[s].nucleus == ks[s] < ref.n_candidates
        assert bound >= 4, "top_k must bind on these rows (the top_k = 1 row of every position at the least)"
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("preset,quant,gs", MODELS)
def test_top_k_zero_is_the_entry_point_without_it(model_dir, preset, quant, gs):
    path, spec = synth_model(model_dir, preset, quant, gs)
    V, B = spec.vocab_size, 3
    a = nb.load_model_file(path, max_seq_len=32, max_batch=B)
    b = nb.load_model_file(path, max_seq_len=32, max_batch=B)
    try:
        ids = np.random.default_rng(9).integers(0, V, size=(B, 4)).astype(np.uint32)
        for p in range(3):
            rows = [(1.1, 1.0, 0.9, 0.2 + 0.3 * s, ids[s, :p]) for s in range(B)]
            old = a.forward_sample_batch(ids[:, p], [p] * B, rows)
            new = b.forward_sample_batch(ids[:, p], [p] * B, rows, top_k=[0] * B)
            assert [record(r) for r in old] == [record(r) for r in new], p
            lg, _ = a.forward(ids[:, p], [p] * B)
            assert [record(r) for r in a.op_sample_batch(lg, rows)] == [record(r) for r in b.op_sample_batch(lg, rows, top_k=[0] * B)] == [record(r) for r in old]
    finally:
        a.close(); b.close()


def child(path, V, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("NANO_SAMPLE_TOP_K", "NANO_HOST_SAMPLER")}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "sample_topk_engine_child.py"), path, str(V)], env=e, capture_output=True, text=True,
                       timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("preset,quant,gs", MODELS)
def test_engine_knob(model_dir, preset, quant, gs):
    path, spec = synth_model(model_dir, preset, quant, gs)
    V = spec.vocab_size
    dev = child(path, V, NANO_SAMPLE_TOP_K="1")
    host = child(path, V, NANO_SAMPLE_TOP_K="1", NANO_HOST_SAMPLER="1")
    off = child(path, V)
    assert len(dev["ids5"]) == 20
    # with the knob: the device sampler and the host loops apply the same truncation
    assert dev["ids5"] == host["ids5"] and dev["batch5"] == host["batch5"]
    assert dev["ids0"] == host["ids0"] and dev["batch0"] == host["batch0"]
    # without the knob top_k is stored and ignored: the top_k = 0 ids
    assert off["ids5"] == off["ids0"] == dev["ids0"] and off["batch5"] == off["batch0"] == dev["batch0"]
    # and the knob does something
    assert dev["ids5"] != dev["ids0"] and dev["batch5"] != dev["batch0"]
