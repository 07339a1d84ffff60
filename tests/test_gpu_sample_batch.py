"""GPU tests of the batched device sampler (nano_hip_forward_sample_batch / nano_hip_op_sample_batch / nano_forward_batch_sample):
every row of a batched step is sampled on the device, and each row's result is what a one-row call returns for that row's logits
alone, field by field -- which test_gpu_sampler.py holds to the reference."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD, synth_model
from nano_amd import binding as nb
import sampler_cases as sc

pytestmark = pytest.mark.gpu
CAP = 8192          # NANO_SAMPLE_MAX_CANDIDATES
EINVAL = -1


def fields(r):
    return (r.token, r.status, r.n_candidates, r.n_sorted, r.nucleus, tuple(r.top), r.sum_bits, r.walked_chunks)


def single(m, l, row):
    rp, temp, top_p, coin, hist = row
    return m.op_sample(l, hist if hist is not None else [], rp, temp, top_p, coin)


@pytest.fixture(scope="module")
def bigvocab64(model_dir):
    path, spec = synth_model(model_dir, "bigvocab-qwen3", "f32", 0)
    m = nb.load_model_file(path, max_seq_len=512, max_batch=64)
    yield m
    m.close()


def test_op_sample_batch_golden(bigvocab64):
    """The 48 golden rows (12 cases x 4 coins at V = 151 936) in one call: each row's token, candidate count and denominator equal the
    compiled reference's; the near-uniform rows go through the wide phase; a shuffled batch gives every row the same result; every row
    equals the single-row sampler's result on that row alone."""
    m = bigvocab64
    g = np.load(os.path.join(GOLD, "sampler_logits.npz"))
    assert [repr(c) for c in sc.CASES] == [str(c) for c in g["cases"]]
    logits, rows, where = [], [], []
    for ci, (seed, sigma, mode, rp, temp, top_p, nh) in enumerate(sc.CASES):
        l, h = sc.logits_of(seed, sigma, mode), sc.history_of(seed, nh)
        for ki, coin in enumerate(sc.COINS):
            logits.append(l); rows.append((rp, temp, top_p, coin, h)); where.append((ci, ki))
    L = np.stack(logits)
    got = m.op_sample_batch(L, rows)
    wide = 0
    for r, (ci, ki), (rp, temp, top_p, coin, h) in zip(got, where, rows):
        assert r.status == 0 and r.token == int(g["tokens"][ci, ki]), (ci, ki, r.status, r.token)
        if temp == 0.0:
            continue
        n_ref = int(g["n_candidates"][ci])
        assert r.n_candidates == n_ref and r.sum_bits == int(g["denominator_bits"][ci]), (ci, ki)
        if n_ref <= CAP:
            assert r.n_sorted == n_ref, (ci, ki)
        if sc.CASES[ci][2] == "plain" and sc.CASES[ci][1] < 1.0:
            assert r.n_sorted == r.n_candidates > CAP, (ci, ki)
        wide += r.n_sorted > CAP
    assert wide >= 4
    perm = np.random.default_rng(1).permutation(len(rows))
    shuffled = m.op_sample_batch(L[perm], [rows[i] for i in perm])
    for j, i in enumerate(perm):
        assert fields(shuffled[j]) == fields(got[i]), (i, j)
    for i in range(len(rows)):
        assert fields(single(m, L[i], rows[i])) == fields(got[i]), i


@pytest.mark.parametrize("preset", ["tiny-nano", "tiny-qwen3"])
def test_op_sample_batch_vs_oracle_small_vocab(oracle, model_dir, preset):
    """V = 512 / 1024: batches of 1..64 rows with random penalties (< 1 and > 1), temperatures (0 included), top_p (negative
    included) and coins, each row against the oracle's sampler."""
    path, spec = synth_model(model_dir, preset, "f32", 0)
    m = nb.load_model_file(path, max_seq_len=32, max_batch=64)
    V = spec.vocab_size
    rng = np.random.default_rng(17)
    for B in (1, 2, 7, 33, 64):
        L = (rng.choice([0.2, 1.0, 3.0, 12.0], size=(B, 1)) * rng.standard_normal((B, V))).astype(np.float32)
        L[::3] = (np.round(L[::3] * 2) / 2).astype(np.float32)
        rows = []
        for _ in range(B):
            h = rng.integers(0, V, size=int(rng.integers(0, 30))).astype(np.uint32)
            rows.append((float(rng.choice([0.8, 1.0, 1.1, 1.5])), float(rng.choice([0.0, 0.5, 1.0, 1.7])),
                         float(rng.choice([-0.05, 0.3, 0.9, 0.999])), float(rng.random(dtype=np.float32)), h))
        got = m.op_sample_batch(L, rows)
        for i, (r, (rp, temp, top_p, coin, h)) in enumerate(zip(got, rows)):
            tok, n = oracle.sample_logits(L[i], h, rp, temp, top_p, coin)
            assert r.status == 0 and r.token == tok, (B, i, r.token, tok)
            if temp != 0.0:
                assert r.n_candidates == n, (B, i)
    m.close()


def run_pair(path, V, B, steps=8, seed=0, kv_paged=None, max_seq_len=48):
    """Model A: forward_sample_batch; model B (same file): forward with logits + the single-row op_sample per row.  Slots start at
    staggered positions (prefilled), histories grow by the sampled ids, which are fed back to both."""
    rng = np.random.default_rng(seed)
    a = nb.load_model_file(path, max_seq_len=max_seq_len, max_batch=B, kv_paged=kv_paged)
    b = nb.load_model_file(path, max_seq_len=max_seq_len, max_batch=B, kv_paged=kv_paged)
    try:
        hist, tok, pos = [], [], []
        for s in range(B):
            n = 1 + (s * 5) % 11
            ids = [int(x) for x in rng.integers(0, V, size=n)]
            if n > 1:
                a.prefill(ids[:-1], 0, s); b.prefill(ids[:-1], 0, s)
            hist.append(ids[:-1]); tok.append(ids[-1]); pos.append(n - 1)
        params = [(float(rng.choice([0.9, 1.0, 1.2])), float(rng.choice([0.0, 0.6, 1.0])), float(rng.choice([0.5, 0.9])))
                  for _ in range(B)]
        n_wide = 0
        for step in range(steps):
            rows = [(rp, t, p, float(rng.random(dtype=np.float32)), np.array(hist[s], np.uint32)) for s, (rp, t, p) in enumerate(params)]
            lg, _ = b.forward(tok, pos)
            got = a.forward_sample_batch(tok, pos, rows)
            for s in range(B):
                want = single(b, lg[s], rows[s])
                assert fields(got[s]) == fields(want), (B, step, s, fields(got[s]), fields(want))
                assert got[s].status == 0
                n_wide += got[s].n_sorted > CAP
            for s in range(B):
                hist[s].append(tok[s]); tok[s] = int(got[s].token); pos[s] += 1
        return n_wide
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("preset,quant,gs,batches", [
    ("tiny-qwen3", "q80", 64, (1, 3, 8, 17, 64)),
    ("tiny-nano", "f32", 0, (1, 3, 8, 17, 64)),
    ("tiny-qwen3", "q4k", 0, (1, 3, 8, 17, 64)),
    ("bigvocab-qwen3", "f32", 0, (3, 17)),
    ("qwen3-0.6b-3l", "q80", 64, (17, 64)),
])
def test_forward_sample_batch_vs_single_rows(model_dir, preset, quant, gs, batches):
    path, spec = synth_model(model_dir, preset, quant, gs)
    for B in batches:
        run_pair(path, spec.vocab_size, B, seed=B)


def test_forward_sample_batch_paged_kv(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 32)
    run_pair(path, spec.vocab_size, 8, seed=5, kv_paged=True)


def test_history_cache_starts_over(model_dir):
    """A slot whose history is not an extension of its last one (unrelated, shorter, same length but different) gives what a freshly
    loaded model gives."""
    path, spec = synth_model(model_dir, "tiny-qwen3", "f32", 0)
    V = spec.vocab_size
    rng = np.random.default_rng(8)
    m = nb.load_model_file(path, max_seq_len=32, max_batch=4)
    L = (3.0 * rng.standard_normal((4, V))).astype(np.float32)
    h0 = [rng.integers(0, V, size=12).astype(np.uint32) for _ in range(4)]
    m.op_sample_batch(L, [(1.5, 0.8, 0.9, 0.4, h) for h in h0])
    m.op_sample_batch(L, [(1.5, 0.8, 0.9, 0.4, np.concatenate([h, [7, 9]]).astype(np.uint32)) for h in h0])     # extensions
    h1 = [rng.integers(0, V, size=20).astype(np.uint32), h0[1][:5].copy(), rng.integers(0, V, size=14).astype(np.uint32),
          np.zeros(0, np.uint32)]
    rows = [(1.5, t, 0.9, 0.61, h) for h, t in zip(h1, (0.8, 0.0, 1.2, 0.8))]
    got = m.op_sample_batch(L, rows)
    m.close()
    f = nb.load_model_file(path, max_seq_len=32, max_batch=4)
    want = f.op_sample_batch(L, rows)
    f.close()
    assert [fields(r) for r in got] == [fields(r) for r in want]


def test_history_record_shared_by_one_row_and_batched_calls(model_dir):
    """A one-row call is slot 0 of a batch of one, so slot 0's record of the marked ids serves both entry points.  Interleaved
    calls -- one row on history A, a batch with slot 0 on B and slot 1 on C, one row on an extension of A, one row (arg-max) on a
    further extension, a batch extending that and C -- each give what a freshly loaded model gives for the same call."""
    path, spec = synth_model(model_dir, "tiny-qwen3", "f32", 0)
    V = spec.vocab_size
    rng = np.random.default_rng(21)
    L = (3.0 * rng.standard_normal((2, V))).astype(np.float32)
    ids = lambda n: rng.integers(0, V, size=n).astype(np.uint32)
    A, B, C = ids(12), ids(9), ids(15)
    A2 = np.concatenate([A, ids(3)]); A3 = np.concatenate([A2, ids(2)])
    calls = [(L[0], [(1.5, 0.8, 0.9, 0.4, A)]),
             (L, [(1.5, 0.8, 0.9, 0.4, B), (1.3, 1.0, 0.9, 0.7, C)]),
             (L[1], [(1.5, 0.8, 0.9, 0.2, A2)]),
             (L[0], [(1.2, 0.0, 0.9, 0.0, A3)]),
             (L, [(1.5, 0.8, 0.9, 0.6, np.concatenate([A3, ids(4)])), (1.3, 1.0, 0.9, 0.3, np.concatenate([C, ids(2)]))])]

    def call(m, l, rows):
        if l.ndim == 1:
            return [fields(single(m, l, rows[0]))]
        return [fields(r) for r in m.op_sample_batch(l, rows)]

    m = nb.load_model_file(path, max_seq_len=32, max_batch=2)
    got = [call(m, l, rows) for l, rows in calls]
    m.close()
    for k, ((l, rows), g) in enumerate(zip(calls, got)):
        f = nb.load_model_file(path, max_seq_len=32, max_batch=2)
        assert call(f, l, rows) == g, k
        assert all(r[1] == 0 for r in g), k
        f.close()


def xorshift_f32(state):
    M = (1 << 64) - 1
    s = state
    s ^= s >> 12; s ^= (s << 25) & M; s ^= s >> 27
    u = ((s * 0x2545F4914F6CDD1D) & M) >> 32
    return s, float(np.float32((u >> 8) / 16777216.0))


def test_engine_forward_batch_sample(oracle, model_dir):
    """nano_forward_batch_sample over 8 sequences with their own samplers against nano_forward_batch's logits on a second context,
    sampled by the oracle with the same xorshift coin stream: the same ids, and the same final generator states."""
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    V, B = spec.vocab_size, 8
    ea = nb.Engine(path, max_seq_len=32, max_batch=B)
    eb = nb.Engine(path, max_seq_len=32, max_batch=B)
    cfg = [(1.1, 0.8, 0.9), (1.0, 1.0, 0.9), (1.3, 0.0, 0.9), (0.9, 0.5, 0.5), (1.0, 0.0, 1.0), (1.2, 1.5, 0.95), (1.0, 0.7, 0.3), (1.1, 1.0, 0.99)]
    seeds = [11 + 1000 * i for i in range(B)]
    samplers = [ea.build_sampler(V, rp, t, p, sd) for (rp, t, p), sd in zip(cfg, seeds)]
    states = list(seeds)
    try:
        rng = np.random.default_rng(4)
        ids = [[int(x) for x in rng.integers(0, V, size=3)] for _ in range(B)]
        for p in range(2):                                                 # the prompts, both contexts
            for e in (ea, eb):
                e.forward_batch([ids[s][p] for s in range(B)], [p] * B, want_logits=False)
        for p in range(2, 12):
            tok = [ids[s][p] for s in range(B)]
            hists = [np.array(ids[s][:p], np.uint32) for s in range(B)]
            got = ea.forward_batch_sample(tok, [p] * B, samplers, hists)
            lg = eb.forward_batch(tok, [p] * B, vocab=V)
            for s, (rp, t, tp) in enumerate(cfg):
                coin = 0.0
                if t != 0.0:
                    states[s], coin = xorshift_f32(states[s])
                want, _n = oracle.sample_logits(lg[s], hists[s], rp, t, tp, coin)
                assert int(got[s]) == want, (p, s, int(got[s]), want)
                ids[s].append(int(got[s]))
        assert [int(sp.contents.rng_state) for sp in samplers] == states
    finally:
        for sp in samplers:
            ea.free_sampler(sp)
        ea.close(); eb.close()


def test_errors_leave_the_model_usable(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 32)
    V = spec.vocab_size
    m = nb.load_model_file(path, max_seq_len=32, max_batch=4)
    ref = nb.load_model_file(path, max_seq_len=32, max_batch=4)
    L = nb.lib()
    row = (1.2, 0.8, 0.9, 0.3, np.array([1, 2], np.uint32))
    out = (nb.NanoHipSample * 8)()
    arr, keep = nb.sample_params([row] * 5)
    t5 = np.arange(5, dtype=np.uint32); p5 = np.zeros(5, np.uint32)
    assert L.nano_hip_forward_sample_batch(m.h, t5, p5, 5, arr, out) == EINVAL                     # batch > max_batch
    bad, keep2 = nb.sample_params([row, (1.2, 0.8, 0.9, 0.3, np.array([3, V], np.uint32))])
    assert L.nano_hip_forward_sample_batch(m.h, t5[:2], p5[:2], 2, bad, out) == EINVAL            # history id >= V
    assert L.nano_hip_op_sample_batch(m.h, np.zeros(2 * V, np.float32), 2, bad, out) == EINVAL
    assert L.nano_hip_forward_sample_batch(m.h, t5[:2], p5[:2], 2, None, out) == EINVAL           # null params
    assert L.nano_hip_op_sample_batch(m.h, np.zeros(2 * V, np.float32), 2, None, out) == EINVAL
    rows = [(1.2, 0.8, 0.9, 0.3, np.array([1, 2], np.uint32)), (1.0, 0.0, 0.9, 0.0, None), (0.9, 1.0, 0.5, 0.8, np.array([5], np.uint32))]
    tok, pos = [3, 4, 5], [0, 0, 0]
    for step in range(3):
        got = m.forward_sample_batch(tok, pos, rows)
        lg, _ = ref.forward(tok, pos)
        for s in range(3):
            assert fields(got[s]) == fields(single(ref, lg[s], rows[s])), (step, s)
        tok = [int(r.token) for r in got]; pos = [p + 1 for p in pos]
    m.close(); ref.close()
