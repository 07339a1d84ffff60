"""GPU tests of greedy decode with lookup drafts (nano_hip_decode_lookup, nano_hip_verify_draft, NANO_LOOKUP_DRAFT in the engine).

The ids must be nano_hip_decode_greedy's on every shape where batched prefill is asserted bit-identical to token-by-token feeding
(test_gpu_e2e.py test_batched_prefill_equals_token_by_token), and the stats must be what tests/lookup_ref.py simulate() gives when it is
replayed on those ids: the loop took exactly the steps the definitions prescribe."""
import ctypes as C
import os

import numpy as np
import pytest

import lookup_ref as lr
from conftest import synth_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf

pytestmark = pytest.mark.gpu

S = 128
N_PROMPT = 5
N_NEW = 100                          # the loop crosses position 64
PERIODIC_SEED = 39                   # model seed of the periodic-by-construction cases (picked on the GPU: see test_periodic_models)


def model_file(model_dir, preset, quant, gs, seed=39, zero_mixers=False):
    """A synthetic model whose RoPE table covers S positions; zero_mixers: Wo and W2 zeroed (Q80: their scales too), so that the residual
    stream stays the fed id's embedding and the logits depend on the last id only."""
    if not zero_mixers and mf.preset(preset, quant, group_size=gs).block_size >= S:
        return synth_model(model_dir, preset, quant, gs, seed)
    spec = mf.preset(preset, quant, group_size=gs, block_size=max(S, mf.preset(preset, quant, group_size=gs).block_size))
    path = os.path.join(model_dir, f"lookup-{preset}-{quant}-{gs}-{seed}-{int(zero_mixers)}.bin")
    if not os.path.exists(path):
        lay = mf.write_model(path, spec, seed=seed)
        if zero_mixers:
            raw = np.memmap(path, dtype=np.uint8, mode="r+")
            for name, (off, nbytes) in lay.entries.items():
                if name.split(".")[0] in ("wo", "w2"):
                    raw[lay.params_offset + off: lay.params_offset + off + nbytes] = 0
            raw.flush(); del raw
    return path, spec


def prepare(m, mode):
    if mode == "strict":
        m.set_strict(True)
    if mode == "exact":
        m.set_exact(True)


_greedy = {}


def greedy_ids(path, prompt, mode=None, **kw):
    """the ids nano_hip_decode_greedy gives after the prompt, up to the end of the context (computed once per case, never modified)"""
    key = (path, prompt.tobytes(), mode, tuple(sorted(kw.items())))
    if key not in _greedy:
        m = nb.load_model_file(path, max_seq_len=S, max_batch=1, **kw)
        prepare(m, mode)
        m.prefill(prompt[:-1])
        ids = m.decode_greedy([int(prompt[-1])], [len(prompt) - 1], S - (len(prompt) - 1))[:, 0].copy()
        m.close()
        ids.setflags(write=False)
        _greedy[key] = ids
    return _greedy[key]


_runs = {}


def lookup_run(path, prompt, D, mode=None, **kw):
    """(ids, stats, the max_draft the model runs) of nano_hip_decode_lookup for N_NEW ids after the prompt; once per case"""
    key = (path, prompt.tobytes(), D, mode, tuple(sorted(kw.items())))
    if key not in _runs:
        m = nb.load_model_file(path, max_seq_len=S, max_batch=1, **kw)
        prepare(m, mode)
        m.prefill(prompt[:-1])
        d_eff = 0 if mode else min(D, m.prefill_chunk_tokens() - 1)
        ids, st = m.decode_lookup(prompt, N_NEW, max_draft=D)
        m.close()
        _runs[key] = (ids, st, d_eff)
    return _runs[key]


def check_against_greedy(path, spec, D, what, mode=None, **kw):
    prompt = mf.prompt_ids(77, N_PROMPT, spec.vocab_size)
    want = greedy_ids(path, prompt, mode, **kw)
    ids, st, d_eff = lookup_run(path, prompt, D, mode, **kw)
    sim_ids, sim = lr.simulate(prompt.tolist(), want.tolist(), N_NEW, d_eff, 1, 3, seq_limit=S)
    print(f"{what} D={D} (runs {d_eff}): {st}")
    assert sim_ids == want[:N_NEW].tolist()                                 # (the lossless property, on this sequence)
    assert ids.tolist() == want[:N_NEW].tolist(), f"{what}: ids differ from decode_greedy's at index {int(np.argmax(ids != want[:ids.size])) if ids.size == N_NEW else ids.size}"
    assert st == sim, (what, st, sim)
    return st


FREE = [("tiny-qwen3", "q80", 64), ("tiny-nano", "f32", 0), ("tiny-nano-odd", "q4k", 0), ("qwen3-0.6b-3l", "q80", 64)]
PERIODIC = [("tiny-nano-ucls", "f32", 0), ("tiny-qwen3-ucls", "q80", 64)]


@pytest.mark.parametrize("D", [3, 7, 15])
@pytest.mark.parametrize("preset,quant,gs", FREE)
def test_free_running_models(model_dir, preset, quant, gs, D):
    path, spec = model_file(model_dir, preset, quant, gs)
    check_against_greedy(path, spec, D, f"{preset}/{quant}")


@pytest.mark.parametrize("D", [3, 7, 15])
@pytest.mark.parametrize("preset,quant,gs", PERIODIC)
def test_periodic_models(model_dir, preset, quant, gs, D):
    """Wo and W2 zeroed: the next id is a function of the last one, so the sequence falls into a loop and drafts are accepted"""
    path, spec = model_file(model_dir, preset, quant, gs, seed=PERIODIC_SEED, zero_mixers=True)
    prompt = mf.prompt_ids(77, N_PROMPT, spec.vocab_size)
    want = greedy_ids(path, prompt)
    nxt = {}
    for a, b in zip([int(prompt[-1])] + want[:-1].tolist(), want.tolist()):
        assert nxt.setdefault(a, b) == b, "the zeroed model's next id must depend on the last id only"
    _, sim = lr.simulate(prompt.tolist(), want.tolist(), N_NEW, 7, 1, 3, seq_limit=S)
    print(f"periodic {preset}/{quant} seed {PERIODIC_SEED}: simulate at D=7 predicts {sim}")
    assert sim["accepted"] >= 30, "pick another PERIODIC_SEED: decode_greedy's ids must hold a loop long before 100 ids"
    check_against_greedy(path, spec, D, f"periodic {preset}/{quant}")


def test_some_draft_was_rejected(model_dir):
    """over both groups: the verify path has seen a wrong draft"""
    rejected = 0
    for zero, cases in ((False, FREE), (True, PERIODIC)):
        for preset, quant, gs in cases:
            path, spec = model_file(model_dir, preset, quant, gs, seed=PERIODIC_SEED if zero else 39, zero_mixers=zero)
            for D in (3, 7, 15):
                _, st, d_eff = lookup_run(path, mf.prompt_ids(77, N_PROMPT, spec.vocab_size), D)
                rejected += st["steps_verify"] * d_eff - st["accepted"]
    assert rejected >= 1


@pytest.mark.parametrize("preset,quant,gs", [("tiny-qwen3", "q80", 64), ("hd256-qwen3", "q80", 64), ("wide-qwen3", "q80", 64)])
def test_verify_argmax_is_prefill_scores(model_dir, preset, quant, gs):
    path, spec = synth_model(model_dir, preset, quant, gs)
    ids = mf.prompt_ids(91, 70, spec.vocab_size)                             # crosses the 64-position bucket: two chunks
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    want = m.prefill_score(ids)["argmax"]
    got, a = m.verify_draft(ids)
    again, _ = m.verify_draft(ids[:23], pos0=0)
    m.close()
    assert np.array_equal(got, want) and np.array_equal(again, want[:23])
    assert a == lr.accepted(ids.tolist(), want.tolist())


@pytest.mark.parametrize("kw", [{}, {"kv_paged": True, "kv_f16": False}, {"kv_f16": True}], ids=["contiguous", "paged", "fp16"])
def test_verify_draft_accepts_and_recovers(model_dir, kw):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    prompt = mf.prompt_ids(77, N_PROMPT, spec.vocab_size)
    g = greedy_ids(path, prompt, **kw)
    p0 = N_PROMPT - 1
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1, **kw)
    m.prefill(prompt[:-1])
    am, a = m.verify_draft([int(prompt[-1])] + g[:7].tolist(), pos0=p0)     # a true continuation
    assert a == 7 and am.tolist() == g[:8].tolist()
    for j in (0, 3, 6):                                                     # wrong at draft index j
        d = g[:7].tolist()
        d[j] = (d[j] + 1) % spec.vocab_size
        am, a = m.verify_draft([int(prompt[-1])] + d, pos0=p0)
        assert a == j and am[:j + 1].tolist() == g[:j + 1].tolist()
    # after the rejected draft (j = 6: rows p0+7 hold a wrong id's K / V): on from the accepted position, the ids of a run that never drafted
    rest = m.decode_greedy([int(am[a])], [p0 + a + 1], 30)[:, 0]
    m.close()
    assert rest.tolist() == g[a + 1: a + 31].tolist()


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_verify_draft_in_a_forked_slot_leaves_the_source(model_dir, paged):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    prompt = mf.prompt_ids(78, 40, spec.vocab_size)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=2, kv_paged=paged, kv_f16=False)
    m.prefill(prompt[:-1])
    rows = lambda: [m.read_state(w, spec.kv_dim, slot=0, layer=l, pos=p).copy() for w in "kv" for l in range(spec.n_layer) for p in (0, 17, 38)]
    before = rows()
    m.kv_fork(0, len(prompt) - 1, [1])
    am1, _ = m.verify_draft(prompt[-1:].tolist() + [1, 2, 3], pos0=len(prompt) - 1, slot=1)
    after = rows()
    am0, _ = m.verify_draft(prompt[-1:].tolist() + [1, 2, 3], pos0=len(prompt) - 1, slot=0)
    m.close()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before, after))
    assert np.array_equal(am0, am1)


def test_no_draft_is_decode_greedy(model_dir):
    path, spec = model_file(model_dir, "tiny-qwen3", "q80", 64)
    st = check_against_greedy(path, spec, 0, "tiny-qwen3/q80")
    assert st["steps_verify"] == 0 and st["steps_plain"] == N_NEW


@pytest.mark.parametrize("mode", ["strict", "exact"])
def test_ordered_modes_take_plain_steps(model_dir, mode):
    path, spec = model_file(model_dir, "tiny-qwen3", "q80", 64)
    st = check_against_greedy(path, spec, 7, f"tiny-qwen3/q80 {mode}", mode=mode)
    assert st["steps_verify"] == 0 and st["steps_plain"] == N_NEW


def test_stop_clip_steps_and_continued_histories(model_dir):
    path, spec = model_file(model_dir, "tiny-qwen3-ucls", "q80", 64, seed=PERIODIC_SEED, zero_mixers=True)
    prompt = mf.prompt_ids(77, N_PROMPT, spec.vocab_size)
    g = greedy_ids(path, prompt).tolist()
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    m.prefill(prompt[:-1])
    stop = g[40]
    ids, st = m.decode_lookup(prompt, N_NEW, stop_token=stop)
    assert ids.tolist() == g[:g.index(stop) + 1] and st["emitted"] == ids.size
    room = S - (N_PROMPT - 1)
    ids, st = m.decode_lookup(prompt, room)                                  # max_new up to the end of the context
    assert ids.tolist() == g[:room] and st == lr.simulate(prompt.tolist(), g, room, 7, 1, 3, seq_limit=S)[1]
    with pytest.raises(nb.NanoHipError, match="error -1"):
        m.decode_lookup(prompt, room + 1)
    # max_steps = 1, call after call with the history grown by what came back: the device keeps the history, only new ids go up
    h, plain, verify = prompt.tolist(), 0, 0
    while len(h) < N_PROMPT + N_NEW:
        ids, st = m.decode_lookup(h, N_PROMPT + N_NEW - len(h), max_steps=1)
        assert 1 <= ids.size <= 8 and st["steps_plain"] + st["steps_verify"] == 1
        plain += st["steps_plain"]; verify += st["steps_verify"]
        h += ids.tolist()
    assert h[N_PROMPT:] == g[:N_NEW] and verify >= 1
    ids, _ = m.decode_lookup(prompt, 0)
    assert ids.size == 0
    m.close()


def test_refused_calls_queue_nothing(model_dir):
    path, spec = model_file(model_dir, "tiny-qwen3", "q80", 64)
    prompt = mf.prompt_ids(77, N_PROMPT, spec.vocab_size)
    g = greedy_ids(path, prompt)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    m.prefill(prompt[:-1])
    bad = [dict(max_draft=16), dict(ngram_max=0), dict(ngram_max=5), dict(ngram_min=0), dict(ngram_min=3, ngram_max=2)]
    for kw in bad:
        with pytest.raises(nb.NanoHipError, match="error -1"):
            m.decode_lookup(prompt, 10, **kw)
    for hist, max_new in (([], 4), ([1, spec.vocab_size], 4), (prompt, S), (list(range(S)) + [1, 2], 1)):
        with pytest.raises(nb.NanoHipError, match="error -1"):
            m.decode_lookup(hist, max_new)
    lib = nb.lib()
    p = nb.NanoHipLookupParams(7, 3, 1, 0xFFFFFFFF, 0)
    out, n = np.zeros(8, np.uint32), C.c_uint32(0)
    h = np.ascontiguousarray(prompt, np.uint32)
    for args in ((m.h, None, 5, 4, C.byref(p), out.ctypes.data, C.byref(n), None), (m.h, h.ctypes.data, 5, 4, None, out.ctypes.data, C.byref(n), None),
                 (m.h, h.ctypes.data, 5, 4, C.byref(p), None, C.byref(n), None), (m.h, h.ctypes.data, 5, 4, C.byref(p), out.ctypes.data, None, None)):
        assert lib.nano_hip_decode_lookup(*args) == -1
    with pytest.raises(nb.NanoHipError, match="error -1"):
        m.verify_draft([], pos0=4)
    with pytest.raises(nb.NanoHipError, match="error -1"):
        m.verify_draft([1, 2, 3], pos0=S - 2)
    # nothing was queued: the slot still continues the prompt
    ids = m.decode_greedy([int(prompt[-1])], [N_PROMPT - 1], 8)[:, 0]
    m.close()
    assert ids.tolist() == g[:8].tolist()


def test_engine_switch(model_dir):
    """generate_next_token with the lookup drafts on returns the ids it returns without them; a caller that overwrites a returned id
    makes the queue drop"""
    path, spec = model_file(model_dir, "tiny-qwen3-ucls", "q80", 64, seed=PERIODIC_SEED, zero_mixers=True)
    prompt = mf.prompt_ids(77, N_PROMPT, spec.vocab_size)
    lib = nb.lib()
    lib.nano_set_lookup_draft.argtypes = [C.c_int]

    def run(draft, overwrite_at):
        lib.nano_set_lookup_draft(draft)
        try:
            e = nb.Engine(path, max_seq_len=S)
            ids = np.zeros(S + 1, np.uint32)
            ids[:N_PROMPT] = prompt
            for pos in range(N_PROMPT - 1):
                e.next_token(ids, pos, 1)
            for i in range(N_NEW):
                pos = N_PROMPT - 1 + i
                t = e.next_token(ids, pos, 0)
                ids[pos + 1] = (t + 1) % spec.vocab_size if i in overwrite_at else t
            e.close()
        finally:
            lib.nano_set_lookup_draft(0)
        return ids[:N_PROMPT + N_NEW].tolist()

    plain = run(0, ())
    assert run(7, ()) == plain
    assert plain[N_PROMPT:] == greedy_ids(path, prompt)[:N_NEW].tolist()
    over = (50, 51, 70)                                                      # inside the loop the sequence has fallen into: the queue is not empty there
    assert run(7, over) == run(0, over)
