"""GPU tests of greedy decode with a draft model (nano_hip_decode_draft, nano_set_draft_model in the engine).

Every emitted id is the arg-max of a target row whose whole prefix is emitted ids: the ids must be a SEPARATE target handle's
nano_hip_decode_greedy ids whatever the draft model is, and the stats must be what tests/draft_ref.py simulate() gives for the draft
model's own continuations: the loop took exactly the rounds the definitions prescribe."""
import ctypes as C

import numpy as np
import pytest

import draft_ref as dr
from nano_amd import binding as nb
from nano_amd import modelfile as mf
from test_gpu_lookup_decode import FREE, model_file, greedy_ids, prepare

pytestmark = pytest.mark.gpu

S = 128
N_PROMPT = 5
N_NEW = 100                          # the loop crosses position 64
DS = [1, 4, 15]


def load(path, **kw):
    return nb.load_model_file(path, max_seq_len=S, max_batch=1, **kw)


def prompt_of(spec, n=N_PROMPT):
    return mf.prompt_ids(77, n, spec.vocab_size)


def continuation_of(full):
    """draft_fn of a draft that continues like `full` (prompt + the greedy ids of that model)"""
    return lambda prefix, k: full[len(prefix): len(prefix) + k]


def run(tpath, dpath, prompt, D, max_new=N_NEW, tkw=None, dkw=None, mode=None, **call):
    """one nano_hip_decode_draft call on fresh handles: (ids, stats, the max_draft the target runs)"""
    t, d = load(tpath, **(tkw or {})), load(dpath, **(dkw or {}))
    prepare(t, mode)
    t.prefill(prompt[:-1])
    d_eff = 0 if mode else min(D, t.prefill_chunk_tokens() - 1)
    ids, st = t.decode_draft(d, prompt, max_new, max_draft=D, **call)
    t.close(); d.close()
    return ids, st, d_eff


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("preset,quant,gs", FREE)
def test_draft_is_a_second_handle_on_the_same_file(model_dir, preset, quant, gs, D):
    """these are the shapes where chunk rows carry token-by-token bits: the draft's ids are the target's, every draft is accepted"""
    path, spec = model_file(model_dir, preset, quant, gs)
    prompt = prompt_of(spec)
    want = greedy_ids(path, prompt)
    ids, st, d_eff = run(path, path, prompt, D)
    full = prompt.tolist() + want.tolist()
    sim_ids, sim = dr.simulate(prompt.tolist(), want.tolist(), N_NEW, d_eff, continuation_of(full), seq_limit=S)
    print(f"{preset}/{quant} D={D} (runs {d_eff}): {st}")
    assert sim_ids == want[:N_NEW].tolist()
    assert ids.tolist() == want[:N_NEW].tolist()
    assert st == sim, (st, sim)
    assert st["accepted"] == st["drafted"] and st["rounds_verify"] >= 1
    # the count the bucket rule prescribes: round after round from n = N_PROMPT, every round emitting all its rows
    n, left, verify = N_PROMPT, N_NEW, 0
    while left:
        rows = dr.round_rows(n, left, d_eff, S)
        verify += rows > 1
        n += rows; left -= rows
    assert st["rounds_verify"] == verify


# (target, draft): the same preset with another seed; another preset with the same vocabulary (512; 20 000 -- Qwen3-0.6B's layer
# shapes drafting for Qwen3-4B's)
OTHER = [(("tiny-qwen3", "q80", 64, 39), ("tiny-qwen3", "q80", 64, 40)),
         (("tiny-qwen3-ucls", "q80", 64, 39), ("tiny-qwen3", "q80", 64, 40)),          # (an un-shared classifier: ids that do not follow the fed id)
         (("tiny-nano", "f32", 0, 39), ("tiny-nano-odd", "q4k", 0, 39)),
         (("wide-qwen3-2l", "q80", 64, 39), ("qwen3-0.6b-3l", "q80", 64, 39))]
_other = {}


def other_run(model_dir, target, draft, D):
    key = (target, draft, D)
    if key not in _other:
        tpath, spec = model_file(model_dir, *target[:3], seed=target[3])
        dpath, _ = model_file(model_dir, *draft[:3], seed=draft[3])
        prompt = prompt_of(spec)
        _other[key] = (tpath, dpath, spec, prompt) + run(tpath, dpath, prompt, D)
    return _other[key]


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("target,draft", OTHER, ids=["other-seed", "other-seed-ucls", "nano-odd-for-nano", "0.6b-shapes-for-4b-shapes"])
def test_any_draft_gives_the_targets_ids(model_dir, target, draft, D):
    tpath, dpath, spec, prompt, ids, st, d_eff = other_run(model_dir, target, draft, D)
    want = greedy_ids(tpath, prompt)
    print(f"{target[0]} <- {draft[0]} D={D} (runs {d_eff}): {st}")
    assert st["emitted"] == ids.size == N_NEW and st["drafted"] >= st["accepted"]
    if target[0].startswith("wide"):
        # wide matrices: every id is the arg-max of a fast-path row whose prefix is the emitted ids (nano_hip_verify_draft's promise), at
        # a near-tie not necessarily decode_greedy's.  Launches of >= 3 rows normalise through another reduction tree than those of 1
        # and 2 rows, and a round has 1 .. D + 1 rows (the bucket rule shortens it): the id is the chunk row's or the one-row step's
        fed = [int(prompt[-1])] + ids.tolist()[:-1]
        m = load(tpath)
        m.prefill(prompt[:-1])
        chunk, _ = m.verify_draft(fed, pos0=N_PROMPT - 1)
        step = [int(m.forward([tok], [N_PROMPT - 1 + i], want_logits=False, want_argmax=True)[1][0]) for i, tok in enumerate(fed)]
        m.close()
        got = ids.tolist()
        print("   ids equal decode_greedy's:", got == want[:N_NEW].tolist(), " differ from the chunk rows' at", [i for i in range(N_NEW) if got[i] != chunk[i]],
              "from the one-row steps' at", [i for i in range(N_NEW) if got[i] != step[i]])
        assert all(got[i] in (int(chunk[i]), step[i]) for i in range(N_NEW))
        if d_eff == 1:
            assert got == want[:N_NEW].tolist()                             # rounds of at most two rows: the one-row step's bits
    else:
        assert ids.tolist() == want[:N_NEW].tolist()


def test_some_draft_was_rejected_and_the_round_after_it_verified(model_dir):
    rejected = after = 0
    for target, draft in OTHER:
        for D in DS:
            st = other_run(model_dir, target, draft, D)[5]
            rejected += st["drafted"] - st["accepted"]
            after += st["rounds_verify"] >= 2 and st["drafted"] > st["accepted"]
    assert rejected >= 1 and after >= 1


def test_stats_with_the_draft_models_own_continuations(model_dir):
    """draft_fn asks a third handle of the draft model: prefill the prefix, decode_greedy k steps"""
    target, draft = OTHER[1]
    tpath, spec = model_file(model_dir, *target[:3], seed=target[3])
    dpath, _ = model_file(model_dir, *draft[:3], seed=draft[3])
    prompt = prompt_of(spec)
    want = greedy_ids(tpath, prompt)
    ids, st, d_eff = run(tpath, dpath, prompt, 4, max_new=40)
    third = load(dpath)

    def draft_fn(prefix, k):
        third.prefill(prefix[:-1])
        return third.decode_greedy([prefix[-1]], [len(prefix) - 1], k)[:, 0].tolist()

    sim_ids, sim = dr.simulate(prompt.tolist(), want.tolist(), 40, d_eff, draft_fn, seq_limit=S)
    third.close()
    assert ids.tolist() == sim_ids == want[:40].tolist()
    assert st == sim, (st, sim)


@pytest.mark.parametrize("dkw", [{"kv_f16": True}, {"kv_fp8": True}, {"kv_paged": True, "kv_f16": False}], ids=["fp16", "fp8", "paged"])
def test_the_drafts_cache_does_not_matter(model_dir, dkw):
    tpath, spec = model_file(model_dir, "tiny-qwen3", "q80", 64)
    dpath, _ = model_file(model_dir, "tiny-qwen3", "q80", 64, seed=40)
    prompt = prompt_of(spec)
    ids, st, _ = run(tpath, dpath, prompt, 4, dkw=dkw)
    same, st2, _ = run(tpath, tpath, prompt, 4, dkw=dkw)                   # its own file on that cache: still drafts that get accepted
    assert ids.tolist() == same.tolist() == greedy_ids(tpath, prompt)[:N_NEW].tolist()
    assert st["rounds_verify"] >= 1 and st2["accepted"] >= 1


@pytest.mark.parametrize("tkw", [{"kv_paged": True, "kv_f16": False}, {"kv_f16": True}], ids=["paged", "fp16"])
def test_target_caches(model_dir, tkw):
    path, spec = model_file(model_dir, "tiny-qwen3", "q80", 64)
    prompt = prompt_of(spec)
    ids, st, _ = run(path, path, prompt, 4, tkw=tkw)
    assert ids.tolist() == greedy_ids(path, prompt, **tkw)[:N_NEW].tolist() and st["rounds_verify"] >= 1


def test_prompt_ingestion_and_continued_calls(model_dir):
    path, spec = model_file(model_dir, "tiny-qwen3", "q80", 64)
    prompt = prompt_of(spec, 40)
    want = greedy_ids(path, prompt).tolist()
    full = prompt.tolist() + want
    n_new = 60
    fn = continuation_of(full)
    # draft_held = 0: the call ingests the prompt into the draft
    ids, st, d_eff = run(path, path, prompt, 4, max_new=n_new)
    sim_ids, sim = dr.simulate(prompt.tolist(), want, n_new, d_eff, fn, seq_limit=S)
    assert ids.tolist() == sim_ids == want[:n_new] and st == sim
    assert st["draft_rows_fed"] >= 39
    # one round per call, the draft_held of one call passed on to the next: the single call's ids and rows
    t, d = load(path), load(path)
    t.prefill(prompt[:-1])
    h, held, fed, rounds = prompt.tolist(), 0, 0, 0
    while len(h) < 40 + n_new:
        got, s1 = t.decode_draft(d, h, 40 + n_new - len(h), max_draft=4, max_rounds=1, draft_held=held)
        assert 1 <= got.size <= 5 and s1["rounds_plain"] + s1["rounds_verify"] == 1
        assert s1 == dr.simulate(h, full[len(h):], 40 + n_new - len(h), d_eff, fn, seq_limit=S, draft_held=held, max_rounds=1)[1]
        h += got.tolist(); held = s1["draft_held"]; fed += s1["draft_rows_fed"]; rounds += 1
    assert h == full[:40 + n_new] and fed == st["draft_rows_fed"] and rounds == st["rounds_plain"] + st["rounds_verify"]
    t.close(); d.close()
    # the draft already holds the prompt: nothing of it is fed again
    t, d = load(path), load(path)
    t.prefill(prompt[:-1]); d.prefill(prompt[:-1])
    ids, s2 = t.decode_draft(d, prompt, n_new, max_draft=4, draft_held=39)
    t.close(); d.close()
    assert ids.tolist() == want[:n_new] and s2["draft_rows_fed"] == st["draft_rows_fed"] - 39
    assert s2 == dr.simulate(prompt.tolist(), want, n_new, d_eff, fn, seq_limit=S, draft_held=39)[1]


def test_clipping(model_dir):
    path, spec = model_file(model_dir, "tiny-qwen3", "q80", 64)
    prompt = prompt_of(spec)
    g = greedy_ids(path, prompt).tolist()
    full = prompt.tolist() + g
    t, d = load(path), load(path)
    t.prefill(prompt[:-1])
    stop = g[40]
    ids, st = t.decode_draft(d, prompt, N_NEW, stop_token=stop)
    assert ids.tolist() == g[:g.index(stop) + 1] and st["emitted"] == ids.size and st["draft_held"] <= N_PROMPT + ids.size - 1
    assert st == dr.simulate(prompt.tolist(), g, N_NEW, 4, continuation_of(full), seq_limit=S, stop_token=stop)[1]
    room = S - (N_PROMPT - 1)
    ids, st = t.decode_draft(d, prompt, room)                               # max_new up to the end of the context (the draft starts over: draft_held = 0)
    assert ids.tolist() == g[:room] and st == dr.simulate(prompt.tolist(), g, room, 4, continuation_of(full), seq_limit=S)[1]
    with pytest.raises(nb.NanoHipError, match="error -1"):
        t.decode_draft(d, prompt, room + 1)
    ids, st = t.decode_draft(d, prompt, 0, draft_held=3)
    assert ids.size == 0 and st["emitted"] == 0 and st["draft_held"] == 3
    t.close(); d.close()


@pytest.mark.parametrize("mode", ["strict", "exact"])
def test_ordered_target_modes_take_plain_steps(model_dir, mode):
    path, spec = model_file(model_dir, "tiny-qwen3", "q80", 64)
    prompt = prompt_of(spec)
    ids, st, _ = run(path, path, prompt, 4, mode=mode)
    assert ids.tolist() == greedy_ids(path, prompt, mode)[:N_NEW].tolist()
    assert st["rounds_verify"] == 0 and st["rounds_plain"] == N_NEW and st["draft_rows_fed"] == 0 and st["drafted"] == 0


def test_refused_calls_queue_nothing(model_dir):
    path, spec = model_file(model_dir, "tiny-nano", "f32", 0)
    other_vocab, _ = model_file(model_dir, "tiny-qwen3", "q80", 64)
    prompt = prompt_of(spec)
    g = greedy_ids(path, prompt)
    t, d, ov = load(path), load(path), load(other_vocab)
    t.prefill(prompt[:-1]); d.prefill(prompt[:-1])
    krow = lambda: [d.read_state("k", spec.kv_dim, slot=0, layer=l, pos=p).copy() for l in range(spec.n_layer) for p in (0, 3)]
    before = krow()

    def refused(draft, hist=prompt, max_new=10, **kw):
        with pytest.raises(nb.NanoHipError, match="error -1"):
            t.decode_draft(draft, hist, max_new, **kw)

    refused(None)                                                           # a null draft
    refused(t)                                                              # draft == target
    refused(ov)                                                             # another vocabulary size
    refused(d, max_draft=16)
    refused(d, draft_held=N_PROMPT)                                         # beyond n_history - 1
    d.set_strict(True); refused(d); d.set_strict(False)
    d.set_exact(True); refused(d); d.set_exact(False)
    r = 2
    lora = np.zeros(spec.n_layer * r * (6 * spec.n_embd + 2 * spec.kv_dim), np.float32)
    nb.check(nb.lib().nano_hip_lora_attach(d.h, r, r, lora, lora.size))
    refused(d)                                                              # LoRA on
    d.lora_enable(False)
    # what nano_hip_decode_lookup refuses
    for hist, max_new in (([], 4), ([1, spec.vocab_size], 4), (prompt, S), (list(range(S)) + [1, 2], 1)):
        refused(d, hist, max_new)
    lib = nb.lib()
    p = nb.NanoHipDraftParams(4, 0xFFFFFFFF, 0, 0)
    out, n = np.zeros(16, np.uint32), C.c_uint32(0)
    h = np.ascontiguousarray(prompt, np.uint32)
    for args in ((t.h, d.h, None, 5, 4, C.byref(p), out.ctypes.data, C.byref(n), None), (t.h, d.h, h.ctypes.data, 5, 4, None, out.ctypes.data, C.byref(n), None),
                 (t.h, d.h, h.ctypes.data, 5, 4, C.byref(p), None, C.byref(n), None), (t.h, d.h, h.ctypes.data, 5, 4, C.byref(p), out.ctypes.data, None, None),
                 (None, d.h, h.ctypes.data, 5, 4, C.byref(p), out.ctypes.data, C.byref(n), None)):
        assert lib.nano_hip_decode_draft(*args) == -1
    # nothing was queued in either model
    after = krow()
    ids = t.decode_greedy([int(prompt[-1])], [N_PROMPT - 1], 8)[:, 0]
    assert ids.tolist() == g[:8].tolist()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before, after))
    # ... and both still serve the call
    t.prefill(prompt[:-1])
    ids, st = t.decode_draft(d, prompt, 20, draft_held=N_PROMPT - 1)
    t.close(); d.close(); ov.close()
    assert ids.tolist() == g[:20].tolist() and st["accepted"] == st["drafted"] >= 1


def test_engine_switch(model_dir):
    """generate_next_token with a draft model returns the ids it returns without one; a caller that overwrites a returned id gets what
    the plain engine returns for the same overwrite; a draft with another vocabulary size is refused"""
    path, spec = model_file(model_dir, "tiny-qwen3", "q80", 64)
    dpath, _ = model_file(model_dir, "tiny-qwen3", "q80", 64, seed=40)
    other_vocab, _ = model_file(model_dir, "tiny-nano", "f32", 0)
    prompt = prompt_of(spec)
    lib = nb.lib()
    lib.nano_set_draft_model.argtypes = [C.c_char_p, C.c_int]
    lib.nano_set_draft_model.restype = C.c_int
    lib.nano_draft_model_open.argtypes = [C.c_void_p]
    lib.nano_draft_model_open.restype = C.c_int

    def run_engine(draft, overwrite_at):
        assert lib.nano_set_draft_model(draft.encode() if draft else None, 4 if draft else 0) == 0
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
            lib.nano_set_draft_model(None, 0)
        return ids[:N_PROMPT + N_NEW].tolist()

    plain = run_engine(None, ())
    assert plain[N_PROMPT:] == greedy_ids(path, prompt)[:N_NEW].tolist()
    assert run_engine(path, ()) == plain                                    # every draft accepted: the queue serves four calls of five
    assert run_engine(dpath, ()) == plain                                   # drafts that fail
    over = (3, 50, 51, 70)
    assert run_engine(path, over) == run_engine(None, over)
    assert lib.nano_set_draft_model(path.encode(), 16) == -1 and lib.nano_set_draft_model(path.encode(), -1) == -1
    assert lib.nano_set_draft_model(other_vocab.encode(), 4) == 0
    try:
        e = nb.Engine(path, max_seq_len=S)
        assert lib.nano_draft_model_open(e.ctx) == -1
        e.close()
    finally:
        lib.nano_set_draft_model(None, 0)
