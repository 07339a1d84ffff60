"""GPU tests of lookup drafts for several sequences (nano_hip_decode_lookup_rows, nano_decode_batch_lookup in the engine).

What is pinned is independence: each sequence's ids are nano_hip_decode_greedy's for that sequence alone on a fresh one-slot handle,
its stats are what tests/lookup_ref.py simulate() gives on those ids with the max_draft the call runs (D_eff), and the call's rounds
are tests/lookup_rows_ref.py simulate_rows()' -- whatever shares the passes."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lookup_ref as lr
import lookup_rows_ref as rr
from conftest import ROOT, synth_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf

pytestmark = pytest.mark.gpu

S = 128
PERIODIC_SEED = 39                   # model seed of the periodic-by-construction cases (as tests/test_gpu_lookup_decode.py)
PROMPTS = [(77, 5), (78, 9), (79, 3), (80, 7)]                              # (prompt seed, prompt length) of sequence 0, 1, 2, 3
MAX_NEW = [100, 37, 5, 64]                                                  # sequence 0 crosses position 64 while the others are before it


def model_file(model_dir, preset, quant, gs, seed=39, zero_mixers=False):
    """A synthetic model whose RoPE table covers S positions; zero_mixers: Wo and W2 zeroed (Q80: their scales too), so that the residual
    stream stays the fed id's embedding and the logits depend on the last id only."""
    if not zero_mixers and mf.preset(preset, quant, group_size=gs).block_size >= S:
        return synth_model(model_dir, preset, quant, gs, seed)
    spec = mf.preset(preset, quant, group_size=gs, block_size=max(S, mf.preset(preset, quant, group_size=gs).block_size))
    path = os.path.join(model_dir, f"lookup-rows-{preset}-{quant}-{gs}-{seed}-{int(zero_mixers)}.bin")
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
    """the ids nano_hip_decode_greedy gives after the prompt on a fresh one-slot handle, up to the end of the context (computed once per
    case, never modified)"""
    prompt = np.ascontiguousarray(prompt, np.uint32)
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


def check_call(m, path, prompts, slots, max_new, D, d_eff, got, what, mode=None, stop=None, **kw):
    """got = (ids, stats, rounds) of one decode_lookup_rows call: every sequence against its own reference, the rounds against simulate_rows"""
    ids, stats, rounds = got
    stop_id = lr.NO_STOP if stop is None else stop
    wants = [greedy_ids(path, p, mode, **kw).tolist() for p in prompts]
    for i, p in enumerate(prompts):
        sim_ids, sim = lr.simulate(list(p), wants[i], max_new[i], d_eff, 1, 3, stop_token=stop_id, seq_limit=S)
        ref = wants[i][:max_new[i]]
        if stop is not None and stop in ref:
            ref = ref[:ref.index(stop) + 1]
        print(f"{what} D={D} (runs {d_eff}) sequence {i} in slot {slots[i]}: {stats[i]}")
        assert sim_ids == ref                                               # (the lossless property, on this sequence)
        assert ids[i].tolist() == ref, f"{what}: sequence {i}: ids differ from decode_greedy's"
        assert stats[i] == sim, (what, i, stats[i], sim)
    want_rounds = rr.simulate_rows([list(p) for p in prompts], wants, max_new, d_eff, 1, 3, stop_token=stop_id, seq_limit=S, max_seq_len=S)[2]
    assert rounds == want_rounds, (what, rounds, want_rounds)
    return wants


def check_rows_left_behind(m, prompts, slots, ids, wants):
    """one decode row per slot through nano_hip_step_rows returns the reference's next id: the cache rows the call left are valid"""
    segs, toks, nxt = [], [], []
    for i, p in enumerate(prompts):
        n = len(p) + ids[i].size
        if n - 1 >= S or ids[i].size >= len(wants[i]):
            continue
        segs.append((slots[i], n - 1, 1)); toks.append(int(ids[i][-1]) if ids[i].size else int(p[-1])); nxt.append(wants[i][ids[i].size])
    assert m.step_rows(segs, toks, want_argmax=True).tolist() == nxt


def run(model_dir, preset, quant, gs, B, D, slots=None, max_batch=None, zero=False, mode=None, stop_from=None, **kw):
    path, spec = model_file(model_dir, preset, quant, gs, seed=PERIODIC_SEED if zero else 39, zero_mixers=zero)
    prompts = [mf.prompt_ids(seed, n, spec.vocab_size) for seed, n in PROMPTS[:B]]
    slots = list(range(B)) if slots is None else slots
    max_new = MAX_NEW[:B]
    stop = None
    if stop_from is not None:                                               # a stop token from the middle of one sequence's greedy ids
        stop = int(greedy_ids(path, prompts[stop_from], mode, **kw)[max_new[stop_from] // 2])
    m = nb.load_model_file(path, max_seq_len=S, max_batch=max_batch or B, **kw)
    prepare(m, mode)
    for p, s in zip(prompts, slots):
        m.prefill(p[:-1], slot=s)
    d_eff = 0 if mode else min(D, m.prefill_chunk_tokens() // B - 1)
    got = m.decode_lookup_rows(prompts, slots, max_new, max_draft=D, stop_token=stop)
    what = f"{preset}/{quant}{' zeroed' if zero else ''}{' ' + mode if mode else ''} {kw or ''} B={B}"
    wants = check_call(m, path, prompts, slots, max_new, D, d_eff, got, what, mode=mode, stop=stop, **kw)
    if not mode:
        check_rows_left_behind(m, prompts, slots, got[0], wants)
    m.close()
    return got, d_eff


FREE = [("tiny-qwen3", "q80", 64), ("tiny-nano", "f32", 0), ("tiny-nano-odd", "q4k", 0)]
PERIODIC = [("tiny-nano-ucls", "f32", 0), ("tiny-qwen3-ucls", "q80", 64)]


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("preset,quant,gs", FREE)
def test_free_running_models(model_dir, preset, quant, gs, B):
    run(model_dir, preset, quant, gs, B, 3)


@pytest.mark.parametrize("D", [3, 15])
@pytest.mark.parametrize("preset,quant,gs", PERIODIC)
def test_periodic_models_accept_drafts(model_dir, preset, quant, gs, D):
    """Wo and W2 zeroed: every sequence falls into a loop and drafts are accepted"""
    (ids, stats, rounds), d_eff = run(model_dir, preset, quant, gs, 4, D, zero=True)
    assert sum(s["accepted"] for s in stats) >= 10 and rounds < max(MAX_NEW)


def test_max_draft_is_clipped_by_the_rows_of_one_pass(model_dir):
    """a model whose passes hold 8 rows: two sequences verify at most 3 drafted ids each, whatever max_draft asks for"""
    (_ids, stats, _rounds), d_eff = run(model_dir, "tiny-nano-odd", "q4k", 0, 2, 15)
    assert d_eff == 3 and all(s["drafted"] == 3 * s["steps_verify"] for s in stats)


def test_slots_out_of_order(model_dir):
    run(model_dir, "tiny-qwen3-ucls", "q80", 64, 3, 7, slots=[2, 0, 3], max_batch=4, zero=True)


def test_stop_token_from_the_middle_of_one_sequence(model_dir):
    (ids, _stats, _rounds), _ = run(model_dir, "tiny-qwen3-ucls", "q80", 64, 4, 7, zero=True, stop_from=1)
    assert ids[1].size <= MAX_NEW[1] // 2 + 1


@pytest.mark.parametrize("kw", [{"kv_f16": True}, {"kv_fp8": True}, {"kv_paged": True, "kv_f16": False}], ids=["fp16", "fp8", "paged"])
def test_other_caches(model_dir, kw):
    run(model_dir, "tiny-qwen3-ucls", "q80", 64, 3, 7, zero=True, **kw)


@pytest.mark.parametrize("mode", ["strict", "exact"])
def test_ordered_modes_take_reference_order_steps(model_dir, mode):
    (_ids, stats, rounds), d_eff = run(model_dir, "tiny-qwen3", "q80", 64, 3, 7, mode=mode)
    assert d_eff == 0 and all(s["steps_verify"] == 0 for s in stats) and rounds == max(MAX_NEW[:3])


def test_paged_cache_with_a_forked_prefix_copies_on_write(model_dir):
    """64 shared positions in all three slots, every sequence goes on from position 40 with a last id of its own: its first row is
    written into the page it shares"""
    path, spec = model_file(model_dir, "tiny-qwen3-ucls", "q80", 64, seed=PERIODIC_SEED, zero_mixers=True)
    kw = {"kv_paged": True, "kv_f16": False}
    prefix = mf.prompt_ids(81, 70, spec.vocab_size)
    prompts = [np.concatenate([prefix[:40], np.array([x], np.uint32)]) for x in (3, 11, 19)]
    m = nb.load_model_file(path, max_seq_len=S, max_batch=3, **kw)
    m.prefill(prefix)
    m.kv_fork(0, 64, [1, 2])
    shared, copies = m.kv_sharing()
    assert shared >= 1
    got = m.decode_lookup_rows(prompts, [0, 1, 2], [30, 30, 30], max_draft=7)
    d_eff = min(7, m.prefill_chunk_tokens() // 3 - 1)
    wants = check_call(m, path, prompts, [0, 1, 2], [30, 30, 30], 7, d_eff, got, "forked prefix", **kw)
    assert m.kv_sharing()[1] > copies
    check_rows_left_behind(m, prompts, [0, 1, 2], got[0], wants)
    m.close()


def test_continued_histories_upload_only_new_ids_and_decode_on(model_dir):
    path, spec = model_file(model_dir, "tiny-qwen3-ucls", "q80", 64, seed=PERIODIC_SEED, zero_mixers=True)
    prompts = [mf.prompt_ids(seed, n, spec.vocab_size) for seed, n in PROMPTS[:3]]
    wants = [greedy_ids(path, p).tolist() for p in prompts]
    m = nb.load_model_file(path, max_seq_len=S, max_batch=3)
    for s, p in enumerate(prompts):
        m.prefill(p[:-1], slot=s)
    first, _st, _r = m.decode_lookup_rows(prompts, [0, 1, 2], [20, 9, 31], max_draft=7)
    hs = [np.concatenate([p, i]) for p, i in zip(prompts, first)]
    assert [i.tolist() for i in first] == [w[:k] for w, k in zip(wants, (20, 9, 31))]
    # the histories extend the first call's; rounds of one pass each, call after call
    second, st, rounds = m.decode_lookup_rows(hs, [0, 1, 2], [40, 40, 0], max_draft=7)
    assert [i.tolist() for i in second] == [wants[0][20:60], wants[1][9:49], []] and st[2]["emitted"] == 0
    hs = [np.concatenate([h, i]) for h, i in zip(hs, second)]
    third, st, rounds = m.decode_lookup_rows(hs, [0, 1, 2], [10, 10, 10], max_draft=7, max_steps=1)
    assert rounds == 1 and all(1 <= i.size <= 8 for i in third)
    assert [i.tolist() for i in third] == [wants[0][60:60 + third[0].size], wants[1][49:49 + third[1].size], wants[2][31:31 + third[2].size]]
    check_rows_left_behind(m, hs, [0, 1, 2], third, [w[len(h) - len(p):] for w, h, p in zip(wants, hs, prompts)])
    ids, st, rounds = m.decode_lookup_rows(hs, [0, 1, 2], [0, 0, 0])
    assert rounds == 0 and all(i.size == 0 for i in ids)
    assert m.decode_lookup_rows([], [], []) == ([], [], 0)
    m.close()


def test_refused_calls_queue_nothing(model_dir):
    path, spec = model_file(model_dir, "tiny-nano", "f32", 0)
    prompts = [mf.prompt_ids(seed, n, spec.vocab_size) for seed, n in PROMPTS[:2]]
    want = greedy_ids(path, prompts[0])
    m = nb.load_model_file(path, max_seq_len=S, max_batch=16)
    for s, p in enumerate(prompts):
        m.prefill(p[:-1], slot=s)
    refuse = lambda *a, **k: pytest.raises(nb.NanoHipError, match="error -1")
    with refuse():
        m.decode_lookup_rows(prompts, [1, 1], [4, 4])                       # two sequences in one slot
    with refuse():
        m.decode_lookup_rows(prompts, [0, 16], [4, 4])                      # a slot out of range
    qpath, qspec = model_file(model_dir, "tiny-nano-odd", "q4k", 0)         # (a model whose passes hold 8 rows)
    q = nb.load_model_file(qpath, max_seq_len=S, max_batch=16)
    chunk = q.prefill_chunk_tokens()
    assert chunk < 16
    one = mf.prompt_ids(77, 1, qspec.vocab_size)
    assert len(q.decode_lookup_rows([one] * chunk, list(range(chunk)), [1] * chunk)[0]) == chunk
    with refuse():
        q.decode_lookup_rows([one] * (chunk + 1), list(range(chunk + 1)), [1] * (chunk + 1))    # more sequences than one pass has rows
    q.close()
    with refuse():
        m.decode_lookup_rows(prompts, [0, 1], [4, S])                       # positions beyond max_seq_len
    with refuse():
        m.decode_lookup_rows([prompts[0], []], [0, 1], [4, 4])              # an empty history
    with refuse():
        m.decode_lookup_rows([prompts[0], [1, spec.vocab_size]], [0, 1], [4, 4])
    with refuse():
        m.decode_lookup_rows(prompts, [0, 1], [4, 4], max_draft=16)
    with refuse():
        m.decode_lookup_rows(prompts, [0, 1], [S * 16 + 1, 4])                  # (also beyond the trace capacity)
    seqs = (nb.NanoHipLookupSeq * 1)(nb.NanoHipLookupSeq(0, len(prompts[0]), 4, 1))                    # reserved != 0
    h, out, n = np.ascontiguousarray(prompts[0], np.uint32), np.zeros(4, np.uint32), np.zeros(1, np.uint32)
    hp, op = (C.c_void_p * 1)(h.ctypes.data), (C.c_void_p * 1)(out.ctypes.data)
    p = nb.NanoHipLookupParams(7, 3, 1, 0xFFFFFFFF, 0)
    lib = nb.lib()
    assert lib.nano_hip_decode_lookup_rows(m.h, seqs, 1, hp, C.byref(p), op, n.ctypes.data, None, None) == -1
    seqs[0].reserved = 0
    for args in ((m.h, None, 1, hp, C.byref(p), op, n.ctypes.data), (m.h, seqs, 1, None, C.byref(p), op, n.ctypes.data), (m.h, seqs, 1, hp, None, op, n.ctypes.data),
                 (m.h, seqs, 1, hp, C.byref(p), None, n.ctypes.data), (m.h, seqs, 1, hp, C.byref(p), op, None)):
        assert lib.nano_hip_decode_lookup_rows(*args, None, None) == -1
    lpath = os.path.join(model_dir, "lookup-rows-tiny-nano.lora")
    mf.write_lora(lpath, spec, rank=4, alpha=8, seed=3)
    m.lora_attach_file(lpath)
    m.lora_enable(True)
    with pytest.raises(nb.NanoHipError, match="LoRA"):
        m.decode_lookup_rows(prompts, [0, 1], [4, 4])
    m.lora_enable(False)
    # nothing was queued: slot 0 still continues its prompt
    ids = m.decode_greedy([int(prompts[0][-1])], [len(prompts[0]) - 1], 8)[:, 0]
    m.close()
    assert ids.tolist() == want[:8].tolist()


def test_engine_call_in_a_child_process(model_dir):
    """nano_decode_batch_lookup on two sequences: the ids of the backend call (tests/lookup_rows_engine_child.py)"""
    path, spec = model_file(model_dir, "tiny-qwen3-ucls", "q80", 64, seed=PERIODIC_SEED, zero_mixers=True)
    cases = [(77, 5, 40), (78, 9, 23)]
    prompts = [mf.prompt_ids(seed, n, spec.vocab_size) for seed, n, _ in cases]
    m = nb.load_model_file(path, max_seq_len=S, max_batch=2)
    for s, p in enumerate(prompts):
        m.prefill(p[:-1], slot=s)
    ids, _st, _r = m.decode_lookup_rows(prompts, [0, 1], [mn for _, _, mn in cases], max_draft=7)
    m.close()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lookup_rows_engine_child.py"), path, str(S), "7"] + [f"{a}:{b}:{c}" for a, b, c in cases],
                       capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ids"] == [i.tolist() for i in ids]
    assert out["ids"] == [greedy_ids(path, p)[:mn].tolist() for p, (_, _, mn) in zip(prompts, cases)]
