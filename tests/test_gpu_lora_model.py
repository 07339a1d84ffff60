"""GPU tests of whole models with a LoRA module switched on (lora.hip's two launches per layer, the addend in Wo's epilogue, and the
gates in front of them), for FP32, Q80 and Q4K weights.

  * Q4K against the compiled reference's teacher-forced logits (tests/golden/lora_*_q4k.npz, tools/make_golden.py), the bar of
    test_gpu_e2e.py::test_lora_logits_vs_reference_golden.
  * Bit-for-bit self-consistency, the project's invariant, with the module on: a batch row is the sequence alone (v_bstride, pos[b],
    the addend's stride and its shift by slice); a prefill of 70 tokens -- a 64-token chunk and a tail of 6 -- is token-by-token
    feeding, K / V rows and the logits of the steps behind it at positions >= 64, where the module forces one attention split; a
    prefill into slot 2 of three gives slot 0's rows of a fresh model and leaves the other slots alone; decode_greedy and the
    lookup-draft decode give the ids of the forward + arg-max loop.
  * Gating: with a module on, the FP16, FP8 and paged caches refuse forward, prefill, the draft and the lookup entries with
    NANO_HIP_EINVAL, ragged steps are refused on every cache, nothing was queued (the model then behaves bit for bit like one that never
    had a module), and lora_enable(False) restores the base model's bits.  FP16 x prefill used to pass the gate: the v branch then
    read-modify-wrote FP32 at a float offset into a cache of halfs."""
import os

import numpy as np
import pytest

import test_gpu_e2e as e2e
from nano_amd import binding as nb
from nano_amd import modelfile as mf
from fused_ref import bits

pytestmark = pytest.mark.gpu

S = 256
CASES = [("tiny-nano", "f32", 0), ("tiny-nano", "q80", 32), ("tiny-nano", "q4k", 0), ("tiny-nano-odd", "q4k", 0)]
RANK, ALPHA = 5, 16                     # a rank that is neither 4 nor 8, an inexact scale
T = 70                                  # a 64-token chunk and a tail of 6

_files = {}


def files(model_dir, preset, quant, gs):
    """(model path, spec, module path): block_size 256, written once per session"""
    key = (preset, quant, gs)
    if key not in _files:
        spec = mf.preset(preset, quant, group_size=gs, block_size=S)
        path = os.path.join(model_dir, f"loramodel-{preset}-{quant}-{gs}.bin")
        lpath = os.path.join(model_dir, f"loramodel-{preset}-{quant}-{gs}.lora")
        mf.write_model(path, spec, seed=39)
        mf.write_lora(lpath, spec, rank=RANK, alpha=ALPHA, seed=13)
        _files[key] = (path, spec, lpath)
    return _files[key]


def load(path, lpath=None, **kw):
    m = nb.load_model_file(path, max_seq_len=S, **kw)
    if lpath:
        m.lora_attach_file(lpath)                   # (attaching switches the module on)
    return m


def kv_rows(m, spec, slot, n_pos):
    return np.stack([m.read_state(w, spec.kv_dim, slot=slot, layer=l, pos=p) for l in range(spec.n_layer) for p in range(n_pos) for w in ("k", "v")])


def same_bits(a, b, what):
    bad = np.argwhere(bits(a) != bits(b))
    assert not bad.size, (what, "first differences at", bad[:6].tolist(), float(np.abs(np.asarray(a, np.float64) - b).max()))


@pytest.mark.parametrize("preset", ["tiny-nano", "tiny-nano-odd"])
def test_q4k_lora_logits_vs_reference_golden(model_dir, preset):
    e2e.test_lora_logits_vs_reference_golden(model_dir, preset, "q4k", 0)


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_batched_decode_rows_equal_the_sequences_alone(model_dir, preset, quant, gs):
    """three sequences at distinct positions (the first at 0: no row behind it): logits and the K / V rows the step wrote"""
    path, spec, lpath = files(model_dir, preset, quant, gs)
    pos = (0, 11, 7)
    prompts = [mf.prompt_ids(300 + b, pos[b] + 1, spec.vocab_size) for b in range(3)]
    m = load(path, lpath, max_batch=3)
    for b in range(1, 3):
        m.prefill(prompts[b][:-1], 0, slot=b)
    lg = m.forward([int(p[-1]) for p in prompts], pos)[0].copy()
    rows = [np.stack([m.read_state(w, spec.kv_dim, slot=b, layer=l, pos=pos[b]) for l in range(spec.n_layer) for w in ("k", "v")]) for b in range(3)]
    m.close()
    off = load(path, max_batch=1)
    for b in range(3):
        one = load(path, lpath, max_batch=1)
        if pos[b]:
            one.prefill(prompts[b][:-1], 0)
        want = one.forward([int(prompts[b][-1])], [pos[b]])[0][0]
        same_bits(lg[b], want, (preset, quant, "logits of sequence", b))
        same_bits(rows[b], np.stack([one.read_state(w, spec.kv_dim, layer=l, pos=pos[b]) for l in range(spec.n_layer) for w in ("k", "v")]), (preset, quant, "K / V rows of sequence", b))
        one.close()
        if pos[b]:
            off.prefill(prompts[b][:-1], 0)
        assert e2e.rel_err(off.forward([int(prompts[b][-1])], [pos[b]])[0][0], want) > 1e-3, "the module changed nothing"
    off.close()


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_prefill_of_70_tokens_equals_token_by_token(model_dir, preset, quant, gs):
    path, spec, lpath = files(model_dir, preset, quant, gs)
    ids = mf.prompt_ids(611, T + 4, spec.vocab_size)
    a, b = load(path, lpath), load(path, lpath)
    for p in range(T):
        a.forward([int(ids[p])], [p], want_logits=False)
    b.prefill(ids[:T], 0)
    same_bits(kv_rows(b, spec, 0, T), kv_rows(a, spec, 0, T), (preset, quant, "K / V rows"))
    for p in range(T, T + 4):                                   # positions >= 64: the module forces one split
        same_bits(b.forward([int(ids[p])], [p])[0][0], a.forward([int(ids[p])], [p])[0][0], (preset, quant, "step at position", p))
    a.close(); b.close()


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_prefill_into_slot_2_leaves_the_other_slots(model_dir, preset, quant, gs):
    path, spec, lpath = files(model_dir, preset, quant, gs)
    ids = mf.prompt_ids(612, T, spec.vocab_size)
    m = load(path, lpath, max_batch=3)
    m.prefill(ids[:9], 0, slot=0); m.prefill(ids[20:27], 0, slot=1)
    before = [kv_rows(m, spec, s, T + 8) for s in (0, 1)]
    m.prefill(ids, 0, slot=2)
    for s in (0, 1):
        same_bits(kv_rows(m, spec, s, T + 8), before[s], (preset, quant, "slot", s, "changed"))
    fresh = load(path, lpath, max_batch=1)
    fresh.prefill(ids, 0)
    same_bits(kv_rows(m, spec, 2, T + 8), kv_rows(fresh, spec, 0, T + 8), (preset, quant, "slot 2 against slot 0 of a fresh model"))
    m.close(); fresh.close()


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_greedy_and_lookup_ids_equal_the_forward_loop(model_dir, preset, quant, gs):
    path, spec, lpath = files(model_dir, preset, quant, gs)
    prompt = mf.prompt_ids(77, 5, spec.vocab_size)
    n_new = 80                                                  # crosses position 64
    m = load(path, lpath)
    m.prefill(prompt[:-1], 0)
    tok, want = int(prompt[-1]), []
    for p in range(len(prompt) - 1, len(prompt) - 1 + n_new):
        lg, am = m.forward([tok], [p], want_argmax=True)
        assert int(am[0]) == int(np.argmax(lg[0]))
        tok = int(am[0]); want.append(tok)
    m.close()
    m = load(path, lpath)
    m.prefill(prompt[:-1], 0)
    got = m.decode_greedy([int(prompt[-1])], [len(prompt) - 1], n_new)[:, 0].tolist()
    m.close()
    assert got == want, (preset, quant, "decode_greedy", int(np.argmax(np.asarray(got) != np.asarray(want))))
    m = load(path, lpath)
    m.prefill(prompt[:-1], 0)
    ids, st = m.decode_lookup(prompt, n_new, max_draft=7)
    m.close()
    print(f"{preset}/{quant} with a module: lookup decode {st}")
    assert ids.tolist() == want, (preset, quant, "decode_lookup", st)
    assert st["steps_verify"] > 0 and st["drafted"] > 0          # verify chunks ran with the module on


CACHES = {"fp16": dict(kv_f16=True), "fp8": dict(kv_fp8=True, kv_f16=False, kv_paged=False), "paged": dict(kv_paged=True, kv_f16=False),
          "fp32": dict(kv_f16=False)}
ENTRIES = {"forward": lambda m, ids: m.forward([int(ids[0])], [0]),
           "greedy": lambda m, ids: m.decode_greedy([int(ids[0])], [0], 2),
           "prefill": lambda m, ids: m.prefill(ids[:5], 0),
           "prefill_score": lambda m, ids: m.prefill_score(ids[:5], ids[1:6]),
           "draft": lambda m, ids: m.verify_draft(ids[:4], 0),
           "lookup": lambda m, ids: m.decode_lookup(ids[:3], 4),
           "ragged": lambda m, ids: m.step_rows([(0, 0, 3)], ids[:3])}


@pytest.mark.parametrize("cache", list(CACHES))
def test_gating_with_a_module_on(model_dir, cache):
    """every refused combination: NANO_HIP_EINVAL, and nothing was queued -- afterwards, the module switched off, the model steps bit for
    bit like one of the same cache that never had a module.  (FP32, the contiguous cache, refuses the ragged step alone.)"""
    path, spec, lpath = files(model_dir, "tiny-nano", "f32", 0)
    ids = mf.prompt_ids(5, 12, spec.vocab_size)
    m = load(path, lpath, max_batch=1, **CACHES[cache])
    for name, call in ENTRIES.items():
        if cache == "fp32" and name != "ragged":
            continue
        with pytest.raises(nb.NanoHipError, match="nano_hip error -1:"):
            call(m, ids)
        assert "LoRA" in nb.last_error(), (cache, name, nb.last_error())
    m.lora_enable(False)
    never = load(path, None, max_batch=1, **CACHES[cache])
    for p in range(6):
        same_bits(m.forward([int(ids[p])], [p])[0][0], never.forward([int(ids[p])], [p])[0][0], (cache, "position", p))
    m.close(); never.close()


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_switching_the_module_off_restores_the_base_model(model_dir, preset, quant, gs):
    """after steps and a prefill WITH the module (rows of the cache carry its deltas), lora_enable(False): the same feeding from position
    0 gives the bits of a model that never had a module; switched on again, the module's own bits"""
    path, spec, lpath = files(model_dir, preset, quant, gs)
    ids = mf.prompt_ids(9, 12, spec.vocab_size)
    m, never = load(path, lpath), load(path)
    with_module = [m.forward([int(ids[p])], [p])[0][0].copy() for p in range(6)]
    m.prefill(ids, 0)
    m.lora_enable(False)
    for p in range(6):
        base = never.forward([int(ids[p])], [p])[0][0]
        same_bits(m.forward([int(ids[p])], [p])[0][0], base, (preset, quant, "off", p))
        assert e2e.rel_err(with_module[p], base) > 1e-3
    m.lora_enable(True)
    for p in range(6):
        same_bits(m.forward([int(ids[p])], [p])[0][0], with_module[p], (preset, quant, "on again", p))
    m.close(); never.close()


def test_attach_refuses_a_rank_the_launches_cannot_run(model_dir):
    """n_embd 128: 128 + 3 * 5408 + 32 floats are the 64 KiB of LDS a launch may ask for, one rank more is refused at attach time (not at
    the first step), and the model goes on as it was"""
    import ctypes as C
    path, spec, lpath = files(model_dir, "tiny-nano", "f32", 0)
    m, never = load(path), load(path)
    L, E, KD = spec.n_layer, spec.n_embd, spec.kv_dim
    for rank, ok in ((5409, False), (0, False), (5408, True)):
        n = L * rank * (4 * E + 2 * E + 2 * KD)
        p = np.zeros(max(n, 1), np.float32)
        rc = nb.lib().nano_hip_lora_attach(m.h, rank, 16, p, n)
        assert (rc == 0) == ok, (rank, rc, nb.last_error())
        if not ok:
            assert rc == -1
            same_bits(m.forward([3], [0])[0][0], never.forward([3], [0])[0][0], ("after the refusal of rank", rank))
    same_bits(m.forward([3], [0])[0][0], never.forward([3], [0])[0][0], "a module of zeros at the largest rank")
    m.close(); never.close()
