"""GPU tests of the shared prompt prefix (nano_hip_kv_fork / nano_hip_kv_sharing / nano_prefill_shared, include/nano_mi355x.h,
include/nano_infer_abi.h).  The reference keeps one cache per context (infer/infer.c:46-51) and ingests every prompt token by token
(:1258-1260); here a prefix is ingested once and forked into other slots -- copied on the contiguous cache, shared page by page with
copy-on-write on the paged one.  The bar is exact: a forked slot must be BIT FOR BIT a slot that ingested the prefix itself ("equal"
below always means equal uint32 views of the floats), and page accounting must add up to the page."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import e2e_golden
from conftest import synth_model as golden_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf
from fused_ref import bits

pytestmark = pytest.mark.gpu

S, B, T = 256, 4, 70                 # context, slots, continuation steps (70 > 64: every continuation enters a new 64-position block)


_models = {}


def synth_model(model_dir, preset, quant, gs, block=256):
    """the tiny presets with a RoPE table (block_size) long enough to cross several 64-position pages"""
    key = (preset, quant, gs, block)
    if key not in _models:
        spec = mf.preset(preset, quant, group_size=gs, block_size=block)
        path = os.path.join(model_dir, f"fork-{preset}-{quant}-{gs}-{block}.bin")
        mf.write_model(path, spec, seed=39)
        _models[key] = (path, spec)
    return _models[key]


def load(path, paged, max_batch=B, max_seq_len=S, **kw):
    return nb.load_model_file(path, max_seq_len=max_seq_len, max_batch=max_batch, kv_paged=paged, **kw)


def prefix_ids(spec, n):
    return mf.prompt_ids(101, n, spec.vocab_size)


def continuations(spec, n=T, slots=B):
    return [mf.prompt_ids(200 + b, n, spec.vocab_size) for b in range(slots)]


def own(m, prefix, slots=range(B)):
    """model A: every slot ingests the prefix itself"""
    for s in slots:
        m.prefill(prefix, 0, s)
    return m


def forked(m, prefix, slots=B):
    """model B: slot 0 ingests, the others are forked from it"""
    m.prefill(prefix, 0, 0)
    m.kv_fork(0, len(prefix), list(range(1, slots)))
    return m


def run_equal(a, b, conts, pos0, steps=None, slots=None, what=""):
    """the same batched steps on both models: logits and arg-max of every slot equal at every step"""
    slots = len(conts) if slots is None else slots
    for t in range(len(conts[0]) if steps is None else steps):
        toks = [int(conts[s][t]) for s in range(slots)]
        la, aa = a.forward(toks, [pos0 + t] * slots, want_argmax=True)
        lb, ab = b.forward(toks, [pos0 + t] * slots, want_argmax=True)
        for s in range(slots):
            assert np.array_equal(bits(la[s]), bits(lb[s])), (what, "step", t, "slot", s)
        assert np.array_equal(aa, ab), (what, t)


def rows_equal(a, b, spec, positions, slots=range(B)):
    for s in slots:
        for layer in (0, spec.n_layer - 1):
            for pos in positions:
                for which in ("k", "v"):
                    ra, rb = a.read_state(which, spec.kv_dim, s, layer, pos), b.read_state(which, spec.kv_dim, s, layer, pos)
                    assert np.array_equal(bits(ra), bits(rb)), (which, s, layer, pos)


def fork_equals_own(path, spec, paged, n_pos, **kw):
    prefix, conts = prefix_ids(spec, n_pos), continuations(spec)
    a, b = own(load(path, paged, **kw), prefix), forked(load(path, paged, **kw), prefix)
    if paged:
        partial = n_pos % 64 != 0
        assert b.kv_pages()[0] == (n_pos + 63) // 64 + 3 * partial
        assert b.kv_sharing() == (n_pos // 64, 0)
        assert a.kv_pages()[0] == B * ((n_pos + 63) // 64) and a.kv_sharing() == (0, 0)
    used0 = b.kv_pages()[0] if paged else 0
    run_equal(a, b, conts, n_pos, what=(paged, n_pos))
    inside = sorted({0, n_pos // 2, max(n_pos - 2, 0)})
    rows_equal(a, b, spec, inside + [n_pos - 1, n_pos, n_pos + T // 2, n_pos + T - 1])
    if paged:
        new_blocks = (n_pos + T + 63) // 64 - (n_pos + 63) // 64
        assert b.kv_pages()[0] == used0 + B * new_blocks
        assert b.kv_sharing() == (n_pos // 64, 0)              # the continuations wrote no shared page: nothing was copied
    a.close(); b.close()


CASES = [("tiny-qwen3", "q80", 64), ("tiny-nano", "f32", 0), ("tiny-qwen3", "q4k", 0)]


# ---- 1. fork = own ingestion ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pos", [64, 128, 100, 1])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_fork_equals_own_ingestion(model_dir, preset, quant, gs, paged, n_pos):
    path, spec = synth_model(model_dir, preset, quant, gs)
    fork_equals_own(path, spec, paged, n_pos)


# ---- 2. the reference's bits through a fork ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "exact"])
@pytest.mark.parametrize("preset,quant,gs", [("tiny-qwen3", "q80", 64), ("tiny-nano-odd", "q4k", 0), ("tiny-nano", "f32", 0)])
def test_reference_bits_through_a_fork(model_dir, preset, quant, gs, mode):
    """prefill prompt[:-1] into slot 0, fork into slot 1, teacher-force the golden ids as batches of two: BOTH rows carry the compiled
    reference's logits and greedy ids at every decode step.  Exact mode: twice (the second pass is pure graph replays), forking again."""
    g = np.load(e2e_golden(preset, quant, gs))
    path, spec = golden_model(model_dir, preset, quant, gs)
    m = nb.load_model_file(path, max_seq_len=int(g["max_seq_len"]), max_batch=2)
    (m.set_strict if mode == "strict" else m.set_exact)(True)
    ids, gl, prompt = g["ids"], g["logits"], g["prompt"]
    n_prompt = len(prompt)
    for rnd in range(2 if mode == "exact" else 1):
        graphs = m.exact_state()["graphs"]
        m.prefill(prompt[:-1], 0, 0)
        m.kv_fork(0, n_prompt - 1, [1])
        for pos in range(n_prompt - 1, len(ids) - 1):
            lg, am = m.forward([int(ids[pos])] * 2, [pos] * 2, want_argmax=True)
            for row in range(2):
                assert np.array_equal(bits(lg[row]), bits(gl[pos - (n_prompt - 1)])), (preset, quant, mode, "pos", pos, "row", row)
                assert int(am[row]) == int(ids[pos + 1])
        if rnd == 1:
            assert m.exact_state()["graphs"] == graphs         # replays only
    m.close()


# ---- 3. copy-on-write ----------------------------------------------------------------------------------------------------------------
def cow_setup(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    prefix = prefix_ids(spec, 128)
    return path, spec, prefix, own(load(path, True), prefix), forked(load(path, True), prefix)


@pytest.mark.parametrize("restarter", [2, 0], ids=["a-destination-restarts", "the-source-restarts"])
def test_copy_on_write_when_a_slot_restarts(model_dir, restarter):
    """after a fork at 128 positions one owner restarts at position 0 with 70 other tokens (blocks 0 and 1 are shared: two copies,
    two more pages in use); it equals a fresh model fed those tokens, and the other owners, continued afterwards, still equal model A.
    The source restarts step by step (slot 0 of one-sequence steps); a destination through nano_hip_prefill, the entry that addresses
    a slot of its own (its rows are those of token-by-token feeding, bit for bit)."""
    path, spec, prefix, a, b = cow_setup(model_dir)
    other = mf.prompt_ids(977, T + 8, spec.vocab_size)
    fresh = load(path, True, max_batch=1)
    assert (b.kv_pages()[0], b.kv_sharing()) == (2, (2, 0))
    if restarter == 0:
        for t in range(T):
            lf, _ = fresh.forward([int(other[t])], [t])
            lb, _ = b.forward([int(other[t])], [t])
            assert np.array_equal(bits(lf[0]), bits(lb[0])), t
    else:
        fresh.prefill(other[:T], 0, 0)
        b.prefill(other[:T], 0, restarter)
    assert b.kv_sharing() == (2, 2) and b.kv_pages()[0] == 2 + 2           # the other three still share both pages
    for layer in range(spec.n_layer):
        for pos in (0, 63, 64, T - 1):
            for which in ("k", "v"):
                assert np.array_equal(bits(fresh.read_state(which, spec.kv_dim, 0, layer, pos)), bits(b.read_state(which, spec.kv_dim, restarter, layer, pos)))
    # everybody goes on: the restarted slot from position 70 like the fresh model, the others from 128 like model A
    keep = [s for s in range(B) if s != restarter]
    conts = continuations(spec, 8)
    for t in range(8):
        toks = [int(conts[s][t]) for s in range(B)]
        toks[restarter] = int(other[T + t])
        pos = [128 + t] * B
        pos[restarter] = T + t
        la, _ = a.forward(toks, pos)
        lb, _ = b.forward(toks, pos)
        lf, _ = fresh.forward([toks[restarter]], [T + t])
        for s in keep:
            assert np.array_equal(bits(la[s]), bits(lb[s])), (t, s)
        assert np.array_equal(bits(lf[0]), bits(lb[restarter])), t
    rows_equal(a, b, spec, [0, 64, 127, 128, 135], slots=keep)
    assert b.kv_sharing() == (2, 2)
    a.close(); b.close(); fresh.close()


def test_copy_on_write_inside_the_greedy_loop(model_dir):
    """decode_greedy started in forked slots at a position BELOW n_pos, with enough steps to cross from a shared block into the next:
    ids equal the unshared model's, and the owner that did not take part is untouched"""
    path, spec, prefix, a, b = cow_setup(model_dir)
    tok = [int(prefix[100])] * 3
    ia = a.decode_greedy(tok, [100] * 3, 40)                   # positions 100 .. 139: block 1 (shared) into block 2
    ib = b.decode_greedy(tok, [100] * 3, 40)
    assert np.array_equal(ia, ib)
    assert b.kv_sharing() == (1, 3)                            # slots 0, 1, 2 each copied block 1 (slot 3 keeps the page), block 0 is shared
    assert b.kv_pages()[0] == 2 + 3 + 3                        # ... and each of the three entered block 2
    rows_equal(a, b, spec, [0, 99, 100, 127, 128, 139], slots=range(3))
    rows_equal(a, b, spec, [0, 99, 100, 127], slots=[3])
    # slot 3 still holds the prefix: it continues like slot 3 of model A (whose slots 0..2 ran the same loop)
    conts = continuations(spec, 4)
    for t in range(4):
        toks = [int(conts[s][t]) for s in range(B)]
        pos = [140 + t] * 3 + [128 + t]
        la, _ = a.forward(toks, pos)
        lb, _ = b.forward(toks, pos)
        for s in range(B):
            assert np.array_equal(bits(la[s]), bits(lb[s])), (t, s)
    a.close(); b.close()


# ---- 4. release and leaks ------------------------------------------------------------------------------------------------------------
def test_release_of_shared_pages_and_reuse(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    prefix = prefix_ids(spec, 100)
    a, b = own(load(path, True), prefix), forked(load(path, True), prefix)
    assert b.kv_pages()[0] == 2 + 3 and b.kv_sharing() == (1, 0)
    b.kv_release(0)                                            # the source leaves: its partial page is nobody else's, block 0 is
    assert b.kv_pages()[0] == 4 and b.kv_sharing() == (1, 0)
    conts = continuations(spec, 8)
    for t in range(8):                                         # (slot 0 of both models is fed a fresh sequence from position 0)
        toks = [int(conts[s][t]) for s in range(B)]
        pos = [t] + [100 + t] * 3
        la, _ = a.forward(toks, pos)
        lb, _ = b.forward(toks, pos)
        for s in range(1, B):
            assert np.array_equal(bits(la[s]), bits(lb[s])), (t, s)
    b.kv_release(0)
    b.kv_release(1); b.kv_release(2)
    assert b.kv_pages()[0] == 2 and b.kv_sharing()[0] == 0     # slot 3 alone: block 0 and its own block 1
    b.kv_release(3)
    assert b.kv_pages()[0] == 0 and b.kv_sharing()[0] == 0
    # the recycled pages serve a fresh sequence with the bits of a fresh model (zero-fill still holds: non-causal reads every row)
    fresh = load(path, True, max_batch=1)
    seq = mf.prompt_ids(55, 70, spec.vocab_size)
    for t in range(70):
        causal = 0 if t in (3, 69) else 1
        lf, _ = fresh.forward([int(seq[t])], [t], is_causal=causal)
        lb, _ = b.forward([int(seq[t])], [t], is_causal=causal)
        assert np.array_equal(bits(lf[0]), bits(lb[0])), t
    a.close(); b.close(); fresh.close()


# ---- 5. zero tail ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_f16", [False, True], ids=["fp32-rows", "fp16-rows"])
def test_fork_does_not_leak_the_sources_later_rows(model_dir, kv_f16):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    m = load(path, True, max_batch=2, kv_f16=kv_f16)
    m.prefill(prefix_ids(spec, 100), 0, 0)
    m.kv_fork(0, 70, [1])
    for layer in range(spec.n_layer):
        for which in ("k", "v"):
            for pos in range(70, 100):
                assert not bits(m.read_state(which, spec.kv_dim, 1, layer, pos)).any(), (which, layer, pos)
                assert bits(m.read_state(which, spec.kv_dim, 0, layer, pos)).any()
            for pos in (0, 63, 64, 69):
                assert np.array_equal(bits(m.read_state(which, spec.kv_dim, 1, layer, pos)), bits(m.read_state(which, spec.kv_dim, 0, layer, pos)))
    m.close()


# ---- 6. pool exhaustion ------------------------------------------------------------------------------------------------------------------
def test_fork_and_copy_on_write_on_an_exhausted_pool(model_dir, monkeypatch):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    monkeypatch.setenv("NANO_KV_PAGES", "4")
    m = load(path, True)
    und = load(path, True)                                     # the undisturbed model: slot 1's sequence alone
    monkeypatch.delenv("NANO_KV_PAGES")
    prefix, seq = prefix_ids(spec, 100), mf.prompt_ids(66, 20, spec.vocab_size)
    m.prefill(prefix, 0, 0)
    m.prefill(seq[:10], 0, 1); und.prefill(seq[:10], 0, 1)
    assert m.kv_pages() == (3, 4)
    with pytest.raises(nb.NanoHipError, match="pages"):        # 3 partial-block pages wanted, 2 to be had (the free one and slot 1's)
        m.kv_fork(0, 100, [1, 2, 3])
    assert m.kv_pages() == (3, 4) and m.kv_sharing() == (0, 0)
    for t in range(10, 14):                                    # slot 1 goes on with its own sequence (slot 0 re-fed its last token)
        lm, _ = m.forward([int(prefix[99]), int(seq[t])], [99, t])
        lu, _ = und.forward([int(prefix[99]), int(seq[t])], [99, t])
        assert np.array_equal(bits(lm[1]), bits(lu[1])), t
    m.kv_fork(0, 100, [1, 2])
    assert m.kv_pages() == (4, 4) and m.kv_sharing() == (1, 0)
    with pytest.raises(nb.NanoHipError, match="pages"):        # slot 1 restarting at 0 must copy block 0: no page left
        m.forward([int(prefix[99]), int(seq[0])], [99, 0])
    assert m.kv_pages() == (4, 4) and m.kv_sharing() == (1, 0)
    m.kv_release(2)
    assert m.kv_pages() == (3, 4) and m.kv_sharing() == (1, 0)
    fresh = load(path, True, max_batch=1)
    lm, _ = m.forward([int(prefix[99]), int(seq[0])], [99, 0])
    lf, _ = fresh.forward([int(seq[0])], [0])
    assert np.array_equal(bits(lm[1]), bits(lf[0]))
    assert m.kv_pages() == (4, 4) and m.kv_sharing() == (0, 1)
    m.close(); und.close(); fresh.close()


# ---- 7. FP16 rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("preset,quant,gs", [("tiny-qwen3", "q80", 64), ("tiny-nano-odd", "f32", 0)])
def test_fork_equals_own_ingestion_fp16_rows(model_dir, preset, quant, gs, paged):
    """FP16 rows (tiny-nano-odd: 96 elements = 192 bytes), one n_pos with a partial block.  Both presets move as 16-byte vectors: no
    preset has FP16 rows that are a multiple of 8 but not of 16 bytes (kv_dim % 8 == 4) -- see the next test for that path."""
    path, spec = synth_model(model_dir, preset, quant, gs)
    fork_equals_own(path, spec, paged, 100, kv_f16=True)


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_fork_equals_own_ingestion_fp16_rows_of_72_bytes(model_dir, paged):
    """the copy kernel's 8-byte path: a hand-made Nano-architecture spec with n_embd 144, 4 heads, 1 KV head has kv_dim 36, so its FP16
    rows are 72 bytes -- a multiple of 8, not of 16.  (Such a model decodes with the step's kernels as they are: head_dim % 4 == 0.)"""
    spec = mf.ModelSpec(mf.ARCH_NANO, 256, 512, 2, 144, 4, 1, 256, 36, 1, mf.QUANT_F32, 0)
    assert spec.kv_dim * 2 % 16 == 8
    path = os.path.join(model_dir, "fork-kv36-f32.bin")
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=39)
    fork_equals_own(path, spec, paged, 100, kv_f16=True)


# ---- 8. sampling and the greedy loop from forked slots --------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_greedy_loop_and_batched_sampling_from_forked_slots(model_dir, paged):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    prefix = prefix_ids(spec, 100)
    a, b = own(load(path, paged), prefix), forked(load(path, paged), prefix)
    firsts = [int(c[0]) for c in continuations(spec, 1)]
    ia = a.decode_greedy(firsts, [100] * B, 40)                # positions 100 .. 139: across the boundary at 128
    ib = b.decode_greedy(firsts, [100] * B, 40)
    assert np.array_equal(ia, ib)
    hist = [np.concatenate([prefix, [firsts[s]], ia[:, s]]).astype(np.uint32) for s in range(B)]
    params = [(1.0 + 0.1 * s, 0.0 if s == 1 else 0.7 + 0.1 * s, 0.9, 0.11 + 0.2 * s, hist[s]) for s in range(B)]
    toks = [int(ia[-1, s]) for s in range(B)]
    ra = a.forward_sample_batch(toks, [140] * B, params)
    rb = b.forward_sample_batch(toks, [140] * B, params)
    for s in range(B):
        for name, _ in nb.NanoHipSample._fields_:
            va, vb = getattr(ra[s], name), getattr(rb[s], name)
            assert (list(va) == list(vb)) if name == "top" else (va == vb), (s, name)
    a.close(); b.close()


# ---- 9. argument errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_argument_errors_change_nothing(model_dir, paged):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    prefix = prefix_ids(spec, 70)
    m = forked(load(path, paged), prefix)
    und = forked(load(path, paged), prefix)
    state = (m.kv_pages(), m.kv_sharing()) if paged else None
    for src, n_pos, dsts in ((B, 10, [1]), (0, 10, [B]), (0, S + 1, [1]), (0, 10, [0]), (0, 10, [1, 0]), (0, 10, [1, 2, 1])):
        with pytest.raises(nb.NanoHipError):
            m.kv_fork(src, n_pos, dsts)
    raw = C.CDLL(nb.LIB_PATH).nano_hip_kv_fork                             # (its own prototype: the binding's refuses None for the list)
    raw.restype, raw.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    one = np.ones(1, np.uint32)
    assert raw(m.h, 0, 10, None, 1) == -1 and raw(None, 0, 10, one.ctypes.data, 1) == -1
    if paged:
        assert (m.kv_pages(), m.kv_sharing()) == state
    else:
        with pytest.raises(nb.NanoHipError):
            m.kv_sharing()                                     # not a paged model, like kv_pages
        with pytest.raises(nb.NanoHipError):
            m.kv_pages()
    run_equal(und, m, continuations(spec, 6), 70, what="after refused forks")
    # n_pos == 0 is valid: paged destinations end up empty, contiguous ones are left alone
    m.kv_fork(0, 0, [1, 2])
    if paged:
        assert m.kv_pages()[0] == 2 + 1 and m.kv_sharing()[0] == 1         # slot 0 and slot 3 remain
    m.close(); und.close()


# ---- 10. engine entry ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("replicas", [1, 2])
def test_engine_prefill_shared(model_dir, replicas):
    """Engine.prefill_shared(prefix, 4) then forward_batch with four different next tokens equals DeviceModels on the same file that
    prefilled each slot themselves; with a second replica on the same device (as tests/test_gpu_e2e.py shares one GPU) sequence i is
    row i // 2 of replica i % 2's two-sequence step, so the models to equal step the same shares (the attention split of a step, and
    with it the last bits, depends on how many sequences the step has)."""
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    prefix = prefix_ids(spec, 100)
    G = replicas
    refs = [own(load(path, False, max_batch=B // G), prefix, range(B // G)) for _ in range(G)]
    e = nb.Engine(path, max_seq_len=S, max_batch=B // G)
    if replicas == 2:
        e.L.nano_context_replicate.restype = C.c_int
        e.L.nano_context_replicate.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
        assert e.L.nano_context_replicate(e.ctx, (C.c_int * 1)(0), 1) == 0, nb.last_error()
    e.prefill_shared(prefix, B)
    conts = continuations(spec, 3)
    for t in range(3):
        toks = [int(conts[s][t]) for s in range(B)]
        le = e.forward_batch(toks, [100 + t] * B, want_logits=True, vocab=spec.vocab_size)
        for r in range(G):
            la, _ = refs[r].forward(toks[r::G], [100 + t] * (B // G))
            for k in range(B // G):
                assert np.array_equal(bits(la[k]), bits(le[k * G + r])), (replicas, t, r, k)
    for m in refs:
        m.close()
    e.close()
