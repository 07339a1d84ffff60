"""GPU tests of ragged steps (nano_hip_step_rows / nano_prefill_batch, include/nano_mi355x.h, include/nano_infer_abi.h): rows of
several KV slots, each with its own position, share the weight reads of one pass.  The bar is exact: whatever a call feeds, every slot
must afterwards be BIT FOR BIT the slot that nano_hip_prefill fed segment by segment ("equal" always means equal uint32 views of the
floats) -- K and V rows, the logits of later steps, the row arg-maxes against nano_hip_verify_draft's -- on the contiguous FP32, the FP16
and the paged cache."""
import os

import numpy as np
import pytest

from nano_amd import binding as nb
from nano_amd import modelfile as mf
from fused_ref import bits

pytestmark = pytest.mark.gpu

S = 256
CASES = [("tiny-qwen3", "q80", 64), ("tiny-nano", "f32", 0), ("tiny-qwen3", "q4k", 0)]
CACHES = {"fp32": dict(kv_f16=False, kv_paged=False), "fp16": dict(kv_f16=True, kv_paged=False), "paged": dict(kv_f16=False, kv_paged=True)}

_models = {}


def synth_model(model_dir, preset, quant, gs, block=256):
    """the tiny presets with a RoPE table (block_size) long enough for several 64-position buckets"""
    key = (preset, quant, gs, block)
    if key not in _models:
        spec = mf.preset(preset, quant, group_size=gs, block_size=block)
        path = os.path.join(model_dir, f"rows-{preset}-{quant}-{gs}-{block}.bin")
        mf.write_model(path, spec, seed=39)
        _models[key] = (path, spec)
    return _models[key]


def load(path, cache, max_batch=4, max_seq_len=S):
    return nb.load_model_file(path, max_seq_len=max_seq_len, max_batch=max_batch, **CACHES[cache])


def slot_ids(spec, slot, n=S):
    return mf.prompt_ids(300 + slot, n, spec.vocab_size)


def seg_tokens(spec, segs, ids=None):
    """the ids of the segments, segment after segment: slot s feeds its own sequence slot_ids(s)"""
    return np.concatenate([(ids[s] if ids else slot_ids(spec, s))[p0:p0 + n] for s, p0, n in segs] + [np.zeros(0, np.uint32)]).astype(np.uint32)


def per_slot(m, spec, segs, verify=False, ids=None):
    """the reference side: every segment through nano_hip_prefill (verify: nano_hip_verify_draft, returning the rows' arg-maxes)"""
    out = []
    for s, p0, n in segs:
        t = (ids[s] if ids else slot_ids(spec, s))[p0:p0 + n]
        if verify and n:
            out.append(m.verify_draft(t, pos0=p0, slot=s)[0])
        else:
            m.prefill(t, p0, s)
    return np.concatenate(out) if out else None


def bucket_positions(length):
    """first / middle / last position of every 64-position bucket of a sequence of `length` positions"""
    ps = set()
    for lo in range(0, length, 64):
        hi = min(lo + 63, length - 1)
        ps |= {lo, (lo + hi) // 2, hi}
    return sorted(ps)


def rows_equal(a, b, spec, lengths, slot_map=None):
    """K and V rows of every layer equal at the bucket positions of every slot (lengths: slot -> positions held; slot_map: a's slot -> b's)"""
    for s, n in lengths.items():
        sb = slot_map[s] if slot_map else s
        for layer in range(spec.n_layer):
            for pos in bucket_positions(n):
                for which in ("k", "v"):
                    ra, rb = a.read_state(which, spec.kv_dim, s, layer, pos), b.read_state(which, spec.kv_dim, sb, layer, pos)
                    assert np.array_equal(bits(ra), bits(rb)), (which, "slot", s, "layer", layer, "pos", pos)


def steps_equal(a, b, spec, lengths, steps=8):
    """teacher-forced batched forward steps of slots 0 .. n-1 from each one's own length: logits and arg-max equal on both models"""
    slots = sorted(lengths)
    assert slots == list(range(len(slots)))
    conts = [mf.prompt_ids(700 + s, steps, spec.vocab_size) for s in slots]
    for t in range(steps):
        toks, pos = [int(conts[s][t]) for s in slots], [lengths[s] + t for s in slots]
        la, aa = a.forward(toks, pos, want_argmax=True)
        lb, ab = b.forward(toks, pos, want_argmax=True)
        for s in slots:
            assert np.array_equal(bits(la[s]), bits(lb[s])), ("step", t, "slot", s)
        assert np.array_equal(aa, ab), t


def apply_lengths(lengths, segs):
    for s, p0, n in segs:
        if n:
            lengths[s] = max(lengths.get(s, 0), p0 + n)
    return lengths


SEGS_1 = [(2, 0, 15), (0, 0, 70), (3, 0, 1), (1, 0, 150)]        # 236 rows: several passes, rows of buckets 0 and 1 of one slot in one pass
SEGS_2 = [(1, 150, 20), (2, 15, 60)]                             # continuing at non-zero pos0; a pass with buckets 2, 0 (and then 0, 1)


# ---- 1. one call = per-slot prefill -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", list(CACHES))
@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_equals_per_slot_prefill(model_dir, preset, quant, gs, cache):
    path, spec = synth_model(model_dir, preset, quant, gs)
    a, b = load(path, cache), load(path, cache)
    lengths = {}
    for segs in (SEGS_1, SEGS_2):
        per_slot(a, spec, segs)
        assert b.step_rows(segs, seg_tokens(spec, segs)) is None
        apply_lengths(lengths, segs)
        rows_equal(a, b, spec, lengths)
    assert lengths == {0: 70, 1: 170, 2: 75, 3: 1}
    if cache == "paged":
        assert a.kv_pages() == b.kv_pages()
    steps_equal(a, b, spec, lengths)
    rows_equal(a, b, spec, {s: n + 8 for s, n in lengths.items()})
    a.close(); b.close()


@pytest.mark.parametrize("cache", list(CACHES))
@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_three_buckets_in_one_pass(model_dir, preset, quant, gs, cache):
    """22 rows whose attention splits 1, 2 and 3 ways (positions below 64, 120..127, 128..131): where the pass holds them all, three
    attention launches per layer over one set of projections"""
    path, spec = synth_model(model_dir, preset, quant, gs)
    a, b = load(path, cache), load(path, cache)
    for m in (a, b):
        m.prefill(slot_ids(spec, 0)[:120], 0, 0)
    segs = [(0, 120, 12), (1, 0, 10)]
    want = per_slot(a, spec, segs, verify=True)
    got = b.step_rows(segs, seg_tokens(spec, segs), want_argmax=True)
    assert np.array_equal(want, got)
    lengths = {0: 132, 1: 10}
    rows_equal(a, b, spec, lengths)
    steps_equal(a, b, spec, lengths, steps=3)
    a.close(); b.close()


# ---- 2. the rows' arg-maxes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", list(CACHES))
@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_argmax_out_is_verify_drafts(model_dir, preset, quant, gs, cache):
    path, spec = synth_model(model_dir, preset, quant, gs)
    a, b = load(path, cache), load(path, cache)
    lengths = {}
    for segs in (SEGS_1, SEGS_2):
        want = per_slot(a, spec, segs, verify=True)
        got = b.step_rows(segs, seg_tokens(spec, segs), want_argmax=True)
        assert got.dtype == np.uint32 and got.shape == want.shape
        assert np.array_equal(want, got), np.flatnonzero(want != got)
        apply_lengths(lengths, segs)
    rows_equal(a, b, spec, lengths)
    a.close(); b.close()


# ---- 3. one full pass over many slots ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", list(CACHES))
@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_sixteen_slots_in_one_pass(model_dir, preset, quant, gs, cache):
    path, spec = synth_model(model_dir, preset, quant, gs)
    a, b = load(path, cache, max_batch=16), load(path, cache, max_batch=16)
    segs = [(s, 0, 4) for s in (5, 0, 15, 9, 1, 2, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14)]          # 64 rows, not in slot order
    if b.prefill_chunk_tokens() == 64:
        assert nb.rows_plan(segs, 64, S)[3] == 1
    want = per_slot(a, spec, segs, verify=True)
    got = b.step_rows(segs, seg_tokens(spec, segs), want_argmax=True)
    assert np.array_equal(want, got)
    lengths = {s: 4 for s in range(16)}
    rows_equal(a, b, spec, lengths)
    steps_equal(a, b, spec, lengths, steps=2)
    a.close(); b.close()


# ---- 4. greedy continuous batching ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", list(CACHES))
@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_greedy_rows_next_to_a_joining_prompt(model_dir, preset, quant, gs, cache):
    """slot 3 decodes 40 ids as one-row segments fed by the returned arg-max (positions 39 .. 78: across a bucket end) while slot 0
    ingests a 100-token prompt, 25 rows per call"""
    path, spec = synth_model(model_dir, preset, quant, gs)
    a, b = load(path, cache), load(path, cache)
    prompt, joiner = mf.prompt_ids(41, 40, spec.vocab_size), mf.prompt_ids(42, 100, spec.vocab_size)
    a.prefill(prompt[:-1], 0, 0)
    alone = a.decode_greedy([int(prompt[-1])], [len(prompt) - 1], 40)[:, 0]
    b.prefill(prompt[:-1], 0, 3)
    tok, pos, ids = int(prompt[-1]), len(prompt) - 1, []
    for i in range(40):
        segs, toks = [(3, pos, 1)], [tok]
        if i < 4:
            segs.append((0, 25 * i, 25)); toks += joiner[25 * i:25 * i + 25].tolist()
        am = b.step_rows(segs, toks, want_argmax=True)
        tok = int(am[0]); ids.append(tok); pos += 1
    assert ids == alone.tolist()
    a.prefill(joiner, 0, 1)
    rows_equal(a, b, spec, {1: 100}, slot_map={1: 0})
    rows_equal(a, b, spec, {0: 79}, slot_map={0: 3})
    a.close(); b.close()


# ---- 5. the paged cache with shared pages -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_paged_shared_pages(model_dir, preset, quant, gs):
    """slots 1 and 2 are forks of slot 0's 100-position prefix: one call continues both from position 100 and restarts slot 0 at
    position 10 -- inside the page all three share, which slot 0 must get a copy of before it writes"""
    path, spec = synth_model(model_dir, preset, quant, gs)
    a, b = load(path, "paged"), load(path, "paged")
    prefix = mf.prompt_ids(101, 100, spec.vocab_size)
    ids = {s: np.concatenate([prefix, mf.prompt_ids(500 + s, 30, spec.vocab_size)]) for s in (1, 2)}
    ids[0] = np.concatenate([prefix[:10], mf.prompt_ids(500, 30, spec.vocab_size)])
    segs = [(1, 100, 30), (2, 100, 30), (0, 10, 30)]
    for s in (0, 1, 2):
        a.prefill(prefix, 0, s)
    per_slot(a, spec, segs, ids=ids)
    b.prefill(prefix, 0, 0)
    b.kv_fork(0, 100, [1, 2])
    assert b.kv_sharing() == (1, 0) and b.kv_pages()[0] == 4          # block 0 shared by three, a page each for the partial block 1
    b.step_rows(segs, seg_tokens(spec, segs, ids=ids))
    # kv_ensure: slot 0 writes into block 0, whose page has two more owners -> one copy; slots 1 and 2 write into pages of their own and
    # go on sharing block 0; block 2 (positions 128 ..) is new for both
    assert b.kv_sharing() == (1, 1)
    assert b.kv_pages()[0] == 4 + 1 + 2
    lengths = {0: 100, 1: 130, 2: 130}                                 # (slot 0: positions 40 .. 99 still hold the prefix's rows)
    rows_equal(a, b, spec, lengths)
    steps_equal(a, b, spec, {0: 40, 1: 130, 2: 130}, steps=4)
    a.close(); b.close()


# ---- 6. strict and exact mode -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "exact"])
def test_reference_order_modes(model_dir, mode):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    a, b = load(path, "fp32"), load(path, "fp32")
    for m in (a, b):
        (m.set_strict if mode == "strict" else m.set_exact)(True)
    assert b.prefill_chunk_tokens() == 1
    segs = [(2, 0, 5), (0, 0, 66), (1, 0, 1)]
    want = per_slot(a, spec, segs, verify=True)
    got = b.step_rows(segs, seg_tokens(spec, segs), want_argmax=True)
    assert np.array_equal(want, got)
    segs2 = [(1, 1, 3), (2, 5, 2)]
    per_slot(a, spec, segs2)
    b.step_rows(segs2, seg_tokens(spec, segs2))
    lengths = {0: 66, 1: 4, 2: 7}
    rows_equal(a, b, spec, lengths)
    steps_equal(a, b, spec, lengths, steps=2)
    a.close(); b.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def snapshot(m, spec, slots, paged):
    rows = [bits(m.read_state("k", spec.kv_dim, s, 0, 5)).copy() for s in slots]
    return rows, (m.kv_pages() if paged else None)


@pytest.mark.parametrize("cache", ["fp32", "paged"])
def test_refusals_feed_nothing(model_dir, cache):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    m = load(path, cache)
    for s in range(4):
        m.prefill(slot_ids(spec, s)[:20], 0, s)
    before = snapshot(m, spec, range(4), cache == "paged")
    V = spec.vocab_size
    bad = [([(4, 0, 2)], [1, 2]),                                    # slot >= max_batch
           ([(1, 5, 2), (0, 5, 1), (1, 9, 1)], [1, 2, 3, 4]),        # two segments with the same slot
           ([(0, 255, 2)], [1, 2]),                                  # beyond max_seq_len
           ([(0, 5, 2), (1, 5, 1)], [1, V, 3]),                      # token >= vocab
           ([(0, 5, 2), (1, 5, 1, 7)], [1, 2, 3])]                   # reserved != 0
    for segs, toks in bad:
        for want in (False, True):
            with pytest.raises(nb.NanoHipError):
                m.step_rows(segs, toks, want_argmax=want)
    L, s, t = nb.lib(), nb.row_segs([(0, 5, 2)]), np.array([1, 2], np.uint32)
    assert L.nano_hip_step_rows(m.h, None, 1, t.ctypes.data, None) == -1         # null segs / tokens
    assert L.nano_hip_step_rows(m.h, s.ctypes.data, 1, None, None) == -1
    # empty calls: 0, nothing touched
    assert L.nano_hip_step_rows(m.h, None, 0, None, None) == 0
    assert m.step_rows([], []) is None and m.step_rows([(2, 5, 0), (3, 250, 0)], [], want_argmax=True).size == 0
    after = snapshot(m, spec, range(4), cache == "paged")
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and before[1] == after[1]
    m.close()


def test_refusals_of_the_rope_table_and_lora(model_dir):
    """Nano architecture: the RoPE table has block_size rows, fewer here than max_seq_len; LoRA switched on refuses the call, off serves it"""
    path, spec = synth_model(model_dir, "tiny-nano", "f32", 0, block=128)
    m = load(path, "fp32")
    m.prefill(slot_ids(spec, 0)[:20], 0, 0)
    before = snapshot(m, spec, [0], False)
    with pytest.raises(nb.NanoHipError, match="RoPE"):
        m.step_rows([(0, 120, 10)], list(range(10)))
    lpath = os.path.join(model_dir, "rows-tiny-nano.lora")
    mf.write_lora(lpath, spec, rank=4, alpha=8, seed=3)
    m.lora_attach_file(lpath)
    m.lora_enable(True)
    with pytest.raises(nb.NanoHipError, match="LoRA"):
        m.step_rows([(0, 5, 2)], [1, 2])
    m.lora_enable(False)
    after = snapshot(m, spec, [0], False)
    assert np.array_equal(before[0][0], after[0][0])
    assert m.step_rows([(0, 5, 2)], [1, 2], want_argmax=True).size == 2
    m.close()


# ---- 8. the engine ----------------------------------------------------------------------------------------------------------------
def test_engine_prefill_batch(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    prompts = [mf.prompt_ids(900 + i, n, spec.vocab_size) for i, n in enumerate((5, 70, 1, 33))]
    e = nb.Engine(path, max_seq_len=S, max_batch=4)
    first = e.prefill_batch(prompts)
    m = load(path, "fp32")
    for s, p in enumerate(prompts):
        m.prefill(p[:-1], 0, s)
    lens = [len(p) for p in prompts]
    _, want = m.forward([int(p[-1]) for p in prompts], [n - 1 for n in lens], want_argmax=True)
    assert np.array_equal(first, want)
    # ... and the engine's sequences go on from there as the model's do
    nxt = e.forward_batch(first, lens, want_logits=False)
    _, want2 = m.forward(first, lens, want_argmax=True)
    assert np.array_equal(nxt, want2)
    with pytest.raises(nb.NanoHipError):
        e.prefill_batch([[1, 2], [spec.vocab_size]])
    e.close(); m.close()
