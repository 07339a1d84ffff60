"""Opt-in FP8 KV cache (NANO_HIP_KV_FP8 / NANO_KV_FP8=1): rows of OCP e4m3fn bytes with scale 1, rounded once when written
(e4m3_rne(clamp(x, -448, 448)), tests/kv8_ref.py), the current token attends to its own rounded rows, arithmetic stays FP32.
The gate on the arithmetic is tests/test_gpu_attention_decode_fp8.py; here, at model level:
  * the stored rows ARE the FP32-cache model's rows in e4m3 (layer 0: its rows depend on no cache row);
  * what holds bit for bit on the FP32 and FP16 cache holds on FP8 rows: a batch equals its sequences alone, batched prefill equals
    token-by-token feeding, a ragged step equals prefill per segment, a forked slot equals a slot that ingested the prefix itself,
    the paged cache equals the contiguous one;
  * rows of kv_dim % 8 == 4 bytes (the copy kernel's 4-byte form) survive fork and release;
  * the gating: not with FP16 rows, strict mode, exact mode or LoRA; with the flag off nothing changes;
  * the distance from the FP32-cache path is PRINTED next to the FP16 cache's, and only asserted to be finite and > 0: e4m3 keeps 3
    mantissa bits against FP16's 10, and there is no reference implementation of an FP8 cache to take a bar from (DESIGN.md §2 and
    profiles/kv_fp8.txt state the measured figures)."""
import os

import numpy as np
import pytest

import kv8_ref
from conftest import e2e_golden, rel_err, synth_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf
from test_gpu_attention_decode import K_TOL
from test_gpu_attention_decode_fp8 import e4m3_step
from test_gpu_kv16 import CASES as KV16_CASES

pytestmark = pytest.mark.gpu

INVARIANT_MODELS = [("tiny-qwen3", "q80", 64), ("tiny-nano", "f32", 0)]
EINVAL = "nano_hip error -1:"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def as_e4m3(x):
    """what an FP8 row holding x reads back as"""
    return kv8_ref.e4m3_decode(kv8_ref.e4m3_encode(x))


def rows_of(m, spec, slot, n_pos):
    """every K and V row of positions 0..n_pos-1 of a slot, all layers: [2][L][n_pos][kv_dim]"""
    return np.stack([np.stack([np.stack([m.read_state(name, spec.kv_dim, slot=slot, layer=l, pos=p) for p in range(n_pos)])
                               for l in range(spec.n_layer)]) for name in ("k", "v")])


@pytest.mark.parametrize("preset,quant,gs", KV16_CASES)
def test_kv8_stored_rows_and_distance(model_dir, preset, quant, gs):
    g = np.load(e2e_golden(preset, quant, gs))
    path, spec = synth_model(model_dir, preset, quant, gs)
    S = int(g["max_seq_len"])
    m32 = nb.load_model_file(path, max_seq_len=S, max_batch=1, kv_f16=False)
    m16 = nb.load_model_file(path, max_seq_len=S, max_batch=1, kv_f16=True)
    m8 = nb.load_model_file(path, max_seq_len=S, max_batch=1, kv_fp8=True)
    ids = g["ids"]
    worst8 = worst16 = 0.0
    for pos in range(len(ids) - 1):
        a, _ = m32.forward([int(ids[pos])], [pos])
        h, _ = m16.forward([int(ids[pos])], [pos])
        b, _ = m8.forward([int(ids[pos])], [pos])
        assert np.isfinite(b).all(), pos
        worst8 = max(worst8, rel_err(b[0], a[0])); worst16 = max(worst16, rel_err(h[0], a[0]))
    for pos in range(len(ids) - 1):
        v32 = m32.read_state("v", spec.kv_dim, layer=0, pos=pos); v8 = m8.read_state("v", spec.kv_dim, layer=0, pos=pos)
        assert np.array_equal(bits(v8), bits(as_e4m3(v32))), ("v", pos)
        k32 = m32.read_state("k", spec.kv_dim, layer=0, pos=pos); k8 = m8.read_state("k", spec.kv_dim, layer=0, pos=pos)
        if pos == 0:
            assert np.array_equal(bits(k8), bits(as_e4m3(k32))), ("k", pos)
        k64 = np.clip(k32.astype(np.float64), -448.0, 448.0)
        assert (np.abs(k8 - k64) <= K_TOL * np.abs(k32).max() + e4m3_step(k64)).all(), ("k", pos)
    m32.close(); m16.close(); m8.close()
    print(f"{preset}/{quant}: logits vs the FP32-cache path over {len(ids) - 1} positions: FP8 rows {worst8:.3e}, FP16 rows {worst16:.3e}")
    assert np.isfinite(worst8) and worst8 > 0.0


@pytest.mark.parametrize("preset,quant,gs", INVARIANT_MODELS)
def test_kv8_batch_prefill_and_paged_invariants(model_dir, preset, quant, gs):
    path, spec = synth_model(model_dir, preset, quant, gs)
    B, T = 3, 21
    seqs = [mf.prompt_ids(900 + b, T, spec.vocab_size) for b in range(B)]
    mb = nb.load_model_file(path, max_seq_len=32, max_batch=B, kv_fp8=True)
    batched = [mb.forward([int(s[pos]) for s in seqs], [pos] * B)[0] for pos in range(T)]
    mb.close()
    m1 = nb.load_model_file(path, max_seq_len=32, max_batch=1, kv_fp8=True)
    mp = nb.load_model_file(path, max_seq_len=32, max_batch=1, kv_fp8=True, kv_paged=True)
    for b in range(B):                                     # a batch of 3 equals its sequences alone; the paged cache equals the contiguous one
        for pos in range(T):
            lg, _ = m1.forward([int(seqs[b][pos])], [pos])
            assert np.array_equal(bits(lg[0]), bits(batched[pos][b])), (b, pos)
            if b == B - 1:
                lp, _ = mp.forward([int(seqs[b][pos])], [pos])
                assert np.array_equal(bits(lp[0]), bits(lg[0])), ("paged", pos)
    fed = rows_of(m1, spec, 0, T - 1)                      # (sequence B - 1, token by token)
    assert np.array_equal(bits(rows_of(mp, spec, 0, T - 1)), bits(fed))
    m1.prefill(seqs[B - 1][:T - 1], 0)                     # batched prefill over the same rows
    assert np.array_equal(bits(rows_of(m1, spec, 0, T - 1)), bits(fed)), "prefill left other rows than token-by-token feeding"
    got, _ = m1.forward([int(seqs[B - 1][T - 1])], [T - 1])
    assert np.array_equal(bits(got[0]), bits(batched[T - 1][B - 1]))
    m1.close(); mp.close()


@pytest.mark.parametrize("preset,quant,gs", INVARIANT_MODELS)
def test_kv8_step_rows_equals_prefill_per_segment(model_dir, preset, quant, gs):
    path, spec = synth_model(model_dir, preset, quant, gs)
    n0, n1 = 13, 21
    t0, t1 = mf.prompt_ids(31, n0 + 1, spec.vocab_size), mf.prompt_ids(32, n1 + 1, spec.vocab_size)
    ma = nb.load_model_file(path, max_seq_len=32, max_batch=2, kv_fp8=True)
    mb = nb.load_model_file(path, max_seq_len=32, max_batch=2, kv_fp8=True)
    ma.step_rows([(0, 0, n0), (1, 0, n1)], list(t0[:n0]) + list(t1[:n1]))
    mb.prefill(t0[:n0], 0, slot=0); mb.prefill(t1[:n1], 0, slot=1)
    for slot, n in ((0, n0), (1, n1)):
        assert np.array_equal(bits(rows_of(ma, spec, slot, n)), bits(rows_of(mb, spec, slot, n))), slot
    la, _ = ma.forward([int(t0[n0]), int(t1[n1])], [n0, n1])
    lb, _ = mb.forward([int(t0[n0]), int(t1[n1])], [n0, n1])
    assert np.array_equal(bits(la), bits(lb))
    ma.close(); mb.close()


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("preset,quant,gs,n_pos", [("tiny-qwen3", "q80", 64, 70), ("tiny-nano", "f32", 0, 21)])
def test_kv8_fork_equals_own_ingestion(model_dir, preset, quant, gs, n_pos, paged):
    """n_pos 70: one full 64-position block (paged: shared) and a partial one of 6 rows; 21: a partial block alone"""
    path, spec = synth_model(model_dir, preset, quant, gs)
    S = 96 if n_pos > 64 else 32
    ids = mf.prompt_ids(77, n_pos + 1, spec.vocab_size)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=3, kv_fp8=True, kv_paged=paged)
    m.prefill(ids[:n_pos], 0, slot=0)
    m.kv_fork(0, n_pos, [1])
    m.prefill(ids[:n_pos], 0, slot=2)
    src, dst, own = (rows_of(m, spec, s, n_pos) for s in (0, 1, 2))
    assert np.array_equal(bits(dst), bits(src)) and np.array_equal(bits(dst), bits(own))
    if n_pos + 1 < S:
        assert not rows_of(m, spec, 1, n_pos + 2)[:, :, n_pos:].any(), "rows behind the forked prefix are not zero"
    lg, _ = m.forward([int(ids[n_pos])] * 3, [n_pos] * 3)
    assert np.array_equal(bits(lg[1]), bits(lg[2])) and np.array_equal(bits(lg[1]), bits(lg[0]))
    if paged:
        assert m.kv_sharing()[0] == (1 if n_pos >= 64 else 0)           # the full block's page has two owners; no byte of it moved
    m.close()


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_kv8_row_copy_of_kv_dim_36(model_dir, paged):
    """One KV head of head_dim 36: a row is 36 bytes (kv_dim % 8 == 4), so the copy kernel moves 4-byte words."""
    spec = mf.ModelSpec(mf.ARCH_NANO, 64, 512, 2, 144, 4, 1, 128, 0)
    assert spec.kv_dim == 36 and spec.kv_dim % 8 == 4
    path = os.path.join(model_dir, "kv8-hd36-f32.bin")
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=41)
    n_pos, S = 21, 32
    ids = mf.prompt_ids(78, n_pos + 1, spec.vocab_size)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=3, kv_fp8=True, kv_paged=paged)
    m.prefill(ids[:n_pos], 0, slot=0)
    src = rows_of(m, spec, 0, S)
    assert src[:, :, :n_pos].any() and not src[:, :, n_pos:].any()
    m.kv_fork(0, n_pos, [1, 2])
    for d in (1, 2):
        got = rows_of(m, spec, d, S)
        assert np.array_equal(bits(got[:, :, :n_pos]), bits(src[:, :, :n_pos])), d
        assert not got[:, :, n_pos:].any(), "the zero tail rows did not stay zero"
    assert np.array_equal(bits(rows_of(m, spec, 0, S)), bits(src))
    lg, _ = m.forward([int(ids[n_pos])] * 3, [n_pos] * 3)
    assert np.array_equal(bits(lg[1]), bits(lg[0])) and np.array_equal(bits(lg[2]), bits(lg[0]))
    if paged:
        used = m.kv_pages()[0]
        m.kv_release(1); m.kv_release(2)
        assert m.kv_pages()[0] == used - 2
        assert not rows_of(m, spec, 1, S).any()                         # (no page: never-written rows)
        assert np.array_equal(bits(rows_of(m, spec, 0, n_pos)), bits(src[:, :, :n_pos]))
    m.close()


def test_kv8_is_gated(model_dir, monkeypatch):
    for var in ("NANO_KV_F16", "NANO_KV_FP8", "NANO_KV_PAGED"):
        monkeypatch.delenv(var, raising=False)
    path, spec = synth_model(model_dir, "tiny-nano", "f32", 0)
    with pytest.raises(nb.NanoHipError, match=EINVAL):     # one element format
        nb.load_model_file(path, max_seq_len=16, max_batch=1, kv_f16=True, kv_fp8=True)
    monkeypatch.setenv("NANO_KV_F16", "1"); monkeypatch.setenv("NANO_KV_FP8", "1")
    with pytest.raises(nb.NanoHipError, match=EINVAL):     # ... also when the two arrive through the environment
        nb.load_model_file(path, max_seq_len=16, max_batch=1)
    monkeypatch.delenv("NANO_KV_F16")
    m = nb.load_model_file(path, max_seq_len=16, max_batch=1)          # NANO_KV_FP8=1 alone: an FP8 model
    m.forward([1], [0])
    v = m.read_state("v", spec.kv_dim, layer=0, pos=0)
    assert v.any() and np.array_equal(bits(v), bits(as_e4m3(v)))
    m.close()
    monkeypatch.delenv("NANO_KV_FP8")
    m = nb.load_model_file(path, max_seq_len=16, max_batch=1, kv_fp8=True)
    m.set_strict(True)
    with pytest.raises(nb.NanoHipError, match=EINVAL):     # strict parity is defined on the reference's FP32 cache
        m.forward([1], [0])
    m.set_strict(False)
    m.set_exact(True)
    with pytest.raises(nb.NanoHipError, match=EINVAL):     # ... and so is exact mode
        m.forward([1], [0])
    m.set_exact(False)
    lpath = os.path.join(model_dir, "tiny-nano-lora-kv8.bin")
    mf.write_lora(lpath, spec, rank=4, alpha=8, seed=3)
    m.lora_attach_file(lpath)
    with pytest.raises(nb.NanoHipError, match=EINVAL):     # the LoRA v branch writes FP32 rows
        m.forward([1], [0])
    with pytest.raises(nb.NanoHipError, match=EINVAL):     # ... in batched prefill as well: refused before anything is queued
        m.prefill([1, 2, 3], 0)
    with pytest.raises(nb.NanoHipError, match=EINVAL):
        m.prefill_score([1, 2, 3], [2, 3, 4])
    m.lora_enable(False)
    lg, _ = m.forward([1], [0])
    assert np.isfinite(lg).all()
    m.close()


def test_kv8_flag_off_changes_nothing(model_dir, monkeypatch):
    for var in ("NANO_KV_F16", "NANO_KV_FP8", "NANO_KV_PAGED"):
        monkeypatch.delenv(var, raising=False)
    path, spec = synth_model(model_dir, "tiny-qwen3", "q80", 64)
    ids = mf.prompt_ids(12, 8, spec.vocab_size)
    plain = nb.load_model_file(path, max_seq_len=16, max_batch=1)                     # nano_hip_model_create
    off = nb.load_model_file(path, max_seq_len=16, max_batch=1, kv_fp8=False)         # nano_hip_model_create_ex, no flag
    on = nb.load_model_file(path, max_seq_len=16, max_batch=1, kv_fp8=True)
    differs = False
    for pos in range(8):
        a, _ = plain.forward([int(ids[pos])], [pos]); b, _ = off.forward([int(ids[pos])], [pos]); c, _ = on.forward([int(ids[pos])], [pos])
        assert np.array_equal(bits(a), bits(b)), pos
        differs |= not np.array_equal(bits(a), bits(c))
    assert differs                                          # (the option really changes the cache)
    plain.close(); off.close(); on.close()
