"""GPU tests of KV images (nano_hip_kv_save / nano_hip_kv_restore, nano_kv_save / nano_kv_restore; include/nano_mi355x.h,
include/nano_infer_abi.h): a slot's K / V rows parked in host memory and brought back.  The reference keeps one cache per context
(infer/infer.c:46-51) and has no counterpart.  The bar is exact -- copies of bytes have no tolerance: the image holds the cache's own
bytes in tests/kv_image_ref.py's layout, and a restored slot is BIT FOR BIT the slot that was never parked ("equal" below always means
equal uint32 views of the floats).  A missing entry point fails these tests."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kv8_ref
import kv_image_ref as kr
from conftest import e2e_golden
from conftest import synth_model as golden_model
from fused_ref import bits
from nano_amd import binding as nb
from nano_amd import modelfile as mf

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

S, B = 256, 4
FP32, FP16, FP8 = {}, {"kv_f16": True}, {"kv_fp8": True}
FMT_OF = {"fp32": (0, FP32), "fp16": (1, FP16), "fp8": (2, FP8)}

_models = {}


def synth_model(model_dir, preset):
    """the tiny presets (tiny-qwen3 as Q80, the others FP32) with a RoPE table long enough for 256 positions, and hand-made Nano specs
    of one KV head whose rows are 36 and 24 elements: FP16 rows of 72 bytes (8-byte vectors), FP8 rows of 36 (4-byte words) and 24 bytes
    (8-byte vectors)"""
    quant, gs = ("q80", 64) if preset == "tiny-qwen3" else ("f32", 0)
    key = preset
    if key not in _models:
        if preset.startswith("kv"):
            kd = int(preset[2:])
            spec = mf.ModelSpec(mf.ARCH_NANO, 256, 512, 2, 4 * kd, 4, 1, 256, kd, 1, mf.QUANT_F32, 0)
            assert spec.kv_dim == kd
        else:
            spec = mf.preset(preset, quant, group_size=gs, block_size=256)
        path = os.path.join(model_dir, f"kvimage-{preset}-{quant}-{gs}.bin")
        mf.write_model(path, spec, seed=39)
        _models[key] = (path, spec)
    return _models[key]


def load(path, paged, max_batch=B, max_seq_len=S, **kw):
    kw = dict({"kv_fp8": False}, **kw)                                       # explicit flags: the environment is not consulted
    return nb.load_model_file(path, max_seq_len=max_seq_len, max_batch=max_batch, kv_paged=paged, **kw)


def ids_of(spec, n, seed=101):
    return mf.prompt_ids(seed, n, spec.vocab_size)


def state_rows(m, spec, slot, n):
    """(k, v) float32 [n_layer][n][kv_dim] as nano_hip_read_state returns them"""
    out = np.zeros((2, spec.n_layer, n, spec.kv_dim), np.float32)
    for w, which in enumerate(("k", "v")):
        for layer in range(spec.n_layer):
            for pos in range(n):
                out[w, layer, pos] = m.read_state(which, spec.kv_dim, slot, layer, pos)
    return out[0], out[1]


def decoded(rows_u8, fmt):
    """the image's rows [..][row_bytes] as the floats read_state widens them to"""
    if fmt == 0:
        return rows_u8.view(np.float32)
    if fmt == 1:
        return rows_u8.view(np.float16).astype(np.float32)
    return kv8_ref.e4m3_decode(rows_u8)


def steps(m, conts, pos0, row, n_steps=None):
    """batched decode steps of all B slots, every slot fed conts[t] at pos0 + t: the logits of slot `row`, step after step"""
    out = []
    for t in range(len(conts) if n_steps is None else n_steps):
        lg, _ = m.forward([int(conts[t])] * B, [pos0 + t] * B)
        out.append(lg[row].copy())
    return out


def same_bits(a, b, what=""):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(bits(x), bits(y)), (what, "step", t)


# ---- 1. the bytes ----------------------------------------------------------------------------------------------------------------------
BYTES_CASES = [("tiny-qwen3", "fp32"), ("tiny-nano-odd", "fp16"), ("kv36", "fp16"), ("tiny-qwen3", "fp8"), ("kv24", "fp8"), ("kv36", "fp8")]


@pytest.mark.parametrize("preset,fmt", BYTES_CASES)
def test_image_bytes_are_the_cache_rows_in_image_order(model_dir, preset, fmt):
    """slot 1 of a 4-slot model after a prefill of n tokens: the payload is the rows read_state returns, arranged by kv_image_ref, and the
    contiguous and the paged cache give the same image.  kv36 / FP16: 72-byte rows; FP8 rows of 128, 24 and 36 bytes: 16-, 8- and 4-byte
    vectors."""
    path, spec = synth_model(model_dir, preset)
    code, kw = FMT_OF[fmt]
    rb = spec.kv_dim * kr.FMT_BYTES[code]
    if fmt == "fp8":
        assert rb % 16 == {"tiny-qwen3": 0, "kv24": 8, "kv36": 4}[preset]
    if (preset, fmt) == ("kv36", "fp16"):
        assert rb == 72
    mc, mp = load(path, False, **kw), load(path, True, **kw)
    tag = kr.model_tag([getattr(mc.desc, f) for f, _ in nb.NanoModelDesc._fields_], os.path.getsize(path) - 256 - int(np.fromfile(path, "<u4", 1, offset=256)[0]))
    for n in (1, 63, 64, 65, 129):
        toks = ids_of(spec, n, seed=500 + n)
        mc.prefill(toks, 0, 1); mp.prefill(toks, 0, 1)
        ic, ip = mc.kv_save(1, n), mp.kv_save(1, n)
        assert ic.size == mc.kv_image_bytes(n) == nb.kv_image_plan(spec.n_layer, spec.kv_dim, kr.FMT_BYTES[code], n)["total_bytes"]
        assert np.array_equal(ic, ip), ("contiguous and paged images differ", n)
        h, k, v = kr.read(ic)
        assert nb.kv_image_check(ic)["n_pos"] == n
        assert (h["format"], h["n_layer"], h["kv_dim"], h["n_pos"], h["row_bytes"], h["model_tag"]) == (code, spec.n_layer, spec.kv_dim, n, rb, tag)
        sk, sv = state_rows(mc, spec, 1, n)
        assert sk.any() and sv.any()
        assert np.array_equal(bits(decoded(k, code)), bits(sk)) and np.array_equal(bits(decoded(v, code)), bits(sv)), n
        assert np.array_equal(ic, kr.write(k, v, code, tag))                 # nothing but the header and the rows
    assert mc.kv_save(1, 0).size == 64 and nb.kv_image_check(mp.kv_save(1, 0))["payload_bytes"] == 0      # n_pos == 0: the header alone
    mc.close(); mp.close()


# ---- 2. resume equals never parked -------------------------------------------------------------------------------------------------------
def resume(path, spec, src, dst, n=100, T=30, kw=FP32):
    """src / dst: (paged, same model?) -- feed n tokens into slot 1 and save; decode T steps from slot 1 (never parked) and record; fill
    slot 3 of the destination model with other tokens at positions 0 .. n + T, restore into it: the same T steps from slot 3 give the
    same logits.  n = 100, T = 30: the continuation crosses the block boundary at 128."""
    a = load(path, src, **kw)
    a.prefill(ids_of(spec, n), 0, 1)
    img = a.kv_save(1, n)
    conts = ids_of(spec, T, seed=202)
    want = steps(a, conts, n, 1)
    b = a if dst is None else load(path, dst, **kw)
    b.prefill(ids_of(spec, n + T + 1, seed=303), 0, 3)
    b.kv_restore(3, img)
    same_bits(want, steps(b, conts, n, 3), (src, dst, kw))
    # and once more from the bytes as a file would hand them back, after the slot moved on: restore is repeatable
    b.kv_restore(3, img.tobytes())
    same_bits(want[:3], steps(b, conts, n, 3, 3), "second restore")
    a.close()
    if b is not a:
        b.close()


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("fmt", ["fp32", "fp16", "fp8"])
def test_resume_equals_never_parked(model_dir, fmt, paged):
    path, spec = synth_model(model_dir, "tiny-qwen3")
    resume(path, spec, paged, None, kw=FMT_OF[fmt][1])


@pytest.mark.parametrize("src,dst", [(False, False), (True, True), (False, True), (True, False)],
                         ids=["restart-contiguous", "restart-paged", "contiguous-into-paged", "paged-into-contiguous"])
@pytest.mark.parametrize("fmt", ["fp32", "fp8"])
def test_resume_in_a_second_model_of_the_same_file(model_dir, fmt, src, dst):
    """the restart case: the image comes back into another model opened from the same file, of the same or of the other cache layout"""
    path, spec = synth_model(model_dir, "tiny-qwen3")
    resume(path, spec, src, dst, kw=FMT_OF[fmt][1])


# ---- 3. the reference's bits through an image -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,quant,gs,mode", [("tiny-qwen3", "q80", 64, "strict"), ("tiny-nano", "f32", 0, "exact")])
def test_reference_bits_through_an_image(model_dir, preset, quant, gs, mode):
    """prefill prompt[:-1] into slot 0, save, overwrite both slots with other tokens, restore into both, teacher-force the golden ids as
    batches of two: BOTH rows carry the compiled reference's logits and greedy ids at every decode step."""
    g = np.load(e2e_golden(preset, quant, gs))
    path, spec = golden_model(model_dir, preset, quant, gs)
    m = nb.load_model_file(path, max_seq_len=int(g["max_seq_len"]), max_batch=2)
    (m.set_strict if mode == "strict" else m.set_exact)(True)
    ids, gl, prompt = g["ids"], g["logits"], g["prompt"]
    n_prompt = len(prompt)
    m.prefill(prompt[:-1], 0, 0)
    img = m.kv_save(0, n_prompt - 1)
    other = mf.prompt_ids(909, len(ids), spec.vocab_size)
    m.prefill(other, 0, 0); m.prefill(other, 0, 1)
    m.kv_restore(0, img); m.kv_restore(1, img)
    for pos in range(n_prompt - 1, len(ids) - 1):
        lg, am = m.forward([int(ids[pos])] * 2, [pos] * 2, want_argmax=True)
        for row in range(2):
            assert np.array_equal(bits(lg[row]), bits(gl[pos - (n_prompt - 1)])), (preset, quant, mode, "pos", pos, "row", row)
            assert int(am[row]) == int(ids[pos + 1])
    m.close()


# ---- 4. prefix restore -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged,fmt", [(False, "fp32"), (True, "fp32"), (True, "fp8"), (False, "fp16")])
def test_prefix_restore_equals_own_ingestion(model_dir, paged, fmt):
    """n' of an image of 129 positions: the slot equals one that was fed n' tokens itself -- rows, and later steps"""
    path, spec = synth_model(model_dir, "tiny-qwen3")
    code, kw = FMT_OF[fmt]
    toks, conts = ids_of(spec, 129), ids_of(spec, 6, seed=404)
    src = load(path, paged, **kw)
    src.prefill(toks, 0, 0)
    img = src.kv_save(0, 129)
    src.close()
    for n in (1, 64, 70):
        a, b = load(path, paged, **kw), load(path, paged, **kw)
        a.prefill(toks[:n], 0, 2)
        b.prefill(ids_of(spec, 140, seed=505), 0, 2)
        b.kv_restore(2, img, n)
        upto = (n + 63) // 64 * 64 if paged else n          # paged: the rest of the last page is zero, as in the slot that ingested; contiguous: rows >= n stay
        for ra, rb in zip(state_rows(a, spec, 2, upto), state_rows(b, spec, 2, upto)):
            assert np.array_equal(bits(ra), bits(rb)), n
        if paged:
            assert not state_rows(b, spec, 2, S)[0][:, n:].any() and b.kv_pages()[0] == (n + 63) // 64
        else:
            assert state_rows(b, spec, 2, n + 1)[0][:, n].any()                                  # the other tokens' row n is still there
        same_bits(steps(a, conts, n, 2), steps(b, conts, n, 2), ("prefix", n))
        a.close(); b.close()


# ---- 5. paged bookkeeping -------------------------------------------------------------------------------------------------------------------
def some_rows(m, spec, slots, positions):
    return [bits(m.read_state(w, spec.kv_dim, s, layer, p)).copy() for s in slots for layer in range(spec.n_layer) for p in positions for w in ("k", "v")]


def test_restore_into_a_slot_that_shares_pages(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3")
    prefix, other, conts = ids_of(spec, 100), ids_of(spec, 70, seed=606), ids_of(spec, 5, seed=707)
    m, und = load(path, True), load(path, True)
    m.prefill(prefix, 0, 0); m.kv_fork(0, 100, [1, 2]); m.prefill(other, 0, 3)
    for s in (0, 2):
        und.prefill(prefix, 0, s)
    for s in (1, 3):
        und.prefill(other, 0, s)
    assert m.kv_pages()[0] == 1 + 3 + 2 and m.kv_sharing() == (1, 0)
    img = m.kv_save(3, 70)
    assert m.kv_pages()[0] == 6 and m.kv_sharing() == (1, 0)                 # save changes nothing
    before = some_rows(m, spec, (0, 2), (0, 63, 64, 99))
    m.kv_restore(1, img)
    # slot 1 left the shared page (two owners remain) and gave its partial page back; it took two pages of its own
    assert m.kv_pages()[0] == 6 - 1 + 2 and m.kv_sharing() == (1, 0)
    for a, b in zip(before, some_rows(m, spec, (0, 2), (0, 63, 64, 99))):
        assert np.array_equal(a, b)
    k1, v1 = state_rows(m, spec, 1, 128)
    assert k1[:, :70].any() and not k1[:, 70:].any() and not v1[:, 70:].any()                  # rows 70 % 64 .. 63 of the last page read as zero
    for t in range(len(conts)):
        pos = [100 + t, 70 + t, 100 + t, 70 + t]
        lm, _ = m.forward([int(conts[t])] * B, pos)
        lu, _ = und.forward([int(conts[t])] * B, pos)
        for s in range(B):
            assert np.array_equal(bits(lm[s]), bits(lu[s])), (t, s)
    for s in range(B):
        m.kv_release(s)
    assert m.kv_pages()[0] == 0 and m.kv_sharing()[0] == 0                   # every page is accounted for
    m.close(); und.close()


def test_restore_on_an_exhausted_pool_changes_nothing(model_dir, monkeypatch):
    path, spec = synth_model(model_dir, "tiny-qwen3")
    big = load(path, False, max_batch=1)
    big.prefill(ids_of(spec, 129), 0, 0)
    img = big.kv_save(0, 129)
    big.close()
    monkeypatch.setenv("NANO_KV_PAGES", "4")
    m, und = load(path, True), load(path, True)
    monkeypatch.delenv("NANO_KV_PAGES")
    prefix, seq = ids_of(spec, 100), ids_of(spec, 20, seed=66)
    for x in (m, und):
        x.prefill(prefix, 0, 0); x.prefill(seq[:10], 0, 1); x.prefill(seq[:10], 0, 2)
    assert m.kv_pages() == (4, 4)
    before = some_rows(m, spec, range(3), (0, 9, 64, 99))
    with pytest.raises(nb.NanoHipError, match="pages") as ei:               # 3 pages wanted; none free, one the slot's own
        m.kv_restore(1, img)
    assert "nano_hip error -4" in str(ei.value)                              # NANO_HIP_ENOMEM
    assert m.kv_pages() == (4, 4) and m.kv_sharing() == (0, 0)
    for a, b in zip(before, some_rows(m, spec, range(3), (0, 9, 64, 99))):
        assert np.array_equal(a, b)
    for t in range(10, 13):
        lm, _ = m.forward([int(prefix[99]), int(seq[t]), int(seq[t])], [99, t, t])
        lu, _ = und.forward([int(prefix[99]), int(seq[t]), int(seq[t])], [99, t, t])
        for s in range(3):
            assert np.array_equal(bits(lm[s]), bits(lu[s])), (t, s)
    m.kv_restore(1, img, 64)                                                  # one page: the slot's own serves it
    assert m.kv_pages() == (4, 4) and m.kv_sharing() == (0, 0)
    und.prefill(ids_of(spec, 64), 0, 1)
    lm, _ = m.forward([int(prefix[99]), 7, int(seq[13])], [99, 63, 13])      # (position 63: no new page for slot 1)
    lu, _ = und.forward([int(prefix[99]), 7, int(seq[13])], [99, 63, 13])
    for s in range(3):
        assert np.array_equal(bits(lm[s]), bits(lu[s])), s
    m.close(); und.close()


def test_save_writes_zeros_for_an_unmapped_block(model_dir):
    path, spec = synth_model(model_dir, "tiny-qwen3")
    mp, mc = load(path, True), load(path, False)
    toks = ids_of(spec, 10)
    mp.prefill(toks, 0, 1); mc.prefill(toks, 0, 1)
    assert mp.kv_pages()[0] == 1
    ip, ic = mp.kv_save(1, 129), mc.kv_save(1, 129)
    assert mp.kv_pages()[0] == 1                                             # saving maps nothing
    _, k, v = kr.read(ip)
    assert k[:, :10].any() and v[:, :10].any() and not k[:, 10:].any() and not v[:, 10:].any()
    assert np.array_equal(ip, ic)                                            # a fresh contiguous cache reads as zero there, too
    mp.close(); mc.close()


# ---- 6. argument errors --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_argument_errors_change_nothing(model_dir, paged):
    path, spec = synth_model(model_dir, "tiny-qwen3")
    path2, spec2 = synth_model(model_dir, "tiny-nano-odd")
    toks = ids_of(spec, 70)
    m, und = load(path, paged), load(path, paged)
    m.prefill(toks, 0, 1); und.prefill(toks, 0, 1)
    img = m.kv_save(1, 70)
    state = (m.kv_pages(), m.kv_sharing()) if paged else None
    f16 = load(path, paged, max_batch=2, kv_f16=True)
    f16.prefill(toks, 0, 1)
    wrong_format = f16.kv_save(1, 70)
    f16.close()
    o = load(path2, paged, max_batch=2)
    o.prefill(ids_of(spec2, 70), 0, 1)
    wrong_dim = o.kv_save(1, 70)
    o.close()
    assert spec2.kv_dim != spec.kv_dim and spec2.n_layer == spec.n_layer
    wrong_tag = img.copy(); wrong_tag[48] ^= 1
    bad_magic = img.copy(); bad_magic[0] ^= 0xff
    reserved = img.copy(); reserved[56] = 1
    for what, image, n_pos in (("format", wrong_format, None), ("kv_dim", wrong_dim, None), ("tag", wrong_tag, None), ("magic", bad_magic, None),
                               ("reserved", reserved, None), ("truncated", img[:-1], None), ("header only", img[:40], None),
                               ("n_pos beyond the image", img, 71)):
        with pytest.raises(nb.NanoHipError) as ei:
            m.kv_restore(1, image, n_pos)
        assert "nano_hip error -1" in str(ei.value), what                     # NANO_HIP_EINVAL
    with pytest.raises(nb.NanoHipError):
        m.kv_restore(B, img)                                                 # slot out of range
    with pytest.raises(nb.NanoHipError):
        m.kv_save(B, 10)
    with pytest.raises(nb.NanoHipError):
        m.kv_save(1, S + 1)                                                  # beyond max_seq_len
    small = load(path, paged, max_batch=2, max_seq_len=64)
    with pytest.raises(nb.NanoHipError, match="max_seq_len"):
        small.kv_restore(1, img)
    small.close()
    L = nb.lib()
    buf, n = np.zeros(img.size, np.uint8), C.c_size_t(0)
    assert L.nano_hip_kv_save(m.h, 1, 70, buf.ctypes.data, img.size - 1, C.byref(n)) == -1 and n.value == img.size     # a short cap still reports the size
    assert not buf.any()
    assert L.nano_hip_kv_save(None, 1, 70, buf.ctypes.data, img.size, C.byref(n)) == -1
    assert L.nano_hip_kv_save(m.h, 1, 70, None, img.size, C.byref(n)) == -1 and L.nano_hip_kv_save(m.h, 1, 70, buf.ctypes.data, img.size, None) == -1
    assert L.nano_hip_kv_restore(None, 1, img.ctypes.data, img.size, 70) == -1 and L.nano_hip_kv_restore(m.h, 1, None, img.size, 70) == -1
    if paged:
        assert (m.kv_pages(), m.kv_sharing()) == state
    assert np.array_equal(m.kv_save(1, 70), img)
    conts = ids_of(spec, 4, seed=808)
    same_bits(steps(und, conts, 70, 1), steps(m, conts, 70, 1), "after refused calls")
    m.close(); und.close()


# ---- 7. the engine, across a restart --------------------------------------------------------------------------------------------------------
def child(mode, path, image, n, n_steps):
    r = subprocess.run([sys.executable, os.path.join(HERE, "kv_image_engine_child.py"), mode, path, image, str(n), str(n_steps)],
                       capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_engine_round_trip_through_another_process(model_dir, tmp_path):
    """nano_kv_save in one process, nano_kv_restore in the next: the continuation after the restore is the uninterrupted one, ids and
    logits; and a context with replicas refuses both calls"""
    path, spec = synth_model(model_dir, "tiny-qwen3")
    image = str(tmp_path / "parked.nkv")
    whole = child("save", path, image, 70, 12)
    assert nb.kv_image_check(np.fromfile(image, np.uint8))["n_pos"] == 70
    resumed = child("resume", path, image, 70, 12)
    assert resumed == whole and len(whole["ids"]) == 12
    e = nb.Engine(path, max_seq_len=S, max_batch=2)
    assert e.kv_image_bytes(70) == os.path.getsize(image)
    e.L.nano_context_replicate.restype = C.c_int
    e.L.nano_context_replicate.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    assert e.L.nano_context_replicate(e.ctx, (C.c_int * 1)(0), 1) == 0, nb.last_error()
    with pytest.raises(nb.NanoHipError):
        e.kv_save(0, 0)
    with pytest.raises(nb.NanoHipError):
        e.kv_restore(0, np.fromfile(image, np.uint8))
    e.close()
