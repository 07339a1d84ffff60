"""The split-attention combine in front of Wo with IN-WAVE weights (wo_w13_fused_cw_kernel; gemv_common.h cw_issue / cw_combine) against the
table form it replaces (combine_weights + the 8-slot accumulation), bit for bit, through the operator a step's launch goes through.

nb.op_wo_w13_fused runs ONE fused Wo + W1|W3 launch as a one-sequence step issues it and reports the plan that ran.  The same call is made
twice: as planned (plan word cw = 1) and with the form refused (NANO_COMBINE_WAVE=0 in the environment, which the operators read: cw = 0, the
table form).  Every element of the residual stream Wo leaves and of hb must carry the same bits, for every split count 2 .. 8, at
  * Wo n = 1280, head_dim 64 and 128 (five live waves of eight, 4 | 2 heads per wave; the shape of tests/test_gpu_fused_launches.py's role 3),
  * Wo n = 2048, head_dim 128, n_embd 1024, hidden 2304 (Qwen3-0.6B's forms: rows of two chunks, W1|W3 folded in the wave).
Inputs: random partials with planted -0.0 and denormals and one split whose partial vector is all -0.0; statistics with a dominant split
per head (maxima more than 100 apart: every other split's e underflows to 0) on half of the heads, ordinary ones on the rest.  Every head
has its live splits -- what the attention kernels write for a causal step -- which is the condition under which skipping the splits
beyond attn_nsplit cannot move a bit (the argument stands next to cw_issue; tests/test_wo_combine_wave_order.py restates the schedule
on the CPU, dead tail included).
The table form itself is anchored elsewhere: tests/test_gpu_fused_launches.py compares the fused launch with the two plain launches and
with the oracle on exact inputs -- since this change its role-3 cases run the in-wave form against the plain launches' table form.

Last, a whole model: qwen3-0.6b-3l (three layers of Qwen3-0.6B's shapes) fed 140 positions -- across 64 and 128, where the split count
goes 1 -> 2 -> 3 -- and a greedy run behind them; the logits' CRC and the ids with the in-wave form, with the table form, and with the
fused launches off (the plain launch: in-wave, and the table form) are the same.

The plain launch (a step with the fusion off): nb.op_fused_gemv(kind 1) with attn, the same way -- as planned (the 17th word of
nano_hip_q80_gemv_plan, nb.q80_gemv_plan_cw: 1) and with NANO_COMBINE_WAVE=0 (0) -- at the shapes whose plain launch holds ONE item per
thread, the only ones that take the form there: Wo n = 256 (head_dim 32: one wave of heads, the other wave dead), n = 512 (head_dim 64 and
128, two waves), n = 1024 on four waves (4096 rows), n = 2048 on eight waves (4096 rows: rows of two chunks).  Wo of n = 1280 and of
Qwen3-0.6B's n = 2048 x 1024 rows hold two items per thread on the plain launch and keep the table form (gemv_q80.hip says why): the
query must say so."""
import zlib

import numpy as np
import pytest

from conftest import synth_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf
from fused_ref import bits
from test_gpu_fused_roles import q80_weights

gpu = pytest.mark.gpu

SHAPES = [(1280, 64, 256, 2304), (1280, 128, 256, 2304), (2048, 128, 1024, 2304)]       # (Wo n, head_dim, n_embd, hidden)


def partials(rng, n, n_head, hd, ns):
    part = rng.standard_normal((ns, n)).astype(np.float32)
    flat = part.reshape(-1)
    idx = rng.permutation(flat.size)
    flat[idx[:64]] = np.float32(-0.0)
    flat[idx[64:128]] = np.float32(1e-41) * rng.choice([-1.0, 1.0], 64).astype(np.float32)      # denormals
    part[ns // 2] = np.float32(-0.0)                                                             # a live split that holds -0.0 only
    ml = np.empty((n_head, ns, 2), np.float32)
    ml[..., 0] = rng.normal(0.0, 3.0, (n_head, ns))
    ml[..., 1] = rng.uniform(1.0, 64.0, (n_head, ns))
    for h in range(0, n_head, 2):                                                                # a dominant split: the others' e is 0
        ml[h, :, 0] = -150.0 - 120.0 * rng.permutation(ns)
        ml[h, rng.integers(ns), 0] = 30.0
    return part, ml


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_in_wave_combine_equals_the_table_form(shape, monkeypatch):
    n, hd, E, hidden = shape
    n_head = n // hd
    rng = np.random.default_rng(n + hd + E)
    wo = (*q80_weights(rng, E, n, 64), E)
    w1, w3 = (*q80_weights(rng, hidden, E, 64), hidden), (*q80_weights(rng, hidden, E, 64), hidden)
    nw = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    old = rng.standard_normal(E).astype(np.float32)
    errors = []
    for ns in range(2, 9):
        part, ml = partials(rng, n, n_head, hd, ns)
        attn = (part, ml, n_head, hd)
        monkeypatch.delenv("NANO_COMBINE_WAVE", raising=False)
        new = nb.op_wo_w13_fused(n, wo, w1, w3, old, nw, attn=attn)
        monkeypatch.setenv("NANO_COMBINE_WAVE", "0")
        tab = nb.op_wo_w13_fused(n, wo, w1, w3, old, nw, attn=attn)
        assert new["plan"]["cw"] == 1 and tab["plan"]["cw"] == 0, (ns, new["plan"], tab["plan"])
        assert {k: v for k, v in new["plan"].items() if k not in ("cw", "lds_bytes")} == {k: v for k, v in tab["plan"].items() if k not in ("cw", "lds_bytes")}
        assert new["err"] == 0 and tab["err"] == 0
        assert np.isfinite(tab["x"]).all() and np.isfinite(tab["hb"]).all() and np.count_nonzero(tab["x"] != old) > E // 2, ns
        for name in ("x", "hb"):
            bad = np.flatnonzero(bits(new[name]) != bits(tab[name]))
            print(f"{shape} nsplit {ns} {name}: {bad.size} of {new[name].size} elements differ")
            if bad.size:
                errors.append(f"nsplit {ns}: {name} differs at {bad.size} elements, first {bad[:6]}, worst |d| {np.abs(new[name] - tab[name]).max():.3e}")
    assert not errors, f"{shape}: " + "; ".join(errors)


PLAIN = [(256, 32, 256), (512, 64, 256), (512, 128, 256), (1024, 128, 4096), (2048, 128, 4096)]         # (Wo n, head_dim, n_embd)


@gpu
@pytest.mark.parametrize("shape", PLAIN, ids=lambda s: "-".join(map(str, s)))
def test_plain_launch_in_wave_combine_equals_the_table_form(shape, monkeypatch):
    n, hd, E = shape
    n_head = n // hd
    rng = np.random.default_rng(3 * n + hd + E)
    wo = (*q80_weights(rng, E, n, 64), E)
    old = rng.standard_normal(E).astype(np.float32)
    errors, forms = [], set()
    for ns in range(2, 9):
        part, ml = partials(rng, n, n_head, hd, ns)
        run = lambda: nb.op_fused_gemv(0x80, 1, n, [wo], None, None, gs=64, resid=old[None], attn=(part[None], ml[None], n_head, hd))[0]
        monkeypatch.delenv("NANO_COMBINE_WAVE", raising=False)
        p = nb.q80_gemv_plan(1, n, [E], 1, attn=(n_head, hd, ns))
        assert nb.q80_gemv_plan_cw(1, n, [E], 1, attn=(n_head, hd, ns)) == 1, (shape, ns, p)
        new = run()
        monkeypatch.setenv("NANO_COMBINE_WAVE", "0")
        assert nb.q80_gemv_plan_cw(1, n, [E], 1, attn=(n_head, hd, ns)) == 0 and nb.q80_gemv_plan(1, n, [E], 1, attn=(n_head, hd, ns)) == p
        tab = run()
        forms.add((p["nv"], nb.Q80_VARIANTS[p["variant"]]))
        assert np.isfinite(tab).all() and np.count_nonzero(tab != old) > E // 2, ns
        bad = np.flatnonzero(bits(new) != bits(tab))
        print(f"{shape} nsplit {ns} (nv {p['nv']}, {nb.Q80_VARIANTS[p['variant']]}): {bad.size} of {new.size} elements differ")
        if bad.size:
            errors.append(f"nsplit {ns}: differs at {bad.size} elements, first {bad[:6]}, worst |d| {np.abs(new - tab).max():.3e}")
    assert not errors, f"{shape}: " + "; ".join(errors)
    assert forms == {(1, "wfc2" if n == 2048 else "plain")}, forms


def test_two_items_per_thread_keep_the_table_form(monkeypatch):
    monkeypatch.delenv("NANO_COMBINE_WAVE", raising=False)
    for n, hd, E in ((1280, 64, 256), (1280, 128, 256), (2048, 128, 1024)):
        for ns in range(2, 9):
            assert nb.q80_gemv_plan(1, n, [E], 1, attn=(n // hd, hd, ns))["nv"] == 2 and nb.q80_gemv_plan_cw(1, n, [E], 1, attn=(n // hd, hd, ns)) == 0


@gpu
def test_three_layer_model_across_the_split_boundaries(model_dir, monkeypatch):
    path, spec = synth_model(model_dir, "qwen3-0.6b-3l", "q80", 64)
    assert nb.wo_w13_fused_plan(spec.n_head * spec.head_dim, spec.n_embd, spec.n_hidden, attn=(spec.n_head, spec.head_dim, 2))["cw"] == 1
    ids = mf.prompt_ids(11, 140, spec.vocab_size)
    res = []
    for fuse, wave in (("3", None), ("3", "0"), ("0", None), ("0", "0")):        # (both variables are read when the model is created)
        monkeypatch.setenv("NANO_FUSE_LAUNCHES", fuse)
        if wave is None:
            monkeypatch.delenv("NANO_COMBINE_WAVE", raising=False)
        else:
            monkeypatch.setenv("NANO_COMBINE_WAVE", wave)
        m = nb.load_model_file(path, max_seq_len=192, max_batch=1)
        crc = 0
        for pos in range(140):
            lg, _ = m.forward([int(ids[pos])], [pos], want_logits=True, want_argmax=True)
            crc = zlib.crc32(lg.tobytes(), crc)
        out = m.decode_greedy([int(ids[-1])], [140], 24)
        m.close()
        res.append((crc, zlib.crc32(np.ascontiguousarray(out).tobytes())))
    print("logits crc, ids crc per setting:", res)
    assert len(set(res)) == 1, res
