"""GPU tests at BASELINE.json's headline size (Qwen3-0.6B, Q80 gs=64, 151 936-token vocabulary, synthetic weights): the
oracle would need minutes per forward here, so parity is carried by size-independent properties of the path — a batch is
the same as its sequences run alone, batched prefill is the same as token-by-token ingestion, the device arg-max is the
arg-max of the logits the device returns, repeated runs are identical, the device sampler draws the token the oracle's
sampler draws from the same logits — plus C-ABI error behaviour."""
import numpy as np
import pytest

from conftest import synth_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def q3(model_dir):
    path, spec = synth_model(model_dir, "qwen3-0.6b", "q80", 64)
    m = nb.load_model_file(path, max_seq_len=96, max_batch=4)
    yield m, spec
    m.close()


def test_batch_equals_sequences_alone_and_runs_repeat(q3):
    m, spec = q3
    prompts = [mf.prompt_ids(s, 6, spec.vocab_size) for s in (1, 2, 3, 4)]
    alone = []
    for pr in prompts:
        for p in range(5):
            m.forward([int(pr[p])], [p], want_logits=False)
        alone.append(m.decode_greedy([int(pr[5])], [5], 24)[:, 0].copy())
    for rep in range(2):                                   # twice: identical again (graph replays, KV rows rewritten)
        for p in range(5):
            m.forward([int(pr[p]) for pr in prompts], [p] * 4, want_logits=False)
        got = m.decode_greedy([int(pr[5]) for pr in prompts], [5] * 4, 24)
        for b in range(4):
            assert np.array_equal(got[:, b], alone[b]), (rep, b)


def test_prefill_equals_token_by_token(q3):
    m, spec = q3
    pr = mf.prompt_ids(9, 70, spec.vocab_size)             # 64-token MFMA chunk + a 5-token remainder
    for p in range(69):
        m.forward([int(pr[p])], [p], want_logits=False)
    want_logits, _ = m.forward([int(pr[69])], [69])
    want_ids = m.decode_greedy([int(pr[69])], [69], 12)[:, 0].copy()
    m.prefill(pr[:69], 0, 0)
    got_logits, am = m.forward([int(pr[69])], [69], want_argmax=True)
    got_ids = m.decode_greedy([int(pr[69])], [69], 12)[:, 0]
    assert np.array_equal(got_logits.view(np.uint32), want_logits.view(np.uint32))      # same KV rows -> same bits
    assert np.array_equal(got_ids, want_ids)
    assert int(am[0]) == int(np.argmax(got_logits[0])) == int(want_ids[0])


def test_device_sampler_at_full_vocabulary(q3, oracle):
    m, spec = q3
    pr = mf.prompt_ids(4, 8, spec.vocab_size)
    ids = [int(x) for x in pr]
    for p in range(7):
        m.forward([ids[p]], [p], want_logits=False)
    rng = np.random.default_rng(8)
    on_device = 0
    for p in range(7, 30):
        coin = float(rng.random(dtype=np.float32))
        temp = 0.04 if p % 3 else 0.0                      # 0.04: the random-weight logits become as peaked as a trained model's
        logits, _ = m.forward([ids[p]], [p])
        want, n_ref = oracle.sample_logits(logits[0], np.array(ids[:p], np.uint32), 1.15, temp, 0.9, coin)
        r = m.forward_sample(ids[p], p, ids[:p], 1.15, temp, 0.9, coin)
        if temp != 0.0:
            assert r.n_candidates == n_ref
        assert r.status == 0, (p, r.n_candidates, r.n_sorted)
        assert r.token == want, (p, r.token, want)
        on_device += 1
        ids.append(int(r.token))
    # temperature 1 on random weights: a near-uniform distribution, the nucleus does not fit the LDS sorter -- the sampler's second phase
    # (sampler_wide.hip, round 5) draws the oracle's token from > 100 000 sorted candidates (rounds 2-4: status 1, the host loops)
    logits, _ = m.forward([ids[29]], [29])
    want, n_ref = oracle.sample_logits(logits[0], np.array(ids[:29], np.uint32), 1.1, 1.0, 0.9, 0.5)
    r = m.forward_sample(ids[29], 29, ids[:29], 1.1, 1.0, 0.9, 0.5)
    assert r.status == 0 and r.n_candidates == n_ref and r.n_sorted == n_ref and n_ref > 100000, (r.status, r.n_candidates, n_ref)
    assert r.token == want, (r.token, want)


def test_c_abi_rejects_bad_arguments(q3):
    m, spec = q3
    with pytest.raises(nb.NanoHipError):
        m.forward([spec.vocab_size], [0])                  # token out of vocabulary
    with pytest.raises(nb.NanoHipError):
        m.forward([1], [96])                               # position == max_seq_len
    with pytest.raises(nb.NanoHipError):
        m.forward([1] * 5, [0] * 5)                        # batch > max_batch
    with pytest.raises(nb.NanoHipError):
        m.decode_greedy([1], [90], 10)                     # runs past max_seq_len
    with pytest.raises(nb.NanoHipError):
        m.forward_sample(1, 0, [spec.vocab_size + 3], 1.1, 1.0, 0.9, 0.5)   # history id out of vocabulary
    lg, _ = m.forward([1], [0])                            # the model is still usable
    assert np.isfinite(lg).all()


# BASELINE.json configs[1..4] at their own size.  The STRICT path is held to every bit of every logit.  The FAST path's bars
# come from the reference itself: tests/golden/interbuild_floor.json holds, per model, how far the reference's own
# Makefile-flag build (-O3 -ffast-math) strays from its strict build on the same teacher-forced run (FP32 1.3e-6, Q80
# 1.4e-2 / 4.7e-2 at 0.6B / 4B, Q4K 0.18: a flipped 8- or 4-bit activation code cascades).
#   tol   free-running drift over the whole context: 2 x that floor (FP32: the north-star's 1e-4);
#   tol1  ONE fast forward on top of the reference's exact KV state: 1 x that floor (FP32: 1e-5).
def _bars():
    import json, os
    from conftest import GOLD
    f = json.load(open(os.path.join(GOLD, "interbuild_floor.json")))
    out = []
    for name, quant, gs in (("nano-168m", "f32", 0), ("qwen3-0.6b", "q80", 64), ("qwen3-0.6b", "q4k", 0), ("qwen3-4b", "q80", 64)):
        fl = f[f"{name}_{quant}"]
        out.append((name, quant, gs, 1e-4 if quant == "f32" else 2.0 * fl, 1e-5 if quant == "f32" else fl))
    return out


FULLSIZE = _bars()


@pytest.mark.parametrize("name,quant,gs,tol,tol1", FULLSIZE)
def test_fullsize_vs_reference_golden(model_dir, name, quant, gs, tol, tol1):
    """The compiled reference's own greedy run on the same synthetic file, from the prompt to the LAST position of the
    context (seq_len 512 for configs[1..3]; tests/golden/fullsize_*.npz, tools/make_golden.py), teacher-forced:
      strict mode   every decode step's logits equal the reference's bit for bit (CRC-32 over all vocab floats) and
                    the arg-max is the reference's greedy token -- positions up to 511 included;
      fast path     strided logits within `tol` * max|logit| at the kept steps (first 16, around every 64-position
                    bucket boundary where the attention split count changes, last 12), arg-max equal wherever the
                    reference's top-2 gap exceeds 4x the measured error; FP32: the on-device greedy loop reproduces
                    the reference's ids to the end of the context;
      one forward   the fast path's last-position forward on top of the strict run's KV cache (= the reference's,
                    bit for bit) within `tol1`: the deviation one forward adds, free of accumulated drift."""
    import os
    import zlib
    from conftest import GOLD, file_sha256
    if name == "qwen3-4b" and os.environ.get("NANO_SKIP_4B") == "1":
        pytest.skip("NANO_SKIP_4B=1")
    g = np.load(os.path.join(GOLD, f"fullsize_{name}_{quant}.npz"))
    path, spec = synth_model(model_dir, name, quant, gs)
    assert file_sha256(path) == str(g["model_sha256"]), "the synthetic model writer does not reproduce the golden file"
    S = int(g["max_seq_len"])
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    ids, n_prompt, stride = g["ids"], len(g["prompt"]), int(g["stride"])
    n_decode = len(ids) - n_prompt
    assert n_prompt - 1 + n_decode == S                      # the run ends at position S - 1

    # ---- strict mode: bit for bit, every step -----------------------------------------------------------------
    m.set_strict(True)
    m.prefill(ids[:n_prompt - 1], 0)
    for i in range(n_decode):
        pos = n_prompt - 1 + i
        logits, am = m.forward([int(ids[pos])], [pos], want_argmax=True)
        assert zlib.crc32(logits[0].tobytes()) == int(g["crc32"][i]), f"strict logits differ from the reference at position {pos}"
        assert int(am[0]) == int(g["argmax"][i]) == int(ids[pos + 1])
    m.set_strict(False)
    last = n_decode - 1                                       # one fast forward from the reference's exact state (8-split attention at 512)
    logits, _ = m.forward([int(ids[S - 1])], [S - 1])
    one = float(np.abs(logits[0, ::stride].astype(np.float64) - g["logits_strided"][-1]).max()) / float(g["max_abs"][last])

    # ---- fast path: tolerance at the kept steps -----------------------------------------------------------------
    keep = {int(k): j for j, k in enumerate(g["keep"])}
    for pos in range(n_prompt - 1):
        m.forward([int(ids[pos])], [pos], want_logits=False)
    worst, worst_pos, agree, checked = 0.0, -1, 0, 0
    for i in range(n_decode):
        pos = n_prompt - 1 + i
        if i not in keep:
            m.forward([int(ids[pos])], [pos], want_logits=False)
            continue
        logits, am = m.forward([int(ids[pos])], [pos], want_argmax=True)
        err = float(np.abs(logits[0, ::stride].astype(np.float64) - g["logits_strided"][keep[i]]).max())
        if err / float(g["max_abs"][i]) > worst:
            worst, worst_pos = err / float(g["max_abs"][i]), pos
        same = int(am[0]) == int(g["argmax"][i])
        agree += same; checked += 1
        if quant == "f32" or float(g["top2_gap"][i]) > 4.0 * err:
            assert same, (i, int(am[0]), int(g["argmax"][i]))
    for pos in range(n_prompt - 1):
        m.forward([int(ids[pos])], [pos], want_logits=False)
    out = m.decode_greedy([int(ids[n_prompt - 1])], [n_prompt - 1], n_decode)[:, 0]
    m.close()
    n_same = int(np.argmin(np.append(out == ids[n_prompt:], False)))
    print(f"{name}/{quant}: strict == reference bit for bit at all {n_decode} steps (positions {n_prompt - 1}..{S - 1}); fast path: worst "
          f"max|dlogit|/max|logit| over {checked} kept steps = {worst:.3e} (position {worst_pos}), arg-max agrees on {agree}/{checked}, "
          f"free-running greedy ids identical for the first {n_same} of {n_decode} steps; one fast forward from the reference's KV state at "
          f"position {S - 1}: {one:.3e}")
    assert worst < tol and one < tol1
    if quant == "f32":
        assert np.array_equal(out, ids[n_prompt:])


def test_config4_64_prompts_vs_reference_golden(model_dir):
    """BASELINE.json configs[4] as SURVEY 8d specifies it: Qwen3-4B Q80, 64 prompts of 16 ids (seeds 39 .. 102), 128 decode steps each,
    decoded as ONE batch of 64 sequences.  The compiled reference ran four of them alone (seeds 39, 40, 70, 102: the first, the
    second, one from the middle, the last; tests/golden/fullsize64_qwen3-4b_q80.npz, tools/make_golden.py fullsize64):
      strict mode   those four slots reproduce the reference's logits BIT FOR BIT (CRC-32 over the vocabulary) and its greedy ids at
                    every one of the 129 steps (positions 15 .. 143), while the other 60 slots decode their own prompts in the same
                    launches (the reference's matmul_quant order through the batched GEMM kernels, infer/infer.c:654-679, 971-1018);
      fast path     the same batch, the four slots teacher-forced with the reference's ids: strided logits within 2 x the reference's
                    own inter-build floor at the kept steps, arg-max agreement over all 129 steps recorded (profiles/r04_parity.txt)."""
    import os
    import zlib
    from conftest import GOLD, file_sha256
    if os.environ.get("NANO_SKIP_4B") == "1":
        pytest.skip("NANO_SKIP_4B=1")
    g = np.load(os.path.join(GOLD, "fullsize64_qwen3-4b_q80.npz"))
    path, spec = synth_model(model_dir, "qwen3-4b", "q80", 64)
    assert file_sha256(path) == str(g["model_sha256"]), "the synthetic model writer does not reproduce the golden file"
    S, n_prompt, stride = int(g["max_seq_len"]), int(g["n_prompt"]), int(g["stride"])
    seeds = list(range(39, 103))
    B = len(seeds)
    gold = {int(s): seeds.index(int(s)) for s in g["seeds"]}
    prompts = [mf.prompt_ids(s, n_prompt, spec.vocab_size) for s in seeds]
    for s, slot in gold.items():
        assert np.array_equal(prompts[slot], g[f"ids_{s}"][:n_prompt])
    n_decode = S - n_prompt + 1
    keep = {int(k): j for j, k in enumerate(g["keep"])}
    floor = FULLSIZE[3][3]                                        # 2 x the inter-build floor of qwen3-4b/q80
    m = nb.load_model_file(path, max_seq_len=S, max_batch=B)

    def run(strict):
        m.set_strict(strict)
        for p in range(n_prompt - 1):
            m.forward([int(pr[p]) for pr in prompts], [p] * B, want_logits=False)
        cur = [int(pr[n_prompt - 1]) for pr in prompts]
        worst, agree = 0.0, 0
        for i in range(n_decode):
            pos = n_prompt - 1 + i
            logits, am = m.forward(cur, [pos] * B, want_argmax=True)
            nxt = [int(t) for t in am]
            for s, slot in gold.items():
                same = int(am[slot]) == int(g[f"argmax_{s}"][i])
                if strict:
                    assert zlib.crc32(logits[slot].tobytes()) == int(g[f"crc32_{s}"][i]), f"strict logits of seed {s} differ from the reference at position {pos}"
                    assert same and int(am[slot]) == int(g[f"ids_{s}"][pos + 1])
                else:
                    agree += same
                    if i in keep:
                        err = float(np.abs(logits[slot, ::stride].astype(np.float64) - g[f"logits_strided_{s}"][keep[i]]).max())
                        worst = max(worst, err / float(g[f"max_abs_{s}"][i]))
                        if float(g[f"top2_gap_{s}"][i]) > 4.0 * err:
                            assert same, (s, i)
                    nxt[slot] = int(g[f"ids_{s}"][pos + 1])                 # teacher-forced: the reference's own continuation
            cur = nxt
        return worst, agree

    run(True)
    worst, agree = run(False)
    m.close()
    print(f"qwen3-4b/q80, 64 prompts x {n_decode} steps as one batch: strict == reference bit for bit in the 4 reference-run slots at every step "
          f"(positions {n_prompt - 1}..{S - 1}); fast path: worst max|dlogit|/max|logit| over {len(keep)} kept steps x 4 slots = {worst:.3e}, "
          f"arg-max agrees on {agree}/{4 * n_decode} steps")
    assert worst < floor


@pytest.mark.parametrize("quant,gs", [("f32", 0), ("q4k", 0), ("q80", 128)])
def test_nano56m_strict_equals_the_oracle_bit_for_bit(model_dir, oracle, quant, gs):
    """BASELINE.json configs[0]'s model (Nano-56M: hidden size 1408 = 5.5 Q4K blocks, the ONE BASELINE shape that takes the reference's
    partial-block source offset `j*d` end to end, infer/tensor.c:307,339) at its own size on the GPU in strict mode against the plain-C
    oracle (bit-identical to the compiled reference: tests/test_oracle_golden.py) -- a 12-token prompt and 10 greedy steps, every
    logit of every step; the FP32 file is the one `bench.py --model nano-56m --quant f32 --cpu-only` times on the CPU
    (profiles/r05_cfg0_cpu.json).  Fast path recorded next to it."""
    from oracle import binding as ob
    path, spec = synth_model(model_dir, "nano-56m", quant, gs)
    prompt = mf.prompt_ids(39, 12, spec.vocab_size)
    n_decode = 10
    ctx = ob.OracleCtx(oracle, path, max_seq_len=64)
    ids, ref, _ = ctx.generate(prompt, n_decode, want_logits=True)
    ctx.close()
    m = nb.load_model_file(path, max_seq_len=64, max_batch=1)
    worst_fast = 0.0
    for strict in (True, False):
        m.set_strict(strict)
        for pos in range(len(ids) - 1):
            want = pos >= len(prompt) - 1
            logits, amax = m.forward([int(ids[pos])], [pos], want_logits=want, want_argmax=want)
            if not want:
                continue
            r = ref[pos - (len(prompt) - 1)]
            if strict:
                assert np.array_equal(logits[0].view(np.uint32), r.view(np.uint32)), (quant, pos, float(np.abs(logits[0] - r).max()))
                assert int(amax[0]) == int(ids[pos + 1])
            else:
                worst_fast = max(worst_fast, float(np.abs(logits[0] - r).max() / np.abs(r).max()))
    m.close()
    print(f"nano-56m/{quant}: strict == oracle bit for bit over {n_decode} steps; fast path worst {worst_fast:.3e}")
    assert worst_fast <= {"f32": 1e-4, "q80": 5e-2, "q4k": 0.5}[quant]


@pytest.mark.parametrize("preset,quant", [("qwen3-0.6b", "q80"), ("wide-qwen3-2l", "q80"), ("qwen3-0.6b-3l", "q80"), ("qwen3-0.6b", "q4k"), ("qwen3-0.6b-3l", "q4k"),
                                          ("nano-168m", "f32"), ("nano-56m", "f32")])
def test_fused_launches_equal_the_five_launches_per_layer(model_dir, preset, quant):
    """One sequence on Qwen3-0.6B Q80: the q|k|v projection and the attention run as ONE launch (qkv_attn_fused_kernel: the attention
    workgroups take q / k / v from the projection's workgroups as write-through granules inside the launch), and so do Wo and W1|W3
    (wo_w13_fused_kernel: W1|W3's workgroups take the residual stream from Wo's as granules -- an all-gather inside the launch).  Same
    kernel bodies, so every logit of every step -- one split and several (positions beyond 64: Wo combines the partials), eager first use
    and graph replays, the greedy loop -- must be BIT-IDENTICAL whichever of them are on (NANO_FUSE_LAUNCHES bits: 1 q|k|v + attention, 2 Wo + W1|W3;
    values 3 | 0 | 1 | 2, read at model creation: child processes).  wide-qwen3-2l = two layers of Qwen3-4B's shapes: BOTH fused launches
    refuse them (n = 2560 wants more than the four waves fused_shape() takes; Wo + W1|W3 has no form for those wide matrices), so every
    setting issues the five plain launches there -- the parameter pins that the refusal falls back correctly, not a fused kernel;
    qwen3-0.6b-3l = an odd layer count (round 6: the granules carry epoch tags, no buffer pair alternates by layer); Q4K and FP32 / Nano:
    the q|k|v + attention launch of their own kernels (bit 0).  Which form each preset takes: tests/test_fused_launch_plan.py PRESETS, asked
    of the launchers' own planners below; every form on caller inputs: tests/test_gpu_fused_launches.py."""
    import os
    import subprocess
    import sys
    import zlib
    from conftest import ROOT
    path, spec = synth_model(model_dir, preset, quant, 64 if quant == "q80" else 0)     # (Q4K, round 6: the q|k|v + attention launch, bit 0)
    # what is claimed as fused is fused (the planners' answer for this model's shapes; no device needed), and what is not, is not
    from test_fused_launch_plan import PRESETS, preset_forms
    forms = preset_forms(preset, quant)
    assert forms == PRESETS[(preset, quant)], (preset, quant, forms)
    assert (forms[0] is not None) == (preset != "wide-qwen3-2l"), (preset, quant, "q|k|v + attention", forms)
    assert (forms[1] is not None and forms[2] is not None) == (quant == "q80" and preset != "wide-qwen3-2l"), (preset, quant, "Wo + W1|W3", forms)
    code = ("import sys, zlib, numpy as np; sys.path.insert(0, %r)\n"
            "from nano_amd import binding as nb, modelfile as mf\n"
            "m = nb.load_model_file(%r, max_seq_len=256, max_batch=1)\n"
            "ids = mf.prompt_ids(7, 150, %d)\n"
            "crc = 0\n"
            "for pos in range(150):\n"
            "    lg, am = m.forward([int(ids[pos])], [pos], want_logits=True, want_argmax=True)\n"
            "    crc = zlib.crc32(lg.tobytes(), crc)\n"
            "out = m.decode_greedy([int(ids[-1])], [150], 40)\n"
            "print('CRC', crc & 0xffffffff, zlib.crc32(out.tobytes()) & 0xffffffff)\n" % (ROOT, path, spec.vocab_size))
    res = []
    for fuse in ("3", "0", "1", "2"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NANO_FUSE_LAUNCHES=fuse), capture_output=True, text=True, timeout=900)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CRC")]
        assert r.returncode == 0 and lines, r.stderr[-2000:]
        res.append(lines[-1])
    assert len(set(res)) == 1, res
