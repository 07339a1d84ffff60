"""Exact mode (nano_hip_set_exact / NANO_EXACT=1, exact.hip): strict mode's results -- the reference CPU engine's logits, arg-max ids
and sampled tokens, bit for bit, F32 / Q80 / Q4K -- from steps that are captured once and replayed as HIP graphs.  The goldens are the
compiled reference's (tools/make_golden.py); where none exists the mode is held to strict mode field by field."""
import json
import os
import zlib

import numpy as np
import pytest

from conftest import E2E_CASES, GOLD, e2e_golden, file_sha256, synth_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf
from fused_ref import bits

pytestmark = pytest.mark.gpu


# ---- 1. tiny models, every golden case ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,quant,gs", E2E_CASES)
def test_exact_logits_bit_identical_to_reference_golden_and_replayed(model_dir, preset, quant, gs):
    g = np.load(e2e_golden(preset, quant, gs))
    path, spec = synth_model(model_dir, preset, quant, gs)
    m = nb.load_model_file(path, max_seq_len=int(g["max_seq_len"]), max_batch=1)
    m.set_exact(True)
    ids, gl, n_prompt = g["ids"], g["logits"], len(g["prompt"])

    def one_pass():
        got = []
        for pos in range(len(ids) - 1):
            want = pos >= n_prompt - 1
            logits, amax = m.forward([int(ids[pos])], [pos], want_logits=want, want_argmax=want)
            if want:
                ref = gl[pos - (n_prompt - 1)]
                assert np.array_equal(bits(logits[0]), bits(ref)), f"{preset}/{quant} pos {pos}"
                assert int(amax[0]) == int(ids[pos + 1])                   # the reference's greedy token
                got.append(bits(logits[0]).copy())
        return got

    first = one_pass()
    st1 = m.exact_state()
    assert st1["on"] and st1["graphs"] >= 1 and st1["launches_per_step"] > 0
    second = one_pass()
    st2 = m.exact_state()
    assert st2["graphs"] == st1["graphs"]                                  # replays: nothing was captured again
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    m.close()
    print(f"{preset}/{quant}: exact == reference bit for bit over {len(gl)} steps, twice; {st2['graphs']} graphs, {st2['launches_per_step']} launches per step")


# ---- 2. greedy loop and prefill --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,quant,gs", [("tiny-qwen3", "q80", 64), ("tiny-nano-odd", "q4k", 0), ("tiny-nano", "f32", 0)])
def test_exact_greedy_loop_and_prefill(model_dir, preset, quant, gs):
    g = np.load(e2e_golden(preset, quant, gs))
    path, spec = synth_model(model_dir, preset, quant, gs)
    m = nb.load_model_file(path, max_seq_len=int(g["max_seq_len"]), max_batch=1)
    m.set_exact(True)
    prompt = g["prompt"]
    n_decode = len(g["ids"]) - len(prompt)
    for _ in range(2):                                                     # the second round replays both graphs
        m.prefill(prompt[:-1], 0)
        out = m.decode_greedy([int(prompt[-1])], [len(prompt) - 1], n_decode)
        assert np.array_equal(out[:, 0], g["ids"][len(prompt):])
    assert m.exact_state()["graphs"] == 2                                  # MODE_NOCLS (prefill) and MODE_LOOP
    m.close()


# ---- 3. full size ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quant,gs", [("qwen3-0.6b", "q80", 64), ("qwen3-0.6b", "q4k", 0), ("nano-168m", "f32", 0), ("qwen3-4b", "q80", 64)])
def test_exact_fullsize_vs_reference_golden(model_dir, name, quant, gs):
    """Every decode step to position S - 1: CRC-32 of the logits and the arg-max are the compiled reference's; then, from a fresh prefill,
    the free-running on-device greedy loop reproduces the reference's ids to the end of the context."""
    if name == "qwen3-4b" and os.environ.get("NANO_SKIP_4B") == "1":
        pytest.skip("NANO_SKIP_4B=1")
    g = np.load(os.path.join(GOLD, f"fullsize_{name}_{quant}.npz"))
    path, spec = synth_model(model_dir, name, quant, gs)
    assert file_sha256(path) == str(g["model_sha256"]), "the synthetic model writer does not reproduce the golden file"
    S = int(g["max_seq_len"])
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    m.set_exact(True)
    ids, n_prompt = g["ids"], len(g["prompt"])
    n_decode = len(ids) - n_prompt
    assert n_prompt - 1 + n_decode == S
    m.prefill(ids[:n_prompt - 1], 0)
    for i in range(n_decode):
        pos = n_prompt - 1 + i
        logits, am = m.forward([int(ids[pos])], [pos], want_argmax=True)
        assert zlib.crc32(logits[0].tobytes()) == int(g["crc32"][i]), f"exact logits differ from the reference at position {pos}"
        assert int(am[0]) == int(g["argmax"][i]) == int(ids[pos + 1])
    m.prefill(ids[:n_prompt - 1], 0)
    out = m.decode_greedy([int(ids[n_prompt - 1])], [n_prompt - 1], n_decode)[:, 0]
    st = m.exact_state()
    m.close()
    n_same = int(np.argmin(np.append(out == ids[n_prompt:], False)))
    print(f"{name}/{quant}: exact == reference bit for bit at all {n_decode} steps; free-running greedy ids identical for {n_same} of {n_decode}; "
          f"{st['graphs']} graphs, {st['launches_per_step']} launches per step")
    assert np.array_equal(out, ids[n_prompt:])


# ---- 4. batches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,quant,gs,B", [("tiny-qwen3", "q80", 64, 3), ("tiny-qwen3", "q80", 64, 9), ("tiny-nano-odd", "q4k", 0, 3), ("tiny-nano", "f32", 0, 3)])
def test_exact_batch_equals_sequences_alone_ragged(model_dir, preset, quant, gs, B):
    """Sequence b starts b steps late (ragged positions in one step); every sequence's logits are those of running it alone."""
    path, spec = synth_model(model_dir, preset, quant, gs)
    T, S = 7, 16
    seqs = [mf.prompt_ids(500 + b, T, spec.vocab_size) for b in range(B)]
    m1 = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    m1.set_exact(True)
    alone = [[bits(m1.forward([int(s[p])], [p])[0][0]).copy() for p in range(T)] for s in seqs]
    m1.close()
    mb = nb.load_model_file(path, max_seq_len=S, max_batch=B)
    mb.set_exact(True)
    for step in range(T + B - 1):
        pos = [min(max(step - b, 0), T - 1) for b in range(B)]            # (a re-fed position rewrites the same KV row)
        lg, _ = mb.forward([int(seqs[b][pos[b]]) for b in range(B)], pos)
        for b in range(B):
            assert np.array_equal(bits(lg[b]), alone[b][pos[b]]), (step, b)
    assert mb.exact_state()["graphs"] == 1
    mb.close()


def test_exact_config4_reference_slots(model_dir):
    """Qwen3-4B Q80, 64 prompts as ONE batch: the four slots the compiled reference ran reproduce its logits and ids bit for bit."""
    if os.environ.get("NANO_SKIP_4B") == "1":
        pytest.skip("NANO_SKIP_4B=1")
    g = np.load(os.path.join(GOLD, "fullsize64_qwen3-4b_q80.npz"))
    path, spec = synth_model(model_dir, "qwen3-4b", "q80", 64)
    assert file_sha256(path) == str(g["model_sha256"])
    S, n_prompt = int(g["max_seq_len"]), int(g["n_prompt"])
    seeds = list(range(39, 103))
    B = len(seeds)
    gold = {int(s): seeds.index(int(s)) for s in g["seeds"]}
    prompts = [mf.prompt_ids(s, n_prompt, spec.vocab_size) for s in seeds]
    m = nb.load_model_file(path, max_seq_len=S, max_batch=B)
    m.set_exact(True)
    for p in range(n_prompt - 1):
        m.forward([int(pr[p]) for pr in prompts], [p] * B, want_logits=False)
    cur = [int(pr[n_prompt - 1]) for pr in prompts]
    for i in range(S - n_prompt + 1):
        pos = n_prompt - 1 + i
        logits, am = m.forward(cur, [pos] * B, want_argmax=True)
        for s, slot in gold.items():
            assert zlib.crc32(logits[slot].tobytes()) == int(g[f"crc32_{s}"][i]), f"exact logits of seed {s} differ from the reference at position {pos}"
            assert int(am[slot]) == int(g[f"argmax_{s}"][i]) == int(g[f"ids_{s}"][pos + 1])
        cur = [int(t) for t in am]
    m.close()


# ---- 5. exact == strict where no golden exists -----------------------------------------------------------------------------------
SAMPLE_FIELDS = ("token", "status", "n_candidates", "n_sorted", "nucleus", "sum_bits", "walked_chunks")
SAMPLERS = [(1.1, 0.0, 0.9, 0.3), (1.1, 0.05, 0.9, 0.77), (1.1, 1.0, 0.9, 0.5)]       # (penalty, temperature, top_p, coin)


def sample_tuple(r):
    return tuple(int(getattr(r, f)) for f in SAMPLE_FIELDS) + tuple(int(t) for t in r.top)


@pytest.mark.parametrize("preset,quant,gs", [("tiny-qwen3", "q80", 64), ("qwen3-0.6b", "q80", 64)])
def test_exact_sampling_equals_strict_field_by_field(model_dir, preset, quant, gs):
    path, spec = synth_model(model_dir, preset, quant, gs)
    B, T = 3, 6
    seqs = [mf.prompt_ids(900 + b, T, spec.vocab_size) for b in range(B)]

    def run(mode):
        m = nb.load_model_file(path, max_seq_len=16, max_batch=B)
        getattr(m, mode)(True)
        one, batch = [], []
        for p in range(T):
            rp, temp, top_p, coin = SAMPLERS[p % 3]
            one.append(sample_tuple(m.forward_sample(int(seqs[0][p]), p, seqs[0][:p], rp, temp, top_p, coin)))
        for p in range(T):
            rows = [SAMPLERS[(p + b) % 3] + (seqs[b][:p],) for b in range(B)]
            batch.append([sample_tuple(r) for r in m.forward_sample_batch([int(s[p]) for s in seqs], [p] * B, rows)])
        m.close()
        return one, batch

    assert run("set_exact") == run("set_strict")


def test_exact_sort_model_non_causal():
    """is_causal = 0 (seq2seq over all S rows): the known answer, and logits bit-equal to strict mode."""
    from test_oracle_golden import sort_vocab
    exp = json.load(open(os.path.join(GOLD, "sort6_expected.json")))
    path = os.path.join(GOLD, "sort6_model.bin")
    vocab = sort_vocab(open(path, "rb").read()); inv = {v: k for k, v in vocab.items()}
    ids = [vocab[c] for c in exp["input"]]
    S = exp["max_seq_len"]

    def run(mode):
        m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
        getattr(m, mode)(True)
        for _ in range(m.spec.n_layer):                                    # reference infer.c:1379-1384
            for pos in range(S):
                m.forward([ids[pos]], [pos], is_causal=0, want_logits=False)
        out, lgs = [], []
        for pos in range(S):                                               # reference infer.c:1387-1396
            lg, am = m.forward([ids[pos]], [pos], is_causal=0, want_argmax=True)
            out.append(inv[int(am[0])]); lgs.append(bits(lg[0]).copy())
        m.close()
        return "".join(out), lgs

    out_x, lg_x = run("set_exact")
    out_s, lg_s = run("set_strict")
    assert out_x == out_s == exp["output"] == "112225"
    assert all(np.array_equal(a, b) for a, b in zip(lg_x, lg_s))


# ---- 6. the two kernels on crafted inputs ------------------------------------------------------------------------------------------
def vector_families(n, rng):
    g = rng.standard_normal(n).astype(np.float32)
    yield "gaussian", g
    yield "heavy-tailed", rng.standard_cauchy(n).astype(np.float32)
    yield "zero", np.zeros(n, np.float32)
    yield "denormal", (g * np.float32(2.0 ** -72)).astype(np.float32)
    d = g.copy(); d[0] = 1000.0
    yield "dominant-first", d
    d = g.copy(); d[-1] = 1000.0
    yield "dominant-last", d
    yield "sixteenths", (np.round(g * 16) / 16).astype(np.float32)


@pytest.mark.parametrize("n", [32, 48, 128, 768, 1000, 1024, 2560, 5120])
def test_op_exact_rmsnorm_equals_oracle_bits(oracle, n):
    rng = np.random.default_rng(n)
    w = rng.standard_normal(n).astype(np.float32)
    for name, x in vector_families(n, rng):
        assert np.array_equal(bits(nb.op_exact_rmsnorm(x, w)), bits(oracle.rmsnorm(x, w))), (n, name)


def attention_restated(oracle, q, kc, vc, n_head, n_kv_head, hd, rng_len):
    """infer/infer.c:842-879 in float32, every chain in the reference's order (chains run side by side as vectors, never re-associated)."""
    kv_mul = n_head // n_kv_head
    out = np.zeros(n_head * hd, np.float32)
    for h in range(n_head):
        o = (h // kv_mul) * hd
        qh, k, v = q[h * hd:(h + 1) * hd], kc[:rng_len, o:o + hd], vc[:rng_len, o:o + hd]
        score = np.zeros(rng_len, np.float32)
        for i in range(hd):                                                # score += q[i] * k[t][i], i ascending
            score = score + qh[i] * k[:, i]
        score = score / np.sqrt(np.float32(hd))
        att = oracle.softmax(score.astype(np.float32))
        acc = np.zeros(hd, np.float32)
        for t in range(rng_len):                                           # xb[i] += a[t] * v[t][i], t ascending
            acc = acc + att[t] * v[t]
        out[h * hd:(h + 1) * hd] = acc
    return out


ATTN_SHAPES = [(32, 4, 4), (48, 4, 2), (128, 4, 1), (256, 2, 1), (128, 8, 2)]          # (head_dim, n_head, n_kv_head): kv_mul 1, 2, 4, 2, 4


@pytest.mark.parametrize("hd,n_head,n_kv_head", ATTN_SHAPES)
def test_op_exact_attention_equals_restated_reference_bits(oracle, hd, n_head, n_kv_head):
    rng = np.random.default_rng(hd * 100 + n_head)
    kvd = n_kv_head * hd
    for rl in (1, 2, 63, 64, 65, 511, 512, 2049):
        if rl == 2049 and hd not in (48, 128):
            continue                                                       # (the longest range on two shapes: the restatement is host work)
        S = rl + 5
        q = rng.standard_normal(n_head * hd).astype(np.float32)
        kc = rng.standard_normal((S, kvd)).astype(np.float32)
        vc = rng.standard_normal((S, kvd)).astype(np.float32)
        kc[rl:] = 1e30; vc[rl:] = -1e30                                    # garbage beyond the range must not reach the result
        for variant in ("plain", "dominant", "equal"):
            k2 = kc.copy()
            if variant == "dominant":
                k2[rl // 2, :] = np.tile(q[:hd], n_kv_head) * 4.0          # one row's score towers over the rest
            if variant == "equal":
                k2[:rl] = 0.0                                              # all scores equal (zero)
            want = attention_restated(oracle, q, k2, vc, n_head, n_kv_head, hd, rl)
            got = nb.op_exact_attention(q, k2, vc, n_head, n_kv_head, hd, rng=rl)
            assert np.array_equal(bits(got), bits(want)), (hd, rl, variant)
            if rl in (65, 512):                                            # the long-context form: strict mode's three launches
                got = nb.op_exact_attention(q, k2, vc, n_head, n_kv_head, hd, rng=rl, long_form=True)
                assert np.array_equal(bits(got), bits(want)), (hd, rl, variant, "long form")
    # non-causal: all S rows
    S = 70
    q = rng.standard_normal(n_head * hd).astype(np.float32)
    kc = rng.standard_normal((S, kvd)).astype(np.float32); vc = rng.standard_normal((S, kvd)).astype(np.float32)
    want = attention_restated(oracle, q, kc, vc, n_head, n_kv_head, hd, S)
    assert np.array_equal(bits(nb.op_exact_attention(q, kc, vc, n_head, n_kv_head, hd, rng=3, is_causal=False)), bits(want))


# ---- 7. interplay and refusals -----------------------------------------------------------------------------------------------------
def golden_run(m, g):
    ids, n_prompt = g["ids"], len(g["prompt"])
    out = []
    for pos in range(len(ids) - 1):
        want = pos >= n_prompt - 1
        lg, _ = m.forward([int(ids[pos])], [pos], want_logits=want)
        if want:
            out.append(bits(lg[0]).copy())
    return out


def test_exact_interplay_with_strict_hook_env_and_fast_path(model_dir):
    preset, quant, gs = "tiny-qwen3", "q80", 64
    g = np.load(e2e_golden(preset, quant, gs))
    path, spec = synth_model(model_dir, preset, quant, gs)
    S = int(g["max_seq_len"])
    gold = [bits(l) for l in g["logits"]]
    never = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    fast = golden_run(never, g)
    never.close()

    m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    # strict wins: no exact graph is built while both are on
    m.set_exact(True); m.set_strict(True)
    assert all(np.array_equal(a, b) for a, b in zip(golden_run(m, g), gold))
    assert m.exact_state() == {"on": True, "graphs": 0, "launches_per_step": 0}
    m.set_strict(False)
    # a phase hook in exact mode: the reference's observation sequence, unchanged logits, served by the strict step
    seen = []
    m.set_phase_hook(lambda layer, phase: seen.append((layer, phase)))
    lg, _ = m.forward([int(g["ids"][0])], [0])
    m.set_phase_hook(None)
    L = spec.n_layer
    assert seen == [(-1, 1)] + [(l, p) for l in range(L) for p in range(2, 10)] + [(L, 10), (L, 11)]
    assert m.exact_state()["graphs"] == 0
    lg2, _ = m.forward([int(g["ids"][0])], [0])
    assert np.array_equal(bits(lg[0]), bits(lg2[0])) and m.exact_state()["graphs"] == 1
    assert all(np.array_equal(a, b) for a, b in zip(golden_run(m, g), gold))
    # switching the mode off returns the fast path's own bits
    m.set_exact(False)
    assert not m.exact_state()["on"]
    assert all(np.array_equal(a, b) for a, b in zip(golden_run(m, g), fast))
    m.close()

    # NANO_EXACT=1 around model creation: the golden bits with no call to set_exact
    keep = os.environ.get("NANO_EXACT")
    os.environ["NANO_EXACT"] = "1"
    try:
        e = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    finally:
        if keep is None:
            os.environ.pop("NANO_EXACT", None)
        else:
            os.environ["NANO_EXACT"] = keep
    assert e.exact_state()["on"]
    assert all(np.array_equal(a, b) for a, b in zip(golden_run(e, g), gold))
    assert e.exact_state()["graphs"] >= 1
    e.close()


@pytest.mark.parametrize("what", ["lora", "kv_f16", "kv_paged"])
def test_exact_refuses_what_strict_refuses_and_the_model_stays_usable(model_dir, what):
    path, spec = synth_model(model_dir, "tiny-nano", "f32", 0)
    kw = {"kv_f16": True} if what == "kv_f16" else {"kv_paged": True} if what == "kv_paged" else {}
    m = nb.load_model_file(path, max_seq_len=16, max_batch=1, **kw)
    if what == "lora":
        lpath = os.path.join(model_dir, "tiny-nano-lora-exact.bin")
        mf.write_lora(lpath, spec, rank=4, alpha=8, seed=3)
        m.lora_attach_file(lpath)
    ref, _ = m.forward([1], [0])
    m.set_exact(True)
    with pytest.raises(nb.NanoHipError, match="error -1"):                 # NANO_HIP_EINVAL, from the first step
        m.forward([1], [0])
    with pytest.raises(nb.NanoHipError, match="error -1"):
        m.prefill([1, 2], 0)
    with pytest.raises(nb.NanoHipError, match="error -1"):
        m.decode_greedy([1], [0], 2)
    m.set_exact(False)
    lg, _ = m.forward([1], [0])
    assert np.array_equal(bits(lg[0]), bits(ref[0]))
    m.close()


# ---- 8. the C engine under NANO_EXACT=1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sample_tiny-nano_f32_rp13", "sample_tiny-nano_f32_t08p09", "sample_tiny-qwen3_q80_rp13", "sample_tiny-qwen3_q4k_t10p05"])
def test_engine_sampler_ids_under_nano_exact(model_dir, name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    path, spec = synth_model(model_dir, str(g["preset"]), str(g["quant"]), int(g["gs"]))
    keep = os.environ.get("NANO_EXACT")
    os.environ["NANO_EXACT"] = "1"
    try:
        e = nb.Engine(path, max_seq_len=int(g["max_seq_len"]), rep_pen=float(g["rep_pen"]), temperature=float(g["temperature"]),
                      top_p=float(g["top_p"]), top_k=0, seed=int(g["seed"]))
        ids = e.generate(g["prompt"], len(g["ids"]) - len(g["prompt"]))
        e.close()
    finally:
        if keep is None:
            os.environ.pop("NANO_EXACT", None)
        else:
            os.environ["NANO_EXACT"] = keep
    assert np.array_equal(ids, g["ids"])
