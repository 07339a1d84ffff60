#!/usr/bin/env python3
"""What logit edits cost when a row has none, and what an edit costs: Qwen3-0.6B Q80 gs64, synthetic weights, temperature 0.7, top_p 0.8,
top_k 20, penalty 1.1.

One process; every variant is warmed, then REPS windows in which the variants run one after another (interleaved, A and B in alternating
order); medians and ranges.
  (a) the unedited path, this library (A) against another build of it (B, --parent-lib: the parent commit's library, loaded into the same
      process through a second copy of the binding):
        seq1   sampled decode of one sequence through the C engine (generate_next_token, NANO_SAMPLE_TOP_K=1): tok/s over 16 prompt +
               N decoded tokens;
        b64    nano_hip_forward_sample_batch_ex over 64 slots at staggered positions: ms per step.
  (b) this library, nano_hip_forward_sample_batch_edit at 1 row and at 64 rows, ms per step: no edit, a table mask (mask_id), a per-call
      mask (19 KB per row going up), 300 bias entries per row; and once per batch size the same constrained step done without the feature:
      nano_hip_forward with logits copied out, the mask applied on the host and a numpy sampler (penalty, temperature, softmax,
      candidates, stable sort, top-k, top-p, draw).
    python tools/logit_edit_probe.py [--parent-lib PATH] [--reps 5] [--steps 20] [--decode 200] [--out FILE]
    NANO_LIB=OTHER_BUILD python tools/logit_edit_probe.py --only-a      part (a) of one build in a process of its own (for alternating processes)
"""
import argparse, importlib.util, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["NANO_SAMPLE_TOP_K"] = "1"
PEN, TEMP, TOP_P, TOP_K = 1.1, 0.7, 0.8, 20


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def second_binding(lib_path):
    """a second copy of nano_amd/binding.py bound to another build of the library"""
    os.environ["NANO_LIB"] = lib_path
    spec = importlib.util.spec_from_file_location("nano_amd.binding_b", os.path.join(ROOT, "nano_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["nano_amd.binding_b"] = mod
    spec.loader.exec_module(mod)
    mod.lib()
    del os.environ["NANO_LIB"]
    return mod


def host_sample(np, l, on, hist, coin):
    """the constrained pick on a host copy of the logits (timing only: numpy's exp, not the pinned libm)"""
    l = np.where(on, l, -np.inf).astype(np.float32)
    ids = np.unique(np.asarray(hist, np.int64))
    l[ids] = l[ids] / np.float32(PEN)
    l = l / np.float32(TEMP)
    e = np.exp(l - l.max())
    p = e / np.cumsum(e, dtype=np.float32)[-1]
    idx = np.nonzero(on & (p >= np.float32((1.0 - TOP_P) / (l.size - 1))))[0]
    order = idx[np.argsort(-p[idx], kind="stable")][:TOP_K]
    cdf = np.cumsum(p[order], dtype=np.float32)
    above = np.nonzero(cdf > np.float32(TOP_P))[0]
    last = int(above[0]) if above.size else order.size - 1
    r = np.float32(coin) * cdf[last]
    above = np.nonzero(cdf[:last + 1] > r)[0]
    return int(order[int(above[0]) if above.size else last])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--decode", type=int, default=200)
    ap.add_argument("--only-a", action="store_true", help="part (a) alone (with NANO_LIB set: another build, a process of its own)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    from nano_amd import binding as nba
    from nano_amd import modelfile as mf
    nba.lib()
    libs = {"A": nba}
    if args.parent_lib:
        libs["B"] = second_binding(os.path.abspath(args.parent_lib))
    spec = mf.preset("qwen3-0.6b", "q80", group_size=64, block_size=1024)
    path = "/tmp/qwen3-0.6b-q80-64.bin"
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=39)
    V = spec.vocab_size
    res = {"reps": args.reps, "steps": args.steps, "decode": args.decode, "settings": {"penalty": PEN, "temperature": TEMP, "top_p": TOP_P, "top_k": TOP_K},
           "B_is": args.parent_lib or None}
    rng = np.random.default_rng(7)
    prompt = mf.prompt_ids(5, 16, V)

    # ---- (a) seq1
    engines = {k: nb.Engine(path, max_seq_len=512, rep_pen=PEN, temperature=TEMP, top_p=TOP_P, top_k=TOP_K, seed=39) for k, nb in libs.items()}
    for e in engines.values():
        e.generate(prompt, 8)
    seq1 = {k: [] for k in libs}
    for w in range(args.reps):
        for k, e in list(engines.items())[::1 if w % 2 == 0 else -1]:           # (A B, B A, A B, ..: neither is always first in its window)
            t0 = time.perf_counter()
            e.generate(prompt, args.decode)
            seq1[k].append((16 + args.decode) / (time.perf_counter() - t0))
    for e in engines.values():
        e.close()
    res["a_seq1_tok_per_s"] = {k: med(v) for k, v in seq1.items()}

    # ---- rows at staggered positions
    def open_rows(nb, B):
        m = nb.load_model_file(path, max_seq_len=512, max_batch=B)
        start = [16 + (7 * s) % 64 for s in range(B)]
        prompts = [[int(x) for x in np.random.default_rng(100 + s).integers(0, V, size=n + 1)] for s, n in enumerate(start)]
        for s in range(B):
            m.prefill(prompts[s][:-1], 0, s)
        return m, start, prompts

    def steps(m, start, prompts, n, edits=None, host_on=None):
        B = len(start)
        tok, pos, hist = [p[-1] for p in prompts], list(start), [list(p[:-1]) for p in prompts]
        t0 = time.perf_counter()
        for _ in range(n):
            coins = [float(rng.random(dtype=np.float32)) for _s in range(B)]
            if host_on is not None:
                lg, _ = m.forward(tok, pos)
                new = [host_sample(np, lg[s], host_on, hist[s], coins[s]) for s in range(B)]
            else:
                rows = [(PEN, TEMP, TOP_P, coins[s], hist[s]) for s in range(B)]
                out = m.forward_sample_batch(tok, pos, rows, top_k=TOP_K, edits=edits) if edits is not None else m.forward_sample_batch(tok, pos, rows, top_k=TOP_K)
                assert all(r.status == 0 for r in out)
                new = [int(r.token) for r in out]
            for s in range(B):
                hist[s].append(tok[s])
            tok = new; pos = [p + 1 for p in pos]
        return (time.perf_counter() - t0) / n * 1e3

    # ---- (a) b64
    rows64 = {k: open_rows(nb, 64) for k, nb in libs.items()}
    for k in libs:
        steps(*rows64[k], 3)
    b64 = {k: [] for k in libs}
    for w in range(args.reps):
        for k in list(libs)[::1 if w % 2 == 0 else -1]:
            b64[k].append(steps(*rows64[k], args.steps))
    res["a_b64_ms_per_step"] = {k: med(v) for k, v in b64.items()}
    for k in libs:
        if k != "A":
            rows64[k][0].close()

    if args.only_a:
        res["lib"] = nba.LIB_PATH
        print(json.dumps(res), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")
        return
    # ---- (b) what an edit costs (this library)
    on = np.random.default_rng(11).random(V) < 0.5
    words = nba.mask_words(on, V)
    btok = np.random.default_rng(12).permutation(V)[:300]
    bval = np.random.default_rng(13).normal(0.0, 2.0, 300).astype(np.float32)
    variants = {"none": None, "table mask": {"mask_id": 1}, "per-call mask": {"allow": words}, "300 bias entries": {"bias": (btok, bval)}}
    res["b_mask"] = {"allowed": int(on.sum()), "mask_bytes_per_row": int(words.nbytes), "bias_entries": 300}
    for B in (1, 64):
        m, start, prompts = rows64["A"] if B == 64 else open_rows(nba, 1)
        m.set_mask_table(words.reshape(1, -1))
        ed = {k: (None if v is None else [v] * B) for k, v in variants.items()}
        for k in variants:
            steps(m, start, prompts, 3, edits=ed[k])
        t = {k: [] for k in variants}
        for _ in range(args.reps):
            for k in variants:
                t[k].append(steps(m, start, prompts, args.steps, edits=ed[k]))
        res[f"b_rows{B}_ms_per_step"] = {k: med(v) for k, v in t.items()}
        steps(m, start, prompts, 2, host_on=on)
        res[f"b_rows{B}_host_edit_ms_per_step"] = steps(m, start, prompts, args.steps, host_on=on)
        m.close()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
