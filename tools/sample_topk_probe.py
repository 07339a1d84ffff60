#!/usr/bin/env python3
"""What top-k truncation costs when it is off and what it buys when it is on: Qwen3-0.6B Q80 gs64, synthetic weights, penalty 1.1, top_p 0.9.

One process, every variant warmed, then REPS rounds in which the variants run one after another (interleaved); medians and ranges:
  seq1    sampled decode of one sequence through the C engine (generate_next_token, NANO_SAMPLE_TOP_K=1 in the environment so that the
          engine passes Sampler.top_k on): tok/s over 16 prompt + N decoded tokens, at temperature 0.05 / top_k 0, 1.0 / top_k 0 and
          1.0 / top_k 20;
  b64     nano_hip_forward_sample_batch[_ex] over 64 slots at staggered positions: ms per step, the same three settings; with the class
          of the rows (LDS sorter or wide phase) and their n_sorted;
  flat    the operator on np.zeros(V) (one histogram bin holds every token: the wide phase with or without top_k): ms per call at
          top_k 0 and 20.
    python tools/sample_topk_probe.py [--reps 5] [--steps 20] [--decode 200] [--out FILE]
    python tools/sample_topk_probe.py --tree OTHER_CHECKOUT      the same from another built checkout of this repository (the parent
          commit: no top_k, so only the top_k 0 variants run)
    python tools/sample_topk_probe.py --against OTHER_CHECKOUT   this tree and the other one in alternating child processes (A B A B)
"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def run(args):
    tree = os.path.abspath(args.tree or ROOT)
    sys.path.insert(0, tree)
    os.environ["NANO_SAMPLE_TOP_K"] = "1"
    import numpy as np
    from nano_amd import binding as nb
    from nano_amd import modelfile as mf
    has_k = hasattr(nb, "NanoHipSampleParamsEx")
    spec = mf.preset("qwen3-0.6b", "q80", group_size=64, block_size=1024)
    path = "/tmp/qwen3-0.6b-q80-64.bin"
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=39)
    V = spec.vocab_size
    settings = [(0.05, 0), (1.0, 0)] + ([(1.0, 20)] if has_k else [])
    name = lambda t, k: f"T{t}/k{k}"
    res = {"tree": tree, "top_k_supported": has_k, "reps": args.reps}

    # seq1: three engines, one per setting
    prompt = mf.prompt_ids(5, 16, V)
    engines = {s: nb.Engine(path, max_seq_len=512, rep_pen=1.1, temperature=s[0], top_p=0.9, top_k=s[1], seed=39) for s in settings}
    for e in engines.values():
        e.generate(prompt, 8)
    seq1 = {s: [] for s in settings}
    for _ in range(args.reps):
        for s, e in engines.items():
            t0 = time.perf_counter()
            e.generate(prompt, args.decode)                               # (every token ends in a stream synchronise)
            seq1[s].append((16 + args.decode) / (time.perf_counter() - t0))
    for e in engines.values():
        e.close()
    res["seq1_tok_per_s"] = {name(*s): med(v) for s, v in seq1.items()}

    # b64: one model, 64 slots at staggered positions
    B = 64
    m = nb.load_model_file(path, max_seq_len=512, max_batch=B)
    rng = np.random.default_rng(7)
    start = [16 + (7 * s) % 64 for s in range(B)]
    prompts = [[int(x) for x in rng.integers(0, V, size=n + 1)] for n in start]
    for s in range(B):
        m.prefill(prompts[s][:-1], 0, s)
    b64 = {s: [] for s in settings}
    rows_seen = {s: {"lds_rows": 0, "wide_rows": 0, "fallback_rows": 0, "n_sorted_max": 0, "nucleus_max": 0} for s in settings}

    def steps(setting, n, timed):
        temp, k = setting
        tok, pos, hist = [p[-1] for p in prompts], list(start), [list(p[:-1]) for p in prompts]
        t0 = time.perf_counter()
        for _ in range(n):
            rows = [(1.1, temp, 0.9, float(rng.random(dtype=np.float32)), hist[s]) for s in range(B)]
            out = m.forward_sample_batch(tok, pos, rows, top_k=k) if k else m.forward_sample_batch(tok, pos, rows)
            for s in range(B):
                hist[s].append(tok[s])
            tok = [int(r.token) for r in out]; pos = [p + 1 for p in pos]
            if timed:
                st = rows_seen[setting]
                st["wide_rows"] += sum(r.n_sorted == r.n_candidates > 8192 for r in out); st["fallback_rows"] += sum(r.status != 0 for r in out)
                st["lds_rows"] += sum(r.status == 0 and not r.n_sorted == r.n_candidates > 8192 for r in out)
                st["n_sorted_max"] = max([st["n_sorted_max"]] + [int(r.n_sorted) for r in out]); st["nucleus_max"] = max([st["nucleus_max"]] + [int(r.nucleus) for r in out])
        return (time.perf_counter() - t0) / n * 1e3
    for s in settings:
        steps(s, 3, False)
    for _ in range(args.reps):
        for s in settings:
            b64[s].append(steps(s, args.steps, True))
    res["b64_ms_per_step"] = {name(*s): med(v) for s, v in b64.items()}
    res["b64_rows"] = {name(*s): v for s, v in rows_seen.items()}

    # flat: the operator on all-equal logits
    flat = np.zeros(V, np.float32)
    ks = [0, 20] if has_k else [0]
    fl = {k: [] for k in ks}
    info = {}
    call = lambda k: m.op_sample(flat, [], 1.1, 1.0, 0.9, 0.37, top_k=k) if k else m.op_sample(flat, [], 1.1, 1.0, 0.9, 0.37)
    for k in ks:
        call(k)
    for _ in range(args.reps):
        for k in ks:
            t0 = time.perf_counter()
            for _i in range(10):
                r = call(k)
            fl[k].append((time.perf_counter() - t0) / 10 * 1e3)
            info[k] = {"status": int(r.status), "token": int(r.token), "n_candidates": int(r.n_candidates), "n_sorted": int(r.n_sorted), "nucleus": int(r.nucleus)}
    res["flat_ms_per_call"] = {f"k{k}": med(v) for k, v in fl.items()}
    res["flat_result"] = {f"k{k}": v for k, v in info.items()}
    m.close()
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--decode", type=int, default=200)
    ap.add_argument("--tree", default="")
    ap.add_argument("--against", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not args.against:
        res = [run(args)]
    else:
        res = []
        for tree in (ROOT, args.against, ROOT, args.against):
            cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--reps", str(args.reps), "--steps", str(args.steps), "--decode", str(args.decode)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, stdin=subprocess.DEVNULL)
            if p.returncode != 0:                                          # (nothing more is started after a failed child)
                sys.exit(f"{tree}: exit {p.returncode}\n{p.stderr[-2000:]}")
            res.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(res[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
