#!/usr/bin/env python3
"""Sampled batched decoding, Qwen3-0.6B Q80 gs64 (the model file tools/sample_decode_probe.py writes): ms per step of
  argmax  the forward with the device arg-max only (greedy: what the batched throughput figures measure);
  device  nano_hip_forward_sample_batch (the forward + every row sampled on the device);
  host    the forward with the logits copied back + the reference's host sampler loops once per row (the oracle's plain-C
          sample_logits: the path callers had before the batched device sampler).
Batches of 1 / 8 / 64 sequences at staggered positions (slot s prefilled to 16 + 7 s mod 64 tokens), repetition penalty 1.1, top_p 0.9,
temperature 0.05 (as peaked as a trained model's logits) and 1.0 (the random model's near-uniform logits: every row's nucleus goes
through the wide phase, one row after another).

    python tools/batch_sample_probe.py [--steps N] [--batches 1,8,64] [--temps 0.05,1.0] [--out FILE]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=4)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--temps", default="0.05,1.0")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from nano_amd import binding as nb
    from nano_amd import modelfile as mf
    from oracle import binding as ob
    spec = mf.preset("qwen3-0.6b", "q80", group_size=64, block_size=1024)
    path = "/tmp/qwen3-0.6b-q80-64.bin"
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=39)
    V = spec.vocab_size
    orc = ob.load_oracle()
    batches = [int(b) for b in args.batches.split(",")]
    m = nb.load_model_file(path, max_seq_len=512, max_batch=max(batches))
    rng = np.random.default_rng(7)
    lines = []

    def emit(rec):
        lines.append(rec); print(json.dumps(rec), flush=True)

    for B in batches:
        start = [16 + (7 * s) % 64 for s in range(B)]
        prompts = [[int(x) for x in rng.integers(0, V, size=n + 1)] for n in start]
        for s in range(B):
            m.prefill(prompts[s][:-1], 0, s)
        for temp in [float(t) for t in args.temps.split(",")]:
            res = {"batch": B, "temperature": temp, "repetition_penalty": 1.1, "top_p": 0.9}

            def fresh():
                return [p[-1] for p in prompts], list(start), [list(p[:-1]) for p in prompts]

            # 1. arg-max only
            tok, pos, _ = fresh()
            for it in range(3 + args.steps):
                if it == 3:
                    t0 = time.perf_counter()
                _, am = m.forward(tok, pos, want_logits=False, want_argmax=True)
                tok = [int(x) for x in am]; pos = [p + 1 for p in pos]
            res["argmax_ms"] = (time.perf_counter() - t0) / args.steps * 1e3
            # 2. the batched device sampler
            tok, pos, hist = fresh()
            n_wide = n_fb = 0
            for it in range(3 + args.steps):
                if it == 3:
                    t0 = time.perf_counter()
                rows = [(1.1, temp, 0.9, float(rng.random(dtype=np.float32)), hist[s]) for s in range(B)]
                out = m.forward_sample_batch(tok, pos, rows)
                for s in range(B):
                    hist[s].append(tok[s])
                tok = [int(r.token) for r in out]; pos = [p + 1 for p in pos]
                if it >= 3:
                    n_wide += sum(r.n_sorted > 8192 for r in out); n_fb += sum(r.status != 0 for r in out)
            res["device_ms"] = (time.perf_counter() - t0) / args.steps * 1e3
            res["wide_rows_per_step"] = n_wide / args.steps
            res["fallback_rows"] = n_fb
            # 3. logits to the host + the host sampler loops per row
            tok, pos, hist = fresh()
            for it in range(1 + args.host_steps):
                if it == 1:
                    t0 = time.perf_counter()
                lg, _ = m.forward(tok, pos, want_logits=True)
                nt = []
                for s in range(B):
                    t, _n = orc.sample_logits(lg[s], np.array(hist[s], np.uint32), 1.1, temp, 0.9, float(rng.random(dtype=np.float32)))
                    nt.append(t); hist[s].append(tok[s])
                tok = nt; pos = [p + 1 for p in pos]
            res["host_ms"] = (time.perf_counter() - t0) / args.host_steps * 1e3
            res["device_over_argmax"] = res["device_ms"] / res["argmax_ms"]
            res["host_over_device"] = res["host_ms"] / res["device_ms"]
            emit(res)
    m.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
