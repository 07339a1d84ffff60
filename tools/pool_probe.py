#!/usr/bin/env python3
"""Text embeddings (nano_hip_step_rows_pool) against what a fed row costs without them.  One process, the four arms of a segment set
alternated `reps` times, medians and ranges:
  (a) step_rows_pool, LAST and MEAN      (b) step_rows with every row's arg-max: what a row costs today (the classifier runs)
  (c) step_rows without outputs: the passes alone, stopped in front of the classifier -- the floor
The pool's own cost is (a) - (c), the saving over today (b) - (a).  Synthetic weights; the numbers are wall time of whole calls.
usage: pool_probe.py [quant = q80] [model = qwen3-0.6b] [reps = 5] [out = profiles/pool_rows.txt]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from nano_amd import binding as nb
from nano_amd import modelfile as mf

quant = sys.argv[1] if len(sys.argv) > 1 else "q80"
model = sys.argv[2] if len(sys.argv) > 2 else "qwen3-0.6b"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "pool_rows.txt")
spec = mf.preset(model, quant, group_size=64 if quant == "q80" else 0, block_size=1024)
path = f"/tmp/{model}-{quant}-64.bin"
if not os.path.exists(path):
    print(f"writing {path}", flush=True)
    mf.write_model(path, spec, seed=39)
B, S = 64, 512
m = nb.load_model_file(path, max_seq_len=S, max_batch=B)
lines = [f"# tools/pool_probe.py {quant} {model} {reps}: {nb.device_info(0)['arch']}, {B} slots, max_seq_len {S}, {m.prefill_chunk_tokens()} rows per pass, "
         f"n_embd {spec.n_embd}; wall ms of whole calls, medians of {reps} (range), arms alternated in one process"]
print(lines[0], flush=True)


def timed(fn):
    m.sync(); t0 = time.perf_counter(); fn(); m.sync()
    return (time.perf_counter() - t0) * 1e3


def workload(name, lengths):
    texts = [mf.prompt_ids(100 + i, n, spec.vocab_size) for i, n in enumerate(lengths)]
    segs = [(i, 0, len(t)) for i, t in enumerate(texts)]
    toks = np.concatenate(texts)
    passes = nb.rows_plan(segs, m.prefill_chunk_tokens(), S)[3]
    arms = {"pool LAST": lambda: m.step_rows_pool(segs, toks, "last", True, 0), "pool MEAN": lambda: m.step_rows_pool(segs, toks, "mean", True, 0),
            "arg-maxes": lambda: m.step_rows(segs, toks, want_argmax=True), "no outputs": lambda: m.step_rows(segs, toks)}
    for fn in arms.values():
        fn()                                                       # warm: code objects, scratch
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    lines.append(f"{name}: {len(toks)} rows, {passes} passes")
    for k, v in t.items():
        lines.append(f"    {k:<10} median {med[k]:8.3f} ms   (range {min(v):.3f} .. {max(v):.3f})")
    for k in ("pool LAST", "pool MEAN"):
        lines.append(f"    {k}: own cost (a) - (c) = {1e3 * (med[k] - med['no outputs']):+.1f} us = {1e3 * (med[k] - med['no outputs']) / passes:+.2f} us per pass;  "
                     f"saving over arg-maxes (b) - (a) = {med['arg-maxes'] - med[k]:+.3f} ms = {100 * (med['arg-maxes'] - med[k]) / med['arg-maxes']:+.1f} %")
    print("\n".join(lines[-8:]), flush=True)


workload("64 texts x 15 tokens", [15] * 64)
workload("64 texts x 100 tokens", [100] * 64)
workload("1 text x 448 tokens", [448])
m.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
