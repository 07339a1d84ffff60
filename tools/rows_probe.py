#!/usr/bin/env python3
"""Ragged steps (nano_hip_step_rows) against what a caller had before: one nano_hip_prefill per prompt, and a decode step plus a
prefill for a prompt that joins running sequences.  One process, A and B alternated `reps` times per workload, medians and ranges.
usage: rows_probe.py [quant = q80] [model = qwen3-0.6b] [reps = 5] [workloads = all | comma list of 64x15,64x100,mixed,join]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from nano_amd import binding as nb
from nano_amd import modelfile as mf

quant = sys.argv[1] if len(sys.argv) > 1 else "q80"
model = sys.argv[2] if len(sys.argv) > 2 else "qwen3-0.6b"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
which = sys.argv[4].split(",") if len(sys.argv) > 4 and sys.argv[4] != "all" else ["64x15", "64x100", "mixed", "join"]
spec = mf.preset(model, quant, group_size=64 if quant == "q80" else 0, block_size=1024)
path = f"/tmp/{model}-{quant}-64.bin"
if not os.path.exists(path):
    print(f"writing {path}", flush=True)
    mf.write_model(path, spec, seed=39)
B = 64
m = nb.load_model_file(path, max_seq_len=256, max_batch=B)
print(f"{model} {quant}: {B} slots, {m.prefill_chunk_tokens()} rows per pass", flush=True)


def timed(fn):
    m.sync(); t0 = time.perf_counter(); fn(); m.sync()
    return (time.perf_counter() - t0) * 1e3


def report(name, rows, ta, tb, what_a, what_b):
    ma, mb = statistics.median(ta), statistics.median(tb)
    print(f"{name}: {rows} rows   A {what_a}: median {ma:.2f} ms (range {min(ta):.2f} .. {max(ta):.2f})   B {what_b}: median {mb:.2f} ms "
          f"(range {min(tb):.2f} .. {max(tb):.2f})   A / B = x{ma / mb:.2f}   ranges {'apart' if max(tb) < min(ta) else 'OVERLAP'}", flush=True)


def prompts_workload(name, lengths):
    prompts = [mf.prompt_ids(100 + i, n, spec.vocab_size) for i, n in enumerate(lengths)]
    segs = [(i, 0, len(p)) for i, p in enumerate(prompts)]
    toks = np.concatenate(prompts)
    passes = nb.rows_plan(segs, m.prefill_chunk_tokens(), 256)[3]

    def a():
        for i, p in enumerate(prompts):
            m.prefill(p, 0, i)

    def b():
        m.step_rows(segs, toks)
    a(); b()                                                       # warm: code objects, scratch, graphs of full chunks
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a)); tb.append(timed(b))
    report(name, len(toks), ta, tb, f"{len(prompts)} x prefill", f"one step_rows ({passes} passes)")


def join_workload():
    """8 running sequences take a decode step while a newcomer's 56-row prompt piece arrives"""
    run = [mf.prompt_ids(300 + i, 40, spec.vocab_size) for i in range(8)]
    new = mf.prompt_ids(399, 56, spec.vocab_size)
    for i, p in enumerate(run):
        m.prefill(p[:-1], 0, i)
    toks8, pos8 = [int(p[-1]) for p in run], [39] * 8
    segs = [(i, 39, 1) for i in range(8)] + [(8, 0, 56)]
    toks = np.concatenate([np.array(toks8, np.uint32), new])

    def a():
        m.forward(toks8, pos8, want_logits=False, want_argmax=True)
        m.prefill(new, 0, 8)

    def b():
        m.step_rows(segs, toks, want_argmax=True)
    a(); b()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a)); tb.append(timed(b))
    report("8 decode rows + a 56-row prompt piece", 64, ta, tb, "forward of 8 + prefill of 56", "one step_rows with every row's arg-max")


if "64x15" in which:
    prompts_workload("64 prompts x 15 tokens", [15] * 64)
if "64x100" in which:
    prompts_workload("64 prompts x 100 tokens", [100] * 64)
if "mixed" in which:
    prompts_workload("64 prompts of mixed lengths 1 .. 120", [1 + (37 * i) % 120 for i in range(64)])
if "join" in which:
    join_workload()
m.close()
