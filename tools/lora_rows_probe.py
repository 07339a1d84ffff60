#!/usr/bin/env python3
"""What the LoRA table costs against one attached module.  Nano-168M shapes, synthetic FP32 weights, max_seq_len 512,
64 KV slots, modules of rank 8.  Four models in one process:
  1. no module;
  2. one module through nano_hip_lora_attach (the same launches, its descriptor in every slot);
  3. a table of one entry, bound to every slot;
  4. a table of 8 entries, bound round-robin.
Per model: a decode step of 8 and of 64 sequences at position 20 (arg-max only; --steps steps per timing, host clock around them and a
stream synchronisation) and a 448-token prefill into slot 0.  The legs are interleaved over the models, every leg warmed first (graphs
captured), medians of --rounds (min .. max).

  python tools/lora_rows_probe.py                      -> profiles/lora_rows.txt (or --out; --append keeps what the file holds)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--preset", default="nano-168m")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rank", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_rows.txt"))
ap.add_argument("--append", action="store_true")
args = ap.parse_args()
S, B, R, PF = 512, 64, args.rounds, 448

from nano_amd import binding as nb      # noqa: E402
from nano_amd import modelfile as mf    # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v, unit=1e3, name="ms"):
    return f"{statistics.median(v) * unit:9.3f} {name} ({min(v) * unit:.3f} .. {max(v) * unit:.3f})"


spec = mf.preset(args.preset, "f32", block_size=S)
path = f"/tmp/{args.preset}-f32-bs{S}.bin"
if not os.path.exists(path):
    mf.write_model(path, spec, seed=39)
lpaths = []
for i in range(8):
    lpaths.append(f"/tmp/{args.preset}-r{args.rank}-{i}.lora")
    mf.write_lora(lpaths[i], spec, rank=args.rank, alpha=16, seed=20 + i)
ids = mf.prompt_ids(5, S, spec.vocab_size)


def model(kind):
    m = nb.load_model_file(path, max_seq_len=S, max_batch=B)
    if kind == "attach":
        m.lora_attach_file(lpaths[0])
    elif kind in ("table1", "table8"):
        n = 1 if kind == "table1" else 8
        for i in range(n):
            m.lora_table_set_file(i, lpaths[i])
        m.lora_bind(list(range(B)), [s % n for s in range(B)])
    return m


KINDS = (("none", "1. no module"), ("attach", "2. one module, nano_hip_lora_attach"), ("table1", "3. table of 1 entry, every slot bound to it"),
         ("table8", "4. table of 8 entries, bound round-robin"))
models = {k: model(k) for k, _ in KINDS}


def step_leg(m, nb_):
    tok, pos = [int(t) for t in ids[:nb_]], [20] * nb_
    m.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        m.forward(tok, pos, want_logits=False, want_argmax=True)
    m.sync()
    return (time.perf_counter() - t0) / args.steps


def prefill_leg(m):
    m.sync()
    t0 = time.perf_counter()
    m.prefill(ids[:PF], 0, 0)
    m.sync()
    return time.perf_counter() - t0


LEGS = (("decode step,  8 sequences", lambda m: step_leg(m, 8)), ("decode step, 64 sequences", lambda m: step_leg(m, 64)),
        (f"prefill of {PF} tokens", prefill_leg))
say(f"# tools/lora_rows_probe.py -- {args.preset} FP32 (synthetic), {spec.n_layer} layers, n_embd {spec.n_embd}, kv_dim {spec.kv_dim}, modules of rank {args.rank}, "
    f"max_seq_len {S}, {B} slots, one MI355X")
say(f"# host clock + a stream synchronisation (Python driver), {args.steps} steps per timing; one process, models interleaved, every leg warmed, medians of {R} (min .. max)")
for name, leg in LEGS:
    t = {k: [] for k, _ in KINDS}
    for k, _ in KINDS:
        leg(models[k]); leg(models[k])                          # warm: the eager first run, the capture, a replay
    for _ in range(R):
        for k, _ in KINDS:
            t[k].append(leg(models[k]))
    say()
    say(f"-- {name} --")
    ref = statistics.median(t["attach"])
    for k, label in KINDS:
        say(f"{label:<46} {med(t[k])}   {statistics.median(t[k]) / ref:6.3f} x configuration 2")
    say(f"configuration 2's own spread: {(max(t['attach']) - min(t['attach'])) / ref * 100:.2f} % of its median;  3 - 2: {(statistics.median(t['table1']) - ref) / ref * 100:+.2f} %;  "
        f"4 - 2: {(statistics.median(t['table8']) - ref) / ref * 100:+.2f} %")
for m in models.values():
    m.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
