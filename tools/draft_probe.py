#!/usr/bin/env python3
"""Greedy decode with a draft model (nano_hip_decode_draft) against nano_hip_decode_greedy and nano_hip_decode_lookup, same box, same
process, interleaved, medians of repeated windows.  SYNTHETIC weights (seeded random; nothing here says anything about text) at Qwen3-4B
Q80 shapes for the target and Qwen3-0.6B Q80 shapes for the draft.  Both ends of what a draft can do are observable:
  fully accepted   the draft is a second handle on the target's own file: every draft is accepted -- and the draft costs a whole target
                   step per drafted id, so this end OVERSTATES the draft's cost (a real draft is the smaller model);
  failing          the draft is an unrelated random model: nearly every draft fails, the round buys one id.
(a) the cost of a round at D = 2, 4, 8 in ms and in plain target steps, split into catch-up | draft steps | stage + chunk + accept from
    timing events around the three parts (NANO_DRAFT_TIMING=1), and the accepted count at which a round breaks even;
(b) tok/s at the fully accepted end (4B target with a 4B-file draft; 0.6B target with a 0.6B-file draft) against decode_greedy and the
    lookup loop on the same ids;
(c) tok/s at the failing end (0.6B-shape draft for the 4B-shape target).
Writes profiles/draft_decode.txt (or --out)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["NANO_DRAFT_TIMING"] = "1"
from nano_amd import binding as nb      # noqa: E402
from nano_amd import modelfile as mf    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--target", default="qwen3-4b")
ap.add_argument("--draft", default="qwen3-0.6b")
ap.add_argument("--starts", default="100,400")
ap.add_argument("--new", type=int, default=192)
ap.add_argument("--seq", type=int, default=640)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draft_decode.txt"))
args = ap.parse_args()
S, N, R = args.seq, args.new, args.reps
DS = (2, 4, 8)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def write(preset, seed):
    spec = mf.preset(preset, "q80", group_size=64)
    path = os.path.join(tempfile.gettempdir(), f"draft_probe_{preset}_{seed}.bin")
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=seed)
    return path, spec


def load(path):
    return nb.load_model_file(path, max_seq_len=S, max_batch=1)


def med(v):
    return statistics.median(v)


L = nb.lib()
L.nano_hip_draft_phase_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]


def phases(t):
    ms, n = (C.c_double * 3)(), C.c_uint32(0)
    nb.check(L.nano_hip_draft_phase_ms(t.h, ms, C.byref(n)))
    return list(ms), n.value


def window(t, prompt, fn):
    """the target's slot re-fed with the prompt (not timed), then fn() timed up to its own last wait"""
    t.prefill(prompt[:-1]); t.sync()
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def measure(title, t, drafts, spec, lookup):
    """drafts: {label: draft handle}.  Every leg runs on the same target handle, interleaved."""
    say(f"\n## {title}")
    for start in (int(s) for s in args.starts.split(",")):
        prompt = mf.prompt_ids(1000 + start, start + 1, spec.vocab_size)
        last, p0 = [int(prompt[-1])], [start]
        legs = {"greedy": lambda: t.decode_greedy(last, p0, N)[:, 0]}
        if lookup:
            legs["lookup K=8"] = lambda: t.decode_lookup(prompt, N, max_draft=7)
        for label, d in drafts.items():
            for D in DS:
                # the draft holds the prompt from the warm-up window on: draft_held says so, the window times decode, not ingestion
                legs[f"{label} D={D}"] = (lambda d=d, D=D: t.decode_draft(d, prompt, N, max_draft=D, draft_held=start))
        for label, d in drafts.items():
            d.prefill(prompt[:-1]); d.sync()
        for name, fn in legs.items():                                       # warm: graphs captured, scratch allocated
            window(t, prompt, fn)
        phases(t)
        tm = {k: [] for k in legs}
        ph = {k: [0.0, 0.0, 0.0, 0] for k in legs}
        out = {}
        for _ in range(R):
            for name, fn in legs.items():
                dt, out[name] = window(t, prompt, fn)
                tm[name].append(dt)
                ms, n = phases(t)
                for i in range(3):
                    ph[name][i] += ms[i]
                ph[name][3] += n
        g = out["greedy"]
        tg = med(tm["greedy"])
        plain = tg / N * 1e3
        say(f"positions {start} .. {start + N - 1}: decode_greedy {N / tg:8.1f} tok/s ({plain:.4f} ms/step, min .. max {min(tm['greedy']) / N * 1e3:.4f} .. {max(tm['greedy']) / N * 1e3:.4f})")
        for name in legs:
            if name == "greedy":
                continue
            ids, st = out[name]
            tw = med(tm[name])
            line = f"    {name:22s} {N / tw:8.1f} tok/s = {tg / tw:.3f} x decode_greedy   ids equal: {np.array_equal(ids, g)}   {st}"
            say(line)
            if ph[name][3]:
                c, dd, v = (ph[name][i] / ph[name][3] for i in range(3))
                rounds = st["rounds_plain"] + st["rounds_verify"]
                wall = (tw * 1e3 - st["rounds_plain"] * plain) / max(st["rounds_verify"], 1)      # host gaps included; plain rounds at decode_greedy's step (they also wait once)
                say(f"        per drafted round: catch-up {c:.4f} + draft steps {dd:.4f} + stage, chunk, accept {v:.4f} = {c + dd + v:.4f} ms on the device "
                    f"({(c + dd + v) / plain:.2f} plain steps); wall {wall:.4f} ms ({wall / plain:.2f} plain steps) over {rounds} rounds; "
                    f"breaks even at {max(wall / plain - 1.0, 0.0):.2f} accepted ids per round; emitted per drafted round {(st['emitted'] - st['rounds_plain']) / max(st['rounds_verify'], 1):.2f}")


say(f"# tools/draft_probe.py -- Q80 group size 64, SYNTHETIC weights, max_seq_len {S}, {N} new ids per window, medians of {R} interleaved windows, one MI355X")
say("# the draft holds the prompt before a window starts (draft_held): the windows time decode rounds, not the draft's prompt ingestion")
tpath, tspec = write(args.target, 39)
dpath, dspec = write(args.draft, 39)
assert tspec.vocab_size == dspec.vocab_size
t = load(tpath)
same, small = load(tpath), load(dpath)
measure(f"{args.target} target: draft = a second handle on its own file (every draft accepted; OVERSTATES the draft's cost) | draft = {args.draft} shapes, unrelated weights (failing end)",
        t, {"own-file": same, f"{args.draft}": small}, tspec, lookup=True)
t.close(); same.close()
t = load(dpath)
same = load(dpath)
measure(f"{args.draft} target: draft = a second handle on its own file (every draft accepted; the draft as dear as the target)", t, {"own-file": same}, dspec, lookup=True)
t.close(); same.close(); small.close()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
