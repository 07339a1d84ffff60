#!/usr/bin/env python3
"""Greedy decode with lookup drafts (nano_hip_decode_lookup) against nano_hip_decode_greedy, same box, same process, interleaved, medians
of repeated windows.  SYNTHETIC weights (seeded random; nothing here says anything about text): two models per preset bracket what a
real one can do --
  ceiling  Wo and W2 zeroed: the next id depends on the last id only, the sequence falls into a loop and every draft is accepted;
  floor    the free-running random model: failed drafts are pure cost -- where its ids do not fall into a loop of their own (the stats beside
           every figure say how many drafts were accepted: read them before calling a run a floor).
Per preset, at positions near --starts: ms per plain step of the loop (one host wait per step), ms per K-row verify step
(K = 4, 8, 16; from the ceiling run's wall time and step counts), their ratio r(K) = the ids a verify step must emit to break even,
tok/s of both entries with the stats beside them, D = 0 against decode_greedy (the price of the host wait), and the verify chunk replayed as
a graph against queued eagerly (NANO_LOOKUP_GRAPH=0).  Writes profiles/lookup_decode.txt (or --out)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nano_amd import binding as nb      # noqa: E402
from nano_amd import modelfile as mf    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--presets", default="qwen3-0.6b,qwen3-4b")
ap.add_argument("--starts", default="100,400")
ap.add_argument("--new", type=int, default=192)
ap.add_argument("--seq", type=int, default=640)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_decode.txt"))
args = ap.parse_args()
S, N, R = args.seq, args.new, args.reps
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def write(preset, zero):
    spec = mf.preset(preset, "q80", group_size=64)
    path = os.path.join(tempfile.gettempdir(), f"lookup_probe_{preset}_{int(zero)}.bin")
    if not os.path.exists(path):
        lay = mf.write_model(path, spec, seed=39)
        if zero:
            raw = np.memmap(path, dtype=np.uint8, mode="r+")
            for name, (off, nbytes) in lay.entries.items():
                if name.split(".")[0] in ("wo", "w2"):
                    raw[lay.params_offset + off: lay.params_offset + off + nbytes] = 0
            raw.flush(); del raw
    return path, spec


def window(m, prompt, fn):
    """the slot re-fed with the prompt (not timed), then fn() timed up to its own last wait"""
    m.prefill(prompt[:-1]); m.sync()
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def med(v):
    return statistics.median(v)


say(f"# tools/lookup_probe.py -- Q80 group size 64, SYNTHETIC weights, max_seq_len {S}, {N} new ids per window, medians of {R} interleaved windows, one MI355X")
for preset in args.presets.split(","):
    for kind, zero in (("ceiling (Wo, W2 zeroed: periodic ids)", True), ("floor (free-running random model)", False)):
        path, spec = write(preset, zero)
        os.environ["NANO_LOOKUP_GRAPH"] = "1"
        m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
        os.environ["NANO_LOOKUP_GRAPH"] = "0"
        me = nb.load_model_file(path, max_seq_len=S, max_batch=1) if zero else None     # the eager form beside it (the switch is read on the first lookup call)
        if me is not None:
            me.prefill([1, 2]); me.decode_lookup([1, 2, 3], 1)
        os.environ.pop("NANO_LOOKUP_GRAPH")
        say(f"\n## {preset} -- {kind}")
        for start in (int(s) for s in args.starts.split(",")):
            prompt = mf.prompt_ids(1000 + start, start + 1, spec.vocab_size)
            last, p0 = [int(prompt[-1])], [start]
            legs = {"greedy": lambda: m.decode_greedy(last, p0, N)[:, 0], "D=0": lambda: m.decode_lookup(prompt, N, max_draft=0)}
            for K in (4, 8, 16):
                legs[f"K={K}"] = (lambda K=K: m.decode_lookup(prompt, N, max_draft=K - 1))
                if me is not None:
                    legs[f"K={K} eager"] = (lambda K=K: me.decode_lookup(prompt, N, max_draft=K - 1))
            for name, fn in legs.items():                                   # warm: graphs captured, scratch allocated
                window(me if name.endswith("eager") else m, prompt, fn)
            t = {k: [] for k in legs}
            out = {}
            for _ in range(R):
                for name, fn in legs.items():
                    dt, out[name] = window(me if name.endswith("eager") else m, prompt, fn)
                    t[name].append(dt)
            g = out["greedy"]
            tg, t0 = med(t["greedy"]), med(t["D=0"])
            assert np.array_equal(out["D=0"][0], g)
            plain = t0 / N
            say(f"positions {start} .. {start + N - 1}: decode_greedy {N / tg:8.1f} tok/s ({tg / N * 1e3:.4f} ms/step, min .. max {min(t['greedy']) / N * 1e3:.4f} .. {max(t['greedy']) / N * 1e3:.4f})")
            say(f"    D=0 (plain steps of the loop, one host wait each) {N / t0:8.1f} tok/s ({plain * 1e3:.4f} ms/step): {t0 / tg:.3f} x decode_greedy's time")
            for name in legs:
                if not name.startswith("K="):
                    continue
                ids, st = out[name]
                same = np.array_equal(ids, g)
                tm = med(t[name])
                line = f"    {name:11s} {N / tm:8.1f} tok/s = {tg / tm:.3f} x decode_greedy   ids equal: {same}   {st}"
                if st["steps_verify"]:
                    tv = (tm - st["steps_plain"] * plain) / st["steps_verify"]
                    line += f"   verify step {tv * 1e3:.4f} ms, r(K) = {tv / plain:.2f}, emitted per verify step {(st['emitted'] - st['steps_plain']) / st['steps_verify']:.2f}"
                say(line)
        m.close()
        if me is not None:
            me.close()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
