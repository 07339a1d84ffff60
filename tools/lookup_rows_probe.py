#!/usr/bin/env python3
"""Lookup drafts for several sequences (nano_hip_decode_lookup_rows) against the two things a caller has without it, same box, same
process, interleaved, medians of repeated windows.  SYNTHETIC weights (seeded random; nothing here says anything about text): two
models bracket what a real one can do --
  looping  Wo and W2 zeroed: the next id depends on the last id only, every sequence falls into a loop and every draft is accepted;
  free     the free-running random model: failed drafts are pure cost -- where its ids do not fall into a loop of their own (the stats
           beside every figure say how many drafts were accepted: read them before calling a run the unfavourable end).
Baselines: (a) nano_hip_decode_greedy with batch B, the graph-replayed loop this entry competes with; (b) B consecutive
nano_hip_decode_lookup calls, each on slot 0 re-fed with its sequence's prompt (the re-feeding is not timed).
Per B and max_draft, near position --start: ms per round and the same as a multiple of (a)'s step, ids emitted per sequence and round,
tok/s of all three, and the break-even acceptance that follows: (a) emits one id per sequence and step, so a round pays once it emits
more ids per live sequence than its time in (a)'s steps.  Writes profiles/lookup_rows.txt (or --out)."""
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
ap.add_argument("--preset", default="qwen3-0.6b")
ap.add_argument("--batches", default="2,4,8")
ap.add_argument("--drafts", default="3,7")
ap.add_argument("--start", type=int, default=100)
ap.add_argument("--new", type=int, default=64)
ap.add_argument("--seq", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_rows.txt"))
args = ap.parse_args()
S, N, R, P0 = args.seq, args.new, args.reps, args.start
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


def med(v):
    return statistics.median(v)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


say(f"# tools/lookup_rows_probe.py -- {args.preset} Q80 group size 64, SYNTHETIC weights, max_seq_len {S}, every sequence {N} new ids from position {P0}, "
    f"medians of {R} interleaved windows, one MI355X")
Bs = [int(b) for b in args.batches.split(",")]
Ds = [int(d) for d in args.drafts.split(",")]
for kind, zero in (("looping (Wo, W2 zeroed: periodic ids, every draft accepted)", True), ("free (free-running random model)", False)):
    path, spec = write(args.preset, zero)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=max(Bs))
    chunk = m.prefill_chunk_tokens()
    say(f"\n## {kind}; a pass holds {chunk} rows")
    for B in Bs:
        prompts = [mf.prompt_ids(1000 + 17 * i, P0 + 1, spec.vocab_size) for i in range(B)]
        slots = list(range(B))
        lasts, pos = [int(p[-1]) for p in prompts], [P0] * B

        def refeed():
            for s, p in enumerate(prompts):
                m.prefill(p[:-1], slot=s)
            m.sync()

        def leg_greedy():
            refeed()
            return timed(lambda: m.decode_greedy(lasts, pos, N))

        def leg_rows(D):
            refeed()
            return timed(lambda: m.decode_lookup_rows(prompts, slots, [N] * B, max_draft=D))

        def leg_single(D):                                                  # (b): one sequence after another in slot 0
            total, outs = 0.0, []
            for p in prompts:
                m.prefill(p[:-1]); m.sync()
                dt, o = timed(lambda: m.decode_lookup(p, N, max_draft=D))
                total += dt; outs.append(o)
            return total, outs

        legs = {"greedy": leg_greedy}
        for D in Ds:
            legs[f"rows D={D}"] = (lambda D=D: leg_rows(D))
            legs[f"single D={D}"] = (lambda D=D: leg_single(D))
        for fn in legs.values():                                            # warm: graphs captured, scratch allocated
            fn()
        t, out = {k: [] for k in legs}, {}
        for _ in range(R):
            for name, fn in legs.items():
                dt, out[name] = fn()
                t[name].append(dt)
        g = out["greedy"]
        tg = med(t["greedy"])
        step = tg / N
        say(f"B = {B}: (a) decode_greedy batch {B}: {B * N / tg:8.1f} tok/s, {step * 1e3:.4f} ms/step (min .. max {min(t['greedy']) / N * 1e3:.4f} .. {max(t['greedy']) / N * 1e3:.4f})")
        for D in Ds:
            ids, st, rounds = out[f"rows D={D}"]
            tr, ts = med(t[f"rows D={D}"]), med(t[f"single D={D}"])
            same = all(np.array_equal(ids[i], g[:, i]) for i in range(B))
            d_eff = min(D, chunk // B - 1)
            seq_rounds = sum(s["steps_plain"] + s["steps_verify"] for s in st)
            per = sum(s["emitted"] for s in st) / max(seq_rounds, 1)
            drafted, accepted = sum(s["drafted"] for s in st), sum(s["accepted"] for s in st)
            say(f"    max_draft {D} (runs {d_eff}): {rounds} rounds, {tr / rounds * 1e3:.4f} ms/round = {tr / rounds / step:.2f} x (a)'s step (min .. max "
                f"{min(t[f'rows D={D}']) / rounds * 1e3:.4f} .. {max(t[f'rows D={D}']) / rounds * 1e3:.4f} ms); {per:.2f} ids per sequence and round "
                f"({accepted} of {drafted} drafted ids accepted); ids equal (a)'s: {same}")
            say(f"        tok/s: rows {B * N / tr:8.1f} = {tg / tr:.3f} x (a) = {ts / tr:.3f} x (b); (b) {B} consecutive decode_lookup calls {B * N / ts:8.1f}; "
                f"break-even: {tr / rounds / step:.2f} ids per sequence and round")
    m.close()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
