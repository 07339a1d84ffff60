#!/usr/bin/env python3
"""The log-probabilities of a text's tokens, three ways, on Qwen3-0.6B shapes (random weights), a 448-token text, max_seq_len 512:
  (a) nano_hip_prefill            -- the prompt ingested, no logits (what scoring adds its cost to);
  (b) nano_hip_prefill_score      -- the same plus the classifier over every row and the row statistics, on the device;
  (c) what there was before       -- one nano_hip_forward per token with the logits copied out, and the statistics in numpy.
One process, every leg warmed once, then --rounds alternations a, b, c, a, b, c ...; medians and min .. max.  Wall clock around calls
that end in a stream synchronisation, and the box's streaming read (nano_hip_membw) to set the statistics kernel's traced time against.
Writes profiles/prefill_score.txt (or --out).

--kernel-run: only leg (b), a few times -- the command to put behind `rocprofv3 --kernel-trace --stats --` in a run of its own.
--baseline-only: only leg (a); uses nothing newer than nano_hip_prefill, so the same script times the parent commit's library."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nano_amd import binding as nb      # noqa: E402
from nano_amd import modelfile as mf    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--quants", default="q80,q4k")
ap.add_argument("--tokens", type=int, default=448)
ap.add_argument("--seq", type=int, default=512)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=5, help="calls per timed window of legs (a) and (b)")
ap.add_argument("--kernel-run", action="store_true")
ap.add_argument("--baseline-only", action="store_true")
ap.add_argument("--model-dir", default="/tmp")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_score.txt"))
args = ap.parse_args()
T, S, R = args.tokens, args.seq, args.rounds

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def stat(v, scale=1e3, unit="ms"):
    return f"median {statistics.median(v) * scale:8.3f} {unit}  (min {min(v) * scale:.3f} .. max {max(v) * scale:.3f})"


def timed(m, fn, reps=1):
    m.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    m.sync()
    return (time.perf_counter() - t0) / reps


def numpy_scores(logits, targets):
    """the host's share of leg (c): float32 log-softmax of the target, arg-max and rank of one row"""
    mx = logits.max()
    lse = mx + np.log(np.exp(logits - mx).sum(dtype=np.float32))
    tl = logits[targets]
    return tl - lse, int(np.argmax(logits)), int((logits > tl).sum())


def leg_c(m, ids):
    out = []
    for p in range(T):
        lg, _ = m.forward([int(ids[p])], [p])
        out.append(numpy_scores(lg[0], int(ids[p + 1])))
    return out


say(f"# tools/score_probe.py -- per-token log-probabilities of a {T}-token text, Qwen3-0.6B shapes (random weights), max_seq_len {S}, one MI355X")
say(f"# one process; every leg warmed once; {R} alternations; (a), (b): mean of {args.reps} calls per window; wall clock + stream synchronisation")
for quant in args.quants.split(","):
    spec = mf.preset("qwen3-0.6b", quant, group_size=64 if quant == "q80" else 0)
    path = os.path.join(args.model_dir, f"score-probe-qwen3-0.6b-{quant}.bin")
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=39)
    ids = mf.prompt_ids(7, T + 1, spec.vocab_size)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1)
    a = lambda: m.prefill(ids[:T])
    if args.baseline_only:
        a(); a()
        ta = [timed(m, a, args.reps) for _ in range(3 * R)]
        say(f"{quant}: (a) prefill                   {stat(ta)}")
        m.close()
        continue
    b = lambda: m.prefill_score(ids[:T], ids[1:T + 1])
    if args.kernel_run:
        for _ in range(4):
            b()
        m.close()
        continue
    a(); a(); b(); b(); leg_c(m, ids)                          # first use allocates, runs eagerly and captures; the second replays
    ta, tb, tc = [], [], []
    for _ in range(R):
        ta.append(timed(m, a, args.reps))
        tb.append(timed(m, b, args.reps))
        tc.append(timed(m, lambda: leg_c(m, ids)))
    ma, mb, mc = (statistics.median(v) for v in (ta, tb, tc))
    say(f"{quant}: (a) prefill                   {stat(ta)}")
    say(f"{quant}: (b) prefill_score             {stat(tb)}")
    say(f"{quant}: (c) {T} x forward + numpy      {stat(tc)}")
    say(f"{quant}: (b) - (a) = {(mb - ma) * 1e3:.3f} ms for {(T + 63) // 64} chunks;  (c) / (b) = {mc / mb:.1f} x;  logits kept on the device: {T * spec.vocab_size * 4 / 1e6:.0f} MB")
    got = b()
    host = leg_c(m, ids)
    same = sum(int(got["argmax"][i]) == host[i][1] and int(got["rank"][i]) == host[i][2] for i in range(T))
    worst = max(abs(float(got["logprob"][i]) - float(host[i][0])) for i in range(T))
    say(f"{quant}: (b) against (c): arg-max and rank equal at {same} of {T} positions, largest |logprob difference| {worst:.2e}")
    m.close()

if not (args.kernel_run or args.baseline_only):
    bw = [nb.membw(0, 1 << 30, 10) for _ in range(3)]
    say(f"streaming read of 1 GiB on this box (nano_hip_membw): {min(bw):.0f} .. {max(bw):.0f} GB/s")

if not args.kernel_run:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
