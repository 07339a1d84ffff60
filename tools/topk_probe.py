#!/usr/bin/env python3
"""What the top-k alternatives cost, on one MI355X.  Three measurements, each one process with its legs alternated; medians of --rounds
(5) and min .. max.  Appends to profiles/topk_logprobs.txt (or --out).

  --op-run              the dispatches of the operator-level measurement and nothing else: REPS x [score pair, then score pair + top-k
                        at k = 1, 5, 20, 32] on 64 x 151 936 logits -- the command to put behind `rocprofv3 --kernel-trace` in a run of
                        its own;
  --op-trace CSV        reads that run's kernel trace (per-dispatch start / end) and reports the score pair and the two top-k launches
                        per k: the kernels' own time, not the operator's uploads;
  --model               scoring prefill of a 448-token text (prefill_score against prefill_score_topk at k = 20 against one forward
                        with logits per token + numpy argpartition) and decode steps at batch 1 and 64 (forward with arg-max only
                        against forward_topk at k = 20 against forward with logits + numpy), Qwen3-0.6B Q80 shapes, random weights;
  --unchanged           the paths this library must not have moved: a 448-token prefill_score and decode steps at batch 1 and 64 with
                        arg-max only.  Uses nothing newer than nano_hip_prefill_score, so NANO_LIB=<the parent commit's library> runs
                        the same legs: start it alternately with both libraries on one box and compare the medians with the spread."""
import argparse
import csv
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
ap.add_argument("--op-run", action="store_true")
ap.add_argument("--op-trace", default=None)
ap.add_argument("--model", action="store_true")
ap.add_argument("--unchanged", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tokens", type=int, default=448)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--model-dir", default="/tmp")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_logprobs.txt"))
args = ap.parse_args()
R, T, K = args.rounds, args.tokens, args.k
KS, OP_ROWS, OP_V, OP_REPS = (1, 5, 20, 32), 64, 151936, 5

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def stat(v, scale=1e3, unit="ms"):
    return f"median {statistics.median(v) * scale:9.3f} {unit}  (min {min(v) * scale:.3f} .. max {max(v) * scale:.3f})"


def timed(m, fn, reps=1):
    m.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    m.sync()
    return (time.perf_counter() - t0) / reps


def numpy_topk(logits, k):
    """the host's share of the route the entry points replace: the k best of one row, ordered, with their log-probs"""
    part = np.argpartition(-logits, k)[:k]
    order = part[np.argsort(-logits[part], kind="stable")]
    mx = logits.max()
    lse = mx + np.log(np.exp(logits - mx).sum(dtype=np.float32))
    return order, logits[order] - lse


def model(max_batch, S=512):
    spec = mf.preset("qwen3-0.6b", "q80", group_size=64)
    path = os.path.join(args.model_dir, "score-probe-qwen3-0.6b-q80.bin")
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=39)
    return spec, nb.load_model_file(path, max_seq_len=S, max_batch=max_batch)


if args.op_run:
    l = (np.random.default_rng(1).standard_normal((OP_ROWS, OP_V)) * 4.0).astype(np.float32)
    for _ in range(OP_REPS + 1):                               # (the first repetition warms: dropped by --op-trace)
        nb.op_score_rows(l)
        for k in KS:
            nb.op_topk_rows(l, k)
    sys.exit(0)

if args.op_trace:
    rows = list(csv.DictReader(open(args.op_trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    seq = [(next(n for n in ("score_tiles", "score_combine", "topk_tiles", "topk_merge") if n in r["Kernel_Name"]), dur(r))
           for r in rows if any(n in r["Kernel_Name"] for n in ("score_", "topk_"))]
    per = 2 + 4 * len(KS)                                      # dispatches per repetition: the pair alone, then the pair + 2 per k
    assert len(seq) == per * (OP_REPS + 1), (len(seq), per)
    pair, tiles, merge = [], {k: [] for k in KS}, {k: [] for k in KS}
    for rep in range(1, OP_REPS + 1):
        s = seq[rep * per:(rep + 1) * per]
        assert [n for n, _ in s[:2]] == ["score_tiles", "score_combine"]
        pair.append(s[0][1] + s[1][1])
        for i, k in enumerate(KS):
            q = s[2 + 4 * i:6 + 4 * i]
            assert [n for n, _ in q] == ["score_tiles", "score_combine", "topk_tiles", "topk_merge"]
            pair.append(q[0][1] + q[1][1]); tiles[k].append(q[2][1]); merge[k].append(q[3][1])
    med = statistics.median
    say(f"# operator level: {OP_ROWS} x {OP_V} logits, the kernels' own time from a kernel trace (rocprofv3 --kernel-trace), {OP_REPS} repetitions after one warm-up")
    say(f"score pair (score_tiles + score_combine):  median {med(pair):7.2f} us  (min {min(pair):.2f} .. max {max(pair):.2f}; yardstick: 18.1 us, profiles/prefill_score.txt)")
    for k in KS:
        add = [a + b for a, b in zip(tiles[k], merge[k])]
        say(f"top-k k = {k:2d}: topk_tiles {med(tiles[k]):7.2f} us + topk_merge {med(merge[k]):6.2f} us = added {med(add):7.2f} us  "
            f"(min {min(add):.2f} .. max {max(add):.2f});  x{med(add) / med(pair):.2f} of the score pair")

if args.unchanged:
    tag = os.path.basename(os.environ.get("NANO_LIB") or "libnano_mi355x.so")
    spec, m = model(64)
    ids = mf.prompt_ids(7, T + 1, spec.vocab_size)
    b = lambda: m.prefill_score(ids[:T], ids[1:T + 1])
    b(); b()
    tb = [timed(m, b, 5) for _ in range(R)]
    say(f"[{tag}] prefill_score, {T} tokens:           {stat(tb)}")
    for B in (1, 64):
        toks, pos = np.arange(B, dtype=np.uint32) + 11, np.full(B, 40, np.uint32)
        for s in range(B):
            m.prefill(ids[:40], 0, s)
        f = lambda: m.forward(toks, pos, want_logits=False, want_argmax=True)
        f(); f()
        tf = [timed(m, f, 50) for _ in range(R)]
        say(f"[{tag}] forward, arg-max only, batch {B:2d}:       {stat(tf)}")
    m.close()

if args.model:
    spec, m = model(64)
    V = spec.vocab_size
    ids = mf.prompt_ids(7, T + 1, V)
    say(f"# scoring prefill: a {T}-token text, Qwen3-0.6B Q80 shapes (random weights), max_seq_len 512; one process, legs alternated, {R} rounds")
    a = lambda: m.prefill_score(ids[:T], ids[1:T + 1])
    b = lambda: m.prefill_score_topk(ids[:T], K, ids[1:T + 1])

    def c():
        return [numpy_topk(m.forward([int(ids[p])], [p])[0][0], K) for p in range(T)]
    a(); a(); b(); b(); c()
    ta, tb, tc = [], [], []
    for _ in range(R):
        ta.append(timed(m, a, 5)); tb.append(timed(m, b, 5)); tc.append(timed(m, c))
    ma, mb, mc = (statistics.median(v) for v in (ta, tb, tc))
    say(f"(a) prefill_score                          {stat(ta)}")
    say(f"(b) prefill_score_topk, k = {K}             {stat(tb)}")
    say(f"(c) {T} x forward with logits + numpy       {stat(tc)}")
    say(f"(b) - (a) = {(mb - ma) * 1e3:.3f} ms for {(T + 63) // 64} chunks;  (c) / (b) = {mc / mb:.1f} x")
    got = b()[1]
    host = c()
    same = sum(np.array_equal(got["token"][i], host[i][0]) for i in range(T))
    say(f"(b) against (c): the {K} tokens equal at {same} of {T} positions (chunk rows against one-row steps)")
    for B in (1, 64):
        toks, pos = np.arange(B, dtype=np.uint32) + 11, np.full(B, 40, np.uint32)
        for s in range(B):
            m.prefill(ids[:40], 0, s)
        say(f"# decode step, batch {B}, position 40, k = {K}")
        f0 = lambda: m.forward(toks, pos, want_logits=False, want_argmax=True)
        f1 = lambda: m.forward_topk(toks, pos, K)

        def f2():
            lg = m.forward(toks, pos)[0]
            return [numpy_topk(lg[s], K) for s in range(B)]
        for f in (f0, f1, f2):
            f(); f()
        t0, t1, t2 = [], [], []
        for _ in range(R):
            t0.append(timed(m, f0, 20)); t1.append(timed(m, f1, 20)); t2.append(timed(m, f2, 5))
        say(f"forward, arg-max only                      {stat(t0)}")
        say(f"forward_topk                               {stat(t1)}")
        say(f"forward with logits + numpy                {stat(t2)}")
        say(f"forward_topk - arg-max only = {(statistics.median(t1) - statistics.median(t0)) * 1e6:.1f} us;  host route / forward_topk = {statistics.median(t2) / statistics.median(t1):.1f} x")
    m.close()

if lines:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
