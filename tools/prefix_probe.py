#!/usr/bin/env python3
"""One prompt prefix in many slots: ingesting it per slot (the only way before nano_hip_kv_fork) against prefill once + fork, on the
contiguous and on the paged KV cache.  Qwen3-0.6B shapes (random weights), max_seq_len 512, 64 slots, a 448-token prefix; three
alternations of every leg, min .. max.  Writes profiles/prefix_share_probe.txt (or --out).

The baseline leg uses only nano_hip_prefill, so the same script gives the same number on a build without the fork
(--baseline-only stops there)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nano_amd import binding as nb      # noqa: E402
from nano_amd import modelfile as mf    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--quants", default="q80,q4k")
ap.add_argument("--slots", type=int, default=64)
ap.add_argument("--prefix", type=int, default=448)
ap.add_argument("--seq", type=int, default=512)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--baseline-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_share_probe.txt"))
args = ap.parse_args()
N, P, S, R = args.slots, args.prefix, args.seq, args.rounds

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def span(v, unit="ms", scale=1e3, fmt="{:.2f}"):
    return f"{fmt.format(min(v) * scale)} .. {fmt.format(max(v) * scale)} {unit}"


def timed(m, fn):
    m.sync()
    t0 = time.perf_counter()
    fn()
    m.sync()
    return time.perf_counter() - t0


def first_steps(m, ids):
    """the first batched decode step behind the prefix (position P: every slot enters a new block), then the mean of four more"""
    toks = [int(ids[(7 * s) % P]) for s in range(N)]
    t1 = timed(m, lambda: m.forward(toks, [P] * N, want_logits=False, want_argmax=True))
    t0 = time.perf_counter()
    for k in range(1, 5):
        m.forward(toks, [P + k] * N, want_logits=False, want_argmax=True)
    return t1, (time.perf_counter() - t0) / 4


say(f"# tools/prefix_probe.py -- {N} slots behind one {P}-token prefix, Qwen3-0.6B shapes (random weights), max_seq_len {S}, one MI355X")
say(f"# wall clock around the calls + a stream synchronisation (Python driver); {R} alternations of every leg, min .. max")
bw = [nb.membw(0, 1 << 30, 10) for _ in range(R)]
say(f"# nano_hip_membw (streaming read of 1 GiB): {min(bw):.0f} .. {max(bw):.0f} GB/s")
say()
for quant in args.quants.split(","):
    spec = mf.preset("qwen3-0.6b", quant, group_size=64 if quant == "q80" else 0, block_size=1024)
    path = f"/tmp/qwen3-0.6b-{quant}-64.bin"
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=39)
    ids = mf.prompt_ids(5, P, spec.vocab_size)
    moved = (N - 1) * 2 * spec.n_layer * P * spec.kv_dim * 4
    say(f"== {quant} ==")
    # ---- contiguous cache: the baseline, then prefill once + fork ----
    m = nb.load_model_file(path, max_seq_len=S, max_batch=N, kv_paged=False)
    m.prefill(ids, 0, 0); m.forward([1] * N, [0] * N, want_logits=False, want_argmax=True); m.sync()        # warm: code objects, the step's graph
    base, once, fork = [], [], []
    for _ in range(R):
        base.append(timed(m, lambda: [m.prefill(ids, 0, s) for s in range(N)]))
        if args.baseline_only:
            continue
        once.append(timed(m, lambda: m.prefill(ids, 0, 0)))
        fork.append(timed(m, lambda: m.kv_fork(0, P, list(range(1, N)))))
    say(f"baseline, {N} x nano_hip_prefill (contiguous):      {span(base)}")
    if args.baseline_only:
        m.close()
        continue
    both = [a + b for a, b in zip(once, fork)]
    say(f"prefill once + fork, contiguous:                  {span(both)}   (prefill {span(once)}, fork {span(fork)})   x{min(base) / min(both):.1f}")
    rate = [moved / t / 1e9 for t in fork]
    say(f"  the fork wrote {moved / 1e6:.0f} MB ({N - 1} x 2 x {spec.n_layer} x {P} x {spec.kv_dim} x 4) and read 1/{N - 1} of that: {min(rate):.0f} .. {max(rate):.0f} GB/s written"
        f" = {min(rate) / max(bw):.2f} .. {max(rate) / min(bw):.2f} of the streaming-read figure")
    c1, cn = first_steps(m, ids)
    m.close()
    # ---- the same fork with non-temporal stores (NANO_KV_COPY_NT=1: measurement only) ----
    os.environ["NANO_KV_COPY_NT"] = "1"
    m = nb.load_model_file(path, max_seq_len=S, max_batch=N, kv_paged=False)
    os.environ.pop("NANO_KV_COPY_NT")
    m.prefill(ids, 0, 0); m.kv_fork(0, P, list(range(1, N)))
    fork_nt = [timed(m, lambda: m.kv_fork(0, P, list(range(1, N)))) for _ in range(R)]
    say(f"  with non-temporal stores (NANO_KV_COPY_NT=1):   fork {span(fork_nt)}")
    m.close()
    # ---- paged cache: unshared (every slot ingests) and shared (prefill once + fork) ----
    m = nb.load_model_file(path, max_seq_len=S, max_batch=N, kv_paged=True)
    m.prefill(ids, 0, 0); m.forward([1] * N, [0] * N, want_logits=False, want_argmax=True); m.sync()
    pbase, pboth, pfork = [], [], []
    for r in range(R):
        for s in range(N):
            m.kv_release(s)
        pbase.append(timed(m, lambda: [m.prefill(ids, 0, s) for s in range(N)]))
        pages_unshared = m.kv_pages()
        if r == R - 1:
            u1, un = first_steps(m, ids)
        for s in range(N):
            m.kv_release(s)
        t_once = timed(m, lambda: m.prefill(ids, 0, 0))
        t_fork = timed(m, lambda: m.kv_fork(0, P, list(range(1, N))))
        pboth.append(t_once + t_fork); pfork.append(t_fork)
        pages_shared, sharing = m.kv_pages(), m.kv_sharing()
    s1, sn = first_steps(m, ids)
    say(f"baseline, {N} x nano_hip_prefill (paged):           {span(pbase)}   kv_pages {pages_unshared}")
    say(f"prefill once + fork, paged:                       {span(pboth)}   (fork {span(pfork)})   x{min(pbase) / min(pboth):.1f}   kv_pages {pages_shared}, kv_sharing {sharing}")
    say(f"  after the first steps: kv_pages {m.kv_pages()}, kv_sharing {m.kv_sharing()}")
    say(f"first batched decode step behind the prefix ({N} sequences at position {P}; every slot enters block {P // 64}), then the mean of the next four:")
    say(f"  contiguous, forked   {c1 * 1e3:.3f} ms, then {cn * 1e3:.3f} ms")
    say(f"  paged, unshared      {u1 * 1e3:.3f} ms, then {un * 1e3:.3f} ms")
    say(f"  paged, shared        {s1 * 1e3:.3f} ms, then {sn * 1e3:.3f} ms")
    say()
    m.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
