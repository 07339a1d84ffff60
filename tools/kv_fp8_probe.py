#!/usr/bin/env python3
"""Decode step time with FP32 / FP16 / FP8 (e4m3) KV rows, one model per format in ONE process, interleaved, medians of 5
(profiles/kv_fp8.txt):
  * Qwen3-4B Q80, 64 sequences, near positions 500 and 4000 (the KV rows' bandwidth rules the attention launch there);
  * Qwen3-0.6B Q80, one sequence, near position 4095 (32 splits).
The three models differ in the attention launch alone (and, for one sequence, in the FP32 model's fused q|k|v + attention launch below
its range limit -- not at these positions), so a difference of step times is a difference of that launch, layers times over.  Also
printed: the cache bytes per position and the load form the attention plan picks for the head shape (w16 = FP16's wide form; FP8 rows
have the narrow form only), asked of the loaded library itself through the decode-attention operator.
Usage: python tools/kv_fp8_probe.py [4b] [0.6b]      (default: both)"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nano_amd import binding as nb      # noqa: E402
from nano_amd import modelfile as mf    # noqa: E402

FORMATS = [("FP32", dict(kv_f16=False, kv_fp8=False), 4), ("FP16", dict(kv_f16=True, kv_fp8=False), 2), ("FP8", dict(kv_f16=False, kv_fp8=True), 1)]
CONFIGS = {"4b": ("qwen3-4b", 64, 4096, (500, 4000), 12), "0.6b": ("qwen3-0.6b", 1, 4096, (4095,), 40)}
ROUNDS = 5


def model_file(name):
    d = os.environ.get("NANO_BENCH_MODEL_DIR", "/tmp")                  # (bench.py's cache of synthetic models)
    spec = mf.preset(name, "q80", group_size=64)
    path = os.path.join(d, f"nano_bench_{name}_q80_gs64.bin")
    if not (os.path.exists(path) and os.path.getsize(path) == mf.param_layout(spec).total_bytes):
        mf.write_model(path + ".tmp", spec, seed=39)
        os.replace(path + ".tmp", path)
    return path, spec


def load_form(spec, fmt):
    """w16 of the plan the library picks for this head shape and format (two sequences, 64 positions: the form depends on neither)"""
    H, KV, hd, S = spec.n_head, spec.n_kv_head, spec.hd, 64
    rng = np.random.default_rng(0)
    dt = {0: np.float32, 1: np.float16, 2: np.uint8}[fmt]
    half = hd // 2
    ang = np.arange(S)[:, None] / 1e6 ** (np.arange(half) * 2 / hd)[None, :]
    r = nb.op_attention_decode(rng.standard_normal((2, H * hd)), rng.standard_normal((2, KV * hd)), [3, 40], np.zeros((2, 1, S, KV * hd), dt),
                               np.zeros((2, 1, S, KV * hd), dt), n_head=H, n_kv_head=KV, hd=hd, n_layer=1, layer=0, S=S, range_hint=S,
                               rope_cos=np.cos(ang), rope_sin=np.sin(ang), rope_qwen3=True, q_norm=np.ones(hd), k_norm=np.ones(hd),
                               vraw=rng.standard_normal((2, KV * hd)) if fmt else None, kv_half=fmt)
    return r["plan"]["w16"]


def main():
    which = [a for a in sys.argv[1:] if a in CONFIGS] or list(CONFIGS)
    print(f"library: {nb.LIB_PATH}")
    for key in which:
        name, B, S, positions, iters = CONFIGS[key]
        path, spec = model_file(name)
        per_pos = {n: 2 * spec.n_layer * spec.kv_dim * esz for n, _, esz in FORMATS}
        print(f"{name} Q80 gs64, {B} sequence(s), max_seq_len {S}, {spec.n_layer} layers, head_dim {spec.hd}, kv_dim {spec.kv_dim}")
        print("  cache bytes per position: " + ", ".join(f"{n} {per_pos[n]}" for n, _, _ in FORMATS))
        print("  load form (w16 of the attention plan): " + ", ".join(f"{n} {load_form(spec, i)}" for i, (n, _, _) in enumerate(FORMATS)))
        models = [(n, nb.load_model_file(path, max_seq_len=S, max_batch=B, **kw)) for n, kw, _ in FORMATS]
        for pos in positions:
            for _, m in models:
                m.time_step(B, pos, 3)                                  # warm: graph capture, first touch of the rows
            t = {n: [] for n, _ in models}
            for _ in range(ROUNDS):
                for n, m in models:                                     # interleaved: one drift hits all three
                    t[n].append(m.time_step(B, pos, iters) * 1e3)
            base = statistics.median(t["FP32"])
            for n, _ in models:
                med = statistics.median(t[n])
                kv_mb = per_pos[n] * (pos + 1) * B / 1e6
                print(f"  pos {pos}: {n:4s} rows {med:8.1f} us/step (min {min(t[n]):.1f} .. max {max(t[n]):.1f}), {B / med * 1e6:8.0f} tok/s, "
                      f"{(med - base) / spec.n_layer:+6.2f} us per layer vs FP32 rows, {kv_mb:7.0f} MB of KV rows read per step", flush=True)
        for _, m in models:
            m.close()


if __name__ == "__main__":
    main()
