#!/usr/bin/env python3
"""Parking a sequence's KV rows in host memory (nano_hip_kv_save / nano_hip_kv_restore) against what a caller pays without it:
ingesting the text again (nano_hip_prefill).  Synthetic weights of Qwen3-0.6B Q80 shapes (--presets adds others), max_seq_len 4096,
n_pos 448 and 4095, FP32 and FP8 rows, contiguous and paged cache.  One process, the legs interleaved, medians of --rounds after a
warm-up of every leg.  Per case: save and restore (host clock around the call; both legs end in a synchronise), the image's bytes, a
pinned-to-device copy of the same byte count and its reverse, plain hipMemcpyAsync through ctypes (the transport's floor: none of this
feature's code),
and nano_hip_prefill of the same n_pos tokens.  Then the staging chunk sizes (NANO_KV_IMAGE_CHUNK_MB) on the 4095-position cases.

  python tools/kv_park_probe.py                      -> profiles/kv_park.txt (or --out)
  NANO_LIB=<a build without KV images> python tools/kv_park_probe.py --prefill-only --out ...   -> that build's prefill legs alone
  rocprofv3 --kernel-trace --output-format csv -d DIR -o k -- python tools/kv_park_probe.py --trace MANIFEST.json   (saves and restores of
                                                     a never-fed cache only: no decode or prefill step runs under the profiler)
  python tools/kv_park_probe.py --read-trace DIR/..._kernel_trace.csv MANIFEST.json          -> the pack / unpack kernel's own time per call"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--presets", default="qwen3-0.6b")
ap.add_argument("--seq", type=int, default=4096)
ap.add_argument("--n-pos", default="448,4095")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--chunks-mb", default="4,16,64,256")
ap.add_argument("--prefill-only", action="store_true")
ap.add_argument("--trace", default="")
ap.add_argument("--read-trace", nargs=2, default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_park.txt"))
args = ap.parse_args()
S, R = args.seq, args.rounds
N_POS = [int(x) for x in args.n_pos.split(",")]
CHUNK_DEFAULT_MB = 16                                      # KVI_CHUNK_BYTES of nano_amd/csrc/backend_kv.hip

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def finish():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if args.read_trace:
    rows = []
    with open(args.read_trace[0]) as f:
        for r in csv.DictReader(f):
            if "kv_image_kernel" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    manifest = json.load(open(args.read_trace[1]))
    assert sum(n for _, n in manifest) == len(rows), (sum(n for _, n in manifest), len(rows))
    say("# the pack / unpack kernel's own time per call: sum over the call's launches, from a rocprofv3 --kernel-trace run of its own")
    at, per = 0, {}
    for label, n in manifest:
        per.setdefault(label, []).append((sum(e - s for s, e in rows[at:at + n]) / 1e3, n))
        at += n
    for label, v in per.items():
        us = [x for x, _ in v]
        say(f"{label:<58} {v[0][1]:>3} launches  median {statistics.median(us):9.1f} us  ({min(us):.1f} .. {max(us):.1f}, {len(us)} calls)")
    finish()
    sys.exit(0)

import numpy as np                      # noqa: E402
from nano_amd import binding as nb      # noqa: E402
from nano_amd import modelfile as mf    # noqa: E402


def timed(m, fn):
    m.sync()
    t0 = time.perf_counter()
    fn()
    m.sync()
    return time.perf_counter() - t0


class Floor:
    """a pinned host buffer and a device buffer of nbytes, and plain hipMemcpyAsync between them (the HIP runtime the library loaded)"""

    def __init__(self, nbytes):
        import ctypes as C
        self.C, self.hip, self.n = C, C.CDLL("libamdhip64.so"), nbytes
        self.host, self.dev = C.c_void_p(), C.c_void_p()
        assert self.hip.hipHostMalloc(C.byref(self.host), C.c_size_t(nbytes), 0) == 0 and self.hip.hipMalloc(C.byref(self.dev), C.c_size_t(nbytes)) == 0
        C.memset(self.host, 1, nbytes)

    def copy(self, to_device):
        dst, src = (self.dev, self.host) if to_device else (self.host, self.dev)
        assert self.hip.hipDeviceSynchronize() == 0
        t0 = time.perf_counter()
        assert self.hip.hipMemcpyAsync(dst, src, self.C.c_size_t(self.n), 1 if to_device else 2, None) == 0 and self.hip.hipDeviceSynchronize() == 0
        return time.perf_counter() - t0

    def close(self):
        self.hip.hipHostFree(self.host); self.hip.hipFree(self.dev)


def med(v):
    return f"{statistics.median(v) * 1e3:8.2f} ms ({min(v) * 1e3:.2f} .. {max(v) * 1e3:.2f})"


def launches(spec, eb, n, chunk_mb):
    stride = 64 * spec.n_layer * 2 * spec.kv_dim * eb
    cb = max(1, min((chunk_mb << 20) // stride, (S + 63) // 64))
    blocks = (n + 63) // 64
    return (blocks + cb - 1) // cb


FMTS = (("fp32", 4, {"kv_fp8": False}), ("fp8", 1, {"kv_fp8": True}))
say(f"# tools/kv_park_probe.py -- a sequence's KV rows to host memory and back, max_seq_len {S}, one MI355X, synthetic weights")
say(f"# host clock around each call + a stream synchronisation (Python driver); one process, legs interleaved, every leg warmed, medians of {R} (min .. max)")
say()
manifest = []
for preset in args.presets.split(","):
    spec = mf.preset(preset, "q80", group_size=64, block_size=S)
    path = f"/tmp/{preset}-q80-64-bs{S}.bin"
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=39)
    ids = mf.prompt_ids(5, S, spec.vocab_size)
    say(f"== {preset} Q80 (gs 64): {spec.n_layer} layers, kv_dim {spec.kv_dim} ==")
    for fmt, eb, kw in FMTS:
        for paged in (False, True):
            m = nb.load_model_file(path, max_seq_len=S, max_batch=2, kv_paged=paged, **kw)
            for n in N_POS:
                label = f"{preset} {fmt} rows, {'paged' if paged else 'contiguous'}, n_pos {n}"
                if args.trace:                                                                   # (no step runs under the profiler: the copies' time does not depend on what the rows hold)
                    nl = launches(spec, eb, n, CHUNK_DEFAULT_MB)
                    for _ in range(R):
                        img = m.kv_save(0, n); m.kv_restore(1, img)
                        manifest += [[label + ", pack", nl], [label + ", unpack", nl]]
                    continue
                t_pf = [timed(m, lambda: m.prefill(ids[:n], 0, 0)) for _ in range(2)]          # fills the slot; warm
                if args.prefill_only:
                    t_pf = [timed(m, lambda: m.prefill(ids[:n], 0, 0)) for _ in range(R)]
                    say(f"{label:<58} nano_hip_prefill {med(t_pf)}   = {n / statistics.median(t_pf) / 1e3:.1f} k tok/s")
                    continue
                nbytes = m.kv_image_bytes(n)
                floor = Floor(nbytes)
                buf = np.zeros(nbytes, np.uint8)                                                 # (touched: the timed saves fault no page in)
                img = m.kv_save(0, n, out=buf); m.kv_restore(1, img)                             # warm: staging buffers, code objects
                floor.copy(True); floor.copy(False)
                t_save, t_rest, t_h2d, t_d2h, t_pf = [], [], [], [], []
                for _ in range(R):
                    t_save.append(timed(m, lambda: m.kv_save(0, n, out=buf)))
                    t_rest.append(timed(m, lambda: m.kv_restore(1, img)))
                    t_h2d.append(floor.copy(True)); t_d2h.append(floor.copy(False))
                    t_pf.append(timed(m, lambda: m.prefill(ids[:n], 0, 0)))
                ms, mr, mp = statistics.median(t_save), statistics.median(t_rest), statistics.median(t_pf)
                say(f"{label}: image {nbytes} bytes ({nbytes / 1e6:.1f} MB)")
                say(f"    save     {med(t_save)}   {nbytes / ms / 1e9:6.1f} GB/s    floor, device -> pinned  {med(t_d2h)}")
                say(f"    restore  {med(t_rest)}   {nbytes / mr / 1e9:6.1f} GB/s    floor, pinned -> device  {med(t_h2d)}")
                say(f"    nano_hip_prefill of the same {n} tokens  {med(t_pf)}   = {n / mp / 1e3:.1f} k tok/s;   restore / prefill = {mr / mp:.2f}")
                floor.close()
            m.close()
    if args.prefill_only or args.trace:
        continue
    say()
    say(f"-- staging chunk size (NANO_KV_IMAGE_CHUNK_MB; the library's constant is {CHUNK_DEFAULT_MB} MiB), contiguous cache, n_pos {max(N_POS)} --")
    n = max(N_POS)
    for fmt, eb, kw in FMTS:
        ms_ = {}
        for mb in [int(x) for x in args.chunks_mb.split(",")]:
            os.environ["NANO_KV_IMAGE_CHUNK_MB"] = str(mb)
            m = nb.load_model_file(path, max_seq_len=S, max_batch=2, kv_paged=False, **kw)
            m.prefill(ids[:n], 0, 0)
            img = m.kv_save(0, n, out=np.zeros(m.kv_image_bytes(n), np.uint8)); m.kv_restore(1, img)
            ms_[mb] = (m, img, [], [])
        os.environ.pop("NANO_KV_IMAGE_CHUNK_MB")
        for _ in range(R):                                                                        # interleaved over the alternatives
            for mb, (m, img, ts, tr) in ms_.items():
                ts.append(timed(m, lambda: m.kv_save(0, n, out=img)))
                tr.append(timed(m, lambda: m.kv_restore(1, img)))
        for mb, (m, img, ts, tr) in ms_.items():
            say(f"{preset} {fmt} rows, chunk {mb:>3} MiB ({launches(spec, eb, n, mb)} chunks): save {med(ts)}   restore {med(tr)}")
            m.close()
    say()

if args.trace:
    with open(args.trace, "w") as f:
        json.dump(manifest, f)
finish()
