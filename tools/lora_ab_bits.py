#!/usr/bin/env python3
"""Do two builds of the library compute the same bits on the LoRA paths?  One process per build prints a SHA-256 of the output bits per
case; --join puts two such listings side by side with a verdict per line.

  python tools/lora_ab_bits.py --out A.txt                           this tree's library
  NANO_LIB=<another build> python tools/lora_ab_bits.py --out B.txt  (nano_amd/binding.py loads the library NANO_LIB names)
  python tools/lora_ab_bits.py --join B.txt A.txt --out profiles/lora_one_path.txt --append     (no device)

Cases.  Operators: nano_hip_op_lora_qkv on lora_ref.inputs over lora_ref.SHAPES x lora_ref.FORMS (q, kraw and the whole v buffer) and
nano_hip_op_lora_o at 1 and 3 rows.  Models: tiny-nano f32 / q80 / q4k and tiny-nano-odd f32 / q4k with a module of rank 5, alpha 16
attached: the logits of three decode steps of four sequences, a 70-token prefill into slot 1 and the step behind it, a step with the
module switched off and one with it on again, 8 tokens of decode_greedy; then the same again after a module of rank 8 replaced the first."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--append", action="store_true")
ap.add_argument("--join", nargs=2, metavar=("PARENT", "THIS"))
args = ap.parse_args()

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def finish():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if args.join:
    cols = [dict(l.rsplit(None, 1) for l in open(p).read().splitlines() if l and not l.startswith("#")) for p in args.join]
    assert list(cols[0]) == list(cols[1]) and cols[0], "the two listings do not name the same cases"
    say("# tools/lora_ab_bits.py -- SHA-256 (first 16 hex digits) of the output bits per case: the parent build | this build")
    for k in cols[0]:
        say(f"{k:<58} {cols[0][k][:16]}  {cols[1][k][:16]}  {'equal' if cols[0][k] == cols[1][k] else 'DIFFERENT'}")
    n = sum(cols[0][k] != cols[1][k] for k in cols[0])
    say(f"# {len(cols[0])} cases, {n} different")
    finish()
    sys.exit(1 if n else 0)

import numpy as np                      # noqa: E402
import lora_ref as lr                   # noqa: E402
from nano_amd import binding as nb      # noqa: E402
from nano_amd import modelfile as mf    # noqa: E402


def digest(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    say(f"{name:<58} {h.hexdigest()}")


say(f"# library: {os.path.basename(os.environ.get('NANO_LIB') or nb.LIB_PATH)}")
for E, KD, rank, alpha in lr.SHAPES:
    for form in lr.FORMS:
        name, n, pos, S, slots, bstride = form
        I = lr.inputs(E, KD, rank, n)
        rng = np.random.default_rng([E, KD, rank, 9])
        q, k, v = I["q"].copy(), I["k"].copy(), rng.standard_normal((slots * S, KD)).astype(np.float32)
        nb.op_lora_qkv(I["x"], I["w"], [(I[c + "a"], I[c + "b"]) for c in "qkv"], q, k, v, pos, KD=KD, rank=rank, alpha=alpha, S=S, v_bstride=bstride * KD)
        digest(f"op qkv E {E} KD {KD} rank {rank} alpha {alpha} {name}", q, k, v)
    for n in (1, 3):
        I = lr.inputs(E, KD, rank, n)
        o1 = np.zeros((n, E), np.float32)
        nb.op_lora_o(I["xba"], (I["oa"], I["ob"]), o1, rank=rank, alpha=alpha)
        digest(f"op o   E {E} KD {KD} rank {rank} alpha {alpha} nb {n}", o1)

S, T = 256, 70
for preset, quant, gs in (("tiny-nano", "f32", 0), ("tiny-nano", "q80", 32), ("tiny-nano", "q4k", 0), ("tiny-nano-odd", "f32", 0), ("tiny-nano-odd", "q4k", 0)):
    spec = mf.preset(preset, quant, group_size=gs, block_size=S)
    path = f"/tmp/lora-ab-{preset}-{quant}.bin"
    mf.write_model(path, spec, seed=39)
    m = nb.load_model_file(path, max_seq_len=S, max_batch=4)
    for rank, seed in ((5, 13), (8, 14)):                       # the second module replaces the first: other LDS size, graphs dropped
        lpath = f"/tmp/lora-ab-{preset}-{quant}-r{rank}.lora"
        mf.write_lora(lpath, spec, rank=rank, alpha=16, seed=seed)
        m.lora_attach_file(lpath)
        tag = f"{preset} {quant} rank {rank}:"
        ids = mf.prompt_ids(611, T + 16, spec.vocab_size)
        for p in range(3):
            digest(f"{tag} decode step {p} of 4 sequences", m.forward([int(ids[4 * p + b]) for b in range(4)], [p] * 4)[0])
        m.prefill(ids[:T], 0, slot=1)
        digest(f"{tag} step behind a {T}-token prefill into slot 1", m.forward([int(ids[0]), int(ids[T])], [3, T])[0])
        m.lora_enable(False)
        digest(f"{tag} a step with the module off", m.forward([int(ids[1]), int(ids[T + 1])], [4, T + 1])[0])
        m.lora_enable(True)
        digest(f"{tag} a step with the module on again", m.forward([int(ids[2]), int(ids[T + 2])], [5, T + 2])[0])
        digest(f"{tag} decode_greedy of 8 tokens", m.decode_greedy([int(ids[3]), int(ids[T + 3])], [6, T + 3], 8))
    m.close()
finish()
