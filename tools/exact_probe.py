#!/usr/bin/env python3
"""What exact mode costs: ms per decode step and greedy tok/s of the FAST path, EXACT mode (nano_hip_set_exact: the reference's bits,
graph-replayed) and STRICT mode (nano_hip_set_strict: the same bits, eager, one thread per chain), alternated three times in one process
per configuration so that the spread between runs of the same mode is visible next to the differences between the modes.

  configurations   Qwen3-0.6B Q80 gs64 (the bench workload), Qwen3-0.6B Q4K, Nano-168M F32, one sequence; Qwen3-0.6B Q80, 8 sequences
  per mode, round  time_step (device events around `iters` steps) at positions 31, 255, 510; a greedy run over positions 31 .. 510
                   (host clock around decode_greedy + the wait for the device), tok/s = sequences x steps / seconds
  exact mode       launches per step (nano_hip_exact_state) next to it

    python tools/exact_probe.py [--out FILE]            every configuration, each in a child process under its own time limit;
                                                        stops at the first child that fails
    python tools/exact_probe.py --one NAME:QUANT:GS:B   one configuration (what the children run)
    python tools/exact_probe.py --trace                 a few exact steps of Qwen3-0.6B Q80 at position 510 and nothing else: the
                                                        program for `rocprofv3 --kernel-trace --stats -- ...` (per-kernel times)
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("qwen3-0.6b", "q80", 64, 1), ("qwen3-0.6b", "q4k", 0, 1), ("nano-168m", "f32", 0, 1), ("qwen3-0.6b", "q80", 64, 8)]
POSITIONS = (31, 255, 510)
MODES = ("fast", "exact", "strict")


def model_path(name, quant, gs):
    from nano_amd import modelfile as mf
    spec = mf.preset(name, quant, group_size=gs)
    path = f"/tmp/exact_probe_{name}_{quant}_{gs}.bin"
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=39)
    return path, spec


def set_mode(m, mode):
    m.set_strict(mode == "strict")
    m.set_exact(mode == "exact")


def one(name, quant, gs, B, iters, out):
    from nano_amd import binding as nb
    from nano_amd import modelfile as mf
    path, spec = model_path(name, quant, gs)
    S = 512
    m = nb.load_model_file(path, max_seq_len=S, max_batch=B)
    prompts = [mf.prompt_ids(39 + b, 32, spec.vocab_size) for b in range(B)]
    n_steps = 510 - 31 + 1
    for rnd in range(3):
        for mode in MODES:
            set_mode(m, mode)
            rec = {"model": f"{name}/{quant}", "sequences": B, "round": rnd, "mode": mode}
            for pos in POSITIONS:
                rec[f"ms_step_pos{pos}"] = round(m.time_step(B, pos, iters), 4)
            for b in range(B):
                m.prefill(prompts[b][:-1], 0, b)
            m.sync()
            t0 = time.perf_counter()
            m.decode_greedy([int(p[-1]) for p in prompts], [31] * B, n_steps, fetch=False)
            m.sync()
            dt = time.perf_counter() - t0
            rec["greedy_ms_step"] = round(1e3 * dt / n_steps, 4)
            rec["greedy_tok_s"] = round(B * n_steps / dt, 1)
            if mode == "exact":
                st = m.exact_state()
                rec["exact_graphs"], rec["exact_launches_per_step"] = st["graphs"], st["launches_per_step"]
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                with open(out, "a") as f:
                    f.write(line + "\n")
    m.close()


def trace():
    from nano_amd import binding as nb
    path, spec = model_path("qwen3-0.6b", "q80", 64)
    m = nb.load_model_file(path, max_seq_len=512, max_batch=1)
    m.set_exact(True)
    print("exact ms/step at position 510 (under the profiler):", m.time_step(1, 510, 20), m.exact_state())
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", default="")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--limit", type=int, default=280, help="seconds per child")
    args = ap.parse_args()
    if args.trace:
        return trace()
    if args.one:
        name, quant, gs, B = args.one.split(":")
        return one(name, quant, int(gs), int(B), args.iters, args.out)
    for name, quant, gs, B in CONFIGS:                                # one child per configuration; nothing is started after a failure
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", f"{name}:{quant}:{gs}:{B}",
               "--iters", str(args.iters if quant != "f32" else max(5, args.iters // 6))] + (["--out", args.out] if args.out else [])
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"exact_probe: {name}/{quant} x{B} ended with status {rc}; stopping", file=sys.stderr)
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
