"""CPU test of the HIP-graph keys of a step (nano_amd/csrc/step_spec.h: StepSpec, step_key): tools/step_key_check.cpp, compiled with g++
alone against the header, enumerates the three kinds of steps x nb {1, 8, 9, 64} x modes 0..5 x causal x hints {64, 80, 2048, max_seq_len}
x slots {0, 1, 63} x LoRA / stamps / skip_embed x the four key_kinds and checks that two steps share a key exactly when they agree in
every field their family's captured nodes depend on, that the three families never collide, and that a value one past a field's width
yields "no key" instead of spilling into the neighbouring field."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tools", "step_key_check.cpp")


def build_and_run(tmp_path, name, flags, max_seq_len):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC])
    out = subprocess.run([exe, str(max_seq_len)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.match(r"(\d+) steps \((\d+) fast, (\d+) chunk, (\d+) ordered\), (\d+) distinct keys, (\d+) width edges, max_seq_len (\d+): 0 failures", out.stdout)
    assert m, out.stdout
    print(out.stdout.strip())
    return [int(g) for g in m.groups()]


@pytest.mark.parametrize("max_seq_len", [4096, 40960])
def test_keys_distinguish_what_the_captured_nodes_depend_on(tmp_path, max_seq_len):
    steps, fast, chunk, ordered, keys, edges, S = build_and_run(tmp_path, "step_key_check", ["-O1"], max_seq_len)
    per = 4 * 6 * 2 * 4 * 8                                    # nb x mode x causal x hint x (LoRA, stamps, skip_embed)
    assert (fast, chunk, ordered, S) == (per, per * 3 * 4, per * 3, max_seq_len) and steps == fast + chunk + ordered
    # fast: skip_embed counts with MODE_LOOP only; chunk: kind, LoRA, slot, hint, nb; ordered: slot, nb, causal, mode
    assert keys == 4 * 2 * 4 * 4 * (6 + 1) + 4 * 2 * 3 * 4 * 4 + 3 * 4 * 2 * 6
    assert edges == 2 * (3 + 2 + 2 + 2 + 2 + 1)


def test_keys_under_the_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (shifts by a field's width among the things looked at)"""
    build_and_run(tmp_path, "step_key_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], 40960)
