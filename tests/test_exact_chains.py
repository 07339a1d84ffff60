"""CPU test of the chain algebra exact mode's sums rest on (nano_amd/csrc/exact_chain.h): the chunked evaluation of rmsnorm's
index-order sum of squares equals the plain float loop of the reference (infer/infer.c:601-606), bit for bit."""
import os
import re
import subprocess

from conftest import ROOT


def test_chunked_sum_of_squares_equals_the_plain_loop(tmp_path):
    """Gaussian, heavy-tailed, all-zero, denormal, one dominant element first / last, multiples of 1/16 (constant ties), overflowing and
    mixed-scale vectors; n in {32, 48, 128, 768, 1024, 2560, 5120} plus lengths that are no multiple of the chunk; chunks of 16, 32, 64."""
    exe = str(tmp_path / "ssq_check")
    src = os.path.join(ROOT, "tools", "exact", "ssq_check.cpp")
    subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-o", exe, src, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout
    m = re.match(r"(\d+) cases", out.stdout)
    assert m and int(m.group(1)) >= 3000
    print(out.stdout.strip())


def test_exact_mode_is_declared_bound_and_documented():
    """The public surface of the mode: C header, Python binding, the environment switch in the knob tables."""
    hdr = open(os.path.join(ROOT, "include", "nano_mi355x.h")).read()
    for decl in ("int nano_hip_set_exact(NanoHipModel *m, int on);",
                 "int nano_hip_exact_state(const NanoHipModel *m, uint32_t *on, uint32_t *graphs, uint32_t *launches_per_step);",
                 "int nano_hip_op_exact_rmsnorm(", "int nano_hip_op_exact_attention("):
        assert decl in hdr, decl
    from nano_amd import binding as nb
    for name in ("set_exact", "exact_state"):
        assert callable(getattr(nb.DeviceModel, name))
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "NANO_EXACT" in open(os.path.join(ROOT, doc)).read(), doc
