"""GPU tests of the two LoRA side-branch launches (nano_amd/csrc/lora.hip) through nano_hip_op_lora_qkv / nano_hip_op_lora_o, which fill
LoraRowsArgs as a decode step with one module in every slot does: every element against the float64 reference within the derived bound of tests/lora_ref.py (held
against the kernels' emulated order, and shown to reject mutants, in tests/test_lora_ref.py), and bit for bit against the float32
restatement of the reference's order on inputs whose A side is exact in any order.  Every buffer travels whole: rows of v other than
(b, pos[b]), slots beyond nb and all guard rows must come back with the bits they went with.

Shapes (lora_ref.SHAPES): E 128 (half a wave idle in a down-projection), 192 and 260 (a second trip with a short tail; 260 is no
multiple of 64 either), 512 and 768 (the Nano sizes); KD in {E / 2, E, 96}; rank 1, 3, 4, 5, 8, 64 (fewer than the four waves, one more,
many); alpha / rank 16/3, 1/8 and 16/8 among them.  Forms (lora_ref.FORMS): one sequence; three sequences decoding at distinct
positions, the last at S - 1; a prefill chunk of five consecutive positions from 3 with v_bstride = 0."""
import numpy as np
import pytest

import lora_ref as lr
from nano_amd import binding as nb

pytestmark = pytest.mark.gpu

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
GUARD = 2                   # rows behind the nb rows of q / kraw / o1
WORST = {"qkv": 0.0, "o": 0.0}


def run_qkv(I, form, E, KD, rank, alpha):
    """one launch of the form on inputs I (I["v"][b] is set from the plane's row); returns (q, kraw, v plane) after the launch and the
    three as they went in"""
    _, nb_, pos, S, slots, bstride = form
    rng = np.random.default_rng([E, KD, rank, 9])
    q = np.concatenate([I["q"], rng.standard_normal((GUARD, E)).astype(np.float32)])
    k = np.concatenate([I["k"], rng.standard_normal((GUARD, KD)).astype(np.float32)])
    v = rng.standard_normal((slots * S, KD)).astype(np.float32)
    for b in range(nb_):
        I["v"][b] = v[lr.v_row_of(form, b)]
    before = (q.copy(), k.copy(), v.copy())
    nb.op_lora_qkv(I["x"], I["w"], [(I[n + "a"], I[n + "b"]) for n in "qkv"], q, k, v, pos, KD=KD, rank=rank, alpha=alpha, S=S, v_bstride=bstride * KD)
    return (q, k, v), before


def untouched(form, after, before):
    """guard rows, slots beyond nb and every v row but (b, pos[b]): the bits they went with"""
    nb_ = form[1]
    (q, k, v), (q0, k0, v0) = after, before
    rows = [lr.v_row_of(form, b) for b in range(nb_)]
    assert len(set(rows)) == nb_
    keep = np.ones(len(v), bool); keep[rows] = False
    assert np.array_equal(bits(q[nb_:]), bits(q0[nb_:])) and np.array_equal(bits(k[nb_:]), bits(k0[nb_:]))
    assert np.array_equal(bits(v[keep]), bits(v0[keep])), np.flatnonzero((bits(v) != bits(v0)).any(axis=1) & keep)
    return rows


@pytest.mark.parametrize("form", lr.FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("E,KD,rank,alpha", lr.SHAPES)
def test_qkv_within_the_bound(E, KD, rank, alpha, form):
    nb_ = form[1]
    I = lr.inputs(E, KD, rank, nb_)
    after, before = run_qkv(I, form, E, KD, rank, alpha)
    rows = untouched(form, after, before)
    worst = 0.0
    for b in range(nb_):
        got = (after[0][b], after[1][b], after[2][rows[b]])
        for name, g, (ref, bound) in zip("qkv", got, lr.exact_qkv(I, b, alpha, rank)):
            r = float((np.abs(g - ref) / bound).max())
            worst = max(worst, r)
            assert r <= 1.0, (name, b, r)
            assert np.any(g != I[name][b])                  # the branch did something
    WORST["qkv"] = max(WORST["qkv"], worst)
    print(f"lora_qkv E {E} KD {KD} rank {rank} alpha {alpha} {form[0]}: worst |d| / bound {worst:.4f} (file so far {WORST['qkv']:.4f})")


@pytest.mark.parametrize("form", lr.FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("E,KD,rank,alpha", lr.SHAPES)
def test_qkv_bit_for_bit(E, KD, rank, alpha, form):
    """order-free x (the sum of squares is exact in any order) and one-hot power-of-two A rows, different for q, k and v: the norm, the
    B side, the scale, the accumulate, and which t vector feeds which output -- the float32 restatement's bits"""
    nb_ = form[1]
    I = lr.exact_inputs(E, KD, rank, nb_)
    after, before = run_qkv(I, form, E, KD, rank, alpha)
    rows = untouched(form, after, before)
    for b in range(nb_):
        got = (after[0][b], after[1][b], after[2][rows[b]])
        for name, g, want in zip("qkv", got, lr.restate_qkv(I, b, alpha, rank)):
            assert np.array_equal(bits(g), bits(want)), (name, b, float(np.abs(g - want).max()))
            assert np.any(want != I[name][b])


@pytest.mark.parametrize("form", lr.FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("zero", ["x", "b"])
def test_qkv_zero_x_and_fresh_adapter_change_nothing(zero, form):
    E, KD, rank, alpha = 260, 130, 5, 16
    I = lr.exact_inputs(E, KD, rank, form[1], zero_x=zero == "x", zero_b=zero == "b")
    after, before = run_qkv(I, form, E, KD, rank, alpha)
    for a, b in zip(after, before):
        assert np.array_equal(bits(a), bits(b))


def run_o(I, E, rank, alpha, nb_):
    rng = np.random.default_rng([E, rank, 11])
    o1 = rng.standard_normal((nb_ + GUARD, E)).astype(np.float32)
    before = o1.copy()
    nb.op_lora_o(I["xba"], (I["oa"], I["ob"]), o1, rank=rank, alpha=alpha)
    assert np.array_equal(bits(o1[nb_:]), bits(before[nb_:]))
    return o1


@pytest.mark.parametrize("nb_", [1, 3])
@pytest.mark.parametrize("E,KD,rank,alpha", lr.SHAPES)
def test_o_within_the_bound(E, KD, rank, alpha, nb_):
    I = lr.inputs(E, KD, rank, nb_)
    o1 = run_o(I, E, rank, alpha, nb_)
    worst = 0.0
    for b in range(nb_):
        ref, bound = lr.exact_o(I, b, alpha, rank)
        worst = max(worst, float((np.abs(o1[b] - ref) / bound).max()))
    WORST["o"] = max(WORST["o"], worst)
    print(f"lora_o E {E} rank {rank} alpha {alpha} nb {nb_}: worst |d| / bound {worst:.4f} (file so far {WORST['o']:.4f})")
    assert 0 < worst <= 1.0


@pytest.mark.parametrize("nb_", [1, 3])
@pytest.mark.parametrize("E,KD,rank,alpha", lr.SHAPES)
def test_o_bit_for_bit(E, KD, rank, alpha, nb_):
    """order-free xba and A: t is exact in any order, the rest runs in the reference's order"""
    I = lr.exact_inputs(E, KD, rank, nb_)
    o1 = run_o(I, E, rank, alpha, nb_)
    for b in range(nb_):
        want = lr.restate_o(I, b, alpha, rank)
        assert np.array_equal(bits(o1[b]), bits(want)), (b, float(np.abs(o1[b] - want).max()))
        assert want.any()


@pytest.mark.parametrize("zero", ["x", "b"])
def test_o_zero_x_and_fresh_adapter_give_zeros(zero):
    E, KD, rank, alpha = 260, 130, 5, 16
    I = lr.exact_inputs(E, KD, rank, 3, zero_x=zero == "x", zero_b=zero == "b")
    o1 = run_o(I, E, rank, alpha, 3)
    assert not o1[:3].any()
