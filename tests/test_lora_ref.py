"""CPU tests of tests/lora_ref.py: the bound of the LoRA side branches holds for a float32 emulation of the kernels' order on every
GPU case's inputs, mutants of that emulation leave it, and the bit-for-bit inputs make the kernels' order and the reference's agree."""
import numpy as np
import pytest

import lora_ref as lr

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
# beyond the GPU cases: a wide one (ten trips of a lane, rank 16)
SHAPES = lr.SHAPES + [(2560, 1024, 16, 16)]
NB = 3


def ratios(I, b, alpha, rank, mutant=None):
    """worst |d| / bound of sequence b over q, k, v and o1"""
    got = lr.emulate_qkv(I, b, alpha, rank, mutant) + (lr.emulate_o(I, b, alpha, rank, mutant),)
    want = lr.exact_qkv(I, b, alpha, rank) + [lr.exact_o(I, b, alpha, rank)]
    return [float((np.abs(g - ref) / bound).max()) for g, (ref, bound) in zip(got, want)]


@pytest.mark.parametrize("E,KD,rank,alpha", SHAPES)
def test_bound_against_the_emulated_order(E, KD, rank, alpha):
    """(the largest ratios belong to the accumulate: where the delta is small beside the old value -- rank 1, alpha / rank = 1/8 -- the
    error is the last rounding's, of which u |ref| is the attainable size)"""
    worst = 0.0
    for nb_ in sorted({f[1] for f in lr.FORMS}):                 # the inputs of every GPU case: lr.inputs() is seeded by the batch too
        I = lr.inputs(E, KD, rank, nb_)
        worst = max(worst, max(max(ratios(I, b, alpha, rank)) for b in range(nb_)))
    print(f"E {E} KD {KD} rank {rank} alpha {alpha}: worst |d| / bound {worst:.4f}")
    assert 0 < worst <= 1.0
    I = lr.inputs(E, KD, rank, NB)
    # the float32 restatement of the reference's order is held by the same bound (it has no fewer roundings per term on the A side, so
    # this is no theorem -- it shows the bound is of the size of either order's error, not far above both)
    for b in range(NB):
        got = lr.restate_qkv(I, b, alpha, rank) + (lr.restate_o(I, b, alpha, rank),)
        want = lr.exact_qkv(I, b, alpha, rank) + [lr.exact_o(I, b, alpha, rank)]
        assert all(float((np.abs(g - ref) / bound).max()) < 8.0 for g, (ref, bound) in zip(got, want))


@pytest.mark.parametrize("mutant", [m for m in lr.MUTANTS if m != "pos0"])
@pytest.mark.parametrize("E,KD,rank,alpha", SHAPES)
def test_mutants_leave_the_bound(E, KD, rank, alpha, mutant):
    I = lr.inputs(E, KD, rank, NB)
    for b in range(NB):
        q, k, v, o = ratios(I, b, alpha, rank, mutant)
        hit = {"drop_float4": max(q, o), "v_reads_k": v, "skip_last_rank": min(q, k, v, o)}[mutant]
        print(f"{mutant} E {E} rank {rank} b {b}: |d| / bound {hit:.1f}")
        assert hit > 1.0, (mutant, b, q, k, v, o)


@pytest.mark.parametrize("form", [f for f in lr.FORMS if f[1] > 1], ids=lambda f: f[0])
def test_pos0_mutant_leaves_the_bound(form):
    """the v buffer as a launch leaves it, every row against its own bound: `pos[0]` for every b piles the deltas on one row"""
    E, KD, rank, alpha = 192, 96, 3, 16
    _, nb, pos, S, slots, bstride = form
    I = lr.inputs(E, KD, rank, nb)
    rng = np.random.default_rng(5)
    v0 = rng.standard_normal((slots * S, KD)).astype(np.float32)
    ref, bound = v0.astype(np.float64), np.zeros((slots * S, KD))
    for b in range(nb):
        I["v"][b] = v0[lr.v_row_of(form, b)]
        ref[lr.v_row_of(form, b)], bound[lr.v_row_of(form, b)] = lr.exact_qkv(I, b, alpha, rank)[2]
    for mutant, inside in ((None, True), ("pos0", False)):
        v = v0.copy()
        for b in range(nb):
            r = lr.v_row_of(form, b, mutant)
            I["v"][b] = v[r]
            v[r] = lr.emulate_qkv(I, b, alpha, rank)[2]
        touched = bound.max(axis=1) > 0
        ok = bool((np.abs(v[touched] - ref[touched]) <= bound[touched]).all()) and np.array_equal(bits(v[~touched]), bits(v0[~touched]))
        assert ok == inside, mutant


@pytest.mark.parametrize("E,KD,rank,alpha", lr.SHAPES)
def test_exact_inputs_make_both_orders_agree(E, KD, rank, alpha):
    """on exact_inputs() the kernels' order gives the reference's bits (what the GPU's bit-for-bit cases rest on), the branches do
    something, and the order mutant -- which no rounding bound can see -- changes bits wherever the scale is inexact"""
    I = lr.exact_inputs(E, KD, rank, NB)
    moved = 0
    for b in range(NB):
        want = lr.restate_qkv(I, b, alpha, rank) + (lr.restate_o(I, b, alpha, rank),)
        got = lr.emulate_qkv(I, b, alpha, rank) + (lr.emulate_o(I, b, alpha, rank),)
        for g, w in zip(got, want):
            assert np.array_equal(bits(g), bits(w))
        assert all(np.any(w != I[n][b]) for n, w in zip("qkv", want)) and np.any(want[3] != 0)
        mut = lr.emulate_qkv(I, b, alpha, rank, "scale_first") + (lr.emulate_o(I, b, alpha, rank, "scale_first"),)
        moved += sum(int(np.any(bits(g) != bits(w))) for g, w in zip(mut, want))
        # a t vector fed to the wrong output
        swapped = dict(I, va=I["ka"])
        assert np.any(bits(lr.emulate_qkv(swapped, b, alpha, rank)[2]) != bits(want[2]))
    if (alpha / rank) != 2.0 ** round(np.log2(alpha / rank)):
        assert moved > 0


@pytest.mark.parametrize("zero", ["x", "b"])
def test_zero_inputs_leave_the_rows(zero):
    E, KD, rank, alpha = 260, 130, 5, 16
    I = lr.exact_inputs(E, KD, rank, 1, zero_x=zero == "x", zero_b=zero == "b")
    q, k, v = lr.restate_qkv(I, 0, alpha, rank)
    assert np.array_equal(bits(q), bits(I["q"][0])) and np.array_equal(bits(k), bits(I["k"][0])) and np.array_equal(bits(v), bits(I["v"][0]))
    assert not lr.restate_o(I, 0, alpha, rank).any()
