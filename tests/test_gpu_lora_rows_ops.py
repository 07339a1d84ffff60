"""GPU tests of the two LoRA launches (nano_amd/csrc/lora.hip lora_qkv_rows_kernel / lora_o_rows_kernel) with rows of different
modules, through nano_hip_op_lora_qkv_rows / nano_hip_op_lora_o_rows, which fill LoraRowsArgs as a step with a LoRA table does.

Three adapters A, B, C of (rank, alpha) (5, 16), (8, 4), (1, 16) -- unequal ranks, an inexact scale, and the rank-1 case in which
tests/lora_ref.py found the largest attainable error -- and five rows with row_adapter = [A, none, B, A, C], in the decode form (a v row
per slot, distinct positions) and the chunk form (v_bstride 0, consecutive positions).  For every row with an adapter, q, k, its v row
and o1 are
  (a) bit for bit what the single-module operators (nano_hip_op_lora_qkv / _o) give that row alone with that adapter -- the same
      kernels in a launch of one row and one adapter: a row's bits depend neither on the other rows, nor on the batch size, nor on
      its adapter's index (what pins the kernels to the reference is tests/test_gpu_lora_ops.py),
  (b) bit for bit lora_ref.emulate_qkv / emulate_o on lora_ref.exact_inputs,
  (c) within lora_ref.exact_qkv / exact_o's derived bound, per element, on lora_ref.inputs.
The row without an adapter keeps the bytes of q, k and its v row, and its o1 row is 0x80000000 (-0.0f) in every element.  Every other
row of the v buffer (a canary pattern), and the guard rows behind q / kraw / o1, keep their bytes.  A second launch with the adapters
listed in another order gives every row the same bits: the result depends on the module, not on its index."""
import numpy as np
import pytest

import lora_ref as lr
from nano_amd import binding as nb

pytestmark = pytest.mark.gpu

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
ADAPTERS = [(5, 16), (8, 4), (1, 16)]               # A, B, C: (rank, alpha)
ROWS = [0, None, 1, 0, 2]
NB = len(ROWS)
SHAPES = [(128, 64), (260, 130), (768, 96)]
# lora_ref's form tuples (name, nb, positions, S, v slots, v_bstride in rows): five rows each
FORMS = [("decode5", NB, (0, 5, 8, 2, 3), 9, 6, 9), next(f for f in lr.FORMS if f[0] == "chunk5")]
GUARD = 2
CANARY = 0x7fc0beef                                 # a NaN pattern: any arithmetic on it, or a store over it, shows


def test_the_cases_are_what_the_file_says():
    assert all((E, KD) in {(s[0], s[1]) for s in lr.SHAPES} for E, KD in SHAPES)
    assert FORMS[0][5] == FORMS[0][3] and len(set(FORMS[0][2])) == NB and FORMS[1][5] == 0 and FORMS[1][1] == NB
    assert np.diff(FORMS[1][2]).tolist() == [1] * (NB - 1)


def make_inputs(E, KD, exact):
    """(base, [per-adapter inputs]): x, w, q, k, v, xba shared by the rows; each adapter's four pairs from its own seed"""
    gen = lr.exact_inputs if exact else lr.inputs
    base = gen(E, KD, ADAPTERS[0][0], NB)
    per = []
    for i, (rank, _alpha) in enumerate(ADAPTERS):
        own = gen(E, KD, rank, NB, seed=10 + i)
        I = dict(base)
        for n in "qkvo":
            I[n + "a"], I[n + "b"] = own[n + "a"], own[n + "b"]
        per.append(I)
    return base, per


def qkv_adapters(per, order):
    return [(ADAPTERS[i][0], ADAPTERS[i][1], tuple((per[i][n + "a"], per[i][n + "b"]) for n in "qkv")) for i in order]


def o_adapters(per, order):
    return [(ADAPTERS[i][0], ADAPTERS[i][1], ((per[i]["oa"], per[i]["ob"]),)) for i in order]


def remap(order):
    return [None if r is None else order.index(r) for r in ROWS]


def run_qkv(base, per, form, KD, order=(0, 1, 2)):
    _, nb_, pos, S, slots, bstride = form
    E = base["x"].shape[1]
    rng = np.random.default_rng([E, KD, 9])
    q = np.concatenate([base["q"], rng.standard_normal((GUARD, E)).astype(np.float32)])
    k = np.concatenate([base["k"], rng.standard_normal((GUARD, KD)).astype(np.float32)])
    v = np.full((slots * S, KD), CANARY, np.uint32).view(np.float32)
    rows = [lr.v_row_of(form, b) for b in range(nb_)]
    assert len(set(rows)) == nb_
    for b in range(nb_):
        v[rows[b]] = base["v"][b]
    before = (q.copy(), k.copy(), v.copy())
    nb.op_lora_qkv_rows(base["x"], base["w"], qkv_adapters(per, order), remap(order), q, k, v, pos, KD=KD, S=S, v_bstride=bstride * KD)
    return (q, k, v), before, rows


def alone_qkv(I, b, form, KD, rank, alpha, before, row):
    """the single-module operator on row b alone: its q, k and a whole slot plane of v as the rows launch saw them"""
    _, _, pos, S, _, _ = form
    q, k = before[0][b:b + 1].copy(), before[1][b:b + 1].copy()
    slot0 = row - pos[b]
    v = before[2][slot0:slot0 + S].copy()
    nb.op_lora_qkv(I["x"][b:b + 1], I["w"], [(I[n + "a"], I[n + "b"]) for n in "qkv"], q, k, v, [pos[b]], KD=KD, rank=rank, alpha=alpha, S=S, v_bstride=S * KD)
    return q[0], k[0], v[pos[b]]


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("exact", [True, False], ids=["exact_inputs", "inputs"])
@pytest.mark.parametrize("E,KD", SHAPES)
def test_qkv_rows(E, KD, exact, form):
    base, per = make_inputs(E, KD, exact)
    after, before, rows = run_qkv(base, per, form, KD)
    (q, k, v), (q0, k0, v0) = after, before
    keep = np.ones(len(v), bool); keep[rows] = False
    assert np.array_equal(bits(v[keep]), bits(v0[keep])), np.flatnonzero((bits(v) != bits(v0)).any(axis=1) & keep)
    assert (bits(v[keep]) == CANARY).all()
    assert np.array_equal(bits(q[NB:]), bits(q0[NB:])) and np.array_equal(bits(k[NB:]), bits(k0[NB:]))
    worst = 0.0
    for b, ad in enumerate(ROWS):
        got = (q[b], k[b], v[rows[b]])
        if ad is None:                                              # no module: the bytes the row went with
            for g, w in zip(got, (q0[b], k0[b], v0[rows[b]])):
                assert np.array_equal(bits(g), bits(w)), b
            continue
        rank, alpha = ADAPTERS[ad]
        I = per[ad]
        for name, g, w in zip("qkv", got, alone_qkv(I, b, form, KD, rank, alpha, before, rows[b])):        # (a)
            assert np.array_equal(bits(g), bits(w)), ("single-module operator", name, b, float(np.abs(g - w).max()))
        if exact:                                                   # (b)
            want = lr.emulate_qkv(I, b, alpha, rank)
            for name, g, w in zip("qkv", got, want):
                assert np.array_equal(bits(g), bits(w)), ("emulation", name, b, float(np.abs(g - w).max()))
            # (a one-hot rank-1 A row may meet a zero of x: one of the three may stand still, not all)
            assert any(np.any(w != I[name][b]) for name, w in zip("qkv", want)), b
        else:                                                       # (c)
            for name, g, (ref, bound) in zip("qkv", got, lr.exact_qkv(I, b, alpha, rank)):
                r = float((np.abs(g - ref) / bound).max())
                worst = max(worst, r)
                assert r <= 1.0, (name, b, r)
                assert np.any(g != I[name][b])
    if not exact:
        print(f"lora_qkv_rows E {E} KD {KD} {form[0]}: worst |d| / bound {worst:.4f}")
    # the adapters in another order: the same bits in every buffer
    again, _, _ = run_qkv(base, per, form, KD, order=(2, 0, 1))
    for a, b_ in zip(again, after):
        assert np.array_equal(bits(a), bits(b_))


def run_o(base, per, order=(0, 1, 2)):
    E = base["xba"].shape[1]
    rng = np.random.default_rng([E, 11])
    o1 = rng.standard_normal((NB + GUARD, E)).astype(np.float32)
    before = o1.copy()
    nb.op_lora_o_rows(base["xba"], o_adapters(per, order), remap(order), o1)
    assert np.array_equal(bits(o1[NB:]), bits(before[NB:]))
    return o1


@pytest.mark.parametrize("exact", [True, False], ids=["exact_inputs", "inputs"])
@pytest.mark.parametrize("E,KD", SHAPES)
def test_o_rows(E, KD, exact):
    base, per = make_inputs(E, KD, exact)
    o1 = run_o(base, per)
    worst = 0.0
    for b, ad in enumerate(ROWS):
        if ad is None:
            assert (bits(o1[b]) == 0x80000000).all(), b             # -0.0f: r + (-0.0f) is r for every float r
            continue
        rank, alpha = ADAPTERS[ad]
        I = per[ad]
        alone = np.full((1, E), 3.0, np.float32)
        nb.op_lora_o(I["xba"][b:b + 1], (I["oa"], I["ob"]), alone, rank=rank, alpha=alpha)
        assert np.array_equal(bits(o1[b]), bits(alone[0])), ("single-module operator", b)                  # (a)
        if exact:
            want = lr.emulate_o(I, b, alpha, rank)                                                          # (b)
            assert np.array_equal(bits(o1[b]), bits(want)), ("emulation", b, float(np.abs(o1[b] - want).max()))
            assert want.any()
        else:
            ref, bound = lr.exact_o(I, b, alpha, rank)                                                      # (c)
            r = float((np.abs(o1[b] - ref) / bound).max())
            worst = max(worst, r)
            assert 0 < r <= 1.0, (b, r)
    if not exact:
        print(f"lora_o_rows E {E}: worst |d| / bound {worst:.4f}")
    assert np.array_equal(bits(run_o(base, per, order=(1, 2, 0))), bits(o1))


def test_adding_minus_zero_changes_no_bit():
    """the identity the Wo epilogue relies on, on the host's IEEE arithmetic: r + (-0.0f) has r's bits, both zeros and the denormals included"""
    r = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 3.4e38, np.inf, -np.inf], np.float32)
    assert np.array_equal(bits(r + np.float32(-0.0)), bits(r))
