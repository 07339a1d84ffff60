"""The residual epilogue's addend, x += (W act + add) (the LoRA o-branch's o1; reference infer/infer.c:898-908), in every kernel body that
carries it: gemv_f32_slab_body.inc, gemv_q80_slab_body.inc, gemv_q4k.hip and gemv_q4k_chunk_body.inc's one-sequence epilogue and its
fold loop of several sequences -- each with its own indexing of the addend.  The launches go through nb.op_fused_gemv(kind=1,
resid_add=...), ordered=False as a step issues its Wo launch, with a DIFFERENT addend per sequence in a buffer whose stride is wider
than the rows (the floats between are a sentinel the result must not contain).

nb in {1, 3, 8, 9, 17}: the role-specialised one-sequence kernel, a capacity-4 kernel with a dead slot, a full capacity-8 kernel, and
the second and third slice of a cut batch (route.hip gemv_slice() shifts the addend by slice).  Shapes: one per kernel body the plan
queries report (Q4K_BODY and the closing test hold them against the queries, without a GPU), with rows that leave a ragged last workgroup (333, 7) and rows of 192 values
(no multiple of 256; Q4K: a block padded with zeros).

BARS.  Q80 and Q4K: bit for bit  old + (ref + add)  in float32, ref as tests/test_gpu_q80_gemv.py references() and
tests/test_gpu_q4k_gemv.py build() define it (canon.py's fold where the launch is canonical, else the oracle's order; the oracle's Q4K).
FP32: test_gpu_f32_gemv.py's row_bound e_r = (10 + nchunk) u S + u |dot| for the dot product, then the two roundings the epilogue adds,
    g = fl(dot^ + add):   |g - (dot + add)|         <= e_g = e_r (1 + u) + u |dot + add|
    out = fl(old + g):    |out - (old + dot + add)| <= e_g (1 + u) + u |old + dot + add|
-- derived, not fitted.  The route reported is a GEMV route, and the plan query asked with the flag set names it and the slicing."""
import numpy as np
import pytest

from nano_amd import binding as nb
from fused_ref import bits
import test_gpu_f32_gemv as f32t
import test_gpu_q80_gemv as q80t
import test_gpu_q4k_gemv as q4kt

F32, Q80, Q4K = 0x00, 0x80, 0x42
SENTINEL = np.float32(-12345.678)
NBS = (1, 3, 8, 9, 17)
PAD = 3                                     # floats between a sequence's addend row and the next one's
U = 2.0 ** -24
# (format, group size, n, rows) -> the kernel body its launches run, by nb: what the plan queries must report
SHAPES = [("f32", 0, 192, 192), ("f32", 0, 768, 768), ("f32", 0, 256, 333),
          ("q80", 32, 192, 192), ("q80", 32, 768, 768), ("q80", 32, 256, 333),
          ("q80", 64, 192, 192), ("q80", 64, 768, 768), ("q80", 64, 256, 333),
          ("q80", 128, 768, 768), ("q80", 128, 256, 333),
          ("q4k", 0, 192, 192), ("q4k", 0, 768, 768), ("q4k", 0, 256, 333), ("q4k", 0, 8448, 7)]
# Q4K picks between its two kernels by shape and batch: (n, rows) -> kernel by nb
Q4K_BODY = {(192, 192): dict.fromkeys(NBS, "slab"),
            (768, 768): {1: "chunk", 3: "slab", 8: "chunk", 9: "chunk", 17: "chunk"},
            (256, 333): {1: "chunk", 3: "slab", 8: "chunk", 9: "chunk", 17: "chunk"},
            (8448, 7): dict.fromkeys(NBS, "chunk")}
WORST = {"f32": 0.0}


def query(fmt, gs, n, rows, nb_):
    if fmt == "f32":
        return nb.f32_gemv_plan(1, n, [rows], nb_, resid_add=True)
    if fmt == "q80":
        return nb.q80_gemv_plan(1, n, [rows], nb_, gs=gs, resid_add=True)
    return nb.q4k_gemv_plan(1, n, [rows], nb_, resid_add=True)


def addend(rng, nb_, rows):
    """[nb, rows + PAD]: a different row per sequence, the floats behind each a sentinel"""
    a = np.full((nb_, rows + PAD), SENTINEL, np.float32)
    a[:, :rows] = rng.standard_normal((nb_, rows)).astype(np.float32)
    return a


def launch(quant, n, W, x, old, add, gs=0):
    nb_, rt = old.shape
    g = np.full((nb_ + 8, rt + 1), SENTINEL, np.float32)
    g[:nb_, :rt] = old
    out, route = nb.op_fused_gemv(quant, 1, n, W, x, None, gs=gs, nb=nb_, guard=g, want_route=True, resid_add=add)
    assert np.all(bits(g[:, rt]) == bits(SENTINEL)) and np.all(bits(g[nb_:]) == bits(SENTINEL)), "guard elements or slots beyond the batch were written"
    return g[:nb_, :rt], route


def check_plan(fmt, q, route, nb_):
    assert q["takes"] == 1, q
    assert q["launches"] * q["seqs_per_launch"] >= nb_ and (q["launches"] - 1) * q["seqs_per_launch"] < nb_, q
    assert q["launches"] == (nb_ + 7) // 8 and q["seqs_per_launch"] == min(nb_, 8), q           # 9 and 17 reach a second and a third slice
    assert route in ("gemv", "gemv_sliced", "q4k"), route
    if fmt == "f32":
        assert route == ("gemv_sliced" if nb_ > 8 else "gemv")
    else:
        assert route == nb.ROUTE_NAMES[q["route"]], (route, q)


@pytest.mark.gpu
@pytest.mark.parametrize("nb_", NBS)
@pytest.mark.parametrize("fmt,gs,n,rows", [s for s in SHAPES if s[0] == "f32"])
def test_f32_addend_within_the_bound(fmt, gs, n, rows, nb_):
    rng = np.random.default_rng([n, rows, nb_])
    W = (0.02 * rng.standard_normal((rows, n))).astype(np.float32)
    x = f32t.order_free(rng, (nb_, n))
    old = rng.standard_normal((nb_, rows)).astype(np.float32)
    add = addend(rng, nb_, rows)
    q = query(fmt, gs, n, rows, nb_)
    out, route = launch(F32, n, [(W, None, rows)], x, old, add)
    worst = 0.0
    for b in range(nb_):
        dot, S = f32t.dot64(W, x[b])
        e_r = f32t.row_bound(dot, S, n)
        g = dot + add[b, :rows].astype(np.float64)
        ref = old[b].astype(np.float64) + g
        bound = (e_r * (1 + U) + U * np.abs(g)) * (1 + U) + U * np.abs(ref)
        r = float((np.abs(out[b] - ref) / bound).max())
        worst = max(worst, r)
        assert r <= 1.0, (b, r)
        # the addend is felt: the same sequence without it is further away than the bound
        assert float((np.abs(add[b, :rows]) / bound).max()) > 1.0
    WORST["f32"] = max(WORST["f32"], worst)
    print(f"f32 addend n {n} rows {rows} nb {nb_}: role {nb.F32_ROLES[q['role']]} B {q['B']} x {q['launches']} launches, worst |d| / bound {worst:.4f} "
          f"(file so far {WORST['f32']:.4f})")
    check_plan(fmt, q, route, nb_)


@pytest.mark.gpu
@pytest.mark.parametrize("nb_", NBS)
@pytest.mark.parametrize("fmt,gs,n,rows", [s for s in SHAPES if s[0] == "q80"])
def test_q80_addend_bit_for_bit(oracle, fmt, gs, n, rows, nb_):
    rng = np.random.default_rng([gs, n, rows, nb_])
    c = dict(gs=gs, n=n, kind=1, rows=(rows,), norm=False)
    W = [(rng.integers(-127, 128, size=rows * n, dtype=np.int8), rng.uniform(1e-4, 2e-3, size=rows * n // gs).astype(np.float32), rows)]
    I = dict(x=f32t.order_free(rng, (nb_, n)), nw=None)
    old = rng.standard_normal((nb_, rows)).astype(np.float32)
    add = addend(rng, nb_, rows)
    q = query(fmt, gs, n, rows, nb_)
    out, route = launch(Q80, n, W, I["x"], old, add, gs=gs)
    for b in range(nb_):
        _, cref = q80t.references(oracle, c, I, b, W)                 # canon.py's fold where the launch is canonical, else the oracle's order
        want = (old[b] + (cref + add[b, :rows]).astype(np.float32)).astype(np.float32)
        bad = np.flatnonzero(bits(out[b]) != bits(want))
        assert bad.size == 0, (b, bad[:6].tolist(), float(np.abs(out[b] - want).max()))
        assert np.any(bits(want) != bits((old[b] + cref).astype(np.float32)))
    assert q["kernel"] == q80t.SLAB, q
    check_plan(fmt, q, route, nb_)


@pytest.mark.gpu
@pytest.mark.parametrize("nb_", NBS)
@pytest.mark.parametrize("fmt,gs,n,rows", [s for s in SHAPES if s[0] == "q4k"])
def test_q4k_addend_bit_for_bit(oracle, fmt, gs, n, rows, nb_):
    rng = np.random.default_rng([n, rows, nb_])
    T, blocks = q4kt.pool(oracle, n)
    idx = rng.integers(0, blocks.shape[0], size=rows)
    W = [(np.ascontiguousarray(blocks[idx]), None, rows)]
    x = f32t.order_free(rng, (nb_, n))
    old = rng.standard_normal((nb_, rows)).astype(np.float32)
    add = addend(rng, nb_, rows)
    q = query(fmt, gs, n, rows, nb_)
    out, route = launch(Q4K, n, W, x, old, add)
    for b in range(nb_):
        ref = oracle.matmul_q4k(oracle.quantize_q4k(x[b], [n]), T, 0, blocks.shape[0])[idx]
        want = (old[b] + (ref + add[b, :rows]).astype(np.float32)).astype(np.float32)
        bad = np.flatnonzero(bits(out[b]) != bits(want))
        assert bad.size == 0, (b, bad[:6].tolist(), float(np.abs(out[b] - want).max()))
        assert np.any(bits(want) != bits((old[b] + ref).astype(np.float32)))
    kernel = nb.Q4K_KERNELS[q["kernel"]]
    assert kernel == Q4K_BODY[(n, rows)][nb_], (kernel, q)
    check_plan(fmt, q, route, nb_)


def test_the_shapes_reach_every_body_that_carries_the_addend():
    """from the plan queries alone (no launch): the five epilogues, the role-specialised and the generic kernels among them"""
    seen = set()
    for fmt, gs, n, rows in SHAPES:
        for nb_ in NBS:
            q = query(fmt, gs, n, rows, nb_)
            role = nb.F32_ROLES[q["role"]]
            if fmt == "q4k":
                k = nb.Q4K_KERNELS[q["kernel"]]
                seen.add(("q4k", k, "one" if q["B"] == 1 else "several"))
            else:
                seen.add((fmt, "slab", "one" if q["B"] == 1 else "several"))
            assert role == ("resid" if q["B"] == 1 and not (fmt == "q80" and gs == 64 and n % 256) else "generic"), (fmt, gs, n, rows, nb_, role)
    assert seen == {(f, k, w) for f, ks in (("f32", ("slab",)), ("q80", ("slab",)), ("q4k", ("slab", "chunk"))) for k in ks for w in ("one", "several")}
    print("bodies and plans the addend cases reach:", sorted(seen))
