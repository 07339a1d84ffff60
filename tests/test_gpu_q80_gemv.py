"""Every Q80 GEMV launch plan (gemv_q80_impl.h, gemv_q80_slab_body.inc, one build per group size) against the reference's own
arithmetic (quantize infer/tensor.c:21-46, matmul_quant infer/infer.c:654-679, rmsnorm 601-614, residual adds 906-908 / 963-965,
SwiGLU 937-944), bit for bit.

The launches go through nb.op_fused_gemv(0x80, ...), i.e. the step's own router (route.hip), and nb.q80_gemv_plan reports the plan the
launchers follow: gemv_q80_slab_kernel<ROLE, GS, B, NV, UPW, EARLY, WF, WFC> or gemv_q80_stream_kernel<ROLE, GS, B, NV>, its waves, rows
per workgroup, LDS bytes and the slices the router cuts a batch into.  Each case names the plan it is meant to reach; the closing
coverage test checks from the reported plans that the cases reach every axis of the template space the CPU sweep
(tests/test_q80_gemv_plan.py UNIVERSE) finds reachable.  Values are checked first (a plan mismatch must not hide a wrong result).

INPUTS (test_gpu_fused_roles.py): activations order-free (multiples of 2^-4 in [-2, 2]: sums of squares of up to 2^14 of them are exact
in any order, so oracle.rmsnorm -- and with it the quantized activation -- is pinned exactly; cases with a norm keep n <= 16384),
weights int8 in [-127, 127], scales uniform in [1e-4, 2e-3], old residual standard_normal; combine cases have equal split maxima (every
exp() an exact 1) and split sums that add to a power of two.

BARS, none of them new.
  * Group size 64, n % 256 == 0, not a tall STORE matrix (kernels.h q80_canonical()): the fast path == canon.matmul_q80_canon bit for
    bit, ordered=True == oracle.matmul_q80 bit for bit, fast vs oracle within 1e-5 of max|ref| (check_q80 of test_gpu_fused_roles.py).
  * Every other launch (other group sizes, n % 256 != 0, tall): both modes bit for bit the oracle's.
  * SwiGLU: the store form of the same two matrices bit for bit as above, the fused form under rtol = 3e-6, atol = 1e-9 (the device's
    expf against libm: test_k4_norm_swiglu_q80's bar).
EVERY BATCHED CASE: each sequence bit-equals the same launch of that sequence alone; the launch runs in a guarded buffer -- nb + 8 slots
of rows_total + 1 floats filled with a sentinel -- and every element outside [b < nb, : rows_total] must come back untouched (the dead
slots of a capacity-4 / -8 kernel at 3 / 5 / 6 / 7 sequences are where a stray store would land).
STREAM CASES also run as the step's classifier launch runs (tests/test_gpu_q4k_gemv.py PARTIALS): with a partials buffer of nb + 2 slots x
partials + 4 pairs prefilled with (+inf, row 0).  The launch reports STREAM_WGS * 4 pairs per sequence, one per wave; every one of the
nb * ntiles pairs is overwritten and every pair behind them untouched; a wave owns strided 16-row tiles, so instead of a row mapping every
written pair (v, i) has i == 0xffffffff (an idle wave) or bits(out[b, i]) == bits(v); the arg-max kernel's rule over the pairs, the arg-max
kernel behind the launch and the arg-max kernel scanning a launch without partials all give np.argmax(out[b]).  One case duplicates the
arg-max row's weights and scales into rows of one 16-row tile, of another tile of the same wave and of another workgroup's tile."""
import numpy as np
import pytest

from nano_amd import binding as nb
from test_q80_gemv_plan import UNIVERSE, VAR, ROLE, SLAB, STREAM, canonical
from fused_ref import bits, order_free, silu_mul, rows_total

Q80 = 0x80
SENTINEL = np.float32(-12345.678)
POISON = np.array([np.inf, 0.0], np.float32)               # (+inf, row 0): wins any reduction that reads it
NO_ROW = 0xffffffff


def case(cid, gs, kind, n, rows, nb_, want, norm=False, comb=None, ties=False, **more):
    """kind 0 store / 1 residual add / 2 SwiGLU (rows: two equal counts); comb = (n_head, head_dim, split sums) for a launch whose prologue
    combines split-attention partials; want = (kernel, B, NV, UPW, variant) of the fast path's launch, more = further plan fields; ties:
    the arg-max row's weights duplicated (STREAM)"""
    k, B, nv, upw, var = want
    target = dict(kernel=k, B=B, nv=nv, upw=upw, variant=VAR[var], **more)
    return pytest.param(dict(id=cid, gs=gs, kind=kind, n=n, rows=tuple(rows), nb=nb_, norm=norm, comb=comb, ties=ties, target=target), id=cid)


R = {k: ROLE[k] for k in ROLE}
CASES = [
    # ---- the slab kernel's (B, NV, UPW), one sequence; the five roles at group size 32 among them -------------------------------------
    case("b1-nv1-upw1-gs32", 32, 0, 64, (4,), 1, (SLAB, 1, 1, 1, "plain"), norm=True, role=R["norm_store"]),
    case("b1-nv2-upw1-gs32", 32, 1, 768, (7,), 1, (SLAB, 1, 2, 1, "plain"), role=R["resid"]),
    case("b1-nv4-upw1-gs32", 32, 0, 8448, (4,), 1, (SLAB, 1, 4, 1, "plain"), norm=True),
    case("b1-loop-upw2", 32, 1, 16640, (4,), 1, (SLAB, 1, 0, 2, "plain"), role=R["resid"]),
    case("b1-loop-upw4-swiglu", 32, 2, 16640, (4, 4), 1, (SLAB, 1, 0, 4, "plain"), role=R["generic"]),
    case("b1-nv1-upw2-swiglu-gs32", 32, 2, 32, (2560, 2560), 1, (SLAB, 1, 1, 2, "plain"), norm=True, role=R["norm_swiglu"], rw=10),
    case("b1-nv1-upw4-swiglu", 32, 2, 32, (8192, 8192), 1, (SLAB, 1, 1, 4, "plain"), norm=True, rw=32),
    case("b1-nv2-upw2-swiglu", 32, 2, 1056, (1024, 1024), 1, (SLAB, 1, 2, 2, "plain"), norm=True),
    case("b1-nv2-upw4", 32, 0, 2816, (6656,), 1, (SLAB, 1, 2, 4, "plain"), norm=True, rw=26),
    case("b1-nv4-upw2-swiglu", 32, 2, 8448, (4, 4), 1, (SLAB, 1, 4, 2, "plain"), norm=True),
    case("b1-nv4-upw4", 32, 0, 6400, (2560,), 1, (SLAB, 1, 4, 4, "plain"), norm=True, rw=10),
    case("b1-combine-gs32", 32, 1, 256, (33,), 1, (SLAB, 1, 1, 1, "plain"), comb=(4, 64, (1, 3, 2, 2)), role=R["resid_combine"]),
    # ---- the roles at group sizes 64 / 128 / 256, ragged rows (7, 33, 333; three tensors 36 | 4 | 12) -----------------------------------
    case("norm-store-gs64-three-tensors", 64, 0, 256, (36, 4, 12), 1, (SLAB, 1, 1, 1, "plain"), norm=True, role=R["norm_store"]),
    case("resid-gs64-333", 64, 1, 256, (333,), 1, (SLAB, 1, 1, 1, "plain"), role=R["resid"]),
    case("combine-gs64-8-splits", 64, 1, 512, (33,), 1, (SLAB, 1, 1, 1, "plain"), comb=(4, 128, (1, 1, 2, 4, 2, 2, 1, 3)), role=R["resid_combine"]),
    case("norm-swiglu-gs64", 64, 2, 256, (12, 12), 1, (SLAB, 1, 1, 1, "plain"), norm=True, role=R["norm_swiglu"]),
    case("generic-gs64-store-no-norm", 64, 0, 256, (7,), 1, (SLAB, 1, 1, 1, "plain"), role=R["generic"]),
    case("norm-store-gs128-three-tensors", 128, 0, 384, (36, 4, 12), 1, (SLAB, 1, 1, 1, "plain"), norm=True, role=R["norm_store"]),
    case("resid-gs128-33", 128, 1, 128, (33,), 1, (SLAB, 1, 1, 1, "plain"), role=R["resid"]),
    case("combine-gs128", 128, 1, 256, (7,), 1, (SLAB, 1, 1, 1, "plain"), comb=(2, 128, (3, 5)), role=R["resid_combine"]),
    case("norm-swiglu-gs128", 128, 2, 1152, (12, 12), 1, (SLAB, 1, 2, 1, "plain"), norm=True, role=R["norm_swiglu"]),
    case("generic-gs128-swiglu-no-norm", 128, 2, 256, (8, 8), 1, (SLAB, 1, 1, 1, "plain"), role=R["generic"]),
    case("norm-store-gs256-three-tensors", 256, 0, 512, (36, 4, 12), 1, (SLAB, 1, 1, 1, "plain"), norm=True, role=R["norm_store"]),
    case("resid-gs256-333", 256, 1, 1280, (333,), 1, (SLAB, 1, 2, 1, "plain"), role=R["resid"]),
    case("combine-gs256", 256, 1, 256, (33,), 1, (SLAB, 1, 1, 1, "plain"), comb=(4, 64, (1, 3, 2, 2)), role=R["resid_combine"]),
    case("norm-swiglu-gs256", 256, 2, 256, (16, 16), 1, (SLAB, 1, 1, 1, "plain"), norm=True, role=R["norm_swiglu"]),
    case("generic-gs256-store-no-norm", 256, 0, 768, (7,), 1, (SLAB, 1, 2, 1, "plain"), role=R["generic"]),
    case("generic-gs32-store-no-norm", 32, 0, 96, (333,), 1, (SLAB, 1, 1, 1, "plain"), role=R["generic"]),
    # ---- group size 64, rows that are no multiple of 256: the generic kernel, the reference's order in both modes ---------------------------
    case("gs64-n1408-ragged", 64, 1, 1408, (33,), 1, (SLAB, 1, 2, 1, "plain"), role=R["generic"]),
    case("gs64-n2304-three-tensors-b4", 64, 0, 2304, (36, 4, 12), 3, (SLAB, 4, 1, 1, "plain"), norm=True),
    # ---- the in-wave folds ---------------------------------------------------------------------------------------------------------------
    case("wf-store", 64, 0, 1024, (36, 4, 12), 1, (SLAB, 1, 2, 1, "wf"), norm=True, role=R["norm_store"]),
    case("wf-swiglu-pairs", 64, 2, 1024, (12, 12), 1, (SLAB, 1, 2, 1, "wf"), norm=True, role=R["norm_swiglu"]),
    case("wfc2-ragged", 64, 1, 2048, (7,), 1, (SLAB, 1, 2, 1, "wfc2"), role=R["resid"]),
    case("wfc2-combine", 64, 1, 2048, (33,), 1, (SLAB, 1, 2, 1, "wfc2"), comb=(16, 128, (1, 3, 2, 2)), role=R["resid_combine"]),
    case("wfc3", 64, 1, 3072, (33,), 1, (SLAB, 1, 2, 1, "wfc3"), role=R["resid"]),
    case("wfc4", 64, 1, 4096, (7,), 1, (SLAB, 1, 2, 1, "wfc4"), role=R["resid"]),
    # ---- EARLY (matrices of >= 8 Mi weights, group size 64) at one and at two sequences ------------------------------------------------------
    case("early-b1-nv4-upw2-swiglu", 64, 2, 8192, (512, 512), 1, (SLAB, 1, 4, 2, "early"), norm=True, role=R["norm_swiglu"]),
    case("early-b2-nv4-upw2-swiglu", 64, 2, 8192, (512, 512), 2, (SLAB, 2, 4, 2, "early"), norm=True, route="gemv"),
    case("early-b2-nv2-upw4", 64, 0, 2816, (6656,), 2, (SLAB, 2, 2, 4, "early"), norm=True, route="gemv"),
    case("early-b2-nv4-upw4", 64, 0, 6400, (2560,), 2, (SLAB, 2, 4, 4, "early"), norm=True, route="gemv"),
    # ---- capacity 2 ---------------------------------------------------------------------------------------------------------------------
    case("b2-nv1-upw1-gs128", 128, 0, 128, (36, 4, 12), 2, (SLAB, 2, 1, 1, "plain"), norm=True),
    case("b2-nv2-upw1-gs256", 256, 1, 768, (33,), 2, (SLAB, 2, 2, 1, "plain")),
    case("b2-nv4-upw1", 32, 0, 8448, (4,), 2, (SLAB, 2, 4, 1, "plain"), norm=True),
    case("b2-loop-upw2", 32, 1, 16640, (4,), 2, (SLAB, 2, 0, 2, "plain")),
    case("b2-loop-upw4-swiglu", 32, 2, 16640, (4, 4), 2, (SLAB, 2, 0, 4, "plain"), lds_bytes=71104),
    case("b2-nv1-upw2-swiglu", 32, 2, 32, (2048, 2048), 2, (SLAB, 2, 1, 2, "plain"), norm=True),
    case("b2-nv1-upw4-swiglu", 32, 2, 32, (8192, 8192), 2, (SLAB, 2, 1, 4, "plain"), norm=True),
    case("b2-nv2-upw2-swiglu", 32, 2, 2080, (4, 4), 2, (SLAB, 2, 2, 2, "plain"), norm=True),
    case("b2-nv4-upw2-swiglu", 32, 2, 8448, (4, 4), 2, (SLAB, 2, 4, 2, "plain"), norm=True),
    case("b2-gs64-canonical-333", 64, 1, 512, (333,), 2, (SLAB, 2, 1, 1, "plain")),
    # ---- capacity 4 (3 sequences: a dead slot) ------------------------------------------------------------------------------------------
    case("b4-nv1-upw1-gs32", 32, 1, 64, (7,), 3, (SLAB, 4, 1, 1, "plain")),
    case("b4-gs64-combine", 64, 1, 512, (33,), 3, (SLAB, 4, 1, 1, "plain"), comb=(4, 128, (1, 3, 2, 2))),
    case("b4-gs128-swiglu", 128, 2, 256, (12, 12), 4, (SLAB, 4, 1, 1, "plain"), norm=True),
    case("b4-gs256-333", 256, 0, 512, (333,), 3, (SLAB, 4, 1, 1, "plain"), norm=True),
    case("b4-nv2-upw1", 32, 0, 4352, (4,), 3, (SLAB, 4, 2, 1, "plain"), norm=True),
    case("b4-loop-upw1", 32, 0, 8448, (4,), 3, (SLAB, 4, 0, 1, "plain"), norm=True),
    case("b4-loop-upw2-106k", 32, 1, 16640, (4,), 3, (SLAB, 4, 0, 2, "plain"), lds_bytes=108672),
    case("b4-loop-upw4-swiglu-139k", 32, 2, 16640, (4, 4), 3, (SLAB, 4, 0, 4, "plain"), lds_bytes=142208),
    case("b4-nv1-upw2-swiglu", 32, 2, 32, (2048, 2048), 3, (SLAB, 4, 1, 2, "plain"), norm=True),
    case("b4-nv1-upw4-swiglu", 32, 2, 32, (8192, 8192), 3, (SLAB, 4, 1, 4, "plain"), norm=True),
    case("b4-nv2-upw2-preq", 32, 0, 6656, (4096,), 3, (SLAB, 4, 2, 2, "plain"), norm=True, route="gemv_preq", pre=1),
    case("b4-nv2-upw4-preq-gs64", 64, 0, 4352, (12800,), 3, (SLAB, 4, 2, 4, "plain"), norm=True, route="gemv_preq", pre=1),
    # ---- capacity 8 (5, 6, 7 sequences: dead slots) -------------------------------------------------------------------------------------
    case("b8-nv1-upw1-gs32-5", 32, 0, 64, (36, 4, 12), 5, (SLAB, 8, 1, 1, "plain"), norm=True),
    case("b8-gs64-6", 64, 1, 256, (333,), 6, (SLAB, 8, 1, 1, "plain")),
    case("b8-gs128-7-combine", 128, 1, 256, (7,), 7, (SLAB, 8, 1, 1, "plain"), comb=(2, 128, (3, 5))),
    case("b8-gs256-8-swiglu", 256, 2, 256, (12, 12), 8, (SLAB, 8, 1, 1, "plain"), norm=True),
    case("b8-loop-upw1", 32, 0, 4352, (4,), 5, (SLAB, 8, 0, 1, "plain"), norm=True),
    case("b8-loop-upw2-152k", 128, 1, 16640, (4,), 6, (SLAB, 8, 0, 2, "plain"), lds_bytes=155264),
    case("b8-loop-upw4-swiglu-151k", 256, 2, 16640, (4, 4), 7, (SLAB, 8, 0, 4, "plain"), lds_bytes=154240),
    case("b8-nv1-upw2-swiglu", 32, 2, 32, (2048, 2048), 6, (SLAB, 8, 1, 2, "plain"), norm=True),
    case("b8-nv1-upw4-swiglu", 32, 2, 32, (8192, 8192), 7, (SLAB, 8, 1, 4, "plain"), norm=True),
    case("b8-loop-upw2-swiglu-gs64", 64, 2, 9728, (4, 4), 5, (SLAB, 8, 0, 2, "plain"), norm=True, lds_bytes=136448),
    # ---- batches the LDS fit rule cuts -------------------------------------------------------------------------------------------------
    case("cut-5-in-4-and-1-swiglu-gs32", 32, 2, 9728, (4, 4), 5, (SLAB, 4, 0, 2, "plain"), norm=True, launches=2, seqs_per_launch=4),
    case("cut-8-in-two-gs64", 64, 1, 16384, (7,), 8, (SLAB, 4, 0, 1, "plain"), launches=2, seqs_per_launch=4),
    # ---- STREAM (tall STORE matrices: the classifier) ---------------------------------------------------------------------------------------
    case("stream-b1-nv1-norm-ragged-tile", 32, 0, 64, (16391,), 1, (STREAM, 1, 1, 0, "plain"), norm=True, role=R["norm_store"]),
    case("stream-b1-nv2-gs64", 64, 0, 1088, (16384,), 1, (STREAM, 1, 2, 0, "plain"), norm=True, role=R["norm_store"]),
    case("stream-b1-nv4-gs128", 128, 0, 2176, (16384,), 1, (STREAM, 1, 4, 0, "plain"), role=R["generic"]),
    case("stream-b1-loop-gs256", 256, 0, 4352, (16384,), 1, (STREAM, 1, 0, 0, "plain"), norm=True, role=R["norm_store"]),
    case("stream-b2-nv1-generic", 64, 0, 256, (16391,), 2, (STREAM, 2, 1, 0, "plain"), role=R["generic"]),
    case("stream-b2-nv2", 256, 0, 1280, (65536,), 2, (STREAM, 2, 2, 0, "plain"), norm=True),
    case("stream-b2-nv4", 256, 0, 2304, (65536,), 2, (STREAM, 2, 4, 0, "plain"), norm=True),
    case("stream-b2-loop", 256, 0, 4352, (65536,), 2, (STREAM, 2, 0, 0, "plain"), norm=True),
    case("stream-b4-nv1-3", 128, 0, 128, (16391,), 3, (STREAM, 4, 1, 0, "plain"), norm=True),
    case("stream-b4-nv2-3", 128, 0, 1152, (65536,), 3, (STREAM, 4, 2, 0, "plain"), norm=True),
    case("stream-b4-loop-3", 256, 0, 2304, (65536,), 3, (STREAM, 4, 0, 0, "plain")),
    case("stream-b8-nv1-5", 32, 0, 96, (16391,), 5, (STREAM, 8, 1, 0, "plain"), norm=True),
    case("stream-b8-nv1-8-gs64", 64, 0, 256, (16400,), 8, (STREAM, 8, 1, 0, "plain"), norm=True),
    case("stream-b8-loop-5", 64, 0, 1088, (65536,), 5, (STREAM, 8, 0, 0, "plain"), norm=True),
    # 4099 tiles on 4096 waves: waves 0..2 own two tiles; the arg-max row duplicated (TIE_ROWS)
    case("stream-b1-ties-two-tiles-a-wave", 32, 0, 64, (65573,), 1, (STREAM, 1, 1, 0, "plain"), norm=True, ties=True, role=R["norm_store"]),
]


def query(c, **kw):
    attn = (c["comb"][0], c["comb"][1], len(c["comb"][2])) if c["comb"] else None
    return nb.q80_gemv_plan(c["kind"], c["n"], c["rows"], c["nb"], gs=c["gs"], norm=c["norm"], attn=attn, **kw)


def build(c):
    """the inputs of a case: weights per tensor, activations (or attention partials), norm weight, old residual"""
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(c["id"])))
    n, nb_, gs = c["n"], c["nb"], c["gs"]
    assert not c["norm"] or n <= 16384, "a norm case beyond 16384 values: the sum of squares is no longer exact in any order"
    W = [(rng.integers(-127, 128, size=r * n, dtype=np.int8), rng.uniform(1e-4, 2e-3, size=r * n // gs).astype(np.float32), r) for r in c["rows"]]
    nw = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32) if c["norm"] else None
    x, attn = order_free(rng, (nb_, n)), None
    if c["comb"]:
        n_head, hd, ls = c["comb"]
        L = sum(ls)
        assert L & (L - 1) == 0 and n_head * hd == n
        part = order_free(rng, (nb_, len(ls), n))
        ml = np.zeros((nb_, n_head, len(ls), 2), np.float32)
        ml[..., 0] = 0.25
        ml[..., 1] = np.asarray(ls, np.float32)
        x = (part.astype(np.float64).sum(axis=1) / L).astype(np.float32)            # every split's weight is exp(0) / L
        assert np.array_equal(x.astype(np.float64), part.astype(np.float64).sum(axis=1) / L)
        attn = (part, ml, n_head, hd)
    old = rng.standard_normal((nb_, rows_total(c["kind"], c["rows"]))).astype(np.float32) if c["kind"] == 1 else None
    return dict(W=W, nw=nw, x=x, attn=attn, old=old)


def canon_rows(xq, xs, wq, ws, n, rows, block=1024):
    """canon.matmul_q80_canon (the fast path's fold: unit sums of 8 groups in ascending order, units ascending), a block of rows at a time"""
    from canon import matmul_q80_canon
    ng = n // 64
    out = np.empty(rows, np.float32)
    for r0 in range(0, rows, block):
        r1 = min(rows, r0 + block)
        out[r0:r1] = matmul_q80_canon(xq, xs, wq[r0 * n:r1 * n], ws[r0 * ng:r1 * ng], n, r1 - r0)
    return out


def references(oracle, c, I, b, W):
    """(the reference's order, the fast path's bits) of sequence b over the tensors W, the residual not yet added"""
    act = oracle.rmsnorm(I["x"][b], I["nw"]) if c["norm"] else I["x"][b]
    xq, xs = oracle.quantize_q80(act, c["gs"])
    ref = np.concatenate([oracle.matmul_q80(xq, xs, wq, ws, c["n"], r, c["gs"]) for wq, ws, r in W])
    if canonical(c["gs"], c["n"], c["kind"], c["rows"], False):
        return ref, np.concatenate([canon_rows(xq, xs, wq, ws, c["n"], r) for wq, ws, r in W])
    return ref, ref


def launch(c, I, *, kind=None, ordered=False, sl=None, guarded=True, partials=None, want_argmax=False):
    """the case's launch, or with sl = b the same launch of sequence b alone; the batched launch runs in a guarded buffer (partials: the
    step's partials buffer, want_argmax: the arg-max kernel behind the launch -- then (out, route, ntiles or None, argmax or None))"""
    kind = c["kind"] if kind is None else kind
    rt = rows_total(c["kind"], c["rows"]) if kind == c["kind"] else sum(c["rows"])
    if sl is not None:
        b = slice(sl, sl + 1)
        attn = (I["attn"][0][b], I["attn"][1][b], I["attn"][2], I["attn"][3]) if I["attn"] else None
        return nb.op_fused_gemv(Q80, kind, c["n"], I["W"], None if attn else I["x"][b], I["nw"], gs=c["gs"], nb=1, ordered=ordered,
                                resid=I["old"][b] if I["old"] is not None else None, attn=attn)[0], None
    g = np.full((c["nb"] + 8, rt + 1), SENTINEL, np.float32)
    if I["old"] is not None:
        g[:c["nb"], :rt] = I["old"]
    res = nb.op_fused_gemv(Q80, kind, c["n"], I["W"], None if I["attn"] else I["x"], I["nw"], gs=c["gs"], nb=c["nb"], ordered=ordered,
                           attn=I["attn"], guard=g, want_route=True, partials=partials, want_argmax=want_argmax)
    route = res[1]
    assert np.all(bits(g[:, rt]) == bits(SENTINEL)), (c["id"], ordered, "a guard element behind a sequence's rows changed")
    assert np.all(bits(g[c["nb"]:]) == bits(SENTINEL)), (c["id"], ordered, "slots beyond the batch were written",
                                                         (np.flatnonzero((bits(g[c["nb"]:]) != bits(SENTINEL)).any(axis=1)) + c["nb"]).tolist())
    if partials is not None or want_argmax:
        return g[:c["nb"], :rt], route, res[2] if partials is not None else None, res[-1] if want_argmax else None
    return g[:c["nb"], :rt], route


# rows the tie case copies the arg-max row's weights and scales into: two of tile 1 (wave 1), one of tile 4097 (wave 1's second tile), one of
# tile 2000 (another workgroup) -- the arg-max row itself stays where the random weights put it
TIE_ROWS = (16 + 3, 16 + 9, 4097 * 16 + 2, 2000 * 16 + 7)


def plant_ties(c, I, ref):
    (wq, ws, r), = I["W"]
    n, ng = c["n"], c["n"] // c["gs"]
    assert c["nb"] == 1 and r > max(TIE_ROWS) and (r + 15) // 16 > 4097
    m = int(np.argmax(ref))
    for t in TIE_ROWS:
        wq[t * n:(t + 1) * n] = wq[m * n:(m + 1) * n]
        ws[t * ng:(t + 1) * ng] = ws[m * ng:(m + 1) * ng]


def reduce_pairs(pairs):
    """argmax_kernel's rule over (value, row bits) pairs: no-row pairs skipped, the larger value, on equal values the lower row"""
    best, bi = None, NO_ROW
    for v, i in zip(pairs[:, 0].tolist(), pairs[:, 1].view(np.uint32).tolist()):
        if i != NO_ROW and (bi == NO_ROW or v > best or (v == best and i < bi)):
            best, bi = v, i
    return 0 if bi == NO_ROW else bi


def check_stream_partials(c, I, q, fused):
    """the STREAM launch as the step's classifier launch: one (max, first row) pair per wave and sequence"""
    nb_, rows = c["nb"], c["rows"][0]
    want_tiles = q["grid"] * 4
    buf = np.empty((nb_ + 2, want_tiles + 4, 2), np.float32)
    buf[:] = POISON
    out, _, ntiles, amax = launch(c, I, partials=buf, want_argmax=True)
    assert np.array_equal(bits(out), bits(fused)), (c["id"], "the launch with partials differs")
    assert ntiles == want_tiles, (c["id"], ntiles, q)
    flat = buf.reshape(-1, 2)
    inside, rest = flat[:nb_ * ntiles].reshape(nb_, ntiles, 2), flat[nb_ * ntiles:]
    stale = np.argwhere((bits(inside) == bits(POISON)).all(axis=2))
    assert stale.size == 0, (c["id"], "pairs the arg-max kernel reads were not written: (sequence, wave)", stale[:6].tolist())
    touched = np.flatnonzero((bits(rest) != bits(POISON)).any(axis=1)) + nb_ * ntiles
    assert touched.size == 0, (c["id"], "pairs beyond the launch's nb * ntiles were written", touched[:6].tolist())
    first = [int(np.argmax(out[b])) for b in range(nb_)]
    for b in range(nb_):
        i = inside[b, :, 1].view(np.uint32)
        live = i != NO_ROW
        assert live.any() and np.all(i[live] < rows), (c["id"], "sequence", b, "a pair names a row beyond the matrix")
        bad = np.flatnonzero(live)[bits(out[b][i[live]]) != bits(inside[b, live, 0])]
        assert bad.size == 0, (c["id"], "sequence", b, "waves whose pair is not (out[row], row)", bad[:6].tolist())
        assert reduce_pairs(inside[b]) == first[b], (c["id"], "sequence", b, "the pairs do not reduce to the first maximum")
    assert amax.tolist() == first, (c["id"], "arg-max from the partials", amax.tolist(), first)
    scan, _, _, amax_scan = launch(c, I, want_argmax=True)                          # no partials buffer: the arg-max kernel scans the logits
    assert np.array_equal(bits(scan), bits(fused)), (c["id"], "the launch without partials differs")
    assert amax_scan.tolist() == first, (c["id"], "arg-max by scanning", amax_scan.tolist(), first)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES)
def test_q80_gemv_plan_case(oracle, c):
    q = query(c)
    assert q["takes"] == 1, (c["id"], "the router refuses this shape: nothing is launched", q)
    I = build(c)
    kind, nb_ = c["kind"], c["nb"]
    canon = canonical(c["gs"], c["n"], kind, c["rows"], False)
    refs = [references(oracle, c, I, b, I["W"]) for b in range(nb_)]
    if c["ties"]:
        plant_ties(c, I, refs[0][0])
        refs = [references(oracle, c, I, b, I["W"]) for b in range(nb_)]
        assert np.all(bits(refs[0][0][list(TIE_ROWS)]) == bits(refs[0][0].max())) and int(np.argmax(refs[0][0])) == min(TIE_ROWS)
    errors = []

    def held(out, mode, what, b, want):
        bad = np.flatnonzero(bits(out) != bits(want))
        if bad.size:
            errors.append(f"{mode} {what} sequence {b}: {bad.size} of {want.size} rows differ, first rows {bad[:6].tolist()}, worst |d| {float(np.abs(out - want).max()):.3e}")

    # 1. values (the launches also assert their guard elements), strict mode first: the reference's own bits
    store_kind = 0 if kind == 2 else kind                      # SwiGLU: the store form of the same two matrices pins the projections
    for ordered in (True, False):
        mode = "ordered" if ordered else "fast"
        out, route = launch(c, I, kind=store_kind, ordered=ordered)
        if not ordered and kind != 2:
            assert route == nb.ROUTE_NAMES[q["route"]], (c["id"], route, q)
        for b in range(nb_):
            ref, cref = refs[b]
            want = ref if ordered else cref
            if kind == 1:
                want = (I["old"][b] + want).astype(np.float32)
            held(out[b], mode, "store form" if kind == 2 else "result", b, want)
            if not ordered and canon:                            # the fast path against the reference's order (SURVEY 7 tier ii)
                strict = (I["old"][b] + ref).astype(np.float32) if kind == 1 else ref
                tier = float(np.abs(out[b] - strict).max()) / float(np.abs(ref).max())
                if not tier <= 1e-5:
                    errors.append(f"fast sequence {b}: {tier:.2e} of max|ref| off the reference's order")
        if kind == 2:
            out, route = launch(c, I, ordered=ordered)
            if not ordered:
                assert route == nb.ROUTE_NAMES[q["route"]], (c["id"], route, q)
                fused = out
            R_ = c["rows"][0]
            for b in range(nb_):
                h = refs[b][0 if ordered else 1]
                want = silu_mul(h[:R_], h[R_:])
                if not np.allclose(out[b], want, rtol=3e-6, atol=1e-9):
                    errors.append(f"{mode} SwiGLU sequence {b}: off by {float(np.abs(out[b] - want).max()):.3e}")
        elif not ordered:
            fused = out
    assert not errors, f"{c['id']} (plan {q}): " + "; ".join(errors[:4])
    # 2. a batch is its sequences alone
    if nb_ > 1:
        for b in range(nb_):
            alone, _ = launch(c, I, sl=b)
            assert np.array_equal(bits(fused[b]), bits(alone)), (c["id"], "sequence", b, "differs from its launch alone", float(np.abs(fused[b] - alone).max()))
    # 3. the arg-max partials of the STREAM launches
    if q["kernel"] == STREAM:
        check_stream_partials(c, I, q, fused)
    # 4. the plan, last
    got = {k: (nb.ROUTE_NAMES[q[k]] if k == "route" else q[k]) for k in c["target"]}
    assert got == c["target"], f"{c['id']}: the launcher's plan is {q}, the case means {c['target']}: a retune moved this case -- pick a new shape for this target"


def test_cases_cover_every_plan_axis():
    """The cases reach every axis of the template space the CPU sweep finds reachable -- read from the plans the query reports (CPU-only),
    which each case's own test also holds against the plan the case states."""
    T = []
    for p in CASES:
        c = p.values[0]
        q = query(c)
        assert q["takes"] == 1, c["id"]
        got = {k: (nb.ROUTE_NAMES[q[k]] if k == "route" else q[k]) for k in c["target"]}
        assert got == c["target"], (c["id"], q)
        assert (q["kernel"], q["B"], q["nv"], q["upw"], q["variant"]) in UNIVERSE, (c["id"], "a plan the sweep does not know", q)
        T.append(dict(q, id=c["id"], kind=c["kind"], n=c["n"], rows=c["rows"], nb=c["nb"], norm=c["norm"], comb=c["comb"] is not None, ties=c["ties"],
                      total=rows_total(c["kind"], c["rows"]), route_name=nb.ROUTE_NAMES[q["route"]]))

    def has(f=None, **kw):
        return any(all(t[k] == v for k, v in kw.items()) and (f is None or f(t)) for t in T)

    missing = []

    def need(what, ok):
        if not ok:
            missing.append(what)

    # every (B, NV, UPW) of the slab kernel and every (B, NV) of the stream kernel that some descriptor of the sweep reaches
    for k, B, nv, upw in sorted({u[:4] for u in UNIVERSE}):
        need(("kernel, B, NV, UPW", k, B, nv, upw), has(kernel=k, B=B, nv=nv, upw=upw))
    for gs in (32, 64, 128, 256):
        for role in nb.Q80_ROLES:
            need(("role", role, gs), has(kernel=SLAB, B=1, gs=gs, role=ROLE[role]))
        for B in (2, 4, 8):
            need(("generic", B, gs), has(kernel=SLAB, B=B, gs=gs, role=ROLE["generic"]))
    for nb_, B in ((3, 4), (5, 8), (6, 8), (7, 8)):
        need(("dead slots", nb_, B), has(kernel=SLAB, nb=nb_, B=B))
    need("early at one sequence", has(variant=VAR["early"], B=1)); need("early at two sequences", has(variant=VAR["early"], B=2))
    for v in ("wf", "wfc2", "wfc3", "wfc4"):
        need(v, has(variant=VAR[v]))
    need("wf with SwiGLU pairs", has(variant=VAR["wf"], kind=2)); need("wfc with the combine", has(variant=VAR["wfc2"], comb=True))
    need("F_PRE through gemv_preq", has(route_name="gemv_preq", pre=1))
    need("more than 64 KiB of LDS at capacity 4", has(kernel=SLAB, B=4, f=lambda t: t["lds_bytes"] > 65536))
    need("more than 64 KiB of LDS at capacity 8", has(kernel=SLAB, B=8, f=lambda t: t["lds_bytes"] > 65536))
    for r in (7, 33, 333):
        need(("ragged rows", r), has(kernel=SLAB, rows=(r,)))
        need(("ragged rows in a batch", r), has(kernel=SLAB, rows=(r,), f=lambda t: t["B"] > 1))
    need("three tensors", has(rows=(36, 4, 12), B=1)); need("three tensors in a batch", has(rows=(36, 4, 12), f=lambda t: t["B"] > 1))
    for n in (1408, 2304):
        need(("group size 64, n % 256 != 0", n), has(gs=64, n=n))
    need("a sliced batch", has(f=lambda t: t["launches"] > 1 and t["nb"] <= 8))
    need("the combine in a batch", has(comb=True, f=lambda t: t["B"] > 1))
    need("stream, norm role", has(kernel=STREAM, role=ROLE["norm_store"])); need("stream, generic role", has(kernel=STREAM, role=ROLE["generic"]))
    for nb_ in (1, 2, 3, 5, 8):
        need(("stream sequences", nb_), has(kernel=STREAM, nb=nb_))
    need("stream, a ragged last tile", has(kernel=STREAM, rows=(16391,)))
    need("stream, two tiles a wave with the arg-max row duplicated", has(kernel=STREAM, ties=True, f=lambda t: (t["total"] + 15) // 16 > 4 * t["grid"] + 1))
    for gs in (32, 64, 128, 256):
        need(("stream group size", gs), has(kernel=STREAM, gs=gs))
    assert not missing, missing
