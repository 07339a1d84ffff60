"""Every FP32 GEMV launch plan (gemv_f32.hip + gemv_f32_slab_body.inc) against a float64 reference of the same projection
(reference: rmsnorm infer/infer.c:601-614, matmul 637-651, residual adds 906-908 / 963-965, SwiGLU 937-944).

The launches go through nb.op_fused_gemv(0x00, ...), i.e. the step's own router (route.hip), and nb.f32_gemv_plan reports the plan
the launcher follows: gemv_f32_slab_kernel<ROLE, B, NV, UPW> on nw waves, rw rows per workgroup, its LDS bytes and the slices the
router cuts a batch into.  Each case below names the plan it is meant to reach; the closing coverage test checks from the reported
plans that the cases reach every axis the planner can pick.  Values are checked first (a plan mismatch must not hide a wrong result).

EXACT CASES (no rmsnorm in front).  Activations are integer multiples of 2^-4 in [-2, 2], weights integer multiples of 2^-4 in
[-1, 1], old residual values multiples of 2^-8.  Every product and every partial sum in ANY association is then an integer multiple
of one power of two g and bounded by n * max|w| * max|a|; whenever bound / g <= 2^24 (asserted per case) all of them are exactly
representable in fp32, so the kernel's FMA chains, its DPP tree, its ordered chunk adds and a float64 dot are the same number.  These
cases are held BIT FOR BIT: a kernel that drops, doubles or misplaces one product, chunk, row or sequence cannot pass.  The
split-attention combine is exact the same way with equal split maxima (every exp() an exact 1) and split sums that add up to a power
of two.  SwiGLU without a norm has exact h1 and h3 and keeps the device expf's tolerance (rtol 3e-6, atol 1e-9: the bar of
test_gpu_fused_roles.py::test_k4_norm_swiglu_q80).

NORM CASES.  The activations are order-free (sums of squares exact in any order), so oracle.rmsnorm pins the normalised activation a
bit for bit (the argument of test_gpu_fused_roles.py's docstring); the weights are 0.02 * standard_normal.  A row of the kernel is
    lane:   p = w0 a0, then three fused multiply-adds            4 roundings on the path of any one product
    wave:   4 DPP levels + (r0 + r1) + (r2 + r3)                 6 roundings
    fold:   the nchunk chunk sums added in ascending order       <= nchunk roundings
Each rounding moves its partial sum by at most 2^-24 of its magnitude, which never exceeds S = sum |w_i a_i|; to first order the row
is off the exact dot by at most (10 + nchunk) 2^-24 S, and the last rounding is at most 2^-24 |ref|:
    |d| <= (10 + nchunk) * 2^-24 * S + 2^-24 * |ref|       per row.
SwiGLU: with e1, e3 those bounds of h1 and h3 and silu' in [-0.1, 1.1],
    |d| <= 1.1 e1 |h3| + |silu(h1)| e3 + 1.1 e1 e3 + 3e-6 |silu(h1) h3|.
The project's global bar max|d| <= 1e-5 max|ref| per sequence stays as a second assertion.
How much slack the bound has: test_bound_against_the_emulated_order() runs a numpy fp32 emulation of exactly that order (float4 FMA
chain, pairwise tree over 64 lanes, ordered chunks) against float64 on every norm case's inputs; its worst |d| / bound over all rows
of all norm cases is 0.097 (cls-151936x64-norm, the most rows; rows of 9728 floats stay below 0.01): random roundings add up like sqrt(depth), the bound
like depth.  The bound is derived, not fitted: it is not to be loosened to make a case pass.

EVERY BATCHED CASE: each sequence bit-equals the same launch of that sequence alone; the output buffer carries one guard element
behind every sequence's rows and 8 guard slots behind the last sequence (where the dead slots of a capacity-4 / -8 kernel would
write), all of which must come back untouched."""
import numpy as np
import pytest

from nano_amd import binding as nb
from fused_ref import bits, order_free, silu_mul, rows_total

F32 = 0x00
U = 2.0 ** -24
SENTINEL = np.float32(-12345.678)
ROLE = {n: i for i, n in enumerate(nb.F32_ROLES)}


def exact_weights(rng, rows, n):
    """multiples of 2^-4 in [-1, 1]"""
    return (rng.integers(-16, 17, size=(rows, n), dtype=np.int8).astype(np.float32) / np.float32(16.0)).astype(np.float32)


def plan(role, B, nv, upw, rw, nw, launches=1, per=None, lds=None):
    t = dict(role=ROLE[role], B=B, nv=nv, upw=upw, rw=rw, nw=nw, launches=launches)
    if per is not None:
        t["seqs_per_launch"] = per
    if lds is not None:
        t["lds_bytes"] = lds
    return t


def case(cid, kind, n, rows, nb_, target, norm=False, comb=None):
    """kind 0 store / 1 residual add / 2 SwiGLU (rows: two equal counts); comb = (n_head, head_dim, split sums) for a launch whose
    prologue combines split-attention partials"""
    return pytest.param(dict(id=cid, kind=kind, n=n, rows=tuple(rows), nb=nb_, norm=norm, comb=comb, target=target), id=cid)


CASES = [
    # ---- exact cases: one sequence, the role-specialised kernels and the generic one --------------------------------------------
    case("wo-nano168", 1, 768, (768,), 1, plan("resid", 1, 1, 1, 4, 3)),
    case("w2-nano168", 1, 2048, (768,), 1, plan("resid", 1, 1, 1, 4, 8)),
    case("w2-06b-nv2", 1, 3072, (1024,), 1, plan("resid", 1, 2, 2, 4, 8)),
    case("w2-4b-nv4-upw4", 1, 9728, (2560,), 1, plan("resid", 1, 4, 4, 4, 10)),
    case("12-waves", 1, 12288, (512,), 1, plan("resid", 1, 4, 4, 4, 12)),
    case("longest-row-16-waves", 1, 16384, (36,), 1, plan("resid", 1, 4, 4, 4, 16, lds=66624)),
    case("rw32-store", 0, 256, (16384,), 1, plan("generic", 1, 1, 1, 32, 8)),
    case("rw16-three-tensors", 0, 512, (8192, 4096, 4096), 1, plan("generic", 1, 1, 1, 16, 8)),
    case("rw8-cls-nano168", 0, 768, (16384,), 1, plan("generic", 1, 1, 1, 8, 6)),
    case("ragged-333x352", 0, 352, (333,), 1, plan("generic", 1, 1, 1, 4, 2)),
    case("ragged-resid-1001x1408", 1, 1408, (1001,), 1, plan("resid", 1, 1, 1, 4, 6)),
    case("three-tensors-odd-n", 0, 192, (36, 4, 12), 1, plan("generic", 1, 1, 1, 4, 2)),
    case("w13-06b-no-norm", 2, 1024, (3072, 3072), 1, plan("generic", 1, 1, 2, 8, 8)),
    case("w13-4b-no-norm", 2, 2560, (1000, 1000), 1, plan("generic", 1, 2, 4, 4, 8)),
    # ---- exact cases: the split-attention combine ------------------------------------------------------------------------------
    case("combine-nano168-4", 1, 768, (768,), 1, plan("resid_combine", 1, 1, 1, 4, 3), comb=(16, 48, (1, 3, 2, 2))),
    case("combine-nano168-2", 1, 768, (768,), 1, plan("resid_combine", 1, 1, 1, 4, 3), comb=(16, 48, (3, 5))),
    case("combine-nano168-8", 1, 768, (768,), 1, plan("resid_combine", 1, 1, 1, 4, 3), comb=(16, 48, (1, 1, 2, 4, 2, 2, 1, 3))),
    case("combine-more-heads-than-threads", 1, 256, (64,), 1, plan("resid_combine", 1, 1, 1, 4, 2), comb=(64, 4, (1, 3, 2, 2))),
    case("combine-nv2", 1, 3072, (1024,), 1, plan("resid_combine", 1, 2, 2, 4, 8), comb=(24, 128, (1, 3, 2, 2))),
    case("combine-b4-dead-slot", 1, 768, (768,), 3, plan("generic", 4, 1, 1, 4, 3), comb=(16, 48, (1, 3, 2, 2))),
    case("combine-b8-loop-form", 1, 4608, (512,), 7, plan("generic", 8, 0, 2, 4, 16, lds=159744), comb=(36, 128, (1, 3, 2, 2))),
    # ---- exact cases: batches (capacities 2 / 4 / 8, dead slots at 3 / 5 / 7 sequences) -----------------------------------------
    case("b2-nv4-upw4", 1, 9728, (2560,), 2, plan("generic", 2, 4, 4, 4, 10, lds=79232)),
    case("b4-loop-form-158k", 1, 9728, (2560,), 4, plan("generic", 4, 0, 4, 4, 16, lds=158464)),
    case("b4-loop-form-dead-slot", 1, 9728, (2560,), 3, plan("generic", 4, 0, 4, 4, 16, lds=158464)),
    case("b8-cut-in-two", 1, 9728, (2560,), 8, plan("generic", 4, 0, 4, 4, 16, launches=2, per=4, lds=158464)),
    case("b11-cut-in-three", 1, 9728, (2560,), 11, plan("generic", 4, 0, 4, 4, 16, launches=3, per=4, lds=158464)),
    case("b4-nv2", 1, 3072, (1024,), 4, plan("generic", 4, 2, 2, 4, 8)),
    case("b8-12-waves", 1, 3072, (1024,), 5, plan("generic", 8, 1, 1, 4, 12, lds=100352)),
    case("b8-loop-form", 0, 4608, (516,), 8, plan("generic", 8, 0, 2, 4, 16, lds=150528)),
    case("b8-rw32", 0, 256, (16384,), 7, plan("generic", 8, 1, 1, 32, 8)),
    case("b8-rw16-three-tensors", 0, 512, (8192, 4096, 4096), 5, plan("generic", 8, 1, 1, 16, 8)),
    case("b4-ragged-333x352", 1, 352, (333,), 3, plan("generic", 4, 1, 1, 4, 2)),
    case("b8-ragged-333x352", 0, 352, (333,), 7, plan("generic", 8, 1, 1, 4, 2)),
    case("b2-w13-no-norm", 2, 1024, (3072, 3072), 2, plan("generic", 2, 1, 2, 8, 8)),
    case("b8-w13-no-norm-upw4", 2, 2560, (1000, 1000), 5, plan("generic", 8, 1, 2, 4, 10)),
    case("b64-qkv-nano168", 0, 768, (768, 384, 384), 64, plan("generic", 8, 1, 1, 4, 3, launches=8, per=8)),
    case("b11-cls-151936x64", 0, 64, (151936,), 11, plan("generic", 8, 1, 1, 32, 8, launches=2, per=8)),
    # ---- norm cases ---------------------------------------------------------------------------------------------------------------
    case("qkv-nano168-norm", 0, 768, (768, 384, 384), 1, plan("norm_store", 1, 1, 1, 4, 3), norm=True),
    case("qkv-rw16-norm", 0, 512, (8192, 4096, 4096), 1, plan("norm_store", 1, 1, 1, 16, 8), norm=True),
    case("cls-151936x64-norm", 0, 64, (151936,), 1, plan("norm_store", 1, 1, 1, 32, 8), norm=True),
    case("w13-nano168-norm", 2, 768, (2048, 2048), 1, plan("norm_swiglu", 1, 1, 2, 8, 8), norm=True),
    case("w13-06b-norm-upw2", 2, 1024, (3072, 3072), 1, plan("norm_swiglu", 1, 1, 2, 8, 8), norm=True),
    case("w13-4b-norm-nv2-upw4", 2, 2560, (9728, 9728), 1, plan("norm_swiglu", 1, 2, 4, 4, 8), norm=True),
    case("store-norm-nv4-upw4", 0, 9728, (516,), 1, plan("norm_store", 1, 4, 4, 4, 10), norm=True),
    case("b4-qkv-norm-generic", 0, 768, (768, 384, 384), 3, plan("generic", 4, 1, 1, 4, 3), norm=True),
    case("b2-w13-norm-generic", 2, 1024, (3072, 3072), 2, plan("generic", 2, 1, 2, 8, 8), norm=True),
    case("b8-w13-norm-generic", 2, 768, (2048, 2048), 7, plan("generic", 8, 1, 2, 8, 8), norm=True),
    case("b4-norm-loop-form", 0, 9728, (516,), 4, plan("generic", 4, 0, 4, 4, 16, lds=158464), norm=True),
    case("b2-norm-nv4", 0, 9728, (516,), 2, plan("generic", 2, 4, 4, 4, 10), norm=True),
]


def query(c):
    attn = (c["comb"][0], c["comb"][1], len(c["comb"][2])) if c["comb"] else None
    return nb.f32_gemv_plan(c["kind"], c["n"], c["rows"], c["nb"], norm=c["norm"], attn=attn)


def build(c):
    """the inputs of a case: weights per tensor, activations (or attention partials), norm weight, old residual"""
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(c["id"])))
    n, nb_ = c["n"], c["nb"]
    if c["norm"]:
        W = [(0.02 * rng.standard_normal((r, n), dtype=np.float32)).astype(np.float32) for r in c["rows"]]
        nw = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    else:
        W = [exact_weights(rng, r, n) for r in c["rows"]]
        nw = None
    x, attn, amax, gran = order_free(rng, (nb_, n)), None, 2.0, 2.0 ** -4
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
        attn, amax, gran = (part, ml, n_head, hd), 2.0 * len(ls) / L, 2.0 ** -4 / L
    old = (rng.integers(-1024, 1025, size=(nb_, rows_total(c["kind"], c["rows"]))).astype(np.float32) / np.float32(256.0)) if c["kind"] == 1 else None
    if not c["norm"]:
        # exactness: every partial sum is a multiple of g = (2^-4 weights) x (activation granularity), the residual of 2^-8 >= g
        g, bound = 2.0 ** -4 * gran, n * 1.0 * amax + 4.0
        assert g <= 2.0 ** -8 and bound / g <= 2 ** 24, (c["id"], "inputs are not exact in fp32", bound / g)
    return dict(W=W, nw=nw, x=x, attn=attn, old=old)


def dot64(W, a, block=2048):
    """float64 dot of every row with a, and S = sum |w_i a_i|"""
    a = a.astype(np.float64)
    ref, S = np.empty(W.shape[0]), np.empty(W.shape[0])
    for r0 in range(0, W.shape[0], block):
        w = W[r0:r0 + block].astype(np.float64)
        ref[r0:r0 + block] = w @ a
        S[r0:r0 + block] = np.abs(w) @ np.abs(a)
    return ref, S


def row_bound(ref, S, n):
    return (10 + (n + 255) // 256) * U * S + U * np.abs(ref)


def emulate_f32(W, a, block=512):
    """the kernel's order in numpy fp32: per 256-float chunk a lane's float4 (multiply, three fused multiply-adds), a pairwise tree over
    the 64 lanes, then the chunk sums added in ascending order.  (A fused multiply-add is the exact float64 product plus the float64
    sum rounded to fp32 -- a double rounding in rare cases, which an estimate of the error's size does not mind.)"""
    rows, n = W.shape
    nchunk = (n + 255) // 256
    ap = np.zeros(nchunk * 256, np.float32); ap[:n] = a
    a4 = ap.reshape(nchunk, 64, 4)
    out = np.empty(rows, np.float32)
    for r0 in range(0, rows, block):
        w = np.zeros((min(block, rows - r0), nchunk * 256), np.float32); w[:, :n] = W[r0:r0 + block]
        w4 = w.reshape(-1, nchunk, 64, 4)
        p = w4[..., 0] * a4[..., 0]
        for k in (1, 2, 3):
            p = (w4[..., k].astype(np.float64) * a4[..., k].astype(np.float64) + p.astype(np.float64)).astype(np.float32)
        while p.shape[-1] > 1:
            p = p[..., 0::2] + p[..., 1::2]
        p = p[..., 0]
        v = np.zeros(p.shape[0], np.float32)
        for ch in range(nchunk):
            v = v + p[:, ch]
        out[r0:r0 + block] = v
    return out


def swiglu_bound(h1, S1, h3, S3, n):
    e1, e3 = row_bound(h1, S1, n), row_bound(h3, S3, n)
    silu = h1 / (1.0 + np.exp(-h1))
    return silu * h3, 1.1 * e1 * np.abs(h3) + np.abs(silu) * e3 + 1.1 * e1 * e3 + 3e-6 * np.abs(silu * h3)


def launch(c, I, sl=None):
    """the case's launch, or with sl = b the same launch of sequence b alone; the batched launch runs in a guarded buffer"""
    weights = [(w, None, w.shape[0]) for w in I["W"]]
    rt = rows_total(c["kind"], c["rows"])
    if sl is not None:
        b = slice(sl, sl + 1)
        attn = (I["attn"][0][b], I["attn"][1][b], I["attn"][2], I["attn"][3]) if I["attn"] else None
        return nb.op_fused_gemv(F32, c["kind"], c["n"], weights, None if attn else I["x"][b], I["nw"], nb=1,
                                resid=I["old"][b] if I["old"] is not None else None, attn=attn)[0]
    g = np.full((c["nb"] + 8, rt + 1), SENTINEL, np.float32)
    if I["old"] is not None:
        g[:c["nb"], :rt] = I["old"]
    nb.op_fused_gemv(F32, c["kind"], c["n"], weights, None if I["attn"] else I["x"], I["nw"], nb=c["nb"], attn=I["attn"], guard=g)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES)
def test_f32_gemv_plan_case(oracle, c):
    q = query(c)
    assert q["takes"] == 1, (c["id"], "the router refuses this shape: nothing is launched", q)
    I = build(c)
    kind, n, nb_, rt = c["kind"], c["n"], c["nb"], rows_total(c["kind"], c["rows"])
    g = launch(c, I)
    out = g[:nb_, :rt]
    errors = []
    # 1. values
    worst = 0.0
    for b in range(nb_):
        a = oracle.rmsnorm(I["x"][b], I["nw"]) if c["norm"] else I["x"][b]
        refs = [dot64(w, a) for w in I["W"]]
        if not c["norm"]:
            if kind == 2:
                h1, h3 = refs[0][0].astype(np.float32), refs[1][0].astype(np.float32)
                assert np.array_equal(h1.astype(np.float64), refs[0][0]) and np.array_equal(h3.astype(np.float64), refs[1][0])
                want = silu_mul(h1, h3)
                if not np.allclose(out[b], want, rtol=3e-6, atol=1e-9):
                    errors.append(f"sequence {b}: SwiGLU of exact h1, h3 off by {np.abs(out[b] - want).max():.3e}")
                continue
            ref = np.concatenate([r for r, _ in refs])
            if kind == 1:
                ref = ref + I["old"][b].astype(np.float64)
            want = ref.astype(np.float32)
            assert np.array_equal(want.astype(np.float64), ref), "the reference itself is not exact in fp32"
            bad = np.flatnonzero(bits(out[b]) != bits(want))
            if bad.size:
                errors.append(f"sequence {b}: {bad.size} of {rt} rows differ from the exact result, first rows {bad[:6]}, worst |d| {np.abs(out[b] - want).max():.3e}")
            continue
        if kind == 2:
            ref, bound = swiglu_bound(refs[0][0], refs[0][1], refs[1][0], refs[1][1], n)
        else:
            ref = np.concatenate([r for r, _ in refs]); S = np.concatenate([s for _, s in refs])
            bound = row_bound(ref, S, n)
        d = np.abs(out[b].astype(np.float64) - ref)
        worst = max(worst, float((d / bound).max()))
        glob = float(d.max() / np.abs(ref).max())
        print(f"{c['id']} sequence {b}: worst |d| / bound {float((d / bound).max()):.3f}, max|d| / max|ref| {glob:.2e}")
        bad = np.flatnonzero(d > bound)
        if bad.size:
            errors.append(f"sequence {b}: {bad.size} of {rt} rows beyond the per-row bound, first rows {bad[:6]}, worst ratio {float((d / bound).max()):.2f}")
        if not glob <= 1e-5:
            errors.append(f"sequence {b}: max|d| / max|ref| = {glob:.3e}")
    assert not errors, f"{c['id']} (plan {q}): " + "; ".join(errors[:4])
    # 2. nothing written beyond a sequence's rows or beyond the batch
    assert np.all(bits(g[:, rt]) == bits(SENTINEL)), "a guard element behind a sequence's rows changed"
    assert np.all(bits(g[nb_:]) == bits(SENTINEL)), f"slots beyond the batch were written: slots {np.flatnonzero((bits(g[nb_:]) != bits(SENTINEL)).any(axis=1)) + nb_}"
    # 3. a batch is its sequences alone
    if nb_ > 1:
        for b in range(nb_):
            alone = launch(c, I, sl=b)
            assert np.array_equal(bits(out[b]), bits(alone)), (c["id"], "sequence", b, "differs from its launch alone", float(np.abs(out[b] - alone).max()))
    # 4. the plan, last
    got = {k: q[k] for k in c["target"]}
    assert got == c["target"], f"{c['id']}: the launcher's plan is {q}, the case means {c['target']}: a retune moved this case -- pick a new shape for this target"


def test_bound_against_the_emulated_order(oracle):
    """CPU: the per-row bound of the norm cases holds for a numpy fp32 emulation of the kernel's summation order on the cases' own
    inputs (first sequence), with the slack the docstring records"""
    worst = {}
    for p in CASES:
        c = p.values[0]
        if not c["norm"]:
            continue
        I = build(c)
        a = oracle.rmsnorm(I["x"][0], I["nw"])
        for w in I["W"]:
            ref, S = dot64(w, a)
            r = np.abs(emulate_f32(w, a).astype(np.float64) - ref) / row_bound(ref, S, c["n"])
            worst[c["id"]] = max(worst.get(c["id"], 0.0), float(r.max()))
    print({k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    assert max(worst.values()) > 0.01, "the emulation is not exercising the rounding it is meant to"


def test_exact_inputs_make_the_emulated_order_exact():
    """CPU: on the exact cases' inputs the kernel's order and float64 are the same number (the claim the bit-for-bit cases rest on)"""
    for cid in ("w2-06b-nv2", "ragged-333x352", "combine-nano168-8"):
        c = next(p.values[0] for p in CASES if p.values[0]["id"] == cid)
        I = build(c)
        ref, _ = dot64(I["W"][0], I["x"][0])
        assert np.array_equal(emulate_f32(I["W"][0], I["x"][0]).astype(np.float64), ref), cid


def test_cases_cover_every_plan_axis():
    """The cases reach every choice the planner and the router can make -- read from the plans the query reports (CPU-only), which each
    case's own test also holds against the plan the case states."""
    T = []
    for p in CASES:
        c = p.values[0]
        q = query(c)
        assert q["takes"] == 1, c["id"]
        assert {k: q[k] for k in c["target"]} == c["target"], (c["id"], q)
        T.append(dict(q, id=c["id"], kind=c["kind"], n=c["n"], rows=c["rows"], nb=c["nb"], norm=c["norm"], comb=c["comb"] is not None,
                      total=rows_total(c["kind"], c["rows"])))

    def has(f=None, **kw):
        return any(all(t[k] == v for k, v in kw.items()) and (f is None or f(t)) for t in T)

    for role in nb.F32_ROLES:
        assert has(role=ROLE[role]), role
    for B in (1, 2, 4, 8):
        assert has(B=B), B
    for nv in (0, 1, 2, 4):
        assert has(nv=nv), nv
    for upw in (1, 2, 4):
        assert has(upw=upw), upw
    for B, nv in ((1, 1), (1, 2), (1, 4), (2, 1), (2, 4), (4, 0), (4, 1), (4, 2), (8, 0), (8, 1)):
        assert has(B=B, nv=nv), (B, nv)
    for rw in (4, 8, 16, 32):
        assert has(rw=rw), rw
        assert has(rw=rw, f=lambda t: t["B"] > 1), rw
    assert has(f=lambda t: t["nw"] >= 9) and has(nw=16) and has(nw=2)
    assert has(f=lambda t: t["lds_bytes"] > 65536 and t["B"] == 1) and has(f=lambda t: t["lds_bytes"] > 65536 and t["B"] > 1)
    assert has(f=lambda t: len(t["rows"]) == 1 and t["total"] % 4 and t["total"] % t["rw"])                 # a ragged last workgroup
    assert has(f=lambda t: len(t["rows"]) == 1 and t["total"] % 4 and t["B"] == 4) and has(f=lambda t: len(t["rows"]) == 1 and t["total"] % 4 and t["B"] == 8)
    assert has(f=lambda t: t["n"] % 256 != 0) and has(f=lambda t: t["n"] % 256 != 0 and t["n"] > 256)
    assert has(kind=0, f=lambda t: len(t["rows"]) == 3) and has(kind=0, f=lambda t: len(t["rows"]) == 3 and t["B"] == 8)
    assert has(n=64, f=lambda t: t["total"] == 151936 and t["norm"]) and has(n=64, f=lambda t: t["total"] == 151936 and t["nb"] > 8)
    for nb_, B in ((3, 4), (5, 8), (7, 8)):
        assert has(nb=nb_, B=B), (nb_, B)                                                                 # dead batch slots
    assert has(nb=11, f=lambda t: t["launches"] > 1) and has(nb=64, launches=8)
    assert has(n=9728, nb=8, launches=2, seqs_per_launch=4, f=lambda t: t["rows"] == (2560,))             # a batch the LDS fit rule cuts
    # the loop form and the register forms, each with a norm, with the combine, and plain; SwiGLU at every UPW
    for nv0 in (True, False):
        assert has(norm=True, f=lambda t: (t["nv"] == 0) == nv0) and has(comb=True, f=lambda t: (t["nv"] == 0) == nv0)
    assert has(comb=True, B=1, nv=2) and has(comb=True, B=4)
    assert has(kind=2, upw=2) and has(kind=2, upw=4) and has(kind=2, norm=True, B=8) and has(kind=2, norm=False, B=8)
    # the table of the shapes the planner was written for
    for n, rows, kw in ((768, (768, 384, 384), dict(nv=1, upw=1)), (1024, (3072, 3072), dict(upw=2)), (3072, (1024,), dict(nv=2)),
                        (2560, (9728, 9728), dict(nv=2, upw=4)), (9728, (2560,), dict(nv=4, upw=4, nb=1)), (9728, (2560,), dict(nv=0, nb=4)),
                        (12288, (512,), dict(nw=12)), (256, (16384,), dict(rw=32)), (512, (8192, 4096, 4096), dict(rw=16))):
        assert has(n=n, rows=rows, **kw), (n, rows, kw)
