"""Every form of the two fused one-sequence launches on caller inputs, bit for bit against the plain launches they replace.

nb.op_qkv_attn_fused and nb.op_wo_w13_fused run ONE fused launch exactly as a decode step issues it (granule buffer and tick words from the
model's own code, the epoch opened as the embed kernel opens it) and report the plan that ran.  tests/test_fused_launch_plan.py sweeps the
planners on the CPU: UNIVERSE is the set of forms a shape can reach, SMALLEST the smallest shape of each.  Here there is one case per
form at that shape, and a closing coverage test that fails when a retune makes a form reachable without a case or moves a case off its form.

What a q | k | v + attention case checks, values first (a moved plan must not hide a wrong value):
  * THE PLAIN SIDE, anchored on its own: nb.op_fused_gemv(kind 0) gives q | k | v -- Q80 (order-free activations: the rmsnorm is exact)
    bit for bit tests/canon.py's fold of the oracle's quantization, Q4K bit for bit the oracle's matmul_q4k, FP32 inside the per-row
    float64 bound of test_gpu_f32_gemv.py; nb.op_attention_decode on those rows gives the finished k row within K_TOL = 2e-6 of the float64
    rmsnorm + RoPE and the head outputs within ATTN_TOL = 1e-5 of the float64 attention over the cache the kernel read
    (test_gpu_attention_decode.py's reference, imported);
  * THE FUSED LAUNCH equals it bit for bit: the q and k rows it stored, every element of both caches (two layers, rows beyond the range:
    "nothing else written" is part of the comparison), the head outputs (several splits: the combined partials); the error word is 0.
Rows in (pos, range_hint) hold finite stale values of +-1e4, as in the attention suite.
A Wo + W1|W3 case: the fused launch equals nb.op_fused_gemv(kind 1) followed by nb.op_fused_gemv(kind 2) on its result, residual stream and
hb, bit for bit; the residual stream equals old + the canonical fold bit for bit; and -- the old residual chosen so that the new stream is
order-free, hence its rmsnorm exact -- hb is within rtol 3e-6, atol 1e-9 (test_gpu_fused_roles.py's SwiGLU bar: the device's expf) of
silu_mul of the two reference projections.

Attention-side edges (the smallest Q80 and FP32 shapes that bring the heads): the fresh row first and last of a block, in the second
split, in the last of 3 / 5 / 8 splits; head ratios 1, 2, 4, 8 on 1 and on 8 KV heads (both workgroup orders of kv_log2); one dominant
score at row 0, at the last row of the first block, at pos (the fresh row, which reaches the attention as granules and not through the
cache: a rank-one Wk, and for Q80 a k_norm weight scaled so that the normalised row still dominates); the smallest FP32 shape itself
(head_dim 4) at 2 and 8 splits.  Hand-off edges (one case per family): the granule buffer pre-filled with
values of +-1e4 under the tags of the previous step, of the previous layer and all ones; layer1 1 and 126; the tag wrapping through 0 --
results bit for bit those of the clean run.  Refusals: one shape just outside each predicate -- the query says takes = 0 and the operator
returns its argument error before any launch.  No case forces a give-up, sets a fault or repeats a launch to provoke one."""
import math

import numpy as np
import pytest

from nano_amd import binding as nb
from fused_ref import bits, order_free, silu_mul
from test_fused_launch_plan import UNIVERSE, SMALLEST, F32, Q80, Q4K, R_RESID, R_COMBINE, qkv_form, wo13_form, qkv_weight_bytes
from test_gpu_attention_decode import ATTN_TOL, K_TOL, STALE, finish64, rope64, rope_tables, attend64      # (rmsnorm64 through finish64)
from test_gpu_f32_gemv import dot64, row_bound
from test_gpu_fused_roles import q80_weights, ref_q80
from test_gpu_q4k_gemv import pool

gpu = pytest.mark.gpu

LAYERS, LAYER = 2, 1        # the cases write layer 1 of a two-layer cache
BLOCK = 32                  # timestep rows of a block (attn_impl.h: 256 threads / 8 lanes per row)
QUANT_OF = {"q80_table": Q80, "q80_wf": Q80, "q4k": Q4K, "f32": F32}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def projection(oracle, quant, n, rows, rng):
    """weights as the operators take them, x, norm weight, and a function act -> the reference q | k | v (FP32: the float64 dot and its bound)"""
    x = order_free(rng, n)
    nw = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    a = oracle.rmsnorm(x, nw)                                            # exact: the activations are order-free
    if quant == Q80:
        W = [(*q80_weights(rng, r, n, 64), r) for r in rows]
        return dict(W=W, x=x, nw=nw, a=a, gs=64, ref=lambda W: ref_q80(oracle, a, W, n, 64, canon=True))
    if quant == Q4K:
        T, blocks = pool(oracle, n)
        xT = oracle.quantize_q4k(a, [n])
        pool_ref = oracle.matmul_q4k(xT, T, 0, blocks.shape[0])
        idx = [rng.integers(0, blocks.shape[0], size=r) for r in rows]
        W = [(np.ascontiguousarray(blocks[i]), None, int(i.size)) for i in idx]
        return dict(W=W, x=x, nw=nw, a=a, gs=0, ref=lambda W: np.concatenate([pool_ref[i] for i in idx]))
    W = [((0.02 * rng.standard_normal((r, n), dtype=np.float32)).astype(np.float32), None, r) for r in rows]
    return dict(W=W, x=x, nw=nw, a=a, gs=0, ref=lambda W: np.concatenate([dot64(w, a)[0] for w, _, _ in W]))


def run_qkv(oracle, quant, shape, *, pos, nsplit=1, rh=64, seed=0, peak=None, want=None, **hand):
    """one q | k | v + attention case; returns the fused operator's result"""
    n, H, KVH, hd = shape
    qwen3 = quant != F32
    QD, KD = H * hd, KVH * hd
    rng = np.random.default_rng(seed + 1000 * n + 7 * H + KVH + hd)
    S = rh + 5
    P = projection(oracle, quant, n, (QD, KD, KD), rng)
    qn = rng.uniform(0.5, 1.5, hd).astype(np.float32) if qwen3 else None
    kn = rng.uniform(0.5, 1.5, hd).astype(np.float32) if qwen3 else None
    cos, sin = rope_tables(S, hd, 1e6 if qwen3 else 1e4)
    kc = rng.standard_normal((LAYERS, S, KD)).astype(np.float32); vc = rng.standard_normal((LAYERS, S, KD)).astype(np.float32)
    for t in range(pos + 1, rh):                                         # stale rows inside the hinted range, beyond pos
        sign = np.where(rng.random(KD) < 0.5, -1.0, 1.0)
        kc[LAYER, t] = (STALE * sign).astype(np.float32); vc[LAYER, t] = (-STALE * sign).astype(np.float32)
    if peak is not None:                                                 # one dominant row: every head's score there is >= 7
        qraw = np.asarray(P["ref"](P["W"])[:QD], np.float64)
        qf = finish64(qraw.reshape(H, hd), qn if qwen3 else 1.0, cos[pos], sin[pos], qwen3).reshape(KVH, H // KVH, hd)
        u = qf.sum(axis=1); u /= np.linalg.norm(u, axis=-1, keepdims=True)
        kappa = 7.0 * math.sqrt(hd) / np.einsum("gmd,gd->gm", qf, u).min(axis=1)
        target = kappa[:, None] * u
        if peak == "pos":                                                # the fresh row, which reaches the attention as granules: Wk of rank one
            assert quant in (F32, Q80)
            a64 = P["a"].astype(np.float64)
            if not qwen3:                                                # raw k = the target with its RoPE undone
                kraw = rope64(target, cos[pos], -sin[pos], False).reshape(KD)
                P["W"][1] = (np.outer(kraw, a64 / (a64 @ a64)).astype(np.float32), None, KD)
            else:
                # Qwen3's body: finished k = RoPE(k_norm * raw / rms(raw)) -- the raw row fixes the direction only.  raw = (u with its
                # RoPE undone) / k_norm per head; then finished = u / rms(raw), and a k_norm weight times c = 1.1 max kappa rms(raw)
                # makes every head's finished row at least kappa u: every score at pos is >= 7 (the dominance assertion below checks it).
                # Rank-one rows quantize to the same integers times the row's own scale: the direction survives Q80.
                t = rope64(u, cos[pos], -sin[pos], True) / kn.astype(np.float64)
                kn = (kn.astype(np.float64) * 1.1 * float((kappa * np.sqrt(np.mean(t * t, axis=-1))).max())).astype(np.float32)
                Wk = np.outer(t.reshape(KD), a64 / (a64 @ a64)).reshape(KD, n // 64, 64)
                ws = (np.abs(Wk).max(axis=-1) / 127.0).astype(np.float32)
                assert ws.min() > 0
                wq = np.rint(Wk / ws[..., None].astype(np.float64)).astype(np.int8)
                P["W"][1] = (wq.reshape(-1), ws.reshape(-1), KD)
        else:
            assert peak <= pos
            kc[LAYER, peak] = target.reshape(KD).astype(np.float32)
    W, x, nw = P["W"], P["x"], P["nw"]
    ref = P["ref"](W)
    errors = []
    # 1. the plain projection, against the oracle / float64
    qkv = nb.op_fused_gemv(quant, 0, n, W, x[None], nw, gs=P["gs"])[0]
    if quant == F32:
        S_ = np.concatenate([dot64(w, P["a"])[1] for w, _, _ in W])
        d = np.abs(qkv.astype(np.float64) - ref)
        print(f"{shape}: plain q|k|v worst |d| / bound {float((d / row_bound(ref, S_, n)).max()):.3f}, max|d| / max|ref| {float(d.max() / np.abs(ref).max()):.2e}")
        if (d > row_bound(ref, S_, n)).any() or not d.max() / np.abs(ref).max() <= 1e-5:
            errors.append(f"plain q|k|v beyond the float64 bound at rows {np.flatnonzero(d > row_bound(ref, S_, n))[:6]}")
    elif not np.array_equal(bits(qkv), bits(ref)):
        errors.append(f"plain q|k|v differs from the reference at rows {np.flatnonzero(bits(qkv) != bits(ref))[:6]}")
    q, k, v = qkv[:QD], qkv[QD:QD + KD], qkv[QD + KD:]
    # 2. the plain attention on those rows, against float64
    vin = vc.copy(); vin[LAYER, pos] = v                                 # (the plain projection stores v straight into its cache row)
    kw = dict(n_head=H, n_kv_head=KVH, hd=hd, S=S, range_hint=rh, rope_cos=cos, rope_sin=sin, rope_qwen3=qwen3, q_norm=qn, k_norm=kn, nsplit=nsplit)
    plain = nb.op_attention_decode(q[None], k[None], [pos], kc[None], vin[None], n_layer=LAYERS, layer=LAYER, **kw)
    pk, pv = plain["k_cache"].reshape(LAYERS, S, KD), plain["v_cache"].reshape(LAYERS, S, KD)
    kref = finish64(k.reshape(KVH, hd), kn if qwen3 else 1.0, cos[pos], sin[pos], qwen3).reshape(KD)
    if (np.abs(pk[LAYER, pos] - kref) > K_TOL * np.abs(kref).max()).any():
        errors.append(f"plain k row off by {np.abs(pk[LAYER, pos] - kref).max():.3e}")
    K = pk[LAYER, :pos + 1].astype(np.float64).reshape(pos + 1, KVH, hd); V = pv[LAYER, :pos + 1].astype(np.float64).reshape(pos + 1, KVH, hd)
    qf = finish64(q.reshape(H, hd), qn if qwen3 else 1.0, cos[pos], sin[pos], qwen3)
    aref = attend64(qf, K, V, H // KVH)
    err = np.abs(plain["out"][0] - aref).max() / np.abs(aref).max()
    if not err <= ATTN_TOL:
        errors.append(f"plain head outputs max|d| / max|ref| = {err:.3e}")
    if peak is not None:
        t = pos if peak == "pos" else peak
        keep = [i for i in range(pos + 1) if i != t]
        assert not keep or np.abs(attend64(qf, K[keep], V[keep], H // KVH) - aref).max() / np.abs(aref).max() > 1e-2, "the peak row does not dominate"
    kexp = kc.copy(); kexp[LAYER, pos] = pk[LAYER, pos]
    if not (np.array_equal(bits(pk), bits(kexp)) and np.array_equal(bits(pv), bits(vin))):
        errors.append("the plain attention wrote outside the fresh k row")
    # 3. the fused launch: the same bits everywhere
    fused = nb.op_qkv_attn_fused(quant, n, W, x, nw, pos, kc, vc, gs=P["gs"], n_layer=LAYERS, layer=LAYER, **kw, **hand)
    fk, fv = fused["k_cache"].reshape(LAYERS, S, KD), fused["v_cache"].reshape(LAYERS, S, KD)
    for name, got, exp in (("q", fused["q"], q), ("raw k", fused["k"], k), ("k cache", fk, pk), ("v cache", fv, pv), ("head outputs", fused["out"], plain["out"][0])):
        bad = np.flatnonzero(bits(got).reshape(-1) != bits(exp).reshape(-1))
        if bad.size:
            errors.append(f"fused {name} differs from the plain launches at {bad.size} elements, first {bad[:6]}, worst |d| "
                          f"{np.nanmax(np.abs(np.asarray(got, np.float64) - np.asarray(exp, np.float64))):.3e}")
    if fused["err"]:
        errors.append(f"error word {fused['err']}")
    assert not errors, f"{shape} pos {pos} nsplit {nsplit} range_hint {rh} (plan {fused['plan']}): " + "; ".join(errors)
    assert fused["plan"]["n_attn"] == H * nsplit
    # 4. the plan, last
    if want is not None:
        assert qkv_form(fused["plan"]) == want, f"ran {qkv_form(fused['plan'])}, the case means {want}: a retune moved this case -- SMALLEST names its new shape"
    return fused


def exact_combine(rng, n, n_head, ls):
    """split-attention partials whose combination is exact: equal maxima, sums that add up to a power of two (test_gpu_fused_roles.py)"""
    L = sum(ls)
    assert L & (L - 1) == 0
    part = order_free(rng, (len(ls), n))
    ml = np.zeros((n_head, len(ls), 2), np.float32)
    ml[..., 0] = 0.25
    ml[..., 1] = np.asarray(ls, np.float32)
    x = (part.astype(np.float64).sum(axis=0) / L).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), part.astype(np.float64).sum(axis=0) / L)
    return part, ml, x


def run_wo13(oracle, shape, *, seed=0, want=None, **hand):
    n_wo, E, hidden, splits = shape
    rng = np.random.default_rng(seed + n_wo + 3 * E + hidden + splits)
    wq, ws = q80_weights(rng, E, n_wo, 64)
    w1, w3 = (*q80_weights(rng, hidden, E, 64), hidden), (*q80_weights(rng, hidden, E, 64), hidden)
    nw = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    attn = None
    if splits > 1:
        part, ml, x = exact_combine(rng, n_wo, n_wo // 128, (3, 5) if splits == 2 else (1,) * splits)
        attn = (part, ml, n_wo // 128, 128)
    else:
        x = order_free(rng, n_wo)
    # Wo's scales times a power of two that brings the rms of its result to about 1/2: the new stream is neither mostly zero nor large
    rms = float(np.sqrt(np.mean(ref_q80(oracle, x, [(wq, ws, E)], n_wo, 64, canon=True).astype(np.float64) ** 2)))
    wo = (wq, (ws * np.float32(2.0 ** round(math.log2(0.5 / rms)))).astype(np.float32), E)
    wo_ref = ref_q80(oracle, x, [wo], n_wo, 64, canon=True)
    # the old residual that makes the new stream order-free: the nearest multiple of 2^-4, and the sum exact in fp32
    new = (np.round(wo_ref.astype(np.float64) * 16) / 16).astype(np.float32)
    old = (new.astype(np.float64) - wo_ref.astype(np.float64)).astype(np.float32)
    assert E * (float(np.abs(new).max()) * 16) ** 2 <= 2 ** 24, "the new stream's sum of squares (in units of 2^-8) is not exact in any order"
    assert np.array_equal(bits((old + wo_ref).astype(np.float32) + np.float32(0)), bits(new + np.float32(0))), "the residual add is not exact"
    assert np.count_nonzero(new) > E // 2, "the new stream is mostly zero"
    xn = oracle.rmsnorm(new, nw)
    hb_ref = silu_mul(ref_q80(oracle, xn, [w1], E, 64, canon=True), ref_q80(oracle, xn, [w3], E, 64, canon=True))
    errors = []
    # 1. the two plain launches, against the references
    px = nb.op_fused_gemv(Q80, 1, n_wo, [wo], None if attn else x[None], None, gs=64, resid=old[None],
                          attn=None if attn is None else (attn[0][None], attn[1][None], attn[2], attn[3]))[0]
    if not np.array_equal(bits(px + np.float32(0)), bits(new + np.float32(0))):
        errors.append(f"plain Wo differs from old + the canonical fold at rows {np.flatnonzero(bits(px) != bits(new))[:6]}")
    phb = nb.op_fused_gemv(Q80, 2, E, [w1, w3], px[None], nw, gs=64)[0]
    if not np.allclose(phb, hb_ref, rtol=3e-6, atol=1e-9):
        errors.append(f"plain SwiGLU off by {np.abs(phb - hb_ref).max():.3e}")
    # 2. the fused launch: the same bits
    fused = nb.op_wo_w13_fused(n_wo, wo, w1, w3, old, nw, x=None if attn else x, attn=attn, **hand)
    for name, got, exp in (("residual stream", fused["x"], px), ("hb", fused["hb"], phb)):
        bad = np.flatnonzero(bits(got) != bits(exp))
        if bad.size:
            errors.append(f"fused {name} differs from the plain launches at {bad.size} rows, first {bad[:6]}, worst |d| {np.abs(got - exp).max():.3e}")
    if fused["err"]:
        errors.append(f"error word {fused['err']}")
    assert not errors, f"{shape} (plan {fused['plan']}): " + "; ".join(errors)
    # 3. the plan, last
    if want is not None:
        assert wo13_form(fused["plan"]) == want, f"ran {wo13_form(fused['plan'])}, the case means {want}: a retune moved this case -- SMALLEST names its new shape"
    return fused


# ---- one case per reachable form, at the smallest shape the sweep meets it at ------------------------------------------------------------
QKV_FORMS = sorted(f for f in UNIVERSE if f[0] != "wo_w13")
WO13_FORMS = sorted(f for f in UNIVERSE if f[0] == "wo_w13")


@gpu
@pytest.mark.parametrize("form", QKV_FORMS, ids=lambda f: "-".join(map(str, f)))
def test_qkv_attn_fused_form(oracle, form):
    run_qkv(oracle, QUANT_OF[form[0]], SMALLEST[form], pos=37, nsplit=1, rh=64, want=form)


@gpu
@pytest.mark.parametrize("form", WO13_FORMS, ids=lambda f: "-".join(map(str, f)))
def test_wo_w13_fused_form(oracle, form):
    run_wo13(oracle, SMALLEST[form], want=form)


def test_cases_cover_every_reachable_form():
    """CPU arithmetic: every form of UNIVERSE has its case, and the case's shape still plans to that form"""
    assert set(QKV_FORMS) | set(WO13_FORMS) == set(UNIVERSE) == set(SMALLEST)
    for f in QKV_FORMS:
        n, H, KVH, hd = SMALLEST[f]
        assert qkv_form(nb.qkv_attn_fused_plan(QUANT_OF[f[0]], n, H, KVH, hd, range_hint=64, nsplit=1)) == f, f
    for f in WO13_FORMS:
        n_wo, E, hidden, splits = SMALLEST[f]
        assert wo13_form(nb.wo_w13_fused_plan(n_wo, E, hidden, attn=(n_wo // 128, 128, splits) if splits > 1 else None)) == f, f
        assert (f[2] == R_COMBINE) == (splits > 1)


# ---- attention-side edges ----------------------------------------------------------------------------------------------------------------
def smallest_taking(quant, ratio, n_kv, hd):
    """the smallest shape (weight bytes) with these heads that the fused launch takes"""
    best = None
    for n in range(64, 4097, 64):
        if nb.qkv_attn_fused_plan(quant, n, n_kv * ratio, n_kv, hd, range_hint=64, nsplit=1)["takes"]:
            key = (qkv_weight_bytes(quant, n, n_kv * ratio, n_kv, hd), n)
            best = key if best is None or key < best else best
    assert best is not None, (quant, ratio, n_kv, hd, "no row length takes these heads")
    return (best[1], n_kv * ratio, n_kv, hd)


EDGE_BASE = {Q80: SMALLEST[("q80_table", 1, 1)], F32: (64, 8, 4, 32)}     # (FP32: the smallest row length, heads and a head_dim that fill the blocks' lanes)
POSITIONS = [(0, 1, 64), (31, 1, 64), (32, 1, 64), (63, 1, 64),            # the fresh row first / last of a block, nothing stale behind it
             (64, 2, 128), (127, 2, 128),                                  # ... first / last of the second split's block
             (3 * 64 - 3, 3, 3 * 64), (5 * 64 - 3, 5, 5 * 64), (8 * 64 - 3, 8, 8 * 64)]      # pos in the last split, stale rows behind it


@gpu
@pytest.mark.parametrize("quant", [Q80, F32], ids=["q80", "f32"])
@pytest.mark.parametrize("pos,nsplit,rh", POSITIONS)
def test_attention_edges_positions_and_splits(oracle, quant, pos, nsplit, rh):
    run_qkv(oracle, quant, EDGE_BASE[quant], pos=pos, nsplit=nsplit, rh=rh, seed=pos)


@gpu
@pytest.mark.parametrize("pos,nsplit,rh", [(127, 2, 128), (8 * 64 - 3, 8, 8 * 64)])
def test_attention_edges_smallest_fp32_shape(oracle, pos, nsplit, rh):
    """the smallest FP32 shape itself -- one head of head_dim 4, a lane's float4 the whole row -- at several splits (the edges above run
    on head_dim 32, which fills a block's lanes)"""
    run_qkv(oracle, F32, SMALLEST[("f32", 1, 1)], pos=pos, nsplit=nsplit, rh=rh, seed=pos)


@gpu
@pytest.mark.parametrize("quant", [Q80, F32], ids=["q80", "f32"])
@pytest.mark.parametrize("n_kv", [1, 8])
@pytest.mark.parametrize("ratio", [1, 2, 4, 8])
def test_attention_edges_head_ratios(oracle, quant, ratio, n_kv):
    """both branches of kv_log2 (n_kv_head 1: plain order; 8: the XCD order) at every head ratio, two splits, stale rows behind pos"""
    shape = smallest_taking(quant, ratio, n_kv, 128 if quant == Q80 else 16)
    run_qkv(oracle, quant, shape, pos=100, nsplit=2, rh=128, seed=ratio)


@gpu
@pytest.mark.parametrize("quant,peak", [(Q80, 0), (Q80, BLOCK - 1), (Q80, "pos"), (F32, 0), (F32, BLOCK - 1), (F32, "pos")], ids=lambda v: str(v))
def test_attention_edges_dominant_row(oracle, quant, peak):
    run_qkv(oracle, quant, EDGE_BASE[quant], pos=70, nsplit=2, rh=128, seed=5, peak=peak)


# ---- hand-off edges ----------------------------------------------------------------------------------------------------------------------
def stale_granules(rng, count, tick0, layer1):
    """granules of other epochs with values of +-1e4: the previous step on this layer, this step on the previous layer, all ones"""
    waited = ((tick0 + 1) * 128 + layer1) & 0xffffffff
    tags = np.array([(tick0 * 128 + layer1) & 0xffffffff, ((tick0 + 1) * 128 + layer1 - 1) & 0xffffffff, 0xffffffff], np.uint64)
    assert waited not in tags.tolist(), "never the tag the launch itself waits for"
    val = np.where(rng.random(count) < 0.5, -STALE, STALE).astype(np.float32).view(np.uint32).astype(np.uint64)
    return (tags[rng.integers(0, 3, count)] << np.uint64(32)) | val


HANDOFF = [(1, 0), (126, 41), (1, 2 ** 25 - 1), (126, 2 ** 25 - 1)]           # (layer1, tick0); 2^25 - 1: the step's tag wraps through 0


@gpu
@pytest.mark.parametrize("form", [("q80_table", 2, 1), ("q80_wf", 1, 1), ("q4k", 1, 1), ("f32", 1, 2)], ids=lambda f: "-".join(map(str, f)))
def test_qkv_attn_handoff_edges(oracle, form):
    quant, shape = QUANT_OF[form[0]], SMALLEST[form]
    n, H, KVH, hd = shape
    clean = run_qkv(oracle, quant, shape, pos=37, want=form)
    for layer1, tick0 in HANDOFF:
        init = stale_granules(np.random.default_rng(layer1 + tick0 % 1000), (H + 2 * KVH) * hd, tick0, layer1)
        got = run_qkv(oracle, quant, shape, pos=37, want=form, layer1=layer1, tick0=tick0, hand_init=init)
        for key in ("out", "k_cache", "v_cache", "q", "k"):
            assert np.array_equal(bits(got[key]), bits(clean[key])), (form, layer1, tick0, key)
        assert got["err"] == 0


@gpu
@pytest.mark.parametrize("form", [("wo_w13", 3, R_RESID, 0, 0), ("wo_w13", 3, R_RESID, 1, 2), ("wo_w13", 3, R_COMBINE, 1, 0)], ids=lambda f: "-".join(map(str, f)))
def test_wo_w13_handoff_edges(oracle, form):
    shape = SMALLEST[form]
    clean = run_wo13(oracle, shape, want=form)
    for layer1, tick0 in HANDOFF:
        init = stale_granules(np.random.default_rng(layer1 + tick0 % 1000), shape[1], tick0, layer1)
        got = run_wo13(oracle, shape, want=form, layer1=layer1, tick0=tick0, hand_init=init)
        assert np.array_equal(bits(got["x"]), bits(clean["x"])) and np.array_equal(bits(got["hb"]), bits(clean["hb"])) and got["err"] == 0, (form, layer1, tick0)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def refused_qkv(oracle, quant, shape, nsplit, rh):
    n, H, KVH, hd = shape
    qwen3 = quant != F32
    assert nb.qkv_attn_fused_plan(quant, n, H, KVH, hd, range_hint=rh, nsplit=nsplit)["takes"] == 0
    rng = np.random.default_rng(n)
    P = projection(oracle, quant, n, (H * hd, KVH * hd, KVH * hd), rng)
    S = rh + 5
    cos, sin = rope_tables(S, hd, 1e4)
    kc = np.zeros((LAYERS, S, KVH * hd), np.float32)
    one = np.ones(hd, np.float32)
    with pytest.raises(nb.NanoHipError, match="nano_hip error -1: the fused q.k.v . attention launch does not take this shape"):
        nb.op_qkv_attn_fused(quant, n, P["W"], P["x"], P["nw"], 3, kc, kc, gs=P["gs"], n_head=H, n_kv_head=KVH, hd=hd, S=S, range_hint=rh, rope_cos=cos,
                             rope_sin=sin, rope_qwen3=qwen3, q_norm=one if qwen3 else None, k_norm=one if qwen3 else None, nsplit=nsplit, n_layer=LAYERS, layer=LAYER)


@gpu
@pytest.mark.parametrize("quant,shape,nsplit,rh", [
    (Q80, (1792, 2, 1, 128), 1, 64),            # n = 1792: five waves
    (F32, (272, 4, 4, 68), 1, 64),              # head_dim 68
    # n_head * nsplit = 264 = 8 x 33: no power-of-two head counts give it, so this shape (66 heads on 2: a ratio of 33) is refused by the
    # head ratio as well -- the two 320s below, with every other predicate met, are the ones that meet n_head * nsplit <= 256 alone
    (F32, (264, 66, 2, 4), 4, 256),
    (F32, (256, 64, 64, 4), 5, 320),
    (Q80, (256, 64, 32, 128), 5, 320),
    (Q80, (256, 8, 4, 128), 2, 2 * 64 + 1),     # range_hint = nsplit * 64 + 1
    (F32, (64, 8, 4, 32), 3, 3 * 64 + 1),
], ids=["q80-n1792", "f32-hd68", "heads-x-splits-264-ratio-33", "f32-heads-x-splits-320", "q80-heads-x-splits-320", "q80-range-129", "f32-range-193"])
def test_qkv_attn_refusals(oracle, quant, shape, nsplit, rh):
    refused_qkv(oracle, quant, shape, nsplit, rh)


@gpu
def test_wo_w13_refusal(oracle):
    """Wo n = 2304: three float4 items per thread on 256 threads -- neither signature"""
    n_wo, E, hidden = 2304, 1024, 3072
    assert nb.wo_w13_fused_plan(n_wo, E, hidden)["takes"] == 0
    rng = np.random.default_rng(2304)
    wo, w1, w3 = (*q80_weights(rng, E, n_wo, 64), E), (*q80_weights(rng, hidden, E, 64), hidden), (*q80_weights(rng, hidden, E, 64), hidden)
    with pytest.raises(nb.NanoHipError, match="nano_hip error -1: the fused Wo . W1.W3 launch does not take this shape"):
        nb.op_wo_w13_fused(n_wo, wo, w1, w3, np.zeros(E, np.float32), np.ones(E, np.float32), x=order_free(rng, n_wo))
    with pytest.raises(nb.NanoHipError, match="layer1 outside"):
        nb.op_wo_w13_fused(2048, (*q80_weights(rng, E, 2048, 64), E), w1, w3, np.zeros(E, np.float32), np.ones(E, np.float32), x=order_free(rng, 2048), layer1=127 + 1)
