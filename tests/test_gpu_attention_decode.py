"""Every decode-attention launch plan against a float64 restatement of the reference's attention (infer/infer.c:810-879).

nano_hip_op_attention_decode runs one attention launch exactly as a decode step issues it (or a prefill chunk's two passes) and
reports the plan that ran: attention_kernel<LPR, QV, KVM, MODE, KVH, PG, NPT, W16> and the split count.  Each case below names the
plan it is meant to reach; the closing coverage test checks that the cases reach every plan axis the launcher can pick.

What a case checks, values first (a plan mismatch must not hide a wrong result):
  * the fresh k row at pos: FP32 within 2e-6 * max|k| of the float64 rmsnorm + RoPE; FP16 within one FP16 ulp (plus that FP32 bar,
    which matters only near the subnormals); the fresh FP16 v row bit-equal to float16(vraw);
  * the head outputs: max|d| / max|ref| <= 1e-5 per sequence (DESIGN.md's bar for tree-reduced float attention), the reference
    computed from the cache the kernel reads -- the half values of an FP16 cache, and at pos the rows the kernel wrote;
  * nothing else written: every other element of both caches (other slots, the other layer, unmapped pool rows) bit-identical;
  * the fragment-order Q80 output, where asked for: bit-equal to the oracle's quantization (group size 64) of the kernel's own output.
Rows in (pos, range_hint) hold stale values of +-1e4 that must not move the result.  They are finite on purpose: a masked row enters the
weighted V sum as an FMA with weight 0, and the engine zeroes the cache at load, so non-finite stale rows are outside the contract.
"""
import math

import numpy as np
import pytest

from nano_amd import binding as nb

EPS = 1e-5              # rmsnorm epsilon (infer.c:608)
ATTN_TOL = 1e-5         # tree-reduced float attention
K_TOL = 2e-6            # the finished FP32 k row
STALE = 1e4
NP = 2                  # timestep blocks a workgroup keeps in flight (attn_impl.h NP)
LAYERS, LAYER = 2, 1    # the cases write layer 1 of a two-layer cache


def plan(mode, lpr, qv, kvm, nsplit, npt=2, w16=0, paged=0, kv_half=0, xcd=1):
    return dict(mode=mode, lpr=lpr, qv=qv, kvm=kvm, npt=npt, w16=w16, paged=paged, kv_half=kv_half, nsplit=nsplit, xcd=xcd)


def case(cid, heads, kv, hd, style, nb_, rh, target, nsplit=0, kv_half=False, paged=False, chunk=None, frag=False, peak=False):
    """style: "qwen3" (q / k rmsnorm, half-split RoPE) or "nano" (adjacent-pair RoPE, no norm).  chunk: first position of a prefill
    chunk of nb_ tokens (target: the plans of pass 1 and pass 2)."""
    return pytest.param(dict(heads=heads, kv=kv, hd=hd, style=style, nb=nb_, rh=rh, nsplit=nsplit, kv_half=kv_half, paged=paged,
                             chunk=chunk, frag=frag, peak=peak, target=target), id=cid)


CASES = [
    # LPR 8, QV 1 (head_dim <= 32)
    case("q1-nano-kvm1", 8, 4, 32, "nano", 3, 64, plan(2, 8, 1, 1, 1)),
    case("q1-nano-kvm2", 8, 4, 32, "nano", 20, 192, plan(2, 8, 1, 2, 3)),
    case("q1-generic-xcd", 16, 8, 32, "qwen3", 2, 128, plan(0, 8, 1, 1, 2)),
    # LPR 8, QV 2 (head_dim <= 64)
    case("q2-qwen3-kvm1-frag", 16, 8, 64, "qwen3", 2, 64, plan(1, 8, 2, 1, 1), frag=True),
    case("q2-qwen3-kvm2-npt4-frag", 16, 8, 64, "qwen3", 20, 128, plan(1, 8, 2, 2, 1, npt=4), nsplit=1, frag=True),
    case("q2-nano-kvm4", 16, 4, 64, "nano", 40, 128, plan(2, 8, 2, 4, 2), nsplit=2),
    case("q2-generic-12of4", 12, 4, 48, "nano", 5, 200, plan(0, 8, 2, 1, 4, xcd=0)),
    # LPR 8, QV 4 (head_dim <= 128)
    case("q4-qwen3-kvm1-npt4", 16, 8, 128, "qwen3", 8, 256, plan(1, 8, 4, 1, 2, npt=4), nsplit=2),
    case("q4-qwen3-kvm2", 16, 8, 128, "qwen3", 16, 128, plan(1, 8, 4, 2, 2)),
    case("q4-qwen3-kvm4", 32, 8, 128, "qwen3", 24, 192, plan(1, 8, 4, 4, 3)),
    case("q4-nano-kvm1-frag", 8, 8, 128, "nano", 4, 64, plan(2, 8, 4, 1, 1), frag=True),
    case("q4-nano-kvm2", 16, 4, 128, "nano", 8, 320, plan(2, 8, 4, 2, 5)),
    case("q4-nano-kvm4", 16, 4, 128, "nano", 33, 128, plan(2, 8, 4, 4, 2)),
    case("q4-generic-24of6", 24, 6, 96, "qwen3", 3, 100, plan(0, 8, 4, 1, 2, xcd=0)),
    case("q4-generic-24of6-kvm2-npt4", 24, 6, 96, "qwen3", 16, 128, plan(0, 8, 4, 2, 1, npt=4, xcd=0), nsplit=1),
    # LPR 16 (head_dim 132 .. 256); KVM 4 is capped at 2 there (the SHARE path has 4 vectors per wave: KVM q heads + the k row)
    case("l16-qwen3-kvm1", 16, 4, 256, "qwen3", 2, 64, plan(1, 16, 4, 1, 2)),
    case("l16-qwen3-kvm2", 16, 4, 256, "qwen3", 12, 64, plan(1, 16, 4, 2, 2)),
    case("l16-qwen3-kvm4-capped", 16, 4, 256, "qwen3", 64, 128, plan(1, 16, 4, 2, 4)),
    case("l16-qwen3-kvm2-npt4-frag", 16, 8, 256, "qwen3", 20, 64, plan(1, 16, 4, 2, 1, npt=4), nsplit=1, frag=True),
    case("l16-nano-kvm1", 8, 8, 256, "nano", 3, 96, plan(2, 16, 4, 1, 3)),
    case("l16-nano-kvm2", 16, 4, 256, "nano", 16, 64, plan(2, 16, 4, 2, 2)),
    case("l16-nano-kvm4-capped", 16, 4, 256, "nano", 48, 160, plan(2, 16, 4, 2, 5)),
    case("l16-generic-hd192-xcd", 16, 8, 192, "qwen3", 2, 64, plan(0, 16, 4, 1, 2)),
    case("l16-generic-hd192-kvm2", 16, 8, 192, "qwen3", 12, 64, plan(0, 16, 4, 2, 2)),
    case("l16-generic-12of4", 12, 4, 160, "nano", 3, 64, plan(0, 16, 4, 1, 2, xcd=0)),
    # FP16 cache: 16-byte loads (W16) and 8-byte loads, with several heads per workgroup (the SHARE path's fresh v store)
    case("f16-w16-kvm2", 16, 8, 128, "qwen3", 16, 128, plan(1, 8, 4, 2, 2, w16=1, kv_half=1), kv_half=True),
    case("f16-hd36-kvm2", 8, 4, 36, "nano", 40, 64, plan(2, 8, 2, 2, 1, kv_half=1), kv_half=True),
    case("f16-hd132-kvm2", 16, 8, 132, "nano", 12, 64, plan(2, 16, 4, 2, 2, kv_half=1), kv_half=True),
    case("f16-w16-l16-kvm1", 16, 4, 256, "qwen3", 2, 64, plan(1, 16, 4, 1, 2, w16=1, kv_half=1), kv_half=True),
    case("f16-generic-24of6", 24, 6, 96, "qwen3", 2, 64, plan(0, 8, 4, 1, 1, w16=1, kv_half=1, xcd=0), kv_half=True),
    # paged cache, pages out of order, spare pool pages unmapped
    case("paged-kvm1", 16, 8, 128, "qwen3", 3, 192, plan(1, 8, 4, 1, 3, paged=1), paged=True),
    case("paged-f16-kvm2", 16, 4, 64, "nano", 12, 128, plan(2, 8, 2, 2, 2, paged=1, kv_half=1), kv_half=True, paged=True),
    case("paged-kvm4", 16, 4, 128, "nano", 40, 128, plan(2, 8, 4, 4, 2, paged=1), paged=True),
    case("paged-f16-l16-kvm2", 16, 4, 256, "qwen3", 12, 64, plan(1, 16, 4, 2, 2, w16=1, paged=1, kv_half=1), kv_half=True, paged=True),
    # more than 8 splits (ranges beyond 2048 positions; combined by the batched / prefill combine)
    case("wide-32-splits", 8, 4, 64, "nano", 2, 2112, plan(2, 8, 2, 2, 32)),
    case("wide-l16-12-splits", 16, 4, 256, "qwen3", 1, 2100, plan(1, 16, 4, 1, 12), nsplit=12),
    # batched prefill chunks: pass 1 (prep_only) stores every token's k row, pass 2 attends
    case("chunk1", 16, 8, 128, "qwen3", 1, 64, [plan(1, 8, 4, 1, 1)] * 2, chunk=40),
    case("chunk17-kvm2", 16, 8, 128, "qwen3", 17, 128, [plan(1, 8, 4, 2, 2)] * 2, chunk=64),
    case("chunk64-kvm4", 16, 4, 128, "nano", 64, 128, [plan(2, 8, 4, 4, 2)] * 2, chunk=64),
    case("chunk1-l16", 8, 8, 256, "nano", 1, 64, [plan(2, 16, 4, 1, 2)] * 2, chunk=40),
    case("chunk17-l16-kvm2", 16, 4, 256, "qwen3", 17, 64, [plan(1, 16, 4, 2, 2)] * 2, chunk=30),
    case("chunk64-l16-kvm4-capped", 16, 4, 256, "qwen3", 64, 64, [plan(1, 16, 4, 2, 2)] * 2, chunk=0),
    case("chunk17-paged-f16", 16, 8, 64, "qwen3", 17, 128, [plan(1, 8, 2, 2, 2, paged=1, kv_half=1)] * 2, kv_half=True, paged=True, chunk=50),
    # one dominant row per sequence: at pos (the fresh row), at row 0, at the last row of a round, in the second round
    case("peak-l8", 16, 8, 128, "nano", 4, 320, plan(2, 8, 4, 1, 2), nsplit=2, peak=True),
    case("peak-l16", 8, 4, 256, "nano", 4, 200, plan(2, 16, 4, 1, 2), nsplit=2, peak=True),
]


# ---- float64 reference (infer.c:601-614 rmsnorm, 681-706 RoPE, 842-879 attention) -------------------------------------------------
def rmsnorm64(x, w):
    x = np.asarray(x, np.float64)
    return np.asarray(w, np.float64) * (x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + EPS))


def rope64(x, c, s, qwen3):
    """x [..., hd] float64; c / s the float32 table row of the position."""
    x = np.array(x, np.float64); c = np.asarray(c, np.float64); s = np.asarray(s, np.float64)
    half = x.shape[-1] // 2
    if qwen3:
        v0, v1 = x[..., :half].copy(), x[..., half:].copy()
        x[..., :half] = v0 * c - v1 * s; x[..., half:] = v1 * c + v0 * s
    else:
        v0, v1 = x[..., 0::2].copy(), x[..., 1::2].copy()
        x[..., 0::2] = v0 * c - v1 * s; x[..., 1::2] = v0 * s + v1 * c
    return x


def finish64(raw, w, c, s, qwen3):
    """rmsnorm (Qwen3) + RoPE of raw head vectors [..., hd]"""
    return rope64(rmsnorm64(raw, w) if qwen3 else np.asarray(raw, np.float64), c, s, qwen3)


def rope_tables(S, hd, theta):
    half = hd // 2
    freq = 1.0 / theta ** (np.arange(half, dtype=np.float64) * 2 / hd)
    ang = np.arange(S, dtype=np.float64)[:, None] * freq[None, :]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def attend64(qf, K, V, kv_mul):
    """qf [n_head, hd] finished q; K / V [range, n_kv, hd] -> [n_head * hd]"""
    n_head, hd = qf.shape
    qg = qf.reshape(-1, kv_mul, hd)                                     # head h reads KV head h // kv_mul
    sc = np.einsum("gmd,tgd->gmt", qg, K) / math.sqrt(hd)
    sc -= sc.max(axis=-1, keepdims=True)
    p = np.exp(sc); p /= p.sum(axis=-1, keepdims=True)
    return np.einsum("gmt,tgd->gmd", p, V).reshape(n_head * hd)


def f16_ulp(x):
    return np.spacing(np.abs(x).astype(np.float16)).astype(np.float64)


def frag_expect(oracle, out, nb_, qd):
    """the Q80 groups of 64 of each row of out in fragment order: xf[tile][group][kq][token % 16][16], xsf[tile][group][token % 16]"""
    tiles, ng = (nb_ + 15) // 16, qd // 64
    xf = np.zeros((tiles, ng, 4, 16, 16), np.int8); xsf = np.zeros((tiles, ng, 16), np.float32)
    for b in range(nb_):
        q, s = oracle.quantize_q80(out[b], 64)
        xf[b // 16, :, :, b % 16, :] = q.reshape(ng, 4, 16)
        xsf[b // 16, :, b % 16] = s
    return xf.reshape(tiles, ng, 1024), xsf


def ragged_positions(rng, n, rh, R, nsplit):
    """n positions < rh: rh - 1 (the whole hinted range: every split and block in flight sees rows), 0 and block / round boundaries
    (multiples of R and of NP * R, the ends of the first round) first"""
    special = [rh - 1, 0, R, R - 1, NP * R, NP * R - 1, NP * nsplit * R - 1, NP * nsplit * R, 2 * R + 1]
    special = [p for p in dict.fromkeys(special) if 0 <= p < rh]
    pos = special[:n] + list(rng.integers(0, rh, max(0, n - len(special))))
    rng.shuffle(pos)
    return np.array(pos, np.uint32)


def build(c, seed):
    rng = np.random.default_rng(seed)
    H, KVH, hd, nb_, rh = c["heads"], c["kv"], c["hd"], c["nb"], c["rh"]
    qwen3 = c["style"] == "qwen3"
    QD, KD, half = H * hd, KVH * hd, hd // 2
    S = rh + 5                                                          # just above the range: small caches
    lpr = 16 if hd > 128 else 8
    R = 256 // lpr
    ns_for_pos = c["nsplit"] or max(1, min(8, -(-rh // (NP * R))))
    if c["chunk"] is not None:
        pos = np.arange(c["chunk"], c["chunk"] + nb_, dtype=np.uint32)
        assert pos[-1] < rh
    elif c["peak"]:
        pos = np.array([rh - 1 - b for b in range(nb_)], np.uint32)   # (late positions: every peak spot lies in the range)
    else:
        pos = ragged_positions(rng, nb_, rh, R, ns_for_pos)
    # (the case must exercise its plan: some sequence reaches the last block a workgroup keeps in flight in the first round, so every
    #  split and every in-flight block sees rows -- a lone sequence at pos 0 would reduce the check to "output = V[0]")
    t = c["target"][-1] if isinstance(c["target"], list) else c["target"]
    reach = (t["npt"] - 1) * t["nsplit"] * R
    assert int(pos.max()) >= reach, f"no sequence reaches row {reach}: some split / block in flight sees no row -- pick positions for this case"
    seqs = 1 if c["chunk"] is not None else nb_
    cdt = np.float16 if c["kv_half"] else np.float32
    inp = dict(q=rng.standard_normal((nb_, QD)).astype(np.float32), k=rng.standard_normal((nb_, KD)).astype(np.float32), pos=pos)
    if qwen3:
        inp["q_norm"] = rng.uniform(0.5, 1.5, hd).astype(np.float32); inp["k_norm"] = rng.uniform(0.5, 1.5, hd).astype(np.float32)
    inp["vraw"] = rng.standard_normal((nb_, KD)).astype(np.float32) if c["kv_half"] else None
    cos, sin = rope_tables(S, hd, 1e6 if qwen3 else 1e4)
    # cache rows of (sequence b, timestep t) in the flat row space of the cache arrays (layer LAYER)
    if c["paged"]:
        pages_per = -(-rh // 64)
        n_pages = seqs * pages_per + 3                                   # three spare pages stay unmapped
        perm = rng.permutation(n_pages)[:seqs * pages_per]               # pages out of order
        pt = np.full((seqs, pages_per + 1), 0xffffffff, np.uint32)      # (one entry past the range: no page)
        pt[:, :pages_per] = (perm.reshape(seqs, pages_per) * 64).astype(np.uint32)
        pool_rows = n_pages * 64
        shape = (LAYERS, pool_rows, KD)

        def row_of(b, t):
            return LAYER * pool_rows + int(pt[b if c["chunk"] is None else 0, t >> 6]) + (t & 63)
    else:
        pt, pool_rows = None, 0
        shape = (seqs, LAYERS, S, KD)

        def row_of(b, t):
            return ((b if c["chunk"] is None else 0) * LAYERS + LAYER) * S + t
    kc = rng.standard_normal(shape).astype(cdt); vc = rng.standard_normal(shape).astype(cdt)
    kf, vf = kc.reshape(-1, KD), vc.reshape(-1, KD)
    last = {}                                                           # sequence -> its last position (chunk: the slot's)
    for b in range(nb_):
        s_ = b if c["chunk"] is None else 0
        last[s_] = max(last.get(s_, 0), int(pos[b]))
    for s_, p in last.items():                                          # stale rows inside the hinted range, beyond pos
        for t in range(p + 1, rh):
            sign = np.where(rng.random(KD) < 0.5, -1.0, 1.0)
            kf[row_of(s_, t)] = (STALE * sign).astype(cdt); vf[row_of(s_, t)] = (-STALE * sign).astype(cdt)
    peaks = {}
    if c["peak"]:                                                       # one dominant row per sequence
        per_round = NP * c["nsplit"] * R
        spots = ["pos", 0, per_round - 1, per_round + R + 3]
        for b in range(nb_):
            spot = spots[b % len(spots)]
            t = int(pos[b]) if spot == "pos" else spot
            assert t <= pos[b]
            qf = finish64(inp["q"][b].reshape(H, hd), inp.get("q_norm", 1.0), cos[pos[b]], sin[pos[b]], qwen3).reshape(KVH, H // KVH, hd)
            u = qf.sum(axis=1); u /= np.linalg.norm(u, axis=-1, keepdims=True)
            kappa = 7.0 * math.sqrt(hd) / np.einsum("gmd,gd->gm", qf, u).min(axis=1)        # every head's score >= 7
            target = kappa[:, None] * u                                  # the finished k row of the peak, per KV head
            if spot == "pos":                                            # the fresh row: raw k whose RoPE is the target (no norm: nano)
                assert not qwen3
                inp["k"][b] = rope64(target, cos[pos[b]], -sin[pos[b]], False).reshape(KD).astype(np.float32)
            else:
                kf[row_of(b, t)] = target.reshape(KD).astype(cdt)
            peaks[b] = t
    return dict(inp=inp, kc=kc, vc=vc, row_of=row_of, pt=pt, pool_rows=pool_rows, S=S, cos=cos, sin=sin, qwen3=qwen3, peaks=peaks, QD=QD, KD=KD)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES)
def test_decode_attention_plan(oracle, c):
    seed = sum(ord(ch) for ch in str(sorted(c.items())))
    B = build(c, seed)
    inp, H, KVH, hd, nb_ = B["inp"], c["heads"], c["kv"], c["hd"], c["nb"]
    qwen3, QD, KD = B["qwen3"], B["QD"], B["KD"]
    chunk = c["chunk"] is not None
    res = nb.op_attention_decode(inp["q"], inp["k"], inp["pos"], B["kc"], B["vc"], n_head=H, n_kv_head=KVH, hd=hd, n_layer=LAYERS,
                                 layer=LAYER, S=B["S"], range_hint=c["rh"], rope_cos=B["cos"], rope_sin=B["sin"], rope_qwen3=qwen3,
                                 q_norm=inp.get("q_norm"), k_norm=inp.get("k_norm"), vraw=inp["vraw"], kv_half=c["kv_half"],
                                 chunk=chunk, nsplit=c["nsplit"], want_frag=c["frag"], pt_rows=B["pt"], pool_rows=B["pool_rows"])
    kc, vc = res["k_cache"].reshape(-1, KD), res["v_cache"].reshape(-1, KD)
    kin, vin = B["kc"].reshape(-1, KD).copy(), B["vc"].reshape(-1, KD).copy()
    pos, row_of = inp["pos"], B["row_of"]
    errors = []                                                         # (the rows and the outputs are both reported before failing)
    # 1. the fresh rows the launch stored
    for b in range(nb_):
        p, r = int(pos[b]), row_of(b, int(pos[b]))
        kref = finish64(inp["k"][b].reshape(KVH, hd), inp.get("k_norm", 1.0), B["cos"][p], B["sin"][p], qwen3).reshape(KD)
        got = kc[r].astype(np.float64)
        bar = K_TOL * np.abs(kref).max() + (f16_ulp(kref) if c["kv_half"] else 0.0)
        bad = np.abs(got - kref) > bar
        if bad.any():
            errors.append(f"sequence {b} (pos {p}): k row wrong at {np.flatnonzero(bad)[:8]} (worst |d| {np.abs(got - kref).max():.3e})")
        kin[r] = kc[r]
        if c["kv_half"]:
            if not np.array_equal(vc[r].view(np.uint16), inp["vraw"][b].astype(np.float16).view(np.uint16)):
                errors.append(f"sequence {b} (pos {p}): FP16 v row is not float16(vraw)")
            vin[r] = vc[r]
    # 2. the head outputs, from the cache the kernel read
    out = res["out"]
    for b in range(nb_):
        p = int(pos[b])
        rows = [row_of(b, t) for t in range(p + 1)]
        K = kc[rows].astype(np.float64).reshape(p + 1, KVH, hd); V = vc[rows].astype(np.float64).reshape(p + 1, KVH, hd)
        qf = finish64(inp["q"][b].reshape(H, hd), inp.get("q_norm", 1.0), B["cos"][p], B["sin"][p], qwen3)
        ref = attend64(qf, K, V, H // KVH)
        err = np.abs(out[b] - ref).max() / np.abs(ref).max()
        if not err <= ATTN_TOL:
            errors.append(f"sequence {b} (pos {p}, range_hint {c['rh']}): output max|d|/max|ref| = {err:.3e}")
        if b in B["peaks"]:                                              # the peak must matter: without it the output moves by far more
            keep = [i for i in range(p + 1) if i != B["peaks"][b]]
            alt = attend64(qf, K[keep], V[keep], H // KVH)
            assert np.abs(alt - ref).max() / np.abs(ref).max() > 1e-2, f"sequence {b}: the peak row does not dominate"
    assert not errors, f"{len(errors)} wrong rows / outputs, first: " + "; ".join(errors[:2] + [e for e in errors if "output" in e][:2])
    # 3. nothing else written
    assert np.array_equal(kc.view(np.uint8), kin.view(np.uint8)), "the k cache changed outside the fresh rows"
    assert np.array_equal(vc.view(np.uint8), vin.view(np.uint8)), "the v cache changed outside the fresh rows"
    # 4. fragment-order Q80 output of the kernel's own result
    if c["frag"]:
        xf, xsf = frag_expect(oracle, out, nb_, QD)
        assert np.array_equal(res["xsf"].view(np.uint32), xsf.view(np.uint32)), "xsf is not the Q80 scales of the output"
        assert np.array_equal(res["xf"], xf), "xf is not the Q80 quantization of the output in fragment order"
    # 5. the plan, last
    want = c["target"]
    assert res["plan"] == want, f"{c}: ran plan {res['plan']}, meant {want}: a retune moved this case -- pick a new shape for this target"


def _targets():
    out = []
    for p in CASES:
        c = p.values[0]
        t = c["target"]
        for i, x in enumerate(t if isinstance(t, list) else [t]):
            out.append(dict(x, hd=c["hd"], heads=c["heads"], kv=c["kv"], style=c["style"], prep=(c["chunk"] is not None and i == 0),
                            chunk=c["nb"] if c["chunk"] is not None else None, frag=c["frag"], peak=c["peak"]))
    return out


def test_cases_cover_every_plan_axis():
    """The targeted plans reach every choice launch_attention() can make (CPU-only: it reads the case table)."""
    T = _targets()

    def has(**kw):
        return any(all(t[k] == v for k, v in kw.items()) for t in T)

    for lq in [(8, 1), (8, 2), (8, 4), (16, 4)]:
        for mode in (2, 0):
            assert has(lpr=lq[0], qv=lq[1], mode=mode), (lq, mode)
    for hd in (64, 128, 256):
        assert has(mode=1, hd=hd), hd
    assert has(mode=0, hd=192, style="qwen3")
    assert any(t["mode"] == 0 and (t["kv"] & (t["kv"] - 1) or (t["heads"] // t["kv"]) & (t["heads"] // t["kv"] - 1)) for t in T)
    assert has(mode=0, xcd=1) and has(mode=0, xcd=0)
    for mode in (1, 2):
        for kvm in (1, 2, 4):
            assert has(lpr=8, mode=mode, kvm=kvm), (mode, kvm)
    for mode in (0, 1, 2):
        for kvm in (1, 2):
            assert has(lpr=16, mode=mode, kvm=kvm), (mode, kvm)
    assert not has(lpr=16, kvm=4)
    assert has(npt=4, kvm=1) and has(npt=4, kvm=2)
    assert any(t["kv_half"] and t["w16"] and t["kvm"] > 1 for t in T)
    assert any(t["kv_half"] and not t["w16"] and t["kvm"] > 1 and t["hd"] % 8 for t in T)
    assert has(paged=1, kvm=1) and any(t["paged"] and t["kvm"] > 1 for t in T) and has(paged=1, kv_half=1)
    assert has(nsplit=1) and any(2 <= t["nsplit"] <= 8 for t in T) and any(9 <= t["nsplit"] <= 32 for t in T)
    for n in (1, 17, 64):
        assert has(prep=True, chunk=n), n
    for kvm in (1, 2, 4):
        assert has(prep=True, lpr=8, kvm=kvm), kvm
    assert has(prep=True, lpr=16, kvm=2) and has(prep=True, lpr=16, kvm=1)
    assert has(frag=True, lpr=8) and has(frag=True, lpr=16)
    assert has(peak=True, lpr=8) and has(peak=True, lpr=16)
