"""The decode-attention launch on an FP8 (OCP e4m3fn, scale 1) KV cache, kv_half = 2, against the float64 reference of
tests/test_gpu_attention_decode.py -- that file's checks with a cache builder of its own.

Cache content: K and V are e4m3_encode (tests/kv8_ref.py) of standard-normal rows; a few V rows inside the attended range hold all 254
finite codes; stale rows beyond pos hold +-448 (0x7E / 0xFE), finite like that file's +-1e4.
What a case checks, values before plan:
  * the fresh v row is byte for byte e4m3_encode(vraw); the first sequences' vraw is the tie and saturation list of tests/test_kv8_ref.py
    (every midpoint between neighbouring values and one float32 step either side, +-0, +-448, +-464, +-1e4, 2^-10 and its neighbours),
    cut into rows of kv_dim: as many sequences as the 1024 values need (q1-nano and narrow-32-splits have 384 and 512 v elements and hold
    a random subset of that size);
  * the fresh k row is within one e4m3 step (of the float64 rmsnorm + RoPE, clamped to +-448) plus that file's K_TOL bar; in the case
    marked `sat` the raw k of the sequence at position 0 is scaled by 2000, and every finished element beyond +-448 must read back as
    0x7E / 0xFE (position 0: its softmax has one row, so the huge scores decide nothing);
  * no byte anywhere in either cache is a NaN code (0x7F / 0xFF);
  * the head outputs: max|d| / max|ref| <= 1e-5 (ATTN_TOL) -- the arithmetic is the FP32 kernel's, the reference is computed from the
    DECODED bytes the kernel read and wrote;
  * nothing else in either cache changed, byte for byte;
  * the plan that ran has kv_half = 2 and w16 = 0: FP8 rows have the narrow load form only (one 4-byte load per float4 slot), also at
    the head sizes where FP16 rows take their wide form.
nb and range_hint are those of the FP16 cases mirrored, so that every split and in-flight block sees rows."""
import math

import numpy as np
import pytest

import kv8_ref
import test_gpu_attention_decode as base
from nano_amd import binding as nb
from test_gpu_attention_decode import ATTN_TOL, K_TOL, LAYER, LAYERS, NP, attend64, finish64, plan, ragged_positions, rope64, rope_tables

FP8 = 2


def case(cid, heads, kv, hd, style, nb_, rh, target, nsplit=0, paged=False, chunk=None, peak=False, sat=False):
    return pytest.param(dict(heads=heads, kv=kv, hd=hd, style=style, nb=nb_, rh=rh, nsplit=nsplit, paged=paged, chunk=chunk, peak=peak,
                             sat=sat, target=target), id=cid)


CASES = [
    # QV 4, head_dim % 8 == 0 (where FP16 rows load wide): LPR 8 and LPR 16
    case("hd128-l8-kvm2", 16, 8, 128, "qwen3", 16, 128, plan(1, 8, 4, 2, 2, kv_half=FP8)),
    case("hd256-l16-kvm1", 16, 4, 256, "qwen3", 2, 64, plan(1, 16, 4, 1, 2, kv_half=FP8)),
    # head_dim % 8 == 4
    case("narrow-hd36-kvm2-sat", 8, 4, 36, "nano", 40, 64, plan(2, 8, 2, 2, 1, kv_half=FP8), sat=True),
    case("narrow-hd132-l16-kvm2", 16, 8, 132, "nano", 12, 64, plan(2, 16, 4, 2, 2, kv_half=FP8)),
    case("generic-24of6", 24, 6, 96, "qwen3", 2, 64, plan(0, 8, 4, 1, 1, kv_half=FP8, xcd=0)),
    case("q1-nano", 8, 4, 32, "nano", 3, 64, plan(2, 8, 1, 1, 1, kv_half=FP8)),
    # paged cache
    case("paged-q2-kvm2", 16, 4, 64, "nano", 12, 128, plan(2, 8, 2, 2, 2, paged=1, kv_half=FP8), paged=True),
    case("paged-hd256-l16-kvm2", 16, 4, 256, "qwen3", 12, 64, plan(1, 16, 4, 2, 2, paged=1, kv_half=FP8), paged=True),
    # a prefill chunk on the paged cache: pass 1 (prep_only) stores every token's k and v row, pass 2 attends
    case("chunk17-paged", 16, 8, 64, "qwen3", 17, 128, [plan(1, 8, 2, 2, 2, paged=1, kv_half=FP8)] * 2, paged=True, chunk=50),
    # more than 8 splits
    case("narrow-32-splits", 8, 4, 64, "nano", 2, 2112, plan(2, 8, 2, 2, 32, kv_half=FP8)),
    # one dominant row per sequence
    case("peak-l8", 16, 8, 128, "nano", 4, 320, plan(2, 8, 4, 1, 2, kv_half=FP8), nsplit=2, peak=True),
]


def e4m3_step(x):
    """the spacing of e4m3 values around x (float64): 2^-9 below 2^-6, else 2^(floor(log2 |x|) - 3)"""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -6)
    return 2.0 ** (np.floor(np.log2(a)) - 3)


def dec(codes):
    return kv8_ref.e4m3_decode(codes).astype(np.float64)


def build(c, seed):
    rng = np.random.default_rng(seed)
    H, KVH, hd, nb_, rh = c["heads"], c["kv"], c["hd"], c["nb"], c["rh"]
    qwen3 = c["style"] == "qwen3"
    QD, KD = H * hd, KVH * hd
    S = rh + 5
    R = 256 // (16 if hd > 128 else 8)
    ns_for_pos = c["nsplit"] or max(1, min(8, -(-rh // (NP * R))))
    if c["chunk"] is not None:
        pos = np.arange(c["chunk"], c["chunk"] + nb_, dtype=np.uint32)
    elif c["peak"]:
        pos = np.array([rh - 1 - b for b in range(nb_)], np.uint32)
    else:
        pos = ragged_positions(rng, nb_, rh, R, ns_for_pos)
    t = c["target"][-1] if isinstance(c["target"], list) else c["target"]
    reach = (t["npt"] - 1) * t["nsplit"] * R
    assert int(pos.max()) >= reach, f"no sequence reaches row {reach}: some split / block in flight sees no row"
    seqs = 1 if c["chunk"] is not None else nb_
    inp = dict(q=rng.standard_normal((nb_, QD)).astype(np.float32), k=rng.standard_normal((nb_, KD)).astype(np.float32), pos=pos)
    if qwen3:
        inp["q_norm"] = rng.uniform(0.5, 1.5, hd).astype(np.float32); inp["k_norm"] = rng.uniform(0.5, 1.5, hd).astype(np.float32)
    inp["vraw"] = rng.standard_normal((nb_, KD)).astype(np.float32)
    edges = rng.permutation(kv8_ref.edge_values())                  # every edge, over as many sequences' rows as it takes (fewer: a subset)
    n_edge = min(nb_, -(-len(edges) // KD))
    inp["vraw"][:n_edge] = np.resize(edges, n_edge * KD).reshape(n_edge, KD)
    sat_b = None
    if c["sat"]:
        assert not qwen3                                                # (no norm: the scale reaches the finished row)
        sat_b = int(np.flatnonzero(pos == 0)[0])
        inp["k"][sat_b] *= np.float32(2000.0)
    cos, sin = rope_tables(S, hd, 1e6 if qwen3 else 1e4)
    if c["paged"]:
        pages_per = -(-rh // 64)
        n_pages = seqs * pages_per + 3
        perm = rng.permutation(n_pages)[:seqs * pages_per]
        pt = np.full((seqs, pages_per + 1), 0xffffffff, np.uint32)
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
    kc = kv8_ref.e4m3_encode(rng.standard_normal(shape).astype(np.float32)); vc = kv8_ref.e4m3_encode(rng.standard_normal(shape).astype(np.float32))
    kf, vf = kc.reshape(-1, KD), vc.reshape(-1, KD)
    last = {}
    for b in range(nb_):
        s_ = b if c["chunk"] is None else 0
        last[s_] = max(last.get(s_, 0), int(pos[b]))
    for s_, p in last.items():                                          # stale rows inside the hinted range, beyond pos: +-448
        for t_ in range(p + 1, rh):
            neg = rng.random(KD) < 0.5
            kf[row_of(s_, t_)] = np.where(neg, 0xFE, 0x7E); vf[row_of(s_, t_)] = np.where(neg, 0x7E, 0xFE)
    # all 254 finite codes in V rows the longest sequence attends to (rows below its position: never the fresh row)
    s_long = max(last, key=last.get)
    n_code_rows = min(last[s_long], -(-254 // KD) + 1)
    assert n_code_rows * KD >= 254, "the attended range is too short to hold every code"
    codes = np.resize(rng.permutation(kv8_ref.finite_codes()), n_code_rows * KD).reshape(n_code_rows, KD)
    code_rows = [row_of(s_long, t_) for t_ in range(n_code_rows)]
    for i, r in enumerate(code_rows):
        vf[r] = codes[i]
    peaks = {}
    if c["peak"]:
        per_round = NP * c["nsplit"] * R
        spots = ["pos", 0, per_round - 1, per_round + R + 3]
        for b in range(nb_):
            spot = spots[b % len(spots)]
            t_ = int(pos[b]) if spot == "pos" else spot
            assert t_ <= pos[b]
            qf = finish64(inp["q"][b].reshape(H, hd), inp.get("q_norm", 1.0), cos[pos[b]], sin[pos[b]], qwen3).reshape(KVH, H // KVH, hd)
            u = qf.sum(axis=1); u /= np.linalg.norm(u, axis=-1, keepdims=True)
            kappa = 7.0 * math.sqrt(hd) / np.einsum("gmd,gd->gm", qf, u).min(axis=1)
            target = kappa[:, None] * u
            if spot == "pos":
                assert not qwen3
                inp["k"][b] = rope64(target, cos[pos[b]], -sin[pos[b]], False).reshape(KD).astype(np.float32)
            else:
                kf[row_of(b, t_)] = kv8_ref.e4m3_encode(target.reshape(KD).astype(np.float32))
            peaks[b] = t_
    return dict(inp=inp, kc=kc, vc=vc, row_of=row_of, pt=pt, pool_rows=pool_rows, S=S, cos=cos, sin=sin, qwen3=qwen3, peaks=peaks, QD=QD, KD=KD,
                sat_b=sat_b, code_rows=code_rows)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES)
def test_decode_attention_fp8(c):
    seed = sum(ord(ch) for ch in str(sorted(c.items())))
    B = build(c, seed)
    inp, H, KVH, hd, nb_ = B["inp"], c["heads"], c["kv"], c["hd"], c["nb"]
    qwen3, KD = B["qwen3"], B["KD"]
    chunk = c["chunk"] is not None
    res = nb.op_attention_decode(inp["q"], inp["k"], inp["pos"], B["kc"], B["vc"], n_head=H, n_kv_head=KVH, hd=hd, n_layer=LAYERS,
                                 layer=LAYER, S=B["S"], range_hint=c["rh"], rope_cos=B["cos"], rope_sin=B["sin"], rope_qwen3=qwen3,
                                 q_norm=inp.get("q_norm"), k_norm=inp.get("k_norm"), vraw=inp["vraw"], kv_half=FP8,
                                 chunk=chunk, nsplit=c["nsplit"], pt_rows=B["pt"], pool_rows=B["pool_rows"])
    assert res["k_cache"].dtype == np.uint8 and res["v_cache"].dtype == np.uint8
    kc, vc = res["k_cache"].reshape(-1, KD), res["v_cache"].reshape(-1, KD)
    kin, vin = B["kc"].reshape(-1, KD).copy(), B["vc"].reshape(-1, KD).copy()
    pos, row_of = inp["pos"], B["row_of"]
    errors = []
    # 1. the fresh rows the launch stored
    n_sat = 0
    for b in range(nb_):
        p, r = int(pos[b]), row_of(b, int(pos[b]))
        kref = finish64(inp["k"][b].reshape(KVH, hd), inp.get("k_norm", 1.0), B["cos"][p], B["sin"][p], qwen3).reshape(KD)
        kclamp = np.clip(kref, -448.0, 448.0)
        got = dec(kc[r])
        bar = K_TOL * np.abs(kref).max() + e4m3_step(kclamp)
        bad = ~(np.abs(got - kclamp) <= bar)
        if bad.any():
            errors.append(f"sequence {b} (pos {p}): k row wrong at {np.flatnonzero(bad)[:8]} (worst |d| {np.abs(got - kclamp).max():.3e})")
        over = np.abs(kref) > 448.0 * (1 + 1e-5)                        # (beyond the FP32 row's own error: certainly out of range)
        if over.any():
            n_sat += int(over.sum())
            if not np.array_equal(kc[r][over], np.where(kref[over] < 0, 0xFE, 0x7E)):
                errors.append(f"sequence {b} (pos {p}): k elements beyond +-448 did not saturate to 0x7E / 0xFE: {[hex(x) for x in kc[r][over][:8]]}")
        kin[r] = kc[r]
        want_v = kv8_ref.e4m3_encode(inp["vraw"][b])
        if not np.array_equal(vc[r], want_v):
            i = np.flatnonzero(vc[r] != want_v)
            errors.append(f"sequence {b} (pos {p}): v row is not e4m3_encode(vraw) at {len(i)} elements, first "
                          f"{[(float(inp['vraw'][b][j]), hex(vc[r][j]), hex(want_v[j])) for j in i[:6]]}")
        vin[r] = vc[r]
    if c["sat"]:
        assert n_sat >= KD // 4, "the saturation case saturates too few elements"
    for name, arr in (("k", kc), ("v", vc)):
        if np.isin(arr, kv8_ref.NAN_CODES).any():
            errors.append(f"the {name} cache holds a NaN code (0x7F / 0xFF)")
    # 2. the head outputs, from the decoded bytes the kernel read and wrote
    out = res["out"]
    for b in range(nb_):
        p = int(pos[b])
        rows = [row_of(b, t) for t in range(p + 1)]
        K = dec(kc[rows]).reshape(p + 1, KVH, hd); V = dec(vc[rows]).reshape(p + 1, KVH, hd)
        qf = finish64(inp["q"][b].reshape(H, hd), inp.get("q_norm", 1.0), B["cos"][p], B["sin"][p], qwen3)
        ref = attend64(qf, K, V, H // KVH)
        err = np.abs(out[b] - ref).max() / np.abs(ref).max()
        print(f"sequence {b} (pos {p}): output max|d|/max|ref| = {err:.3e}")
        if not err <= ATTN_TOL:
            errors.append(f"sequence {b} (pos {p}, range_hint {c['rh']}): output max|d|/max|ref| = {err:.3e}")
        if b in B["peaks"]:
            keep = [i for i in range(p + 1) if i != B["peaks"][b]]
            alt = attend64(qf, K[keep], V[keep], H // KVH)
            assert np.abs(alt - ref).max() / np.abs(ref).max() > 1e-2, f"sequence {b}: the peak row does not dominate"
    assert not errors, f"{len(errors)} wrong rows / outputs, first: " + "; ".join(errors[:3] + [e for e in errors if "output" in e][:2])
    # 3. nothing else written
    assert np.array_equal(kc, kin), "the k cache changed outside the fresh rows"
    assert np.array_equal(vc, vin), "the v cache changed outside the fresh rows"
    # 4. the plan, last
    assert res["plan"] == c["target"], f"{c}: ran plan {res['plan']}, meant {c['target']}"


def test_fp8_cases_reach_every_new_path():
    """LPR 8 and LPR 16, at head sizes with hd % 8 == 0 and hd % 8 == 4, QV 1 / 2 / 4, the paged cache, a prefill chunk (both passes) and
    more than 8 splits; every vraw but those of the two smallest cases holds the whole edge list (CPU-only: the case table)."""
    T = []
    for p in CASES:
        c = p.values[0]
        t = c["target"]
        for i, x in enumerate(t if isinstance(t, list) else [t]):
            T.append(dict(x, hd=c["hd"], prep=(c["chunk"] is not None and i == 0), chunk=c["chunk"] is not None, sat=c["sat"], peak=c["peak"]))

    def has(**kw):
        return any(all(t[k] == v for k, v in kw.items()) for t in T)

    assert all(t["kv_half"] == FP8 for t in T)
    assert all(t["w16"] == 0 for t in T)                               # attention_plan() never sets w16 for FP8 rows
    for lpr in (8, 16):
        assert any(t["lpr"] == lpr and t["qv"] == 4 and t["hd"] % 8 == 0 for t in T), lpr
    assert any(t["lpr"] == 16 and t["hd"] % 8 == 4 for t in T) and any(t["qv"] == 2 and t["hd"] % 8 == 4 for t in T)
    for p in CASES:
        c = p.values[0]
        assert c["nb"] * c["kv"] * c["hd"] >= len(kv8_ref.edge_values()) or p.id in ("q1-nano", "narrow-32-splits"), p.id
    assert has(qv=1) and has(mode=0) and has(mode=1) and has(mode=2)
    assert has(paged=1, qv=2) and has(paged=1, lpr=16)
    assert has(prep=True, paged=1) and has(chunk=True, prep=False)
    assert any(t["nsplit"] > 8 for t in T)
    assert has(sat=True, mode=2) and has(peak=True)
    assert any(t["kvm"] > 1 and t["hd"] % 8 == 0 for t in T) and any(t["kvm"] > 1 and t["hd"] % 8 for t in T)
    assert base.LAYERS == 2 and base.LAYER == 1
