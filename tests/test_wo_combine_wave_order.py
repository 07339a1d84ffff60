"""CPU restatement of the split-attention combine with in-wave weights (gemv_common.h cw_issue / cw_combine, gemv_q80_slab_body.inc SLAB_CW;
the kernel wo_w13_fused_cw_kernel) in numpy float32, lane by lane, against a restatement of the table form it replaces (combine_weights:
thread t makes the weight of head t >> 3, split t & 7 into an LDS table; then eight multiply-add rounds per item, whatever the split count).

The lane schedule restated: wave w of NW, item round j: the wave's 64 float4 items are the 256 values from (w + j NW) * 256, i.e. heads
(w + j NW) HPW .. + HPW - 1 with HPW = 256 / head_dim.  Lane l < 8 HPW loads the (max, sum) pair of head (w + j NW) HPW + (l >> 3), split
l & 7 (a head beyond the last: head 0's; a split >= nsplit or a lane >= 8 HPW: an out-of-range load, +0), runs the chain -- live = l > 0;
fmaxf with the DPP partners lane ^ 1 (quad_perm 0xB1), lane ^ 2 (0x4E), the mirrored lane of the 8-lane half-row (0x141); expf(m - M);
L = l e summed through the same three partners in the same order; e / L -- and every lane fetches weight s of its item's head from lane
8 (head within the wave) + s (ds_bpermute).  The live splits are added in ascending order, one multiply and one add each.

Checked for head_dim 32 / 64 / 128 / 256 and 1 .. 8 splits, on random partials with planted -0.0, denormals and one split whose partial
vector is all -0.0, statistics with a dominant split (the others' e underflows to 0) on every other head:
  * every item receives the weights of its own head;
  * every element carries the bits of the table form, whose dead tail (splits >= nsplit: partial +0, weight 0 / L) is run here in full;
  * items beyond the row's end stay finite (+0): a dead wave never takes the quantizer's slow path.
And the plan sweep's invariant: nano_hip_wo_w13_fused_plan names the form (cw = 1) exactly for launches behind split attention with
heads of 32 | 64 | 128 | 256 values that tile the row and 1 .. 8 splits, changes nothing else of the plan but the LDS bytes, reaches
the four built instantiations <WF, WFC> of {0, 1} x {0, 2}, and NANO_COMBINE_WAVE=0 refuses it.  nano_hip_q80_gemv_plan does the same for
the plain launch (gemv_q80_slab_cw_kernel<1, UPW, WFC>, one item per thread) in a 17th word behind takes: its first 16 words do
not move with the form.
The built kernels keep the code hygiene of tests/test_isa_hygiene.py (needs hipcc)."""
import os
import shutil
import sys

import numpy as np
import pytest

from nano_amd import binding as nb
from test_fused_launch_plan import SMALLEST, wo13_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)


def chain(m, l):
    """combine_weights' arithmetic on arrays [..., 8]: axis -1 is the 8-lane DPP half-row of one head"""
    lane = np.arange(8)
    p1, p2, p3 = lane ^ 1, lane ^ 2, 7 - lane
    live = l > 0
    with np.errstate(all="ignore"):
        M = np.where(live, m, f32(-np.inf)).astype(f32)
        for p in (p1, p2, p3):
            M = np.maximum(M, M[..., p])
        e = np.where(live, np.exp((m - M).astype(f32)).astype(f32), f32(0)).astype(f32)
        L = (l * e).astype(f32)
        for p in (p1, p2, p3):
            L = (L + L[..., p]).astype(f32)
        return (e / L).astype(f32)


def table_form(part, ml, n, hd, ns, items):
    """the table form: weights per (head, split slot 0 .. 7), then 8 rounds per item; items beyond n read +0 and head 0's weights"""
    nh = n // hd
    m = np.zeros((nh, 8), f32); l = np.zeros((nh, 8), f32)
    m[:, :ns] = ml[:, :, 0]; l[:, :ns] = ml[:, :, 1]
    wgt = chain(m, l)                                           # [nh][8]
    out = np.zeros((items, 4), f32)
    for it in range(items):
        i = it * 4
        head = (i if i < n else 0) // hd
        acc = np.zeros(4, f32)
        for s in range(8):
            pv = part[s, i:i + 4] if (s < ns and i < n) else np.zeros(4, f32)
            with np.errstate(all="ignore"):
                acc = (acc + (pv * wgt[head, s]).astype(f32)).astype(f32)
        out[it] = acc
    return out, wgt


def wave_form(part, ml, n, hd, ns, nthr):
    """the in-wave form on nthr threads: -> (values [items][4], the weights every item fetched [items][8], heads they came from)"""
    nh, NW = n // hd, nthr // 64
    NV = (n // 4 + nthr - 1) // nthr
    lg = hd.bit_length() - 1
    hpw = 256 >> lg
    out = np.zeros((NV * nthr, 4), f32); got = np.zeros((NV * nthr, 8), f32)
    lane = np.arange(64)
    for j in range(NV):
        for w in range(NW):
            hl, sp = lane >> 3, lane & 7
            h = (w + j * NW) * hpw + hl
            ok = (hl < hpw) & (sp < ns)
            hc = np.where(h < nh, h, 0)
            m = np.where(ok, ml[hc, np.minimum(sp, ns - 1), 0], f32(0)).astype(f32)
            l = np.where(ok, ml[hc, np.minimum(sp, ns - 1), 1], f32(0)).astype(f32)
            wq = chain(m.reshape(8, 8), l.reshape(8, 8)).reshape(64)      # half-rows of 8 lanes
            src = ((lane * 4) >> lg) * 8
            for ln in range(64):
                it = ln + 64 * w + j * nthr
                i = it * 4
                wl = wq[src[ln]:src[ln] + 8]
                got[it] = wl
                acc = np.zeros(4, f32)
                for s in range(ns):                                       # the live splits only, ascending
                    pv = part[s, i:i + 4] if i < n else np.zeros(4, f32)
                    with np.errstate(all="ignore"):
                        acc = (acc + (pv * wl[s]).astype(f32)).astype(f32)
                out[it] = acc
    return out, got


def inputs(rng, n, hd, ns):
    nh = n // hd
    part = rng.standard_normal((ns, n)).astype(f32)
    flat = part.reshape(-1)
    idx = rng.permutation(flat.size)
    flat[idx[:48]] = f32(-0.0)
    flat[idx[48:96]] = (f32(1e-41) * rng.choice([-1.0, 1.0], 48)).astype(f32)
    part[ns // 2] = f32(-0.0)
    ml = np.empty((nh, ns, 2), f32)
    ml[..., 0] = rng.normal(0.0, 3.0, (nh, ns)); ml[..., 1] = rng.uniform(1.0, 64.0, (nh, ns))
    for h in range(0, nh, 2):
        ml[h, :, 0] = -150.0 - 120.0 * rng.permutation(ns)
        ml[h, rng.integers(ns), 0] = 30.0
    return part, ml


@pytest.mark.parametrize("hd", [32, 64, 128, 256])
@pytest.mark.parametrize("n,nthr", [(2048, 512), (1280, 512), (768, 256), (1280, 256)])
def test_lane_schedule_hands_out_own_heads_weights_and_the_table_forms_bits(hd, n, nthr):
    rng = np.random.default_rng(hd * 7 + n + nthr)
    for ns in range(1, 9):
        part, ml = inputs(rng, n, hd, ns)
        new, got = wave_form(part, ml, n, hd, ns, nthr)
        old, wgt = table_form(part, ml, n, hd, ns, new.shape[0])
        live = n // 4
        heads = (np.arange(live) * 4) // hd
        assert np.array_equal(bits(got[:live, :ns]), bits(wgt[heads, :ns])), (hd, n, ns, "an item fetched another head's weights")
        assert np.array_equal(bits(new[:live]), bits(old[:live])), (hd, n, ns, np.flatnonzero((bits(new[:live]) != bits(old[:live])).any(axis=1))[:6])
        assert np.isfinite(new).all() and not new[live:].any() and not np.signbit(new[live:]).any(), (hd, n, ns, "items beyond the row")
        assert np.isfinite(wgt[:, :ns]).all() and (wgt[0::2, :ns] == 0).sum() == (ns - 1) * len(wgt[0::2]), "a dominant split leaves the others weight 0"


def test_head_dim_128_row_has_the_splits_it_says():
    """the weights are a softmax over the splits' statistics: sum_s l_s w_s == 1 to rounding, per head"""
    rng = np.random.default_rng(5)
    part, ml = inputs(rng, 2048, 128, 5)
    _, got = wave_form(part, ml, 2048, 128, 5, 512)
    heads = (np.arange(512) * 4) // 128
    s = (got[:, :5].astype(np.float64) * ml[heads, :, 1]).sum(axis=1)
    assert np.abs(s - 1).max() < 1e-6


def expect_cw(n_wo, attn):
    if attn is None:
        return 0
    n_head, hd, ns = attn
    return int(hd in (32, 64, 128, 256) and n_head * hd == n_wo and 1 <= ns <= 8)


def test_plan_names_the_form_only_inside_its_conditions(monkeypatch):
    monkeypatch.delenv("NANO_COMBINE_WAVE", raising=False)
    seen = set()
    for n_wo, E, hidden in sorted({v[:3] for k, v in SMALLEST.items() if k[0] == "wo_w13"} | {(2048, 1024, 3072)}):
        for hd in (4, 16, 32, 48, 64, 96, 128, 256, 512):
            for n_head in sorted({max(n_wo // hd, 1), max(n_wo // hd - 1, 1), n_wo // hd + 1}):
                for ns in range(1, 10):
                    attn = (n_head, hd, ns)
                    monkeypatch.delenv("NANO_COMBINE_WAVE", raising=False)
                    p = nb.wo_w13_fused_plan(n_wo, E, hidden, attn=attn)
                    monkeypatch.setenv("NANO_COMBINE_WAVE", "0")
                    q = nb.wo_w13_fused_plan(n_wo, E, hidden, attn=attn)
                    # (the descriptor itself asks for 1 .. 8 splits and heads that tile the row: everything else is refused before any plan)
                    assert p["takes"] == q["takes"] == int(ns <= 8 and n_head * hd == n_wo), (n_wo, E, hidden, attn, p, q)
                    if not p["takes"]:
                        assert not any(p.values()) and not any(q.values())
                        continue
                    assert p["cw"] == expect_cw(n_wo, attn) and q["cw"] == 0, (n_wo, E, hidden, attn, p, q)
                    assert {k: v for k, v in p.items() if k not in ("cw", "lds_bytes")} == {k: v for k, v in q.items() if k not in ("cw", "lds_bytes")}
                    # the weight table [n_head][8] floats leaves Wo's carve-up (the launch asks for the larger of its two bodies' bytes)
                    assert q["lds_bytes"] - n_head * 32 * p["cw"] <= p["lds_bytes"] <= q["lds_bytes"], (p, q)
                    if p["cw"]:
                        assert p["role"] == nb.Q80_ROLES.index("resid_combine") and (p["threads"], p["nv_a"]) == (512, 1)
                        assert n_wo // 4 <= p["threads"] and 256 % hd == 0, "one float4 item per thread, whole heads per wave"
                        seen.add((p["wf"], p["wfc"]))
        monkeypatch.delenv("NANO_COMBINE_WAVE", raising=False)
        assert nb.wo_w13_fused_plan(n_wo, E, hidden)["cw"] == 0                 # no split attention in front: the residual role
    assert seen == {(0, 0), (0, 2), (1, 0), (1, 2)}, ("the built instantiations wo_w13_fused_cw_kernel<WF, WFC>", seen)
    # the forms of tests/test_fused_launch_plan.py do not move: cw is a word of its own
    for f, (n_wo, E, hidden, splits) in SMALLEST.items():
        if f[0] == "wo_w13":
            assert wo13_form(nb.wo_w13_fused_plan(n_wo, E, hidden, attn=(n_wo // 128, 128, splits) if splits > 1 else None)) == f


def test_plain_launch_plan_names_the_form_only_inside_its_conditions(monkeypatch):
    seen = set()
    for n, rows in ((256, 256), (512, 256), (768, 1024), (1024, 1024), (1280, 256), (2048, 1024), (3072, 1024), (4096, 2560), (9728, 2560), (320, 256)):
        for hd in (16, 32, 64, 128, 256, 512):
            if n % hd:
                continue
            for ns in range(1, 9):
                for nb_ in (1, 2):
                    for gs, ordered in ((64, False), (64, True), (128, False)):
                        if n % gs:
                            continue
                        kw = dict(gs=gs, attn=(n // hd, hd, ns), ordered=ordered)
                        monkeypatch.delenv("NANO_COMBINE_WAVE", raising=False)
                        p, cw = nb.q80_gemv_plan(1, n, [rows], nb_, **kw), nb.q80_gemv_plan_cw(1, n, [rows], nb_, **kw)
                        monkeypatch.setenv("NANO_COMBINE_WAVE", "0")
                        q, cq = nb.q80_gemv_plan(1, n, [rows], nb_, **kw), nb.q80_gemv_plan_cw(1, n, [rows], nb_, **kw)
                        assert p == q and cq == 0, (n, rows, kw, nb_, p, q, cq)            # the 16 words do not move with the form
                        want = int(bool(p["takes"]) and nb.Q80_KERNELS[p["kernel"]] == "slab" and nb.Q80_ROLES[p["role"]] == "resid_combine" and gs == 64
                                   and p["B"] == 1 and p["nv"] == 1 and nb.Q80_VARIANTS[p["variant"]] != "early" and hd in (32, 64, 128, 256))
                        assert cw == want, (n, rows, kw, nb_, p, cw)
                        if cw:
                            assert 256 % hd == 0 and p["nv"] * 256 * p["nw"] >= n
                            seen.add((p["nv"], p["upw"], nb.Q80_VARIANTS[p["variant"]]))
    monkeypatch.delenv("NANO_COMBINE_WAVE", raising=False)
    assert nb.q80_gemv_plan_cw(1, 2048, [1024], 1) == 0 and nb.q80_gemv_plan_cw(0, 1024, [2048, 1024, 1024], 1, norm=True) == 0
    assert (1, 1, "plain") in seen and all(nv == 1 for nv, _, _ in seen), seen
    print("plain-launch forms met:", sorted(seen))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None, reason="needs hipcc")
def test_built_instantiations_keep_the_hygiene():
    """no waterfall loop, no wait-for-everything inside the issue phase, no scratch, no spill; no barrier and no LDS table for the weights:
    two barriers fewer than the table form's kernel (combine_weights' two variants), eight ds_bpermute"""
    import re
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_scan
    asm = isa_scan.compile_to_asm(os.path.join(ROOT, "nano_amd", "csrc", "gemv_q80_gs64.hip"))
    expected = ["wo_w13_fused_cw_kernelILi%dELi%dEE" % (wf, wfc) for wf in (0, 1) for wfc in (0, 2)]
    recs = isa_scan.scan(asm, "wo_w13_fused_cw_kernel")
    assert len(recs) == 4
    plain = isa_scan.scan(asm, "gemv_q80_slab_cw_kernel")
    assert len(plain) == 3 + 2 * 3                              # <1, UPW, 0> of UPW 1, 2, 4 and <1, UPW, WFC> of {1, 2} x {2, 3, 4}
    expected += [re.search(r"gemv_q80_slab_cw_kernelILi\d+ELi\d+ELi\d+EE", k["name"]).group(0) for k in plain]
    for k in recs + plain:
        assert k["waterfall_compares"] == 0, (k["name"], "waterfall loop")
        early = [w for w in k["full_waits_before_later_loads"] if w < k["first_barrier"]]
        assert not early, (k["name"], "s_waitcnt vmcnt(0) inside the issue phase at instruction", early)
        # no late kernel-argument fetch the table form's kernel of the same shape does not have
        m = re.search(r"wo_w13_fused_cw_kernelILi(\d+)ELi(\d+)EE", k["name"])
        if m:
            sib = isa_scan.scan(asm, "wo_w13_fused_kernelILi3ELi%sELi%sEE" % m.groups())
        else:
            nv, upw, wfc = re.search(r"gemv_q80_slab_cw_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", k["name"]).groups()
            sib = isa_scan.scan(asm, "gemv_q80_slab_kernelILi3ELi64ELi1ELi%sELi%sELi0ELi0ELi%sEE" % (nv, upw, wfc))
        assert len(sib) == 1, (k["name"], "the table form's kernel of the same shape")
        assert len(k["late_scalar_loads"]) <= len(sib[0]["late_scalar_loads"]), (k["name"], k["late_scalar_loads"], sib[0]["late_scalar_loads"])
    seen = set()
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size: *\d+", asm, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        hits = [e for e in expected if e in name]
        if hits:
            seen.update(hits)
            assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1)) == 0, (name, "scratch")
            assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1)) == 0, (name, "spills")
    assert seen == set(expected), sorted(set(expected) - seen)

    def body(sym):
        lines = asm.split("\n")
        start = next(i for i, ln in enumerate(lines) if ln.startswith("_Z") and sym in ln and ln.split(";")[0].rstrip().endswith(":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        return [ln.split(";")[0].strip() for ln in lines[start + 1:end]]
    for wf in (0, 1):
        for wfc in (0, 2):
            new, old = body("wo_w13_fused_cw_kernelILi%dELi%dEE" % (wf, wfc)), body("wo_w13_fused_kernelILi3ELi%dELi%dEE" % (wf, wfc))
            count = lambda b, s: sum(t.startswith(s) for t in b)
            assert count(new, "s_barrier") == count(old, "s_barrier") - 2 and count(new, "ds_bpermute_b32") == 8 and count(old, "ds_bpermute_b32") == 0
