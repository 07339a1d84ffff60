"""GPU tests of whole models with a LoRA table: several modules resident at once, a module (or none) bound to each KV slot, and one step
serving rows of different modules from one read of the base weights.  The oracle is the single-module path (nano_hip_lora_attach), itself
pinned to the compiled reference (test_gpu_lora_model.py, tests/golden/lora_*.npz): a table step has exactly the structure of a step
with an attached module, so

  * a row whose slot is bound to module i is BIT FOR BIT -- logits and the K / V rows the step wrote -- the row of a max_batch = 1 model
    with module i attached and the same feeding: four rows (bound A, none, B, A), ten rows (across the 9-row switch to the matrix-core
    GEMMs), a 70-token prefill (a 64-token chunk and a tail) into a bound slot, decode_greedy over 80 ids, a fork;
  * a row without a module is bit for bit a model that never had one at positions below 64; at positions >= 64 the table step attends in
    one split where the base model takes two, so there it is bit for bit the same row alone in a table model (batch invariance) and
    within test_gpu_e2e.TOL of the base model;
  * rebinding a slot is seen by the captured graphs when they replay; storing an entry of another rank drops them;
  * the gates refuse a table exactly as they refuse a module.

Modules A, B, C: (rank, alpha) = (5, 16), (8, 4), (1, 16); D (8, 16) overwrites C's entry in the rebinding case."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_e2e as e2e
from conftest import ROOT
from nano_amd import binding as nb
from nano_amd import modelfile as mf
from fused_ref import bits

pytestmark = pytest.mark.gpu

S = 256
CASES = [("tiny-nano", "f32", 0), ("tiny-nano", "q80", 32), ("tiny-nano", "q4k", 0), ("tiny-nano-odd", "q4k", 0)]
MODS = {"A": (5, 16, 13), "B": (8, 4, 14), "C": (1, 16, 15), "D": (8, 16, 16)}      # name: (rank, alpha, seed)
ENTRY = {"A": 0, "B": 1, "C": 2}
T = 70                                  # a 64-token chunk and a tail of 6

_files = {}


def files(model_dir, preset, quant, gs):
    """(model path, spec, {module name: path}): block_size 256, written once per session"""
    key = (preset, quant, gs)
    if key not in _files:
        spec = mf.preset(preset, quant, group_size=gs, block_size=S)
        path = os.path.join(model_dir, f"loratable-{preset}-{quant}-{gs}.bin")
        mf.write_model(path, spec, seed=39)
        lp = {}
        for name, (rank, alpha, seed) in MODS.items():
            lp[name] = os.path.join(model_dir, f"loratable-{preset}-{quant}-{gs}-{name}.lora")
            mf.write_lora(lp[name], spec, rank=rank, alpha=alpha, seed=seed)
        _files[key] = (path, spec, lp)
    return _files[key]


def table_model(path, lp, max_batch, **kw):
    m = nb.load_model_file(path, max_seq_len=S, max_batch=max_batch, **kw)
    for name, i in ENTRY.items():
        m.lora_table_set_file(i, lp[name])
    return m


def single(path, lp, name, **kw):
    """the oracle: max_batch = 1, module `name` attached (None: a model that never had a module)"""
    m = nb.load_model_file(path, max_seq_len=S, max_batch=1, **kw)
    if name:
        m.lora_attach_file(lp[name])
    return m


def bind(m, names):
    m.lora_bind(list(range(len(names))), [None if n is None else ENTRY[n] for n in names])
    assert [m.lora_binding(s) for s in range(len(names))] == [None if n is None else ENTRY[n] for n in names]


def kv_rows(m, spec, slot, positions):
    return np.stack([m.read_state(w, spec.kv_dim, slot=slot, layer=l, pos=p) for l in range(spec.n_layer) for p in positions for w in ("k", "v")])


def same_bits(a, b, what):
    bad = np.argwhere(bits(a) != bits(b))
    assert not bad.size, (what, "first differences at", bad[:6].tolist(), float(np.abs(np.asarray(a, np.float64) - b).max()))


def feed_rows(m, spec, prompts, pos):
    """every row's history by prefill into its slot, then ONE forward of all rows: (logits [nb][V], the K / V rows the step wrote, per row)"""
    for b, p in enumerate(pos):
        if p:
            m.prefill(prompts[b][:-1], 0, slot=b)
    lg = m.forward([int(p[-1]) for p in prompts], pos)[0].copy()
    return lg, [kv_rows(m, spec, b, [pos[b]]) for b in range(len(pos))]


def feed_alone(one, spec, prompt, p):
    if p:
        one.prefill(prompt[:-1], 0)
    return one.forward([int(prompt[-1])], [p])[0][0].copy(), kv_rows(one, spec, 0, [p])


def check_rows(path, spec, lp, names, prompts, pos, lg, rows, tag, quant):
    """every row against the single-module model of its binding, same feeding; rows below 64 without a module against the base model's bits"""
    ones = {n: single(path, lp, n) for n in set(names)}
    for b, n in enumerate(names):
        want_lg, want_rows = feed_alone(ones[n], spec, prompts[b], pos[b])
        if n is None and pos[b] >= 64:                              # one split here, two in the base model: the fast path's own bar
            assert e2e.rel_err(lg[b], want_lg) < e2e.TOL[quant], (tag, b)
            continue
        same_bits(lg[b], want_lg, (tag, "logits of row", b, "module", n))
        same_bits(rows[b], want_rows, (tag, "K / V rows of row", b, "module", n))
    for o in ones.values():
        o.close()


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_four_rows_of_three_bindings_and_a_rebinding(model_dir, preset, quant, gs):
    path, spec, lp = files(model_dir, preset, quant, gs)
    names, pos = ["A", None, "B", "A"], (0, 11, 7, T)
    prompts = [mf.prompt_ids(300 + b, pos[b] + 1, spec.vocab_size) for b in range(4)]
    m = table_model(path, lp, 4)
    bind(m, names)
    lg, rows = feed_rows(m, spec, prompts, pos)
    check_rows(path, spec, lp, names, prompts, pos, lg, rows, (preset, quant), quant)
    assert bits(lg[0]).tolist() != bits(lg[3]).tolist()                                     # rows 0 and 3 share A and differ by their history
    base = single(path, lp, None)
    for b in (0, 3):
        assert e2e.rel_err(feed_alone(base, spec, prompts[b], pos[b])[0], lg[b]) > 1e-3, "module A changed nothing"
    base.close()
    # rebinding: slot 1 takes C, the table untouched; the same history again from position 0.  The step's graph is replayed: it must
    # read the new descriptor
    names[1] = "C"
    bind(m, names)
    lg, rows = feed_rows(m, spec, prompts, pos)
    check_rows(path, spec, lp, names, prompts, pos, lg, rows, (preset, quant, "slot 1 rebound to C"), quant)
    # a rank-8 entry over the rank-1 one (refused while slot 1 is bound to it): the graphs, captured with LDS for rank 8 = max(5, 8, 1)
    # all the same, are dropped and the new module's own bits come out
    with pytest.raises(nb.NanoHipError, match="nano_hip error -1:"):
        m.lora_table_set_file(ENTRY["C"], lp["D"])
    m.lora_bind([1], [None])
    m.lora_table_set_file(ENTRY["C"], lp["D"])
    m.lora_bind([1], [ENTRY["C"]])
    lg, rows = feed_rows(m, spec, prompts, pos)
    ones = single(path, lp, "D")
    want_lg, want_rows = feed_alone(ones, spec, prompts[1], pos[1])
    same_bits(lg[1], want_lg, (preset, quant, "entry overwritten by D: logits")); same_bits(rows[1], want_rows, (preset, quant, "entry overwritten by D: K / V"))
    ones.close()
    names[1] = None                                                                         # (the other rows: untouched by all that)
    check_rows(path, spec, lp, [names[0], names[2], names[3]], [prompts[0], prompts[2], prompts[3]], (pos[0], pos[2], pos[3]),
               lg[[0, 2, 3]], [rows[0], rows[2], rows[3]], (preset, quant, "after the overwrite"), quant)
    m.close()


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_ten_rows_cross_the_switch_to_the_gemms(model_dir, preset, quant, gs):
    path, spec, lp = files(model_dir, preset, quant, gs)
    names = [("A", "B", None, "C")[b % 4] for b in range(10)]
    pos = (0, 11, 7, T, 3, 5, 2, 9, 4, 6)
    prompts = [mf.prompt_ids(400 + b, pos[b] + 1, spec.vocab_size) for b in range(10)]
    m = table_model(path, lp, 10)
    bind(m, names)
    lg, rows = feed_rows(m, spec, prompts, pos)
    m.close()
    check_rows(path, spec, lp, names, prompts, pos, lg, rows, (preset, quant, "ten rows"), quant)


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_prefill_into_a_bound_slot(model_dir, preset, quant, gs):
    """70 tokens into slot 2 (bound to B) = slot 0 of a fresh model with B attached: the K / V rows and the four steps behind; slots 0
    and 1 (bound to A and to none) keep their rows"""
    path, spec, lp = files(model_dir, preset, quant, gs)
    ids = mf.prompt_ids(612, T + 4, spec.vocab_size)
    m = table_model(path, lp, 3)
    bind(m, ["A", None, "B"])
    m.prefill(ids[:9], 0, slot=0); m.prefill(ids[20:27], 0, slot=1)
    before = [kv_rows(m, spec, s, range(T + 4)) for s in (0, 1)]
    m.prefill(ids[:T], 0, slot=2)
    for s in (0, 1):
        same_bits(kv_rows(m, spec, s, range(T + 4)), before[s], (preset, quant, "slot", s, "changed"))
    fresh = single(path, lp, "B")
    fresh.prefill(ids[:T], 0)
    same_bits(kv_rows(m, spec, 2, range(T)), kv_rows(fresh, spec, 0, range(T)), (preset, quant, "slot 2 against slot 0 of a model with B attached"))
    for p in range(T, T + 4):
        # (rows 0 and 1 step along at their own positions: a decode step's rows are slots 0 .. nb - 1)
        got = m.forward([int(ids[9 + p - T]), int(ids[27 + p - T]), int(ids[p])], [9 + p - T, 7 + p - T, p])[0][2]
        same_bits(got, fresh.forward([int(ids[p])], [p])[0][0], (preset, quant, "step at position", p))
    m.close(); fresh.close()


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_decode_greedy_of_two_bound_slots(model_dir, preset, quant, gs):
    path, spec, lp = files(model_dir, preset, quant, gs)
    n_new = 80                                                  # crosses position 64
    prompts = [mf.prompt_ids(77 + b, 5, spec.vocab_size) for b in range(2)]
    m = table_model(path, lp, 2)
    bind(m, ["A", "B"])
    for b in range(2):
        m.prefill(prompts[b][:-1], 0, slot=b)
    got = m.decode_greedy([int(p[-1]) for p in prompts], [4, 4], n_new)
    m.close()
    for b, n in enumerate(("A", "B")):
        one = single(path, lp, n)
        one.prefill(prompts[b][:-1], 0)
        want = one.decode_greedy([int(prompts[b][-1])], [4], n_new)[:, 0].tolist()
        one.close()
        assert got[:, b].tolist() == want, (preset, quant, "slot", b, int(np.argmax(got[:, b] != np.asarray(want))))


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_a_row_without_a_module_beyond_position_64(model_dir, preset, quant, gs):
    path, spec, lp = files(model_dir, preset, quant, gs)
    pos = (3, T, 9)
    prompts = [mf.prompt_ids(500 + b, pos[b] + 1, spec.vocab_size) for b in range(3)]
    m = table_model(path, lp, 3)
    bind(m, ["A", None, "B"])
    lg, rows = feed_rows(m, spec, prompts, pos)
    m.close()
    alone = table_model(path, lp, 1)                            # the same row alone in a table model: batch invariance, bit for bit
    want_lg, want_rows = feed_alone(alone, spec, prompts[1], pos[1])
    alone.close()
    same_bits(lg[1], want_lg, (preset, quant, "logits")); same_bits(rows[1], want_rows, (preset, quant, "K / V rows"))
    base = single(path, lp, None)                               # the base model splits the range in two: test_gpu_e2e's fast-path bar
    base_lg, _ = feed_alone(base, spec, prompts[1], pos[1])
    base.close()
    err = e2e.rel_err(lg[1], base_lg)
    print(f"{preset}/{quant}: row without a module at position {T} against the base model: {err:.3e} (bar {e2e.TOL[quant]:g})")
    assert err < e2e.TOL[quant]


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_fork_takes_the_binding_along(model_dir, preset, quant, gs):
    path, spec, lp = files(model_dir, preset, quant, gs)
    ids = mf.prompt_ids(81, 30, spec.vocab_size)
    m = table_model(path, lp, 2)
    bind(m, ["A", None])
    m.prefill(ids[:20], 0, slot=0)
    m.kv_fork(0, 20, [1])
    assert m.lora_binding(1) == ENTRY["A"]
    conts = (ids[20:25], ids[25:30])                            # the two slots go different ways behind the shared prefix
    got = [m.forward([int(conts[0][t]), int(conts[1][t])], [20 + t, 20 + t])[0].copy() for t in range(5)]
    m.close()
    for b in range(2):
        one = single(path, lp, "A")
        one.prefill(ids[:20], 0)
        for t in range(5):
            same_bits(got[t][b], one.forward([int(conts[b][t])], [20 + t])[0][0], (preset, quant, "slot", b, "step", t))
        one.close()


CACHES = {"fp16": dict(kv_f16=True), "fp8": dict(kv_fp8=True, kv_f16=False, kv_paged=False), "paged": dict(kv_paged=True, kv_f16=False)}
ENTRIES = {"forward": lambda m, ids: m.forward([int(ids[0])], [0]),
           "greedy": lambda m, ids: m.decode_greedy([int(ids[0])], [0], 2),
           "prefill": lambda m, ids: m.prefill(ids[:5], 0),
           "prefill_score": lambda m, ids: m.prefill_score(ids[:5], ids[1:6]),
           "draft": lambda m, ids: m.verify_draft(ids[:4], 0),
           "lookup": lambda m, ids: m.decode_lookup(ids[:3], 4)}
RAGGED = {"step_rows": lambda m, ids: m.step_rows([(0, 0, 3)], ids[:3]),
          "step_rows_pool": lambda m, ids: m.step_rows_pool([(0, 0, 3)], ids[:3])}


def refused(call, m, ids, what):
    with pytest.raises(nb.NanoHipError, match="nano_hip error -1:"):
        call(m, ids)
    assert "LoRA" in nb.last_error(), (what, nb.last_error())


@pytest.mark.parametrize("cache", list(CACHES))
def test_gating_of_the_caches(model_dir, cache):
    path, spec, lp = files(model_dir, "tiny-nano", "f32", 0)
    ids = mf.prompt_ids(5, 12, spec.vocab_size)
    m = table_model(path, lp, 1, **CACHES[cache])
    bind(m, ["A"])
    for name, call in {**ENTRIES, **RAGGED}.items():
        refused(call, m, ids, (cache, name))
    m.lora_enable(False)
    never = single(path, lp, None, **CACHES[cache])
    for p in range(6):
        same_bits(m.forward([int(ids[p])], [p])[0][0], never.forward([int(ids[p])], [p])[0][0], (cache, "position", p))
    m.close(); never.close()


def test_gating_of_the_modes_and_the_ragged_steps(model_dir):
    path, spec, lp = files(model_dir, "tiny-nano", "f32", 0)
    ids = mf.prompt_ids(5, 12, spec.vocab_size)
    m = table_model(path, lp, 1)
    bind(m, ["B"])
    for name, call in RAGGED.items():
        refused(call, m, ids, name)
    for mode, switch in (("strict", m.set_strict), ("exact", m.set_exact)):
        switch(True)
        for name in ("forward", "prefill"):
            refused(ENTRIES[name], m, ids, (mode, name))
        switch(False)
    # the table and an attached module exclude each other, whichever comes second; the model goes on as it was
    with pytest.raises(nb.NanoHipError, match="nano_hip error -1:"):
        m.lora_attach_file(lp["A"])
    other = single(path, lp, "A")
    with pytest.raises(nb.NanoHipError, match="nano_hip error -1:"):
        other.lora_table_set_file(0, lp["B"])
    with pytest.raises(nb.NanoHipError, match="nano_hip error -1:"):
        other.lora_bind([0], [None])
    # refusals of the table calls on a live model: each leaves the bindings and the table as they were
    for call in (lambda: m.lora_bind([1], [0]), lambda: m.lora_bind([0, 0], [0, 1]), lambda: m.lora_bind([0], [7]), lambda: m.lora_bind([0], [64]),
                 lambda: m.lora_table_clear(ENTRY["B"]), lambda: m.lora_table_clear(9), lambda: m.lora_table_clear(64), lambda: m.lora_binding(1)):
        with pytest.raises(nb.NanoHipError, match="nano_hip error -1:"):
            call()
    assert m.lora_binding(0) == ENTRY["B"]
    wb, wa = single(path, lp, "B"), other
    same_bits(m.forward([int(ids[0])], [0])[0][0], wb.forward([int(ids[0])], [0])[0][0], "the table model after the refusals")
    same_bits(wa.forward([int(ids[0])], [0])[0][0], single_logits(path, lp, "A", ids), "the attached model after the refusals")
    wb.close(); wa.close(); m.close()


def single_logits(path, lp, name, ids):
    one = single(path, lp, name)
    lg = one.forward([int(ids[0])], [0])[0][0].copy()
    one.close()
    return lg


@pytest.mark.parametrize("preset,quant,gs", CASES)
def test_switching_the_table_off_and_on(model_dir, preset, quant, gs):
    """after steps and a prefill WITH the table, lora_enable(False): the same feeding from position 0 gives the bits of a model that never
    had a module; switched on again, the table's own bits"""
    path, spec, lp = files(model_dir, preset, quant, gs)
    ids = mf.prompt_ids(9, 12, spec.vocab_size)
    m, never = table_model(path, lp, 1), single(path, lp, None)
    bind(m, ["A"])
    with_table = [m.forward([int(ids[p])], [p])[0][0].copy() for p in range(6)]
    m.prefill(ids, 0)
    m.lora_enable(False)
    for p in range(6):
        base = never.forward([int(ids[p])], [p])[0][0]
        same_bits(m.forward([int(ids[p])], [p])[0][0], base, (preset, quant, "off", p))
        assert e2e.rel_err(with_table[p], base) > 1e-3
    m.lora_enable(True)
    for p in range(6):
        same_bits(m.forward([int(ids[p])], [p])[0][0], with_table[p], (preset, quant, "on again", p))
    m.close(); never.close()


def test_engine_table_in_a_child_process(model_dir):
    """nano_lora_table_load twice and nano_lora_bind: nano_forward_batch's arg-maxes over 12 steps, two sequences with modules A and B, equal
    those of two single-module contexts (tests/lora_table_engine_child.py)"""
    path, spec, lp = files(model_dir, "tiny-nano", "q80", 32)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lora_table_engine_child.py"), path, lp["A"], lp["B"], "12"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["table"][0] == out["single"][0] and out["table"][1] == out["single"][1], out
    assert out["single"][0] != out["single"][1]                  # the two modules lead the same prompt different ways
    assert out["refused"] == {"bind_empty": -1, "free_bound": -1, "load_missing": -1, "load_wrong_base": -1}, out
