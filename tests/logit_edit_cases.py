"""Overlays of the logit-edit tests: a row of the device sampler plus a mask and / or a bias list, each built to sit on one edge of the edit
(tests/test_logit_edit_ref.py on the CPU, tests/test_gpu_logit_edit.py on the device).

Vocabularies: tiny-qwen3's 1024 (32 full mask words, one prep window) and 9000 (281 full words plus a tail word with 8 live bits, eight full
windows of the prep kernel plus a partial ninth, more tokens than the LDS sorter holds: superset and wide phases are reachable)."""
import dataclasses

import numpy as np

import logit_edit_ref as er
import sampler_path_cases as pc

VT, VB = 1024, 9000
COINS = (0.0, 0.37, pc.ALMOST1)
NINF = np.float32(-np.inf)


@dataclasses.dataclass(frozen=True, eq=False)
class Overlay:
    name: str
    V: int
    logits: np.ndarray
    allow: object = None             # mask words, or None
    bias: object = None              # (tokens, values), or None
    top_p: float = 0.9
    top_k: int = 0
    penalty: float = 1.0
    temperature: float = 1.0
    history: np.ndarray = pc.NO_HISTORY
    coins: tuple = COINS

    def row(self, coin):
        return (self.penalty, self.temperature, self.top_p, coin, self.history)

    def edit(self):
        return {"allow": self.allow, "bias": self.bias}

    def ref(self, coin):
        return er.sample(self.logits, self.history, self.penalty, self.temperature, self.top_p, coin, self.top_k, self.allow, self.bias)

    def edited(self):
        return er.edited(self.logits, self.allow, self.bias)

    def on(self):
        return er.allowed(self.allow, self.V)


_base = {}


def base(V):
    """random logits, sigma 1: a nucleus of hundreds at V = 1024; at V = 9000 more candidates than the sorter holds"""
    if V not in _base:
        _base[V] = pc.rnd(V, 31, sigma=1.0)
        _base[V].setflags(write=False)
    return _base[V]


def only(V, *ids):
    return er.words(np.array(ids), V)


def pattern(V, word):
    return np.full(-(-V // 32), word, np.uint32)


def build():
    out = []

    def add(name, V, logits=None, **kw):
        out.append(Overlay(f"{name}-V{V}", V, base(V) if logits is None else logits, **kw))

    for V in (VT, VB):
        l = base(V)
        top = int(np.argmax(l))
        second = int(np.argsort(-l, kind="stable")[1])
        # ---- masks
        for j in (0, V - 1, 31, 32):
            add(f"mask-only-{j if j != V - 1 else 'last'}", V, allow=only(V, j))
        add("mask-all-but-argmax", V, allow=er.words(np.arange(V) != top, V))
        add("mask-0x55555555", V, allow=pattern(V, 0x55555555))
        add("mask-0xAAAAAAAA", V, allow=pattern(V, 0xAAAAAAAA))
        add("mask-nibbles", V, allow=pattern(V, 0x87654321))                      # eight nibbles, all different
        add("mask-t0-all-but-argmax", V, allow=er.words(np.arange(V) != top, V), temperature=0.0, coins=(0.0,))
        add("mask-0x55555555-k3", V, allow=pattern(V, 0x55555555), top_k=3)
        # ---- bias lists
        edge = sorted({0, 1023, V - 1} | ({1024} if V > 1024 else set()))
        add("bias-edges", V, bias=(np.array(edge), np.array([6.0, 5.5, 5.0, 4.5][:len(edge)], np.float32)))
        add("bias-moves-argmax", V, bias=(np.array([second]), np.array([20.0], np.float32)))
        add("bias-ninf-on-argmax", V, bias=(np.array([top]), np.array([NINF], np.float32)))
        add("bias-on-disallowed", V, allow=er.words(np.arange(V) != second, V), bias=(np.array([second]), np.array([50.0], np.float32)))
        add("bias-in-history", V, bias=(np.array([second, 7]), np.array([3.0, 9.0], np.float32)), penalty=1.1,
            history=np.array([second, 7, 11, second], np.uint32))
        rng = np.random.default_rng(77 + V)
        toks = rng.permutation(V)[:er.BIAS_MAX] if V > er.BIAS_MAX else rng.permutation(V)
        add("bias-max-shuffled", V, bias=(toks, rng.normal(0.0, 2.0, toks.size).astype(np.float32)))
        add("mask-and-bias", V, allow=pattern(V, 0x0F0FF0F0), bias=(toks[:300], rng.normal(0.0, 3.0, 300).astype(np.float32)), penalty=1.1,
            history=pc.hist(V, 5, 20))
        add("bias-t0-moves-argmax", V, bias=(np.array([second]), np.array([20.0], np.float32)), temperature=0.0, coins=(0.0,))
    # ---- V = 9000 only
    tail = np.zeros(-(-VB // 32), np.uint32)
    tail[-1] = 0xFFFFFFFF                                                         # tokens 8992 .. 8999 live, the 24 dead bits set as well
    out.append(Overlay("mask-tail-word-V9000", VB, base(VB), allow=tail))
    flat = np.zeros(VB, np.float32)
    flat.setflags(write=False)
    # equal logits: unedited, the leading bin alone exceeds the sorter (the wide phase); five allowed: every candidate sorted in LDS
    out.append(Overlay("flat-five-allowed-V9000", VB, flat, allow=only(VB, 3, 1000, 4095, 4096, 8999)))
    # equal logits, top_p = 1, every 16th token disallowed: 8437 allowed > 8192, the wide phase runs with the filter
    out.append(Overlay("flat-16th-banned-top_p1-V9000", VB, flat, allow=er.words(np.arange(VB) % 16 != 0, VB), top_p=1.0))
    return out


OVERLAYS = build()
BY_NAME = {o.name: o for o in OVERLAYS}
assert len(BY_NAME) == len(OVERLAYS)


def four_allowed(V):
    """four allowed tokens at top_p = 1: the case in which the filter differs from the unfiltered sampler on the edited logits"""
    l = pc.rnd(V, 41, sigma=1.0)
    ids = np.array([5, V // 3, V // 2 + 1, V - 2])
    return l, ids, er.words(ids, V)
