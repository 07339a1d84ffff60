"""Constructed inputs of the device sampler (tests/test_gpu_sampler_paths.py), each stating what it is meant to reach.

Random logits almost never put a decision of the sampler on an edge, so every case here is built to put one there, and states
  * the class it reaches, observable from the device's result:
      ALL       n_sorted == n_candidates <= CAP     every candidate sorted in LDS
      SUPERSET  n_sorted <  n_candidates,  n_candidates > CAP, n_sorted >= nucleus     the histogram's bins hold the nucleus
      WIDE      n_sorted == n_candidates > CAP      the radix sort and the wide cut
      ARGMAX    temperature 0
      NONE      n_candidates == 0, status NANO_SAMPLE_FALLBACK
  * its tags: the edges it sits on (REQUIRED lists them all).
observe() computes class and tags of a case from the restatement (tests/sampler_ref.py) alone; tests/test_sampler_ref.py holds every
case to the tags it states and the union of the stated tags to REQUIRED, so that a later retune of an input cannot silently empty a
tag.  SUPERSET against WIDE is the one distinction the restatement cannot decide (it depends on the device's bins): where the nucleus
itself fits the LDS sorter observe() reports BIG and the GPU test settles it."""
import dataclasses
import functools

import numpy as np

import sampler_cases as sc
import sampler_ref as sr

CAP = 8192                       # NANO_SAMPLE_MAX_CANDIDATES
CHUNK = sr.CHUNK
VQ = sc.V_QWEN3                  # 151 936: 593.5 chunks
VMAX = 1024 * CHUNK              # SAMPLE_MAX_CHUNKS * SAMPLE_CHUNK
NINF = np.float32(-np.inf)
ALMOST1 = 0.99999994             # the largest float32 below 1: the largest coin random_f32 returns
ALL, SUPERSET, WIDE, ARGMAX, NONE, BIG = "ALL", "SUPERSET", "WIDE", "ARGMAX", "NONE", "BIG"
NO_HISTORY = np.zeros(0, np.uint32)


def below(x):
    return float(np.nextafter(np.float32(x), np.float32(0.0)))


# ---- logits constructors (each returns float32[V]) ------------------------------------------------------------------------------------
def rnd(V, seed, mode="plain", sigma=3.0):
    rng = np.random.default_rng(seed)
    l = (sigma * rng.standard_normal(V)).astype(np.float32)
    if mode == "peak":
        l[int(rng.integers(V))] += np.float32(30.0)
    elif mode == "ties":
        l = (np.round(l * 4.0) / 4.0).astype(np.float32)
    return l


def peak(V, j, floor):
    l = np.full(V, floor, np.float32)
    l[j] = 0.0
    return l


def spaced(V, K, stride=None):
    """K equal logits, the rest -inf: the probabilities 1/K (exact where K is a power of two), the stable order the index order"""
    l = np.full(V, NINF, np.float32)
    l[(np.arange(K) * V) // K if stride is None else stride * np.arange(K) + 1] = 0.0
    return l


def levels(V, seed, counts_values, rest):
    l = np.full(V, rest, np.float32)
    perm = np.random.default_rng(seed).permutation(V)
    at = 0
    for n, v in counts_values:
        l[perm[at:at + n]] = v
        at += n
    return l


def masked(V, seed, keep):
    rng = np.random.default_rng(seed)
    l = (3.0 * rng.standard_normal(V)).astype(np.float32)
    l[rng.random(V) >= keep] = NINF
    return l


def tied(V, seed, a, b, top, sign):
    """random logits below two equal maxima at a < b; sign < 0: every logit negative"""
    l = np.random.default_rng(seed).standard_normal(V).astype(np.float32)
    l = (np.minimum(l, 3.0) if sign > 0 else -np.abs(l) - np.float32(1.0)).astype(np.float32)
    l[a] = l[b] = top
    return l


def hist(V, seed, n, *more):
    h = np.random.default_rng(1000 + seed).integers(0, V, size=n).astype(np.uint32)
    return np.concatenate([h, np.array(more, np.uint32)]).astype(np.uint32)


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    V: int
    make: object                  # () -> logits
    cls: str
    tags: frozenset
    top_p: float = 0.9
    coins: tuple = (0.0, 0.37, ALMOST1)
    penalty: float = 1.0
    temperature: float = 1.0
    history: np.ndarray = NO_HISTORY

    @functools.cached_property
    def logits(self):
        l = np.ascontiguousarray(self.make(), np.float32)
        assert l.shape == (self.V,)
        l.setflags(write=False)
        return l

    def ref(self, coin):
        return sr.sample(self.logits, self.history, self.penalty, self.temperature, self.top_p, coin)

    def row(self, coin):
        return (self.penalty, self.temperature, self.top_p, coin, self.history)


def case(name, V, make, cls, tags=(), **kw):
    return Case(name, V, make, cls, frozenset(tags), **kw)


LDS_COINS = (0.0, 0.25, below(0.25), ALMOST1, 1.0)          # 0.25 of a power-of-two total is a stored running sum exactly
CASES = []

# a. vocabulary geometry: random logits with a penalty history at every V around a chunk, a 64-chunk scan step and the declared limit
for V in (2, 3, 255, 256, 257, 1023, 1025, 9000, 16384, 16385, VMAX):
    for mode in ("plain", "peak", "ties"):
        geo = {f"V={V}"} | ({"V%4"} if V % 4 else set()) | ({"V<chunk"} if V < CHUNK else set())
        CASES.append(case(f"vocab-{V}-{mode}", V, functools.partial(rnd, V, 7 * V + len(mode), mode),
                          WIDE if V == VMAX and mode != "peak" else ALL, geo,
                          penalty=1.2, history=hist(V, V, min(40, 2 * V)), coins=(0.0, 0.37, ALMOST1)))
CASES.append(case("vocab-9000-flat", 9000, lambda: np.zeros(9000, np.float32), WIDE, {"wide@V=9000"}))
CASES.append(case("vocab-9000-noisy", 9000, lambda: rnd(9000, 5, sigma=0.3), WIDE, {"wide@V=9000"}, top_p=0.99,
                  penalty=1.1, history=hist(9000, 3, 30)))

# b. where the denominator changes binade: one 0.0 over a floor of -20 (the sum climbs through ~10 binades before / behind the peak) or of
#    -inf (the sum is 0 up to the peak and 1.0 behind it: the one crossing is in the peak's chunk, every other chunk function applies)
for j, tags in ((0, {"cross@first-chunk"}), (255, {"cross@elem255"}), (256, {"cross@elem0"}), (16383, {"cross@lane63", "cross@elem255"}),
                (16384, {"cross@lane0", "cross@elem0"}), (65535, {"cross@lane63", "cross>=10"}), (VQ - 1, {"cross@padded-chunk", "cross>=10"})):
    CASES.append(case(f"binade-floor20-{j}", VQ, functools.partial(peak, VQ, j, -20.0), ALL, tags | {"nucleus=1"}, coins=(0.0, 1.0)))
for j, tags in ((0, set()), (255, {"cross@elem255"}), (256, {"cross@elem0"}), (16383, {"cross-only@63"}), (16384, {"cross-only@64"}),
                (65535, {"cross@lane63"}), (VQ - 1, {"cross@padded-chunk"}), (63 * CHUNK + 100, {"cross-only@63"}), (127 * CHUNK + 100, {"cross-only@127"})):
    CASES.append(case(f"binade-masked-{j}", VQ, functools.partial(peak, VQ, j, NINF), ALL, tags | {"cross-single", "masked:all-but-one", "nucleus=1"},
                      coins=(0.0, 1.0)))

# c. the LDS cut and draw at V = 1024: K equal logits, so the running sums are k / K (exact for K a power of two)
for K, top_p, tags, coins in (
        (64, 0.49, {"cut@k15", "r==sum", "r<sum-by-1ulp", "coin=0", "coin=1", "coin~1"}, LDS_COINS + (5.0 / 32.0, below(5.0 / 32.0), 0.5)),
        (16, 0.99, {"cut@k15", "r==sum"}, LDS_COINS),
        (33, 0.5, {"cut@k0", "cut@k0-block2"}, LDS_COINS),
        (5, 0.5, {"n0<6", "n0<16", "cut@tail"}, LDS_COINS),
        (1, 0.9, {"n0<6", "nucleus=1"}, LDS_COINS),
        (17, 2.0, {"no-cut", "zero-candidates", "top_p>1", "pick=n0-1"}, LDS_COINS),
        (6, 0.7, {"last=4", "n0<16", "cut@tail"}, LDS_COINS),
        (7, 0.8, {"last=5", "n0<16", "cut@tail"}, LDS_COINS),
        (15, 0.45, {"last=6", "n0<16", "cut@tail"}, LDS_COINS),
        (31, 0.8, {"cut@tail"}, LDS_COINS),
        (32, 1.0, {"no-cut", "zero-candidates", "top_p=1", "r==sum", "pick=n0-1"}, LDS_COINS),
        (48, 0.68, {"cut@k0"}, LDS_COINS),
        (48, 0.98, {"cut@k15"}, LDS_COINS)):
    CASES.append(case(f"lds-K{K}-p{top_p}", 1024, functools.partial(spaced, 1024, K), ALL, tags, top_p=top_p, coins=coins))
# a probability that EQUALS the cutoff is a candidate (p >= cutoff, infer.c:1064-1072): V - 1 equal tokens at top_p 0, p = cutoff = 1 / (V - 1)
CASES.append(case("cutoff-equal-V257", 257, functools.partial(spaced, 257, 256, 1), ALL, {"p==cutoff", "top_p=0", "nucleus=1"}, top_p=0.0, coins=(0.0, 0.37, 1.0)))
CASES.append(case("cutoff-equal-V16385", 16385, functools.partial(spaced, 16385, 16384, 1), WIDE, {"wide:p==cutoff", "top_p=0", "nucleus=1"}, top_p=0.0, coins=(0.0, 0.37, 1.0)))

# d. the candidate cap: K equal tokens around NANO_SAMPLE_MAX_CANDIDATES (one histogram bin: no superset smaller than all of them)
for K, cls, tags in ((8191, ALL, {"n=8191"}), (8192, ALL, {"n=8192"}), (8193, WIDE, {"n=8193", "wide:n%256==1"}), (16384, WIDE, {"wide:n%256==0"})):
    CASES.append(case(f"cap-K{K}", VQ, functools.partial(spaced, VQ, K, 9), cls, tags, top_p=0.49, coins=(0.0, 0.37, 1.0)))

# e. supersets: more candidates than the sorter holds, the nucleus inside the histogram's leading bins
for ci in (0, 1, 7, 10):
    seed, sigma, mode, rp, temp, top_p, nh = sc.CASES[ci]
    # (vector 10: 74 469 candidates at temperature 2 and top_p 0.99, a nucleus of 34 607 -- beyond the sorter whatever the bins say)
    CASES.append(case(f"golden-{ci}", VQ, functools.partial(sc.logits_of, seed, sigma, mode), WIDE if ci == 10 else SUPERSET, (), top_p=top_p, coins=sc.COINS,
                      penalty=rp, temperature=temp, history=sc.history_of(seed, nh)))
CASES.append(case("levels-superset", VQ, functools.partial(levels, VQ, 1, ((100, 6.0), (5000, 2.0), (30000, 0.0)), NINF), SUPERSET, {"masked"}, top_p=0.5))
CASES.append(case("levels-wide", VQ, functools.partial(levels, VQ, 2, ((100, 6.0), (20000, 2.0)), -4.0), WIDE, (), top_p=0.5))     # the middle level alone exceeds the cap

# f. top_p outside (0, 1): 100 peaks at 6.0 over -6.0
peaks100 = functools.partial(levels, VQ, 3, ((100, 6.0),), -6.0)
CASES.append(case("top_p=1", VQ, peaks100, WIDE, {"top_p=1", "wide:no-cut"}, top_p=1.0, coins=(0.0, 0.37, ALMOST1, 1.0)))
CASES.append(case("top_p=1.5", VQ, peaks100, WIDE, {"top_p>1", "wide:no-cut"}, top_p=1.5, coins=(0.0, 0.37, ALMOST1, 1.0)))
CASES.append(case("top_p=0", VQ, peaks100, ALL, {"top_p=0", "nucleus=1"}, top_p=0.0, coins=(0.0, 0.37, 1.0)))
CASES.append(case("top_p=-0.01", VQ, peaks100, ALL, {"top_p<0", "nucleus=1"}, top_p=-0.01, coins=(0.0, 0.37, 1.0)))
CASES.append(case("none-flat", VQ, lambda: np.zeros(VQ, np.float32), NONE, {"none@flat", "top_p<0"}, top_p=-0.01, coins=(0.37,)))
CASES.append(case("none-V2", 2, lambda: np.zeros(2, np.float32), NONE, {"none@V=2", "top_p=0"}, top_p=0.0, coins=(0.37,)))

# g. the wide cut and draw: 16 384 equal tokens (running sums k / 16384 exactly; top_p 0.49999 cuts at entry 8191, the last of chunk 31, and
#    coin k / 8192 makes r the running sum of entry k - 1: the draw is entry k), other counts, no cut, a cut at the first entry
W = functools.partial(spaced, VQ, 16384, 9)
CASES.append(case("wide-16384-cut8191", VQ, W, WIDE, {"wide:last@255", "wide:draw==cut-chunk", "wide:draw<cut-chunk", "wide:r==boundary-sum", "coin=1"},
                  top_p=0.49999, coins=tuple(k / 8192.0 for k in (0, 255, 256, 257, 511, 512, 7936, 8190, 8191)) + (below(256 / 8192.0), ALMOST1, 1.0)))
CASES.append(case("wide-16384-cut8192", VQ, W, WIDE, {"wide:last@0", "wide:draw==cut-chunk", "wide:draw<cut-chunk"}, top_p=0.50001,
                  coins=(0.0, 0.5, 8191.0 / 8193.0, 8192.0 / 8193.0, ALMOST1, 1.0)))
CASES.append(case("wide-16384-nocut", VQ, W, WIDE, {"wide:no-cut", "wide:pick=n0-1", "zero-candidates", "top_p>1"}, top_p=2.0,
                  coins=(0.0, 0.999, ALMOST1, 1.0)))
CASES.append(case("wide-16384-first", VQ, W, WIDE, {"wide:top_p<0", "top_p<0", "nucleus=1"}, top_p=-0.01, coins=(0.0, 0.37, 1.0)))
for K in (8448, 8449):
    CASES.append(case(f"wide-K{K}", VQ, functools.partial(spaced, VQ, K, 9), WIDE, {f"wide:n%256=={K % 256}"}, coins=(0.0, 0.37, 0.93, 1.0)))
CASES.append(case("wide-noisy", VQ, lambda: rnd(VQ, 5, sigma=0.3), WIDE, (), penalty=1.2, history=hist(VQ, 5, 100), coins=(0.0, 0.31, 0.77, ALMOST1)))

# h. masked vocabularies and arg-max ties after the penalty (two equal maxima at a < b; the penalised value decides, the first maximum wins)
CASES.append(case("masked-6/7", VQ, functools.partial(masked, VQ, 4, 1.0 / 7.0), SUPERSET, {"masked:most"}, penalty=1.3, history=hist(VQ, 4, 64)))
CASES.append(case("masked-6/7-V1025", 1025, functools.partial(masked, 1025, 4, 1.0 / 7.0), ALL, {"masked:most"}, penalty=1.3, history=hist(1025, 4, 20)))
TA, TB = 70001, 140002
for name, sign, pen, h, tag in (("pos-pen>1", 1, 1.5, (TA,), "tie:pen>1,pos"), ("pos-pen<1", 1, 0.5, (TB,), "tie:pen<1,pos"),
                                ("neg-pen>1", -1, 1.5, (TA,), "tie:pen>1,neg"), ("neg-pen<1", -1, 0.5, (TA,), "tie:pen<1,neg"),
                                ("both-penalised", 1, 1.5, (TA, TB), "tie:both"), ("plain", 1, 1.0, (), "tie:plain")):
    CASES.append(case(f"argmax-tie-{name}", VQ, functools.partial(tied, VQ, 6, TA, TB, 5.0 if sign > 0 else -0.5, sign), ARGMAX, {tag},
                      temperature=0.0, penalty=pen, history=hist(VQ, 9, 20 if h else 0, *h), coins=(0.0,)))
seed, sigma, mode, rp, temp, top_p, nh = sc.CASES[9]
CASES.append(case("golden-9", VQ, functools.partial(sc.logits_of, seed, sigma, mode), ARGMAX, (), temperature=temp, penalty=rp, top_p=top_p,
                  history=sc.history_of(seed, nh), coins=(0.0,)))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

REQUIRED = frozenset({
    # vocabulary geometry
    "V=2", "V=3", "V=255", "V=256", "V=257", "V=1023", "V=1025", "V=9000", "V=16384", "V=16385", f"V={VMAX}", "V%4", "V<chunk", "wide@V=9000",
    # binade crossings of the denominator
    "cross@first-chunk", "cross@elem0", "cross@elem255", "cross@lane0", "cross@lane63", "cross@padded-chunk", "cross>=10", "cross-single",
    "cross-only@63", "cross-only@64", "cross-only@127",
    # the LDS cut and draw
    "cut@k0", "cut@k15", "cut@k0-block2", "cut@tail", "n0<16", "n0<6", "last=4", "last=5", "last=6", "no-cut", "nucleus=1", "zero-candidates", "pick=n0-1",
    "coin=0", "coin=1", "coin~1", "r==sum", "r<sum-by-1ulp",
    # the cap
    "n=8191", "n=8192", "n=8193",
    # top_p outside (0, 1), no candidate
    "top_p=1", "top_p>1", "top_p=0", "top_p<0", "none@flat", "none@V=2", "p==cutoff", "wide:p==cutoff",
    # the wide cut and draw
    "wide:draw==cut-chunk", "wide:draw<cut-chunk", "wide:no-cut", "wide:top_p<0", "wide:last@255", "wide:last@0", "wide:n%256==0", "wide:n%256==1",
    "wide:r==boundary-sum", "wide:pick=n0-1",
    # masked and tied
    "masked", "masked:most", "masked:all-but-one", "tie:pen>1,pos", "tie:pen<1,pos", "tie:pen>1,neg", "tie:pen<1,neg", "tie:both", "tie:plain",
})


def observe(c):
    """(class, tags) of a case from the restatement alone, over all its coins"""
    V, l = c.V, c.logits
    tags = {f"V={V}"}
    if V % 4:
        tags.add("V%4")
    if V < CHUNK:
        tags.add("V<chunk")
    ninf = int(np.count_nonzero(l == NINF))
    if ninf:
        tags.add("masked")
        if 0.8 * V < ninf < V - 1:
            tags.add("masked:most")
        if ninf == V - 1:
            tags.add("masked:all-but-one")
    tp = np.float32(c.top_p)
    tags |= {t for t, on in (("top_p=1", tp == 1), ("top_p>1", tp > 1), ("top_p=0", tp == 0), ("top_p<0", tp < 0)) if on and c.temperature != 0.0}
    if c.temperature == 0.0:
        top = np.nonzero(l == l.max())[0]
        hit = np.intersect1d(top, c.history)
        if top.size >= 2:
            side = "pos" if l.max() > 0 else "neg"
            tags.add("tie:plain" if c.penalty == 1.0 else "tie:both" if hit.size == top.size else
                     f"tie:pen{'>' if c.penalty > 1 else '<'}1,{side}" if hit.size else "tie:unpenalised")
        return ARGMAX, tags
    d, n = sr.parts(l, c.history, c.penalty, c.temperature, c.top_p)
    el, ch = d.crossing_elems, sorted(d.crossings)
    tags |= {t for t, on in (("cross@first-chunk", 0 in ch), ("cross@elem0", bool(np.any((el % CHUNK == 0) & (el > 0)))),
                             ("cross@elem255", bool(np.any(el % CHUNK == CHUNK - 1))), ("cross@lane0", any(x % 64 == 0 and x for x in ch)),
                             ("cross@lane63", any(x % 64 == 63 for x in ch)), ("cross@padded-chunk", V % CHUNK != 0 and (V - 1) // CHUNK in ch),
                             ("cross>=10", len(ch) >= 10), ("cross-single", len(ch) == 1)) if on}
    if len(ch) == 1:
        tags.add(f"cross-only@{ch[0]}")
    if n.n0 == 0:
        return NONE, tags | {"none@V=2" if V == 2 else "none@flat" if np.all(l == l[0]) else "none"}
    n0, last = n.n0, n.last
    tags |= {f"n={n0}"} if abs(n0 - CAP) <= 1 else set()
    if last == 0:
        tags.add("nucleus=1")
    if n0 > int(np.count_nonzero(d.p)):
        tags.add("zero-candidates")
    lds = n0 <= CAP
    with np.errstate(divide="ignore"):
        if np.any(d.p == np.float32((np.float32(1.0) - tp) / np.float32(V - 1))):
            tags.add("p==cutoff" if lds else "wide:p==cutoff")
    if n0 > CAP and V == 9000:
        tags.add("wide@V=9000")
    blocks = 16 * (n0 // 16)                                    # entries the sixteen-wide cut loop covers
    if lds:
        tags |= {t for t, on in (("n0<16", n0 < 16), ("n0<6", n0 < 6), ("no-cut", not n.cut), ("cut@tail", n.cut and last >= blocks),
                                 ("cut@k0", n.cut and last < blocks and last % 16 == 0), ("cut@k15", n.cut and last < blocks and last % 16 == 15),
                                 ("cut@k0-block2", n.cut and last == 16 < blocks)) if on}
        if n.cut and last in (4, 5, 6):
            tags.add(f"last={last}")
    else:
        tags |= {t for t, on in (("wide:no-cut", not n.cut), ("wide:top_p<0", tp < 0), ("wide:last@255", n.cut and last % CHUNK == CHUNK - 1),
                                 ("wide:last@0", n.cut and last % CHUNK == 0 and last > 0), (f"wide:n%256=={n0 % CHUNK}", n0 % CHUNK < 2)) if on}
    for coin in c.coins:
        s = c.ref(coin)
        r = np.float32(s.r)
        sums = n.cdf[:last + 1]
        tags |= {t for t, on in (("coin=0", coin == 0.0), ("coin=1", coin == 1.0), ("coin~1", np.float32(coin) == np.float32(ALMOST1)),
                                 ("r==sum", bool(np.any(sums == r))), ("r<sum-by-1ulp", bool(np.any(sums == np.nextafter(r, np.float32(np.inf))))),
                                 ("pick=n0-1", lds and s.pick == n0 - 1 and not n.cut)) if on}
        if not lds:
            tags |= {t for t, on in (("wide:draw==cut-chunk", n.cut and s.pick // CHUNK == last // CHUNK), ("wide:draw<cut-chunk", n.cut and s.pick // CHUNK < last // CHUNK),
                                     ("wide:r==boundary-sum", bool(np.any(sums[CHUNK - 1::CHUNK] == r))), ("wide:pick=n0-1", not n.cut and s.pick == n0 - 1)) if on}
    return (ALL if lds else WIDE if last + 1 > CAP else BIG), tags
