"""Constructed inputs of the device sampler with top_k (tests/test_gpu_sample_topk.py), each stating the class it reaches and the edges it
sits on, after tests/sampler_path_cases.py.

Classes, observable from the device's result:
    ALL       n_sorted == n_candidates <= CAP                    every candidate sorted in LDS
    SUPERSET  n_sorted <  n_candidates, n_candidates > CAP       the histogram's leading bins sorted in LDS, the result certified
    WIDE      n_sorted == n_candidates > CAP                     the radix sort and the wide cut, truncated
    ARGMAX    temperature 0
    NONE      n_candidates == 0, status NANO_SAMPLE_FALLBACK
observe() computes class and tags from the restatement (tests/sampler_topk_ref.py) and a numpy restatement of the histogram's bins alone;
tests/test_sampler_topk_ref.py holds every case to what it states and the union of the tags to REQUIRED.  With more candidates than CAP
the restatement says SUPERSET where the bins down to the one in which the count reaches max(top_k, 6) hold at most CAP tokens and entry
top_k - 1 of the sorted list lies strictly above every token behind those bins (the certificate of samp_pick), WIDE where the leading
bin alone exceeds CAP; anything between is BIG and no case may be that.

Vocabularies: tiny-qwen3's 1024 for everything that fits the LDS sorter, 9000 (a little above 8192 + 256) for more candidates than the
sorter holds, Qwen3's 151 936 (593.5 chunks) once."""
import dataclasses
import functools

import numpy as np

import sampler_path_cases as pc
import sampler_ref as sr
import sampler_topk_ref as tr

CAP, VQ, ALMOST1, NINF = pc.CAP, pc.VQ, pc.ALMOST1, pc.NINF
VT, VB = 1024, 9000
ALL, SUPERSET, WIDE, ARGMAX, NONE, BIG = pc.ALL, pc.SUPERSET, pc.WIDE, pc.ARGMAX, pc.NONE, pc.BIG
COINS = (0.0, 0.37, ALMOST1)
BINS = 256
UMAX = 0xFFFFFFFF


def exp_bin(e):
    """sampler.hip exp_bin: 8 bins per binade of a numerator in [0, 1], bin 7 = {1.0}, larger numerator -> smaller bin"""
    u = np.ascontiguousarray(e, np.float32).view(np.uint32).astype(np.int64)
    f = u >> 23
    b = (127 - f) * 8 + (7 - ((u >> 20) & 7))
    return np.where(f > 127, 0, np.minimum(b, BINS - 1))


def two_levels(V, n_top, low):
    """n_top tokens at 0.0 (numerator 1.0: bin 7 holds exactly them), spread over the vocabulary, the rest at `low` (one later bin)"""
    l = np.full(V, low, np.float32)
    l[(np.arange(n_top) * V) // n_top] = 0.0
    return l


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    V: int
    make: object
    top_k: int
    cls: str
    tags: frozenset
    top_p: float = 0.9
    coins: tuple = COINS
    penalty: float = 1.0
    temperature: float = 1.0
    history: np.ndarray = pc.NO_HISTORY

    @functools.cached_property
    def logits(self):
        l = np.ascontiguousarray(self.make(), np.float32)
        assert l.shape == (self.V,)
        l.setflags(write=False)
        return l

    def ref(self, coin, top_k=None):
        return tr.sample(self.logits, self.history, self.penalty, self.temperature, self.top_p, coin, self.top_k if top_k is None else top_k)

    def row(self, coin):
        return (self.penalty, self.temperature, self.top_p, coin, self.history)


def case(name, V, make, top_k, cls, tags=(), **kw):
    return Case(name, V, make, top_k, cls, frozenset(tags), **kw)


CASES = []
rnd3 = functools.partial(pc.rnd, VT, 11)                               # sigma 3: a nucleus of a few dozen tokens
rnd1 = functools.partial(pc.rnd, VT, 12, sigma=1.0)                    # sigma 1: a nucleus of hundreds
# k >= n_candidates: nothing changes
for k in (UMAX, VT, 1000):
    CASES.append(case(f"k>=n0-{k}", VT, rnd1, k, ALL, {"k>=n0"}))
CASES.append(case("k==n0", VT, functools.partial(pc.spaced, VT, 48), 48, ALL, {"k>=n0", "k==n0"}, top_p=0.99))
# top-p binds: the cut falls in front of entry k - 1
CASES.append(case("p-binds-k64", VT, rnd3, 64, ALL, {"p-binds"}))
CASES.append(case("p-binds-k6", VT, functools.partial(pc.rnd, VT, 13, "peak"), 6, ALL, {"p-binds", "nucleus=1"}))
# k binds, no cut: r = coin * cdf[k - 1]
for k in (20, 64, 17):
    CASES.append(case(f"k-binds-k{k}", VT, rnd1, k, ALL, {"k-binds"} | ({"k%16"} if k % 16 else {"k%16==0"})))
# k = 1: the first of the stable order, the lower index of two equal maxima
CASES.append(case("k1-tied-maxima", VT, functools.partial(pc.tied, VT, 14, 300, 600, 5.0, 1), 1, ALL, {"k=1", "equal-maxima", "k<6", "k-binds"}))
CASES.append(case("k1-plain", VT, rnd1, 1, ALL, {"k=1", "k<6", "k-binds"}))
# k < 6: top[k..5] == 0
for k in (2, 3, 5):
    CASES.append(case(f"k{k}-top-zeros", VT, rnd1, k, ALL, {"k<6", "k-binds"}))
CASES.append(case("k6-top-full", VT, rnd1, 6, ALL, {"k=6", "k-binds"}))
# equal probabilities across the k boundary: index order decides who is inside
CASES.append(case("tie@k-spaced", VT, functools.partial(pc.spaced, VT, 64), 20, ALL, {"tie@k", "k-binds"}))
CASES.append(case("tie@k-spaced-cut58", VT, functools.partial(pc.spaced, VT, 64), 64, ALL, {"k>=n0", "k==n0", "p-binds"}))
CASES.append(case("tie@k-ties", VT, functools.partial(pc.rnd, VT, 15, "ties", 1.0), 20, ALL, {"tie@k", "k-binds"}))
# more candidates than the sorter holds, random logits: the bins down to the k-th entry are sorted in LDS
rndB = functools.partial(pc.rnd, VB, 16, sigma=1.0)
for k in (20, 1000):
    CASES.append(case(f"big-rnd-k{k}", VB, rndB, k, SUPERSET, {"n0>cap", "k-binds"}, top_p=0.99))
CASES.append(case("big-ties-k64", VB, functools.partial(pc.rnd, VB, 17, "ties", 1.0), 64, SUPERSET, {"n0>cap", "k-binds", "tie@k"}, top_p=0.99))
CASES.append(case("qwen3-rnd-k20", VQ, functools.partial(pc.rnd, VQ, 18, sigma=1.0), 20, SUPERSET, {"n0>cap", "k-binds", f"V={VQ}"}))
# one bin holds more than the sorter: the wide phase, truncated
CASES.append(case("flat-k20", VB, lambda: np.zeros(VB, np.float32), 20, WIDE, {"n0>cap", "lead-bin>cap", "k-binds", "tie@k"}))
CASES.append(case("flat-k300", VB, lambda: np.zeros(VB, np.float32), 300, WIDE, {"n0>cap", "lead-bin>cap", "k-binds", "tie@k", "wide:k>chunk"}))
CASES.append(case("flat-k20-p-binds", VB, lambda: np.zeros(VB, np.float32), 20, WIDE, {"n0>cap", "lead-bin>cap", "p-binds"}, top_p=0.001))   # the cut at entry 9
# the count reaches k exactly at a bin's end (20 tokens of numerator 1.0, 8980 one bin later): certified at k <= 20; at k = 21 the second
# bin is needed and exceeds the sorter
for k, cls, tags in ((19, SUPERSET, set()), (20, SUPERSET, {"k@bin-end"}), (21, WIDE, {"k@bin-end+1"})):
    CASES.append(case(f"bin-end-k{k}", VB, functools.partial(two_levels, VB, 20, -1.0), k, cls, {"n0>cap", "k-binds"} | tags))
# penalty 1.1 with a history that holds the most probable tokens; temperature 0 with top_k set
HT = np.concatenate([np.argsort(-pc.rnd(VT, 12, sigma=1.0))[:3], pc.hist(VT, 19, 20)]).astype(np.uint32)
CASES.append(case("penalty-k5", VT, rnd1, 5, ALL, {"penalised", "k<6", "k-binds"}, penalty=1.1, history=HT))
CASES.append(case("penalty-big-k20", VB, rndB, 20, SUPERSET, {"penalised", "n0>cap", "k-binds"}, top_p=0.99, penalty=1.1,
                  history=np.concatenate([np.argsort(-pc.rnd(VB, 16, sigma=1.0))[:3], pc.hist(VB, 20, 30)]).astype(np.uint32)))
CASES.append(case("argmax-k7", VT, rnd1, 7, ARGMAX, {"argmax"}, temperature=0.0, penalty=1.1, history=HT, coins=(0.0,)))
# no candidate at all: the one case that may end in NANO_SAMPLE_FALLBACK
CASES.append(case("none-flat-k20", VB, lambda: np.zeros(VB, np.float32), 20, NONE, {"none"}, top_p=-0.01, coins=(0.37,)))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

REQUIRED = frozenset({"k>=n0", "k==n0", "p-binds", "k-binds", "k%16", "k%16==0", "k=1", "equal-maxima", "k<6", "k=6", "tie@k", "n0>cap", f"V={VQ}",
                      "lead-bin>cap", "wide:k>chunk", "nucleus=1", "k@bin-end", "k@bin-end+1", "penalised", "argmax", "none"})


def observe(c):
    """(class, tags) of a case from the restatement and the bins alone, over all its coins"""
    if c.temperature == 0.0:
        return ARGMAX, {"argmax"}
    d, n = sr.parts(c.logits, c.history, c.penalty, c.temperature, c.top_p)
    if n.n0 == 0:
        return NONE, {"none"}
    k, n0 = c.top_k, n.n0
    s = c.ref(c.coins[0])
    tags = set()
    if c.V == VQ:
        tags.add(f"V={VQ}")
    if k >= n0:
        tags |= {"k>=n0"} | ({"k==n0"} if k == n0 else set())
    else:
        tags |= {"k%16" if k % 16 else "k%16==0"} if not s.cut else set()
        if d.p[n.order[k - 1]] == d.p[n.order[k]]:
            assert n.order[k - 1] < n.order[k]
            tags.add("tie@k")
    if s.cut and s.nucleus < k:
        tags.add("p-binds")
    if not s.cut and k < n0:
        assert s.nucleus == k
        tags.add("k-binds")
    if s.nucleus == 1 and s.cut:
        tags.add("nucleus=1")
    tags |= {t for t, on in (("k=1", k == 1), ("k<6", k < 6), ("k=6", k == 6)) if on}
    if k == 1 and np.count_nonzero(d.p == d.p.max()) >= 2:
        tags.add("equal-maxima")
    if c.penalty != 1.0 and s.top != tr.sample(c.logits, [], 1.0, c.temperature, c.top_p, c.coins[0], k).top:
        tags.add("penalised")
    if n0 <= CAP:
        return ALL, tags
    tags.add("n0>cap")
    with np.errstate(invalid="ignore"):
        e = sr.expf(d.y - d.y[int(np.argmax(d.y))])
    cnt = np.cumsum(np.bincount(exp_bin(e[e != 0]), minlength=BINS))
    lead = int(np.nonzero(cnt)[0][0])
    bk = int(np.nonzero(cnt >= max(min(k, n0), 6))[0][0])
    if cnt[lead] > CAP:
        tags.add("lead-bin>cap")
    if k > sr.CHUNK and cnt[lead] > CAP:
        tags.add("wide:k>chunk")
    if k < n0 and cnt[bk] == k:
        tags.add("k@bin-end")
    if k < n0 and k > 6 and cnt[bk - 1] == k - 1 and bk > lead:
        tags.add("k@bin-end+1")
    if cnt[bk] > CAP:
        return (WIDE if cnt[lead] > CAP or "k@bin-end+1" in tags else BIG), tags
    behind = np.zeros(c.V, bool)
    behind[n.order] = True
    behind &= exp_bin(e) > bk                                          # candidates behind the sorted bins
    dropmax = float(d.p[behind].max()) if np.any(behind) else 0.0
    certified = k <= n0 and float(d.p[n.order[min(k, n0) - 1]]) > dropmax
    return (SUPERSET if certified else BIG), tags
