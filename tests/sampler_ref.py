"""A plain restatement of the reference's sampler that returns every field the device sampler reports (tests only).

generate_next_token (infer/infer.c:1156-1189), softmax (:616-634) and sample_top_p (:1062-1109) in numpy, one step per line of the
recipe below.  The oracle (oracle/nano_oracle.c orc_sample_logits) returns the token and the candidate count only; this returns the
denominator's bits, the nucleus, the six most probable tokens, whether the cut loop found a cut, the draw's position and the chunks
in which the denominator changes binade as well.  tests/test_sampler_ref.py pins it: to the compiled reference's golden
(tests/golden/sampler_logits.npz), to the oracle's sampler on every case of tests/sampler_path_cases.py and, bit for bit, to the
oracle's softmax -- which ties the libm called here to the one the oracle links.

  1. the logits of the distinct history ids are divided by the penalty, once each;
  2. temperature 0: the first maximum;
  3. divide by the temperature;
  4. subtract the first maximum, expf (the host libm through ctypes: numpy's float32 exp is not glibc's bit for bit);
  5. the denominator is a sequential float32 sum in index order (np.cumsum is sequential);
  6. p = e / sum;
  7. cutoff = (1.0f - top_p) / (V - 1) in float32;
  8. candidates: p >= cutoff, in index order;
  9. a stable sort by probability, descending (glibc's qsort is a merge sort);
 10. cdf = the sequential float32 running sum of the sorted probabilities;
 11. last = the first cdf > top_p, else n0 - 1;
 12. r = coin * cdf[last];
 13. pick = the first cdf[:last + 1] > r, else last.
"""
import ctypes
import ctypes.util
import dataclasses
import hashlib

import numpy as np

CHUNK = 256          # SAMPLE_CHUNK: elements per chunk function of the device's denominator

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


def expf(x):
    """libm's expf over a float32 array: called once per distinct argument (constructed vectors have a handful)."""
    x = np.ascontiguousarray(x, np.float32)
    u, inv = np.unique(x.view(np.uint32), return_inverse=True)        # by bits: -0.0 / 0.0 and the NaNs stay apart
    out = np.array([_libm.expf(float(v)) for v in u.view(np.float32)], np.float32)
    return out[inv.reshape(x.shape)]


def exp_field(bits):
    """exponent field of float32 bits with 0 folded to 1 (exact_math.h sum_exp)"""
    f = np.asarray(bits, np.uint32) >> np.uint32(23)
    return np.where(f == 0, np.uint32(1), f)


@dataclasses.dataclass(frozen=True)
class Dist:
    """steps 1-6"""
    y: np.ndarray                  # penalised, tempered logits
    p: np.ndarray                  # probabilities
    sum_bits: int                  # the denominator's bits
    crossings: frozenset           # chunks in which the running sum's exponent field changes, from the empty sum
    crossing_elems: np.ndarray     # the elements behind which it has changed


@dataclasses.dataclass(frozen=True)
class Nucleus:
    """steps 7-11"""
    n0: int
    order: np.ndarray              # candidate ids, sorted
    cdf: np.ndarray
    last: int
    cut: bool


@dataclasses.dataclass(frozen=True)
class Sample:
    token: int
    n_candidates: int
    none: bool = False             # no candidate at all: the reference indexes probindex[-1]; only that fact is returned
    argmax: bool = False           # temperature 0: only the token
    sum_bits: int = 0
    nucleus: int = 0
    top: tuple = (0,) * 6
    cut: bool = False
    last: int = 0
    pick: int = 0
    r: float = 0.0
    crossings: frozenset = frozenset()


_dist_cache, _nucleus_cache = {}, {}


def penalised(logits, history, penalty, temperature):
    y = np.array(logits, np.float32).reshape(-1)
    ids = np.unique(np.asarray(history, np.int64).reshape(-1))
    y[ids] = y[ids] / np.float32(penalty)
    if temperature != 0.0:
        y = y / np.float32(temperature)
    return y


def distribution(y):
    key = hashlib.blake2b(y.tobytes(), digest_size=16).digest()
    d = _dist_cache.get(key)
    if d is None:
        with np.errstate(invalid="ignore", over="ignore"):
            e = expf(y - y[int(np.argmax(y))])
            csum = np.cumsum(e, dtype=np.float32)
            p = e / csum[-1]
        f = exp_field(csum.view(np.uint32))
        el = np.nonzero(f != np.concatenate([[np.uint32(1)], f[:-1]]))[0]
        d = Dist(y, p, int(csum[-1:].view(np.uint32)[0]), frozenset(int(c) for c in np.unique(el // CHUNK)), el)
        _dist_cache[key] = d
    return d, key


def nucleus(d, key, top_p):
    V = d.p.size
    tp = np.float32(top_p)
    k = (key, tp.tobytes())
    n = _nucleus_cache.get(k)
    if n is None:
        with np.errstate(divide="ignore"):
            cutoff = np.float32((np.float32(1.0) - tp) / np.float32(V - 1))
        idx = np.nonzero(d.p >= cutoff)[0]
        order = idx[np.argsort(-d.p[idx], kind="stable")]
        cdf = np.cumsum(d.p[order], dtype=np.float32)
        above = np.nonzero(cdf > tp)[0]
        n = Nucleus(int(idx.size), order, cdf, int(above[0]) if above.size else int(idx.size) - 1, bool(above.size))
        _nucleus_cache[k] = n
    return n


def sample(logits, history, penalty, temperature, top_p, coin):
    y = penalised(logits, history, penalty, temperature)
    if temperature == 0.0:
        return Sample(int(np.argmax(y)), 0, argmax=True)
    d, key = distribution(y)
    n = nucleus(d, key, top_p)
    if n.n0 == 0:
        return Sample(0, 0, none=True, sum_bits=d.sum_bits, crossings=d.crossings)
    r = np.float32(coin) * n.cdf[n.last]
    above = np.nonzero(n.cdf[:n.last + 1] > r)[0]
    pick = int(above[0]) if above.size else n.last
    top = tuple(int(t) for t in n.order[:6]) + (0,) * max(0, 6 - n.n0)
    return Sample(int(n.order[pick]), n.n0, sum_bits=d.sum_bits, nucleus=n.last + 1, top=top, cut=n.cut, last=n.last, pick=pick,
                  r=float(r), crossings=d.crossings)


def parts(logits, history, penalty, temperature, top_p):
    """(Dist, Nucleus) behind sample(): the sorted order and the running sums, for tests that probe many coins"""
    d, key = distribution(penalised(logits, history, penalty, temperature))
    return d, nucleus(d, key, top_p)
