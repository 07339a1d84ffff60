"""Numpy statement of the pooled final-norm vector (include/nano_mi355x.h, "text embeddings"), in two forms.

ordered   float32, every chain written out as the explicit ascending loop strict / exact mode run: the per-row norm through the
          oracle's rmsnorm (the reference's bits), the mean as (((y_0 + y_1) + y_2) + ...) / count, the normalisation's sum of squares
          in index order.  `cuts` carries the running sum across pass boundaries the way the kernel does (stored, loaded, continued).
float64   the same quantity in float64: what the fast path's fixed summation orders are measured against.
"""
import numpy as np

LAST, MEAN = 0, 1
F = np.float32


def pooling_id(pooling):
    return {"last": LAST, "mean": MEAN}[pooling] if isinstance(pooling, str) else int(pooling)


def norm_rows_ordered(oracle, x, w):
    """y_r = w * (x_r * rsqrt(mean(x_r^2) + 1e-5)) per row, through the oracle's rmsnorm (infer.c:601-614's order)"""
    x = np.ascontiguousarray(x, F)
    return np.stack([oracle.rmsnorm(r, w) for r in x]) if len(x) else np.zeros((0, x.shape[1]), F)


def norm_rows_f64(x, w):
    x = np.asarray(x, np.float64)
    return np.asarray(w, np.float64) * (x / np.sqrt((x * x).mean(axis=1, keepdims=True) + np.float64(F(1e-5))))


def pool_ordered(y, pooling="last", normalize=True, dim=0, cuts=()):
    """one segment: y [count, n_embd] float32 normed rows -> float32 [dim or n_embd].  cuts: row indices at which a pass ends"""
    y = np.ascontiguousarray(y, F)
    count, E = y.shape
    d = dim or E
    if count == 0:
        return np.zeros(d, F)
    if pooling_id(pooling) == LAST:
        v = y[-1].copy()
    else:
        acc = None                                                # the running sum a pass hands to the next (float32 in memory)
        edges = [0] + sorted(c for c in set(cuts) if 0 < c < count) + [count]
        for a, b in zip(edges[:-1], edges[1:]):                   # one pass: seeded from the stored sum if the segment began earlier
            part = None if acc is None else acc.copy()
            for r in range(a, b):
                part = y[r].copy() if part is None else part + y[r]      # (float32 arrays: one IEEE add per column)
            acc = part
        v = acc / F(count)
    v = v[:d].copy()
    if not normalize:
        return v
    s = F(0.0)
    for i in range(d):
        s = F(s + F(v[i] * v[i]))
    if not s > 0:
        return np.zeros(d, F)
    scale = F(F(1.0) / np.sqrt(s))
    return v * scale


def pool_f64(y, pooling="last", normalize=True, dim=0):
    y = np.asarray(y, np.float64)
    count, E = y.shape
    d = dim or E
    if count == 0:
        return np.zeros(d)
    v = (y[-1] if pooling_id(pooling) == LAST else y.sum(axis=0) / count)[:d]
    if not normalize:
        return v
    s = float((v * v).sum())
    return v / np.sqrt(s) if s > 0 else np.zeros(d)


def normalize_f64(v):
    """float64 normalisation of a vector as given (the kernel's own un-normalised float32 output)"""
    v = np.asarray(v, np.float64)
    s = float((v * v).sum())
    return v / np.sqrt(s) if s > 0 else np.zeros_like(v)


def embed_ordered(oracle, x, w, seg_count, pooling="last", normalize=True, dim=0):
    """a call: x [rows, n_embd] residual rows, segment after segment -> float32 [n_segs, dim or n_embd]"""
    x = np.ascontiguousarray(x, F)
    out, at = [], 0
    for c in seg_count:
        out.append(pool_ordered(norm_rows_ordered(oracle, x[at:at + c], w), pooling, normalize, dim))
        at += c
    return np.stack(out)
