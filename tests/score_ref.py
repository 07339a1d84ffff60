"""The numpy reference of the row statistics (include/nano_mi355x.h NanoHipTokenScore), shared by the scoring tests.

Selections (arg-max, the maximum, the target's logit) and `rank` are exact and compared for equality; `lse` is taken in float64 and
compared within LSE_TOL = 1e-5 * max(1, |ref|), the tolerance the project holds its float32 reduction chains to (DESIGN.md section 1:
rmsnorm, attention); `logprob` must be the float32 difference of the RETURNED target_logit and lse, bit for bit."""
import numpy as np

LSE_TOL = 1e-5


def ref_scores(logits, targets=None):
    """logits [rows, V] float32 -> dict of arrays: argmax, max_bits, target_bits, rank, lse (float64)."""
    l = np.asarray(logits, np.float32)
    rows, V = l.shape
    am = np.argmax(l, axis=1).astype(np.uint32)                                   # first maximum
    t = am if targets is None else np.asarray(targets, np.uint32).reshape(-1)
    r = np.arange(rows)
    tl = l[r, t]
    idx = np.arange(V)[None, :]
    rank = ((l > tl[:, None]).sum(axis=1) + ((l == tl[:, None]) & (idx < t[:, None])).sum(axis=1)).astype(np.uint32)
    mx = l[r, am]
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = mx.astype(np.float64) + np.log(np.exp(l.astype(np.float64) - mx.astype(np.float64)[:, None]).sum(axis=1))
    return {"argmax": am, "max_bits": mx.view(np.uint32), "target_bits": tl.copy().view(np.uint32), "rank": rank, "lse": lse, "targets": t}


def check_scores(got, logits, targets=None, what="", lse_tol=LSE_TOL):
    """Assert a TOKEN_SCORE_DTYPE array against the reference on `logits`; returns the worst lse error relative to its bound."""
    ref = ref_scores(logits, targets)
    assert np.array_equal(got["argmax"], ref["argmax"]), f"{what}: argmax"
    assert np.array_equal(got["max_logit"].view(np.uint32), ref["max_bits"]), f"{what}: max_logit"
    assert np.array_equal(got["target_logit"].view(np.uint32), ref["target_bits"]), f"{what}: target_logit"
    assert np.array_equal(got["rank"], ref["rank"]), f"{what}: rank"
    err = np.abs(got["lse"].astype(np.float64) - ref["lse"]) / np.maximum(1.0, np.abs(ref["lse"]))
    assert np.all(err <= lse_tol), f"{what}: lse off by {err.max():.3e} (bound {lse_tol:g})"
    with np.errstate(invalid="ignore"):
        want_lp = got["target_logit"].astype(np.float32) - got["lse"].astype(np.float32)
    assert np.array_equal(got["logprob"].view(np.uint32), want_lp.view(np.uint32)), f"{what}: logprob is not target_logit - lse"
    if targets is None:
        assert not got["rank"].any(), f"{what}: the arg-max has rank 0"
    return float(err.max()) / lse_tol if err.size else 0.0
