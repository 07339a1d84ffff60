"""The numpy reference of the top-k entries (include/nano_mi355x.h NanoHipTopEntry), shared by the top-k tests.

The selection is exact: tokens are compared for equality with a stable descending sort (float comparison, ties by index), `logit` and
`logprob` bit for bit -- logprob against the float32 difference of the returned logit and the RETURNED lse of the row's score record.
The score record itself goes through score_ref.check_scores."""
import numpy as np

from score_ref import check_scores


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ref_topk(logits, k):
    """logits [rows, V] float32 -> [rows, k] indices: descending by float comparison (-0.0 == +0.0), equal floats by index"""
    l = np.asarray(logits, np.float32)
    return np.argsort(-l, axis=1, kind="stable")[:, :k].astype(np.uint32)


def check_topk(got_top, got_scores, logits, k, targets=None, what="", check_record=True):
    """Assert a [rows, k] TOP_ENTRY_DTYPE array and its TOKEN_SCORE_DTYPE records against the reference on `logits`."""
    l = np.asarray(logits, np.float32)
    rows = l.shape[0]
    assert got_top.shape == (rows, k), f"{what}: shape {got_top.shape}"
    want = ref_topk(l, k)
    assert np.array_equal(got_top["token"], want), f"{what}: tokens"
    r = np.arange(rows)[:, None]
    assert np.array_equal(bits(got_top["logit"]), bits(l[r, want])), f"{what}: logit is not the stored float"
    with np.errstate(invalid="ignore"):
        lp = got_top["logit"].astype(np.float32) - got_scores["lse"].astype(np.float32)[:, None]
    assert np.array_equal(bits(got_top["logprob"]), bits(lp)), f"{what}: logprob is not logit - lse"
    assert np.array_equal(got_top["token"][:, 0], got_scores["argmax"]), f"{what}: the first entry is not the record's arg-max"
    if targets is not None:
        t = np.asarray(targets, np.uint32).reshape(-1)
        among = (got_top["token"] == t[:, None]).any(axis=1)
        assert np.array_equal(got_scores["rank"] < k, among), f"{what}: rank < k exactly when the target is among the entries"
        for i in np.nonzero(among)[0]:
            e = got_top[i, int(got_scores["rank"][i])]
            assert e["token"] == t[i], f"{what}: row {i}: entry `rank` is not the target"
            assert bits(e["logprob"]) == bits(got_scores["logprob"][i]), f"{what}: row {i}: the target's logprob is not the record's"
    if check_record:
        check_scores(got_scores, l, targets, what)


# ---- the 64-bit key of topk.hip, restated: (ord(logit) << 32) | (0xffffffff - index); the LARGEST key is the first entry ----
def key_ord(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0                                   # -0.0f ties with +0.0f
    neg = (b & 0x80000000) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def keys(x):
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    return (key_ord(x).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(x.size, dtype=np.uint64))
