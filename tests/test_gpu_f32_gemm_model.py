"""GPU tests of FP32 models on the FP32 MFMA GEMM (nano_amd/csrc/gemm_f32.hip): 64-token prefill chunks and batched decode steps of
9..64 sequences.  The bar is the project's invariant: batched prefill is bit for bit token-by-token ingestion, a batch row is bit for
bit the sequence alone, and every result equals what the sliced GEMV route (NANO_MFMA_MIN_NB=65, the A/B switch) computes.
Models: tiny-nano and tiny-nano-odd (head_dim 48, hidden size 352: a ragged last unit) with block_size 256."""
import os

import numpy as np
import pytest

from nano_amd import binding as nb
from nano_amd import modelfile as mf
from fused_ref import bits

pytestmark = pytest.mark.gpu

S, T = 256, 150                          # 150 prompt tokens: two full chunks and a tail of 22
PRESETS = ["tiny-nano", "tiny-nano-odd"]


class min_nb:
    """NANO_MFMA_MIN_NB for the models created inside (read at model creation): 65 = the sliced GEMV route, the A/B switch"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.old = os.environ.get("NANO_MFMA_MIN_NB")
        if self.v is not None:
            os.environ["NANO_MFMA_MIN_NB"] = str(self.v)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("NANO_MFMA_MIN_NB", None)
        else:
            os.environ["NANO_MFMA_MIN_NB"] = self.old


_models = {}


def model_file(model_dir, preset):
    if preset not in _models:
        spec = mf.preset(preset, "f32", block_size=S)
        path = os.path.join(model_dir, f"f32gemm-{preset}.bin")
        mf.write_model(path, spec, seed=39)
        _models[preset] = (path, spec)
    return _models[preset]


def load(path, v=None, **kw):
    with min_nb(v):
        return nb.load_model_file(path, max_seq_len=S, **kw)


def state(m, spec, ids, pos0, slot=0):
    """every K and V row the prompt wrote, and the logits of the next step"""
    rows = np.stack([m.read_state(w, spec.kv_dim, slot=slot, layer=l, pos=pos0 + p) for l in range(spec.n_layer) for p in range(T) for w in ("k", "v")])
    return rows, m.forward([int(ids[T])], [pos0 + T])[0][0].copy()


_ref = {}


def token_by_token(model_dir, preset, pos0):
    """the reference of the prefill tests: one forward per prompt token (computed once per model and start position)"""
    if (preset, pos0) not in _ref:
        path, spec = model_file(model_dir, preset)
        ids = mf.prompt_ids(611, T + 1, spec.vocab_size)
        m = load(path)
        for p in range(T):
            m.forward([int(ids[p])], [pos0 + p], want_logits=False)
        _ref[(preset, pos0)] = (ids, *state(m, spec, ids, pos0))
        m.close()
    return _ref[(preset, pos0)]


def same_state(got, want, what):
    bad = np.argwhere(bits(got[0]) != bits(want[0]))
    assert not bad.size, (what, "KV rows differ at (row, element)", bad[:6])
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, "the next logits differ", float(np.abs(got[1] - want[1]).max()))


@pytest.mark.parametrize("preset", PRESETS)
def test_prefill_chunk_tokens(model_dir, preset):
    path, _ = model_file(model_dir, preset)
    m = load(path)
    assert m.prefill_chunk_tokens() == 64
    m.set_strict(True)
    assert m.prefill_chunk_tokens() == 1
    m.set_strict(False)
    m.close()
    m = load(path, 65)
    assert m.prefill_chunk_tokens() == 8
    m.close()


@pytest.mark.parametrize("pos0", [0, 5])
@pytest.mark.parametrize("preset", PRESETS)
def test_prefill_equals_token_by_token_and_the_sliced_route(model_dir, preset, pos0):
    """... and fed a second time, when the full chunks replay their graphs: the same bits"""
    path, spec = model_file(model_dir, preset)
    ids, ref_rows, ref_lg = token_by_token(model_dir, preset, pos0)
    for v in (None, 65):
        m = load(path, v)
        assert m.prefill_chunk_tokens() == (64 if v is None else 8)
        m.prefill(ids[:T], pos0)
        same_state(state(m, spec, ids, pos0), (ref_rows, ref_lg), (preset, pos0, v, "first run"))
        if v is None:
            m.prefill(ids[:T], pos0)
            same_state(state(m, spec, ids, pos0), (ref_rows, ref_lg), (preset, pos0, v, "second run: the chunk graphs replayed"))
        m.close()


@pytest.mark.parametrize("B", [9, 33, 64])
@pytest.mark.parametrize("preset", PRESETS)
def test_batched_forward_rows_equal_the_sequences_alone(model_dir, preset, B):
    """B sequences at distinct positions below 64 (one attention split for every batch size) on fresh caches"""
    path, spec = model_file(model_dir, preset)
    toks = mf.prompt_ids(900 + B, B, spec.vocab_size)
    pos = [(7 * b + 3) % 64 for b in range(B)]
    assert len(set(pos)) == B
    out = {}
    for v in (None, 65):
        m = load(path, v, max_batch=B)
        out[v] = m.forward([int(t) for t in toks], pos)[0].copy()
        m.close()
    assert np.array_equal(bits(out[None]), bits(out[65])), "differs from the sliced route"
    one = load(path)
    for b in sorted(range(B), key=lambda b: -pos[b]):              # descending positions: a later forward never attends an earlier one's row
        lg = one.forward([int(toks[b])], [pos[b]])[0][0]
        assert np.array_equal(bits(out[None][b]), bits(lg)), (b, pos[b], float(np.abs(out[None][b] - lg).max()))
    one.close()


@pytest.mark.parametrize("preset", PRESETS)
def test_prefill_score_equals_the_sliced_route(model_dir, preset):
    path, spec = model_file(model_dir, preset)
    ids = mf.prompt_ids(611, T + 1, spec.vocab_size)
    got = {}
    for v in (None, 65):
        m = load(path, v)
        got[v] = (m.prefill_score(ids[:T], ids[1:T + 1]).copy(), m.prefill_score(ids[:T], None).copy())
        m.close()
    for a, b in zip(got[None], got[65]):
        assert a.tobytes() == b.tobytes(), [(f, np.flatnonzero(a[f] != b[f])[:4]) for f in a.dtype.names if not np.array_equal(a[f], b[f])]


def test_lora_prefill_equals_the_sliced_route(model_dir):
    """Wo carries the LoRA addend and keeps the slices; q | k | v, W1|W3 and W2 take the GEMM"""
    path, spec = model_file(model_dir, "tiny-nano")
    lpath = os.path.join(model_dir, "f32gemm-tiny-nano.lora")
    mf.write_lora(lpath, spec, rank=4, alpha=8, seed=3)
    ids = mf.prompt_ids(611, T + 1, spec.vocab_size)
    got = {}
    for v in (None, 65):
        m = load(path, v)
        m.lora_attach_file(lpath)
        m.lora_enable(True)
        m.prefill(ids[:T], 0)
        got[v] = state(m, spec, ids, 0)
        m.close()
    same_state(got[None], got[65], "lora")
    assert not np.array_equal(bits(got[None][1]), bits(token_by_token(model_dir, "tiny-nano", 0)[2])), "the module changed nothing"


def test_paged_kv_prefill_equals_token_by_token(model_dir):
    path, spec = model_file(model_dir, "tiny-nano-odd")
    ids, ref_rows, ref_lg = token_by_token(model_dir, "tiny-nano-odd", 0)
    m = load(path, kv_paged=True)
    assert m.prefill_chunk_tokens() == 64
    m.prefill(ids[:T], 0)
    same_state(state(m, spec, ids, 0), (ref_rows, ref_lg), "paged")
    m.close()
