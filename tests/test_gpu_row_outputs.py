"""GPU test of the entry families that hand back a result per fed row (verify-draft arg-maxes, scoring prefill, ragged steps, top-k
alternatives, the decode step with scores) taking turns on ONE model: they share one scratch owner (backend_rows.hip rows_scratch), and
the third call feeds more rows than max_seq_len, so the call buffers are replaced in the middle of the sequence.

Every call feeds its slots from position 0 and so needs no precondition: each result must equal, byte for byte, the same call made on a
fresh model that makes only that call."""
import os

import numpy as np
import pytest

from nano_amd import binding as nb
from nano_amd import modelfile as mf

pytestmark = pytest.mark.gpu

# preset, quant, group size, max_batch, max_seq_len, tokens of a prefill, rows per slot of the ragged step, mode
#   chunks of 64 / chunks of 8 with a decode step of more rows (9) than a chunk / exact mode: one reference-order step per row, on a smaller
#   max_seq_len so that rows per slot > max_seq_len / 2 still outgrows the call buffers
CASES = {"q80 chunks of 64": ("tiny-qwen3", "q80", 64, 4, 96, 70, 30, None),
         "f32 chunks of 8": ("tiny-nano", "f32", 0, 9, 96, 70, 30, None),
         "q80 exact": ("tiny-qwen3", "q80", 64, 4, 24, 20, 13, "exact")}


def same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("case", list(CASES))
def test_entry_families_take_turns(model_dir, case):
    preset, quant, gs, B, S, T, n, mode = CASES[case]
    spec = mf.preset(preset, quant, group_size=gs, block_size=256)
    path = os.path.join(model_dir, f"rowout-{preset}-{quant}-{gs}.bin")
    if not os.path.exists(path):
        mf.write_model(path, spec, seed=39)

    def load():
        m = nb.load_model_file(path, max_seq_len=S, max_batch=B)
        if mode == "exact":
            m.set_exact(True)
        return m

    V = spec.vocab_size
    ids = mf.prompt_ids(77, T + 1, V)
    segs = [(s, 0, n) for s in range(B)]
    assert B * n > S                                                         # the call buffers hold max_seq_len rows until a call needs more
    rows = np.concatenate([mf.prompt_ids(500 + s, n + 1, V)[:n] for s in range(B)])
    rows_tg = np.concatenate([mf.prompt_ids(500 + s, n + 1, V)[1:] for s in range(B)])
    step_tok, step_tg = mf.prompt_ids(78, B, V), mf.prompt_ids(79, B, V)
    calls = [lambda m: m.verify_draft(ids[:T]),                              # crosses a chunk and (T = 70) the 64-position bucket
             lambda m: m.prefill_score(ids[:T], ids[1:T + 1], slot=1),
             lambda m: m.step_rows_score(segs, rows, 20, rows_tg),
             lambda m: m.prefill_score_topk(ids[:T], 5, ids[1:T + 1]),
             lambda m: m.forward_topk(step_tok, np.zeros(B, np.uint32), 20, step_tg),
             lambda m: m.step_rows(segs, rows, want_argmax=True),
             lambda m: m.verify_draft(ids[:T])]
    m = load()
    got = [call(m) for call in calls]
    m.close()
    for i, call in enumerate(calls):
        fresh = load()
        want = call(fresh)
        fresh.close()
        assert same(got[i], want), f"{case}: call {i + 1} differs from the same call on a fresh model"
    assert same(got[6], got[0])
    assert np.array_equal(got[5], got[2][0]["argmax"])
