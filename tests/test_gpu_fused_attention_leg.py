"""The attention leg of the one-sequence q|k|v + attention launch against the attention launch of its own.

attn_impl.h runs the fused launch's Qwen3 attention (head_dim 128, one q head per workgroup: the Q80 and the Q4K launch) through a body of
its own (FAST: one give-up vote and barrier, the fresh k / v row swapped into the one block that holds it, the sub-groups of a wave met
through LDS).  The plain attention launch (NANO_FUSE_LAUNCHES bit 0 off) still runs the general body.  Both must write the same bits:
every k and v cache row of every layer, the head outputs and the logits, at positions 0..71.  That covers the fresh row (t == pos) in
every sub-group of both blocks of one split (positions 0..63, range hint 64) and the steps past the 64 boundary, where the range hint
grows and the launch runs several splits."""
import numpy as np
import pytest

from conftest import synth_model
from nano_amd import binding as nb
from nano_amd import modelfile as mf

pytestmark = pytest.mark.gpu

NPOS = 72


def run(path, spec, mask):
    m = nb.load_model_file(path, max_seq_len=256, max_batch=1)
    try:
        m.set_fusion(mask)
        ids = mf.prompt_ids(11, NPOS, spec.vocab_size)
        logits, heads = [], []
        for pos in range(NPOS):
            lg, _ = m.forward([int(ids[pos])], [pos], want_logits=True)
            logits.append(np.array(lg[0]))
            heads.append(m.read_state("xba", spec.q_dim))                  # the last layer's head outputs of this step
        k = np.stack([m.read_state("k", spec.kv_dim, layer=l, pos=p) for l in range(spec.n_layer) for p in range(NPOS)])
        v = np.stack([m.read_state("v", spec.kv_dim, layer=l, pos=p) for l in range(spec.n_layer) for p in range(NPOS)])
        fused, fallbacks, _ = m.handoff_state()
        assert fused == mask and fallbacks == 0, (fused, fallbacks)
        return np.stack(logits), np.stack(heads), k, v
    finally:
        m.close()


@pytest.mark.parametrize("preset,quant", [("qwen3-0.6b-3l", "q80"), ("qwen3-0.6b-3l", "q4k")])
def test_fused_attention_leg_equals_the_plain_launch(model_dir, preset, quant):
    path, spec = synth_model(model_dir, preset, quant, 64 if quant == "q80" else 0)
    got = run(path, spec, 1)                                                 # q|k|v + attention in one launch
    want = run(path, spec, 0)                                                # q|k|v, then the attention launch
    for name, a, b in zip(("logits", "head outputs", "k rows", "v rows"), got, want):
        assert a.shape == b.shape, name
        bad = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (name, bad[:8].tolist())
