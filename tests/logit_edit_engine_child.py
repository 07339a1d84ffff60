"""Child process of tests/test_gpu_logit_edit_model.py: the engine reads NANO_HOST_SAMPLER once per process, so the device run and the host
run are processes of their own.  argv: model path, vocabulary.  Prints one JSON line:
  sess_edit / sess_cleared   24-step sessions (temperature 0.8, penalty 1.1, top_p 0.9, seed 77) with nano_set_logit_edit (ten allowed ids
                             plus a bias) and, in the same context, after clearing it;
  sess_plain                 the second of two such sessions of a context that never had an edit (the same coins as sess_cleared);
  greedy_edit / greedy_plain twelve ids of generate_next_token at temperature 0, penalty 1, with the edit and without;
  batch_edit / batch_plain   eight steps of nano_forward_batch_sample_edit over three sequences with per-sequence edits, and with none."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nano_amd import binding as nb     # noqa: E402

ALLOWED = [100, 131, 132, 163, 400, 511, 512, 777, 1000, 1023]
BIAS = ([131, 777, 5], [1.5, -0.5, 30.0])                     # (token 5 is not allowed: its bias changes nothing)
SEQ_ALLOWED = [[7, 8, 9, 600], None, [1, 1022]]
SEQ_BIAS = [None, ([300, 301], [4.0, 4.0]), ([1], [-2.0])]


def main():
    path, V = sys.argv[1], int(sys.argv[2])
    prompt = [int(x) for x in np.random.default_rng(6).integers(0, V, size=4)]
    w = nb.mask_words(ALLOWED, V)
    out = {}
    e = nb.Engine(path, max_seq_len=64, rep_pen=1.1, temperature=0.8, top_p=0.9, seed=77)
    e.set_logit_edit(w, BIAS)
    out["sess_edit"] = e.run_session(prompt, 40)[0][:24]
    e.set_logit_edit()
    out["sess_cleared"] = e.run_session(prompt, 40)[0][:24]
    e.close()
    e = nb.Engine(path, max_seq_len=64, rep_pen=1.1, temperature=0.8, top_p=0.9, seed=77)
    e.run_session(prompt, 40)
    out["sess_plain"] = e.run_session(prompt, 40)[0][:24]
    e.close()
    e = nb.Engine(path, max_seq_len=64)
    out["greedy_plain"] = [int(t) for t in e.generate(prompt, 12)[len(prompt):]]
    e.set_logit_edit(w, BIAS)
    out["greedy_edit"] = [int(t) for t in e.generate(prompt, 12)[len(prompt):]]
    e.close()
    for name, edits in (("batch_edit", [(nb.mask_words(a, V) if a else None, b) for a, b in zip(SEQ_ALLOWED, SEQ_BIAS)]), ("batch_plain", None)):
        e = nb.Engine(path, max_seq_len=64, max_batch=3)
        samplers = [e.build_sampler(V, 1.1, [1.0, 0.7, 0.0][s], 0.9, 100 + s) for s in range(3)]
        ids = [[prompt[s], prompt[(s + 1) % 4]] for s in range(3)]
        e.forward_batch([i[0] for i in ids], [0, 0, 0], want_logits=False)
        for p in range(1, 9):
            got = e.forward_batch_sample([i[p] for i in ids], [p] * 3, samplers, [np.array(i[:p], np.uint32) for i in ids], edits=edits)
            for s in range(3):
                ids[s].append(int(got[s]))
        out[name] = [i[2:] for i in ids]
        for sp in samplers:
            e.free_sampler(sp)
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
