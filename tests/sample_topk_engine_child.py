"""Child process of tests/test_gpu_sample_topk_model.py: the engine reads NANO_SAMPLE_TOP_K and NANO_HOST_SAMPLER once per process, so each
setting of them runs in a process of its own.  argv: model path, vocabulary.  Prints one JSON line: per top_k in (5, 0), twenty ids of
generate_next_token at temperature 1 (penalty 1.1, top_p 0.9, seed 77), and six steps of nano_forward_batch_sample over two sequences
whose samplers carry that top_k."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nano_amd import binding as nb     # noqa: E402


def main():
    path, V = sys.argv[1], int(sys.argv[2])
    prompt = [int(x) for x in np.random.default_rng(6).integers(0, V, size=4)]
    out = {}
    for k in (5, 0):
        e = nb.Engine(path, max_seq_len=32, rep_pen=1.1, temperature=1.0, top_p=0.9, top_k=k, seed=77)
        out[f"ids{k}"] = [int(t) for t in e.generate(prompt, 20)[len(prompt):]]
        e.close()
        e = nb.Engine(path, max_seq_len=32, max_batch=2)
        samplers = [e.build_sampler(V, 1.1, 1.0, 0.9, 100 + s, top_k=k) for s in range(2)]
        ids = [[prompt[s], prompt[s + 1]] for s in range(2)]
        e.forward_batch([ids[0][0], ids[1][0]], [0, 0], want_logits=False)
        for p in range(1, 7):
            got = e.forward_batch_sample([ids[0][p], ids[1][p]], [p, p], samplers, [np.array(ids[s][:p], np.uint32) for s in range(2)])
            for s in range(2):
                ids[s].append(int(got[s]))
        out[f"batch{k}"] = [ids[0][2:], ids[1][2:]]
        for sp in samplers:
            e.free_sampler(sp)
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
