"""Print, for every case of tests/sampler_path_cases.py, what the device sampler reports next to the restatement (tests/sampler_ref.py).

    python tools/sampler_paths_probe.py > profiles/sampler_paths.txt        (one MI355X; needs the built library)

Per case (its first coin): vocabulary, the class it states, n_candidates, n_sorted, nucleus, the number of chunks in which the
softmax denominator changes binade (restatement) and the chunks the device added element by element (walked_chunks)."""
import dataclasses
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from nano_amd import binding as nb                      # noqa: E402
from nano_amd import modelfile as mf                    # noqa: E402
import sampler_path_cases as pc                         # noqa: E402


def main():
    models = {}
    print(f"{'case':28s} {'V':>6s} {'class':8s} {'n_cand':>6s} {'sorted':>6s} {'nucleus':>7s} {'cross':>5s} {'walked':>6s}  values")
    with tempfile.TemporaryDirectory() as d:
        for c in pc.CASES:
            if c.V not in models:
                path = os.path.join(d, f"V{c.V}.bin")
                mf.write_model(path, dataclasses.replace(mf.preset("bigvocab-qwen3"), vocab_size=c.V))
                models[c.V] = nb.load_model_file(path, max_seq_len=512, max_batch=1)
            coin = c.coins[0]
            s = c.ref(coin)
            r = models[c.V].op_sample(c.logits, c.history, c.penalty, c.temperature, c.top_p, coin)
            got = (r.token, r.status, r.n_candidates, r.nucleus, tuple(r.top), r.sum_bits)
            same = (r.token == s.token and r.status == 0) if s.argmax else (r.status == 1 and r.n_candidates == 0 and r.sum_bits == s.sum_bits) if s.none \
                else got == (s.token, 0, s.n_candidates, s.nucleus, s.top, s.sum_bits)
            nuc = "-" if s.argmax or s.none else str(r.nucleus)
            print(f"{c.name:28s} {c.V:6d} {c.cls:8s} {r.n_candidates:6d} {r.n_sorted:6d} {nuc:>7s} {len(s.crossings):5d} {r.walked_chunks:6d}  "
                  f"{'== restatement' if same else 'DIFFER'}")
        for m in models.values():
            m.close()


if __name__ == "__main__":
    main()
