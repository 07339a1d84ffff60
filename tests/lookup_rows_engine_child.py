"""Child process of tests/test_gpu_lookup_rows_decode.py: lookup drafts for several sequences through the engine
(nano_decode_batch_lookup).  argv: model path, max_seq_len, max_draft, then per sequence "prompt seed:prompt length:max_new".
Sequence i ingests its prompt but the last id into slot i (nano_prefill_batch), then all decode in one call.
Prints one JSON line: {"ids": [ids of sequence 0, ...]}."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nano_amd import binding as nb     # noqa: E402
from nano_amd import modelfile as mf   # noqa: E402


def main():
    path, S, D = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    spec = mf.read_header(path)
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[4:]]
    prompts = [mf.prompt_ids(seed, n, spec.vocab_size) for seed, n, _ in cases]
    e = nb.Engine(path, max_seq_len=S, max_batch=len(cases))
    e.prefill_batch([p[:-1] for p in prompts], want_first_ids=False)
    ids = e.decode_batch_lookup(prompts, [mn for _, _, mn in cases], max_draft=D)
    e.close()
    print(json.dumps({"ids": [i.tolist() for i in ids]}))


if __name__ == "__main__":
    main()
