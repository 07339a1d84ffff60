"""Child process of tests/test_gpu_lora_table_model.py: the LoRA table through the engine (nano_lora_table_load / nano_lora_bind).
argv: model path, module A's path, module B's path, decode steps.  One context with both modules in its table, sequence 0 bound to A and
sequence 1 to B, steps both greedily from the same prompt through nano_forward_batch; then two single-module contexts (llm_context_init
with a module path) step the same prompt alone.  Also asks for the refusals an engine caller can meet.
Prints one JSON line: {"table": [ids of sequence 0, ids of sequence 1], "single": [ids with A, ids with B], "refused": {...}}."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nano_amd import binding as nb     # noqa: E402
from nano_amd import modelfile as mf   # noqa: E402


def greedy(e, n_seq, prompt, steps):
    """n_seq sequences ingest the prompt token by token, then decode greedily: the ids of each"""
    for pos in range(len(prompt) - 1):
        e.forward_batch([int(prompt[pos])] * n_seq, [pos] * n_seq, want_logits=False)
    tok, ids = [int(prompt[-1])] * n_seq, [[] for _ in range(n_seq)]
    for t in range(steps):
        am = e.forward_batch(tok, [len(prompt) - 1 + t] * n_seq, want_logits=False)
        tok = [int(a) for a in am]
        for s in range(n_seq):
            ids[s].append(tok[s])
    return ids


def code(call):
    try:
        call()
        return 0
    except nb.NanoHipError as err:
        return int(str(err).split("nano_hip error ")[1].split(":")[0])


def main():
    path, lora_a, lora_b, steps = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
    spec = mf.read_header(path)
    prompt = mf.prompt_ids(313, 6, spec.vocab_size)
    e = nb.Engine(path, max_seq_len=256, max_batch=2)
    e.lora_table_load(0, lora_a)
    e.lora_table_load_bytes(1, open(lora_b, "rb").read())
    refused = {"bind_empty": code(lambda: e.lora_bind([0], [5])), "load_missing": code(lambda: e.lora_table_load(2, lora_a + ".missing"))}
    wrong = bytearray(open(lora_a, "rb").read())
    hdr = np.frombuffer(wrong, np.uint32, 64)
    hdr[9] += 16                                                # n_embd of another base model
    refused["load_wrong_base"] = code(lambda: e.lora_table_load_bytes(2, bytes(wrong)))
    e.lora_bind([0, 1], [0, 1])
    refused["free_bound"] = code(lambda: e.lora_table_free(1))
    table = greedy(e, 2, prompt, steps)
    e.close()
    single = []
    for lp in (lora_a, lora_b):
        one = nb.Engine(path, max_seq_len=256, max_batch=1, lora_path=lp)
        single.append(greedy(one, 1, prompt, steps)[0])
        one.close()
    print(json.dumps({"table": table, "single": single, "refused": refused}))


if __name__ == "__main__":
    main()
