"""Child process of tests/test_gpu_kv_image.py: the restart case through the engine (nano_kv_save / nano_kv_restore).
argv: "save" | "resume", model path, image path, prompt length, decode steps.  Both feed greedy steps to sequence 0 of an Engine:
  save    ingests the prompt token by token, writes the KV image of its n positions to the image path, then decodes on;
  resume  ingests nothing: it restores the image and decodes the same steps.
Prints one JSON line: the greedy ids and a SHA-256 of every step's logits."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nano_amd import binding as nb     # noqa: E402
from nano_amd import modelfile as mf   # noqa: E402


def main():
    mode, path, image, n, steps = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
    spec = mf.read_header(path)
    prompt = mf.prompt_ids(313, n + 1, spec.vocab_size)
    e = nb.Engine(path, max_seq_len=256, max_batch=2)
    if mode == "save":
        for pos in range(n):
            e.forward_batch([int(prompt[pos])], [pos], want_logits=False)
        img = e.kv_save(0, n)
        assert img.size == e.kv_image_bytes(n)
        img.tofile(image)
    else:
        e.kv_restore(0, np.fromfile(image, np.uint8))
    ids, h, tok = [], hashlib.sha256(), int(prompt[n])
    for t in range(steps):
        lg = e.forward_batch([tok], [n + t], want_logits=True, vocab=spec.vocab_size)
        h.update(lg.tobytes())
        tok = int(np.argmax(lg[0]))
        ids.append(tok)
    e.close()
    print(json.dumps({"ids": ids, "logits_sha256": h.hexdigest()}))


if __name__ == "__main__":
    main()
