"""Greedy decode with lookup drafts, restated in plain Python (nano_amd/csrc/lookup.hip is the device form).

Nothing here imports the native library: the CPU tests check these definitions against each other, the GPU tests check the kernel
and the loop against them.

History h[0..n), n >= 1.  Parameters: max_draft D in 0..15, 1 <= ngram_min <= ngram_max <= 4, stop_token (NO_STOP = none).  K = D + 1.
"""
NO_STOP = 0xFFFFFFFF
NONE = 0xFFFFFFFF          # what the operator entry leaves in unused rows of the next step
MAX_ROWS = 16


def match_len(h, e, ngram_max):
    """L(e): how many j = 0, 1, .. < min(ngram_max, e) have h[e-1-j] == h[n-1-j], counted from j = 0 up to the first mismatch."""
    n = len(h)
    L = 0
    while L < min(ngram_max, e) and h[e - 1 - L] == h[n - 1 - L]:
        L += 1
    return L


def find_match(h, ngram_min, ngram_max):
    """The definition, two loops: over the lengths from the longest down, over the ends from the most recent down.
    Returns (L, e) or None."""
    n = len(h)
    for L in range(ngram_max, ngram_min - 1, -1):
        for e in range(n - 1, 0, -1):
            if match_len(h, e, ngram_max) == L:
                return L, e
    return None


def find_match_key(h, ngram_min, ngram_max):
    """The single pass the kernel makes: the maximum of (L(e) << 32) | e over the ends whose L(e) >= ngram_min.  (L, e) or None."""
    best = 0
    for e in range(1, len(h)):
        L = match_len(h, e, ngram_max)
        if L >= ngram_min:
            best = max(best, (L << 32) | e)
    return (best >> 32, best & 0xFFFFFFFF) if best else None


def draft(h, e, D):
    """d[i] = h[e+i] while e+i < n, then d[e+i-n]: the periodic extension."""
    n = len(h)
    d = []
    for i in range(D):
        d.append(h[e + i] if e + i < n else d[e + i - n])
    return d


def accepted(fed, amax):
    """a: the largest a <= nb-1 with fed[i] == amax[i-1] for all 1 <= i <= a."""
    a = 0
    while a + 1 < len(fed) and fed[a + 1] == amax[a]:
        a += 1
    return a


def step(h, fed, amax, left, D, ngram_min, ngram_max, stop_token, seq_limit):
    """What lookup_step_kernel does behind a step that fed `fed` and left the row arg-maxes `amax` (both empty: no step has run).
    Returns (record dict, new history, next tokens, next positions)."""
    h = list(h)
    nb = len(fed)
    a = emitted = 0
    done = left == 0
    if nb:
        a = accepted(fed, amax)
        for i in range(min(a + 1, left)):
            h.append(amax[i])
            emitted += 1
            if amax[i] == stop_token:
                done = True
                break
        left -= emitted
        if left == 0:
            done = True
    n = len(h)
    m = find_match_key(h, ngram_min, ngram_max) if (not done and D >= 1 and n >= 2) else None
    K = D + 1
    nb_next = 0 if done else 1
    if not done and m and D >= 1 and left >= 2 and (n - 1) % 64 + K <= 64 and n - 1 + K <= seq_limit:
        nb_next = K
    toks, pos = [], []
    if not done:
        toks, pos = [h[n - 1]], [n - 1]
        if nb_next == K and K > 1:
            toks += draft(h, m[1], D)
            pos += [n + i for i in range(D)]
    rec = {"emitted": emitted, "accepted": a, "nb_next": nb_next, "n": n, "match_len": m[0] if m else 0, "match_end": m[1] if m else 0,
           "done": int(done), "left": left}
    return rec, h, toks, pos


RECORD_FIELDS = ("emitted", "accepted", "nb_next", "n", "match_len", "match_end", "done", "left")


def simulate(history, truth, max_new, D, ngram_min=1, ngram_max=3, stop_token=NO_STOP, seq_limit=1 << 30, max_steps=0):
    """The loop against a model that always answers with the truth: truth[i] is the greedy id at index len(history) + i of the
    sequence whatever was drafted (which is what a verify chunk's accepted rows compute).  Returns (emitted ids, stats dict)."""
    h = list(history)
    n0 = len(h)
    full = list(history) + list(truth)
    stats = {"steps_plain": 0, "steps_verify": 0, "drafted": 0, "accepted": 0, "emitted": 0}
    rec, h, toks, pos = step(h, [], [], max_new, D, ngram_min, ngram_max, stop_token, seq_limit)
    steps = 0
    while not rec["done"] and not (max_steps and steps == max_steps):
        steps += 1
        # row i is fed toks[i] at position pos[i]; its arg-max is the true id at index pos[i] + 1 as long as every earlier row was right
        amax = []
        for i in range(len(toks)):
            ok = all(pos[j] < len(full) and toks[j] == full[pos[j]] for j in range(i + 1)) and pos[i] + 1 < len(full)
            amax.append(full[pos[i] + 1] if ok else NONE - 1 - i)
        nb = len(toks)
        rec, h, toks, pos = step(h, toks, amax, rec["left"], D, ngram_min, ngram_max, stop_token, seq_limit)
        if nb > 1:
            stats["steps_verify"] += 1
            stats["drafted"] += D
            stats["accepted"] += rec["accepted"]
        else:
            stats["steps_plain"] += 1
        stats["emitted"] += rec["emitted"]
    return h[n0:], stats
