"""Lookup drafts for several sequences, restated in plain Python on top of lookup_ref.step (DESIGN.md section 10;
nano_amd/csrc/lookup_rows.hip is the device form, nano_hip_lookup_rows_plan the host's planner).

Nothing here imports the native library: the CPU tests check these definitions against each other and the planner of the library
against plan(), the GPU tests check the kernels and the loop against them.

A round: every live sequence has rows in ONE pass -- one row, or a verify chunk of D + 1 rows.  Behind the pass lookup_ref.step runs
for every sequence on its own rows (a sequence never sees another's), and the next pass is packed: the live sequences ordered stably
by the range hint of position n - 1, each sequence's rows contiguous and ascending.
"""
import lookup_ref as lr

NONE = 0xFFFFFFFF          # row_start of a sequence without rows in the pass; unused words of the operator entry's outputs
MAX_ROWS = lr.MAX_ROWS


def hint(n, max_seq_len):
    """The range hint of position n - 1 (nano_hip_rows_plan's row_hint): the end of its 64-position bucket, clipped to max_seq_len."""
    return min(((n - 1 + 64) // 64) * 64, max_seq_len)


def plan(n, nb_next, max_seq_len):
    """The pass of a round.  n[i]: ids in sequence i's history; nb_next[i]: its rows (0: dead).
    Returns (order: the live sequences in pass order, row_start per sequence (NONE: dead), groups: [(hint, rows)] runs of equal hints)."""
    live = [i for i in range(len(n)) if nb_next[i]]
    order = sorted(live, key=lambda i: hint(n[i], max_seq_len))            # (sorted() is stable)
    row_start = [NONE] * len(n)
    groups, row = [], 0
    for i in order:
        h = hint(n[i], max_seq_len)
        row_start[i] = row
        if groups and groups[-1][0] == h:
            groups[-1] = (h, groups[-1][1] + nb_next[i])
        else:
            groups.append((h, nb_next[i]))
        row += nb_next[i]
    return order, row_start, groups


def round_step(histories, left, slots, fed, amax, row_start, nb, D, ngram_min=1, ngram_max=3, stop_token=lr.NO_STOP, seq_limit=1 << 30,
               max_seq_len=1 << 30):
    """What the two launches of lookup_rows.hip do behind a pass that fed `fed` and left the row arg-maxes `amax` (pass order), sequence
    i's rows being row_start[i] .. row_start[i] + nb[i] (nb[i] = 0: it had none).
    Returns (records, new histories, next tokens, next positions, next slots -- the three in pass order --, next row_start)."""
    recs, hs, toks, poss = [], [], [], []
    for i, h in enumerate(histories):
        r0 = row_start[i] if nb[i] else 0
        rec, h2, t, p = lr.step(h, list(fed[r0:r0 + nb[i]]), list(amax[r0:r0 + nb[i]]), left[i], D, ngram_min, ngram_max, stop_token, seq_limit)
        recs.append(rec); hs.append(h2); toks.append(t); poss.append(p)
    order, start, _groups = plan([r["n"] for r in recs], [r["nb_next"] for r in recs], max_seq_len)
    nt, npos, nsl = [], [], []
    for i in order:
        nt += toks[i]; npos += poss[i]; nsl += [slots[i]] * len(toks[i])
    return recs, hs, nt, npos, nsl, start


def simulate_rows(histories, truths, max_new, D, ngram_min=1, ngram_max=3, stop_token=lr.NO_STOP, seq_limit=1 << 30, max_seq_len=1 << 30,
                  max_steps=0):
    """The loop against models that always answer with the truth (lookup_ref.simulate's convention, per sequence).
    Returns (per-sequence emitted ids, per-sequence stats dicts, rounds = passes run)."""
    B = len(histories)
    hs = [list(h) for h in histories]
    n0 = [len(h) for h in hs]
    full = [list(histories[i]) + list(truths[i]) for i in range(B)]
    slots = list(range(B))
    stats = [{"steps_plain": 0, "steps_verify": 0, "drafted": 0, "accepted": 0, "emitted": 0} for _ in range(B)]
    left = list(max_new)
    fin = [False] * B
    recs, hs, toks, pos, sl, start = round_step(hs, left, slots, [], [], [NONE] * B, [0] * B, D, ngram_min, ngram_max, stop_token, seq_limit, max_seq_len)
    nb = [0] * B
    rounds = 0
    while True:
        for i in range(B):
            if fin[i]:
                continue
            if nb[i] > 1:
                stats[i]["steps_verify"] += 1; stats[i]["drafted"] += D; stats[i]["accepted"] += recs[i]["accepted"]
            elif nb[i] == 1:
                stats[i]["steps_plain"] += 1
            stats[i]["emitted"] += recs[i]["emitted"]
            left[i] = recs[i]["left"]
            if recs[i]["done"]:
                fin[i] = True
                left[i] = 0                                                 # (a finished sequence stays finished, whatever was left when it stopped)
        nb = [0 if fin[i] else recs[i]["nb_next"] for i in range(B)]
        if all(fin) or (max_steps and rounds == max_steps):
            break
        rounds += 1
        # row r of the pass belongs to the sequence whose slot it names; its arg-max is the true id behind its position as long as every
        # earlier row of ITS sequence was right
        amax = [0] * len(toks)
        for i in range(B):
            if not nb[i]:
                continue
            r0 = start[i]
            for k in range(nb[i]):
                ok = all(pos[r0 + j] < len(full[i]) and toks[r0 + j] == full[i][pos[r0 + j]] for j in range(k + 1)) and pos[r0 + k] + 1 < len(full[i])
                amax[r0 + k] = full[i][pos[r0 + k] + 1] if ok else NONE - 1 - k
        recs, hs, toks, pos, sl, start = round_step(hs, left, slots, toks, amax, start, nb, D, ngram_min, ngram_max, stop_token, seq_limit, max_seq_len)
    return [hs[i][n0[i]:] for i in range(B)], stats, rounds
