"""Greedy decode with a draft model, restated in plain Python (nano_amd/csrc/draft.hip is the device form, the
loop is nano_amd/csrc/backend_draft.hip's).

Nothing here imports the native library: the CPU tests check these definitions against each other, the GPU tests check the kernel
and the loop against them.

History h[0..n), n >= 1; the target holds positions 0 .. n-2 and is fed h[n-1] first; the draft holds dn <= n-1 leading positions.
A round of D' drafted ids feeds the target [h[n-1], d1 .. dD'] at positions n-1 .. n-1+D'; the draft model made d1 .. dD' by feeding
h[n-1], d1 .. d(D'-1) at positions n-1 .. n-2+D'.
"""
from lookup_ref import NO_STOP, NONE, MAX_ROWS, accepted          # accepted(): the lookup loop's definition, word for word

RECORD_FIELDS = ("emitted", "accepted", "nb_next", "n", "dn", "cursor", "done", "left")


def round_rows(n, left, D, seq_limit):
    """Rows of the round that starts at a history of n ids with `left` ids to emit: 1 + D', D' = min(D, 63 - (n-1) % 64, left - 1,
    seq_limit - n) -- the chunk stays inside one 64-position bucket and its last position n-1+D' below seq_limit.  0: nothing left."""
    if left == 0:
        return 0
    return 1 + max(0, min(D, MAX_ROWS - 1, 63 - (n - 1) % 64, left - 1, seq_limit - n))


def catch_up_rows(n, dn):
    """Rows the draft is fed before it drafts: h[dn .. n-2]."""
    return n - 1 - dn


def history_cap(n, seq_limit):
    """Capacity of the operator entry's device history: the loop's holds max_seq_len + 1 ids, rounded up to 4."""
    return (max(n, min(n + MAX_ROWS, seq_limit + 1)) + 3) & ~3


def step(h, fed, amax, left, D, stop_token, seq_limit, dn, cap=1 << 40, cursor=0):
    """What draft_round_kernel's ACCEPT role does behind a round that fed `fed` and left the row arg-maxes `amax` (both empty: no round
    has run).  Returns (record dict, new history, row 0 of the next round or None, its positions)."""
    h = list(h)
    n_old = len(h)
    nb = len(fed)
    a = emitted = 0
    done = left == 0
    if nb:
        a = accepted(fed, amax)
        for i in range(min(a + 1, left)):
            if len(h) >= cap:
                break
            h.append(amax[i])
            emitted += 1
            if amax[i] == stop_token:
                done = True
                break
        left -= emitted
        if left == 0 or len(h) >= cap:
            done = True
        if nb > 1:
            # the draft's rows are right up to position n_old - 1 + min(a, D' - 1), D' = nb - 1; it never holds the last id's position
            dn = min(n_old + min(a, nb - 2), len(h) - 1)
    n = len(h)
    nb_next = 0 if done else round_rows(n, left, D, seq_limit)
    tok0, pos = None, []
    if not done:
        tok0, pos = h[n - 1], [n - 1 + i for i in range(nb_next)]
    rec = {"emitted": emitted, "accepted": a, "nb_next": nb_next, "n": n, "dn": dn, "cursor": cursor + emitted, "done": int(done), "left": left}
    return rec, h, tok0, pos


def simulate(prompt, want, max_new, D, draft_fn, seq_limit=1 << 30, draft_held=0, stop_token=NO_STOP, max_rounds=0):
    """The loop against a target that always answers with the truth: want[i] is the target's greedy id at index len(prompt) + i whatever
    was drafted.  draft_fn(prefix, k) -> the k ids the draft model continues `prefix` with.  Returns (emitted ids, stats dict)."""
    h = list(prompt)
    n0 = len(h)
    full = list(prompt) + list(want)
    st = {"rounds_plain": 0, "rounds_verify": 0, "drafted": 0, "accepted": 0, "emitted": 0, "draft_rows_fed": 0, "draft_held": draft_held}
    dn = draft_held
    rec, h, tok0, pos = step(h, [], [], max_new, D, stop_token, seq_limit, dn)
    rounds = 0
    while not rec["done"] and not (max_rounds and rounds == max_rounds):
        rounds += 1
        nb = rec["nb_next"]
        toks = [tok0]
        if nb > 1:
            st["draft_rows_fed"] += catch_up_rows(len(h), dn)
            toks += [int(t) for t in draft_fn(list(h), nb - 1)]
            assert len(toks) == nb
        # row i's arg-max is the true id at index pos[i] + 1 as long as every row up to it was fed the true id
        amax = []
        for i in range(nb):
            ok = all(pos[j] < len(full) and toks[j] == full[pos[j]] for j in range(i + 1)) and pos[i] + 1 < len(full)
            amax.append(full[pos[i] + 1] if ok else NONE - 1 - i)
        rec, h, tok0, pos = step(h, toks, amax, rec["left"], D, stop_token, seq_limit, dn)
        dn = rec["dn"]
        if nb > 1:
            st["rounds_verify"] += 1
            st["drafted"] += nb - 1
            st["accepted"] += rec["accepted"]
        else:
            st["rounds_plain"] += 1
        st["emitted"] += rec["emitted"]
    st["draft_held"] = dn
    return h[n0:], st
