"""References, the error bound and the cases of the LoRA side branches (nano_amd/csrc/lora.hip; reference infer/infer.c:792-808, 898-908).

    q += s * B_q (A_q xb),  k += s * B_k (A_k xb),  v += s * B_v (A_v xb),  o1 = s * B_o (A_o xba)
    xb = rmsnorm(x, w) (infer.c:601-614, eps 1e-5),  s = (float)alpha / (float)rank,  A [rank][E],  B [out][rank]

Three statements of it:
  * restate_*  float32, the reference's own order: sequential `matmul` (infer.c:637-651), `scale` (589-593), `accum`;
  * exact_*    float64 with the exact alpha / rank -- what the bound is measured from;
  * emulate_*  float32 in the kernels' order: squares at stride 256, the xor tree over a wave, the four waves' sums added in ascending
               order; per A row a lane's float4 fused multiply-add chain at stride 256 and the xor tree; the B side sequential.
               (A fused multiply-add is the exact float64 product plus the float64 sum rounded to fp32 -- a double rounding in rare
               cases, which an estimate of the error's size does not mind.)  `mutant` breaks one thing in it (MUTANTS).

The bound, per element (u = 2^-24, c = ceil(E / 256), T_j = sum_i |A_ji| |xb_i|, t_j = sum_i A_ji xb_i, both exact):

    |out_i - ref_i| <= u * [ (c_x + c_d) * s * sum_j |B_ij| T_j  +  (rank + 3) * s * sum_j |B_ij| |t_j|  +  |ref_i| ]

  c_x = c + 17   roundings on the way from x to xb: a square (1); the thread's chain of c adds; six levels of the wave tree; four adds
                 over the waves; / E; + eps; sqrt; 1 /; the two multiplies ss * x and w * (.).  The sum is one of positive terms, so
                 the counts add up as a relative error; sqrt halves what reaches it, which is NOT used: that slack of (c + 13) / 2
                 roundings pays for every second-order term below ((c_x + c_d) * (rank + 3) * u^2 and the like, < 1e-4 of the first).
                 lora_o reads xba as it is: c_x = 0.
  c_d = 4c + 6   roundings of a down-projection output on top of xb's: a lane runs 4 fused multiply-adds per trip, c trips at the
                 most (float4 at lane * 4 + 256 k), one rounding each, then six levels of the wave tree.  With |xb^ - xb| <= c_x u |xb|:
                 |t^_j - t_j| <= (c_x + c_d) u T_j.
  rank + 3       the B side: term j of `val += row[j] * t[j]` is rounded by its multiply and by at most rank - 1 adds that follow (the
                 first add, to 0, is exact): rank; `* s`: 1; s = (float)alpha / (float)rank itself: 1; one to spare.  It multiplies
                 |t^_j| <= |t_j| + (c_x + c_d) u T_j, the surplus being second order.
  |ref_i|        the accumulate `q[i] += ...`: one rounding of the result.  lora_o stores: no such term (exact_branch without `old`).
                 Where the delta is small beside the old value (rank 1, alpha / rank = 1/8) this term is the error, and it is attainable:
                 the worst |d| / bound measured is 0.54 on the device and 0.62 in the emulation, both at E 128, rank 1; shapes whose
                 delta is of the old value's size stay below 0.06.
The bound is derived from the kernel's operations; nothing in it is fitted to what the kernel returns.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
EPS = 1e-5

# (E, KD, rank, alpha): what the GPU cases run (tests/test_gpu_lora_ops.py), and what the bound is held against on the CPU
SHAPES = [(128, 64, 4, 8), (128, 128, 1, 16), (192, 96, 3, 16), (260, 130, 5, 16), (260, 96, 8, 1), (512, 256, 8, 16), (512, 512, 64, 16),
          (768, 384, 8, 16), (768, 96, 3, 16), (768, 768, 5, 16)]
# (name, nb, positions, S, v slots, v_bstride in rows: S = decode, 0 = a prefill chunk)
FORMS = [("one", 1, (2,), 4, 2, 4), ("decode3", 3, (0, 5, 8), 9, 4, 9), ("chunk5", 5, (3, 4, 5, 6, 7), 9, 2, 0)]
MUTANTS = ("drop_float4", "v_reads_k", "pos0", "skip_last_rank")
# a mutant of ORDER alone: `val += row[j] * (t[j] * s)`.  It moves roundings without adding error of another size -- rank + 1 more of
# them on sum |B| |t| at the worst -- so no bound derived from rounding can tell it from the kernel; the bit-for-bit cases do.
ORDER_MUTANTS = ("scale_first",)


def inputs(E, KD, rank, nb, seed=0):
    """x, w, the four pairs and the old q / k / v rows of nb sequences: plain random data of the sizes a model has"""
    rng = np.random.default_rng([E, KD, rank, nb, seed])
    g = lambda *s, std=1.0: (std * rng.standard_normal(s)).astype(F)
    I = dict(x=g(nb, E), w=(1 + 0.1 * rng.standard_normal(E)).astype(F))
    for n, rows in (("q", E), ("k", KD), ("v", KD), ("o", E)):
        I[n + "a"], I[n + "b"] = g(rank, E, std=0.05), g(rows, rank, std=0.05)
    I["q"], I["k"], I["v"] = g(nb, E), g(nb, KD), g(nb, KD)
    I["xba"] = g(nb, E)
    return I


# ---- float32, the reference's order ---------------------------------------------------------------
def _matmul32(W, x):
    """infer.c matmul: val = 0; val += w[i][j] * x[j] in ascending j, every operation rounded to fp32"""
    val = np.zeros(W.shape[0], F)
    for j in range(W.shape[1]):
        val = (val + (W[:, j] * x[j]).astype(F)).astype(F)
    return val


def rmsnorm32(x, w):
    ss = F(0)
    for v in x:
        ss = F(ss + F(v * v))
    ss = F(ss / F(len(x))); ss = F(ss + F(EPS)); ss = F(F(1) / np.sqrt(ss, dtype=F))
    return (w * (ss * x).astype(F)).astype(F)


def scale32(alpha, rank):
    return F(F(alpha) / F(rank))


def restate_branch(A, B, act, alpha, rank):
    """s * (B (A act)) as the reference computes it: matmul, matmul, scale"""
    return (_matmul32(B, _matmul32(A, act)) * scale32(alpha, rank)).astype(F)


def restate_qkv(I, b, alpha, rank):
    xb = rmsnorm32(I["x"][b], I["w"])
    return tuple((I[n][b] + restate_branch(I[n + "a"], I[n + "b"], xb, alpha, rank)).astype(F) for n in "qkv")


def restate_o(I, b, alpha, rank):
    return restate_branch(I["oa"], I["ob"], I["xba"][b], alpha, rank)


# ---- float64 and the bound ------------------------------------------------------------------------
def exact_branch(A, B, act64, alpha, rank, old=None, c_x=0):
    """(ref, bound) of one branch in float64; act64 = the exact activation"""
    A, B = A.astype(np.float64), B.astype(np.float64)
    E = A.shape[1]
    c = (E + 255) // 256
    s = alpha / rank
    t, T = A @ act64, np.abs(A) @ np.abs(act64)
    ref = s * (B @ t)
    bound = (c_x + 4 * c + 6) * s * (np.abs(B) @ T) + (rank + 3) * s * (np.abs(B) @ np.abs(t))
    if old is not None:
        ref = old.astype(np.float64) + ref
        bound = bound + np.abs(ref)
    return ref, U * bound


def exact_qkv(I, b, alpha, rank):
    """[(ref, bound)] for q, k, v of sequence b"""
    x = I["x"][b].astype(np.float64)
    E = len(x)
    xb = I["w"].astype(np.float64) * x / np.sqrt((x * x).sum() / E + EPS)
    return [exact_branch(I[n + "a"], I[n + "b"], xb, alpha, rank, I[n][b], c_x=(E + 255) // 256 + 17) for n in "qkv"]


def exact_o(I, b, alpha, rank):
    return exact_branch(I["oa"], I["ob"], I["xba"][b].astype(np.float64), alpha, rank)


# ---- float32, the kernels' order -------------------------------------------------------------------
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _xor_tree(v):
    """wave_sum: v += shfl_xor(v, o) for o = 32 .. 1 over the last axis of 64 lanes; every lane ends with the same sum"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(F)
    return v[..., 0]


def _down(A, act, drop_row=None):
    """lowrank_down: t[j] = the xor tree over the lanes' chains acc = fma(A[j, i], act[i], acc), i = lane * 4 + 256 k + (0 .. 3)"""
    rank, E = A.shape
    c = (E + 255) // 256
    Ap = np.zeros((rank, c * 256), F); Ap[:, :E] = A           # beyond E a lane makes no trip: fma(0, 0, acc) = acc
    if drop_row is not None:
        Ap[drop_row, E - 4:E] = 0                               # mutant: the row's last float4 never loaded
    ap = np.zeros(c * 256, F); ap[:E] = act
    A4, a4 = Ap.reshape(rank, c, 64, 4), ap.reshape(c, 64, 4)
    acc = np.zeros((rank, 64), F)
    for k in range(c):
        for e in range(4):
            acc = _fma(A4[:, k, :, e], np.broadcast_to(a4[k, :, e], (rank, 64)), acc)
    return _xor_tree(acc)


def _up(B, t, s, skip_last=False, scale_first=False):
    """lowrank_up: val += row[j] * t[j] in ascending j, then * s"""
    val = np.zeros(B.shape[0], F)
    for j in range(B.shape[1] - (1 if skip_last else 0)):
        val = (val + (B[:, j] * (F(t[j] * s) if scale_first else t[j])).astype(F)).astype(F)
    return val if scale_first else (val * s).astype(F)


def emulate_norm(x, w):
    E = len(x)
    c = (E + 255) // 256
    xp = np.zeros(c * 256, F); xp[:E] = x
    acc = np.zeros(256, F)
    for k in range(c):                                          # thread tid: i = tid + 256 k
        acc = (acc + (xp[256 * k:256 * k + 256] * xp[256 * k:256 * k + 256]).astype(F)).astype(F)
    red = _xor_tree(acc.reshape(4, 64))
    ss = F(0)
    for r in red:
        ss = F(ss + r)
    ss = F(ss / F(E)); ss = F(ss + F(EPS)); ss = F(F(1) / np.sqrt(ss, dtype=F))
    return (w * (ss * x).astype(F)).astype(F)


def emulate_qkv(I, b, alpha, rank, mutant=None):
    """q, k, v rows of sequence b after lora_qkv_kernel.  mutant "pos0" is one of addressing: emulate_v_rows() applies it."""
    assert mutant is None or mutant in MUTANTS + ORDER_MUTANTS
    xb = emulate_norm(I["x"][b], I["w"])
    s = scale32(alpha, rank)
    t = {n: _down(I[n + "a"], xb, drop_row=rank - 1 if mutant == "drop_float4" and n == "q" else None) for n in "qkv"}
    if mutant == "v_reads_k":
        t["v"] = t["k"]
    return tuple((I[n][b] + _up(I[n + "b"], t[n], s, skip_last=mutant == "skip_last_rank", scale_first=mutant == "scale_first")).astype(F) for n in "qkv")


def emulate_o(I, b, alpha, rank, mutant=None):
    assert mutant is None or mutant in MUTANTS + ORDER_MUTANTS
    t = _down(I["oa"], I["xba"][b], drop_row=rank - 1 if mutant == "drop_float4" else None)
    return _up(I["ob"], t, scale32(alpha, rank), skip_last=mutant == "skip_last_rank", scale_first=mutant == "scale_first")


def v_row_of(form, b, mutant=None):
    """the row of the whole v buffer [slots * S] that sequence b's delta goes to: b * v_bstride + pos[b] (in rows)"""
    _, _, pos, _, _, bstride = form
    return b * bstride + (pos[0] if mutant == "pos0" else pos[b])


# ---- inputs on which the kernels' order and the reference's give the same bits ---------------------------
def _order_free(rng, shape, amp=32):
    """multiples of 2^-4 in [-2, 2] (tests/fused_ref.py order_free): sums of up to 2^14 squares or products of them are exact in any order"""
    return (rng.integers(-amp, amp + 1, size=shape).astype(F) / F(16.0)).astype(F)


def exact_inputs(E, KD, rank, nb, seed=0, zero_x=False, zero_b=False):
    """inputs() with the A side made exact in any order: x and xba order-free (the sum of squares, and A_o xba with an order-free A_o,
    are exact), the q / k / v A rows one-hot powers of two at places and exponents that differ between the three (t_j = 2^e * xb[i]
    whatever the order, and a t vector fed to the wrong output changes it).  Everything after t runs in the reference's order."""
    rng = np.random.default_rng([E, KD, rank, nb, seed, 77])
    I = inputs(E, KD, rank, nb, seed)
    I["x"] = np.zeros((nb, E), F) if zero_x else _order_free(rng, (nb, E))
    I["xba"] = np.zeros((nb, E), F) if zero_x else _order_free(rng, (nb, E))
    I["oa"] = _order_free(rng, (rank, E))
    for k, n in enumerate("qkv"):
        A = np.zeros((rank, E), F)
        A[np.arange(rank), rng.permutation(E)[:rank]] = np.ldexp(F(1), rng.integers(-3, 4, rank) + k - 1).astype(F)
        I[n + "a"] = A
    if zero_b:
        for n in "qkvo":
            I[n + "b"][:] = 0
    return I
