"""Every Q4K GEMV launch plan (gemv_q4k.hip's item kernel gemv_q4k_slab_kernel<ROLE, B, NV, IPT>, gemv_q4k_chunk.hip's
gemv_q4k_chunk_kernel<ROLE, NV, D, LOOP, NB>) against the reference's own arithmetic (the block quantizer infer/tensor.c:144-242,
matmul_q4k tensor.c:438-471, rmsnorm infer/infer.c:601-614, the residual adds 906-908 / 963-965, SwiGLU 937-944), bit for bit -- and the
arg-max partials a one-tensor STORE launch writes for the step's sampler (gemv_q4k.hip, gemv_q4k_chunk_body.inc), which argmax_kernel
(misc.hip) reduces instead of scanning the logits.

The launches go through nb.op_fused_gemv(0x42, ...), i.e. the step's own router (route.hip), which hands a launch the partials buffer
exactly where the step's classifier does (route_partials()); nb.q4k_gemv_plan reports the plan the launchers follow.  There is ONE
case per kernel instantiation the CPU sweep finds reachable (tests/test_q4k_gemv_plan.py UNIVERSE: 55 slab and 90 chunk tuples), named by
its tuple, at the smallest shape the search found for it, plus cases for the axes the tuples do not carry; the closing coverage test reads
the plans (no GPU) and holds both.  Values are checked first (a plan mismatch must not hide a wrong result).

WEIGHTS.  A pool of distinct standard_normal * 0.05 rows per row length is quantized once by the oracle (oracle.quantize_q4k); a case's
tensors gather pool rows with a seeded choice with repetition.  Row k of matmul_q4k depends on row k's blocks and the activation only, so
the reference of a tensor is oracle.matmul_q4k over the pool, gathered the same way (small cases also run the oracle on the gathered
tensor itself and compare).  Repeated rows have bit-equal logits: every launch with partials meets ties, and the cases marked ties=True
plant the row with the sequence's largest logit where a tie is most awkward -- twice in one wave of a workgroup, in its last row, 64 rows on
(another wave of the chunk kernel), in the workgroups before and after, in the last row of the ragged last workgroup.
INPUTS (test_gpu_q80_gemv.py): activations order-free (multiples of 2^-4 in [-2, 2]: the sum of squares of up to 2^14 of them is exact in
any order, so oracle.rmsnorm -- and with it the quantized activation -- is pinned exactly; norm cases beyond 16384 values use [-1, 1]),
old residual standard_normal; combine cases have equal split maxima (every exp() an exact 1) and split sums that add to a power of two.

BARS, none of them new.  Every launch bit for bit the oracle's (oracle.rmsnorm where there is a norm, oracle.quantize_q4k of the
activation, oracle.matmul_q4k per tensor, kind 1: + the old residual in fp32).  SwiGLU: the store form of the same two matrices bit for
bit, the fused form under rtol = 3e-6, atol = 1e-9 (the device's expf against libm: test_k4_norm_swiglu_q4k's bar).
EVERY CASE runs in a guarded buffer -- nb + 8 slots of rows_total + 1 floats filled with a sentinel -- and every element outside
[b < nb, : rows_total] must come back untouched (the dead slots of a capacity-4 / -8 kernel at 3 / 5 / 6 / 7 sequences are where a stray
store would land); in a batch each sequence bit-equals the same launch of that sequence alone.
PARTIALS.  Every case runs with a partials buffer of nb + 2 slots x partials + 4 pairs prefilled with a pair that would win any reduction
(+inf, row 0).  Planned partials > 0: the launch reports that count; pair t of sequence b -- the launch writes them densely, pair
b * ntiles + t -- is bit for bit (max, first row of that max) of out[b, t * rw : (t + 1) * rw]; every pair behind the nb * ntiles written
ones is still the poison; the arg-max kernel's rule over the pairs, the arg-max kernel itself behind the launch and the arg-max kernel
scanning the logits of a launch without partials all give np.argmax(out[b]).  Planned partials == 0 (several tensors, kind 1 or 2, the
chunk form at 2..8 sequences, a sliced batch): the launch reports 0, the buffer comes back untouched, the arg-max kernel scans.

Largest case: chunk-norm-store-b1-nv1-d8-loop, 65573 rows of 1536 (100.7 M weights, 63 MB of blocks): the looping form reaches a third
round only where a wave has more than 16 wave-loads, i.e. rw * n / 256 > 768 blocks per workgroup of a grid sized for 256 CUs."""
import numpy as np
import pytest

from nano_amd import binding as nb
from test_q4k_gemv_plan import UNIVERSE, ROLE, plan_tuple
from fused_ref import bits, order_free, silu_mul, rows_total

Q4K = 0x42
SENTINEL = np.float32(-12345.678)
POISON = np.array([np.inf, 0.0], np.float32)               # (+inf, row 0): wins any reduction that reads it
NO_ROW = 0xffffffff


def case(cid, kind, n, rows, nb_, want, norm=False, comb=None, ties=False, **more):
    """kind 0 store / 1 residual add / 2 SwiGLU (rows: two equal counts); comb = (n_head, head_dim, split sums) for a launch whose prologue
    combines split-attention partials; want = the plan_tuple() of the launch, more = further plan fields; ties: plant tied maxima"""
    target = dict(tuple=want, **more)
    return pytest.param(dict(id=cid, kind=kind, n=n, rows=tuple(rows), nb=nb_, norm=norm, comb=comb, ties=ties, target=target), id=cid)


R = ROLE
SLAB, CHUNK = "slab", "chunk"                              # (the names plan_tuple() uses)
CASES = [
    # ---- one case per tuple of UNIVERSE, named by it: the smallest shape found, ragged row counts (7, 33, 333) where they cost nothing ----
    case("chunk-generic-b1-nv1-d1", 0, 256, (7,), 1, (CHUNK, R["generic"], 1, 1, 1, 0), rw=1, grid=7, partials=7),
    case("chunk-generic-b1-nv1-d2", 0, 256, (4096, 1024, 1024), 1, (CHUNK, R["generic"], 1, 1, 2, 0), rw=25, grid=246, partials=0),
    case("chunk-generic-b1-nv1-d4", 0, 2048, (4096, 1024, 1024), 1, (CHUNK, R["generic"], 1, 1, 4, 0), rw=25, grid=246, partials=0),
    case("chunk-generic-b1-nv1-d8", 0, 4096, (4096, 1024, 1024), 1, (CHUNK, R["generic"], 1, 1, 8, 0), rw=25, grid=246, partials=0),
    case("chunk-generic-b1-nv1-d8-loop", 0, 3072, (16391,), 1, (CHUNK, R["generic"], 1, 1, 8, 1), ties=True, rw=65, grid=253, partials=253,
         rounds=2),
    case("chunk-generic-b1-nv2-d1", 0, 4352, (33,), 1, (CHUNK, R["generic"], 1, 2, 1, 0), rw=1, grid=33, partials=33),
    case("chunk-generic-b1-nv2-d2", 2, 6400, (333, 333), 1, (CHUNK, R["generic"], 1, 2, 2, 0), rw=2, grid=167, partials=0),
    case("chunk-generic-b1-nv2-d4", 0, 5120, (2560,), 1, (CHUNK, R["generic"], 1, 2, 4, 0), rw=10, grid=256, partials=256),
    case("chunk-generic-b1-nv2-d8", 0, 6400, (4096,), 1, (CHUNK, R["generic"], 1, 2, 8, 0), rw=16, grid=256, partials=256),
    case("chunk-generic-b1-nv2-d8-loop", 0, 7936, (4096, 1024, 1024), 1, (CHUNK, R["generic"], 1, 2, 8, 1), rw=25, grid=246, partials=0,
         rounds=2),
    case("chunk-generic-b1-nv4-d1", 0, 8448, (7,), 1, (CHUNK, R["generic"], 1, 4, 1, 0), rw=1, grid=7, partials=7),
    case("chunk-generic-b1-nv4-d2", 2, 12544, (33, 33), 1, (CHUNK, R["generic"], 1, 4, 2, 0), rw=1, grid=33, partials=0),
    case("chunk-generic-b1-nv4-d4", 2, 12544, (333, 333), 1, (CHUNK, R["generic"], 1, 4, 4, 0), rw=2, grid=167, partials=0),
    case("chunk-generic-b1-nv4-d8", 0, 9984, (2560,), 1, (CHUNK, R["generic"], 1, 4, 8, 0), rw=10, grid=256, partials=256),
    case("chunk-generic-b1-nv4-d8-loop", 2, 9984, (2560, 2560), 1, (CHUNK, R["generic"], 1, 4, 8, 1), rw=10, grid=256, partials=0,
         rounds=2),
    case("chunk-generic-b2-nv1-d1", 1, 13824, (7,), 2, (CHUNK, R["generic"], 2, 1, 1, 0), comb=(108, 128, (1, 3, 2, 2)), rw=1, grid=7,
         partials=0),
    case("chunk-generic-b2-nv1-d2", 2, 13312, (33, 33), 2, (CHUNK, R["generic"], 2, 1, 2, 0), rw=1, grid=33, partials=0),
    case("chunk-generic-b2-nv1-d4", 2, 13312, (333, 333), 2, (CHUNK, R["generic"], 2, 1, 4, 0), rw=2, grid=167, partials=0),
    case("chunk-generic-b2-nv1-d8", 0, 4096, (4096, 1024, 1024), 2, (CHUNK, R["generic"], 2, 1, 8, 0), rw=25, grid=246, partials=0),
    case("chunk-generic-b2-nv1-d8-loop", 0, 7936, (4096, 1024, 1024), 2, (CHUNK, R["generic"], 2, 1, 8, 1), rw=25, grid=246, partials=0,
         rounds=2),
    case("chunk-generic-b4-nv1-d1", 1, 6912, (7,), 3, (CHUNK, R["generic"], 4, 1, 1, 0), comb=(54, 128, (1, 3, 2, 2)), rw=1, grid=7,
         partials=0),
    case("chunk-generic-b4-nv1-d2", 2, 12544, (33, 33), 4, (CHUNK, R["generic"], 4, 1, 2, 0), rw=1, grid=33, partials=0, lds_bytes=68336),
    case("chunk-generic-b4-nv1-d4", 2, 12544, (333, 333), 3, (CHUNK, R["generic"], 4, 1, 4, 0), rw=2, grid=167, partials=0,
         lds_bytes=69904),
    case("chunk-generic-b4-nv1-d8", 0, 4096, (4096, 1024, 1024), 3, (CHUNK, R["generic"], 4, 1, 8, 0), rw=25, grid=246, partials=0),
    case("chunk-generic-b4-nv1-d8-loop", 0, 7936, (4096, 1024, 1024), 3, (CHUNK, R["generic"], 4, 1, 8, 1), rw=25, grid=246, partials=0,
         rounds=2),
    case("chunk-generic-b8-nv1-d1", 0, 256, (7,), 5, (CHUNK, R["generic"], 8, 1, 1, 0), rw=1, grid=7, partials=0),
    case("chunk-generic-b8-nv1-d2", 2, 12544, (33, 33), 6, (CHUNK, R["generic"], 8, 1, 2, 0), rw=1, grid=33, partials=0, lds_bytes=136464),
    case("chunk-generic-b8-nv1-d4", 2, 12544, (333, 333), 7, (CHUNK, R["generic"], 8, 1, 4, 0), rw=2, grid=167, partials=0,
         lds_bytes=139600),
    case("chunk-generic-b8-nv1-d8", 0, 4096, (4096, 1024, 1024), 8, (CHUNK, R["generic"], 8, 1, 8, 0), rw=25, grid=246, partials=0,
         lds_bytes=79344),
    case("chunk-generic-b8-nv1-d8-loop", 0, 7936, (4096, 1024, 1024), 5, (CHUNK, R["generic"], 8, 1, 8, 1), rw=25, grid=246, partials=0,
         rounds=2, lds_bytes=121264),
    case("chunk-norm-store-b1-nv1-d1", 0, 256, (7,), 1, (CHUNK, R["norm_store"], 1, 1, 1, 0), norm=True, rw=1, grid=7, partials=7),
    case("chunk-norm-store-b1-nv1-d2", 0, 256, (4096, 1024, 1024), 1, (CHUNK, R["norm_store"], 1, 1, 2, 0), norm=True, rw=25, grid=246,
         partials=0),
    case("chunk-norm-store-b1-nv1-d4", 0, 2048, (4096, 1024, 1024), 1, (CHUNK, R["norm_store"], 1, 1, 4, 0), norm=True, rw=25, grid=246,
         partials=0),
    case("chunk-norm-store-b1-nv1-d8", 0, 4096, (4096, 1024, 1024), 1, (CHUNK, R["norm_store"], 1, 1, 8, 0), norm=True, rw=25, grid=246,
         partials=0),
    case("chunk-norm-store-b1-nv1-d8-loop", 0, 1536, (65573,), 1, (CHUNK, R["norm_store"], 1, 1, 8, 1), norm=True, ties=True, rw=129,
         grid=509, partials=509, rounds=3),
    case("chunk-norm-store-b1-nv2-d1", 0, 4352, (33,), 1, (CHUNK, R["norm_store"], 1, 2, 1, 0), norm=True, rw=1, grid=33, partials=33),
    case("chunk-norm-store-b1-nv2-d2", 0, 5120, (1000, 40, 36), 1, (CHUNK, R["norm_store"], 1, 2, 2, 0), norm=True, rw=5, grid=216,
         partials=0),
    case("chunk-norm-store-b1-nv2-d4", 0, 5120, (2560,), 1, (CHUNK, R["norm_store"], 1, 2, 4, 0), norm=True, rw=10, grid=256, partials=256),
    case("chunk-norm-store-b1-nv2-d8", 0, 6400, (4096,), 1, (CHUNK, R["norm_store"], 1, 2, 8, 0), norm=True, rw=16, grid=256, partials=256),
    case("chunk-norm-store-b1-nv2-d8-loop", 0, 7936, (4096, 1024, 1024), 1, (CHUNK, R["norm_store"], 1, 2, 8, 1), norm=True, rw=25,
         grid=246, partials=0, rounds=2),
    case("chunk-norm-store-b1-nv4-d1", 0, 8448, (7,), 1, (CHUNK, R["norm_store"], 1, 4, 1, 0), norm=True, rw=1, grid=7, partials=7),
    case("chunk-norm-store-b1-nv4-d2", 0, 12544, (333,), 1, (CHUNK, R["norm_store"], 1, 4, 2, 0), norm=True, rw=2, grid=167, partials=167),
    case("chunk-norm-store-b1-nv4-d4", 0, 9984, (1000, 40, 36), 1, (CHUNK, R["norm_store"], 1, 4, 4, 0), norm=True, rw=5, grid=216,
         partials=0),
    case("chunk-norm-store-b1-nv4-d8", 0, 9984, (2560,), 1, (CHUNK, R["norm_store"], 1, 4, 8, 0), norm=True, rw=10, grid=256, partials=256),
    case("chunk-norm-store-b1-nv4-d8-loop", 0, 12544, (4096,), 1, (CHUNK, R["norm_store"], 1, 4, 8, 1), norm=True, rw=16, grid=256,
         partials=256, rounds=2),
    case("chunk-resid-b1-nv1-d1", 1, 256, (7,), 1, (CHUNK, R["resid"], 1, 1, 1, 0), rw=1, grid=7, partials=0),
    case("chunk-resid-b1-nv1-d2", 1, 256, (4096, 1024, 1024), 1, (CHUNK, R["resid"], 1, 1, 2, 0), rw=25, grid=246, partials=0),
    case("chunk-resid-b1-nv1-d4", 1, 2048, (4096, 1024, 1024), 1, (CHUNK, R["resid"], 1, 1, 4, 0), rw=25, grid=246, partials=0),
    case("chunk-resid-b1-nv1-d8", 1, 4096, (4096, 1024, 1024), 1, (CHUNK, R["resid"], 1, 1, 8, 0), rw=25, grid=246, partials=0),
    case("chunk-resid-b1-nv1-d8-loop", 1, 3072, (16391,), 1, (CHUNK, R["resid"], 1, 1, 8, 1), rw=65, grid=253, partials=0, rounds=2),
    case("chunk-resid-b1-nv2-d1", 1, 4352, (33,), 1, (CHUNK, R["resid"], 1, 2, 1, 0), rw=1, grid=33, partials=0),
    case("chunk-resid-b1-nv2-d2", 1, 5120, (1000, 40, 36), 1, (CHUNK, R["resid"], 1, 2, 2, 0), rw=5, grid=216, partials=0),
    case("chunk-resid-b1-nv2-d4", 1, 5120, (2560,), 1, (CHUNK, R["resid"], 1, 2, 4, 0), rw=10, grid=256, partials=0),
    case("chunk-resid-b1-nv2-d8", 1, 6400, (4096,), 1, (CHUNK, R["resid"], 1, 2, 8, 0), rw=16, grid=256, partials=0),
    case("chunk-resid-b1-nv2-d8-loop", 1, 7936, (4096, 1024, 1024), 1, (CHUNK, R["resid"], 1, 2, 8, 1), rw=25, grid=246, partials=0,
         rounds=2),
    case("chunk-resid-b1-nv4-d1", 1, 8448, (7,), 1, (CHUNK, R["resid"], 1, 4, 1, 0), rw=1, grid=7, partials=0),
    case("chunk-resid-b1-nv4-d2", 1, 12544, (333,), 1, (CHUNK, R["resid"], 1, 4, 2, 0), rw=2, grid=167, partials=0),
    case("chunk-resid-b1-nv4-d4", 1, 9984, (1000, 40, 36), 1, (CHUNK, R["resid"], 1, 4, 4, 0), rw=5, grid=216, partials=0),
    case("chunk-resid-b1-nv4-d8", 1, 9984, (2560,), 1, (CHUNK, R["resid"], 1, 4, 8, 0), rw=10, grid=256, partials=0),
    case("chunk-resid-b1-nv4-d8-loop", 1, 12544, (4096,), 1, (CHUNK, R["resid"], 1, 4, 8, 1), rw=16, grid=256, partials=0, rounds=2),
    case("chunk-resid-combine-b1-nv1-d1", 1, 256, (7,), 1, (CHUNK, R["resid_combine"], 1, 1, 1, 0), comb=(2, 128, (1, 3, 2, 2)), rw=1,
         grid=7, partials=0),
    case("chunk-resid-combine-b1-nv1-d2", 1, 768, (2560,), 1, (CHUNK, R["resid_combine"], 1, 1, 2, 0), comb=(6, 128, (1, 3, 2, 2)), rw=10,
         grid=256, partials=0),
    case("chunk-resid-combine-b1-nv1-d4", 1, 768, (16391,), 1, (CHUNK, R["resid_combine"], 1, 1, 4, 0), comb=(6, 128, (1, 3, 2, 2)), rw=65,
         grid=253, partials=0),
    case("chunk-resid-combine-b1-nv1-d8", 1, 1536, (16391,), 1, (CHUNK, R["resid_combine"], 1, 1, 8, 0), comb=(12, 128, (1, 3, 2, 2)),
         rw=65, grid=253, partials=0),
    case("chunk-resid-combine-b1-nv1-d8-loop", 1, 3072, (16391,), 1, (CHUNK, R["resid_combine"], 1, 1, 8, 1), comb=(24, 128, (1, 3, 2, 2)),
         rw=65, grid=253, partials=0, rounds=2),
    case("chunk-resid-combine-b1-nv2-d1", 1, 4352, (33,), 1, (CHUNK, R["resid_combine"], 1, 2, 1, 0), comb=(34, 128, (1, 3, 2, 2)), rw=1,
         grid=33, partials=0),
    case("chunk-resid-combine-b1-nv2-d2", 1, 6400, (1024,), 1, (CHUNK, R["resid_combine"], 1, 2, 2, 0), comb=(50, 128, (1, 3, 2, 2)), rw=4,
         grid=256, partials=0),
    case("chunk-resid-combine-b1-nv2-d4", 1, 5120, (2560,), 1, (CHUNK, R["resid_combine"], 1, 2, 4, 0), comb=(40, 128, (1, 3, 2, 2)),
         rw=10, grid=256, partials=0),
    case("chunk-resid-combine-b1-nv2-d8", 1, 6400, (4096,), 1, (CHUNK, R["resid_combine"], 1, 2, 8, 0), comb=(50, 128, (1, 3, 2, 2)),
         rw=16, grid=256, partials=0),
    case("chunk-resid-combine-b1-nv2-d8-loop", 1, 5376, (9728,), 1, (CHUNK, R["resid_combine"], 1, 2, 8, 1), comb=(42, 128, (1, 3, 2, 2)),
         rw=38, grid=256, partials=0, rounds=2),
    case("chunk-resid-combine-b1-nv4-d1", 1, 8448, (7,), 1, (CHUNK, R["resid_combine"], 1, 4, 1, 0), comb=(66, 128, (1, 3, 2, 2)), rw=1,
         grid=7, partials=0),
    case("chunk-resid-combine-b1-nv4-d2", 1, 12544, (333,), 1, (CHUNK, R["resid_combine"], 1, 4, 2, 0), comb=(98, 128, (1, 3, 2, 2)), rw=2,
         grid=167, partials=0),
    case("chunk-resid-combine-b1-nv4-d4", 1, 12544, (1024,), 1, (CHUNK, R["resid_combine"], 1, 4, 4, 0), comb=(98, 128, (1, 3, 2, 2)),
         rw=4, grid=256, partials=0),
    case("chunk-resid-combine-b1-nv4-d8", 1, 9984, (2560,), 1, (CHUNK, R["resid_combine"], 1, 4, 8, 0), comb=(78, 128, (1, 3, 2, 2)),
         rw=10, grid=256, partials=0),
    case("chunk-resid-combine-b1-nv4-d8-loop", 1, 12544, (4096,), 1, (CHUNK, R["resid_combine"], 1, 4, 8, 1), comb=(98, 128, (1, 3, 2, 2)),
         rw=16, grid=256, partials=0, rounds=2),
    case("chunk-norm-swiglu-b1-nv1-d1", 2, 256, (7, 7), 1, (CHUNK, R["norm_swiglu"], 1, 1, 1, 0), norm=True, rw=1, grid=7, partials=0),
    case("chunk-norm-swiglu-b1-nv1-d2", 2, 1280, (768, 768), 1, (CHUNK, R["norm_swiglu"], 1, 1, 2, 0), norm=True, rw=3, grid=256,
         partials=0),
    case("chunk-norm-swiglu-b1-nv1-d4", 2, 2560, (2560, 2560), 1, (CHUNK, R["norm_swiglu"], 1, 1, 4, 0), norm=True, rw=10, grid=256,
         partials=0),
    case("chunk-norm-swiglu-b1-nv1-d8", 2, 768, (16391, 16391), 1, (CHUNK, R["norm_swiglu"], 1, 1, 8, 0), norm=True, rw=65, grid=253,
         partials=0),
    case("chunk-norm-swiglu-b1-nv1-d8-loop", 2, 1536, (16391, 16391), 1, (CHUNK, R["norm_swiglu"], 1, 1, 8, 1), norm=True, rw=65, grid=253,
         partials=0, rounds=2),
    case("chunk-norm-swiglu-b1-nv2-d1", 2, 4352, (33, 33), 1, (CHUNK, R["norm_swiglu"], 1, 2, 1, 0), norm=True, rw=1, grid=33, partials=0),
    case("chunk-norm-swiglu-b1-nv2-d2", 2, 6400, (333, 333), 1, (CHUNK, R["norm_swiglu"], 1, 2, 2, 0), norm=True, rw=2, grid=167,
         partials=0),
    case("chunk-norm-swiglu-b1-nv2-d4", 2, 6400, (1024, 1024), 1, (CHUNK, R["norm_swiglu"], 1, 2, 4, 0), norm=True, rw=4, grid=256,
         partials=0),
    case("chunk-norm-swiglu-b1-nv2-d8", 2, 5120, (2560, 2560), 1, (CHUNK, R["norm_swiglu"], 1, 2, 8, 0), norm=True, rw=10, grid=256,
         partials=0),
    case("chunk-norm-swiglu-b1-nv2-d8-loop", 2, 6400, (4096, 4096), 1, (CHUNK, R["norm_swiglu"], 1, 2, 8, 1), norm=True, rw=16, grid=256,
         partials=0, rounds=2),
    case("chunk-norm-swiglu-b1-nv4-d1", 2, 8448, (7, 7), 1, (CHUNK, R["norm_swiglu"], 1, 4, 1, 0), norm=True, rw=1, grid=7, partials=0),
    case("chunk-norm-swiglu-b1-nv4-d2", 2, 12544, (33, 33), 1, (CHUNK, R["norm_swiglu"], 1, 4, 2, 0), norm=True, rw=1, grid=33, partials=0),
    case("chunk-norm-swiglu-b1-nv4-d4", 2, 12544, (333, 333), 1, (CHUNK, R["norm_swiglu"], 1, 4, 4, 0), norm=True, rw=2, grid=167,
         partials=0),
    case("chunk-norm-swiglu-b1-nv4-d8", 2, 12544, (1024, 1024), 1, (CHUNK, R["norm_swiglu"], 1, 4, 8, 0), norm=True, rw=4, grid=256,
         partials=0),
    case("chunk-norm-swiglu-b1-nv4-d8-loop", 2, 9984, (2560, 2560), 1, (CHUNK, R["norm_swiglu"], 1, 4, 8, 1), norm=True, rw=10, grid=256,
         partials=0, rounds=2),
    case("slab-generic-b1-nv0-ipt4", 0, 16388, (7,), 1, (SLAB, R["generic"], 1, 0, 4), rw=4, grid=2, partials=2, lds_bytes=94816),
    case("slab-generic-b1-nv1-ipt1", 0, 4, (33,), 1, (SLAB, R["generic"], 1, 1, 1), rw=4, grid=9, partials=9),
    case("slab-generic-b1-nv1-ipt2", 2, 4, (9728, 9728), 1, (SLAB, R["generic"], 1, 1, 2), rw=64, grid=152, partials=0),
    case("slab-generic-b1-nv1-ipt4", 0, 2052, (4096,), 1, (SLAB, R["generic"], 1, 1, 4), rw=32, grid=128, partials=128),
    case("slab-generic-b1-nv2-ipt1", 0, 4100, (333,), 1, (SLAB, R["generic"], 1, 2, 1), rw=4, grid=84, partials=84),
    case("slab-generic-b1-nv2-ipt2", 2, 4100, (7, 7), 1, (SLAB, R["generic"], 1, 2, 2), rw=4, grid=2, partials=0),
    case("slab-generic-b1-nv2-ipt4", 0, 4100, (2048,), 1, (SLAB, R["generic"], 1, 2, 4), rw=16, grid=128, partials=128),
    case("slab-generic-b1-nv4-ipt2", 0, 8196, (33,), 1, (SLAB, R["generic"], 1, 4, 2), rw=4, grid=9, partials=9),
    case("slab-generic-b1-nv4-ipt4", 2, 8196, (7, 7), 1, (SLAB, R["generic"], 1, 4, 4), rw=4, grid=2, partials=0),
    case("slab-generic-b2-nv1-ipt1", 0, 4, (333,), 2, (SLAB, R["generic"], 2, 1, 1), rw=4, grid=84, partials=84),
    case("slab-generic-b2-nv1-ipt2", 2, 4, (9728, 9728), 2, (SLAB, R["generic"], 2, 1, 2), rw=64, grid=152, partials=0),
    case("slab-generic-b2-nv1-ipt4", 0, 2052, (4096,), 2, (SLAB, R["generic"], 2, 1, 4), rw=32, grid=128, partials=128),
    case("slab-generic-b2-nv2-ipt1", 0, 4100, (7,), 2, (SLAB, R["generic"], 2, 2, 1), rw=4, grid=2, partials=2),
    case("slab-generic-b2-nv2-ipt2", 2, 4100, (33, 33), 2, (SLAB, R["generic"], 2, 2, 2), rw=4, grid=9, partials=0),
    case("slab-generic-b2-nv2-ipt4", 0, 4100, (2048,), 2, (SLAB, R["generic"], 2, 2, 4), rw=16, grid=128, partials=128),
    case("slab-generic-b2-nv4-ipt2", 0, 8196, (7,), 2, (SLAB, R["generic"], 2, 4, 2), rw=4, grid=2, partials=2, lds_bytes=95408),
    case("slab-generic-b2-nv4-ipt4", 2, 8196, (7, 7), 2, (SLAB, R["generic"], 2, 4, 4), rw=4, grid=2, partials=0, lds_bytes=103984),
    case("slab-generic-b4-nv1-ipt1", 0, 4, (333,), 4, (SLAB, R["generic"], 4, 1, 1), rw=4, grid=84, partials=84),
    case("slab-generic-b4-nv1-ipt2", 2, 4, (9728, 9728), 3, (SLAB, R["generic"], 4, 1, 2), rw=64, grid=152, partials=0),
    case("slab-generic-b4-nv1-ipt4", 0, 2052, (4096,), 3, (SLAB, R["generic"], 4, 1, 4), rw=32, grid=128, partials=128, lds_bytes=83536),
    case("slab-generic-b4-nv2-ipt1", 0, 4100, (7,), 3, (SLAB, R["generic"], 4, 2, 1), rw=4, grid=2, partials=2, lds_bytes=96592),
    case("slab-generic-b4-nv2-ipt2", 2, 4100, (33, 33), 4, (SLAB, R["generic"], 4, 2, 2), rw=4, grid=9, partials=0, lds_bytes=105552),
    case("slab-generic-b4-nv2-ipt4", 0, 4100, (2048,), 3, (SLAB, R["generic"], 4, 2, 4), rw=16, grid=128, partials=128, lds_bytes=123472),
    case("slab-generic-b8-nv1-ipt1", 0, 4, (333,), 6, (SLAB, R["generic"], 8, 1, 1), rw=4, grid=84, partials=84),
    case("slab-generic-b8-nv1-ipt2", 2, 4, (9728, 9728), 7, (SLAB, R["generic"], 8, 1, 2), rw=64, grid=152, partials=0),
    case("slab-generic-b8-nv1-ipt4", 0, 516, (16384,), 8, (SLAB, R["generic"], 8, 1, 4), rw=64, grid=256, partials=256, lds_bytes=82064),
    case("slab-norm-store-b1-nv0-ipt4", 0, 16388, (7,), 1, (SLAB, R["norm_store"], 1, 0, 4), norm=True, rw=4, grid=2, partials=2,
         lds_bytes=94816),
    case("slab-norm-store-b1-nv1-ipt1", 0, 4, (33,), 1, (SLAB, R["norm_store"], 1, 1, 1), norm=True, rw=4, grid=9, partials=9),
    case("slab-norm-store-b1-nv1-ipt2", 0, 260, (16391,), 1, (SLAB, R["norm_store"], 1, 1, 2), norm=True, ties=True, rw=64, grid=257,
         partials=257),
    case("slab-norm-store-b1-nv1-ipt4", 0, 2052, (4096,), 1, (SLAB, R["norm_store"], 1, 1, 4), norm=True, rw=32, grid=128, partials=128),
    case("slab-norm-store-b1-nv2-ipt1", 0, 4100, (333,), 1, (SLAB, R["norm_store"], 1, 2, 1), norm=True, rw=4, grid=84, partials=84),
    case("slab-norm-store-b1-nv2-ipt4", 0, 4100, (2048,), 1, (SLAB, R["norm_store"], 1, 2, 4), norm=True, rw=16, grid=128, partials=128),
    case("slab-norm-store-b1-nv4-ipt2", 0, 8196, (7,), 1, (SLAB, R["norm_store"], 1, 4, 2), norm=True, rw=4, grid=2, partials=2),
    case("slab-norm-store-b1-nv4-ipt4", 0, 8196, (1024,), 1, (SLAB, R["norm_store"], 1, 4, 4), norm=True, rw=8, grid=128, partials=128),
    case("slab-resid-b1-nv0-ipt4", 1, 16388, (33,), 1, (SLAB, R["resid"], 1, 0, 4), rw=4, grid=9, partials=0, lds_bytes=94816),
    case("slab-resid-b1-nv1-ipt1", 1, 4, (333,), 1, (SLAB, R["resid"], 1, 1, 1), rw=4, grid=84, partials=0),
    case("slab-resid-b1-nv1-ipt2", 1, 260, (16384,), 1, (SLAB, R["resid"], 1, 1, 2), rw=64, grid=256, partials=0),
    case("slab-resid-b1-nv1-ipt4", 1, 2052, (4096,), 1, (SLAB, R["resid"], 1, 1, 4), rw=32, grid=128, partials=0),
    case("slab-resid-b1-nv2-ipt1", 1, 4100, (7,), 1, (SLAB, R["resid"], 1, 2, 1), rw=4, grid=2, partials=0),
    case("slab-resid-b1-nv2-ipt4", 1, 4100, (2048,), 1, (SLAB, R["resid"], 1, 2, 4), rw=16, grid=128, partials=0),
    case("slab-resid-b1-nv4-ipt2", 1, 8196, (33,), 1, (SLAB, R["resid"], 1, 4, 2), rw=4, grid=9, partials=0),
    case("slab-resid-b1-nv4-ipt4", 1, 8196, (1024,), 1, (SLAB, R["resid"], 1, 4, 4), rw=8, grid=128, partials=0),
    case("slab-resid-combine-b1-nv0-ipt4", 1, 16640, (7,), 1, (SLAB, R["resid_combine"], 1, 0, 4), comb=(130, 128, (1, 3, 2, 2)), rw=4,
         grid=2, partials=0, lds_bytes=99984),
    case("slab-resid-combine-b1-nv1-ipt1", 1, 4, (333,), 1, (SLAB, R["resid_combine"], 1, 1, 1), comb=(1, 4, (1, 3, 2, 2)), rw=4, grid=84,
         partials=0),
    case("slab-resid-combine-b1-nv1-ipt2", 1, 260, (16384,), 1, (SLAB, R["resid_combine"], 1, 1, 2), comb=(65, 4, (1, 3, 2, 2)), rw=64,
         grid=256, partials=0),
    case("slab-resid-combine-b1-nv1-ipt4", 1, 2052, (4096,), 1, (SLAB, R["resid_combine"], 1, 1, 4), comb=(513, 4, (1, 3, 2, 2)), rw=32,
         grid=128, partials=0),
    case("slab-resid-combine-b1-nv2-ipt1", 1, 4100, (7,), 1, (SLAB, R["resid_combine"], 1, 2, 1), comb=(1025, 4, (1, 3, 2, 2)), rw=4,
         grid=2, partials=0),
    case("slab-resid-combine-b1-nv2-ipt4", 1, 4100, (2048,), 1, (SLAB, R["resid_combine"], 1, 2, 4), comb=(1025, 4, (1, 3, 2, 2)), rw=16,
         grid=128, partials=0),
    case("slab-resid-combine-b1-nv4-ipt2", 1, 8196, (33,), 1, (SLAB, R["resid_combine"], 1, 4, 2), comb=(2049, 4, (1, 3, 2, 2)), rw=4,
         grid=9, partials=0, lds_bytes=113280),
    case("slab-resid-combine-b1-nv4-ipt4", 1, 8196, (1024,), 1, (SLAB, R["resid_combine"], 1, 4, 4), comb=(2049, 4, (1, 3, 2, 2)), rw=8,
         grid=128, partials=0, lds_bytes=117568),
    case("slab-norm-swiglu-b1-nv1-ipt1", 2, 260, (333, 333), 1, (SLAB, R["norm_swiglu"], 1, 1, 1), norm=True, rw=4, grid=84, partials=0),
    case("slab-norm-swiglu-b1-nv1-ipt2", 2, 4, (9728, 9728), 1, (SLAB, R["norm_swiglu"], 1, 1, 2), norm=True, rw=64, grid=152, partials=0),
    case("slab-norm-swiglu-b1-nv1-ipt4", 2, 260, (16384, 16384), 1, (SLAB, R["norm_swiglu"], 1, 1, 4), norm=True, rw=64, grid=256,
         partials=0),
    case("slab-norm-swiglu-b1-nv2-ipt4", 2, 4100, (2048, 2048), 1, (SLAB, R["norm_swiglu"], 1, 2, 4), norm=True, rw=8, grid=256,
         partials=0),
    case("slab-norm-swiglu-b1-nv4-ipt4", 2, 8452, (8, 8), 1, (SLAB, R["norm_swiglu"], 1, 4, 4), norm=True, rw=4, grid=2, partials=0),
    # ---- the axes the tuples do not carry ------------------------------------------------------------------------------------------------
    case("slab-three-tensors", 0, 192, (36, 4, 12), 1, (SLAB, R["norm_store"], 1, 1, 1), norm=True, rw=4, grid=13, partials=0),
    case("slab-three-tensors-b8-5", 0, 192, (36, 4, 12), 5, (SLAB, R["generic"], 8, 1, 1), norm=True, rw=4, grid=13, partials=0),
    case("slab-cut-5-in-2-2-1", 1, 9732, (64,), 5, (SLAB, R["generic"], 2, 4, 2), rw=4, grid=16, partials=0, lds_bytes=113072, launches=3,
         seqs_per_launch=2),
    case("slab-cut-7-in-4-3", 0, 4100, (64, 32, 32), 7, (SLAB, R["generic"], 4, 2, 1), norm=True, rw=4, grid=32, partials=0, lds_bytes=96592,
         launches=2, seqs_per_launch=4),
    case("slab-combine-b4-3", 1, 516, (33,), 3, (SLAB, R["generic"], 4, 1, 1), comb=(129, 4, (1, 3, 2, 2)), rw=4, grid=9, partials=0),
    case("slab-combine-b8-6", 1, 192, (33,), 6, (SLAB, R["generic"], 8, 1, 1), comb=(4, 48, (1, 3, 2, 2)), rw=4, grid=9, partials=0),
    case("slab-swiglu-demoted", 2, 4100, (8, 8), 1, (SLAB, R["generic"], 1, 2, 2), norm=True, rw=4, grid=2, partials=0),
    case("slab-ties-b1-rw32-ragged", 0, 260, (4100,), 1, (SLAB, R["norm_store"], 1, 1, 1), norm=True, ties=True, rw=32, grid=129, partials=129),
    case("slab-ties-b4-3-rw32-ragged", 0, 192, (4100,), 3, (SLAB, R["generic"], 4, 1, 1), ties=True, rw=32, grid=129, partials=129),
    case("slab-partials-b8-5-rw64-ragged", 0, 516, (16391,), 5, (SLAB, R["generic"], 8, 1, 4), rw=64, grid=257, partials=257, lds_bytes=82064),
]


def query(c, **kw):
    attn = (c["comb"][0], c["comb"][1], len(c["comb"][2])) if c["comb"] else None
    return nb.q4k_gemv_plan(c["kind"], c["n"], c["rows"], c["nb"], norm=c["norm"], attn=attn, **kw)


_POOLS = {}


def pool(oracle, n):
    """(framed tensor [P, n], its blocks [P, bytes per row]) of P distinct rows, quantized once per row length"""
    if n not in _POOLS:
        P = int(min(2048, max(64, (2 << 20) // n)))
        w = (np.random.default_rng(n).standard_normal((P, n)) * 0.05).astype(np.float32)
        T = oracle.quantize_q4k(w, [P, n])
        _POOLS[n] = (T, T[44:].reshape(P, -1))
    return _POOLS[n]


def plant_ties(c, q, idx, pool_ref):
    """the pool row with sequence b's largest logit, planted around workgroup grid / 2 + b of the launch and at the end of the matrix"""
    rows, rw, grid = c["rows"][0], q["rw"], q["grid"]
    assert q["partials"] == grid and grid >= 8 + c["nb"] and rw >= 4 and rows % rw, (c["id"], "a tie case needs partials, workgroups around and a ragged last one")
    for b in range(c["nb"]):
        p = int(np.argmax(pool_ref[b]))
        base = (grid // 2 + b) * rw
        spots = [base + 1, base + 2, base + rw - 1, base - 1, base + rw, rows - 1 - b]      # one wave, the last row, the workgroups around, the ragged end
        if rw > 64:
            spots += [base + 64, base + 65]                                                   # another wave of the chunk kernel's workgroup
        assert rows - 1 - b >= (grid - 1) * rw
        idx[spots] = p


def build(oracle, c, q):
    """the inputs of a case and the reference's result per sequence (the residual not yet added)"""
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(c["id"])))
    n, nb_ = c["n"], c["nb"]
    amp = 32 if (not c["norm"] or n <= 16384) else 16
    assert not c["norm"] or n * (amp * amp) <= 1 << 24, "the sum of squares (in units of 2^-8) is no longer exact in any order"
    T, blocks = pool(oracle, n)
    P = blocks.shape[0]
    idx = [rng.integers(0, P, size=r) for r in c["rows"]]
    nw = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32) if c["norm"] else None
    x, attn = order_free(rng, (nb_, n), amp), None
    if c["comb"]:
        n_head, hd, ls = c["comb"]
        L = sum(ls)
        assert L & (L - 1) == 0 and n_head * hd == n
        part = order_free(rng, (nb_, len(ls), n))
        ml = np.zeros((nb_, n_head, len(ls), 2), np.float32)
        ml[..., 0] = 0.25
        ml[..., 1] = np.asarray(ls, np.float32)
        x = (part.astype(np.float64).sum(axis=1) / L).astype(np.float32)            # every split's weight is exp(0) / L
        assert np.array_equal(x.astype(np.float64), part.astype(np.float64).sum(axis=1) / L)
        attn = (part, ml, n_head, hd)
    old = rng.standard_normal((nb_, rows_total(c["kind"], c["rows"]))).astype(np.float32) if c["kind"] == 1 else None
    XT = [oracle.quantize_q4k(oracle.rmsnorm(x[b], nw) if c["norm"] else x[b], [n]) for b in range(nb_)]
    pool_ref = [oracle.matmul_q4k(XT[b], T, 0, P) for b in range(nb_)]
    if c["ties"]:
        plant_ties(c, q, idx[0], pool_ref)
    W = [(np.ascontiguousarray(blocks[i]), None, int(i.size)) for i in idx]
    ref = [np.concatenate([pool_ref[b][i] for i in idx]) for b in range(nb_)]
    if sum(c["rows"]) * n <= 1 << 20:                                                # the shortcut against the oracle on the gathered tensors themselves
        for (w, _, r), i in zip(W, idx):
            G = oracle.quantize_q4k(np.zeros((r, n), np.float32), [r, n])
            G[44:] = w.reshape(-1)
            for b in range(nb_):
                assert np.array_equal(bits(oracle.matmul_q4k(XT[b], G, 0, r)), bits(pool_ref[b][i])), (c["id"], "gathered rows are not the pool's")
    return dict(W=W, nw=nw, x=x, attn=attn, old=old, ref=ref)


def launch(c, I, *, kind=None, W=None, sl=None, partials=None, want_argmax=False):
    """the case's launch in a guarded buffer -- or with sl = b the same launch of sequence b alone --: (out, route, ntiles, argmax)"""
    kind = c["kind"] if kind is None else kind
    W = I["W"] if W is None else W
    rt = W[0][2] if kind == 2 else sum(r for _, _, r in W)
    b0, nb_ = (0, c["nb"]) if sl is None else (sl, 1)
    s = slice(b0, b0 + nb_)
    attn = (I["attn"][0][s], I["attn"][1][s], I["attn"][2], I["attn"][3]) if I["attn"] else None
    g = np.full((nb_ + 8, rt + 1), SENTINEL, np.float32)
    if kind == 1:
        g[:nb_, :rt] = I["old"][s]
    res = nb.op_fused_gemv(Q4K, kind, c["n"], W, None if attn else I["x"][s], I["nw"], nb=nb_, attn=attn, guard=g, want_route=True,
                           partials=partials, want_argmax=want_argmax)
    assert np.all(bits(g[:, rt]) == bits(SENTINEL)), (c["id"], "a guard element behind a sequence's rows changed")
    assert np.all(bits(g[nb_:]) == bits(SENTINEL)), (c["id"], "slots beyond the batch were written",
                                                      (np.flatnonzero((bits(g[nb_:]) != bits(SENTINEL)).any(axis=1)) + nb_).tolist())
    return (g[:nb_, :rt], res[1], res[2] if partials is not None else None, res[-1] if want_argmax else None)


def reduce_pairs(pairs):
    """argmax_kernel's rule over (value, row bits) pairs: no-row pairs skipped, the larger value, on equal values the lower row"""
    best, bi = None, NO_ROW
    for v, i in zip(pairs[:, 0].tolist(), pairs[:, 1].view(np.uint32).tolist()):
        if i != NO_ROW and (bi == NO_ROW or v > best or (v == best and i < bi)):
            best, bi = v, i
    return 0 if bi == NO_ROW else bi


def check_partials(c, q, out, buf, ntiles, amax):
    """check 4 of the module docstring for a launch that planned partials: the pairs, the untouched rest, the reductions"""
    nb_, rows, rw, grid = c["nb"], c["rows"][0], q["rw"], q["grid"]
    assert ntiles == q["partials"] == grid, (c["id"], ntiles, q)
    flat = buf.reshape(-1, 2)
    inside, rest = flat[:nb_ * ntiles].reshape(nb_, ntiles, 2), flat[nb_ * ntiles:]
    stale = np.argwhere((bits(inside) == bits(POISON)).all(axis=2))
    assert stale.size == 0, (c["id"], "pairs the arg-max kernel reads were not written: (sequence, workgroup)", stale[:6].tolist())
    touched = np.flatnonzero((bits(rest) != bits(POISON)).any(axis=1)) + nb_ * ntiles
    assert touched.size == 0, (c["id"], "pairs beyond the launch's nb * ntiles were written", touched[:6].tolist())
    for b in range(nb_):
        tiles = np.full(grid * rw, -np.inf, np.float32)
        tiles[:rows] = out[b]
        tiles = tiles.reshape(grid, rw)
        first = tiles.argmax(axis=1)                                              # the first maximum of each workgroup's rows
        want_v, want_i = tiles[np.arange(grid), first], (np.arange(grid) * rw + first).astype(np.uint32)
        bad = np.flatnonzero((bits(inside[b, :, 0]) != bits(want_v)) | (inside[b, :, 1].view(np.uint32) != want_i))
        assert bad.size == 0, (c["id"], "sequence", b, "workgroups", bad[:6].tolist(), "pairs", inside[b, bad[:3], 0].tolist(),
                               inside[b, bad[:3], 1].view(np.uint32).tolist(), "want", want_v[bad[:3]].tolist(), want_i[bad[:3]].tolist())
        assert reduce_pairs(inside[b]) == int(np.argmax(out[b])), (c["id"], "sequence", b, "the pairs do not reduce to the first maximum")
    assert amax.tolist() == [int(np.argmax(out[b])) for b in range(nb_)], (c["id"], "arg-max from the partials", amax.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES)
def test_q4k_gemv_plan_case(oracle, c):
    q = query(c)
    assert q["takes"] == 1 and nb.ROUTE_NAMES[q["route"]] == "q4k", (c["id"], "the router sends this shape elsewhere or refuses it", q)
    I = build(oracle, c, q)
    kind, nb_, rt = c["kind"], c["nb"], rows_total(c["kind"], c["rows"])
    errors = []

    def held(out, what, b, want):
        bad = np.flatnonzero(bits(out) != bits(want))
        if bad.size:
            errors.append(f"{what} sequence {b}: {bad.size} of {want.size} rows differ, first rows {bad[:6].tolist()}, worst |d| {float(np.abs(out - want).max()):.3e}")

    # 1. values (every launch also asserts its guard elements); the case's own launch carries the partials buffer and the arg-max kernel
    buf = np.empty((nb_ + 2, q["partials"] + 4, 2), np.float32)
    buf[:] = POISON
    fused, route, ntiles, amax = launch(c, I, partials=buf, want_argmax=True)
    assert route == "q4k", (c["id"], route)
    if kind == 2:
        # the store form of the same two matrices pins the projections (one launch where the router takes the two tensors, else one each)
        if nb.q4k_gemv_plan(0, c["n"], c["rows"], nb_, norm=c["norm"])["takes"]:
            both = launch(c, I, kind=0)[0]
        else:
            both = np.concatenate([launch(c, I, kind=0, W=[w])[0] for w in I["W"]], axis=1)
        for b in range(nb_):
            held(both[b], "store form", b, I["ref"][b])
            want = silu_mul(I["ref"][b][:rt], I["ref"][b][rt:])
            if not np.allclose(fused[b], want, rtol=3e-6, atol=1e-9):
                errors.append(f"SwiGLU sequence {b}: off by {float(np.abs(fused[b] - want).max()):.3e}")
    else:
        for b in range(nb_):
            held(fused[b], "result", b, (I["old"][b] + I["ref"][b]).astype(np.float32) if kind == 1 else I["ref"][b])
    assert not errors, f"{c['id']} (plan {q}): " + "; ".join(errors[:4])
    # 2. a batch is its sequences alone
    if nb_ > 1:
        for b in range(nb_):
            alone = launch(c, I, sl=b)[0][0]
            assert np.array_equal(bits(fused[b]), bits(alone)), (c["id"], "sequence", b, "differs from its launch alone", float(np.abs(fused[b] - alone).max()))
    # 3. the arg-max partials, or their absence
    first = [int(np.argmax(fused[b])) for b in range(nb_)]
    if q["partials"]:
        assert kind == 0 and len(c["rows"]) == 1 and q["launches"] == 1, (c["id"], "partials planned where the step's classifier asks for none", q)
        check_partials(c, q, fused, buf, ntiles, amax)
        scan, _, _, amax_scan = launch(c, I, want_argmax=True)                     # no partials buffer: the arg-max kernel scans the logits
        assert np.array_equal(bits(scan), bits(fused)), (c["id"], "the launch without partials differs")
        assert amax_scan.tolist() == first, (c["id"], "arg-max by scanning", amax_scan.tolist(), first)
    else:
        assert ntiles == 0, (c["id"], "partials written where none are planned", ntiles)
        assert np.all(bits(buf) == bits(POISON)), (c["id"], "the partials buffer was written by a launch that plans none")
        assert amax.tolist() == first, (c["id"], "arg-max by scanning", amax.tolist(), first)
    # 4. the plan, last
    got = {k: (plan_tuple(q) if k == "tuple" else q[k]) for k in c["target"]}
    assert got == c["target"], f"{c['id']}: the launcher's plan is {q}, the case means {c['target']}: a retune moved this case -- pick a new shape for this target"


@pytest.mark.gpu
def test_partials_buffer_smaller_than_the_launch_is_an_error(oracle):
    """a buffer with fewer slots than sequences or fewer pairs than the launch writes is refused before any launch"""
    c = next(p.values[0] for p in CASES if p.id == "slab-ties-b4-3-rw32-ragged")
    q = query(c)
    I = build(oracle, c, q)
    for shape in ((c["nb"] - 1, q["partials"] + 4, 2), (c["nb"], q["partials"] - 1, 2)):
        buf = np.empty(shape, np.float32)
        buf[:] = POISON
        with pytest.raises(nb.NanoHipError):
            launch(c, I, partials=buf)
        assert np.all(bits(buf) == bits(POISON))


def test_cases_cover_every_plan_tuple():
    """The cases reach every kernel instantiation the CPU sweep finds reachable, and the axes the tuples do not carry -- read from the plans
    the query reports (CPU-only), which each case's own test also holds against the plan the case states."""
    T = []
    for p in CASES:
        assert not p.marks, (p.id, "no case may be skipped or expected to fail")
        c = p.values[0]
        q = query(c)
        assert q["takes"] == 1 and nb.ROUTE_NAMES[q["route"]] == "q4k", c["id"]
        got = {k: (plan_tuple(q) if k == "tuple" else q[k]) for k in c["target"]}
        assert got == c["target"], (c["id"], q)
        bpl = (c["n"] + 255) // 256
        T.append(dict(q, id=c["id"], tuple=plan_tuple(q), kern=plan_tuple(q)[0], kind=c["kind"], n=c["n"], rows=c["rows"], nb=c["nb"], norm=c["norm"],
                      comb=c["comb"] is not None, ties=c["ties"], total=rows_total(c["kind"], c["rows"]), GT=bpl * 8, last=c["rows"][0] % q["rw"]))
    reached = {t["tuple"] for t in T}
    assert reached == UNIVERSE, ("not reached", sorted(UNIVERSE - reached), "not in the sweep's universe", sorted(reached - UNIVERSE))
    assert len({t["id"] for t in T}) == len(T)

    def has(f=None, **kw):
        return any(all(t[k] == v for k, v in kw.items()) and (f is None or f(t)) for t in T)

    missing = []

    def need(what, ok):
        if not ok:
            missing.append(what)

    for kern in (SLAB, CHUNK):
        for nb_, B in ((3, 4), (5, 8), (6, 8), (7, 8)):
            need(("dead slots", kern, nb_, B), has(kern=kern, nb=nb_, B=B))
        need(("more than 64 KiB of LDS", kern), has(kern=kern, f=lambda t: t["lds_bytes"] > 65536))
        need(("tied maxima planted", kern), has(kern=kern, ties=True, f=lambda t: t["partials"] > 0))
    for r in (7, 33, 333):
        need(("ragged rows", r), has(nb=1, f=lambda t: t["rows"][0] == r))
        need(("ragged rows in a batch", r), has(f=lambda t: t["rows"][0] == r and t["nb"] > 1))
    need("three tensors on the slab kernel", has(kern=SLAB, rows=(36, 4, 12)))
    need("three tensors on the chunk kernel", has(kern=CHUNK, rows=(1000, 40, 36)))
    need("partial-block rows with a short last group", has(kern=SLAB, n=4100) and has(kern=SLAB, f=lambda t: t["n"] % 256 and t["n"] % 32 and t["nb"] > 1))
    need("norm_swiglu demoted to generic", has(kern=SLAB, kind=2, norm=True, B=1, role=ROLE["generic"], f=lambda t: (t["rw"] * t["GT"]) % 64 != 0))
    need("the combine at one sequence", has(comb=True, nb=1, kern=SLAB) and has(comb=True, nb=1, kern=CHUNK))
    need("the combine in a batch", has(comb=True, kern=SLAB, f=lambda t: t["nb"] > 1) and has(comb=True, kern=CHUNK, f=lambda t: t["nb"] > 1))
    need("a batch cut 2 + 2 + 1", has(kind=1, n=9732, rows=(64,), nb=5, launches=3, seqs_per_launch=2))
    need("a batch cut 4 + 3", has(kind=0, n=4100, rows=(64, 32, 32), nb=7, launches=2, seqs_per_launch=4))
    need("2..4 sequences of a wide matrix on the chunk form", has(kern=CHUNK, f=lambda t: 2 <= t["nb"] <= 4 and t["total"] * t["n"] >= 8 << 20))
    need("loop, two rounds", has(kern=CHUNK, loop=1, rounds=2))
    need("loop, three rounds or more", has(kern=CHUNK, loop=1, f=lambda t: t["rounds"] >= 3))
    need("partials, one row per workgroup", has(rw=1, f=lambda t: t["partials"] > 0))
    need("partials, a few rows per workgroup", has(f=lambda t: t["partials"] > 0 and 2 <= t["rw"] <= 16))
    need("partials, 64 rows or more per workgroup", has(f=lambda t: t["partials"] > 0 and t["rw"] >= 64))
    need("partials across the chunk kernel's waves", has(kern=CHUNK, f=lambda t: t["partials"] > 0 and t["rw"] > 64))
    for kern in (SLAB, CHUNK):
        need(("partials with a ragged last workgroup", kern), has(kern=kern, f=lambda t: t["partials"] > 1 and t["last"] != 0))
    need("partials in a slab batch with dead slots", has(kern=SLAB, f=lambda t: t["partials"] > 0 and t["nb"] < t["B"]))
    need("tied maxima planted in a slab batch", has(kern=SLAB, ties=True, f=lambda t: t["nb"] > 1))
    for why, f in (("several tensors", lambda t: len(t["rows"]) > 1 and t["kind"] == 0), ("kind 1", lambda t: t["kind"] == 1), ("kind 2", lambda t: t["kind"] == 2),
                   ("the chunk form at 2..8 sequences", lambda t: t["kern"] == CHUNK and t["nb"] > 1 and t["kind"] == 0 and len(t["rows"]) == 1),
                   ("a sliced batch", lambda t: t["launches"] > 1 and t["kind"] == 0)):
        need(("no partials: " + why), has(partials=0, f=f))
    assert not missing, missing
