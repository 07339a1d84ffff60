// gemv_q4k_host.h -- host-side planning shared by the Q4K GEMV translation units: the two searches behind gemv_q4k_plan() and the
// launchers that consume its plan.
#pragma once
#include "kernels.h"

namespace nano {

inline uint32_t q4k_capacity(uint32_t nb) { return nb <= 1 ? 1u : nb <= 2 ? 2u : nb <= 4 ? 4u : 8u; }     // the template capacity B / NB of nb sequences

// gemv_q4k.hip, the item kernel: rows per workgroup, threads, (row, group) items per thread and float4 activation items per thread at
// capacity B (ipt > 4: no such kernel), and the dynamic LDS of such a launch
struct Q4kSlabPlan { uint32_t rw, nthr, ipt, nv; };
Q4kSlabPlan plan_q4k(const GemvArgs &a, int B);
size_t q4k_lds_bytes(uint32_t n, uint32_t epi, bool combine, uint32_t attn_n_head, uint32_t rw, uint32_t B);
hipError_t launch_q4k_slab(const GemvArgs &a, const Q4kGemvPlan &p, hipStream_t st);

// gemv_q4k_chunk.hip, the chunk kernel: the ONE search behind gemv_q4k_plan(), the quantizer launch and the fused q | k | v + attention
// launch (force_nw: its 256 threads -- same bits, see q4k_fused_shape).  false: the kernel does not take the shape.
struct ChunkPlan { uint32_t rw, nthr, d, loop, rounds, nv, wg[3], grid; size_t lds; };
bool plan_chunk(const GemvArgs &a, ChunkPlan &p, uint32_t force_nw = 0);
hipError_t launch_q4k_chunk(const GemvArgs &a, const Q4kGemvPlan &p, hipStream_t st);

}  // namespace nano
