// kv_copy.hip -- the one kernel that moves KV-cache rows between slots / pages: the contiguous fork (rows [0, n_pos) of a slot to every
// destination slot), the partial-block copy of a paged fork and the copy-on-write of a shared page (backend_kv.hip nano_hip_kv_fork,
// kv_ensure).  The reference has no counterpart: it keeps one cache per context (infer/infer.c:46-51) and never copies rows.
//
// Work is a JOB LIST in device memory, {src_row, dst_row, rows, keep_rows} in cache rows inside a layer plane, cut into GROUPS of jobs that
// share a source (src_row, rows, keep_rows equal): gstart[g] .. gstart[g + 1] are group g's jobs.  The grid is (group x row chunk, layer,
// K | V): a workgroup loads its vectors of the source run ONCE and stores them to every destination of the group from registers, so a fork
// into 63 slots reads the source once per plane and is one launch.  The trailing rows - keep_rows rows of a destination are written as
// zero (a forked page must not carry the source's later rows: a fresh page is zero, and non-causal attention reads unwritten rows).
// Inside a plane a run of rows is contiguous memory: it moves as 16-byte vectors (FP32 rows, FP16 rows of kv_dim % 8 == 0, FP8 rows of
// kv_dim % 16 == 0), 8-byte vectors (FP16 rows of kv_dim % 8 == 4, FP8 rows of kv_dim % 16 == 8) or 4-byte words (FP8 rows of
// kv_dim % 8 == 4: kv_dim is a multiple of 4 always); the host picks, there is no per-element path.  Plain vector loads and stores only.
#include "device_common.h"
#include "kernels.h"

namespace nano {

typedef unsigned int kvc_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int kvc_u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t KVC_THREADS = 256, KVC_UNROLL = 4;

template <typename V, bool NT>
__global__ __launch_bounds__(KVC_THREADS) void kv_copy_kernel(KvCopyArgs a) {
    const uint32_t g = blockIdx.x / a.cx, c = blockIdx.x % a.cx;
    const uint32_t j0 = a.gstart[g], j1 = a.gstart[g + 1];
    if (j0 >= j1) return;
    const KvCopyJob lead = a.jobs[j0];
    uint8_t *plane = reinterpret_cast<uint8_t *>(blockIdx.z ? a.v : a.k) + (size_t)blockIdx.y * a.plane_bytes;
    const V *src = reinterpret_cast<const V *>(plane + (size_t)lead.src_row * a.row_bytes);
    const size_t nvec = (size_t)lead.rows * a.row_bytes / sizeof(V), nkeep = (size_t)lead.keep_rows * a.row_bytes / sizeof(V);
    const size_t stride = (size_t)a.cx * KVC_THREADS;
    for (size_t i = (size_t)c * KVC_THREADS + threadIdx.x; i < nvec; i += KVC_UNROLL * stride) {
        V r[KVC_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < KVC_UNROLL; u++) {                         // the loads first: KVC_UNROLL of them in flight per lane
            const size_t idx = i + u * stride;
            r[u] = V(0u);
            if (idx < nkeep) r[u] = src[idx];
        }
        for (uint32_t j = j0; j < j1; j++) {
            V *dst = reinterpret_cast<V *>(plane + (size_t)a.jobs[j].dst_row * a.row_bytes);
#pragma unroll
            for (uint32_t u = 0; u < KVC_UNROLL; u++) {
                const size_t idx = i + u * stride;
                if (idx < nvec) {
                    if (NT) __builtin_nontemporal_store(r[u], dst + idx);
                    else dst[idx] = r[u];
                }
            }
        }
    }
}

// max_rows: the longest run of any group (sizes the chunk dimension); cus: the device's compute units.  About 8 workgroups per CU over the
// whole grid, never more chunks than a run has KVC_UNROLL x 256 vectors for.
hipError_t launch_kv_copy(KvCopyArgs a, uint32_t n_layer, uint32_t max_rows, uint32_t cus, bool nt_stores, hipStream_t st) {
    if (!a.n_groups || !max_rows || !n_layer) return hipSuccess;
    const uint32_t vb = a.row_bytes % 16 == 0 ? 16u : a.row_bytes % 8 == 0 ? 8u : 4u;
    if (a.row_bytes % vb || a.plane_bytes % vb) return hipErrorInvalidValue;
    const size_t nvec = (size_t)max_rows * a.row_bytes / vb;
    const size_t per_wg = (size_t)KVC_THREADS * KVC_UNROLL;
    size_t chunks = (nvec + per_wg - 1) / per_wg;
    const size_t planes = (size_t)a.n_groups * n_layer * 2, target = (size_t)(cus ? cus : 256u) * 8;
    size_t cx = target / planes;
    if (cx < 1) cx = 1;
    if (cx > chunks) cx = chunks;
    if ((size_t)a.n_groups * cx > 0x7fffffffull || n_layer > 65535u) return hipErrorInvalidValue;
    a.cx = (uint32_t)cx;
    const dim3 grid((uint32_t)(a.n_groups * cx), n_layer, 2), block(KVC_THREADS);
    if (vb == 16) {
        if (nt_stores) hipLaunchKernelGGL((kv_copy_kernel<kvc_u32x4, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((kv_copy_kernel<kvc_u32x4, false>), grid, block, 0, st, a);
    } else if (vb == 8) {
        if (nt_stores) hipLaunchKernelGGL((kv_copy_kernel<kvc_u32x2, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((kv_copy_kernel<kvc_u32x2, false>), grid, block, 0, st, a);
    } else {
        if (nt_stores) hipLaunchKernelGGL((kv_copy_kernel<uint32_t, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((kv_copy_kernel<uint32_t, false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace nano
