// kv_image.hip -- the one kernel between the KV cache and a KV image (include/nano_mi355x.h "KV images", kv_image.h): PACK gathers a
// slot's rows into a contiguous device staging buffer in image order, UNPACK scatters them back (backend_kv.hip nano_hip_kv_save /
// nano_hip_kv_restore; the staging buffer travels to and from the host by plain copies).  The reference has no counterpart: it keeps one
// cache per context (infer/infer.c:46-51) and never moves rows.
//
// kv_copy.hip's discipline.  Work is a JOB LIST in device memory, {cache_row, staging_off, rows, zero_rows} in cache rows inside a layer
// plane (kernels.h KvImageJob): on the contiguous cache one job per staging chunk with the slot's base folded into cache_row, on the paged
// cache one job per 64-position block through the host's page table.  The grid is (job x block of the job x row chunk, layer, K | V).
// The rows of one block in one plane are contiguous memory on both sides -- 64 consecutive cache rows, one run of the image -- so they
// move as 16-byte vectors (FP32 rows, FP16 rows of kv_dim % 8 == 0, FP8 rows of kv_dim % 16 == 0), 8-byte vectors (FP16 rows of
// kv_dim % 8 == 4, FP8 rows of kv_dim % 16 == 8) or 4-byte words (FP8 rows of kv_dim % 8 == 4: kv_dim is a multiple of 4 always); the
// host picks by launch_kv_copy's rule, there is no per-element path.  KVI_UNROLL loads are in flight per lane before the first store.
// Plain vector loads and stores only: no atomics, no waits on other workgroups.
#include "device_common.h"
#include "kernels.h"

namespace nano {

typedef unsigned int kvi_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int kvi_u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t KVI_THREADS = 256, KVI_UNROLL = 4;

template <typename V, bool PACK>
__global__ __launch_bounds__(KVI_THREADS) void kv_image_kernel(KvImageArgs a) {
    const uint32_t g = blockIdx.x / a.cx, c = blockIdx.x % a.cx;
    const uint32_t ji = g / a.job_blocks, bi = g % a.job_blocks;
    const KvImageJob job = a.jobs[ji];
    if (bi * 64u >= job.rows) return;                                       // (a job shorter than the longest one)
    const uint32_t left = job.rows - bi * 64u, run = left < 64u ? left : 64u;                   // rows of this block's runs
    // rows of the block that come from the other side; rows of the destination behind them that are written as zero
    uint32_t live = run, zero = 0;
    if (PACK) { const uint32_t keep = job.rows - job.zero_rows; live = keep <= bi * 64u ? 0u : keep - bi * 64u < run ? keep - bi * 64u : run; zero = run - live; }
    else if (left <= 64u) zero = job.zero_rows;                             // (the job's last block)
    uint8_t *plane = reinterpret_cast<uint8_t *>(blockIdx.z ? a.v : a.k) + (size_t)blockIdx.y * a.plane_bytes;
    V *cache = reinterpret_cast<V *>(plane + ((size_t)job.cache_row + bi * 64u) * a.row_bytes);
    V *stage = reinterpret_cast<V *>(reinterpret_cast<uint8_t *>(a.staging) + job.staging_off + (size_t)bi * 64u * a.n_layer * 2u * a.row_bytes +
                                     (size_t)(blockIdx.y * 2u + blockIdx.z) * run * a.row_bytes);
    const V *src = PACK ? cache : stage;
    V *dst = PACK ? stage : cache;
    const uint32_t nlive = live * a.row_bytes / (uint32_t)sizeof(V), nvec = (live + zero) * a.row_bytes / (uint32_t)sizeof(V);
    const uint32_t stride = a.cx * KVI_THREADS;
    for (uint32_t i = c * KVI_THREADS + threadIdx.x; i < nvec; i += KVI_UNROLL * stride) {
        V r[KVI_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < KVI_UNROLL; u++) {                         // the loads first: KVI_UNROLL of them in flight per lane
            const uint32_t idx = i + u * stride;
            r[u] = V(0u);
            if (idx < nlive) r[u] = src[idx];
        }
#pragma unroll
        for (uint32_t u = 0; u < KVI_UNROLL; u++) {
            const uint32_t idx = i + u * stride;
            if (idx < nvec) dst[idx] = r[u];
        }
    }
}

// About 8 workgroups per CU over the whole grid, never more chunks than a block's run has KVI_UNROLL x 256 vectors for.
hipError_t launch_kv_image(KvImageArgs a, bool pack, uint32_t cus, hipStream_t st) {
    if (!a.n_jobs || !a.job_blocks || !a.n_layer) return hipSuccess;
    const uint32_t vb = a.row_bytes % 16 == 0 ? 16u : a.row_bytes % 8 == 0 ? 8u : 4u;
    if (!a.row_bytes || a.row_bytes % vb || a.plane_bytes % vb || 64ull * a.row_bytes > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t nvec = (size_t)64 * a.row_bytes / vb, per_wg = (size_t)KVI_THREADS * KVI_UNROLL;
    const size_t chunks = (nvec + per_wg - 1) / per_wg;
    const size_t blocks = (size_t)a.n_jobs * a.job_blocks, planes = blocks * a.n_layer * 2, target = (size_t)(cus ? cus : 256u) * 8;
    size_t cx = target / planes;
    if (cx < 1) cx = 1;
    if (cx > chunks) cx = chunks;
    if (blocks * cx > 0x7fffffffull || a.n_layer > 65535u) return hipErrorInvalidValue;
    a.cx = (uint32_t)cx;
    const dim3 grid((uint32_t)(blocks * cx), a.n_layer, 2), block(KVI_THREADS);
    if (vb == 16) {
        if (pack) hipLaunchKernelGGL((kv_image_kernel<kvi_u32x4, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((kv_image_kernel<kvi_u32x4, false>), grid, block, 0, st, a);
    } else if (vb == 8) {
        if (pack) hipLaunchKernelGGL((kv_image_kernel<kvi_u32x2, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((kv_image_kernel<kvi_u32x2, false>), grid, block, 0, st, a);
    } else {
        if (pack) hipLaunchKernelGGL((kv_image_kernel<uint32_t, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((kv_image_kernel<uint32_t, false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace nano
