// pool.hip -- text embeddings: the final-norm hidden states of a ragged pass's rows, pooled per segment (include/nano_mi355x.h
// "text embeddings").  One launch behind each pass, one workgroup of 256 threads per segment that has pooled rows in
// the pass; the pass's residual rows are read where the pass left them (m->x, row stride n_embd), nothing is copied.
//
// What a workgroup is told (PoolArgs::groups, 4 words per workgroup, built on the host from the call's row map by pool_plan() in
// backend_rows.hip): the segment, where the ascending list of its pooled pass rows starts in PoolArgs::lists, how many there are,
// whether the segment began in an earlier pass (the running sum is seeded from acc[seg]) and whether it ends in this one (the workgroup
// finishes it: divide, truncate, normalise, store; else the running sum goes back to acc[seg]), and the segment's row count.
//
// The float chains (every one fixed: no atomics, no dependence on the pass a row landed in, its pass row, or the other rows):
//   * per-row norm (fast form, w != nullptr).  One wave per row, the segment's rows dealt round-robin to the 4 waves.  Lane l takes the
//     column quads q = l, l + 64, l + 128, ... (quad q = columns 4q .. 4q + 3; columns >= n_embd count as 0) in ascending q and adds
//     their squares one at a time, x0^2 first: s_l = ((((0 + x0^2) + x1^2) + x2^2) + x3^2) + ...  The 64 lane sums are added by the xor
//     butterfly of wave_sum() (partners 32, 16, 8, 4, 2, 1 lanes apart: a balanced tree of depth 6, every lane gets the same bits).
//     inv = 1 / sqrtf(sum / n_embd + 1e-5f) with IEEE divide and sqrt; y[i] = w[i] * (x[i] * inv).
//     (ordered form, w == nullptr: the rows were normed by the reference-order rmsnorm launch, y = x.)
//   * pooling.  A thread owns the columns tid * 4 + 1024 j; per column the rows are added in ascending position, plain FP32 adds:
//     acc = y_0, then acc = acc + y_r.  LAST has one pooled row per segment.  MEAN divides once, acc / (float)count.
//   * truncation: only columns < dim are computed, stored or summed.
//   * normalisation (fast form): thread t adds the squares of its own columns in ascending column order, s_t = (0 + v_a^2) + v_b^2 ...;
//     block_sum() adds the 64 threads of a wave by the same butterfly and then the 4 wave sums in ascending wave order from 0.
//     (ordered form: thread 0 adds v[i]^2 for i = 0 .. dim - 1 in ascending order.)  out = v * (1 / sqrtf(sum)); sum == 0: zeros.
// Loads are dwordx4 where n_embd % 4 == 0 (every row then starts 16-byte aligned), else four predicated dword loads; nothing is read
// past a row.  The running sums have a row stride of dim rounded up to 4, so they always move as dwordx4; out rows have stride dim and
// are stored as dwordx4 where dim % 4 == 0, else as predicated dwords.  No scalar-unit stores, no atomics.
#include "device_common.h"
#include "kernels.h"

namespace nano {

namespace {

__device__ __forceinline__ float4 pool_load4(const float *row, uint32_t c, uint32_t lim, bool vec) {
    if (vec) return *reinterpret_cast<const float4 *>(row + c);              // (c < lim, lim % 4 == 0: the quad is inside the row)
    float4 v;
    v.x = c < lim ? row[c] : 0.0f; v.y = c + 1 < lim ? row[c + 1] : 0.0f; v.z = c + 2 < lim ? row[c + 2] : 0.0f; v.w = c + 3 < lim ? row[c + 3] : 0.0f;
    return v;
}
__device__ __forceinline__ void pool_store4(float *row, uint32_t c, uint32_t lim, bool vec, float4 v) {
    if (vec) { *reinterpret_cast<float4 *>(row + c) = v; return; }
    if (c < lim) row[c] = v.x;
    if (c + 1 < lim) row[c + 1] = v.y;
    if (c + 2 < lim) row[c + 2] = v.z;
    if (c + 3 < lim) row[c + 3] = v.w;
}

__global__ __launch_bounds__(POOL_THREADS) void pool_rows_kernel(const PoolArgs a) {
    __shared__ float inv[POOL_MAX_ROWS];
    __shared__ float red[POOL_THREADS / 64 + 1];
    const uint32_t *g = a.groups + (size_t)blockIdx.x * POOL_GROUP_WORDS;
    const uint32_t seg = g[0], n = g[2] & POOL_N_MASK, count = g[3], tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const bool begun = (g[2] & POOL_BEGUN) != 0, ends = (g[2] & POOL_ENDS) != 0;
    const uint32_t *list = a.lists + g[1];
    const uint32_t E = a.n_embd, dim = a.dim, dpad = (dim + 3u) & ~3u;
    const bool xvec = (E & 3u) == 0 && (a.x_stride & 3u) == 0, ovec = (dim & 3u) == 0;
    if (a.w) {
        // phase a: every pooled row's inverse RMS, one wave per row
        for (uint32_t i = wid; i < n; i += POOL_THREADS / 64) {
            const float *row = a.x + (size_t)list[i] * a.x_stride;
            float s = 0.0f;
            for (uint32_t c = lane * 4u; c < E; c += 256u) {
                const float4 v = pool_load4(row, c, E, xvec);
                s += v.x * v.x; s += v.y * v.y; s += v.z * v.z; s += v.w * v.w;
            }
            s = wave_sum(s);
            if (lane == 0) inv[i] = 1.0f / sqrtf(s / (float)E + 1e-5f);
        }
        __syncthreads();
    }
    // phase b: the columns below dim, a quad per thread and tile of 1024; the rows in ascending position
    float *acc_row = a.acc + (size_t)seg * dpad, *out_row = a.out + (size_t)seg * dim;
    const float fcount = (float)count;
    float ss = 0.0f;
    for (uint32_t c = tid * 4u; c < dim; c += POOL_THREADS * 4u) {
        float4 w4 = make_float4(1.0f, 1.0f, 1.0f, 1.0f), acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (a.w) w4 = pool_load4(a.w, c, dim, (E & 3u) == 0);
        if (begun) acc = *reinterpret_cast<const float4 *>(acc_row + c);
#pragma unroll 4
        for (uint32_t i = 0; i < n; i++) {
            float4 y = pool_load4(a.x + (size_t)list[i] * a.x_stride, c, dim, xvec);
            if (a.w) {
                const float r = inv[i];
                y.x = w4.x * (y.x * r); y.y = w4.y * (y.y * r); y.z = w4.z * (y.z * r); y.w = w4.w * (y.w * r);
            }
            if (i == 0 && !begun) acc = y;
            else { acc.x += y.x; acc.y += y.y; acc.z += y.z; acc.w += y.w; }
        }
        if (!ends) { *reinterpret_cast<float4 *>(acc_row + c) = acc; continue; }
        if (a.mean) { acc.x /= fcount; acc.y /= fcount; acc.z /= fcount; acc.w /= fcount; }
        if (c < dim) ss += acc.x * acc.x;
        if (c + 1 < dim) ss += acc.y * acc.y;
        if (c + 2 < dim) ss += acc.z * acc.z;
        if (c + 3 < dim) ss += acc.w * acc.w;
        pool_store4(out_row, c, dim, ovec, acc);
    }
    if (!ends || !a.normalize) return;                                       // (wave-uniform: the group's words)
    float total;
    if (a.w) total = block_sum(ss, red);
    else {
        __syncthreads();                                                     // the workgroup's own stores of v, visible to thread 0
        if (tid == 0) {
            float s = 0.0f;
            for (uint32_t i = 0; i < dim; i++) s += out_row[i] * out_row[i];
            red[0] = s;
        }
        __syncthreads();
        total = red[0];
    }
    const float scale = total > 0.0f ? 1.0f / sqrtf(total) : 0.0f;
    for (uint32_t c = tid * 4u; c < dim; c += POOL_THREADS * 4u) {         // every thread rescales the columns it stored itself
        float4 v = pool_load4(out_row, c, dim, ovec);
        v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
        pool_store4(out_row, c, dim, ovec, v);
    }
}

}  // namespace

hipError_t launch_pool_rows(const PoolArgs &a, uint32_t n_groups, hipStream_t st) {
    if (!n_groups) return hipSuccess;
    if (!a.x || !a.groups || !a.lists || !a.acc || !a.out || !a.n_embd || !a.dim || a.dim > a.n_embd || a.x_stride < a.n_embd ||
        a.rows_max > POOL_MAX_ROWS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pool_rows_kernel, dim3(n_groups), dim3(POOL_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace nano
