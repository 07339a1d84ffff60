// exact.hip -- the float chains of the forward in the REFERENCE'S OWN ORDER, built to be replayed: the kernels of exact mode
// (NANO_EXACT=1 / nano_hip_set_exact).  Same bits as strict.hip's (the reference CPU engine's), fewer launches and no chain that
// waits on global memory: every chain reads its terms from LDS or registers, the loads in front of it are coalesced and issued ahead.
//
//   exact_rmsnorm_kernel     infer/infer.c:601-614   x and the squares x[j]*x[j] staged in LDS by the whole workgroup; one lane adds
//                                                    the squares in index order (32 per round, read as float4); w[j] * (ss * x[j])
//   exact_attention_kernel   infer/infer.c:810-879   ONE launch per layer for q / k prep + scores + softmax + weighted V, att[range] in LDS:
//                              prep     (fold_prep) [rmsnorm] + RoPE of the q head and of its KV group's k row at pos; k row -> cache
//                              scores   one lane per position t, score += q[i]*k[t][i] for i ascending; a wave's 64 K rows reach its
//                                       lanes 32 columns at a time through coalesced float4 loads and an LDS transposition
//                              softmax  infer.c:616-634: max (order-free), exact_expf(x - max), the sum in index order on one lane
//                                       out of LDS, x /= sum
//                              V        one lane per output element i, o += att[t] * v[t][i] for t ascending; the V rows of the next
//                                       16 positions are in flight while the chain works on the current 16
//
// The index-order sums (squares, softmax denominator) run term by term on one lane (exact_chain.h chain_sum_plain's order).
// exact_chain.h's chunked evaluation (chain_sum_chunked; CPU-checked by tools/exact/ssq_check.cpp) has no device form yet: with
// one 64-term chunk per wave and four waves it does about as many dependent instructions as the 1024-term chain it replaces
// (DESIGN.md section 4 has the count and the measured time of this form).
//
// The attention launch holds att[range] in the workgroup's LDS; range can reach the model's max_seq_len (one graph serves every
// position).  exact_attention_fits() says whether that fits XA_LDS_BYTES; where it does not (max_seq_len > 7168) the step keeps
// strict.hip's three attention launches with att in global memory (backend_step.hip enqueue_step_ordered), so no context length is refused.
#include "device_common.h"
#include "exact_math.h"
#include "kernels.h"

namespace nano {

namespace {

constexpr uint32_t XA_THREADS = 256, XA_DC = 32, XA_TILE = 64 * (XA_DC + 1), XA_VU = 16;
constexpr uint32_t XA_FIXED = 256 + 256 + XA_THREADS + (XA_THREADS / 64) * XA_TILE;    // floats: q | k row of pos | reduction cells | one K tile per wave
constexpr uint32_t XA_LDS_BYTES = 64u * 1024u;

// sum of p[0..n) in index order, p in LDS (16-byte aligned): the reference's loop.  32 terms per round, read as float4; the next
// round's reads are issued before this round's adds, so the chain waits on its own adds only (one lane's LDS read takes ~50+ cycles)
__device__ __forceinline__ float lds_chain_sum(const float *p, uint32_t n) {
    float s = 0.0f;
    uint32_t j = 0;
    float4 cur[8], nxt[8];
    if (n >= 32) {
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) cur[k] = *reinterpret_cast<const float4 *>(p + 4 * k);
    }
    for (; j + 32 <= n; j += 32) {
        if (j + 64 <= n) {
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) nxt[k] = *reinterpret_cast<const float4 *>(p + j + 32 + 4 * k);
        }
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) { s += cur[k].x; s += cur[k].y; s += cur[k].z; s += cur[k].w; }
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) cur[k] = nxt[k];
    }
    for (; j < n; j++) s += p[j];
    return s;
}

// keep_x: x stays in LDS next to its squares (2 n floats fit); else the output pass reads x again
__global__ __launch_bounds__(256) void exact_rmsnorm_kernel(float *o, const float *x, const float *w, uint32_t n, uint32_t x_stride, uint32_t o_stride, uint32_t keep_x) {
    extern __shared__ __align__(16) float sh[];                    // p[n4] | cell[4] | x[n] (keep_x)
    const uint32_t n4 = (n + 3u) & ~3u, tid = threadIdx.x;
    float *p = sh, *cell = sh + n4, *xs = cell + 4;
    const float *xv = x + (size_t)blockIdx.x * x_stride;
    float *ov = o + (size_t)blockIdx.x * o_stride;
    for (uint32_t j = tid; j < n; j += blockDim.x) { const float v = xv[j]; p[j] = v * v; if (keep_x) xs[j] = v; }
    __syncthreads();
    if (tid == 0) {
        float ss = lds_chain_sum(p, n);
        ss /= (float)n;
        ss += 1e-5f;
        ss = 1.0f / sqrtf(ss);
        cell[0] = ss;
    }
    __syncthreads();
    const float ss = cell[0];
    for (uint32_t j = tid; j < n; j += blockDim.x) ov[j] = w[j] * (ss * (keep_x ? xs[j] : xv[j]));
}

__global__ __launch_bounds__(XA_THREADS) void exact_attention_kernel(const StrictAttnArgs a, uint32_t att_cap) {
    extern __shared__ __align__(16) float sh[];                    // att[att_cap] | q[256] | k[256] | red[256] | tile[4][64][33]
    const uint32_t h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, hd = a.hd;
    float *att = sh, *qs = sh + att_cap, *ks = qs + 256, *red = ks + 256, *tile = red + XA_THREADS + wave * XA_TILE;
    const uint32_t pos = a.pos[b];
    uint32_t range = a.is_causal ? pos + 1u : a.S;
    if (range > a.S) range = a.S;                                  // (never: the host checks pos < S; att holds att_cap >= S cells)
    const uint32_t kv_mul = a.n_head / a.n_kv_head;
    const size_t head_off = (((size_t)(a.slot0 + b) * a.n_layer + a.layer) * a.S) * a.kv_dim + (size_t)(h / kv_mul) * hd;
    const float *kbase = a.kcache + head_off, *vbase = a.vcache + head_off;
    const float *qh = a.q + (size_t)b * a.q_dim + (size_t)h * hd;
    uint32_t kpos = 0xffffffffu;                                   // the row whose k comes from LDS instead of the cache
    if (a.fold_prep) {
        // ---- q / k prep (infer.c:810-835; strict_qk_kernel's expressions): [rmsnorm] + RoPE of q head h, in place, and of the k head
        // of its KV group at pos.  Every head of a group prepares the k row for itself (it may not wait for a sibling workgroup's
        // store); the group's first head stores it to the cache.
        const uint32_t half = hd >> 1, g = h / kv_mul;
        const float *kr = a.kraw + (size_t)b * a.kv_dim + (size_t)g * hd;
        float *sq = red + XA_THREADS;                              // squares of q | k, in the tile region (free until the scores)
        for (uint32_t j = tid; j < hd; j += XA_THREADS) { const float qv = qh[j], kv = kr[j]; qs[j] = qv; ks[j] = kv; sq[j] = qv * qv; sq[256 + j] = kv * kv; }
        __syncthreads();
        if (a.q_norm || a.k_norm) {                                // Qwen3 q/k-norm (infer.c:824-835): one lane per chain
            if ((tid == 0 && a.q_norm) || (tid == 64 && a.k_norm)) {
                float ss = lds_chain_sum(sq + (tid == 0 ? 0 : 256), hd);
                ss /= (float)hd;
                ss += 1e-5f;
                ss = 1.0f / sqrtf(ss);
                red[tid == 0 ? 0 : 1] = ss;
            }
            __syncthreads();
            for (uint32_t j = tid; j < hd; j += XA_THREADS) {
                if (a.q_norm) qs[j] = a.q_norm[j] * (red[0] * qs[j]);
                if (a.k_norm) ks[j] = a.k_norm[j] * (red[1] * ks[j]);
            }
            __syncthreads();
        }
        if (a.rope_cos) {
            const float *fcr = a.rope_cos + (size_t)pos * half, *fci = a.rope_sin + (size_t)pos * half;
            for (uint32_t p = tid; p < 2u * half; p += XA_THREADS) {       // pairs of q, then pairs of k: a thread reads and writes its own pair only
                float *v = p < half ? qs : ks;
                const uint32_t pp = p < half ? p : p - half;
                const float c = fcr[pp], sn = fci[pp];
                if (a.rope_qwen3) {                                    // infer.c:692-706
                    const float x0 = v[pp], x1 = v[pp + half];
                    v[pp] = x0 * c - x1 * sn;
                    v[pp + half] = x1 * c + x0 * sn;
                } else {                                               // infer.c:681-690
                    const float x0 = v[2 * pp], x1 = v[2 * pp + 1];
                    v[2 * pp] = x0 * c - x1 * sn;
                    v[2 * pp + 1] = x0 * sn + x1 * c;
                }
            }
            __syncthreads();
        }
        float *qout = a.q + (size_t)b * a.q_dim + (size_t)h * hd;      // finished q in place, as strict_qk_kernel leaves it (nano_hip_read_state)
        float *kout = a.kcache + head_off + (size_t)pos * a.kv_dim;
        for (uint32_t j = tid; j < hd; j += XA_THREADS) { qout[j] = qs[j]; if (h % kv_mul == 0) kout[j] = ks[j]; }
        kpos = pos;
    } else {
        for (uint32_t j = tid; j < hd; j += XA_THREADS) qs[j] = qh[j];
    }

    // ---- scores (infer.c:850-861) ----
    // One item = 32 columns of one round of blocks (a round: XA_THREADS / 64 blocks of 64 positions, one per wave); the K loads of the
    // next item are issued before this item's tile is written and walked.
    const uint32_t nblk = (range + 63u) / 64u, lr = lane >> 3, lc = (lane & 7u) * 4u;
    const uint32_t nchunk = (hd + XA_DC - 1u) / XA_DC, nitem = ((nblk + XA_THREADS / 64 - 1u) / (XA_THREADS / 64)) * nchunk;
    const float *trow = tile + lane * (XA_DC + 1);
    auto load_item = [&](uint32_t it, float4 (&v)[8]) {
        const uint32_t t0 = ((it / nchunk) * (XA_THREADS / 64) + wave) * 64u, c0 = (it % nchunk) * XA_DC;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t row = t0 + lr + 8u * k;                 // (rows beyond the range are never read: the cache may end there)
            v[k] = !(row < range && c0 + lc < hd) ? make_float4(0.0f, 0.0f, 0.0f, 0.0f)
                 : row == kpos ? *reinterpret_cast<const float4 *>(ks + c0 + lc) : *reinterpret_cast<const float4 *>(kbase + (size_t)row * a.kv_dim + c0 + lc);
        }
    };
    float4 kc[8], kn[8];
    load_item(0, kc);
    float score = 0.0f;
    for (uint32_t it = 0; it < nitem; it++) {
        if (it + 1 < nitem) load_item(it + 1, kn);
        const uint32_t t0 = ((it / nchunk) * (XA_THREADS / 64) + wave) * 64u, c0 = (it % nchunk) * XA_DC;
        __syncthreads();                                           // the previous tile has been read (and q is staged)
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            float *d = tile + (lr + 8u * k) * (XA_DC + 1) + lc;
            d[0] = kc[k].x; d[1] = kc[k].y; d[2] = kc[k].z; d[3] = kc[k].w;
        }
        __syncthreads();
        if (c0 == 0) score = 0.0f;
        const uint32_t lim = hd - c0 < XA_DC ? hd - c0 : XA_DC;
        if (lim == XA_DC) {
#pragma unroll
            for (uint32_t i = 0; i < XA_DC; i++) score += qs[c0 + i] * trow[i];
        } else {
            for (uint32_t i = 0; i < lim; i++) score += qs[c0 + i] * trow[i];
        }
        if (c0 + XA_DC >= hd) {                                    // the row's last columns: infer.c:860
            score /= sqrtf((float)hd);
            if (t0 + lane < range) att[t0 + lane] = score;
        }
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) kc[k] = kn[k];
    }
    __syncthreads();

    // ---- softmax (infer.c:616-634) ----
    float m = -INFINITY;                                           // the maximum does not depend on the scan order
    for (uint32_t t = tid; t < range; t += XA_THREADS) m = fmaxf(m, att[t]);
    red[tid] = m;
    __syncthreads();
    for (uint32_t s = XA_THREADS / 2; s > 0; s >>= 1) { if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]); __syncthreads(); }
    m = red[0];
    __syncthreads();
    for (uint32_t t = tid; t < range; t += XA_THREADS) att[t] = nano_exact::exact_expf(att[t] - m, nano_exact::kExp2Tab);
    __syncthreads();
    if (tid == 0) red[0] = lds_chain_sum(att, range);
    __syncthreads();
    const float sum = red[0];
    for (uint32_t t = tid; t < range; t += XA_THREADS) att[t] /= sum;
    __syncthreads();

    // ---- weighted V (infer.c:866-877) ----
    if (tid < hd) {
        const float *vp = vbase + tid;
        float cur[XA_VU], nxt[XA_VU];
#pragma unroll
        for (uint32_t k = 0; k < XA_VU; k++) cur[k] = k < range ? vp[(size_t)k * a.kv_dim] : 0.0f;
        float o = 0.0f;
        for (uint32_t t = 0; t < range; t += XA_VU) {
#pragma unroll
            for (uint32_t k = 0; k < XA_VU; k++) nxt[k] = t + XA_VU + k < range ? vp[(size_t)(t + XA_VU + k) * a.kv_dim] : 0.0f;
            if (t + XA_VU <= range) {
#pragma unroll
                for (uint32_t k = 0; k < XA_VU; k++) o += att[t + k] * cur[k];
            } else {                                               // the last, partial group (cur[] stays in registers: no dynamic index)
#pragma unroll
                for (uint32_t k = 0; k < XA_VU; k++) if (t + k < range) o += att[t + k] * cur[k];
            }
#pragma unroll
            for (uint32_t k = 0; k < XA_VU; k++) cur[k] = nxt[k];
        }
        a.xba[(size_t)b * a.q_dim + (size_t)h * hd + tid] = o;
    }
}

}  // namespace

hipError_t launch_exact_rmsnorm(float *o, const float *x, const float *w, uint32_t n, uint32_t nvec, uint32_t x_stride, uint32_t o_stride, hipStream_t st) {
    const uint32_t n4 = (n + 3u) & ~3u;
    if (n == 0 || (size_t)(n4 + 4) * 4 > XA_LDS_BYTES) return hipErrorInvalidValue;
    const uint32_t keep_x = (size_t)(n4 + 4 + n) * 4 <= XA_LDS_BYTES ? 1u : 0u;
    hipLaunchKernelGGL(exact_rmsnorm_kernel, dim3(nvec), dim3(256), (size_t)(n4 + 4 + (keep_x ? n : 0)) * 4, st, o, x, w, n, x_stride, o_stride, keep_x);
    return hipGetLastError();
}

bool exact_attention_fits(uint32_t hd, uint32_t max_range) {
    return hd <= 256 && hd % 4u == 0 && (size_t)(((max_range + 3u) & ~3u) + XA_FIXED) * 4 <= XA_LDS_BYTES;
}

hipError_t launch_exact_attention(const StrictAttnArgs &a, uint32_t nb, hipStream_t st) {
    if (!exact_attention_fits(a.hd, a.S) || a.kv_dim % 4u) return hipErrorInvalidValue;
    const uint32_t att_cap = (a.S + 3u) & ~3u;
    hipLaunchKernelGGL(exact_attention_kernel, dim3(a.n_head, nb), dim3(XA_THREADS), (size_t)(att_cap + XA_FIXED) * 4, st, a, att_cap);
    return hipGetLastError();
}

}  // namespace nano
