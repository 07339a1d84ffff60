// gemm_q80_host.h -- host-side planning of the batched Q80 kernels (G6 gemm_q80_g6.hip, G7 / G7K gemm_q80_g7.hip, GC gemm_q80_cls.hip,
// G2 gemm_q80.hip): the sizes the kernels' LDS layouts are built from, one section planner per kernel -- each fills its part of a
// Q80GemmPlan (kernels.h) or refuses --, the prototypes of the launchers that consume a plan and the one helper they share to raise a
// kernel's LDS limit (the only code here that calls the runtime).  gemm_q80_plan() (route.hip) puts the sections in their order of
// preference; the planners are arithmetic on a shape and touch no device.
#pragma once
#include <atomic>
#include "kernels.h"

namespace nano {

constexpr uint32_t Q80_GEMM_LDS_MAX = 160u * 1024u;             // what a CU has: every kernel's request is held to it here, not at launch

constexpr uint32_t G6_PITCH = 528, G6_WBUF = 16 * G6_PITCH;
constexpr uint32_t G6_LDS_WAVE = G6_WBUF + 512 + 512;          // + weight scales [8 groups][16 rows] + (F) activation scales [8][16 tokens]
constexpr uint32_t G6_NW = 8;                                   // waves of a workgroup (launches with fewer items use fewer)

constexpr uint32_t G7_NCW = 14;                     // consumer waves
constexpr uint32_t G7_NLA = 2;                      // weight loader waves (steps k % 2)
constexpr uint32_t G7_NW = G7_NCW + G7_NLA;         // 16 waves: four per SIMD (<= 128 registers each)
constexpr uint32_t G7_MAXNSA = 32;
constexpr uint32_t G7_LDS = Q80_GEMM_LDS_MAX;
constexpr uint32_t G7K_STAGE = 4096u + 256u;        // a stage: the tile's 16 rows x 256 B, then its 16 x 4 weight scales

constexpr uint32_t GC_PITCH = 528, GC_WBUF = 16 * GC_PITCH;             // transposition buffer of one wave: 16 rows x 512 B
constexpr uint32_t GC_LDS_WAVE = GC_WBUF + 512;                         // + weight scales [8 groups][16 rows]

constexpr uint32_t G2_PK = 512, G2_PITCH = 528;

// raise a kernel's dynamic LDS limit to a CU's 160 KiB, once per device (a bit each): the attribute call is a host round trip and stays
// off the per-launch path
template <auto KERN> static inline void q80_gemm_lds_limit_once() {
    static std::atomic<unsigned long long> armed{0};
    int dev = 0; (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !((armed.load(std::memory_order_acquire) >> dev) & 1ull)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)Q80_GEMM_LDS_MAX);
        if (dev >= 0 && dev < 64) armed.fetch_or(1ull << dev, std::memory_order_release);
    }
}

static inline uint32_t q80_gemm_token_tiles(const GemvArgs &a) { return (a.nb + 15u) / 16u; }
static inline uint32_t q80_gemm_tt(const GemvArgs &a) { const uint32_t t = q80_gemm_token_tiles(a); return t <= 1u ? 1u : t == 2u ? 2u : 4u; }   // the TT template value: 1 | 2 | 4

// what the canonical-fold kernels (G6, G7) take: group size 64, whole 256-value chunks, one to three tensors (SwiGLU: the pair), 32-bit
// buffer offsets per segment, not the classifier (it has kernels of its own: STREAM / GC)
static inline bool q80_gemm_canon_shape(const GemvArgs &a) {
    if (a.gs != 64 || a.nb == 0 || a.nb > 64 || a.n % 256u || a.nseg == 0 || a.nseg > 3 || a.resid_add || a.tile_max || a.attn_part) return false;
    if (a.epi == GEMV_EPI_SWIGLU && (a.nseg != 2 || a.seg[0].rows != a.seg[1].rows)) return false;
    const uint32_t nseg = a.epi == GEMV_EPI_SWIGLU ? 1u : a.nseg;
    for (uint32_t s = 0; s < nseg; s++) if ((uint64_t)a.seg[s].rows * a.n >= (1ull << 32) - (1u << 20)) return false;
    return gemv_total_rows(a) < 65536u;
}

// Row tiles of G6 and G7: a TILE is up to 16 matrix rows = two halves of hh <= 8 rows (SwiGLU: half 0 = rows of W1, half 1 = the same rows
// of W3), a tile stays inside one weight tensor, workgroup b owns tiles b, b + grid, ...  The height is fitted to the chip: the one that
// minimises cost(tiles of the busiest workgroup, bytes a tile streams per row step + a per-tile overhead worth ~2 rows), ties to the
// taller tile.
template <class Cost> static inline void q80_gemm_row_tiles(const GemvArgs &a, Q80GemmPlan &p, Cost cost) {
    const bool sw = a.epi == GEMV_EPI_SWIGLU;
    const uint32_t cus = a.cus ? a.cus : 256u, nseg = sw ? 1u : a.nseg;
    auto tiles_of = [&](uint32_t trw, uint32_t *tc) {
        uint32_t tiles = 0;
        for (uint32_t s = 0; s < nseg; s++) { tiles += (a.seg[s].rows + trw - 1) / trw; if (tc && s < 2) tc[s] = tiles; }
        return tiles;
    };
    uint32_t best = 0, best_cost = ~0u;
    for (uint32_t hh = 1; hh <= 8; hh++) {
        const uint32_t trw = sw ? hh : 2u * hh, tiles = tiles_of(trw, nullptr);
        const uint32_t grid = tiles < cus ? tiles : cus, tpw = (tiles + grid - 1) / grid;
        const uint32_t c = cost(tpw, trw * (sw ? 2u : 1u) + 2u);
        if (c <= best_cost) { best_cost = c; best = hh; }              // ties: the taller tile
    }
    uint32_t tc[2] = {0xffffffffu, 0xffffffffu};
    p.hh = best;
    p.ntiles = tiles_of(sw ? best : 2u * best, tc);
    p.tc0 = nseg > 1 ? tc[0] : 0xffffffffu; p.tc1 = nseg > 2 ? tc[1] : 0xffffffffu;
    p.grid = p.ntiles < cus ? p.ntiles : cus; p.tpw = (p.ntiles + p.grid - 1) / p.grid;
    p.full = p.ntiles - (p.tpw - 1u) * p.grid;
    p.ms = (!sw && a.nseg > 1) ? 1u : 0u;
}

// ---- G6: MODE S where the activation fits LDS next to everything else (<= 16 tokens, rows <= 4096 values), else MODE F (fragments
// fetched per item; 1 | 2 | 4 token tiles: the unit-sum table of all of a workgroup's tiles must fit LDS next to the waves' buffers) ----
static inline bool q80_gemm_plan_g6(const GemvArgs &a, Q80GemmPlan &p) {
    if (!q80_gemm_canon_shape(a)) return false;
    const uint32_t tt = q80_gemm_tt(a);
    // tile height: minimise the rows the busiest workgroup streams
    q80_gemm_row_tiles(a, p, [](uint32_t tpw, uint32_t bytes) { return tpw * bytes; });
    p.nu = (a.n / 64u + 7u) / 8u;
    // token tiles (tt = 1 | 2 | 4): SERIAL inside an item (an item's weights are transposed once and meet every tile), or -- small launches
    // whose (tile, unit) items leave waves idle: Qwen3-0.6B's matrices at 17..64 tokens -- SPREAD over the waves: an item is (tile, unit,
    // token tile), the weights of a (tile, unit) are fetched by up to four waves of the same workgroup (L1 / L2 hits on matrices of a few MB)
    // MEASURED (round 4, Qwen3-0.6B, one box): 32 sequences 1.347 ms spread vs 1.386 serial; 64 sequences 2.039 vs 1.888, prompt ingestion
    // of 64-token chunks 32.4 k vs 36.1 k tok/s -- four waves re-fetching and re-transposing an item's weights cost more than the idle waves
    // they fill.  So: spread two tiles, keep four serial.
    constexpr uint32_t spread_max = 2u;
    p.tts = (tt > 1u && tt <= spread_max && p.tpw * p.nu < G6_NW && p.tpw * p.nu * tt <= 4u * G6_NW) ? tt : 1u;
    const uint32_t items = p.tpw * p.nu * p.tts;
    p.nw = G6_NW;
    while (p.nw > items) p.nw >>= 1;                                   // a power of two (the kernel finds a tile's finisher with a mask)
    p.rounds = (items + p.nw - 1u) / p.nw;                             // the most items a wave owns
    const uint32_t ipt = p.nu * p.tts;
    p.magic = (65536u + ipt - 1u) / ipt;                               // (it * magic) >> 16 == it / ipt for every item index of a workgroup
    for (uint32_t it = 0; it < items + 8u * G6_NW; it++) if (((it * p.magic) >> 16) != it / ipt) return false;
    p.tt = (tt == 1u || p.tts > 1u) ? 1u : tt;                         // (spread token tiles: one tile per item)
    // (4 token tiles x 4 rounds is not instantiated: its registers spill; the launches that would need it -- Qwen3-4B's W1|W3 beyond 32
    //  tokens -- do not fit LDS either: G7 takes them)
    if (p.rounds > (p.tt == 4u ? 3u : 4u)) return false;
    // LDS: the waves' buffers | unit sums [tpw][nu][token tiles][256] | tile counters | (S: the activation, one 1 KB block per group + scales)
    const size_t common = (size_t)p.nw * G6_LDS_WAVE + (size_t)p.tpw * p.nu * tt * 1024u + (size_t)((p.tpw + 3u) & ~3u) * 4u;
    const size_t ngp = (size_t)p.nu * 8u, lds_s = common + ngp * 1024u + 64u + ngp * 64u + 64u;
    if (common + 64u > Q80_GEMM_LDS_MAX) return false;
    p.threads = p.nw * 64u;
    if (tt == 1u && p.nw == G6_NW && a.n <= 4096u && lds_s <= Q80_GEMM_LDS_MAX) {
        p.kernel = Q80_GEMM_G6S; p.lds_bytes = (uint32_t)lds_s;
        p.nv = a.n <= 2560u ? 5u : 8u;                                 // 16-byte units per thread: 5 (rows up to 2560 values) or 8 (up to 4096)
        p.r = p.rounds <= 2u ? p.rounds : 4u;
    } else {
        p.kernel = Q80_GEMM_G6F; p.lds_bytes = (uint32_t)(common + 64u);
        p.nv = 1u; p.r = p.rounds;
    }
    return true;
}

// ---- G7: 17..64 tokens, several row tiles per CU or very short rows ------------------------------------------------------------------
// Tile height.  At 17..64 tokens a launch is bound by the consumers' VALU work as much as by its bytes (measured, round 5: ~120 SIMD-cycles
// per matrix-core result of 16 rows x 16 tokens x one group -- cvt, two multiplies and an add per output -- i.e. ~0.23 us per row tile and
// step at four token tiles, where the tile's 16 x 256 B stream in ~0.18 us), and a tile costs that whatever its live rows: minimise
// (tiles per CU) x max(VALU, bytes), ties to the taller tile (Qwen3-4B's q|k|v: 384 tiles of 16 rows, 2 on the busiest CU, instead of G6's
// 768 tiles of 8 rows, 3 per CU).
static inline bool q80_gemm_plan_g7(const GemvArgs &a, Q80GemmPlan &p) {
    if (!q80_gemm_canon_shape(a) || a.nb < 17u) return false;
    p.ttl = q80_gemm_token_tiles(a);
    const uint32_t valu = 6u * p.ttl;
    q80_gemm_row_tiles(a, p, [valu](uint32_t tpw, uint32_t bytes) { return tpw * (valu > bytes ? valu : bytes); });
    p.nk = a.n / 256u;
    p.tp = p.tpw <= 1 ? 1u : p.tpw == 2 ? 2u : p.tpw == 3 ? 3u : p.tpw <= 5 ? 5u : p.tpw <= 8 ? 8u : 0u;
    if (!p.tp) return false;
    p.pp = 0;
    for (uint32_t pp = 1; pp <= 2u && !p.pp; pp *= 2u) if (p.tpw * ((p.ttl + pp - 1u) / pp) <= G7_NCW) p.pp = pp;
    if (!p.pp) return false;
    // LDS: the weight ring (a stage = the tiles' 16 rows x 256 B + their scales, one 1-KB DMA instruction per four tiles), then the two
    // fragment stages (token tiles x 4 KB + 1 KB of activation scales)
    p.a_ws = p.tpw * 4096u; p.a_stage = p.a_ws + ((p.tpw + 3u) / 4u) * 1024u;
    p.b_xs = ((p.ttl + p.pp - 1u) / p.pp) * p.pp * 4096u; p.b_stage = p.b_xs + 1024u;    // (token tiles rounded up to the waves' PP: a wave reads all of its PP)
    if (2u * p.b_stage + 1024u + 2u * p.a_stage > G7_LDS) return false;
    uint32_t nsa = (G7_LDS - 2u * p.b_stage - 1024u) / p.a_stage;
    // vmcnt is a 6-bit counter per wave: a loader's steps in flight behind the one it waits for (every second step is its own)
    const uint32_t ips = 4u * p.tpw + (p.tpw + 3u) / 4u;
    if (nsa > 1u + 2u * (63u / ips)) nsa = 1u + 2u * (63u / ips);
    if (nsa > G7_MAXNSA) nsa = G7_MAXNSA;
    if (nsa > p.nk + 1u) nsa = p.nk + 1u;
    if (nsa < 2u) return false;
    p.nsa = nsa;
    p.pre = nsa - 1u < p.nk ? nsa - 1u : p.nk;
    if (p.pre > 3u) p.pre = 3u;         // (2 / 3 / all nsa - 1 before the first barrier: 3.249 / 3.248 / 3.279 ms per 64-sequence Qwen3-4B step, one box, two runs each)
    p.b_base = nsa * p.a_stage;
    p.lds_bytes = p.b_base + 2u * p.b_stage + 1024u;                    // + the dummy kilobyte dead chunks are parked in
    // Where it pays (round 5, same-box A/B against G6 MODE F, profiles/r05_g7_stamps.txt): launches with several row tiles per CU
    // (q|k|v, W1|W3: one weight stage feeds 8..20 matrix-core pairs) and very short rows.  A launch of ONE row tile per CU and a long
    // row (Wo, W2 of Qwen3-4B: 16 / 38 steps of ~0.6 us with four of the fourteen consumer waves at work) stays with G7K / G6, whose
    // waves split the row length: 8.3 / 15.8 us there against 13.9 / 27.9 here.
    if (!(p.tpw * p.ttl >= 8u || p.nk <= 4u)) return false;
    p.kernel = Q80_GEMM_G7; p.threads = G7_NW * 64u;
    return true;
}

// ---- G7K: one row tile per CU and a long row, 3..48 tokens: the K-phase form --------------------------------------------------------
static inline bool q80_gemm_plan_g7k(const GemvArgs &a, Q80GemmPlan &p) {
    if (!q80_gemm_canon_shape(a) || a.nb < 3u || a.nseg != 1 || a.epi == GEMV_EPI_SWIGLU) return false;
    const uint32_t cus = a.cus ? a.cus : 256u, rows = a.seg[0].rows;
    p.hh = 0;
    // tile height: a workgroup's time does not depend on its live rows (a matrix-core tile and its VALU work cost the same): the lowest tile
    // that still gives every workgroup a CU of its own = the most CUs at work (Qwen3-0.6B's Wo / W2: 256 workgroups of 4 rows instead of 64 of 16:
    // 1.437 -> 1.413 ms per 64-sequence step; Qwen3-4B's: 256 of 10 rows instead of 160 of 16: 3.215 -> 3.19)
    for (uint32_t hh = 1; hh <= 8 && !p.hh; hh++) if ((rows + 2u * hh - 1u) / (2u * hh) <= cus) p.hh = hh;
    if (!p.hh) return false;
    p.ntiles = p.grid = (rows + 2u * p.hh - 1u) / (2u * p.hh);
    p.nk = a.n / 256u; p.nu = (p.nk + 1u) / 2u; p.ttl = q80_gemm_token_tiles(a);
    if (p.nk < 8u) return false;                                       // short rows: G7 / G6
    // Where it pays (same-box A/Bs against G6 MODE F, profiles/r06_g7k.txt): up to three token tiles.  Qwen3-0.6B at 32 sequences 1.253 ->
    // 1.18-1.23 ms per step, Qwen3-4B at 48: 3.012 -> 2.981, at 32: even; with FOUR token tiles (49..64 tokens) it LOSES: Qwen3-4B at 64
    // sequences 3.127 -> 3.19 ms, Qwen3-0.6B even -- both kernels then sit at the same ~0.1 us per (16 rows x 16 tokens x 256 B) of a CU.
    if (p.ttl > 3u) return false;
    // (3..16 tokens, round 6: Qwen3-0.6B at 16 sequences 1.068 -> 1.016 ms per step, Qwen3-4B at 4 / 8 / 16: -0.9 % each; the loaders are the
    //  waves the consumers leave, up to six -- at 32..48 tokens four loaders instead of two changed nothing)
    // phases: as many as the fourteen consumer waves and the ring + table allow
    // the ring comes first: THREE super-steps (the weights of super-step s + 2 go out at barrier s; with two, every super-step pays a DMA issue
    // + an HBM round trip -- Qwen3-4B at 64 sequences 3.24-3.27 ms against 3.195-3.215), then as many phases as still fit; two only when no
    // phase count leaves room for three (the most phases first, the ring second, measured 0.6-0.8 % slower on Qwen3-4B at 8 / 16 / 32 sequences)
    const uint32_t ks_max = G7_NCW / p.ttl < 6u ? G7_NCW / p.ttl : 6u;
    auto fits = [&](uint32_t ks, uint32_t rg) {
        const uint32_t nl = G7_NW - ks * p.ttl < 6u ? G7_NW - ks * p.ttl : 6u;     // the waves the consumers leave load
        const size_t ring = (size_t)rg * 2u * ks * G7K_STAGE, tab = (size_t)p.nu * p.ttl * 1024u;
        if (ks > p.nu || ring + tab > G7_LDS) return false;
        if (rg * ((2u * ks + nl - 1u) / nl) * 5u > 60u) return false;  // a loader's instructions in flight (ring super-steps x its steps x <= 5) fit vmcnt's six bits
        p.ks = ks; p.ncw = ks * p.ttl; p.nss = (p.nu + ks - 1u) / ks; p.ring = rg; p.nl = nl;
        p.tab = (uint32_t)ring; p.lds_bytes = (uint32_t)(ring + tab);
        return true;
    };
    for (uint32_t rg = 3u; rg >= 2u; rg--) for (uint32_t ks = ks_max; ks >= 2u; ks--) if (fits(ks, rg)) {
        p.kernel = Q80_GEMM_G7K; p.threads = (p.ncw + p.nl) * 64u;
        return true;
    }
    return false;
}

// ---- GC: tall matrices with short rows (the classifier of a batched step), the reference's order -----------------------------------
static inline bool q80_gemm_plan_gc(const GemvArgs &a, Q80GemmPlan &p) {
    if (a.gs != 64 || a.nseg != 1 || a.epi != GEMV_EPI_STORE || a.seg[0].out_pstride != 0 || a.attn_part || a.resid_add) return false;
    if (a.nb < 2 || a.nb > 64 || a.n % 64 || (a.n / 64) % 4 != 0 || a.n > 8192) return false;
    if (a.seg[0].rows < 16384 || (a.seg[0].out_bstride % 4) != 0) return false;          // tall matrices; 16-byte output stores
    if ((uint64_t)a.seg[0].rows * a.n >= (1ull << 32) - (1u << 20)) return false;         // 32-bit buffer offsets
    p.ng = a.n / 64; p.nhc = (p.ng + 7) / 8; p.ntiles = (a.seg[0].rows + 15) / 16; p.ttl = q80_gemm_token_tiles(a);
    // waves per workgroup (one workgroup per CU): as many as leave room to stage every token tile, or at least two of them (the
    // kernel keeps at most two unstaged tiles in registers: tiles 2 and 3)
    const size_t tile_lds = (size_t)p.ng * 1088u;
    uint32_t waves = 8, lt = 0;
    for (; waves >= 4; waves -= 2) {
        const size_t room = Q80_GEMM_LDS_MAX - (size_t)waves * GC_LDS_WAVE - 256u;
        lt = (uint32_t)(room / tile_lds);
        if (lt > p.ttl) lt = p.ttl;
        if (lt == p.ttl || (lt >= 2 && p.ttl - lt <= 2)) break;
    }
    if (waves < 4) return false;                                        // not even four waves next to the tiles that must be staged
    if (lt < p.ttl) lt = 2;
    p.kernel = Q80_GEMM_GC; p.tt = q80_gemm_tt(a);
    p.waves = waves; p.lt = lt;
    p.grid = a.cus ? a.cus : 256u;                                      // one persistent workgroup per CU
    p.nwaves = p.grid * waves; p.threads = waves * 64u;
    p.lds_bytes = (uint32_t)((size_t)lt * tile_lds + (size_t)waves * GC_LDS_WAVE + 64u);
    return true;
}

// ---- G2: the general kernel in the reference's order (any group size 32..256, any group count) --------------------------------------
// Not taken: interior segments that are not multiples of the 16-row tile, a split-attention input, the LoRA o-branch addend, and the
// launches whose stages, weight scales and product tables do not fit a CU's LDS -- group size 32: SwiGLU at 17..64 tokens always and at
// 1..16 tokens from rows of 15104 values on, STORE / residual at 33..64 tokens from rows of 6912 values on (17..32: 39680, 1..16: 56064);
// group size 64: SwiGLU at 17..64 tokens from rows of ~31000 values on; group sizes 128 / 256: never up to 65536 values.  What it does
// not take goes through the GEMV kernels in groups of up to 8 sequences (route.hip).
static inline bool q80_gemm_plan_g2(const GemvArgs &a, Q80GemmPlan &p) {
    if (a.nb == 0 || a.nb > 64 || a.gs == 0 || a.n % a.gs || a.n % 16 || a.nseg == 0 || a.nseg > 3 || a.attn_part || a.resid_add) return false;
    if (!(a.gs == 32 || a.gs == 64 || a.gs == 128 || a.gs == 256)) return false;
    const bool sw = a.epi == GEMV_EPI_SWIGLU;
    if (!sw && a.nseg > 1)
        for (uint32_t s = 0; s + 1 < a.nseg; s++) if (a.seg[s].rows % 16) return false;     // a 16-row tile stays inside one segment
    p.ng = a.n / a.gs;
    p.magic = ((1u << 20) + p.ng - 1) / p.ng;
    for (uint32_t e = 0; e < 16 * p.ng + 4096; e++) if (((e * p.magic) >> 20) != e / p.ng) return false;
    p.gs = a.gs; p.sw = sw ? 1u : 0u; p.tt = q80_gemm_tt(a);
    // LDS: two weight stages [matrices][16 rows][pitch] | weight scales [matrices][16][ng | 1] | the product tables
    // [matrices][groups of a pass][16 rows][16 TT + 1 tokens] -- two of them (the pipelined form) except SwiGLU at four token tiles
    const uint32_t gpp = G2_PK / a.gs, nmat = sw ? 2u : 1u, ntp = 16u * p.tt + 1u, tables = (p.tt == 4u && sw) ? 1u : 2u;
    const size_t lds = (size_t)2 * nmat * 16 * G2_PITCH + (size_t)nmat * 16 * (p.ng | 1u) * 4 + (size_t)tables * nmat * gpp * 16 * ntp * 4;
    if (lds > Q80_GEMM_LDS_MAX) return false;
    p.kernel = Q80_GEMM_G2; p.lds_bytes = (uint32_t)lds;
    p.npass = (a.n + G2_PK - 1) / G2_PK;
    p.grid = (gemv_total_rows(a) + 15) / 16; p.threads = 512u;
    return true;
}

// the launchers: a.xq_in / a.xs_in = the activations in fragment order (launch_quant_rows_frag); they take every choice from the plan
hipError_t launch_gemm_q80_g6(const GemvArgs &a, const Q80GemmPlan &p, hipStream_t st);     // G6S, G6F
hipError_t launch_gemm_q80_g7(const GemvArgs &a, const Q80GemmPlan &p, hipStream_t st);     // G7, G7K
hipError_t launch_gemm_q80_cls(const GemvArgs &a, const Q80GemmPlan &p, hipStream_t st);    // GC
hipError_t launch_gemm_q80_g2(const GemvArgs &a, const Q80GemmPlan &p, hipStream_t st);     // G2

}  // namespace nano
