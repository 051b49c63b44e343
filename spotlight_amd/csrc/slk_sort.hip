// slk_sort.hip -- the engine's own stable LSD radix sort for gfx950 (round 4: replaces rocPRIM's radix_sort_pairs, the one
// library kernel that was on the training path).
//
// What the row-owner passes need (slk_bilinear.hip, slk_seq.hip): interactions grouped by (minibatch, user) and occurrences
// grouped by (minibatch, item), every group in position order -- the sparse-gradient coalesce of the reference's
// `loss.backward(); optimizer.step()` (spotlight/factorization/implicit.py:242-243), made deterministic.  Three things a
// general-purpose library sort cannot know are used here:
//   * the minibatch is implied by the position (minibatch m = positions [m B, (m+1) B)), so its bits are never sorted: the
//     sort is SEGMENTED -- every minibatch of a chunk is sorted on the id bits only, all of them in the same launches
//     (C2: 24 bits = 3 passes instead of 27 = 4; 20 bits instead of 23 on the item side);
//   * the keys do not exist yet: the first pass builds them from the id arrays it reads anyway (k_build_user_keys /
//     k_build_item_keys are gone: one write and one read of every key and payload less);
//   * digits are split evenly (20 bits = 7 + 7 + 6, not 8 + 8 + 4): fewer buckets per pass = longer runs per (tile, bucket),
//     and the scatter's partial-line writes are what a radix pass pays for.
//
// Structure of one sort of n pairs in P passes: ONE histogram kernel (every pass's digit counts per segment, LDS atomics) ->
// ONE scan kernel (bucket bases) -> P scatter kernels.  A scatter workgroup takes a tile (ticket = dependency order), ranks
// its keys with wave-wide digit matches (ballots; stable by construction: element order = wave, round, lane), publishes the
// tile's digit counts and finds the counts of the tiles before it by decoupled look-back over one 32-bit {flag, count} word per
// (tile, digit) (sc1 stores / loads: the producer may sit on another XCD), exchanges keys then payloads through LDS so that
// every (tile, bucket) run leaves as consecutive lanes, and writes.  HBM-bound: 8 B (u32 payload) / 12 B (u64) read + written
// per pair and pass, + 4 B for the histogram.
//
// A second route, for the training prep's large segmented sorts of u32 keys (segments of >= RS_FIN_MIN_SEG pairs, more than 8
// key bits): TWO global passes instead of three.  A per-tile count of the TOP digit (k_rs_tile_hist), a prefix over each
// segment's tiles (k_rs_tile_scan, k_rs_bucket_base), ONE scatter on the top digit that reads "pairs before this tile" from that
// table (k_rs_scatter<TOP>: no ticket, no status word, no look-back), then one workgroup per (segment, bucket) sorts its bucket
// on the remaining bits in registers + LDS and writes it out in full lines (k_rs_finish).  The top digit's width is chosen on
// the host from the segment length and the id range (rs_pick_topw) so that a bucket stays under RS_FIN_CAP pairs; whether every
// bucket did is decided on the device (`nofit`): if not -- skewed ids -- these kernels return at once and the LSD kernels, always
// enqueued behind them, sort; otherwise those return at once.  Nothing on this route waits for another workgroup.
#include <math.h>

#include "slk_common.h"

namespace {

constexpr int RS_RB = 8;                  // widest digit
constexpr int RS_RADIX = 1 << RS_RB;
constexpr uint32_t RS_VAL_MASK = (1u << 30) - 1u;  // status word: flag << 30 | count (segments hold < 2^30 pairs)
constexpr uint32_t RS_AGG = 1u, RS_INC = 2u;
constexpr int RS_MAX_PASS = 8;
constexpr int RS_HIST_KEYS = 8192;        // keys per histogram workgroup
constexpr int RS_LBW = 16;                // look-back: status words in flight per digit and round trip
constexpr uint32_t RS_MAX_SPINS = 1u << 22;  // x (s_sleep + one fabric round trip): seconds; then the sort gives up (sticky flag)

enum { RS_LOAD_PLAIN = 0, RS_LOAD_USER_FAT, RS_LOAD_USER_IDX, RS_LOAD_ITEM_OCC, RS_LOAD_FY_STEPS };

struct rs_args {
    const void *kin, *vin;
    void *kout, *vout;
    // sources of the fused first pass (the training prep, slk_bilinear.hip)
    const int64_t *users, *items;
    const uint32_t *neg32, *uit;
    uint32_t n, seg_len, tps, ntiles, hbps;  // pairs, pairs per segment, tiles / histogram workgroups per segment
    uint32_t kseg;                           // fused keys of an UNSEGMENTED sort: pairs per minibatch (0: the segment is the minibatch)
    unsigned idbits;                         // fused keys: (minibatch << idbits) | id
    uint32_t fy_n;                           // RS_LOAD_FY_STEPS: elements of the shuffle (slk_shuffle.hip)
    int npass, pass;
    int shift[RS_MAX_PASS], width[RS_MAX_PASS];
    uint32_t *hist, *base;   // [segment][pass][RS_RADIX]: digit counts / first output position of the bucket
    uint32_t *ticket;        // [pass]
    uint32_t *status;        // this pass: [tile][1 << width]
    int32_t *abort_flag;     // sticky (slk_rng_dev::sort_abort): a look-back gave up
    int xcd;                 // 1: a segment's tiles are taken by the workgroups of ONE XCD (segment s -> XCD s % 8)
    uint32_t nseg;
    int debug;               // measurement only (option "sort_debug"): 1 no look-back walk, 2 ranks from LDS atomics
    // the top-digit route (below): one scatter on the key bits [topshift, topshift + topw), then a finish per bucket
    int topw, topshift;
    uint32_t *tpre;          // [tile][1 << topw]: the tile's top-digit counts, then those of the segment's tiles before it
    uint32_t *btot, *bbase;  // [segment][RS_RADIX]: pairs of the bucket / its first output position
    uint32_t *nofit;         // one word per sort: != 0 when a bucket holds more than RS_FIN_CAP pairs (the LSD passes run instead)
    uint32_t *fallbacks;     // slk_rng_dev::sort_fallbacks: sorts whose nofit came out != 0
    int gate;                // LSD kernels enqueued behind the top-digit route: return at once unless *nofit
};

template <class KeyT>
__device__ __forceinline__ uint32_t rs_digit(KeyT k, int shift, uint32_t mask) {
    return (uint32_t)(k >> shift) & mask;
}

// element gi of the sort's input: (key, payload)
template <class KeyT, class ValT, int LOADER>
__device__ __forceinline__ void rs_load(const rs_args &a, uint32_t gi, uint32_t seg, KeyT &k, ValT &v) {
    if (LOADER == RS_LOAD_FY_STEPS) {
        // the epoch shuffle's swaps (slk_shuffle.hip): step g (i = n - 1 - g) writes position j = J[g]: key = j, value = i;
        // a step that swaps with itself gets the sentinel key n
        const uint32_t i = a.fy_n - 1u - gi, j = a.uit[gi];
        k = (KeyT)(j == i ? a.fy_n : j);
        v = (ValT)i;
        return;
    }
    if (LOADER != RS_LOAD_PLAIN && a.kseg) seg = gi / a.kseg;
    if (LOADER == RS_LOAD_PLAIN) {
        k = ((const KeyT *)a.kin)[gi];
        v = ((const ValT *)a.vin)[gi];
    } else if (LOADER == RS_LOAD_USER_FAT) {
        // key = (minibatch-in-chunk, user); payload = the (positive, negative) item pair the user pass reads with the key
        k = (KeyT)((seg << a.idbits) | (uint32_t)a.users[gi]);
        v = (ValT)(((uint64_t)a.neg32[gi] << 32) | (uint64_t)(uint32_t)a.items[gi]);
    } else if (LOADER == RS_LOAD_USER_IDX) {
        k = (KeyT)((seg << a.idbits) | (uint32_t)a.users[gi]);
        v = (ValT)gi;
    } else {
        // occurrence r = (user-sorted position q, slot) of the packed item list: key = (minibatch, item), payload = r
        k = (KeyT)((seg << a.idbits) | a.uit[gi]);
        v = (ValT)gi;
    }
}

template <class KeyT, int LOADER>
__device__ __forceinline__ KeyT rs_load_key(const rs_args &a, uint32_t gi, uint32_t seg) {
    if (LOADER == RS_LOAD_PLAIN) return ((const KeyT *)a.kin)[gi];
    if (LOADER == RS_LOAD_FY_STEPS) {
        const uint32_t j = a.uit[gi];
        return (KeyT)(j == a.fy_n - 1u - gi ? a.fy_n : j);
    }
    if (a.kseg) seg = gi / a.kseg;
    if (LOADER == RS_LOAD_ITEM_OCC) return (KeyT)((seg << a.idbits) | a.uit[gi]);
    return (KeyT)((seg << a.idbits) | (uint32_t)a.users[gi]);
}

// ---- digit counts of every pass, per segment ------------------------------------------------------------------------------
template <class KeyT, int LOADER>
__global__ __launch_bounds__(256) void k_rs_hist(rs_args a) {
    __shared__ uint32_t sh[RS_MAX_PASS * RS_RADIX];
    if (a.gate && !*a.nofit) return;  // (the top-digit route sorted it)
    const uint32_t seg = blockIdx.x / a.hbps, hb = blockIdx.x - seg * a.hbps;
    const uint32_t s0 = seg * a.seg_len;
    const uint32_t s1 = (a.n - s0 < a.seg_len) ? a.n : s0 + a.seg_len;
    const uint32_t b0 = s0 + hb * (uint32_t)RS_HIST_KEYS;
    const uint32_t b1 = (b0 >= s1 || s1 - b0 < (uint32_t)RS_HIST_KEYS) ? s1 : b0 + (uint32_t)RS_HIST_KEYS;  // (a short last segment)
    for (int i = threadIdx.x; i < a.npass * RS_RADIX; i += 256) sh[i] = 0u;
    __syncthreads();
    // eight keys per thread in flight (the kernel is otherwise one dependent load -> LDS-atomics chain per key)
    for (uint32_t g0 = b0 + threadIdx.x; g0 < b1; g0 += 8u * 256u) {
        KeyT k[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t gi = g0 + (uint32_t)u * 256u;
            k[u] = gi < b1 ? rs_load_key<KeyT, LOADER>(a, gi, seg) : (KeyT)0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (g0 + (uint32_t)u * 256u >= b1) continue;
            for (int p = 0; p < a.npass; ++p)
                atomicAdd(&sh[p * RS_RADIX + rs_digit<KeyT>(k[u], a.shift[p], (1u << a.width[p]) - 1u)], 1u);
        }
    }
    __syncthreads();
    uint32_t *gh = a.hist + (size_t)seg * a.npass * RS_RADIX;
    for (int i = threadIdx.x; i < a.npass * RS_RADIX; i += 256) {
        const uint32_t c = sh[i];
        if (c) atomicAdd(&gh[i], c);
    }
}

// exclusive scan of one value per thread over the workgroup (THREADS a multiple of 64)
template <int THREADS>
__device__ __forceinline__ uint32_t rs_block_excl_scan(uint32_t v, uint32_t *s_wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_wsum[w] = inc;
    __syncthreads();
    uint32_t off = 0;
    for (int i = 0; i < THREADS / 64; ++i)
        if (i < w) off += s_wsum[i];
    __syncthreads();
    return off + inc - v;
}

// bucket bases: base[segment][pass][d] = segment start + (pairs of the segment whose digit is < d)
__global__ __launch_bounds__(256) void k_rs_scan(rs_args a) {
    __shared__ uint32_t s_wsum[4];
    if (a.gate && !*a.nofit) return;
    const uint32_t seg = blockIdx.x / (uint32_t)a.npass;
    const size_t o = (size_t)blockIdx.x * RS_RADIX + threadIdx.x;
    const uint32_t c = a.hist[o];
    a.base[o] = seg * a.seg_len + rs_block_excl_scan<256>(c, s_wsum);
}

// the XCD this workgroup runs on (0..7)
__device__ __forceinline__ uint32_t rs_xcc_id() {
#if defined(__HIPCC__)
    return (uint32_t)__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;  // HW_REG_XCC_ID[3:0]
#else
    return blockIdx.x & 7u;
#endif
}

// lanes of the wave that hold the same digit as this one (valid lanes only)
__device__ __forceinline__ unsigned long long rs_match(uint32_t d, int nbits, bool valid) {
    unsigned long long m = __ballot(valid);
    for (int b = 0; b < nbits; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return valid ? m : 0ull;
}

// ---- one pass: tile -> ranks -> look-back -> LDS exchange -> scatter ----------------------------------------------------------
// The counts of the segment's tiles before this one, for digit d: RS_LBW status words per round trip, back to the nearest tile
// that knows its own inclusive count.  Returns false when a tile never published (the sort gives up: sticky flag).
__device__ __forceinline__ bool rs_walk(const rs_args &a, const uint32_t *row0, uint32_t radix, uint32_t tis, uint32_t &before) {
    int32_t t = (int32_t)tis - 1;
    uint32_t spins = 0;
    bool done = false;
    while (!done) {
        uint32_t v[RS_LBW];
#pragma unroll
        for (int i = 0; i < RS_LBW; ++i) {
            const int32_t ti = t - i;
            v[i] = ti >= 0 ? __hip_atomic_load(row0 + (size_t)ti * radix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        }
        int consumed = 0;
#pragma unroll
        for (int i = 0; i < RS_LBW; ++i) {
            const uint32_t f = v[i] >> 30;
            if (done || f == 0u || consumed != i) continue;
            before += v[i] & RS_VAL_MASK;
            ++consumed;
            if (f == RS_INC) done = true;
        }
        t -= consumed;
        if (!done && consumed == 0) {
            if (++spins > RS_MAX_SPINS) {  // a tile before this one never published: give up, loudly
                *a.abort_flag = 1;
                return false;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    return true;
}

// SINGLE: the whole input is one tile (no histogram, no look-back: bucket bases are the tile's own scan).
// (A dedicated WALKER wave -- the workgroup's last wave holds no keys, publishes the counts, walks back with four digits per
// lane and forms the bucket offsets while the other seven rank -- was built and measured in round 4: 0.235 / 0.314 ms against
// 0.227 / 0.304 ms for the C2 user / item sorts without it, profiles/r04_l_*.  The walk of the FIRST wave of tiles is a chain
// through the tiles before them whoever walks it; the tiles behind find inclusive counts at once.  Removed.)
// TOP: the top-digit route's scatter (below): the tile is the workgroup's index and the counts of the tiles before it come from
// the table k_rs_tile_scan wrote -- no ticket, no status word, no look-back.
template <class KeyT, class ValT, int THREADS, int KPT, int LOADER, bool SINGLE, bool TOP = false>
__global__ __launch_bounds__(THREADS) SLK_WAVES_PER_EU_RANGE(4, 6) void k_rs_scatter(rs_args a) {
    constexpr int WAVES = THREADS / 64, KW = WAVES, TILE = KW * 64 * KPT;
    constexpr int OPT = (TILE + THREADS - 1) / THREADS;  // output positions per thread
    constexpr int XB = sizeof(KeyT) > sizeof(ValT) ? sizeof(KeyT) : sizeof(ValT);
    __shared__ uint32_t s_cnt[KW * RS_RADIX];     // per key wave: running digit counts, then the wave's first rank in the tile's bucket
    __shared__ uint32_t s_lbase[RS_RADIX];        // the tile's digit counts, then the first position of the bucket in the tile's sorted order
    __shared__ uint32_t s_goff[RS_RADIX];         // output index of the bucket's element at tile position i = s_goff + i
    __shared__ uint32_t s_wsum[WAVES];
    __shared__ uint32_t s_tile;
    __shared__ __attribute__((aligned(16))) unsigned char s_x[(size_t)TILE * XB];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr bool is_key = true;  // (every wave holds keys)
    if (TOP) {
        if (*a.nofit) return;
    } else if (!SINGLE && a.gate && !*a.nofit) {
        return;
    }
    const int shift = TOP ? a.topshift : a.shift[a.pass], nbits = TOP ? a.topw : a.width[a.pass];
    const uint32_t radix = 1u << nbits, dmask = radix - 1u;
    if (!SINGLE && !TOP && threadIdx.x == 0) {
        if (a.xcd) {
            // Segment s belongs to XCD s % 8: its tiles' runs meet in ONE L2 (adjacent tiles complete each other's partial lines
            // before they are written back) and its look-back words never cross the fabric.  A workgroup whose XCD has run out
            // of tiles takes one of the next XCD's (the grid has exactly one workgroup per tile, so every tile is taken); the
            // order of the tickets of one XCD is still the order of the dependency chain of its segments.
            const uint32_t x0 = rs_xcc_id();
            uint32_t t = 0xffffffffu;
            for (uint32_t i = 0; i < 8u && t == 0xffffffffu; ++i) {
                const uint32_t x = (x0 + i) & 7u;
                const uint32_t nsx = a.nseg > x ? (a.nseg - x + 7u) / 8u : 0u;
                if (!nsx) continue;
                const uint32_t k = atomicAdd(a.ticket + 8 + a.pass * 8 + x, 1u);
                if (k < nsx * a.tps) t = (x + 8u * (k / a.tps)) * a.tps + k % a.tps;
            }
            s_tile = t;
        } else {
            s_tile = atomicAdd(a.ticket + a.pass, 1u);
        }
    }
    for (int i = threadIdx.x; i < KW * RS_RADIX; i += THREADS) s_cnt[i] = 0u;
    if (threadIdx.x < RS_RADIX) s_lbase[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t tile = SINGLE ? 0u : (TOP ? blockIdx.x : s_tile);
    if (tile == 0xffffffffu) return;  // (cannot happen: one workgroup per tile)
    const uint32_t seg = tile / a.tps, tis = tile - seg * a.tps;
    const uint32_t s0 = seg * a.seg_len;
    const uint32_t s1 = (a.n - s0 < a.seg_len) ? a.n : s0 + a.seg_len;
    const uint32_t t0 = s0 + tis * (uint32_t)TILE;
    const uint32_t cnt = t0 >= s1 ? 0u : ((s1 - t0 < (uint32_t)TILE) ? s1 - t0 : (uint32_t)TILE);  // (0: a tile past a short last segment)

    KeyT key[KPT];
    ValT val[KPT];
    uint32_t pos2[KPT / 2];  // tile positions (< 2^16), two per register
    const uint32_t e0 = (uint32_t)wave * 64u * KPT + (uint32_t)lane;
    if (is_key) {
        // every key load first, then every payload load: the keys are waited for alone, the payloads land behind the ranking
        if (LOADER == RS_LOAD_PLAIN) {
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const uint32_t e = e0 + (uint32_t)j * 64u;
                key[j] = e < cnt ? ((const KeyT *)a.kin)[t0 + e] : (KeyT)0;
            }
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const uint32_t e = e0 + (uint32_t)j * 64u;
                val[j] = e < cnt ? ((const ValT *)a.vin)[t0 + e] : (ValT)0;
            }
        } else {
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const uint32_t e = e0 + (uint32_t)j * 64u;
                key[j] = 0;
                val[j] = 0;
                if (e < cnt) rs_load<KeyT, ValT, LOADER>(a, t0 + e, seg, key[j], val[j]);
            }
        }
        // the tile's digit counts: published BEFORE the ranking, so the tiles behind this one add them up while it ranks
        if (!SINGLE && !TOP) {
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                if (e0 + (uint32_t)j * 64u < cnt) atomicAdd(&s_lbase[rs_digit<KeyT>(key[j], shift, dmask)], 1u);
        }
    } else {
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            key[j] = 0;
            val[j] = 0;
        }
    }
    if (!SINGLE && !TOP) __syncthreads();

    uint32_t tcount = 0, before = 0;
    uint32_t *wcnt = s_cnt + (is_key ? wave : 0) * RS_RADIX;
    auto rank_keys = [&]() {
        // ranks inside the wave's 64 * KPT elements, in element order (round j, then lane)
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            if ((j & 1) == 0) pos2[j / 2] = 0u;
            if ((uint32_t)wave * 64u * KPT + (uint32_t)j * 64u >= cnt) continue;  // (wave-uniform: a round past the tile's end)
            const bool valid = e0 + (uint32_t)j * 64u < cnt;
            const uint32_t dj = rs_digit<KeyT>(key[j], shift, dmask);
            uint32_t r;
            if (a.debug & 2) {  // measurement only: ranks from LDS atomics (unstable order)
                r = valid ? atomicAdd(&wcnt[dj], 1u) : 0u;
            } else {
                const unsigned long long m = rs_match(dj, nbits, valid);
                const int leader = m ? __ffsll((long long)m) - 1 : lane;
                uint32_t first = 0;
                if (m && lane == leader) first = atomicAdd(&wcnt[dj], (uint32_t)__popcll(m));
                first = __shfl(first, leader);
                r = first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            }
            pos2[j / 2] = (j & 1) ? (pos2[j / 2] | (r << 16)) : r;
        }
    };
    {
        const uint32_t d = threadIdx.x;
        if (TOP && d < radix) before = a.tpre[(size_t)tile * radix + d];
        if (!SINGLE && !TOP && d < radix) {
            tcount = s_lbase[d];
            __hip_atomic_store(a.status + (size_t)tile * radix + d, ((tis == 0 ? RS_INC : RS_AGG) << 30) | tcount, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            // the digit owners (the first `radix` threads) walk back NOW, before they rank: the workgroup's other waves -- and
            // the other workgroups of the CU -- rank meanwhile
            if (tis != 0 && !(a.debug & 1)) {
                rs_walk(a, a.status + (size_t)(tile - tis) * radix + d, radix, tis, before);
                __hip_atomic_store(a.status + (size_t)tile * radix + d, (RS_INC << 30) | ((before + tcount) & RS_VAL_MASK), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        rank_keys();
        __syncthreads();
        // per digit: waves' counts -> the wave's first rank in the tile's bucket
        if (d < radix) {
            uint32_t run = 0;
            for (int w = 0; w < KW; ++w) {
                const uint32_t c = s_cnt[w * RS_RADIX + d];
                s_cnt[w * RS_RADIX + d] = run;
                run += c;
            }
            if (SINGLE || TOP) tcount = run;
        }
        const uint32_t lb = rs_block_excl_scan<THREADS>(tcount, s_wsum);
        if (d < radix) {
            uint32_t gbase = lb;
            if (TOP) gbase = a.bbase[(size_t)seg * RS_RADIX + d];
            else if (!SINGLE) gbase = a.base[((size_t)seg * a.npass + a.pass) * RS_RADIX + d];
            s_lbase[d] = lb;
            s_goff[d] = gbase + before - lb;
        }
    }
    __syncthreads();
    // keys through LDS into the tile's sorted order, then out: thread i takes tile positions i, i + THREADS, ...
    KeyT *xk = reinterpret_cast<KeyT *>(s_x);
    if (is_key) {
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            if (e0 + (uint32_t)j * 64u < cnt) {
                const uint32_t dj = rs_digit<KeyT>(key[j], shift, dmask);
                const uint32_t pj = ((pos2[j / 2] >> ((j & 1) * 16)) & 0xffffu) + s_lbase[dj] + wcnt[dj];
                pos2[j / 2] = (j & 1) ? ((pos2[j / 2] & 0xffffu) | (pj << 16)) : ((pos2[j / 2] & 0xffff0000u) | pj);
                xk[pj] = key[j];
            }
        }
    }
    __syncthreads();
    uint32_t gidx[OPT];
#pragma unroll
    for (int j = 0; j < OPT; ++j) {
        const uint32_t i = (uint32_t)j * THREADS + threadIdx.x;
        gidx[j] = 0;
        if (i < cnt) {
            const KeyT k = xk[i];
            gidx[j] = s_goff[rs_digit<KeyT>(k, shift, dmask)] + i;
            ((KeyT *)a.kout)[gidx[j]] = k;
        }
    }
    __syncthreads();
    ValT *xv = reinterpret_cast<ValT *>(s_x);
    if (is_key) {
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if (e0 + (uint32_t)j * 64u < cnt) xv[(pos2[j / 2] >> ((j & 1) * 16)) & 0xffffu] = val[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < OPT; ++j) {
        const uint32_t i = (uint32_t)j * THREADS + threadIdx.x;
        if (i < cnt) ((ValT *)a.vout)[gidx[j]] = xv[i];
    }
}

// ---- the top-digit route: ONE global scatter on the top `topw` key bits, then every bucket is finished inside one workgroup ----
// For the segmented sorts of u32 keys (the training prep): two global passes instead of three, and nothing in them waits for
// another workgroup.  k_rs_tile_hist counts the top digit per scatter tile -> k_rs_tile_scan turns the counts into "pairs of the
// segment's tiles before this one" -> k_rs_bucket_base forms the bucket bases and the word `nofit` -> k_rs_scatter<TOP> ->
// k_rs_finish.  A bucket of more than RS_FIN_CAP pairs (skewed ids) raises `nofit`: scatter and finish return at once and the
// LSD kernels enqueued behind them do the sort; otherwise those return at once.  The host never reads `nofit`.

// the finish's workgroup: capacity RS_FIN_CAP = threads x keys per thread (9216: the C2 item side's buckets hold 8559 + 6 sigma)
#ifndef RS_FIN_THREADS
#define RS_FIN_THREADS 512
#endif
#ifndef RS_FIN_KPT
#define RS_FIN_KPT 18
#endif
// Segments shorter than this keep the LSD passes: measured (profiles/r07_a_sort_sweep.md), the route wins at segments of 2^20 /
// 2^21 pairs, is even at 2^18 and loses at 2^16, where the digit that keeps a bucket under the capacity is narrow and the finish
// needs three local rounds.  The test hook "sort_big_min" lowers the gate with the tile threshold: min(this, sort_big_min).
#ifndef RS_FIN_MIN_SEG
#define RS_FIN_MIN_SEG (1 << 20)
#endif
constexpr uint32_t RS_FIN_CAP = (uint32_t)RS_FIN_THREADS * RS_FIN_KPT;
static_assert(RS_FIN_KPT % 2 == 0 && RS_FIN_THREADS % 64 == 0 && RS_FIN_THREADS >= RS_RADIX && RS_FIN_CAP <= 65536u, "finish tile shape");

// the top digit's counts of one scatter tile, written plainly to tpre[tile][1 << topw]
template <class KeyT, int LOADER, int THREADS, int KPT>
__global__ __launch_bounds__(THREADS) void k_rs_tile_hist(rs_args a) {
    constexpr uint32_t TILE = (uint32_t)THREADS * KPT;
    __shared__ uint32_t sh[RS_RADIX];
    const uint32_t tile = blockIdx.x, seg = tile / a.tps, tis = tile - seg * a.tps;
    const uint32_t s0 = seg * a.seg_len;
    const uint32_t s1 = (a.n - s0 < a.seg_len) ? a.n : s0 + a.seg_len;
    const uint32_t t0 = s0 + tis * TILE;
    const uint32_t cnt = t0 >= s1 ? 0u : ((s1 - t0 < TILE) ? s1 - t0 : TILE);
    const uint32_t radix = 1u << a.topw, dmask = radix - 1u;
    for (uint32_t i = threadIdx.x; i < radix; i += THREADS) sh[i] = 0u;
    __syncthreads();
    KeyT k[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const uint32_t e = (uint32_t)j * THREADS + threadIdx.x;
        k[j] = e < cnt ? rs_load_key<KeyT, LOADER>(a, t0 + e, seg) : (KeyT)0;
    }
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if ((uint32_t)j * THREADS + threadIdx.x < cnt) atomicAdd(&sh[rs_digit<KeyT>(k[j], a.topshift, dmask)], 1u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < radix; i += THREADS) a.tpre[(size_t)tile * radix + i] = sh[i];
}

// per (segment, digit): tpre[tile][d] -> pairs with digit d in the segment's tiles before `tile`; btot[segment][d] = the bucket's
// size.  One workgroup per (segment, 32 digits): 32 lanes read one 128-byte line of a tile's row, 8 such groups share the tiles.
__global__ __launch_bounds__(256) void k_rs_tile_scan(rs_args a) {
    __shared__ uint32_t s_part[256];
    const uint32_t radix = 1u << a.topw;
    const uint32_t dg = radix < 32u ? radix : 32u, ngr = radix / dg, parts = 256u / dg;
    const uint32_t seg = blockIdx.x / ngr, dl = threadIdx.x % dg, part = threadIdx.x / dg;
    const uint32_t d = (blockIdx.x - seg * ngr) * dg + dl;
    const uint32_t tpp = (a.tps + parts - 1u) / parts;
    const uint32_t ta = part * tpp < a.tps ? part * tpp : a.tps, tb = ta + tpp < a.tps ? ta + tpp : a.tps;
    uint32_t *col = a.tpre + (size_t)seg * a.tps * radix + d;
    uint32_t sum = 0;
#pragma unroll 8
    for (uint32_t t = ta; t < tb; ++t) sum += col[(size_t)t * radix];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    uint32_t run = 0, tot = 0;
    for (uint32_t p = 0; p < parts; ++p) {
        const uint32_t v = s_part[p * dg + dl];
        if (p < part) run += v;
        tot += v;
    }
    for (uint32_t t = ta; t < tb; t += 8u) {  // (eight loads in flight, then their stores)
        uint32_t c[8];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) c[u] = t + u < tb ? col[(size_t)(t + u) * radix] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) {
            if (t + u < tb) col[(size_t)(t + u) * radix] = run;
            run += c[u];
        }
    }
    if (part == 0) a.btot[(size_t)seg * RS_RADIX + d] = tot;
}

// bucket bases of one segment, and the sort's `nofit`
__global__ __launch_bounds__(256) void k_rs_bucket_base(rs_args a) {
    __shared__ uint32_t s_wsum[4];
    __shared__ uint32_t s_over;
    const uint32_t seg = blockIdx.x, d = threadIdx.x, radix = 1u << a.topw;
    if (d == 0) s_over = 0u;
    const uint32_t c = d < radix ? a.btot[(size_t)seg * RS_RADIX + d] : 0u;
    const uint32_t ex = rs_block_excl_scan<256>(c, s_wsum);
    if (d < radix) a.bbase[(size_t)seg * RS_RADIX + d] = seg * a.seg_len + ex;
    if (c > RS_FIN_CAP) atomicOr(&s_over, 1u);
    __syncthreads();
    if (d == 0 && s_over && atomicExch(a.nofit, 1u) == 0u) atomicAdd(a.fallbacks, 1u);  // (counted once per sort)
}

// One workgroup per (segment, bucket): the bucket's pairs (at most RS_FIN_CAP, in the order the scatter left them = input order)
// are sorted on the key bits below the top digit in ceil(topshift / 8) stable local rounds -- the scatter's ballot ranking,
// per-wave counters and scan -- and written to the final pair, every wave 64 consecutive pairs at a time.  Keys and payloads stay
// in registers between rounds and cross the workgroup through ONE 4-byte-per-pair LDS buffer (a u64 payload in two halves), so
// the capacity is bounded by registers, not LDS: 36 KB exchange + 8 KB counters per workgroup.
// Occupancy the compiler gives at 512 x 18 (gfx950): u32 payload 93 VGPRs = 5 waves per SIMD, u64 payload 118 VGPRs = 4 waves per
// SIMD; a workgroup is 2 waves per SIMD, so 2 workgroups per CU on both sides (LDS, 45 KB per workgroup, would allow 3).
// Measured against 1024 x 10 and 768 x 12 (profiles/r07_a_sort_sweep.md): 512 x 18 is the fastest on the user side and within
// 6 % of the best on the item side.
template <class ValT>
__global__ __launch_bounds__(RS_FIN_THREADS) SLK_WAVES_PER_EU_RANGE(4, 8) void k_rs_finish(rs_args a) {
    constexpr int THREADS = RS_FIN_THREADS, KPT = RS_FIN_KPT, WAVES = THREADS / 64;
    __shared__ uint32_t s_cnt[WAVES * RS_RADIX];
    __shared__ uint32_t s_lbase[RS_RADIX];
    __shared__ uint32_t s_wsum[WAVES];
    __shared__ uint32_t s_x[RS_FIN_CAP];
    if (*a.nofit) return;
    const uint32_t seg = blockIdx.x >> a.topw, b = blockIdx.x & ((1u << a.topw) - 1u);
    const uint32_t cnt = a.btot[(size_t)seg * RS_RADIX + b];
    if (cnt == 0u) return;  // (cnt <= RS_FIN_CAP: nofit is clear)
    const uint32_t b0 = a.bbase[(size_t)seg * RS_RADIX + b];
    const uint32_t *kin = (const uint32_t *)a.kin + b0;
    const ValT *vin = (const ValT *)a.vin + b0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t e0 = (uint32_t)wave * 64u * KPT + (uint32_t)lane;  // element order = wave, round, lane
    uint32_t key[KPT];
    ValT val[KPT];
    uint32_t pos2[KPT / 2];
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const uint32_t e = e0 + (uint32_t)j * 64u;
        key[j] = e < cnt ? kin[e] : 0u;
    }
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const uint32_t e = e0 + (uint32_t)j * 64u;
        val[j] = e < cnt ? vin[e] : (ValT)0;
    }
    const int rem = a.topshift, R = (rem + RS_RB - 1) / RS_RB, lo = rem / R, extra = rem % R;
    uint32_t *wcnt = s_cnt + wave * RS_RADIX;
    int shift = 0;
    for (int r = 0; r < R; ++r) {
        const int nbits = lo + (r < extra ? 1 : 0);
        const uint32_t radix = 1u << nbits, dmask = radix - 1u;
        for (int i = threadIdx.x; i < WAVES * RS_RADIX; i += THREADS) s_cnt[i] = 0u;
        __syncthreads();
        // ranks inside the wave's 64 * KPT elements, in element order
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            if ((j & 1) == 0) pos2[j / 2] = 0u;
            if ((uint32_t)wave * 64u * KPT + (uint32_t)j * 64u >= cnt) continue;  // (wave-uniform)
            const bool valid = e0 + (uint32_t)j * 64u < cnt;
            const uint32_t dj = rs_digit<uint32_t>(key[j], shift, dmask);
            const unsigned long long m = rs_match(dj, nbits, valid);
            const int leader = m ? __ffsll((long long)m) - 1 : lane;
            uint32_t first = 0;
            if (m && lane == leader) first = atomicAdd(&wcnt[dj], (uint32_t)__popcll(m));
            first = __shfl(first, leader);
            const uint32_t rk = first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            pos2[j / 2] = (j & 1) ? (pos2[j / 2] | (rk << 16)) : rk;
        }
        __syncthreads();
        // per digit: waves' counts -> the wave's first rank in the bucket of this round; the digit's count -> its first position
        uint32_t tcount = 0;
        if (threadIdx.x < radix) {
            uint32_t run = 0;
            for (int w = 0; w < WAVES; ++w) {
                const uint32_t c = s_cnt[w * RS_RADIX + threadIdx.x];
                s_cnt[w * RS_RADIX + threadIdx.x] = run;
                run += c;
            }
            tcount = run;
        }
        const uint32_t lb = rs_block_excl_scan<THREADS>(tcount, s_wsum);
        if (threadIdx.x < radix) s_lbase[threadIdx.x] = lb;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            if (e0 + (uint32_t)j * 64u < cnt) {
                const uint32_t dj = rs_digit<uint32_t>(key[j], shift, dmask);
                const uint32_t pj = ((pos2[j / 2] >> ((j & 1) * 16)) & 0xffffu) + s_lbase[dj] + wcnt[dj];
                pos2[j / 2] = (j & 1) ? ((pos2[j / 2] & 0xffffu) | (pj << 16)) : ((pos2[j / 2] & 0xffff0000u) | pj);
                s_x[pj] = key[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if (e0 + (uint32_t)j * 64u < cnt) key[j] = s_x[e0 + (uint32_t)j * 64u];
        __syncthreads();
        // the payload behind its key: 32 bits per crossing
#pragma unroll
        for (int h = 0; h < (int)(sizeof(ValT) / 4); ++h) {
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                if (e0 + (uint32_t)j * 64u < cnt)
                    s_x[(pos2[j / 2] >> ((j & 1) * 16)) & 0xffffu] = (uint32_t)((uint64_t)val[j] >> (32 * h));
            __syncthreads();
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                if (e0 + (uint32_t)j * 64u < cnt) {
                    const uint64_t w32 = s_x[e0 + (uint32_t)j * 64u];
                    if (sizeof(ValT) == 4) val[j] = (ValT)w32;
                    else val[j] = (ValT)(h == 0 ? (((uint64_t)val[j] & 0xffffffff00000000ull) | w32)
                                                : (((uint64_t)val[j] & 0xffffffffull) | (w32 << 32)));
                }
            __syncthreads();
        }
        shift += nbits;
    }
    uint32_t *kout = (uint32_t *)a.kout + b0;
    ValT *vout = (ValT *)a.vout + b0;
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if (e0 + (uint32_t)j * 64u < cnt) kout[e0 + (uint32_t)j * 64u] = key[j];
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if (e0 + (uint32_t)j * 64u < cnt) vout[e0 + (uint32_t)j * 64u] = val[j];
}

struct rs_plan {
    uint32_t n = 0, seg_len = 0, nseg = 0, tps = 0, ntiles = 0, hbps = 0;
    int npass = 0, shift[RS_MAX_PASS], width[RS_MAX_PASS];
    size_t off_ticket = 0, off_status[RS_MAX_PASS], zero_bytes = 0, off_base = 0, off_data = 0, ctl_bytes = 0;
    size_t off_tpre = 0, off_btot = 0, off_bbase = 0;  // the top-digit route's tables (topw > 0)
};

// digits: `bits` key bits in ceil(bits / 8) passes of (nearly) equal width
static void rs_split_bits(unsigned bits, int *npass, int *shift, int *width) {
    int P = (int)((bits + RS_RB - 1) / RS_RB);
    if (P < 1) P = 1;
    const int lo = (int)bits / P, rem = (int)bits % P;
    int s = 0;
    for (int p = 0; p < P; ++p) {
        width[p] = lo + (p < rem ? 1 : 0);
        if (width[p] < 1) width[p] = 1;
        shift[p] = s;
        s += width[p];
    }
    *npass = P;
}

// The top digit's width for the top-digit route, 0: the sort keeps the LSD passes.  The narrowest digit (longest runs per (tile,
// bucket) in the scatter) whose buckets -- seg_len pairs over the part of the 2^w buckets that ids below `krange` reach -- stay
// under the finish's capacity with 6 sigma to spare.  krange = 0: the caller does not know the range (slk_probe_sort); ids may
// fill as little as half of 2^bits, so that is tried first, then the full range (if the buckets turn out larger, `nofit` says so).
static int rs_pick_topw(size_t seg_len, unsigned bits, size_t krange) {
    const double full = ldexp(1.0, (int)bits);
    double fill[2] = {0.5, 1.0};
    if (krange) fill[0] = fill[1] = (double)krange < full ? (double)krange / full : 1.0;
    for (int f = 0; f < 2; ++f)
        for (int w = 1; w <= RS_RB; ++w) {
            const double mean = (double)seg_len / (ldexp(1.0, w) * fill[f]);
            if (mean + 6.0 * sqrt(mean) <= (double)RS_FIN_CAP) return w;
        }
    return 0;
}

static void rs_make_plan(rs_plan &pl, size_t n, size_t seg_len, unsigned bits, unsigned tile, int topw = 0) {
    pl.n = (uint32_t)n;
    pl.seg_len = (uint32_t)(seg_len && seg_len < n ? seg_len : n);
    pl.nseg = (uint32_t)((n + pl.seg_len - 1) / pl.seg_len);
    pl.tps = (pl.seg_len + tile - 1) / tile;
    pl.ntiles = pl.nseg * pl.tps;
    pl.hbps = (pl.seg_len + RS_HIST_KEYS - 1) / RS_HIST_KEYS;
    rs_split_bits(bits, &pl.npass, pl.shift, pl.width);
    size_t o = (size_t)pl.nseg * pl.npass * RS_RADIX * 4;  // hist
    pl.off_ticket = o;
    o += 512;  // [0, 8): one ticket per pass; [8 + 8 p, 16 + 8 p): pass p's tickets per XCD
    for (int p = 0; p < pl.npass; ++p) {
        pl.off_status[p] = o;
        o += (size_t)pl.ntiles * ((size_t)1 << pl.width[p]) * 4;
    }
    pl.zero_bytes = o;
    o = (o + 255) & ~(size_t)255;
    pl.off_base = o;
    o += (size_t)pl.nseg * pl.npass * RS_RADIX * 4;
    if (topw > 0) {
        pl.off_tpre = o = (o + 255) & ~(size_t)255;
        o += (size_t)pl.ntiles * ((size_t)1 << topw) * 4;
        pl.off_btot = o = (o + 255) & ~(size_t)255;
        o += (size_t)pl.nseg * RS_RADIX * 4;
        pl.off_bbase = o;
        o += (size_t)pl.nseg * RS_RADIX * 4;
    }
    pl.off_data = (o + 255) & ~(size_t)255;
    pl.ctl_bytes = pl.off_data;
}

// the large sorts' tile shape (build-time: the A/Bs of round 4 and round 6 are in profiles/)
#ifndef RS_BIG_THREADS
#define RS_BIG_THREADS 512
#endif
#ifndef RS_BIG_KPT
#define RS_BIG_KPT 16
#endif

template <class KeyT, class ValT, int LOADER>
struct rs_kernels {
    // two tile shapes: 256 threads x 16 keys, and 512 x 16 (twice the run length per (tile, bucket): the large sorts)
    static void launch(int cfg, bool single, unsigned grid, hipStream_t s, const rs_args &a) {
        if (single)
            hipLaunchKernelGGL((k_rs_scatter<KeyT, ValT, 256, 16, RS_LOAD_PLAIN, true>), dim3(1), dim3(256), 0, s, a);
        else if (cfg == 1)
            hipLaunchKernelGGL((k_rs_scatter<KeyT, ValT, RS_BIG_THREADS, RS_BIG_KPT, LOADER, false>), dim3(grid), dim3(RS_BIG_THREADS), 0, s, a);
        else
            hipLaunchKernelGGL((k_rs_scatter<KeyT, ValT, 256, 16, LOADER, false>), dim3(grid), dim3(256), 0, s, a);
    }
};

static inline unsigned rs_tile_of(int cfg) { return cfg == 1 ? (unsigned)(RS_BIG_THREADS * RS_BIG_KPT) : 4096u; }

// The sort.  Pass p reads what pass p - 1 wrote; the last pass writes (kout, vout).  Intermediate passes alternate between
// (kout, vout) and a second buffer pair: (kalt, valt) when the caller has one (the training prep's double buffers, or an
// input the caller allows to be overwritten), else space behind the control block in `scratch`.
// krange: the keys' sorted bits are ids below this (0: not known) -- sizes the top-digit route's buckets.
template <class KeyT, class ValT, int LOADER>
static int rs_sort(slk_ctx *ctx, slk_buf &scratch, rs_args a, size_t n, size_t seg_len, unsigned bits, void *kalt, void *valt,
                   hipStream_t s, size_t krange = 0) {
    if (n == 0) return SLK_OK;
    if (n >= ((size_t)1 << 31)) return slk_fail(ctx, SLK_EINVAL, "sort of %zu pairs: at most 2^31 - 1", n);
    if (bits > 8 * sizeof(KeyT)) bits = 8 * sizeof(KeyT);
    if (bits < 1) bits = 1;
    // (one tile, one workgroup -- for an UNSEGMENTED sort only: a segmented request of <= 4096 pairs keeps its segments)
    const bool single = LOADER == RS_LOAD_PLAIN && n <= 4096 && (seg_len == 0 || seg_len >= n);
    const int cfg = (!single && n >= (size_t)ctx->opt_sort_big_min) ? 1 : 0;
    const unsigned tile = rs_tile_of(cfg);
    // the top-digit route: segmented sorts of u32 keys with the large sorts' tiles, more than one digit
    int topw = 0;
    if (sizeof(KeyT) == 4 && LOADER != RS_LOAD_FY_STEPS && cfg == 1 && seg_len > 0 && bits > (unsigned)RS_RB &&
        (seg_len < n ? seg_len : n) >= ((size_t)ctx->opt_sort_big_min < (size_t)RS_FIN_MIN_SEG ? (size_t)ctx->opt_sort_big_min : (size_t)RS_FIN_MIN_SEG))
        topw = rs_pick_topw(seg_len < n ? seg_len : n, bits, krange);
    rs_plan pl;
    rs_make_plan(pl, n, single ? 0 : seg_len, bits, tile, topw);
    if (pl.seg_len >= (1u << 30)) return slk_fail(ctx, SLK_EINVAL, "sort segment of %u pairs: at most 2^30 - 1", pl.seg_len);
    // With the input as the second buffer pair (`clobber`) and an even number of passes the first pass would have to write over
    // its own input: that one hop goes through the scratch instead.  (The top-digit scatter never writes over its input either.)
    const bool inplace0 = kalt && kalt == a.kin && (pl.npass & 1) == 0;
    const bool need_tmp = (pl.npass > 1 && (!kalt || inplace0)) || (topw && kalt && kalt == a.kin);
    const size_t koff = pl.off_data, voff = (koff + n * sizeof(KeyT) + 255) & ~(size_t)255;
    int rc = slk_ensure(ctx, scratch, need_tmp ? voff + n * sizeof(ValT) : pl.ctl_bytes);
    if (rc) return rc;
    char *base = (char *)scratch.p;
    void *const kmid = (kalt && kalt != a.kin) ? kalt : (void *)(base + koff);  // top-digit route: scatter -> (kmid, vmid) -> finish
    void *const vmid = (kalt && kalt != a.kin) ? valt : (void *)(base + voff);
    void *k0dst = nullptr, *v0dst = nullptr;  // destination of pass 0 when it is neither the final nor the alternate pair
    if (need_tmp && !kalt) {
        kalt = base + koff;
        valt = base + voff;
    } else if (inplace0) {
        k0dst = base + koff;
        v0dst = base + voff;
    }
    a.n = pl.n;
    a.seg_len = pl.seg_len;
    a.tps = pl.tps;
    a.ntiles = pl.ntiles;
    a.hbps = pl.hbps;
    a.npass = pl.npass;
    for (int p = 0; p < pl.npass; ++p) {
        a.shift[p] = pl.shift[p];
        a.width[p] = pl.width[p];
    }
    a.hist = (uint32_t *)base;
    a.base = (uint32_t *)(base + pl.off_base);
    a.ticket = (uint32_t *)(base + pl.off_ticket);
    a.abort_flag = &ctx->d_rng->sort_abort;
    a.debug = ctx->opt_sort_debug;
    a.nseg = pl.nseg;
    a.xcd = pl.nseg >= 2 ? 1 : 0;
    void *kfinal = a.kout, *vfinal = a.vout;
    if (!single) SLK_HIP(ctx, hipMemsetAsync(base, 0, pl.zero_bytes, s));
    if constexpr (sizeof(KeyT) == 4 && LOADER != RS_LOAD_FY_STEPS) {
        if (topw) {
            a.topw = topw;
            a.topshift = (int)bits - topw;
            a.tpre = (uint32_t *)(base + pl.off_tpre);
            a.btot = (uint32_t *)(base + pl.off_btot);
            a.bbase = (uint32_t *)(base + pl.off_bbase);
            a.nofit = a.ticket + 120;  // (inside the zeroed ticket block, behind the tickets)
            a.fallbacks = &ctx->d_rng->sort_fallbacks;
            const unsigned ngr = (1u << topw) < 32u ? 1u : (1u << topw) / 32u;
            hipLaunchKernelGGL((k_rs_tile_hist<KeyT, LOADER, RS_BIG_THREADS, RS_BIG_KPT>), dim3(pl.ntiles), dim3(RS_BIG_THREADS), 0, s, a);
            SLK_LAUNCH_CHECK(ctx, "k_rs_tile_hist");
            hipLaunchKernelGGL(k_rs_tile_scan, dim3(pl.nseg * ngr), dim3(256), 0, s, a);
            SLK_LAUNCH_CHECK(ctx, "k_rs_tile_scan");
            hipLaunchKernelGGL(k_rs_bucket_base, dim3(pl.nseg), dim3(256), 0, s, a);
            SLK_LAUNCH_CHECK(ctx, "k_rs_bucket_base");
            rs_args t = a;
            t.kout = kmid;
            t.vout = vmid;
            hipLaunchKernelGGL((k_rs_scatter<KeyT, ValT, RS_BIG_THREADS, RS_BIG_KPT, LOADER, false, true>), dim3(pl.ntiles), dim3(RS_BIG_THREADS),
                               0, s, t);
            SLK_LAUNCH_CHECK(ctx, "k_rs_scatter (top digit)");
            t.kin = kmid;
            t.vin = vmid;
            t.kout = kfinal;
            t.vout = vfinal;
            hipLaunchKernelGGL((k_rs_finish<ValT>), dim3(pl.nseg << topw), dim3(RS_FIN_THREADS), 0, s, t);
            SLK_LAUNCH_CHECK(ctx, "k_rs_finish");
            a.gate = 1;  // the LSD kernels below: only when a bucket did not fit
            ++ctx->stat_sort_finish_sorts;
        }
    }
    if (!single) {
        a.pass = 0;
        hipLaunchKernelGGL((k_rs_hist<KeyT, LOADER>), dim3(pl.nseg * pl.hbps), dim3(256), 0, s, a);
        SLK_LAUNCH_CHECK(ctx, "k_rs_hist");
        hipLaunchKernelGGL(k_rs_scan, dim3(pl.nseg * (unsigned)pl.npass), dim3(256), 0, s, a);
        SLK_LAUNCH_CHECK(ctx, "k_rs_scan");
    }
    for (int p = 0; p < pl.npass; ++p) {
        const bool to_final = ((pl.npass - 1 - p) & 1) == 0;
        a.pass = p;
        a.kout = to_final ? kfinal : kalt;
        a.vout = to_final ? vfinal : valt;
        if (p == 0 && k0dst) {
            a.kout = k0dst;
            a.vout = v0dst;
        }
        a.status = (uint32_t *)(base + pl.off_status[p]);
        if (p == 0)
            rs_kernels<KeyT, ValT, LOADER>::launch(cfg, single, pl.ntiles, s, a);
        else
            rs_kernels<KeyT, ValT, RS_LOAD_PLAIN>::launch(cfg, single, pl.ntiles, s, a);
        SLK_LAUNCH_CHECK(ctx, "k_rs_scatter");
        a.kin = a.kout;
        a.vin = a.vout;
    }
    return SLK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// generic stable pair sorts by the key bits [0, end_bit).  `clobber`: the input arrays may be used as the second buffer pair.
// ---------------------------------------------------------------------------------------------------------------------------
int slk_sort_pairs_u32_u32_in(slk_ctx *ctx, slk_buf &scratch, const uint32_t *kin, uint32_t *kout, const uint32_t *vin,
                              uint32_t *vout, size_t n, unsigned end_bit, hipStream_t s, bool clobber) {
    rs_args a;
    memset(&a, 0, sizeof(a));
    a.kin = kin;
    a.vin = vin;
    a.kout = kout;
    a.vout = vout;
    return rs_sort<uint32_t, uint32_t, RS_LOAD_PLAIN>(ctx, scratch, a, n, 0, end_bit, clobber ? (void *)kin : nullptr,
                                                      clobber ? (void *)vin : nullptr, s);
}

// 64-bit keys (timestamps whose range needs more than 32 bits, slk_seqprep.hip)
int slk_sort_pairs_u64_u32_in(slk_ctx *ctx, slk_buf &scratch, const uint64_t *kin, uint64_t *kout, const uint32_t *vin,
                              uint32_t *vout, size_t n, unsigned end_bit, hipStream_t s, bool clobber) {
    rs_args a;
    memset(&a, 0, sizeof(a));
    a.kin = kin;
    a.vin = vin;
    a.kout = kout;
    a.vout = vout;
    return rs_sort<uint64_t, uint32_t, RS_LOAD_PLAIN>(ctx, scratch, a, n, 0, end_bit, clobber ? (void *)kin : nullptr,
                                                      clobber ? (void *)vin : nullptr, s);
}

int slk_sort_pairs_u32_u32(slk_ctx *ctx, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, size_t n,
                           unsigned end_bit, hipStream_t s, bool clobber) {
    return slk_sort_pairs_u32_u32_in(ctx, ctx->sort_tmp, kin, kout, vin, vout, n, end_bit, s, clobber);
}

int slk_sort_pairs_u32_u64(slk_ctx *ctx, const uint32_t *kin, uint32_t *kout, const uint64_t *vin, uint64_t *vout, size_t n,
                           unsigned end_bit, hipStream_t s, bool clobber) {
    rs_args a;
    memset(&a, 0, sizeof(a));
    a.kin = kin;
    a.vin = vin;
    a.kout = kout;
    a.vout = vout;
    return rs_sort<uint32_t, uint64_t, RS_LOAD_PLAIN>(ctx, ctx->sort_tmp, a, n, 0, end_bit, clobber ? (void *)kin : nullptr,
                                                      clobber ? (void *)vin : nullptr, s);
}

// The epoch shuffle's (target position, step) pairs, formed by the first pass from the draws J[0 .. n - 2] themselves (rounds
// 1-5: a kernel wrote both arrays first) and sorted by target position, stable: result in (key[1], val[1]), (key[0], val[0]) is
// the second buffer pair.  `scratch`: the shuffle's own sort scratch (it may run on another stream than the training sorts).
int slk_sort_fy_steps(slk_ctx *ctx, slk_buf &scratch, const uint32_t *J, uint32_t n, uint32_t *const key[2], uint32_t *const val[2],
                      hipStream_t s) {
    rs_args a;
    memset(&a, 0, sizeof(a));
    a.uit = J;
    a.fy_n = n;
    a.kout = key[1];
    a.vout = val[1];
    return rs_sort<uint32_t, uint32_t, RS_LOAD_FY_STEPS>(ctx, scratch, a, (size_t)n - 1, 0, slk_bits_for((uint64_t)n), key[0], val[0], s);
}

// measurement / test entry (slk_probe.hip): kind 0 = u32 keys + u32 payloads, 1 = u32 + u64, 2 = u64 + u32; seg_len > 0 sorts
// every segment of seg_len pairs on its own (on the key bits [0, bits))
int slk_sort_pairs_any(slk_ctx *ctx, int kind, const void *kin, void *kout, const void *vin, void *vout, size_t n, size_t seg_len,
                       unsigned bits, hipStream_t s, bool clobber) {
    rs_args a;
    memset(&a, 0, sizeof(a));
    a.kin = kin;
    a.vin = vin;
    a.kout = kout;
    a.vout = vout;
    void *ka = clobber ? (void *)kin : nullptr, *va = clobber ? (void *)vin : nullptr;
    if (kind == 0) return rs_sort<uint32_t, uint32_t, RS_LOAD_PLAIN>(ctx, ctx->sort_tmp, a, n, seg_len, bits, ka, va, s);
    if (kind == 1) return rs_sort<uint32_t, uint64_t, RS_LOAD_PLAIN>(ctx, ctx->sort_tmp, a, n, seg_len, bits, ka, va, s);
    if (kind == 2) return rs_sort<uint64_t, uint32_t, RS_LOAD_PLAIN>(ctx, ctx->sort_tmp, a, n, seg_len, bits, ka, va, s);
    return slk_fail(ctx, SLK_EINVAL, "slk_sort_pairs_any: kind %d", kind);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the training prep's sorts (slk_bilinear.hip::prep_sort): keys built by the first pass, one segment per minibatch
// ---------------------------------------------------------------------------------------------------------------------------
// Is a chunk of minibatches of `seg_len` pairs each sorted as segments (on the id bits only)?  Short segments are not: their
// last tiles would be mostly empty -- the chunk is then one array sorted on (minibatch, id).
static bool rs_segmented(size_t n, size_t seg_len) { return seg_len < n && seg_len >= 32768; }

template <class KeyT, class ValT, int LOADER>
static int rs_sort_fused(slk_ctx *ctx, rs_args a, size_t n, size_t seg_len, unsigned idbits, unsigned mbbits, size_t nids,
                         void *const key[2], void *const val[2], hipStream_t s) {
    a.idbits = idbits;
    a.kout = key[1];
    a.vout = val[1];
    const bool seg = rs_segmented(n, seg_len), one = seg_len >= n;  // one: a single minibatch, its number (0) needs no bits
    a.kseg = seg ? 0u : (uint32_t)seg_len;
    return rs_sort<KeyT, ValT, LOADER>(ctx, ctx->sort_tmp, a, n, seg ? seg_len : 0, (seg || one) ? idbits : idbits + mbbits, key[0],
                                       val[0], s, nids);
}

// interactions of a chunk -> (key = (minibatch, user), payload = (negative << 32 | positive)) sorted by key, stable; the result
// in (key[1], val[1]), (key[0], val[0]) is scratch
int slk_sort_user_fat(slk_ctx *ctx, const int64_t *users, const int64_t *items, const uint32_t *neg32, size_t nc, size_t bsz,
                      unsigned ubits, unsigned mbbits, size_t num_users, uint32_t *const key[2], uint64_t *const val[2], hipStream_t s) {
    rs_args a;
    memset(&a, 0, sizeof(a));
    a.users = users;
    a.items = items;
    a.neg32 = neg32;
    return rs_sort_fused<uint32_t, uint64_t, RS_LOAD_USER_FAT>(ctx, a, nc, bsz, ubits, mbbits, num_users, (void *const *)key, (void *const *)val, s);
}

// same keys, payload = the interaction's index in the chunk (the routes whose dL/dscore exists before the user pass)
int slk_sort_user_idx(slk_ctx *ctx, const int64_t *users, size_t nc, size_t bsz, unsigned ubits, unsigned mbbits, size_t num_users,
                      uint32_t *const key[2], uint32_t *const val[2], hipStream_t s) {
    rs_args a;
    memset(&a, 0, sizeof(a));
    a.users = users;
    return rs_sort_fused<uint32_t, uint32_t, RS_LOAD_USER_IDX>(ctx, a, nc, bsz, ubits, mbbits, num_users, (void *const *)key, (void *const *)val, s);
}

// occurrences r of the packed item list uit[nocc] (NP per user-sorted position) -> (key = (minibatch, item), payload = r)
int slk_sort_item_occ(slk_ctx *ctx, const uint32_t *uit, size_t nocc, size_t bsz, int NP, unsigned ibits, unsigned mbbits,
                      size_t num_items, uint32_t *const key[2], uint32_t *const val[2], hipStream_t s) {
    rs_args a;
    memset(&a, 0, sizeof(a));
    a.uit = uit;
    return rs_sort_fused<uint32_t, uint32_t, RS_LOAD_ITEM_OCC>(ctx, a, nocc, bsz * (size_t)NP, ibits, mbbits, num_items, (void *const *)key,
                                                               (void *const *)val, s);
}

int64_t slk_sort_finish_cap(void) { return (int64_t)RS_FIN_CAP; }

// Sizes ctx->sort_tmp's control block (histograms, tickets, look-back words) for sorts of up to n pairs, so that a training
// call allocates nothing; the second buffer pair of a sort without one is added on demand.
int slk_sort_reserve(slk_ctx *ctx, size_t n) {
    if (n == 0) return SLK_OK;
    rs_plan pl;
    rs_make_plan(pl, n, 0, 32, 4096);
    size_t need = pl.ctl_bytes;
    // a segmented plan of the same size has one partial tile per segment more: bounded by 2 x the tiles
    need += (size_t)pl.ntiles * RS_RADIX * 4 * 4;
    // the top-digit route's tables: 2^8 counts per tile of RS_BIG_THREADS x RS_BIG_KPT pairs (one partial tile per segment more;
    // segmented chunks have segments of >= 32768 pairs), and two words per (segment, bucket)
    need += ((n / rs_tile_of(1)) + n / 32768 + 2) * RS_RADIX * 4 + (n / 32768 + 2) * RS_RADIX * 8 + 1024;
    return slk_ensure(ctx, ctx->sort_tmp, need);
}
