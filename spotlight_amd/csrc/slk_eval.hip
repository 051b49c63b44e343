// slk_eval.hip -- the evaluation side of the path: batched predict and on-GPU ranking.
//
// spotlight/evaluation.py:9-109 (mrr_score, sequence_mrr_score) calls model.predict() once per
// user / sequence -- one pass over the whole item table each (num_items * (4D + 4) bytes) -- and
// ranks the scores on the host with scipy.stats.rankdata.  Here a TILE of users (sequences) is
// scored per pass over the item table (the item rows are read once per 16 representations), and
// the rank of every held-out item is counted on the GPU:
//
//   slk_bilinear_scores  out[r][i] = <U[user_r], V[i]> + bu[user_r] + bi[i]      (BilinearNet.forward)
//   slk_poolnet_scores   out[r][i] = bi[i] + <final representation of sequence r, V[i]>  (PoolNet)
//   slk_rank_targets     rankdata(-out[row])[item] ('average' ties) for each (row, item) target, after
//                        out[row][excluded] = -FLT_MAX (the reference sets predictions[...] = FLOAT_MAX)
//
// Scores are formed exactly as k_predict / k_seq_predict form them (same lane layout, same
// summation order), so the batched path returns bit-identical numbers.
#include <float.h>
#include <math.h>

#include "slk_kernels.h"

// representation of row r for BilinearNet: the user's embedding vector and bias
template <int VEC, int G>
__global__ __launch_bounds__(256) void k_eval_user_rows(const float *U, const float *bu, slk_bloom_dev ub, int D,
                                                        const int64_t *users, int64_t n, float *rep, float *rbias) {
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const int d0 = lane * VEC;
    const bool on = d0 < D;
    for (int64_t r = (int64_t)blockIdx.x * GPB + grp; r < n; r += (int64_t)gridDim.x * GPB) {
        const int64_t u = users[r];
        const slk_vec<VEC> v = slk_emb_vec<VEC>(U, ub, (uint32_t)u, D, d0, on);
        if (on) slk_vstore<VEC>(rep + (size_t)r * D + d0, v);
        if (lane == 0) rbias[r] = bu[u];
    }
}

// representation of row r for PoolNet: user_representation's final state (sequence/implicit.py:331-335,
// sequence/representations.py:92-114): sum of the L item vectors / (per-dimension non-zero count + 1)
template <int VEC, int G>
__global__ __launch_bounds__(256) void k_eval_seq_rows(const float *E, slk_bloom_dev ib, int D, const int64_t *seqs,
                                                       int64_t n, int L, float *rep) {
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const int d0 = lane * VEC;
    const bool on = d0 < D;
    for (int64_t r = (int64_t)blockIdx.x * GPB + grp; r < n; r += (int64_t)gridDim.x * GPB) {
        const int64_t *seq = seqs + (size_t)r * L;
        slk_vec<VEC> S = slk_vzero<VEC>(), Cn = slk_vzero<VEC>();
        for (int t = 0; t < L; ++t) {
            const slk_vec<VEC> e = slk_emb_vec<VEC>(E, ib, (uint32_t)seq[t], D, d0, on);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                S.v[i] += e.v[i];
                Cn.v[i] += (e.v[i] != 0.0f) ? 1.0f : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) S.v[i] = S.v[i] / (Cn.v[i] + 1.0f);
        if (on) slk_vstore<VEC>(rep + (size_t)r * D + d0, S);
    }
}

// out[r] = 1 / sqrt(sum_d x[r][d]^2) (slk_rows_inv_norm: the factors of the cosine), the sum formed as THE chain
// s = fmaf(x_d, x_d, s) over d = 0 .. D-1 from 0 (slk_chain_dot of the row with itself: lane s continues lane s - 1), so that
// every build and every caller -- a table's own vector, a rank's copy of a fetched row -- defines the same bits.  A row whose
// sum is exactly 0 gets 0.0f (it scores 0 against everything, never NaN); a NaN or inf sum propagates.
template <int VEC, int G>
__global__ __launch_bounds__(256) void k_rows_inv_norm(const float *T, int D, int64_t n, float *out) {
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const int d0 = lane * VEC;
    const bool on = d0 < D;
    for (int64_t r = (int64_t)blockIdx.x * GPB + grp; r < n; r += (int64_t)gridDim.x * GPB) {
        const slk_vec<VEC> x = on ? slk_vload<VEC>(T + (size_t)r * D + d0) : slk_vzero<VEC>();
        const float ss = slk_chain_dot<VEC, G>(x, x);
        if (lane == 0) out[r] = ss == 0.0f ? 0.0f : 1.0f / sqrtf(ss);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Scores as a GEMM on the matrix cores.  scores[r][i] = <rep_r, V_i> is a (rows x D) x (D x items) product in fp32: the one
// place on this path where MFMA is the right unit.  v_mfma_f32_32x32x2_f32 is EXACT fp32 -- bit for bit the k-ordered chain
// acc = fmaf(a_k, b_k, acc) (cdna_hip_programming.md 3) -- so "the score" of this package is DEFINED as that chain over
// d = 0 .. D-1 (slk_chain_dot in slk_kernels.h is the same chain on the vector unit, for explicit (row, item) pairs), and
// predict(), the batched score rows and the fused ranking below agree bit for bit whichever unit formed them.
//
// k_score_gemm: a workgroup (4 waves) keeps a tile of RT = 32 * MT representations in LDS and sweeps a chunk of the item
// table in blocks of 128 rows (each wave 32 of them: one 32x32 accumulator tile per 32 representations), staging every block
// through registers into LDS while the previous one is multiplied.  MODE WRITE stores the scores (slk_*_scores, predict of
// one row against every item); MODE COUNT never stores them: every score is compared with its row's target score as it
// leaves the accumulators (rank = #greater + (#equal + 1) / 2, scipy's 'average'), per-lane packed counters, one atomic per
// row and workgroup at the end -- the [rows x items] score matrix of the round-3 path (written, then read back per target)
// does not exist.  Item traffic: items * (4 D + 4) bytes per row tile, i.e. per 64 rows.
// ---------------------------------------------------------------------------------------------------------------------------
#define SLK_GEMM_IB 128  // item rows per block of the sweep (4 waves x 32)
#define SLK_GEMM_KC 64   // depth of one staged chunk
#define SLK_GEMM_KS 65   // LDS row stride in floats (odd: the 32 lanes of an operand read hit 32 banks)

struct slk_gemm_args {
    const float *rep, *rbias;     // [groups][D], [groups] (nullptr: no row bias, PoolNet)
    const int64_t *rowmap;        // row r belongs to group rowmap[r] (nullptr: r)
    const int64_t *gmap;          // group g's representation is row gmap[g] of rep / rbias (nullptr: g) -- a plain user table
                                  // is read in place through the user ids
    const float *V, *bi;
    slk_bloom_dev ib;
    int D;
    int64_t R, I, items_per_wg;
    float *out;                   // WRITE: [R][I]
    const float *st;              // COUNT: the row's target score
    unsigned *gt, *eq;            // COUNT: per-row counts (atomicAdd)
    int k, cap;                   // SELECT: keys kept per row, candidate slots per row in LDS (>= k + SLK_GEMM_IB)
    const int64_t *exc_off, *exc_items;  // SELECT: row r's excluded items, sorted and distinct (CSR; exc_off nullptr: none)
    unsigned long long *cand;     // SELECT: [R][gridDim.x][k] keys, 0 = empty
};

enum { SLK_GEMM_WRITE = 0, SLK_GEMM_COUNT = 1, SLK_GEMM_SELECT = 2 };  // what the sweep does with a score
// ... and WRITE / SELECT with the neighbour epilogue (slk_neighbors_*: factors in the place of biases, see k_score_gemm)
enum { SLK_GEMM_NBR_WRITE = 3, SLK_GEMM_NBR_SELECT = 4 };

#if defined(__HIPCC__)
typedef float slk_f32x16 __attribute__((ext_vector_type(16)));
#else
struct slk_f32x16 {
    float v[16];
    float &operator[](int i) { return v[i]; }
};
#endif

// element (item, d) of the item-side operand: one row of a plain table or the sum of a bloom id's hashed rows
__device__ __forceinline__ float slk_gemm_item_elem(const float *V, const slk_bloom_dev &b, uint32_t id, int D, int d) {
    if (b.n_hash == 0) return V[(size_t)id * D + d];
    float v = V[(size_t)slk_bloom_row(b, id, 0) * D + d];
    for (int h = 1; h < b.n_hash; ++h) v += V[(size_t)slk_bloom_row(b, id, h) * D + d];
    return v;
}


// ---------------------------------------------------------------------------------------------------------------------------
// MODE SELECT (slk_*_topk): the k best items of every row, by the total order of include/spotlight_hip.h -- score descending
// (-0.0 == +0.0), ties to the smaller id, NaN below every number.  One 64-bit key carries the order: the high word is the
// score's orderable bits (0 = NaN, then -inf .. +inf ascending), the low word ~item, so "better" is one unsigned compare and no
// two items of a row share a key; key 0 is no item at all (an empty slot: item -1, score -inf).  Every row of the tile keeps in
// LDS a threshold key (the k-th best key seen so far, 0 until there are k), a count and `cap` candidate slots.  A lane whose
// score beats its row's threshold looks the item up in the row's exclusion list (binary search: only survivors pay for it) and
// takes a slot with one LDS atomic.  A block of the sweep adds at most SLK_GEMM_IB candidates to a row, so a row whose count
// is at most cap - SLK_GEMM_IB cannot overflow in the next block; a row above that is compacted first: one wave sorts its
// slots (a bitonic network whose comparators all point the same way, so the slots past `cap` may stay virtual), the threshold
// becomes the k-th key and the count k.  A stale threshold is a lower bound of the true k-th key: it only lets more candidates in,
// the result does not depend on when rows are compacted, on the chunking or on the order of the atomics.
// ---------------------------------------------------------------------------------------------------------------------------
typedef unsigned long long slk_key;

__device__ __forceinline__ unsigned slk_topk_hi(float sc) {
    if (sc != sc) return 0u;
    if (sc == 0.0f) return 0x80000000u;  // both zeros
    unsigned b;
    memcpy(&b, &sc, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float slk_topk_score(unsigned hi) {
    const unsigned b = hi == 0u ? 0x7fc00000u : ((hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi);
    float sc;
    memcpy(&sc, &b, 4);
    return sc;
}

__device__ __forceinline__ bool slk_topk_excluded(const int64_t *list, int64_t lo, int64_t end, int64_t item) {
    int64_t hi = end;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (list[mid] < item) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && list[lo] == item;
}

// ONE WAVE: sorts c[0, cap) descending (the slots from `count` on are emptied first) and keeps the k best: *thr = the k-th key
// (0 while there are fewer), *cnt = min(count, k).  Every lane of the wave calls it with the same arguments.
__device__ inline void slk_topk_compact(slk_key *c, unsigned count, int k, int cap, int lane, slk_key *thr, unsigned *cnt) {
    for (int i = (int)count + lane; i < cap; i += 64) c[i] = 0ull;
    int n = 64;
    while (n < cap) n <<= 1;
    SLK_SUBWAVE_SYNC();
    for (int kk = 2; kk <= n; kk <<= 1) {
        // two sorted runs of kk / 2: element i against its mirror image in the pair of runs ...
        for (int t = lane; t < n / 2; t += 64) {
            const int b = t / (kk / 2), off = t - b * (kk / 2);
            const int i = b * kk + off, p = b * kk + kk - 1 - off;
            if (p < cap) {  // (a slot past cap is empty and stays so: the better key goes to the smaller index)
                const slk_key x = c[i], y = c[p];
                if (y > x) {
                    c[i] = y;
                    c[p] = x;
                }
            }
        }
        SLK_SUBWAVE_SYNC();
        // ... then the half-cleaners of every run
        for (int j = kk >> 2; j >= 1; j >>= 1) {
            for (int t = lane; t < n / 2; t += 64) {
                const int i = (t / j) * 2 * j + (t % j), p = i + j;
                if (p < cap) {
                    const slk_key x = c[i], y = c[p];
                    if (y > x) {
                        c[i] = y;
                        c[p] = x;
                    }
                }
            }
            SLK_SUBWAVE_SYNC();
        }
    }
    if (lane == 0) {
        *thr = count >= (unsigned)k ? c[k - 1] : 0ull;
        *cnt = count < (unsigned)k ? count : (unsigned)k;
    }
    SLK_SUBWAVE_SYNC();
}

// MODE NBR_WRITE / NBR_SELECT (slk_neighbors_*: rows of any dense table against dense query rows): WRITE / SELECT with no
// biases; a.rbias / a.bi, where given, are per-row and per-item FACTORS -- the score is (acc * rbias[row]) * bi[item] (cosine:
// the inverse norms), the bare chain where both are nullptr.  Compile-time variants of the epilogue: the other instantiations
// are what they were.
template <int MT, int MODE, bool VEC4, bool AREG>
__global__ __launch_bounds__(256) SLK_WAVES_PER_EU(2) void k_score_gemm(slk_gemm_args a) {  // (two workgroups per CU by LDS footprint, eval_gemm: 2 waves per SIMD)
    constexpr int RT = 32 * MT, IB = SLK_GEMM_IB, KC = SLK_GEMM_KC, KS = SLK_GEMM_KS;
    constexpr int BREG = VEC4 ? IB * KC / 256 : 1;  // staged floats per thread (plain tables of dim % 4 == 0)
    constexpr bool SCALE = MODE == SLK_GEMM_NBR_WRITE || MODE == SLK_GEMM_NBR_SELECT;
    constexpr bool COUNT = MODE == SLK_GEMM_COUNT, SELECT = MODE == SLK_GEMM_SELECT || MODE == SLK_GEMM_NBR_SELECT;
    constexpr bool WRITE = MODE == SLK_GEMM_WRITE || MODE == SLK_GEMM_NBR_WRITE;
    HIP_DYNAMIC_SHARED(float, lds)
    float *sA = lds;                      // [RT][KS]
    float *sB = sA + RT * KS;             // [IB][KS]
    float *s_rb = sB + IB * KS;           // [RT]
    float *s_st = s_rb + RT;              // [RT]
    unsigned *s_gt = reinterpret_cast<unsigned *>(s_st + RT);  // [RT]
    unsigned *s_eq = s_gt + RT;           // [RT]
    // SELECT: per row the threshold key, the window of its exclusion list, the candidate count and the candidates
    slk_key *s_thr = reinterpret_cast<slk_key *>(s_eq + RT);   // [RT]  ((RT + IB) * KS + 4 * RT floats: a multiple of 8 bytes)
    int64_t *s_eo = reinterpret_cast<int64_t *>(s_thr + RT);   // [RT][2]
    slk_key *s_cand = reinterpret_cast<slk_key *>(s_eo + 2 * RT);  // [RT][a.cap]
    unsigned *s_cnt = reinterpret_cast<unsigned *>(s_cand + (SELECT ? (size_t)RT * a.cap : 0));  // [RT]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D;
    const int64_t r0 = (int64_t)blockIdx.y * RT;
    const int64_t i_begin = (int64_t)blockIdx.x * a.items_per_wg;
    const int64_t i_end = (a.I - i_begin < a.items_per_wg) ? a.I : i_begin + a.items_per_wg;
    if (i_begin >= i_end) return;
    const int nkc = (D + KC - 1) / KC;
    for (int t = tid; t < RT; t += 256) {
        const bool live = r0 + t < a.R;
        int64_t g = live ? (a.rowmap ? a.rowmap[r0 + t] : r0 + t) : 0;
        if (live && a.gmap) g = a.gmap[g];
        s_rb[t] = (live && a.rbias) ? a.rbias[g] : 0.0f;
        if (COUNT) {
            s_st[t] = live ? a.st[r0 + t] : 0.0f;
            s_gt[t] = 0u;
            s_eq[t] = 0u;
        }
        if (SELECT) {
            s_thr[t] = live ? 0ull : ~0ull;  // (a row past the last one takes no candidate)
            s_cnt[t] = 0u;
            s_eo[2 * t] = (live && a.exc_off) ? a.exc_off[r0 + t] : 0;
            s_eo[2 * t + 1] = (live && a.exc_off) ? a.exc_off[r0 + t + 1] : 0;
        }
    }
    // the representations' chunk [kc, kc + KC) -> sA (zero beyond D and beyond the last row)
    auto stage_a = [&](int kc) {
        for (int e = tid; e < RT * KC; e += 256) {
            const int row = e / KC, k = e - row * KC;
            float v = 0.0f;
            if (r0 + row < a.R && kc + k < D) {
                int64_t g = a.rowmap ? a.rowmap[r0 + row] : r0 + row;
                if (a.gmap) g = a.gmap[g];
                v = a.rep[(size_t)g * D + kc + k];
            }
            sA[row * KS + k] = v;
        }
    };
    // block [i0, i0 + IB) x chunk [kc, kc + KC) of the item operand -> registers (the loads are in flight while the previous
    // block is multiplied), then registers -> sB
    float breg[BREG];
    auto fetch_b = [&](int64_t i0, int kc) {
        if (VEC4) {
#pragma unroll
            for (int u = 0; u < BREG / 4; ++u) {
                const int q = tid + 256 * u, item = q / (KC / 4), k = (q - item * (KC / 4)) * 4;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (i0 + item < i_end && kc + k < D) v = *reinterpret_cast<const float4 *>(a.V + (size_t)(i0 + item) * D + kc + k);
                breg[4 * u] = v.x;
                breg[4 * u + 1] = v.y;
                breg[4 * u + 2] = v.z;
                breg[4 * u + 3] = v.w;
            }
        }
        // (any other table -- odd dims, BloomEmbedding rows -- is staged in store_b, element by element: not the fast route)
    };
    auto store_b = [&](int64_t i0, int kc) {
        if (VEC4) {
#pragma unroll
            for (int u = 0; u < BREG / 4; ++u) {
                const int q = tid + 256 * u, item = q / (KC / 4), k = (q - item * (KC / 4)) * 4;
#pragma unroll
                for (int c = 0; c < 4; ++c) sB[item * KS + k + c] = breg[4 * u + c];
            }
        } else {
            for (int q = tid; q < IB * KC; q += 256) {
                const int item = q / KC, k = q - item * KC;
                sB[item * KS + k] =
                    (i0 + item < i_end && kc + k < D) ? slk_gemm_item_elem(a.V, a.ib, (uint32_t)(i0 + item), D, kc + k) : 0.0f;
            }
        }
    };
    // COUNT: (#equal << 16) | #greater among this lane's columns so far, per accumulator element's row.  (One wave vote per
    // comparison with the row's counter kept by one lane -- 16 * MT registers less -- was measured: 9.0 instead of 6.6 ms
    // for 4096 x 10^6 scores, the votes' scalar work sits in the epilogue of every block: profiles/r04_g_*.)
    unsigned cnt[MT * 16];
    if (COUNT) {
#pragma unroll
        for (int i = 0; i < MT * 16; ++i) cnt[i] = 0u;
    }
    if (nkc == 1) stage_a(0);
    fetch_b(i_begin, 0);
#if defined(__HIPCC__)
    float areg[AREG ? MT * (KC / 2) : 1];
    if (AREG) {
        __syncthreads();  // sA is complete (zero beyond D: the chain adds +0 for the padded depth)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int k = 0; k < KC; k += 2) areg[m * (KC / 2) + k / 2] = sA[(m * 32 + (lane & 31)) * KS + (lane >> 5) + k];
    }
#endif
    for (int64_t i0 = i_begin; i0 < i_end; i0 += IB) {
        slk_f32x16 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[m][v] = 0.0f;
        for (int c = 0; c < nkc; ++c) {
            const int kc = c * KC;
            __syncthreads();  // the previous chunk's operands have been read
            if (nkc > 1) stage_a(kc);
            store_b(i0, kc);
            __syncthreads();
            // the next chunk (or the next block's first) into the registers
            {
                const bool more_k = c + 1 < nkc;
                const int64_t ni = more_k ? i0 : i0 + IB;
                if (ni < i_end) fetch_b(ni, more_k ? kc + KC : 0);
            }
            const int kw = (D - kc < KC) ? ((D - kc + 1) & ~1) : KC;  // even: the pad column is zero
#if defined(__HIPCC__)
            const float *pa = sA + (lane & 31) * KS + (lane >> 5);
            const float *pb = sB + (wave * 32 + (lane & 31)) * KS + (lane >> 5);
            if (AREG) {
                // the representations' operand lives in registers for the whole sweep (dim <= 64: one chunk): one LDS read per
                // two matrix instructions instead of three
#pragma unroll
                for (int k = 0; k < KC; k += 2) {
                    const float b = pb[k];
#pragma unroll
                    for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[m * (KC / 2) + k / 2], b, acc[m], 0, 0, 0);
                }
            } else {
#pragma unroll 2
                for (int k = 0; k < kw; k += 2) {
                    const float b = pb[k];
#pragma unroll
                    for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[m * 32 * KS + k], b, acc[m], 0, 0, 0);
                }
            }
#else
            // the test harness's host build: the same k-ordered fmaf chain per accumulator element, operands from LDS
            for (int k = 0; k < kw; ++k)
                for (int m = 0; m < MT; ++m)
                    for (int v = 0; v < 16; ++v) {
                        const int row = m * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5);
                        acc[m][v] = fmaf(sA[row * KS + k], sB[(wave * 32 + (lane & 31)) * KS + k], acc[m][v]);
                    }
#endif
        }
        // epilogue: accumulator element v of tile m = (row m*32 + (v&3) + 8*(v>>2) + 4*(lane>>5), item i0 + wave*32 + (lane&31))
        const int64_t item = i0 + wave * 32 + (lane & 31);
        const bool live = item < i_end;
        const float bias = SCALE ? ((live && a.bi) ? a.bi[item] : 0.0f) : (live ? a.bi[item] : 0.0f);
        // (WRITE: this lane's output column; the row offsets below are wave-uniform multiples of the row stride)
        float *ocol = !WRITE ? nullptr : a.out + (size_t)(r0 + 4 * (lane >> 5)) * a.I + item;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                // (a compiler barrier per four elements: the row constants are re-read from LDS where they are used instead
                // of all 32 * MT of them being hoisted into registers)
                if ((v & 3) == 0) asm volatile("" ::: "memory");
                const int row_a = m * 32 + (v & 3) + 8 * (v >> 2);  // lanes 0..31; lanes 32..63 hold row_a + 4
                const int row = row_a + 4 * (lane >> 5);
                // k_predict: (dot + bu) + bi;  k_seq_predict: bi + dot
                const float sc = SCALE ? (a.bi ? (acc[m][v] * s_rb[row]) * bias : acc[m][v])
                                       : (a.rbias ? (acc[m][v] + s_rb[row]) + bias : bias + acc[m][v]);
                if (COUNT) {
                    const float t = s_st[row];
                    cnt[m * 16 + v] += (live && sc > t ? 1u : 0u) + (live && sc == t ? 0x10000u : 0u);
                } else if (SELECT) {
                    // the high words alone turn nearly every score away; an equal high word is a tie: the ids decide
                    const unsigned hi = slk_topk_hi(sc);
                    if (live && hi >= (unsigned)(s_thr[row] >> 32)) {
                        const slk_key key = ((slk_key)hi << 32) | (slk_key)(~(unsigned)item);
                        if (key > s_thr[row] && !slk_topk_excluded(a.exc_items, s_eo[2 * row], s_eo[2 * row + 1], item))
                            s_cand[(size_t)row * a.cap + atomicAdd(&s_cnt[row], 1u)] = key;
                    }
                } else if (live && r0 + row < a.R) {
                    ocol[(size_t)row_a * a.I] = sc;
                }
            }
        if (SELECT) {
            __syncthreads();  // the block's candidates are in
            for (int row = wave; row < RT; row += 4) {
                const unsigned c = s_cnt[row];
                if (c > (unsigned)(a.cap - IB)) slk_topk_compact(s_cand + (size_t)row * a.cap, c, a.k, a.cap, lane, &s_thr[row], &s_cnt[row]);
            }
            // (the next block's epilogue is two barriers away)
        }
    }
    if (SELECT) {
        // the chunk's at most k keys of every row -> a.cand[row][chunk][k]
        __syncthreads();
        for (int row = wave; row < RT; row += 4) {
            unsigned c = s_cnt[row];
            slk_key *cs = s_cand + (size_t)row * a.cap;
            if (c > (unsigned)a.k) {
                slk_topk_compact(cs, c, a.k, a.cap, lane, &s_thr[row], &s_cnt[row]);
                c = (unsigned)a.k;
            }
            if (r0 + row < a.R) {
                slk_key *dst = a.cand + ((size_t)(r0 + row) * gridDim.x + blockIdx.x) * a.k;
                for (int i = lane; i < a.k; i += 64) dst[i] = i < (int)c ? cs[i] : 0ull;
            }
        }
    }
    if (COUNT) {
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = m * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5);
                const unsigned c = cnt[m * 16 + v];
                if (c & 0xffffu) atomicAdd(&s_gt[row], c & 0xffffu);
                if (c >> 16) atomicAdd(&s_eq[row], c >> 16);
            }
        __syncthreads();
        for (int t = tid; t < RT; t += 256)
            if (r0 + t < a.R) {
                if (s_gt[t]) atomicAdd(&a.gt[r0 + t], s_gt[t]);
                if (s_eq[t]) atomicAdd(&a.eq[r0 + t], s_eq[t]);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// A handful of rows against every item (predict(user): ONE row; implicit.py:277-311 with item_ids = None): a GEMV, bound by the
// one pass over the item table -- 32 rows of matrix-core tile around a single live row buy nothing.  k_score_rows streams the
// table in blocks of 256 item rows through registers into LDS (the next block's 64 KB are in flight while the current one is
// used; two workgroups per CU = 128 KB per CU in flight) and every thread walks the score chain of ONE item against the NR
// rows: acc[r] = fmaf(a_r[k], b[k], acc[r]), k ascending -- the chain of slk_chain_dot and of the MFMA, so the scores are the
// same bits whichever kernel forms them.  Plain tables with dim % 4 == 0 (anything else takes k_score_gemm's general loader).
// ---------------------------------------------------------------------------------------------------------------------------
#define SLK_ROWS_IB 256  // items per block: one per thread

template <int NR>
__global__ __launch_bounds__(256) void k_score_rows(slk_gemm_args a) {
    constexpr int IB = SLK_ROWS_IB, KC = SLK_GEMM_KC, KS = SLK_GEMM_KS;
    constexpr int BREG = IB * KC / 256;  // staged floats per thread
    HIP_DYNAMIC_SHARED(float, lds)
    float *sB = lds;              // [IB][KS]
    float *sA = sB + IB * KS;     // [NR][KC]
    float *s_rb = sA + NR * KC;   // [NR]
    const int tid = threadIdx.x;
    const int D = a.D;
    const int64_t i_begin = (int64_t)blockIdx.x * a.items_per_wg;
    const int64_t i_end = (a.I - i_begin < a.items_per_wg) ? a.I : i_begin + a.items_per_wg;
    if (i_begin >= i_end) return;
    const int nkc = (D + KC - 1) / KC;
    auto group_of = [&](int r) -> int64_t {
        int64_t g = a.rowmap ? a.rowmap[r] : r;
        return a.gmap ? a.gmap[g] : g;
    };
    if (tid < NR) s_rb[tid] = (tid < a.R && a.rbias) ? a.rbias[group_of(tid)] : 0.0f;
    auto stage_a = [&](int kc) {
        for (int e = tid; e < NR * KC; e += 256) {
            const int row = e / KC, k = e - row * KC;
            sA[e] = (row < a.R && kc + k < D) ? a.rep[(size_t)group_of(row) * D + kc + k] : 0.0f;
        }
    };
    float breg[BREG];
    auto fetch_b = [&](int64_t i0, int kc) {
#pragma unroll
        for (int u = 0; u < BREG / 4; ++u) {
            const int q = tid + 256 * u, item = q / (KC / 4), k = (q - item * (KC / 4)) * 4;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i0 + item < i_end && kc + k < D) v = *reinterpret_cast<const float4 *>(a.V + (size_t)(i0 + item) * D + kc + k);
            breg[4 * u] = v.x;
            breg[4 * u + 1] = v.y;
            breg[4 * u + 2] = v.z;
            breg[4 * u + 3] = v.w;
        }
    };
    auto store_b = [&]() {
#pragma unroll
        for (int u = 0; u < BREG / 4; ++u) {
            const int q = tid + 256 * u, item = q / (KC / 4), k = (q - item * (KC / 4)) * 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) sB[item * KS + k + c] = breg[4 * u + c];
        }
    };
    if (nkc == 1) stage_a(0);
    fetch_b(i_begin, 0);
    for (int64_t i0 = i_begin; i0 < i_end; i0 += IB) {
        float acc[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r] = 0.0f;
        for (int c = 0; c < nkc; ++c) {
            const int kc = c * KC;
            __syncthreads();  // the previous chunk's operands have been read
            if (nkc > 1) stage_a(kc);
            store_b();
            __syncthreads();
            {
                const bool more_k = c + 1 < nkc;
                const int64_t ni = more_k ? i0 : i0 + IB;
                if (ni < i_end) fetch_b(ni, more_k ? kc + KC : 0);
            }
            const int kw = (D - kc < KC) ? D - kc : KC;
            const float *pb = sB + tid * KS;
#pragma unroll 8
            for (int k = 0; k < kw; ++k) {
                const float b = pb[k];
#pragma unroll
                for (int r = 0; r < NR; ++r) acc[r] = fmaf(sA[r * KC + k], b, acc[r]);
            }
        }
        const int64_t item = i0 + tid;
        if (item < i_end) {
            const float bias = a.bi[item];
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (r < a.R) a.out[(size_t)r * a.I + item] = a.rbias ? (acc[r] + s_rb[r]) + bias : bias + acc[r];
        }
    }
}

// st[r] = score(representation of row r, its target item) on the vector unit (the same chain); a target that is on its own
// group's exclusion list scores -FLT_MAX, as the reference's `predictions[excluded] = FLOAT_MAX` makes it
// SHARD (slk_shard_target_scores): V / bi are ONE RANK's rows and tgt[r] is the target's LOCAL row, or -1 where another rank
// owns it (any row outside [0, I) is treated so): such a row scores -INFINITY, the identity of the ranks' MAX
template <int VEC, int G, bool SHARD>
__global__ __launch_bounds__(256) void k_rank_target_scores(const float *rep, const float *rbias, const int64_t *rowmap,
                                                            const int64_t *gmap, const float *V, const float *bi, slk_bloom_dev ib, int D,
                                                            int64_t I, const int64_t *tgt, const int64_t *exc_off,
                                                            const int64_t *exc_items, int64_t n_rows, float *st) {
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const int d0 = lane * VEC;
    const bool on = d0 < D;
    for (int64_t r = (int64_t)blockIdx.x * GPB + grp; r < n_rows; r += (int64_t)gridDim.x * GPB) {
        const int64_t g = rowmap ? rowmap[r] : r;
        const bool owned = !SHARD || (tgt[r] >= 0 && tgt[r] < I);
        const int64_t item = owned ? tgt[r] : 0;  // (a row that is not owned walks row 0: the group's lanes stay together)
        const int64_t src = gmap ? gmap[g] : g;
        const slk_vec<VEC> x = on ? slk_vload<VEC>(rep + (size_t)src * D + d0) : slk_vzero<VEC>();
        const slk_vec<VEC> y = slk_emb_vec<VEC>(V, ib, (uint32_t)item, D, d0, on);
        const float dot = slk_chain_dot<VEC, G>(x, y);
        float sc = rbias ? (dot + rbias[src]) + bi[item] : bi[item] + dot;
        if (exc_off) {
            unsigned long long hit = 0;
            for (int64_t e = exc_off[g] + lane; e < exc_off[g + 1]; e += G) hit |= (exc_items[e] == item) ? 1ull : 0ull;
            if (slk_group_or<G>(hit)) sc = -FLT_MAX;
        }
        if (SHARD && !owned) sc = -INFINITY;
        if (lane == 0) st[r] = sc;
    }
}

// The sweep counted every item with its real score.  For every item on the row's exclusion list: take its real score's
// contribution out and put -FLT_MAX's in (dgt / deq: signed corrections, one writer per row)
template <int VEC, int G>
__global__ __launch_bounds__(256) void k_rank_exclusions(const float *rep, const float *rbias, const int64_t *rowmap,
                                                         const int64_t *gmap, const float *V, const float *bi, slk_bloom_dev ib, int D,
                                                         const int64_t *exc_off, const int64_t *exc_items, const float *st,
                                                         int64_t n_rows, int *dgt, int *deq) {
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const int d0 = lane * VEC;
    const bool on = d0 < D;
    for (int64_t r = (int64_t)blockIdx.x * GPB + grp; r < n_rows; r += (int64_t)gridDim.x * GPB) {
        const int64_t g = rowmap ? rowmap[r] : r;
        const int64_t src = gmap ? gmap[g] : g;
        const slk_vec<VEC> x = on ? slk_vload<VEC>(rep + (size_t)src * D + d0) : slk_vzero<VEC>();
        const float t = st[r], rb = rbias ? rbias[src] : 0.0f;
        int cg = 0, ce = 0;
        for (int64_t e = exc_off[g]; e < exc_off[g + 1]; ++e) {
            const int64_t item = exc_items[e];
            const slk_vec<VEC> y = slk_emb_vec<VEC>(V, ib, (uint32_t)item, D, d0, on);
            const float dot = slk_chain_dot<VEC, G>(x, y);
            const float sc = rbias ? (dot + rb) + bi[item] : bi[item] + dot;
            cg += (-FLT_MAX > t ? 1 : 0) - (sc > t ? 1 : 0);
            ce += (-FLT_MAX == t ? 1 : 0) - (sc == t ? 1 : 0);
        }
        if (lane == 0) {
            dgt[r] = cg;
            deq[r] = ce;
        }
    }
}

__global__ __launch_bounds__(256) void k_rank_final(const unsigned *gt, const unsigned *eq, const int *dgt, const int *deq,
                                                    int64_t n_rows, double *rank) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * 256) {
        const double g = (double)gt[r] + (dgt ? (double)dgt[r] : 0.0), e = (double)eq[r] + (deq ? (double)deq[r] : 0.0);
        rank[r] = g + (e + 1.0) * 0.5;
    }
}

// the sharded form of k_rank_final: ONE RANK's share of the two counts, corrections applied, widened for the ranks' SUM
__global__ __launch_bounds__(256) void k_rank_counts_out(const unsigned *gt, const unsigned *eq, const int *dgt, const int *deq,
                                                         int64_t n_rows, int64_t *gt_out, int64_t *eq_out) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * 256) {
        gt_out[r] = (int64_t)gt[r] + (dgt ? (int64_t)dgt[r] : 0);
        eq_out[r] = (int64_t)eq[r] + (deq ? (int64_t)deq[r] : 0);
    }
}

__global__ __launch_bounds__(256) void k_eval_exclude(float *scores, int64_t n_items, const int64_t *rows,
                                                      const int64_t *items, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256)
        scores[(size_t)rows[e] * n_items + items[e]] = -FLT_MAX;
}

// one workgroup per target: rank = #{j: s_j > s_t} + (#{j: s_j == s_t} + 1) / 2
// (= scipy.stats.rankdata(-scores)[t], method 'average': ties share the mean of their ranks)
__global__ __launch_bounds__(256) void k_eval_rank(const float *scores, int64_t n_items, const int64_t *rows,
                                                   const int64_t *items, int64_t n, double *rank) {
    __shared__ unsigned long long s_gt[256], s_eq[256];
    for (int64_t t = blockIdx.x; t < n; t += gridDim.x) {
        const float *row = scores + (size_t)rows[t] * n_items;
        const float st = row[items[t]];
        unsigned long long gt = 0, eq = 0;
        for (int64_t j = threadIdx.x; j < n_items; j += 256) {
            const float s = row[j];
            gt += s > st;
            eq += s == st;
        }
        s_gt[threadIdx.x] = gt;
        s_eq[threadIdx.x] = eq;
        __syncthreads();
        for (int off = 128; off >= 1; off >>= 1) {
            if ((int)threadIdx.x < off) {
                s_gt[threadIdx.x] += s_gt[threadIdx.x + off];
                s_eq[threadIdx.x] += s_eq[threadIdx.x + off];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) rank[t] = (double)s_gt[0] + ((double)s_eq[0] + 1.0) * 0.5;
        __syncthreads();
    }
}


// SELECT, second stage: row r's n_chunks * k keys -> its k best, best first, decoded.  One wave per row: the keys stream
// through the same threshold + candidate buffer + compaction as in the sweep.
#define SLK_TOPK_MERGE_CAP 256
__global__ __launch_bounds__(256) void k_topk_merge(const slk_key *cand, int64_t n_rows, int64_t per_row, int k, int64_t *items_out,
                                                    float *scores_out) {
    constexpr int CAP = SLK_TOPK_MERGE_CAP;
    __shared__ slk_key s_c[4][CAP];
    __shared__ slk_key s_thr[4];
    __shared__ unsigned s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n_rows; r += (int64_t)gridDim.x * 4) {
        if (lane == 0) {
            s_thr[wave] = 0ull;
            s_cnt[wave] = 0u;
        }
        SLK_SUBWAVE_SYNC();
        const slk_key *src = cand + (size_t)r * per_row;
        for (int64_t base = 0; base < per_row; base += 64) {
            const slk_key key = base + lane < per_row ? src[base + lane] : 0ull;
            if (key > s_thr[wave]) s_c[wave][atomicAdd(&s_cnt[wave], 1u)] = key;
            SLK_SUBWAVE_SYNC();
            const unsigned c = s_cnt[wave];
            SLK_SUBWAVE_SYNC();  // (every lane has read the count before the next piece's first candidate moves it)
            if (c > (unsigned)(CAP - 64)) slk_topk_compact(s_c[wave], c, k, CAP, lane, &s_thr[wave], &s_cnt[wave]);
        }
        slk_topk_compact(s_c[wave], s_cnt[wave], k, CAP, lane, &s_thr[wave], &s_cnt[wave]);  // sorted, empty slots last
        for (int i = lane; i < k; i += 64) {
            const slk_key key = s_c[wave][i];
            items_out[(size_t)r * k + i] = key ? (int64_t)(~(unsigned)key) : (int64_t)-1;
            scores_out[(size_t)r * k + i] = key ? slk_topk_score((unsigned)(key >> 32)) : -INFINITY;
        }
        SLK_SUBWAVE_SYNC();
    }
}

// *bad = 1 unless 0 <= exc_off[0] <= exc_off[1] <= ... <= exc_off[n]
__global__ __launch_bounds__(256) void k_topk_check_offsets(const int64_t *exc_off, int64_t n, int *bad) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256)
        if (exc_off[g] < 0 || exc_off[g + 1] < exc_off[g]) *bad = 1;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
typedef void (*gemm_fn)(slk_gemm_args);

// the rows' representations: group g's is row gmap[g] (nullptr: g) of rep / rbias (rbias nullptr: no row bias, PoolNet)
struct eval_rows {
    const float *rep, *rbias;
    const int64_t *gmap;
};

// the groups' exclusion lists: group g's excluded items are items[off[g] .. off[g + 1]) (off nullptr: none)
struct eval_exc {
    const int64_t *off, *items;
};

// the swept table: an slk_tables' item side, or any dense table with its rows' factors (or nullptr) where the item biases go
// (the neighbour entries)
struct eval_table {
    const float *V, *bi;
    const slk_bloom *bloom;
    int D;
    int64_t I;
};

static eval_table item_table(const slk_tables *t) {
    return {(const float *)t->d_param[1], (const float *)t->d_param[3], t->item_bloom, t->dim, t->num_items};
}

// the sweep's arguments for R rows (row r = group r) against the table; what the MODE reads or writes is the caller's to add
static slk_gemm_args sweep_args(const eval_table &t, const eval_rows &rows, int64_t R) {
    slk_gemm_args a;
    memset(&a, 0, sizeof(a));
    a.rep = rows.rep;
    a.rbias = rows.rbias;
    a.gmap = rows.gmap;
    a.R = R;
    slk_bloom_to_dev(t.bloom, &a.ib);
    a.V = t.V;
    a.bi = t.bi;
    a.D = t.D;
    a.I = t.I;
    return a;
}

// areg: the representations' operand in registers for the whole sweep (plain tables of dim <= 64)
template <int MODE>
static gemm_fn gemm_kernel(int mt, bool vec4, bool areg) {
    if (areg) return mt == 1 ? k_score_gemm<1, MODE, true, true> : k_score_gemm<2, MODE, true, true>;
    if (mt == 1) return vec4 ? k_score_gemm<1, MODE, true, false> : k_score_gemm<1, MODE, false, false>;
    return vec4 ? k_score_gemm<2, MODE, true, false> : k_score_gemm<2, MODE, false, false>;
}

// k_score_gemm for a MODE (SLK_GEMM_*), a tile of 32 * mt rows and the table of `a`, granted `lds` bytes of LDS
static int gemm_kernel_for(slk_ctx *ctx, int mode, const slk_gemm_args &a, int mt, size_t lds, gemm_fn *fn) {
    const bool vec4 = a.ib.n_hash == 0 && a.D % 4 == 0;
    const bool areg = vec4 && a.D <= SLK_GEMM_KC;
    switch (mode) {
        case SLK_GEMM_WRITE: *fn = gemm_kernel<SLK_GEMM_WRITE>(mt, vec4, areg); break;
        case SLK_GEMM_COUNT: *fn = gemm_kernel<SLK_GEMM_COUNT>(mt, vec4, areg); break;
        case SLK_GEMM_SELECT: *fn = gemm_kernel<SLK_GEMM_SELECT>(mt, vec4, areg); break;
        case SLK_GEMM_NBR_WRITE: *fn = gemm_kernel<SLK_GEMM_NBR_WRITE>(mt, vec4, areg); break;
        default: *fn = gemm_kernel<SLK_GEMM_NBR_SELECT>(mt, vec4, areg); break;
    }
    if (lds > 48 * 1024) SLK_HIP(ctx, hipFuncSetAttribute((const void *)*fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return SLK_OK;
}

// LDS of k_score_gemm without the SELECT modes' candidates: the row tile, one staged block, the tile's biases and targets
static size_t gemm_lds(int mt) { return ((size_t)(32 * mt + SLK_GEMM_IB) * SLK_GEMM_KS + 4 * 32 * mt) * 4; }

// items per workgroup of a sweep of I items for `rows` rows in tiles of `rt`: the option's value (0: the automatic cut), else
// enough workgroups for the chip (~4 per CU over all row tiles; 2 per CU for a single row tile, whose workgroups are all
// resident at once: longer sweeps amortise a workgroup's first, unhidden block); whole blocks of `block` items
static int64_t sweep_cut(int64_t I, int64_t rows, int rt, int64_t opt, int num_cus, int block) {
    const int64_t row_tiles = (rows + rt - 1) / rt;
    int64_t want = ((row_tiles == 1 ? 2 : 4) * (int64_t)num_cus + row_tiles - 1) / row_tiles;
    if (want < 1) want = 1;
    const int64_t per = opt > 0 ? opt : (I + want - 1) / want;
    return (per + block - 1) / block * block;
}

// one sweep of the table per tile of 32 * mt rows in MODE WRITE / NBR_WRITE (store a.out) or COUNT (compare with a.st and add
// into a.gt / a.eq); `a` from sweep_args.  (The SELECT modes tile their rows themselves: topk_run.)
static int eval_gemm(slk_ctx *ctx, int mode, slk_gemm_args a, hipStream_t s) {
    if (a.R <= 0 || a.I <= 0) return SLK_OK;
    if (mode == SLK_GEMM_WRITE && a.R <= 8 && a.ib.n_hash == 0 && a.D % 4 == 0) {
        // a handful of rows: the streaming form (k_score_rows), two workgroups per CU each sweeping whole blocks of 256 items
        // (option "eval_items_per_wg": the cut given, a test and measurement switch)
        const int64_t per = sweep_cut(a.I, a.R, 8, ctx->opt_eval_items_per_wg, ctx->num_cus, SLK_ROWS_IB);
        a.items_per_wg = per;
        const int nr = a.R == 1 ? 1 : (a.R == 2 ? 2 : (a.R <= 4 ? 4 : 8));
        const size_t lds = ((size_t)SLK_ROWS_IB * SLK_GEMM_KS + (size_t)nr * SLK_GEMM_KC + nr) * 4;
        gemm_fn fn = nr == 1 ? k_score_rows<1> : (nr == 2 ? k_score_rows<2> : (nr == 4 ? k_score_rows<4> : k_score_rows<8>));
        SLK_HIP(ctx, hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(fn, dim3((unsigned)((a.I + per - 1) / per)), dim3(256), lds, s, a);
        SLK_LAUNCH_CHECK(ctx, "k_score_rows");
        return SLK_OK;
    }
    // rows per workgroup: 64 (the item rows are streamed once per row tile; a 128-row tile was measured out: its four
    // accumulator tiles + the staged block leave no room for three workgroups per CU, and the sweep is bound by how many
    // blocks the CU has in flight), 32 for a handful (predict: one row -- a 32-row tile keeps the matrix-core time below the
    // table's streaming time)
    const int mt = a.R > 32 ? 2 : 1;
    const int64_t row_tiles = (a.R + 32 * mt - 1) / (32 * mt);
    int64_t per = sweep_cut(a.I, a.R, 32 * mt, ctx->opt_eval_items_per_wg, ctx->num_cus, SLK_GEMM_IB);
    if (per > ((int64_t)1 << 22)) per = (int64_t)1 << 22;  // (the packed per-lane counters hold 2^16 - 1 columns: 2^23 items)
    a.items_per_wg = per;
    const int64_t chunks = (a.I + per - 1) / per;
    if (row_tiles > 65535) return slk_fail(ctx, SLK_EINVAL, "scoring: %lld rows per call, at most %d", (long long)a.R, 65535 * 32 * mt);
    size_t lds = gemm_lds(mt);
    // two resident workgroups per CU, by LDS footprint: the registers would allow three, and three share the LDS bandwidth and
    // the L2 worse (4096 x 10^6: 8.3 ms against 7.06, profiles/r04_h_bench_eval_{2,3}wg.json)
    // (the pad is half of the CU's LDS as the DEVICE reports it -- 160 KB on gfx950 -- and is skipped where a workgroup cannot be
    // granted that much: never more than the device can give)
    if (lds > ctx->lds_per_block)
        return slk_fail(ctx, SLK_EINVAL, "scoring: the sweep needs %zu B of LDS per workgroup, the device grants %zu", lds, ctx->lds_per_block);
    const size_t half_lds = ctx->lds_per_cu / 2 - 256;
    if (lds < half_lds && half_lds <= ctx->lds_per_block) lds = half_lds;
    int rc;
    gemm_fn fn;
    if ((rc = gemm_kernel_for(ctx, mode, a, mt, lds, &fn))) return rc;
    hipLaunchKernelGGL(fn, dim3((unsigned)chunks, (unsigned)row_tiles), dim3(256), lds, s, a);
    SLK_LAUNCH_CHECK(ctx, "k_score_gemm");
    return SLK_OK;
}

// out[r][i]: R rows against every row of the table (MODE WRITE, or NBR_WRITE with the neighbour epilogue)
static int eval_scores(slk_ctx *ctx, int mode, const eval_table &t, const eval_rows &rows, int64_t R, float *d_out, hipStream_t s) {
    slk_gemm_args a = sweep_args(t, rows, R);
    a.out = d_out;
    return eval_gemm(ctx, mode, a, s);
}

// The rows' representations.  Plain user table: the table itself, addressed through the ids (gmap = d_users; no kernel, no
// copy).  BloomEmbedding user table: the hashed rows are summed into scratch first (gmap = NULL).
static int eval_user_rows(slk_ctx *ctx, const slk_tables *tables, int vec, int g, const int64_t *d_users, int64_t n_users,
                          eval_rows *rows, hipStream_t s) {
    int rc;
    if (!tables->user_bloom || tables->user_bloom->n_hash == 0) {
        *rows = {(const float *)tables->d_param[0], (const float *)tables->d_param[2], d_users};
        return SLK_OK;
    }
    const int D = tables->dim;
    if ((rc = slk_ensure(ctx, ctx->extra[EV_REP], (size_t)n_users * D * 4))) return rc;
    if ((rc = slk_ensure(ctx, ctx->extra[EV_RBIAS], (size_t)n_users * 4))) return rc;
    float *rep_w = (float *)ctx->extra[EV_REP].p, *rbias_w = (float *)ctx->extra[EV_RBIAS].p;
    *rows = {rep_w, rbias_w, nullptr};
    slk_bloom_dev ubd;
    slk_bloom_to_dev(tables->user_bloom, &ubd);
#define SLK_ROWS(V_, G_)                                                                                          \
    hipLaunchKernelGGL((k_eval_user_rows<V_, G_>), dim3(slk_grid_for(ctx, (size_t)n_users, 256 / G_)), dim3(256), 0, s, \
                       (const float *)tables->d_param[0], (const float *)tables->d_param[2], ubd, D, d_users,      \
                       n_users, rep_w, rbias_w)
    SLK_FOR_LAYOUT(vec, g, SLK_ROWS);
#undef SLK_ROWS
    SLK_LAUNCH_CHECK(ctx, "k_eval_user_rows");
    return SLK_OK;
}

static int eval_seq_rows(slk_ctx *ctx, const slk_tables *tables, int vec, int g, const int64_t *d_sequences, int64_t n_seq,
                         int64_t seq_len, eval_rows *rows, hipStream_t s) {
    int rc;
    const int D = tables->dim;
    if ((rc = slk_ensure(ctx, ctx->extra[EV_REP], (size_t)n_seq * D * 4))) return rc;
    float *rep_w = (float *)ctx->extra[EV_REP].p;
    *rows = {rep_w, nullptr, nullptr};
    slk_bloom_dev ibd;
    slk_bloom_to_dev(tables->item_bloom, &ibd);
#define SLK_ROWS(V_, G_)                                                                                         \
    hipLaunchKernelGGL((k_eval_seq_rows<V_, G_>), dim3(slk_grid_for(ctx, (size_t)n_seq, 256 / G_)), dim3(256), 0, s, \
                       (const float *)tables->d_param[1], ibd, D, d_sequences, n_seq, (int)seq_len, rep_w)
    SLK_FOR_LAYOUT(vec, g, SLK_ROWS);
#undef SLK_ROWS
    SLK_LAUNCH_CHECK(ctx, "k_eval_seq_rows");
    return SLK_OK;
}

SLK_EXPORT int slk_bilinear_scores(slk_ctx *ctx, const slk_tables *tables, const int64_t *d_users, int64_t n_users,
                                   float *d_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = slk_check_tables(ctx, tables, 15u, &vec, &g))) return rc;
    if (n_users < 0 || (n_users > 0 && (!d_users || !d_out))) return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_scores: bad arguments");
    if (n_users == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    eval_rows rows;
    if ((rc = eval_user_rows(ctx, tables, vec, g, d_users, n_users, &rows, call.s))) return rc;
    return eval_scores(ctx, SLK_GEMM_WRITE, item_table(tables), rows, n_users, d_out, call.s);
}

SLK_EXPORT int slk_poolnet_scores(slk_ctx *ctx, const slk_tables *tables, const int64_t *d_sequences, int64_t n_seq,
                                  int64_t seq_len, float *d_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = slk_check_tables(ctx, tables, 10u, &vec, &g))) return rc;
    if (n_seq < 0 || seq_len < 1 || (n_seq > 0 && (!d_sequences || !d_out)))
        return slk_fail(ctx, SLK_EINVAL, "slk_poolnet_scores: bad arguments");
    if (n_seq == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    eval_rows rows;
    if ((rc = eval_seq_rows(ctx, tables, vec, g, d_sequences, n_seq, seq_len, &rows, call.s))) return rc;
    return eval_scores(ctx, SLK_GEMM_WRITE, item_table(tables), rows, n_seq, d_out, call.s);
}

// Fused ranking: rank_out[r] = rankdata(-scores(group row_group[r]) with the group's exclusions pushed last)[row_target[r]]
// without a score matrix, in three stages: the target scores (vector unit), ONE counting sweep of the item table per 64 rows
// (matrix cores) with the exclusion lists' corrections (vector unit), and the counts' way out.  rows: the groups'
// representations.  The one-device entries run the stages back to back (rank_fused); the sharded entries run the first two on
// ONE RANK's item rows with a collective of the host's after each (slk_shard_target_scores / slk_shard_rank_counts).
struct rank_counters {
    unsigned *gt, *eq;  // the sweep's counts
    int *dgt, *deq;     // the exclusion lists' signed corrections
};

static int rank_scratch(slk_ctx *ctx, int64_t n_rows, bool want_st, float **st, rank_counters *c) {
    int rc;
    if (want_st) {
        if ((rc = slk_ensure(ctx, ctx->extra[EV_ST], (size_t)n_rows * 4))) return rc;
        *st = (float *)ctx->extra[EV_ST].p;
    }
    if ((rc = slk_ensure(ctx, ctx->extra[EV_CNT], (size_t)n_rows * 16))) return rc;
    c->gt = (unsigned *)ctx->extra[EV_CNT].p;
    c->eq = c->gt + n_rows;
    c->dgt = (int *)(c->eq + n_rows);
    c->deq = c->dgt + n_rows;
    return SLK_OK;
}

// stage 1: st[r] = the score of row r's target (-FLT_MAX where the target is on its group's exclusion list; `shard`: -INFINITY
// where d_row_target[r] is no row of these tables)
static int rank_target_scores(slk_ctx *ctx, const slk_tables *tables, int vec, int g, const eval_rows &rows,
                              const int64_t *d_row_group, const int64_t *d_row_target, int64_t n_rows, const eval_exc &exc,
                              bool shard, float *st, hipStream_t s) {
    const slk_gemm_args a = sweep_args(item_table(tables), rows, n_rows);
#define SLK_TGT(V_, G_)                                                                                                      \
    do {                                                                                                                     \
        if (shard)                                                                                                           \
            hipLaunchKernelGGL((k_rank_target_scores<V_, G_, true>), dim3(slk_grid_for(ctx, (size_t)n_rows, 256 / G_)),      \
                               dim3(256), 0, s, a.rep, a.rbias, d_row_group, a.gmap, a.V, a.bi, a.ib, a.D, a.I, d_row_target, \
                               exc.off, exc.items, n_rows, st);                                                              \
        else                                                                                                                 \
            hipLaunchKernelGGL((k_rank_target_scores<V_, G_, false>), dim3(slk_grid_for(ctx, (size_t)n_rows, 256 / G_)),     \
                               dim3(256), 0, s, a.rep, a.rbias, d_row_group, a.gmap, a.V, a.bi, a.ib, a.D, a.I, d_row_target, \
                               exc.off, exc.items, n_rows, st);                                                              \
    } while (0)
    SLK_FOR_LAYOUT(vec, g, SLK_TGT);
#undef SLK_TGT
    SLK_LAUNCH_CHECK(ctx, "k_rank_target_scores");
    return SLK_OK;
}

// stage 2: c.gt / c.eq = #{items of these tables scoring > / == st[r]}; c.dgt / c.deq (written iff exc.off): what pushing the
// exclusion list's items of these tables to -FLT_MAX changes of them
static int rank_counts(slk_ctx *ctx, const slk_tables *tables, int vec, int g, const eval_rows &rows, const int64_t *d_row_group,
                       int64_t n_rows, const eval_exc &exc, const float *st, const rank_counters &c, hipStream_t s) {
    int rc;
    SLK_HIP(ctx, hipMemsetAsync(c.gt, 0, (size_t)n_rows * 8, s));
    slk_gemm_args a = sweep_args(item_table(tables), rows, n_rows);
    a.rowmap = d_row_group;
    a.st = st;
    a.gt = c.gt;
    a.eq = c.eq;
    if ((rc = eval_gemm(ctx, SLK_GEMM_COUNT, a, s))) return rc;
    if (exc.off) {
#define SLK_EXC(V_, G_)                                                                                             \
    hipLaunchKernelGGL((k_rank_exclusions<V_, G_>), dim3(slk_grid_for(ctx, (size_t)n_rows, 256 / G_)), dim3(256), 0, s, a.rep, \
                       a.rbias, d_row_group, a.gmap, a.V, a.bi, a.ib, a.D, exc.off, exc.items, st, n_rows, c.dgt, c.deq)
        SLK_FOR_LAYOUT(vec, g, SLK_EXC);
#undef SLK_EXC
        SLK_LAUNCH_CHECK(ctx, "k_rank_exclusions");
    }
    return SLK_OK;
}

static int rank_fused(slk_ctx *ctx, const slk_tables *tables, int vec, int g, const eval_rows &rows, const int64_t *d_row_group,
                      const int64_t *d_row_target, int64_t n_rows, const eval_exc &exc, double *d_rank_out, hipStream_t s) {
    int rc;
    float *st = nullptr;
    rank_counters c;
    if ((rc = rank_scratch(ctx, n_rows, true, &st, &c))) return rc;
    if ((rc = rank_target_scores(ctx, tables, vec, g, rows, d_row_group, d_row_target, n_rows, exc, false, st, s))) return rc;
    if ((rc = rank_counts(ctx, tables, vec, g, rows, d_row_group, n_rows, exc, st, c, s))) return rc;
    hipLaunchKernelGGL(k_rank_final, dim3(slk_grid_for(ctx, (size_t)n_rows, 256)), dim3(256), 0, s, (const unsigned *)c.gt,
                       (const unsigned *)c.eq, exc.off ? (const int *)c.dgt : (const int *)nullptr,
                       exc.off ? (const int *)c.deq : (const int *)nullptr, n_rows, d_rank_out);
    SLK_LAUNCH_CHECK(ctx, "k_rank_final");
    return SLK_OK;
}

// (exc.off without exc.items is NOT refused here: an empty torch tensor's data_ptr() is 0, so all-empty lists arrive that way)
static int check_rank_args(slk_ctx *ctx, const char *who, int64_t n_groups, const void *groups, const int64_t *d_row_group,
                           const int64_t *d_row_target, int64_t n_rows, const double *d_rank_out) {
    if (n_groups < 0 || n_rows < 0 || (n_groups > 0 && !groups) || (n_rows > 0 && (!d_row_group || !d_row_target || !d_rank_out)))
        return slk_fail(ctx, SLK_EINVAL, "%s: bad arguments", who);
    if (n_rows > 0 && n_groups == 0) return slk_fail(ctx, SLK_EINVAL, "%s: rows without groups", who);
    return SLK_OK;
}

SLK_EXPORT int slk_bilinear_rank(slk_ctx *ctx, const slk_tables *tables, const int64_t *d_group_users, int64_t n_groups,
                                 const int64_t *d_row_group, const int64_t *d_row_target, int64_t n_rows,
                                 const int64_t *d_exc_off, const int64_t *d_exc_items, double *d_rank_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = slk_check_tables(ctx, tables, 15u, &vec, &g))) return rc;
    if ((rc = check_rank_args(ctx, "slk_bilinear_rank", n_groups, d_group_users, d_row_group, d_row_target, n_rows, d_rank_out))) return rc;
    if (n_rows == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    eval_rows rows;
    if ((rc = eval_user_rows(ctx, tables, vec, g, d_group_users, n_groups, &rows, call.s))) return rc;
    return rank_fused(ctx, tables, vec, g, rows, d_row_group, d_row_target, n_rows, {d_exc_off, d_exc_items}, d_rank_out, call.s);
}

SLK_EXPORT int slk_poolnet_rank(slk_ctx *ctx, const slk_tables *tables, const int64_t *d_group_sequences, int64_t n_groups,
                                int64_t seq_len, const int64_t *d_row_group, const int64_t *d_row_target, int64_t n_rows,
                                const int64_t *d_exc_off, const int64_t *d_exc_items, double *d_rank_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = slk_check_tables(ctx, tables, 10u, &vec, &g))) return rc;
    if (seq_len < 1) return slk_fail(ctx, SLK_EINVAL, "slk_poolnet_rank: seq_len %lld", (long long)seq_len);
    if ((rc = check_rank_args(ctx, "slk_poolnet_rank", n_groups, d_group_sequences, d_row_group, d_row_target, n_rows, d_rank_out)))
        return rc;
    if (n_rows == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    eval_rows rows;
    if ((rc = eval_seq_rows(ctx, tables, vec, g, d_group_sequences, n_groups, seq_len, &rows, call.s))) return rc;
    return rank_fused(ctx, tables, vec, g, rows, d_row_group, d_row_target, n_rows, {d_exc_off, d_exc_items}, d_rank_out, call.s);
}

// ---- sharded evaluation: one rank's item rows against caller-supplied representations ----------------------------------------
// (include/spotlight_hip.h: the item side of `local` only -- a group's user row usually lives on another rank, so the
// representations come as dense arrays.  The counts are integers: their sum over the ranks is the one-device count.)
static int check_shard_eval(slk_ctx *ctx, const char *who, const slk_tables *local, const float *d_rep, const float *d_rbias,
                            int64_t n_rep, int *vec, int *g) {
    if (local && local->item_bloom)
        return slk_fail(ctx, SLK_EINVAL, "%s: a bloom item table cannot be row-sharded (plain tables only)", who);
    int rc;
    if ((rc = slk_check_tables(ctx, local, 10u, vec, g))) return rc;  // (item side: refuses item biases inside a bias-shadow scope)
    if (n_rep < 0) return slk_fail(ctx, SLK_EINVAL, "%s: bad arguments", who);
    if (n_rep > 0 && (!d_rep || !d_rbias)) return slk_fail(ctx, SLK_EINVAL, "%s: the representations (d_rep / d_rbias) are NULL", who);
    return SLK_OK;
}

SLK_EXPORT int slk_shard_target_scores(slk_ctx *ctx, const slk_tables *local, const float *d_rep, const float *d_rbias,
                                       int64_t n_groups, const int64_t *d_row_group, const int64_t *d_row_target_local,
                                       int64_t n_rows, const int64_t *d_exc_off, const int64_t *d_exc_items_local,
                                       float *d_st_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = check_shard_eval(ctx, "slk_shard_target_scores", local, d_rep, d_rbias, n_groups, &vec, &g))) return rc;
    if (n_rows < 0 || (n_rows > 0 && (!d_row_group || !d_row_target_local || !d_st_out)))
        return slk_fail(ctx, SLK_EINVAL, "slk_shard_target_scores: bad arguments");
    if (n_rows > 0 && n_groups == 0) return slk_fail(ctx, SLK_EINVAL, "slk_shard_target_scores: rows without groups");
    if (n_rows == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    return rank_target_scores(ctx, local, vec, g, {d_rep, d_rbias, nullptr}, d_row_group, d_row_target_local, n_rows,
                              {d_exc_off, d_exc_items_local}, true, d_st_out, call.s);
}

SLK_EXPORT int slk_shard_rank_counts(slk_ctx *ctx, const slk_tables *local, const float *d_rep, const float *d_rbias,
                                     int64_t n_groups, const int64_t *d_row_group, const float *d_st, int64_t n_rows,
                                     const int64_t *d_exc_off, const int64_t *d_exc_items_local, int64_t *d_gt_out,
                                     int64_t *d_eq_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = check_shard_eval(ctx, "slk_shard_rank_counts", local, d_rep, d_rbias, n_groups, &vec, &g))) return rc;
    if (n_rows < 0 || (n_rows > 0 && (!d_row_group || !d_st || !d_gt_out || !d_eq_out)))
        return slk_fail(ctx, SLK_EINVAL, "slk_shard_rank_counts: bad arguments");
    if (n_rows > 0 && n_groups == 0) return slk_fail(ctx, SLK_EINVAL, "slk_shard_rank_counts: rows without groups");
    if (n_rows == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    hipStream_t s = call.s;
    rank_counters c;
    if ((rc = rank_scratch(ctx, n_rows, false, nullptr, &c))) return rc;
    if ((rc = rank_counts(ctx, local, vec, g, {d_rep, d_rbias, nullptr}, d_row_group, n_rows, {d_exc_off, d_exc_items_local}, d_st, c, s)))
        return rc;
    hipLaunchKernelGGL(k_rank_counts_out, dim3(slk_grid_for(ctx, (size_t)n_rows, 256)), dim3(256), 0, s, (const unsigned *)c.gt,
                       (const unsigned *)c.eq, d_exc_off ? (const int *)c.dgt : (const int *)nullptr,
                       d_exc_off ? (const int *)c.deq : (const int *)nullptr, n_rows, d_gt_out, d_eq_out);
    SLK_LAUNCH_CHECK(ctx, "k_rank_counts_out");
    return SLK_OK;
}

SLK_EXPORT int slk_shard_scores(slk_ctx *ctx, const slk_tables *local, const float *d_rep, const float *d_rbias, int64_t n_rows,
                                float *d_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = check_shard_eval(ctx, "slk_shard_scores", local, d_rep, d_rbias, n_rows, &vec, &g))) return rc;
    if (n_rows > 0 && !d_out) return slk_fail(ctx, SLK_EINVAL, "slk_shard_scores: bad arguments");
    if (n_rows == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    return eval_scores(ctx, SLK_GEMM_WRITE, item_table(local), {d_rep, d_rbias, nullptr}, n_rows, d_out, call.s);
}

// ---- top-k: MODE SELECT of the sweep + k_topk_merge ------------------------------------------------------------------------------
#define SLK_TOPK_SCRATCH_BYTES ((size_t)64 << 20)  // candidate scratch of one launch (rows are processed in tiles to stay below it)

static size_t topk_lds(int mt, int cap) { return gemm_lds(mt) + (size_t)32 * mt * ((size_t)cap * 8 + 32); }

// the top k of R rows (row r = group r, exc.off[R + 1]) against the table; mode: SLK_GEMM_SELECT or SLK_GEMM_NBR_SELECT
static int topk_run(slk_ctx *ctx, const char *who, int mode, const eval_table &t, const eval_rows &rows, int64_t R, int64_t k,
                    const eval_exc &exc, int64_t *d_items_out, float *d_scores_out, hipStream_t s) {
    int rc;
    const int64_t I = t.I;
    if (I <= 0) return slk_fail(ctx, SLK_EINVAL, "%s: no items", who);
    if (I >= ((int64_t)1 << 32) - 1) return slk_fail(ctx, SLK_EINVAL, "%s: %lld items, ids must fit 32 bits", who, (long long)I);
    if (exc.off) {
        // the offsets index exc.items inside the sweep: checked here, the one host wait of the call
        if ((rc = slk_ensure(ctx, ctx->extra[EV_TOPK_FLAG], sizeof(int)))) return rc;
        int *d_bad = (int *)ctx->extra[EV_TOPK_FLAG].p, h_bad = 0;
        SLK_HIP(ctx, hipMemsetAsync(d_bad, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_topk_check_offsets, dim3(slk_grid_for(ctx, (size_t)R, 256)), dim3(256), 0, s, exc.off, R, d_bad);
        SLK_LAUNCH_CHECK(ctx, "k_topk_check_offsets");
        SLK_HIP(ctx, hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
        SLK_HIP(ctx, hipStreamSynchronize(s));
        if (h_bad) return slk_fail(ctx, SLK_EINVAL, "%s: d_exc_off is not sorted (offsets must start at >= 0 and never decrease)", who);
    }
    // the row tile: 64 rows where their candidate slots fit beside the operands (small k), else 32; every slot the LDS has
    // left (up to 512) goes to the candidates: the more slack above k + SLK_GEMM_IB, the fewer compactions
    int mt = 0, cap = 0;
    for (int m = R > 32 ? 2 : 1; m >= 1 && !mt; --m) {
        const size_t base = topk_lds(m, 0);
        if (ctx->lds_per_block <= base) continue;
        size_t c = (ctx->lds_per_block - base) / ((size_t)32 * m * 8);
        if (c > 512) c = 512;
        if ((int64_t)c >= k + SLK_GEMM_IB) {
            mt = m;
            cap = (int)c;
        }
    }
    if (!mt) return slk_fail(ctx, SLK_EINVAL, "%s: k = %lld does not fit the device's %zu B of LDS per workgroup", who, (long long)k, ctx->lds_per_block);
    const int RT = 32 * mt;
    slk_gemm_args a = sweep_args(t, rows, R);
    a.k = (int)k;
    a.cap = cap;
    a.exc_items = exc.items;
    const size_t lds = topk_lds(mt, cap);
    gemm_fn fn;
    if ((rc = gemm_kernel_for(ctx, mode, a, mt, lds, &fn))) return rc;
    int64_t row_step = 16384;
    for (int64_t r_lo = 0; r_lo < R; r_lo += row_step) {
        int64_t n = R - r_lo < row_step ? R - r_lo : row_step;
        // item chunks: the option's, else as eval_gemm cuts them (~4 workgroups per CU over all row tiles)
        const int64_t per = sweep_cut(I, n, RT, ctx->opt_topk_items_per_wg, ctx->num_cus, SLK_GEMM_IB);
        const int64_t chunks = (I + per - 1) / per;
        if (chunks > 0x7fffffff) return slk_fail(ctx, SLK_EINVAL, "%s: %lld item chunks per row tile", who, (long long)chunks);
        // rows of this launch: as many whole tiles as keep the candidate scratch bounded
        const size_t row_bytes = (size_t)chunks * (size_t)k * 8;
        if ((size_t)n * row_bytes > SLK_TOPK_SCRATCH_BYTES) {
            int64_t fit = (int64_t)(SLK_TOPK_SCRATCH_BYTES / row_bytes) / RT * RT;
            if (fit < RT) fit = RT;
            if (fit < n) n = fit;
            row_step = n;
        }
        if ((rc = slk_ensure(ctx, ctx->extra[EV_TOPK], (size_t)n * row_bytes))) return rc;
        a.cand = (slk_key *)ctx->extra[EV_TOPK].p;
        a.items_per_wg = per;
        a.R = n;
        a.rep = rows.gmap ? rows.rep : rows.rep + (size_t)r_lo * t.D;
        a.rbias = (rows.gmap || !rows.rbias) ? rows.rbias : rows.rbias + r_lo;
        a.gmap = rows.gmap ? rows.gmap + r_lo : nullptr;
        a.exc_off = exc.off ? exc.off + r_lo : nullptr;
        hipLaunchKernelGGL(fn, dim3((unsigned)chunks, (unsigned)((n + RT - 1) / RT)), dim3(256), lds, s, a);
        SLK_LAUNCH_CHECK(ctx, "k_score_gemm<SELECT>");
        hipLaunchKernelGGL(k_topk_merge, dim3(slk_grid_for(ctx, (size_t)n, 4)), dim3(256), 0, s, (const slk_key *)a.cand, n,
                           chunks * k, (int)k, d_items_out + (size_t)r_lo * k, d_scores_out + (size_t)r_lo * k);
        SLK_LAUNCH_CHECK(ctx, "k_topk_merge");
    }
    return SLK_OK;
}

static int check_topk_args(slk_ctx *ctx, const char *who, int64_t n_rows, const void *rows, int64_t k, const int64_t *d_exc_off,
                           const int64_t *d_exc_items, const int64_t *d_items_out, const float *d_scores_out) {
    if (k < 1) return slk_fail(ctx, SLK_EINVAL, "%s: k = %lld, at least 1", who, (long long)k);
    if (k > SLK_TOPK_K_MAX) return slk_fail(ctx, SLK_EINVAL, "%s: k = %lld, at most SLK_TOPK_K_MAX = %d", who, (long long)k, SLK_TOPK_K_MAX);
    if (n_rows < 0 || (n_rows > 0 && !rows) || (d_exc_off && !d_exc_items)) return slk_fail(ctx, SLK_EINVAL, "%s: bad arguments", who);
    if (n_rows > 0 && (!d_items_out || !d_scores_out)) return slk_fail(ctx, SLK_EINVAL, "%s: the outputs (d_items_out / d_scores_out) are NULL", who);
    return SLK_OK;
}

SLK_EXPORT int slk_bilinear_topk(slk_ctx *ctx, const slk_tables *tables, const int64_t *d_users, int64_t n_users, int64_t k,
                                 const int64_t *d_exc_off, const int64_t *d_exc_items, int64_t *d_items_out, float *d_scores_out,
                                 void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = slk_check_tables(ctx, tables, 15u, &vec, &g))) return rc;
    if ((rc = check_topk_args(ctx, "slk_bilinear_topk", n_users, d_users, k, d_exc_off, d_exc_items, d_items_out, d_scores_out))) return rc;
    if (n_users == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    eval_rows rows;
    if ((rc = eval_user_rows(ctx, tables, vec, g, d_users, n_users, &rows, call.s))) return rc;
    return topk_run(ctx, "slk_bilinear_topk", SLK_GEMM_SELECT, item_table(tables), rows, n_users, k, {d_exc_off, d_exc_items},
                    d_items_out, d_scores_out, call.s);
}

SLK_EXPORT int slk_poolnet_topk(slk_ctx *ctx, const slk_tables *tables, const int64_t *d_sequences, int64_t n_seq, int64_t seq_len,
                                int64_t k, const int64_t *d_exc_off, const int64_t *d_exc_items, int64_t *d_items_out,
                                float *d_scores_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = slk_check_tables(ctx, tables, 10u, &vec, &g))) return rc;
    if (seq_len < 1) return slk_fail(ctx, SLK_EINVAL, "slk_poolnet_topk: seq_len %lld", (long long)seq_len);
    if ((rc = check_topk_args(ctx, "slk_poolnet_topk", n_seq, d_sequences, k, d_exc_off, d_exc_items, d_items_out, d_scores_out))) return rc;
    if (n_seq == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    eval_rows rows;
    if ((rc = eval_seq_rows(ctx, tables, vec, g, d_sequences, n_seq, seq_len, &rows, call.s))) return rc;
    return topk_run(ctx, "slk_poolnet_topk", SLK_GEMM_SELECT, item_table(tables), rows, n_seq, k, {d_exc_off, d_exc_items},
                    d_items_out, d_scores_out, call.s);
}

SLK_EXPORT int slk_shard_topk(slk_ctx *ctx, const slk_tables *local, const float *d_rep, const float *d_rbias, int64_t n_rows,
                              int64_t k, const int64_t *d_exc_off, const int64_t *d_exc_items_local, int64_t *d_items_local_out,
                              float *d_scores_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = check_shard_eval(ctx, "slk_shard_topk", local, d_rep, d_rbias, n_rows, &vec, &g))) return rc;
    if ((rc = check_topk_args(ctx, "slk_shard_topk", n_rows, d_rep, k, d_exc_off, d_exc_items_local, d_items_local_out, d_scores_out)))
        return rc;
    if (n_rows == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    return topk_run(ctx, "slk_shard_topk", SLK_GEMM_SELECT, item_table(local), {d_rep, d_rbias, nullptr}, n_rows, k,
                    {d_exc_off, d_exc_items_local}, d_items_local_out, d_scores_out, call.s);
}

// ---- neighbours in the embedding space: rows of ANY dense table against dense query rows (the SCALE epilogue) -----------------
static int check_neighbor_args(slk_ctx *ctx, const char *who, const float *d_table, int64_t n_table_rows, int64_t dim,
                               const float *d_tscale, const float *d_queries, const float *d_qscale, int64_t n_q, int *vec, int *g) {
    if (!d_table) return slk_fail(ctx, SLK_EINVAL, "%s: d_table is NULL", who);
    if (n_table_rows <= 0) return slk_fail(ctx, SLK_EINVAL, "%s: no table rows (n_table_rows = %lld)", who, (long long)n_table_rows);
    if (n_table_rows >= ((int64_t)1 << 32) - 1)
        return slk_fail(ctx, SLK_EINVAL, "%s: %lld table rows, ids must fit 32 bits", who, (long long)n_table_rows);
    if (dim < 1) return slk_fail(ctx, SLK_EINVAL, "%s: dim = %lld, at least 1", who, (long long)dim);
    if (dim > 256 || !slk_pick_layout((int)dim, vec, g))
        return slk_fail(ctx, SLK_EINVAL, "%s: embedding dim %lld unsupported (need dim %% 4 == 0 and <= 256, or dim <= 64)", who, (long long)dim);
    if (n_q < 0 || (n_q > 0 && !d_queries)) return slk_fail(ctx, SLK_EINVAL, "%s: bad arguments (the queries)", who);
    if ((d_tscale == nullptr) != (d_qscale == nullptr))
        return slk_fail(ctx, SLK_EINVAL, "%s: d_tscale and d_qscale go together (both: cosine, neither: dot)", who);
    if (ctx->pp_active && (d_table == ctx->pp_src_u || (d_queries && d_queries == ctx->pp_src_u)))
        return slk_fail(ctx, SLK_EINVAL, "%s: the user rows of this table are ping-ponged (slk_user_pingpong_begin): the array holds only "
                                         "some of the current rows until slk_user_pingpong_end", who);
    return SLK_OK;
}

SLK_EXPORT int slk_rows_inv_norm(slk_ctx *ctx, const float *d_table, int64_t n_rows, int64_t dim, float *d_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if (n_rows < 0) return slk_fail(ctx, SLK_EINVAL, "slk_rows_inv_norm: n_rows = %lld", (long long)n_rows);
    if (dim < 1) return slk_fail(ctx, SLK_EINVAL, "slk_rows_inv_norm: dim = %lld, at least 1", (long long)dim);
    if (dim > 256 || !slk_pick_layout((int)dim, &vec, &g))
        return slk_fail(ctx, SLK_EINVAL, "slk_rows_inv_norm: embedding dim %lld unsupported (need dim %% 4 == 0 and <= 256, or dim <= 64)",
                        (long long)dim);
    if (n_rows == 0) return SLK_OK;
    if (!d_table || !d_out) return slk_fail(ctx, SLK_EINVAL, "slk_rows_inv_norm: d_table / d_out is NULL");
    if (ctx->pp_active && d_table == ctx->pp_src_u)
        return slk_fail(ctx, SLK_EINVAL, "slk_rows_inv_norm: the user rows of this table are ping-ponged (slk_user_pingpong_begin): the "
                                         "array holds only some of the current rows until slk_user_pingpong_end");
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
#define SLK_ROWS(V_, G_)                                                                                                 \
    hipLaunchKernelGGL((k_rows_inv_norm<V_, G_>), dim3(slk_grid_for(ctx, (size_t)n_rows, 256 / G_)), dim3(256), 0, call.s, d_table, \
                       (int)dim, n_rows, d_out)
    SLK_FOR_LAYOUT(vec, g, SLK_ROWS);
#undef SLK_ROWS
    SLK_LAUNCH_CHECK(ctx, "k_rows_inv_norm");
    return SLK_OK;
}

SLK_EXPORT int slk_neighbors_topk(slk_ctx *ctx, const float *d_table, int64_t n_table_rows, int64_t dim, const float *d_tscale,
                                  const float *d_queries, const float *d_qscale, int64_t n_q, int64_t k, const int64_t *d_exc_off,
                                  const int64_t *d_exc_items, int64_t *d_items_out, float *d_scores_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = check_topk_args(ctx, "slk_neighbors_topk", n_q, d_queries, k, d_exc_off, d_exc_items, d_items_out, d_scores_out))) return rc;
    if ((rc = check_neighbor_args(ctx, "slk_neighbors_topk", d_table, n_table_rows, dim, d_tscale, d_queries, d_qscale, n_q, &vec, &g)))
        return rc;
    if (n_q == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    return topk_run(ctx, "slk_neighbors_topk", SLK_GEMM_NBR_SELECT, {d_table, d_tscale, nullptr, (int)dim, n_table_rows},
                    {d_queries, d_qscale, nullptr}, n_q, k, {d_exc_off, d_exc_items}, d_items_out, d_scores_out, call.s);
}

SLK_EXPORT int slk_neighbors_scores(slk_ctx *ctx, const float *d_table, int64_t n_table_rows, int64_t dim, const float *d_tscale,
                                    const float *d_queries, const float *d_qscale, int64_t n_q, float *d_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = check_neighbor_args(ctx, "slk_neighbors_scores", d_table, n_table_rows, dim, d_tscale, d_queries, d_qscale, n_q, &vec, &g)))
        return rc;
    if (n_q > 0 && !d_out) return slk_fail(ctx, SLK_EINVAL, "slk_neighbors_scores: the output (d_out) is NULL");
    if (n_q == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    return eval_scores(ctx, SLK_GEMM_NBR_WRITE, {d_table, d_tscale, nullptr, (int)dim, n_table_rows}, {d_queries, d_qscale, nullptr},
                       n_q, d_out, call.s);
}

// predict() of ONE representation against EVERY item (slk_bilinear_predict / slk_poolnet_predict with d_items == NULL):
// the same sweep with a 32-row tile holding one live row.  (Inside the caller's profile span: no scope of its own.)
int slk_eval_predict_all(slk_ctx *ctx, const slk_tables *tables, const float *rep, const float *rbias, const int64_t *gmap,
                         float *d_out, hipStream_t s) {
    return eval_scores(ctx, SLK_GEMM_WRITE, item_table(tables), {rep, rbias, gmap}, 1, d_out, s);
}

int slk_eval_user_rep(slk_ctx *ctx, const slk_tables *tables, int vec, int g, const int64_t *d_user, const float **rep,
                      const float **rbias, const int64_t **gmap, hipStream_t s) {
    eval_rows rows = {nullptr, nullptr, nullptr};
    const int rc = eval_user_rows(ctx, tables, vec, g, d_user, 1, &rows, s);
    *rep = rows.rep;
    *rbias = rows.rbias;
    *gmap = rows.gmap;
    return rc;
}

SLK_EXPORT int slk_rank_targets(slk_ctx *ctx, float *d_scores, int64_t n_rows, int64_t num_items,
                                const int64_t *d_exc_rows, const int64_t *d_exc_items, int64_t n_exc,
                                const int64_t *d_tgt_rows, const int64_t *d_tgt_items, int64_t n_tgt,
                                double *d_rank_out, void *stream) {
    if (!ctx) return SLK_EINVAL;
    if (n_rows < 0 || num_items < 1 || n_exc < 0 || n_tgt < 0 || (n_rows > 0 && !d_scores) ||
        (n_exc > 0 && (!d_exc_rows || !d_exc_items)) || (n_tgt > 0 && (!d_tgt_rows || !d_tgt_items || !d_rank_out)))
        return slk_fail(ctx, SLK_EINVAL, "slk_rank_targets: bad arguments");
    int rc;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    if (n_exc > 0) {
        hipLaunchKernelGGL(k_eval_exclude, dim3(slk_grid_for(ctx, (size_t)n_exc, 256)), dim3(256), 0, call.s, d_scores,
                           num_items, d_exc_rows, d_exc_items, n_exc);
        SLK_LAUNCH_CHECK(ctx, "k_eval_exclude");
    }
    if (n_tgt > 0) {
        hipLaunchKernelGGL(k_eval_rank, dim3(slk_grid_for(ctx, (size_t)n_tgt, 1, 32)), dim3(256), 0, call.s,
                           (const float *)d_scores, num_items, d_tgt_rows, d_tgt_items, n_tgt, d_rank_out);
        SLK_LAUNCH_CHECK(ctx, "k_eval_rank");
    }
    return SLK_OK;
}
