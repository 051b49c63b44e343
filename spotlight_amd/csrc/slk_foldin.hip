// slk_foldin.hip -- slk_bilinear_foldin: rows for users who arrived after fit(), trained against FROZEN item tables.
//
// With the item side read-only, users do not interact: a user's trajectory is a function of their own history, their negatives
// and the optimizer.  So there is no sort, no ownership pass and nothing between workgroups: one unit owns one user for all steps
// of a launch, keeps the row, the bias and their optimizer state in registers and writes them once at the end.  The cost is the
// gather of the item rows, issued as the training passes issue it (slk_pick_layout row groups, 16 B per lane).
//   k_foldin_wave  one wavefront per user; its 64 / G row groups stride over the history, every group accumulates its part of the
//                  gradient in registers, the parts are combined by a fixed butterfly over the group index
//   k_foldin_wg    one 256-thread workgroup per user (long histories: the split rule for skewed lists); the 256 / G row groups'
//                  parts go through LDS and are added in group order by the lanes that hold the row, which republish it in LDS
// Which route a user takes depends on the length of their history alone (option "foldin_wg_min_len"); inside a route the order of
// every sum is fixed by the position of an interaction in the history -- a user's bits do not depend on the grid or on who else
// is in the call.  No float atomics, no spins, no barrier between workgroups.  Both kernels are launched for every call; the
// units whose user belongs to the other route leave at once (no host wait, no compaction pass).
#include "slk_kernels.h"

#define SLK_FOLDIN_MAX_STEPS 16     // steps per launch: their coefficients travel as kernel arguments; longer calls chain launches
#define SLK_FOLDIN_WG_MIN_LEN 64    // "foldin_wg_min_len" 0 (automatic): histories from this length on take the workgroup route -- the best of
                                    // 64 / 256 / 1024 / 4096 on the Zipf shape of scripts/bench_foldin.py (profiles/bench_foldin.json)
#define SLK_FOLDIN_UNROLL 2         // pair losses: positions per row group whose item rows are in flight together
#define SLK_FOLDIN_NEG_BATCH 4      // adaptive hinge: candidate rows in flight together

struct slk_foldin_args {
    float *U, *BU;                  // the new users' rows [H][D] and biases [H]
    float *S1U, *S2U, *S1B, *S2B;   // their optimizer state
    const float *V, *BI;            // the model's item tables (read-only)
    const int64_t *off, *items;     // histories, CSR
    const int64_t *neg;             // [nsteps][nn][n], the launch's first step first
    float *loss;                    // nullptr or [nsteps][H], likewise
    int64_t n;
    int64_t wg_min;                 // histories of at least this many interactions are the workgroup route's
    uint32_t H;
    uint32_t num_items;             // warp: the catalogue size of the rank estimate (slk_warp_weight)
    int D, nn, loss_kind, kind, nsteps;
    slk_opt_hyper hyper;
    slk_opt_coef c[SLK_FOLDIN_MAX_STEPS];
};

// One element's optimizer step (slk_opt_step), the kind chosen at run time: one kernel serves all five.
__device__ __forceinline__ void slk_foldin_step(const slk_foldin_args &a, const slk_opt_coef &c, float &p, float &s1, float &s2, float g) {
    switch (a.kind) {
        case SLK_OPT_ADAGRAD: return slk_opt_step<SLK_OPT_ADAGRAD>(a.hyper, c, p, s1, s2, g);
        case SLK_OPT_SPARSE_ADAM: return slk_opt_step<SLK_OPT_SPARSE_ADAM>(a.hyper, c, p, s1, s2, g);
        case SLK_OPT_SGD: return slk_opt_step<SLK_OPT_SGD>(a.hyper, c, p, s1, s2, g);
        case SLK_OPT_ADAM_DENSE: return slk_opt_step<SLK_OPT_ADAM_DENSE>(a.hyper, c, p, s1, s2, g);
        default: return slk_opt_step<SLK_OPT_ADAGRAD_DENSE>(a.hyper, c, p, s1, s2, g);
    }
}

// One step's pass of ONE row group over its share of the history: positions grp, grp + NGRP, grp + 2 NGRP, ... of the m
// interactions at `pos` (negatives: neg[r * n + position]).  Every group of the unit makes the same number of trips (the
// shuffles inside are then taken by whole waves); a group without a position in a trip loads nothing and adds nothing.
// All row loads of a trip are issued before the first use, the ids of the next trip behind them.
// ADP: 0 the pair losses (a.loss_kind), else the column loss this instantiation is compiled for (SLK_LOSS_ADAPTIVE_HINGE /
// SLK_LOSS_WARP: a constant, so that adaptive hinge keeps its registers -- read from the arguments it cost the gfx950 build
// 2-5 VGPRs and 2-13 spilled SGPRs)
template <int VEC, int G, int ADP, int NGRP>
__device__ __forceinline__ void slk_foldin_gather(const slk_foldin_args &a, const int64_t *pos, const int64_t *neg, int64_t m, int grp,
                                                  int d0, bool on, const slk_vec<VEC> &u, float bu, float inv_b, slk_vec<VEC> &gacc,
                                                  float &gb, double &lacc) {
    const int D = a.D;
    const float *V = a.V, *BI = a.BI;
    if (!ADP) {
        constexpr int UN = SLK_FOLDIN_UNROLL;
        uint32_t ip[UN], in[UN];
        bool act[UN];
#pragma unroll
        for (int e = 0; e < UN; ++e) {
            const int64_t j = (int64_t)e * NGRP + grp;
            act[e] = j < m;
            ip[e] = act[e] ? (uint32_t)pos[j] : 0u;
            in[e] = act[e] ? (uint32_t)neg[j] : 0u;
        }
        for (int64_t j0 = 0; j0 < m; j0 += (int64_t)UN * NGRP) {
            slk_vec<VEC> vi[UN], vj[UN];
            float bip[UN], bin[UN];
#pragma unroll
            for (int e = 0; e < UN; ++e) {
                vi[e] = (act[e] && on) ? slk_vload<VEC>(V + (size_t)ip[e] * D + d0) : slk_vzero<VEC>();
                vj[e] = (act[e] && on) ? slk_vload<VEC>(V + (size_t)in[e] * D + d0) : slk_vzero<VEC>();
                bip[e] = act[e] ? BI[ip[e]] : 0.0f;
                bin[e] = act[e] ? BI[in[e]] : 0.0f;
            }
            bool actn[UN];
            uint32_t ipn[UN], inn[UN];
#pragma unroll
            for (int e = 0; e < UN; ++e) {
                const int64_t j = j0 + (int64_t)(UN + e) * NGRP + grp;
                actn[e] = j < m;
                ipn[e] = actn[e] ? (uint32_t)pos[j] : 0u;
                inn[e] = actn[e] ? (uint32_t)neg[j] : 0u;
            }
#pragma unroll
            for (int e = 0; e < UN; ++e) {
                const float sp = slk_group_sum<G>(slk_vdot<VEC>(u, vi[e])) + bu + bip[e];
                const float sn = slk_group_sum<G>(slk_vdot<VEC>(u, vj[e])) + bu + bin[e];
                if (act[e]) {
                    float l, gp, gn;
                    slk_pair_loss(a.loss_kind, sp, sn, inv_b, l, gp, gn);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) gacc.v[i] += gp * vi[e].v[i] + gn * vj[e].v[i];
                    gb += gp + gn;
                    lacc += (double)l;
                }
                act[e] = actn[e];
                ip[e] = ipn[e];
                in[e] = inn[e];
            }
        }
    } else {
        // the column losses on a one-user minibatch (row r of column j is neg[r * n + j]).  Adaptive hinge (spotlight/losses.py:
        // 127-166): of the position's nn candidates the one with the largest score, the FIRST on ties (torch.max(dim=0)), and
        // the hinge against it.  Warp: the first candidate that violates the margin, latched (slk_column_feed), and the hinge
        // against it scaled by the weight of its row; no violator adds nothing.  The rule is k_adaptive_select's.
        constexpr int NB = SLK_FOLDIN_NEG_BATCH;
        const int nn = a.nn;
        bool act = grp < m;
        uint32_t ip = act ? (uint32_t)pos[grp] : 0u;
        for (int64_t j0 = 0; j0 < m; j0 += NGRP) {
            const int64_t j = j0 + grp;
            const slk_vec<VEC> vi = (act && on) ? slk_vload<VEC>(V + (size_t)ip * D + d0) : slk_vzero<VEC>();
            const float bip = act ? BI[ip] : 0.0f;
            const int64_t jn = j + NGRP;
            const bool actn = jn < m;
            const uint32_t ipn = actn ? (uint32_t)pos[jn] : 0u;
            slk_vec<VEC> vbest = slk_vzero<VEC>();
            // the positive's score: warp's latch needs it ahead of the candidates; adaptive hinge forms it behind them, where it
            // always has (a register held across the candidate loop cost k_foldin_wave<VEC 1> a wave of occupancy)
            float sp = 0.0f;
            if (ADP == SLK_LOSS_WARP) sp = slk_group_sum<G>(slk_vdot<VEC>(u, vi)) + bu + bip;
            slk_column_pick pick = slk_column_begin();
            for (int r0 = 0; r0 < nn; r0 += NB) {
                uint32_t in[NB];
                bool ra[NB];
#pragma unroll
                for (int e = 0; e < NB; ++e) {
                    ra[e] = act && r0 + e < nn;
                    in[e] = ra[e] ? (uint32_t)neg[(size_t)(r0 + e) * (size_t)a.n + (size_t)j] : 0u;
                }
                slk_vec<VEC> vj[NB];
                float bin[NB];
#pragma unroll
                for (int e = 0; e < NB; ++e) {
                    vj[e] = (ra[e] && on) ? slk_vload<VEC>(V + (size_t)in[e] * D + d0) : slk_vzero<VEC>();
                    bin[e] = ra[e] ? BI[in[e]] : 0.0f;
                }
#pragma unroll
                for (int e = 0; e < NB; ++e) {
                    const float sc = slk_group_sum<G>(slk_vdot<VEC>(u, vj[e])) + bu + bin[e];
                    if (ra[e] && slk_column_feed(ADP, pick, sp, (uint32_t)(r0 + e), sc)) vbest = vj[e];
                }
            }
            if (ADP != SLK_LOSS_WARP) sp = slk_group_sum<G>(slk_vdot<VEC>(u, vi)) + bu + bip;
            if (act) {
                float l, g_unit;
                slk_column_finish(ADP, a.num_items, pick, sp, g_unit, l);
                const float gn = slk_column_g(g_unit, inv_b), gp = -gn;
#pragma unroll
                for (int i = 0; i < VEC; ++i) gacc.v[i] += gp * vi.v[i] + gn * vbest.v[i];
                gb += gp + gn;
                lacc += (double)l;
            }
            act = actn;
            ip = ipn;
        }
    }
}

// ---- wave route -----------------------------------------------------------------------------------------------------------------
template <int VEC, int G, int ADP>
__global__ __launch_bounds__(256) void k_foldin_wave(slk_foldin_args a) {
    constexpr int NG = 64 / G;
    const int lane64 = (int)(threadIdx.x & 63u);
    const int grp = lane64 / G, gl = lane64 % G;
    const uint32_t user = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (user >= a.H) return;  // (whole waves leave here and below: no lane of a wave waits for another)
    const int64_t o0 = a.off[user];
    const int64_t m = a.off[user + 1] - o0;
    if (m <= 0) {  // no history: row, bias and state stay as they are, the loss slots are 0
        if (a.loss && lane64 == 0)
            for (int t = 0; t < a.nsteps; ++t) a.loss[(size_t)t * a.H + user] = 0.0f;
        return;
    }
    if (m >= a.wg_min) return;  // the workgroup route's
    const int D = a.D;
    const int d0 = gl * VEC;
    const bool on = d0 < D;
    const bool has1 = slk_opt_has_s1(a.kind), has2 = slk_opt_has_s2(a.kind);
    const size_t uoff = (size_t)user * D + d0;
    slk_vec<VEC> u = on ? slk_vload<VEC>(a.U + uoff) : slk_vzero<VEC>();
    slk_vec<VEC> s1 = (on && has1) ? slk_vload<VEC>(a.S1U + uoff) : slk_vzero<VEC>();
    slk_vec<VEC> s2 = (on && has2) ? slk_vload<VEC>(a.S2U + uoff) : slk_vzero<VEC>();
    float bu = a.BU[user];
    float sb1 = has1 ? a.S1B[user] : 0.0f, sb2 = has2 ? a.S2B[user] : 0.0f;
    const float inv_b = 1.0f / (float)m;
    const int64_t *pos = a.items + o0;
    for (int t = 0; t < a.nsteps; ++t) {
        const int64_t *neg = a.neg + (size_t)t * (size_t)a.nn * (size_t)a.n + (size_t)o0;
        slk_vec<VEC> gacc = slk_vzero<VEC>();
        float gb = 0.0f;
        double lacc = 0.0;
        slk_foldin_gather<VEC, G, ADP, NG>(a, pos, neg, m, grp, d0, on, u, bu, inv_b, gacc, gb, lacc);
        // the row groups' parts, combined by a butterfly over the group index: x + y == y + x bit for bit, so every lane ends with
        // the same sum, associated the same way for every user
#pragma unroll
        for (int mask = G; mask < 64; mask <<= 1) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) gacc.v[i] += __shfl_xor(gacc.v[i], mask, 64);
            gb += __shfl_xor(gb, mask, 64);
            lacc += __shfl_xor(lacc, mask, 64);
        }
        const slk_opt_coef c = a.c[t];
        if (on) {  // (a padding lane's elements stay 0: with eps == 0 their update would be 0 / 0)
#pragma unroll
            for (int i = 0; i < VEC; ++i) slk_foldin_step(a, c, u.v[i], s1.v[i], s2.v[i], gacc.v[i]);
        }
        slk_foldin_step(a, c, bu, sb1, sb2, gb);
        if (a.loss && lane64 == 0) a.loss[(size_t)t * a.H + user] = (float)(lacc / (double)m);
    }
    if (grp == 0 && on) {
        slk_vstore<VEC>(a.U + uoff, u);
        if (has1) slk_vstore<VEC>(a.S1U + uoff, s1);
        if (has2) slk_vstore<VEC>(a.S2U + uoff, s2);
    }
    if (lane64 == 0) {
        a.BU[user] = bu;
        if (has1) a.S1B[user] = sb1;
        if (has2) a.S2B[user] = sb2;
    }
}

// ---- workgroup route ------------------------------------------------------------------------------------------------------------
template <int VEC, int G, int ADP>
__global__ __launch_bounds__(256) void k_foldin_wg(slk_foldin_args a) {
    constexpr int GPB = 256 / G;
    constexpr int DL = G * VEC;  // LDS row length (>= D)
    __shared__ __attribute__((aligned(16))) float s_u[DL];
    __shared__ __attribute__((aligned(16))) float s_part[GPB * DL];
    __shared__ float s_gb[GPB];
    __shared__ double s_l[GPB];
    __shared__ float s_bu;
    const uint32_t user = blockIdx.x;
    const int64_t o0 = a.off[user];
    const int64_t m = a.off[user + 1] - o0;
    if (m <= 0 || m < a.wg_min) return;  // (the whole workgroup) the wave route's
    const int grp = (int)threadIdx.x / G, gl = (int)threadIdx.x % G;
    const int D = a.D;
    const int d0 = gl * VEC;
    const bool on = d0 < D;
    const bool has1 = slk_opt_has_s1(a.kind), has2 = slk_opt_has_s2(a.kind);
    const bool holder = grp == 0;  // the lanes (of wave 0) that keep the row and its state in registers for all steps
    const size_t uoff = (size_t)user * D + d0;
    slk_vec<VEC> p = slk_vzero<VEC>(), s1 = slk_vzero<VEC>(), s2 = slk_vzero<VEC>();
    float pb = 0.0f, sb1 = 0.0f, sb2 = 0.0f;
    if (holder) {
        if (on) {
            p = slk_vload<VEC>(a.U + uoff);
            if (has1) s1 = slk_vload<VEC>(a.S1U + uoff);
            if (has2) s2 = slk_vload<VEC>(a.S2U + uoff);
        }
        slk_vstore<VEC>(s_u + d0, p);
        if (threadIdx.x == 0) {
            pb = a.BU[user];
            if (has1) sb1 = a.S1B[user];
            if (has2) sb2 = a.S2B[user];
            s_bu = pb;
        }
    }
    const float inv_b = 1.0f / (float)m;
    const int64_t *pos = a.items + o0;
    for (int t = 0; t < a.nsteps; ++t) {
        __syncthreads();  // the row of this step is in LDS
        const slk_vec<VEC> u = slk_vload<VEC>(s_u + d0);
        const float bu = s_bu;
        const int64_t *neg = a.neg + (size_t)t * (size_t)a.nn * (size_t)a.n + (size_t)o0;
        slk_vec<VEC> gacc = slk_vzero<VEC>();
        float gb = 0.0f;
        double lacc = 0.0;
        slk_foldin_gather<VEC, G, ADP, GPB>(a, pos, neg, m, grp, d0, on, u, bu, inv_b, gacc, gb, lacc);
        slk_vstore<VEC>(s_part + grp * DL + d0, gacc);
        if (gl == 0) {
            s_gb[grp] = gb;
            s_l[grp] = lacc;
        }
        __syncthreads();  // every group's part is in LDS (and every thread has read this step's row)
        if (holder) {
            const slk_opt_coef c = a.c[t];
            slk_vec<VEC> g = slk_vzero<VEC>();
            for (int k = 0; k < GPB; ++k) {  // in group order
                const slk_vec<VEC> x = slk_vload<VEC>(s_part + k * DL + d0);
#pragma unroll
                for (int i = 0; i < VEC; ++i) g.v[i] += x.v[i];
            }
            if (on) {  // (a padding lane's elements stay 0, as in the wave route)
#pragma unroll
                for (int i = 0; i < VEC; ++i) slk_foldin_step(a, c, p.v[i], s1.v[i], s2.v[i], g.v[i]);
            }
            slk_vstore<VEC>(s_u + d0, p);
            if (threadIdx.x == 0) {
                float gbt = 0.0f;
                double lt = 0.0;
                for (int k = 0; k < GPB; ++k) {
                    gbt += s_gb[k];
                    lt += s_l[k];
                }
                slk_foldin_step(a, c, pb, sb1, sb2, gbt);
                s_bu = pb;
                if (a.loss) a.loss[(size_t)t * a.H + user] = (float)(lt / (double)m);
            }
        }
    }
    if (holder) {
        if (on) {
            slk_vstore<VEC>(a.U + uoff, p);
            if (has1) slk_vstore<VEC>(a.S1U + uoff, s1);
            if (has2) slk_vstore<VEC>(a.S2U + uoff, s2);
        }
        if (threadIdx.x == 0) {
            a.BU[user] = pb;
            if (has1) a.S1B[user] = sb1;
            if (has2) a.S2B[user] = sb2;
        }
    }
}

typedef void (*slk_foldin_fn)(slk_foldin_args);

static void foldin_pick(int vec, int g, int column_loss, slk_foldin_fn *wave, slk_foldin_fn *wg) {
#define SLK_FOLDIN_PICK(V, GG)                                  \
    do {                                                        \
        if (column_loss == SLK_LOSS_WARP) {                     \
            *wave = k_foldin_wave<V, GG, SLK_LOSS_WARP>;        \
            *wg = k_foldin_wg<V, GG, SLK_LOSS_WARP>;            \
        } else if (column_loss) {                               \
            *wave = k_foldin_wave<V, GG, SLK_LOSS_ADAPTIVE_HINGE>; \
            *wg = k_foldin_wg<V, GG, SLK_LOSS_ADAPTIVE_HINGE>;  \
        } else {                                                \
            *wave = k_foldin_wave<V, GG, 0>;                    \
            *wg = k_foldin_wg<V, GG, 0>;                        \
        }                                                       \
    } while (0)
    SLK_FOR_LAYOUT(vec, g, SLK_FOLDIN_PICK);
#undef SLK_FOLDIN_PICK
}

SLK_EXPORT int slk_bilinear_foldin(slk_ctx *ctx, const slk_tables *tables, slk_optim *optim, const int64_t *d_off,
                                   const int64_t *d_items, int64_t n_new_users, int64_t n, int32_t loss, int32_t n_neg,
                                   int64_t n_steps, const int64_t *d_neg, float *d_loss, void *stream) {
    if (!ctx) return SLK_EINVAL;
    if (n_steps < 1 || n_new_users < 1)
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_foldin: n_steps %lld and n_new_users %lld must be at least 1", (long long)n_steps,
                        (long long)n_new_users);
    if (n < 0) return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_foldin: n %lld is negative", (long long)n);
    if (loss == SLK_LOSS_SOFTMAX)  // (every candidate live: not this gather's pair / column rule; the host takes its generic route)
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_foldin: softmax (loss kind %d) is not built for fold-in", loss);
    if (loss < SLK_LOSS_POINTWISE || loss > SLK_LOSS_WARP || slk_loss_is_explicit(loss))
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_foldin: loss %d is not an implicit-feedback loss (explicit feedback needs ratings)",
                        loss);
    const bool column = slk_loss_is_column(loss);
    if (column && n_neg < 1)
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_foldin: %s needs n_neg >= 1 (got %d)", slk_column_loss_name(loss), n_neg);
    if (!d_off || (n > 0 && (!d_items || !d_neg)))
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_foldin: the histories (d_off / d_items) or the negatives (d_neg) are NULL");
    if (tables && (tables->user_bloom || tables->item_bloom))
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_foldin: plain tables only (a BloomEmbedding table on the %s side)",
                        tables->user_bloom ? "user" : "item");
    int vec, g, rc;
    if ((rc = slk_check_tables(ctx, tables, 15u, &vec, &g))) return rc;  // (refuses item biases inside a bias-shadow scope)
    if (tables->num_users != n_new_users)
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_foldin: tables->num_users %lld != n_new_users %lld (d_param[0] / [2] are the new rows)",
                        (long long)tables->num_users, (long long)n_new_users);
    if ((rc = slk_check_optim(ctx, optim, 5u))) return rc;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_USER_PASS))) return rc;

    const int nn = column ? n_neg : 1;
    slk_foldin_fn wave_fn = nullptr, wg_fn = nullptr;
    foldin_pick(vec, g, column ? (int)loss : 0, &wave_fn, &wg_fn);
    slk_foldin_args a;
    memset(&a, 0, sizeof(a));
    a.U = tables->d_param[0];
    a.BU = tables->d_param[2];
    a.V = tables->d_param[1];
    a.BI = tables->d_param[3];
    a.S1U = optim->d_state1[0];
    a.S1B = optim->d_state1[2];
    a.S2U = optim->d_state2[0];
    a.S2B = optim->d_state2[2];
    a.off = d_off;
    a.items = d_items;
    a.n = n;
    a.H = (uint32_t)n_new_users;
    a.num_items = (uint32_t)tables->num_items;
    a.D = tables->dim;
    a.nn = nn;
    a.loss_kind = loss;
    a.kind = optim->kind;
    a.wg_min = ctx->opt_foldin_wg_min_len > 0 ? ctx->opt_foldin_wg_min_len : SLK_FOLDIN_WG_MIN_LEN;
    a.hyper = slk_opt_hyper_of(optim);
    const unsigned wave_grid = (unsigned)((n_new_users + 3) / 4), wg_grid = (unsigned)n_new_users;
    for (int64_t t0 = 0; t0 < n_steps; t0 += SLK_FOLDIN_MAX_STEPS) {
        const int ns = (int)(n_steps - t0 < SLK_FOLDIN_MAX_STEPS ? n_steps - t0 : SLK_FOLDIN_MAX_STEPS);
        a.nsteps = ns;
        a.neg = d_neg ? d_neg + (size_t)t0 * (size_t)nn * (size_t)n : nullptr;
        a.loss = d_loss ? d_loss + (size_t)t0 * (size_t)n_new_users : nullptr;
        for (int t = 0; t < ns; ++t) a.c[t] = slk_opt_coef_at(optim, optim->step + t0 + t + 1);
        // long histories first: they are the launch's tail
        hipLaunchKernelGGL(wg_fn, dim3(wg_grid), dim3(256), 0, call.s, a);
        SLK_LAUNCH_CHECK(ctx, "k_foldin_wg");
        hipLaunchKernelGGL(wave_fn, dim3(wave_grid), dim3(256), 0, call.s, a);
        SLK_LAUNCH_CHECK(ctx, "k_foldin_wave");
    }
    optim->step += n_steps;
    return SLK_OK;
}
