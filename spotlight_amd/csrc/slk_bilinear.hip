// slk_bilinear.hip -- the fused negative-sampled BilinearNet training step for gfx950.
//
// Replaces the minibatch body of ImplicitFactorizationModel.fit()
// (spotlight/factorization/implicit.py:229-243): 2x BilinearNet.forward
// (factorization/representations.py:61-91), the loss (losses.py:18-166), autograd's
// embedding backward (duplicate rows SUMMED before the non-linear optimizer update) and
// torch.optim.{Adagrad,SparseAdam,Adam}.step().
//
// Exactness constraint that shapes the design (hard part 1): within a minibatch
// every forward reads pre-step parameters, and every row receives the SUM of its gradient
// contributions before one optimizer update.  So per minibatch:
//
//   prep (per chunk of minibatches, slk_prep): radix-sort the interactions by
//        (minibatch, user) and the (interaction, item) occurrences by (minibatch, item).
//        Sorted order makes each unique row the property of exactly ONE row group, turns
//        row traffic into ascending-address streams, and needs no atomics.
//   USER PASS  one row group (G = dim/4 lanes, 16 B per lane, a D=64 row = one 256-B line)
//        per unique user: gathers U[u], V[pos], V[neg] and the biases, wave-shuffle dot
//        products, loss + dL/dscore, accumulates the user-row gradient over the user's
//        occurrences, snapshots the pre-step user row (coalesced, position-indexed) for the
//        item pass, writes dL/dscore per occurrence, then applies the optimizer to U[u] in
//        place.
//   ITEM PASS  one row group per unique item: sums g * snapshot(user row) over the item's
//        occurrences (positive or negative), then applies the optimizer to V[i] in place.
//
// The path is HBM-bound (0.2 flop/B): no MFMA, no LDS tiling of rows -- each row is touched
// once per pass by the lanes that own it.
#include <math.h>

#include "slk_kernels.h"

// ---------------------------------------------------------------------------------------
// USER PASS
// ---------------------------------------------------------------------------------------
// BLOOM: the user and/or item embedding layer is a BloomEmbedding (slk_kernels.h).  Item vectors
// are then sums of hashed rows; a bloom USER vector is shared between users, so its gradient is
// not applied here but parked in a.urec for a ROW-mode owner pass over the hashed user rows.
// UMODE: 0 = the (positive, negative) pair's scores, loss and dL/dscore formed here; 1 = dL/dscore read from a.gk
// (adaptive hinge, staged explicit route); 2 = explicit feedback, fused: one pair, score + loss against a.ratings
// LAT (pair mode, plain tables): the latency-bound form for minibatches that do not fill the chip (a few thousand to ~10^5
// interactions: every row group then handles one or two positions and the pass is a chain of dependent round trips, not a
// stream).  The position's item pair is fetched WITH its key (before the head test: wasted for the few non-head positions)
// and the user row's optimizer state with the row, so a position costs two round trips -- (key, pair), then (user row +
// state, both item rows, the three biases) -- instead of four.  Same arithmetic in the same order: bit-identical results.
// ULONG (plain user table): HOT USERS.  A user's occurrences in the minibatch are walked by ONE row group; a power user
// with thousands of them is a serial tail longer than the whole pass.  As in the item pass, a run that wholly covers an
// aligned tile of SLK_USER_TILE positions is LONG: it is cut at the tile boundaries, every segment is walked by its own row
// group from the same pre-step user row (records, dL/dscore and loss terms as usual) and leaves its part of the user
// gradient as a PARTIAL (a.upart / upart_meta, at most two per tile); nobody updates U[u] here -- k_user_stitch, behind the
// pass, adds a long run's partials in tile order and applies the one update.  Every position of a run decides "long" the
// same way (a head looks at the first aligned tile behind it, a boundary position at the tile before and the tile behind
// it).  Short runs are walked and applied exactly as in the plain form; the host launches this form only for minibatches
// that hold a long run (k_user_long_flags).
// PP (pair mode, plain tables): inside a user-row ping-pong scope (slk_user_pingpong_begin; slk_pass_args::uflag / P0alt) --
// the user's current row is read from the copy its flag byte names, the updated row goes to the OTHER copy, the byte is
// flipped, and no record is written: the item pass (SLK_ITEM_SNAPPP) gathers the pre-step row from where it still stands.
#ifndef SLK_PP_PIPE
#define SLK_PP_PIPE 2  // software pipeline of the bandwidth-bound ping-pong user pass (below): 0 none, 1 keys + flag, 2 + item pair, 3 + early state.  Same box, C2 user pass: one-table form 0.3135 ms, 0: 0.306, 1: 0.289, 2: 0.284, 3: 0.295 (profiles/r06_p_*)
#endif
// (Holding the pipelined form to the one-table form's occupancy -- amdgpu_waves_per_eu 8: 64 VGPRs instead of 65, SparseAdam 7: 72
// instead of 81 -- spills two to eight dwords and LOSES: user pass 0.283 -> 0.289 ms, SparseAdam 0.422 -> 0.467, profiles/r06_t_ab_occ.txt.)
// SGL (the bandwidth-bound ping-pong form, Adagrad): the single-occurrence fast path (slk_pass_args::mflag) -- an item that occurs
// ONCE in the minibatch is updated HERE: the pass holds its pre-step row (read for the score), dL/dscore and the pre-step user row,
// so the item pass's re-read of the row and its gather of the user row are spared (catalogues far larger than a minibatch: 98 % of
// the occurrences at the C5 shard's shape).  The same operations in the same order as the item pass applies to a run of length
// one (0 + g * u, then slk_apply_vec_pre): bit-identical tables.  Nobody else reads or writes such a row in this minibatch.
// (The form compiles to 102 VGPRs = 4 waves per SIMD.  Held to 5 -- amdgpu_waves_per_eu: 96 VGPRs, 28 B of scratch -- it LOSES: C5 shard
// user pass 0.683-0.689 -> 0.721-0.724 ms, profiles/r06_z3_ab_sgl_waves.txt.)
template <int VEC, int G, int UPD, int UMODE, bool BLOOM, bool LAT = false, bool ULONG = false, bool PP = false, bool SGL = false>
__global__ __launch_bounds__(256) void k_user_pass(slk_pass_args a) {
    static_assert(!LAT || (UMODE == 0 && !BLOOM), "LAT is the pair mode over plain tables");
    static_assert(!PP || (UMODE == 0 && !BLOOM), "PP is the pair mode over plain tables");
    static_assert(!SGL || (PP && !LAT && !ULONG && UPD == SLK_UPD_ADAGRAD), "SGL: the plain ping-pong form, Adagrad");
    static_assert(!ULONG || !BLOOM, "long user runs: plain tables");
    constexpr uint32_t S = SLK_USER_TILE;
    constexpr bool PRE = UMODE != 0;
    constexpr bool EXPL = UMODE == 2;
    __shared__ double red[256];
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const int D = a.D;
    const int d0 = lane * VEC;
    const bool on = d0 < D;
    const uint32_t stride = gridDim.x * GPB;
    float loss_acc = 0.0f;

    // Plain form: row group g takes positions g, g + stride, ... (one position per turn).  ULONG: row group g takes TILES g,
    // g + stride, ... and walks the positions of a tile itself, run piece by run piece.  A segment of a long run is one tile's
    // worth of occurrences walked by ONE row group; with one position per turn the segment heads (every SLK_USER_TILE-th
    // position) land on one row group of a wavefront while its other three idle behind the divergent walk -- measured,
    // profiles/r03_c_*, r03_d_*: Zipf(1.0) users 2.0-2.9 ms per pass.  With a tile per row group the four groups of a
    // wavefront each walk their own tile, hot or not, at the plain form's memory parallelism.
    const uint32_t n_turns = ULONG ? (a.end - a.begin + S - 1u) / S : a.end - a.begin;
    // PIPE (the bandwidth-bound ping-pong form): a position costs key -> flag byte -> row, one dependent round trip more than the
    // one-table form's key -> row.  The row group's turns are therefore software-pipelined: entering turn t it holds {key, previous
    // key, flag} of turn t and {key, previous key} of turn t + 1; it issues the flag load of turn t + 1 and the key loads of turn
    // t + 2 in front of turn t's own row loads.  (Only the user's owner -- this group, in turn t + 1 -- writes that flag byte.)
    // SLK_PP_PIPE >= 2: the turn's (positive, negative) item pair travels with its key, so that a head issues its user row, both
    // item rows and the biases in ONE round trip; >= 3: and the row's optimizer state with them (as the latency-bound form does).
    // (Two further steps were measured and not kept: DESIGN.md section 6 "Round 8", profiles/r08_a_pass_waits.md.)
    constexpr bool PIPE = PP && !LAT && !ULONG && SLK_PP_PIPE >= 1;
    constexpr bool PIPE_IDS = PIPE && SLK_PP_PIPE >= 2;
    uint32_t pk_key = 0u, pk_prev = 0u, pk_flag = 0u, pn_key = 0u, pn_prev = 0u;
    uint32_t pk_ip = 0u, pk_in = 0u, pn_ip = 0u, pn_in = 0u;
    uint32_t pk_mf = 0u, pn_mf = 0u;  // SGL: the turn's two "occurs more than once" bytes (positive | negative << 8)
    auto ld_mf = [&](uint32_t pos) -> uint32_t { return (uint32_t)*reinterpret_cast<const uint16_t *>(a.mflag + 2 * (size_t)pos); };
    if (PIPE) {
        const uint32_t t0 = blockIdx.x * GPB + grp;
        if (t0 < n_turns) {
            pk_key = a.ukey[a.begin + t0];
            pk_prev = t0 > 0u ? a.ukey[a.begin + t0 - 1u] : 0u;
            if (PIPE_IDS) {
                pk_ip = a.uit[2 * (size_t)(a.begin + t0)];
                pk_in = a.uit[2 * (size_t)(a.begin + t0) + 1];
            }
            if (SGL) pk_mf = ld_mf(a.begin + t0);
            pk_flag = (uint32_t)a.uflag[pk_key & a.umask];
        }
        if (t0 + stride < n_turns) {
            pn_key = a.ukey[a.begin + t0 + stride];
            pn_prev = a.ukey[a.begin + t0 + stride - 1u];
            if (PIPE_IDS) {
                pn_ip = a.uit[2 * (size_t)(a.begin + t0 + stride)];
                pn_in = a.uit[2 * (size_t)(a.begin + t0 + stride) + 1];
            }
            if (SGL) pn_mf = ld_mf(a.begin + t0 + stride);
        }
    }
    for (uint32_t turn = blockIdx.x * GPB + grp; turn < n_turns; turn += stride) {
    const uint32_t p_lo = a.begin + (ULONG ? turn * S : turn);
    const uint32_t p_hi = ULONG ? (p_lo + S < a.end ? p_lo + S : a.end) : p_lo + 1u;
    for (uint32_t p = p_lo; p < p_hi; ++p) {
        const bool nt_keys = (SLK_NT_OF(a) & 8) != 0;
        const uint32_t key = PIPE ? pk_key : slk_ld_u32(a.ukey + p, nt_keys);
        uint32_t lat_ip = 0u, lat_in = 0u;
        bool is_head;
        uint32_t cur_piped = 0u, mf_piped = 0u;
        if (PIPE) {
            is_head = !(p > a.begin && pk_prev == key);
            cur_piped = pk_flag;
            lat_ip = pk_ip;
            lat_in = pk_in;
            mf_piped = pk_mf;
            pk_mf = pn_mf;
            pk_key = pn_key;
            pk_prev = pn_prev;
            pk_ip = pn_ip;
            pk_in = pn_in;
            if (turn + stride < n_turns) pk_flag = (uint32_t)a.uflag[pn_key & a.umask];
            if (turn + 2u * stride < n_turns) {
                pn_key = a.ukey[p + 2u * stride];
                pn_prev = a.ukey[p + 2u * stride - 1u];
                if (PIPE_IDS) {
                    pn_ip = a.uit[2 * (size_t)(p + 2u * stride)];
                    pn_in = a.uit[2 * (size_t)(p + 2u * stride) + 1];
                }
                if (SGL) pn_mf = ld_mf(p + 2u * stride);
            }
        } else if (LAT) {
            const uint32_t prev = p > a.begin ? a.ukey[p - 1] : ~key;
            lat_ip = a.uit[2 * (size_t)p];
            lat_in = a.uit[2 * (size_t)p + 1];
            is_head = prev != key;
        } else {
            is_head = !(p > a.begin && a.ukey[p - 1] == key);
        }
        bool run_long = false;
        uint32_t seg_limit = a.end;  // the walk stops here at the latest
        if (ULONG) {
            const uint32_t rel = p - a.begin;
            if (is_head) {
                const uint32_t t0 = a.begin + (rel + S - 1u) / S * S;  // the first aligned tile behind the head
                run_long = t0 + S <= a.end && a.ukey[t0 + S - 1u] == key;
            } else if (rel % S == 0u) {
                run_long = (rel >= S && a.ukey[p - S] == key) || (p + S <= a.end && a.ukey[p + S - 1u] == key);
                is_head = false;
            }
            if (!is_head && !(run_long && rel % S == 0u)) continue;
            if (run_long) seg_limit = a.begin + (rel / S + 1u) * S < a.end ? a.begin + (rel / S + 1u) * S : a.end;
        } else if (!is_head) {
            continue;  // not the head of its user segment
        }
        const uint32_t user = key & a.umask;
        const size_t uoff = (size_t)user * D + d0;
        // user-row ping-pong (slk_pass_args::uflag): the copy that holds this user's current row; the updated row goes to the
        // other copy, the item pass gathers the pre-step row from this one -- no record is written
        constexpr bool pp = PP;
        const uint32_t cur = PIPE ? cur_piped : (pp ? (uint32_t)a.uflag[user] : 0u);
        float *const unew = pp ? (cur ? a.P[0] : a.P0alt) + uoff : nullptr;
        slk_vec<VEC> u;
        if (BLOOM)
            u = slk_emb_vec<VEC>(a.P[0], a.ub, user, D, d0, on);
        else
            u = on ? slk_vload_if_nt<VEC>((cur ? a.P0alt : a.P[0]) + uoff, (SLK_NT_OF(a) & 1) != 0) : slk_vzero<VEC>();
        const float bu = (UMODE == 0 && !BLOOM && a.ubz) ? 0.0f : a.P[2][user];  // (SLK_TABLES_USER_BIAS_ZERO: a line per interaction for a table of zeros)
        // explicit feedback: the pass is bound by its chain of dependent loads, so the Adagrad state of the
        // user row is fetched with the row instead of after the loss (the pair mode is bandwidth-bound:
        // fetching early there only lengthens register lifetimes)
        // SparseAdam (round 4): both moment rows (and the bias's moments) with the row in every mode -- its update otherwise
        // starts with a dependent round trip of TWO more rows per user behind the loss (the pass ran at 0.45 of the roofline
        // against Adagrad's 0.63, profiles/r03_final_bench_sparse_adam.json)
        constexpr bool EARLY_ADAM = !BLOOM && UPD == SLK_UPD_SPARSE_ADAM && !ULONG;
        // (SGL: the pass is one round trip per position -- user row, both item rows AND every optimizer-state row the position will
        // update -- then arithmetic and stores; loaded one after the other behind the loss the three state rows cost it three more)
        constexpr bool EARLY_STATE = ((EXPL || LAT || SGL || (PIPE && SLK_PP_PIPE >= 3)) && !BLOOM && UPD == SLK_UPD_ADAGRAD) || EARLY_ADAM;
        slk_vec<VEC> su = slk_vzero<VEC>(), su2 = slk_vzero<VEC>();
        if (EARLY_STATE && on) su = slk_vload_if_nt<VEC>(a.S1[0] + uoff, (SLK_NT_OF(a) & 1) != 0);
        if (EARLY_ADAM && on) su2 = slk_vload_if_nt<VEC>(a.S2[0] + uoff, (SLK_NT_OF(a) & 1) != 0);
        float sbu = 0.0f, sbu2 = 0.0f;
        if (EARLY_STATE && !(SGL && a.ubz)) sbu = a.S1[2][user];  // (SLK_TABLES_USER_BIAS_ZERO: the user-bias gradient is exactly zero, its state is never used)
        if (EARLY_ADAM) sbu2 = a.S2[2][user];
        slk_vec<VEC> gu = slk_vzero<VEC>();
        float gbu = 0.0f;
        uint32_t q = p;
        // the key after the current position travels one iteration ahead of its use (the segment-end test)
        // (latency-bound modes only: same-box A/B, +5 % on the adaptive pass, -1 % on the bandwidth-bound pair pass)
        constexpr bool NEXT_KEY = UMODE != 0;
        uint32_t next_key = 0;
        if (NEXT_KEY) next_key = (q + 1 < seg_limit) ? a.ukey[q + 1] : ~key;
        do {
            float *rec = a.snap + (size_t)(q - a.begin) * a.RS;
            // explicit feedback: the rating's gather is issued first so that it overlaps the item row's
            uint32_t e_item = 0;
            float e_rating = 0.0f;
            if (EXPL) {
                e_item = a.uit[q];
                e_rating = a.ratings[a.uk[q]];
            }
            if (on && !pp) slk_vstore_if_nt<VEC>(rec + d0, u, (SLK_NT_OF(a) & 16) != 0);
            if (!PRE) {
                uint32_t ip, in;
                if ((LAT || PIPE_IDS) && q == p) {
                    ip = lat_ip;
                    in = lat_in;
                } else {
                    ip = slk_ld_u32(a.uit + 2 * (size_t)q, nt_keys);
                    in = slk_ld_u32(a.uit + 2 * (size_t)q + 1, nt_keys);
                }
                slk_vec<VEC> vi, vj;
                if (BLOOM) {
                    vi = slk_emb_vec<VEC>(a.P[1], a.ib, ip, D, d0, on);
                    vj = slk_emb_vec<VEC>(a.P[1], a.ib, in, D, d0, on);
                } else {
                    vi = on ? slk_vload<VEC>(a.P[1] + (size_t)ip * D + d0) : slk_vzero<VEC>();
                    vj = on ? slk_vload<VEC>(a.P[1] + (size_t)in * D + d0) : slk_vzero<VEC>();
                }
                const float bip = a.P[3][SLK_B3(a, ip)], bin = a.P[3][SLK_B3(a, in)];  // issued with the rows, not behind the dots' shuffles
                // SGL: the optimizer state of the once-only items of this position, with their rows
                uint32_t mf = 0xffffu;
                slk_vec<VEC> svi = slk_vzero<VEC>(), svj = slk_vzero<VEC>();
                float sbi = 0.0f, sbj = 0.0f;
                if (SGL) {
                    mf = (q == p) ? mf_piped : ld_mf(q);
                    const bool nt_rows = (SLK_NT_OF(a) & 2) != 0;
                    if (!(mf & 0xffu)) {
                        if (on) svi = slk_vload_if_nt<VEC>(a.S1[1] + (size_t)ip * D + d0, nt_rows);
                        if (lane == 0) sbi = a.S1[3][SLK_B3(a, ip)];
                    }
                    if (!(mf >> 8)) {
                        if (on) svj = slk_vload_if_nt<VEC>(a.S1[1] + (size_t)in * D + d0, nt_rows);
                        if (lane == 0) sbj = a.S1[3][SLK_B3(a, in)];
                    }
                }
                const float sp = slk_group_sum<G>(slk_vdot<VEC>(u, vi)) + bu + bip;
                const float sn = slk_group_sum<G>(slk_vdot<VEC>(u, vj)) + bu + bin;
                float l, gp, gn;
                slk_pair_loss(a.loss_kind, sp, sn, a.inv_b, l, gp, gn);
#pragma unroll
                for (int i = 0; i < VEC; ++i) gu.v[i] += gp * vi.v[i] + gn * vj.v[i];
                gbu += gp + gn;
                if (lane == 0) {
                    if (pp) {  // {dL/dscore, src} per pair: one 16-B store
                        float srcf;
                        const uint32_t src = user | (cur << 31);
                        memcpy(&srcf, &src, 4);
                        reinterpret_cast<float4 *>(a.gsn)[q - a.begin] = make_float4(gp, srcf, gn, srcf);
                    } else {
                        float *gq = a.gsn + 2 * (size_t)(q - a.begin);
                        gq[0] = gp;
                        gq[1] = gn;
                    }
                    loss_acc += l;
                }
                if (SGL) {
                    // once-only items of this position: their whole update, as the item pass applies it to a run of length one --
                    // nothing for dL/dscore == 0 (Adagrad: the item pass leaves an untouched-gradient row alone), else the summed
                    // gradient 0 + g * u_old and 0 + g, then the row / bias update in place (the rows and biases are this pass's own
                    // pre-step loads)
                    const bool nt_rows = (SLK_NT_OF(a) & 2) != 0;
                    auto once = [&](uint32_t item, slk_vec<VEC> &v, slk_vec<VEC> &sv, float g, float b, float bs) {
                        const size_t voff = (size_t)item * D + d0;
                        if (on) {
                            slk_vec<VEC> gv;
#pragma unroll
                            for (int i = 0; i < VEC; ++i) gv.v[i] = 0.0f + g * u.v[i];
                            slk_apply_vec_pre<VEC, UPD>(a, 1, voff, v, sv, gv, nullptr, nt_rows);
                        }
                        if (lane == 0) {
                            slk_vec<1> bpv, bsv, gbv;
                            bpv.v[0] = b;
                            bsv.v[0] = bs;
                            gbv.v[0] = 0.0f + g;
                            slk_apply_vec_pre<1, UPD>(a, 3, SLK_B3(a, item), bpv, bsv, gbv);
                        }
                    };
                    if (!(mf & 0xffu) && gp != 0.0f) once(ip, vi, svi, gp, bip, sbi);
                    if (!(mf >> 8) && gn != 0.0f) once(in, vj, svj, gn, bin, sbj);
                }
            } else if (EXPL) {
                // explicit feedback (one pair per interaction): score, loss and dL/dscore formed here
                const uint32_t it = e_item;
                const float bi = a.P[3][SLK_B3(a, it)];  // issued with the row, not after the dot's shuffles
                slk_vec<VEC> v;
                if (BLOOM)
                    v = slk_emb_vec<VEC>(a.P[1], a.ib, it, D, d0, on);
                else
                    v = on ? slk_vload<VEC>(a.P[1] + (size_t)it * D + d0) : slk_vzero<VEC>();
                const float sc = slk_group_sum<G>(slk_vdot<VEC>(u, v)) + bu + bi;
                float l, g;
                slk_explicit_loss(a.loss_kind, sc, e_rating, a.inv_b, a.end - a.begin, l, g);
                if (lane == 0) {
                    a.gsn[q - a.begin] = g;
                    loss_acc += l;
                }
                if (g != 0.0f) {
                    slk_vaxpy<VEC>(gu, g, v);
                    gbu += g;
                }
            } else {
                // dL/dscore of the interaction's 1 + n pairs, one per lane (one round trip for all of them, with the pairs' item
                // ids), then the rows of the LIVE pairs -- adaptive hinge: the positive and the selected draw -- two at a time,
                // added in pair order (the order the one-pair-at-a-time loop this replaces added them in: same bits; a pair per
                // iteration cost a dependent dL/dscore -> id -> row chain each)
                const size_t kb = (size_t)a.uk[q] * a.NP, qb = (size_t)q * a.NP;
                for (int s0 = 0; s0 < a.NP; s0 += G) {
                    const int s = s0 + lane;
                    float gs = 0.0f;
                    uint32_t it_l = 0u;
                    if (s < a.NP) {
                        gs = a.gk[kb + s];
                        it_l = a.uit[qb + s];
                        a.gsn[(size_t)(q - a.begin) * a.NP + s] = gs;
                    }
                    unsigned long long live = slk_group_or<G>(gs != 0.0f ? 1ull << lane : 0ull);
                    while (live) {
                        const int j0 = __builtin_ctzll(live);
                        live &= live - 1ull;
                        const bool two = live != 0ull;
                        const int j1 = two ? __builtin_ctzll(live) : j0;
                        if (two) live &= live - 1ull;
                        const uint32_t i0 = __shfl(it_l, j0, G), i1 = __shfl(it_l, j1, G);
                        const float g0 = __shfl(gs, j0, G), g1 = __shfl(gs, j1, G);
                        slk_vec<VEC> v0, v1 = slk_vzero<VEC>();
                        if (BLOOM) {
                            v0 = slk_emb_vec<VEC>(a.P[1], a.ib, i0, D, d0, on);
                            if (two) v1 = slk_emb_vec<VEC>(a.P[1], a.ib, i1, D, d0, on);
                        } else {
                            v0 = on ? slk_vload<VEC>(a.P[1] + (size_t)i0 * D + d0) : slk_vzero<VEC>();
                            if (two && on) v1 = slk_vload<VEC>(a.P[1] + (size_t)i1 * D + d0);
                        }
                        slk_vaxpy<VEC>(gu, g0, v0);
                        gbu += g0;
                        if (two) {
                            slk_vaxpy<VEC>(gu, g1, v1);
                            gbu += g1;
                        }
                    }
                }
            }
            ++q;
            if (NEXT_KEY) {
                if (next_key != key) break;
                next_key = (q + 1 < seg_limit) ? a.ukey[q + 1] : ~key;
            } else if (!(q < seg_limit && a.ukey[q] == key)) {
                break;
            }
        } while (true);
        // sampled softmax: an interaction's 1 + n pairs are all this user's and their dL/dscore add up to 0 in exact arithmetic
        // (-Zneg / Z + sum e_j / Z): the user-bias gradient IS zero.  The fp32 sum leaves a residue of 1e-9, which Adagrad and
        // Adam from a zero accumulator turn into a step of lr -- the exact value is applied instead (include/spotlight_hip.h)
        if (UMODE == 1 && a.ubg0) gbu = 0.0f;

        if (ULONG && run_long) {
            // a segment of a long run: its part of the user gradient, for k_user_stitch
            const bool ends = !(q < a.end && a.ukey[q] == key);
            const size_t slot = 2 * (size_t)((p - a.begin) / S) + (is_head ? 1u : 0u);
            float *pp = a.upart + slot * (size_t)a.UPS;
            if (on) slk_vstore<VEC>(pp + d0, gu);
            if (lane == 0) {
                pp[a.UPS - 1] = gbu;
                a.upart_meta[2 * slot] = key;
                a.upart_meta[2 * slot + 1] = (a.upart_gen << SLK_IPART_GEN_SHIFT) | (is_head ? (uint32_t)SLK_IPART_STARTS : 0u) |
                                             (ends ? (uint32_t)SLK_IPART_ENDS : 0u);
                if (is_head) atomicAdd(a.upart_count, 1u);
            }
            p = q - 1u;  // (a run that ends inside the tile: the walk goes on with the run behind it)
            continue;
        }
        if (BLOOM && a.ub.n_hash) {
            if (on) slk_vstore<VEC>(a.urec + (size_t)(p - a.begin) * a.RSU + d0, gu);
        } else if (on) {
            if (EARLY_ADAM)
                slk_apply_vec_pre<VEC, UPD, true>(a, 0, uoff, u, su, gu, &su2, (SLK_NT_OF(a) & 1) != 0, unew);
            else if (EARLY_STATE)
                slk_apply_vec_pre<VEC, UPD>(a, 0, uoff, u, su, gu, nullptr, (SLK_NT_OF(a) & 1) != 0, unew);
            else
                slk_apply_vec<VEC, UPD>(a, 0, uoff, u, gu, (SLK_NT_OF(a) & 1) != 0, unew);
        }
        if (pp && lane == 0) a.uflag[user] = (uint8_t)(cur ^ 1u);  // (this group owns the user: nobody else reads or writes the byte in this launch)
        if (EARLY_ADAM) {
            if (lane == 0) {  // (SparseAdam decays the moments of a looked-up row whatever its gradient is)
                slk_vec<1> bpv, bsv, bsv2, gbv;
                bpv.v[0] = bu;
                bsv.v[0] = sbu;
                bsv2.v[0] = sbu2;
                gbv.v[0] = gbu;
                slk_apply_vec_pre<1, UPD, true>(a, 2, user, bpv, bsv, gbv, &bsv2);
            }
        } else if (EARLY_STATE) {
            if (lane == 0 && gbu != 0.0f) {  // gbu == 0 is an exact no-op for Adagrad (slk_apply_bias)
                slk_vec<1> bpv, bsv, gbv;
                bpv.v[0] = bu;
                bsv.v[0] = sbu;
                gbv.v[0] = gbu;
                slk_apply_vec_pre<1, UPD>(a, 2, user, bpv, bsv, gbv);
            }
        } else if (lane == 0) {
            slk_apply_bias<UPD>(a, 2, user, gbu);
        }
        if (ULONG) p = q - 1u;  // the run's other positions (in this tile; beyond it the loop ends) are done
    }
    }
    if (!PRE || EXPL) {
        const double tot = slk_block_sum_256((double)loss_acc, red);
        if (threadIdx.x == 0) a.loss_partial[blockIdx.x] = tot;
    }
}

// Behind k_user_pass<..., ULONG>: one row group per tile of SLK_USER_TILE positions.  The group of the tile in which a long
// run STARTS adds the run's partials in tile order -- its own tile's slot 1, then slot 0 of the following tiles up to the
// one in which the run ends (the next G tiles' metas are read at once, the lanes that still belong to the run are a
// prefix) -- and applies the one update of U[u] and its bias.
template <int VEC, int G, int UPD, bool PP = false>
__global__ __launch_bounds__(256) void k_user_stitch(slk_pass_args a) {
    constexpr int GPB = 256 / G;
    constexpr uint32_t S = SLK_USER_TILE;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const int D = a.D;
    const int d0 = lane * VEC;
    const bool on = d0 < D;
    const uint32_t ntiles = (a.end - a.begin + S - 1u) / S;
    if (*a.upart_count == 0u) return;
    const uint32_t gen = a.upart_gen;
    for (uint32_t tile = blockIdx.x * GPB + grp; tile < ntiles; tile += gridDim.x * GPB) {
        const size_t slot = 2 * (size_t)tile + 1;
        const uint32_t fl = a.upart_meta[2 * slot + 1];
        if ((fl >> SLK_IPART_GEN_SHIFT) != gen) continue;  // no long run starts in this tile
        const uint32_t key = a.upart_meta[2 * slot];
        const float *pp = a.upart + slot * (size_t)a.UPS;
        slk_vec<VEC> gu = on ? slk_vload<VEC>(pp + d0) : slk_vzero<VEC>();
        float gbu = pp[a.UPS - 1];
        uint32_t t2 = tile + 1;
        bool more = (fl & SLK_IPART_ENDS) == 0;
        // A round looks at the next TPR = R * G tiles: lane l reads the metas of tiles t2 + l + j * G ({key, flags}: one 8-B load;
        // the tiles that continue this run are a prefix), and the partials the round can consume are fetched WITH the metas --
        // their addresses do not depend on them -- so a run that fills thousands of tiles costs its owner one round trip per TPR
        // tiles (measured before: one per tile, then three per G tiles; profiles/r03_*).  What the run does not reach is
        // dropped.  The sums are added in tile order, as the persistent kernel's walk adds them.
        constexpr int R = G <= 16 ? 2 : 1;
        constexpr int TPR = R * G;
        constexpr bool SPEC = G <= 16;  // wider groups: partials fetched after the metas, SLK_STITCH_BATCH at a time
        while (more) {
            // every load of the round is issued before anything waits: the partials first, then the metas (the compiler keeps
            // program order, and a compare right behind a meta load would put a full round trip in front of the partial loads)
            slk_vec<VEC> sc[SPEC ? TPR : 1];
            float sb[SPEC ? TPR : 1];
            if (SPEC) {
#pragma unroll
                for (int e = 0; e < (SPEC ? TPR : 1); ++e) {
                    sc[e] = slk_vzero<VEC>();
                    sb[e] = 0.0f;
                    if (t2 + (uint32_t)e < ntiles) {
                        const float *q = a.upart + 2 * (size_t)(t2 + (uint32_t)e) * (size_t)a.UPS;
                        if (on) sc[e] = slk_vload<VEC>(q + d0);
                        sb[e] = q[a.UPS - 1];
                    }
                }
            }
            uint2 kf[R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const uint32_t tl = t2 + (uint32_t)(lane + j * G);
                kf[j] = make_uint2(0u, 0u);
                if (tl < ntiles) kf[j] = *reinterpret_cast<const uint2 *>(a.upart_meta + 4 * (size_t)tl);
            }
            uint32_t f[R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                f[j] = kf[j].y;
                if (t2 + (uint32_t)(lane + j * G) >= ntiles || (f[j] >> SLK_IPART_GEN_SHIFT) != gen || (f[j] & SLK_IPART_STARTS) ||
                    kf[j].x != key)
                    f[j] = 0u;
                else
                    f[j] |= 1u;  // bit 0: part of this run
            }
            // cnt = tiles of this round that belong to the run: up to and including the first one that ends it
            // (the lanes' flags as bit masks of the group, OR-reduced in log2(G) exchanges: a loop of G dependent
            // lane-to-lane reads per round was what the stitch of a run over thousands of tiles spent its time in)
            int cnt = 0;
            bool ended = false;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if (!ended && cnt == j * G) {
                    const unsigned long long valid = slk_group_or<G>((f[j] & 1u) ? 1ull << lane : 0ull);
                    const unsigned long long ends = slk_group_or<G>((f[j] & SLK_IPART_ENDS) ? 1ull << lane : 0ull);
                    const unsigned long long full = G == 64 ? ~0ull : (1ull << G) - 1ull;
                    int c = (valid & full) == full ? G : __builtin_ctzll(~valid);      // the leading lanes that continue the run
                    const unsigned long long e_in = ends & (c == 64 ? ~0ull : (1ull << c) - 1ull);
                    if (e_in) {
                        c = __builtin_ctzll(e_in) + 1;                                 // ... up to and including the one that ends it
                        ended = true;
                    }
                    cnt += c;
                }
            }
            if (SPEC) {
#pragma unroll
                for (int e = 0; e < (SPEC ? TPR : 1); ++e) {
                    if (e < cnt) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) gu.v[i] += sc[e].v[i];
                        gbu += sb[e];
                    }
                }
            }
            for (int l0 = 0; !SPEC && l0 < cnt; l0 += SLK_STITCH_BATCH) {
                slk_vec<VEC> cc[SLK_STITCH_BATCH];
                float cb[SLK_STITCH_BATCH];
#pragma unroll
                for (int e = 0; e < SLK_STITCH_BATCH; ++e) {
                    cc[e] = slk_vzero<VEC>();
                    cb[e] = 0.0f;
                    if (l0 + e < cnt) {
                        const float *q = a.upart + 2 * (size_t)(t2 + (uint32_t)(l0 + e)) * (size_t)a.UPS;
                        if (on) cc[e] = slk_vload<VEC>(q + d0);
                        cb[e] = q[a.UPS - 1];
                    }
                }
#pragma unroll
                for (int e = 0; e < SLK_STITCH_BATCH; ++e) {
                    if (l0 + e < cnt) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) gu.v[i] += cc[e].v[i];
                        gbu += cb[e];
                    }
                }
            }
            more = !ended && cnt == TPR;
            t2 += (uint32_t)TPR;
        }
        const uint32_t user = key & a.umask;
        const size_t uoff = (size_t)user * D + d0;
        // (user-row ping-pong: the long run's segments read the row from the current copy and left the flag alone)
        constexpr bool pingpong = PP;
        // (read by lane 0 and handed round: nothing else separates the other lanes' read from lane 0's write below)
        uint32_t cur = 0u;
        if (pingpong) cur = __shfl(lane == 0 ? (uint32_t)a.uflag[user] : 0u, 0, G);
        if (on) {
            slk_vec<VEC> u = slk_vload_if_nt<VEC>((cur ? a.P0alt : a.P[0]) + uoff, (SLK_NT_OF(a) & 1) != 0);
            slk_apply_vec<VEC, UPD>(a, 0, uoff, u, gu, (SLK_NT_OF(a) & 1) != 0, pingpong ? (cur ? a.P[0] : a.P0alt) + uoff : nullptr);
        }
        if (pingpong && lane == 0) a.uflag[user] = (uint8_t)(cur ^ 1u);
        if (lane == 0) slk_apply_bias<UPD>(a, 2, user, gbu);
    }
}

// flags[mb] |= 1 iff some user run of minibatch mb's window of the user-sorted list wholly covers an aligned tile of
// SLK_USER_TILE positions (ids only: once per chunk, read back by the host with the item pass's flags)
__global__ __launch_bounds__(256) void k_user_long_flags(const uint32_t *ukey, uint32_t n, uint32_t per_mb, int *flags) {
    constexpr uint32_t S = SLK_USER_TILE;
    const uint32_t tiles_per_mb = (per_mb + S - 1) / S;
    const uint32_t n_mb = (n + per_mb - 1) / per_mb;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_mb * tiles_per_mb; i += gridDim.x * 256) {
        const uint32_t mb = i / tiles_per_mb, q = i - mb * tiles_per_mb;
        const uint32_t w0 = mb * per_mb, w1 = (n - w0 < per_mb) ? n : w0 + per_mb;
        const uint32_t t0 = w0 + q * S;
        if (t0 >= w1 || w1 - t0 < S) continue;  // only full tiles make a run long
        if (ukey[t0] == ukey[t0 + S - 1]) flags[mb] = 1;
    }
}

// ---------------------------------------------------------------------------------------
// adaptive hinge: scores for every (interaction, pair), then the per-column selection of
// _get_multiple_negative_predictions' view(n, B) layout (factorization/implicit.py:266-275)
// ---------------------------------------------------------------------------------------
template <int VEC, int G>
__global__ __launch_bounds__(256) void k_score_pass(slk_pass_args a) {
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const int D = a.D;
    const int d0 = lane * VEC;
    const bool on = d0 < D;
    const uint32_t stride = gridDim.x * GPB;
    for (uint32_t q = a.begin + blockIdx.x * GPB + grp; q < a.end; q += stride) {
        const uint32_t user = a.ukey[q] & a.umask;
        const slk_vec<VEC> u = slk_emb_vec<VEC>(a.P[0], a.ub, user, D, d0, on);
        const float bu = a.P[2][user];
        const size_t kb = (size_t)a.uk[q] * a.NP, qb = (size_t)q * a.NP;
        constexpr int SB = 3;  // candidates whose rows are in flight together (1 + 5 draws: two batches)
        for (int s0 = 0; s0 < a.NP; s0 += SB) {
            slk_vec<VEC> v[SB];
            float bi[SB];
#pragma unroll
            for (int j = 0; j < SB; ++j) {
                v[j] = slk_vzero<VEC>();
                bi[j] = 0.0f;
                if (s0 + j < a.NP) {
                    const uint32_t it = a.uit[qb + s0 + j];
                    v[j] = slk_emb_vec<VEC>(a.P[1], a.ib, it, D, d0, on);
                    bi[j] = a.P[3][SLK_B3(a, it)];
                }
            }
#pragma unroll
            for (int j = 0; j < SB; ++j) {
                const float sc = slk_group_sum<G>(slk_vdot<VEC>(u, v[j])) + bu + bi[j];
                if (lane == 0 && s0 + j < a.NP) a.sk[kb + s0 + j] = sc;
            }
        }
    }
}

// (k_adaptive_select: slk_kernels.h -- the row-sharded path launches it too)

// ---------------------------------------------------------------------------------------
// sampled softmax (include/spotlight_hip.h: SLK_LOSS_SOFTMAX) behind k_score_pass: per interaction the softmax over its
// positive and its OWN n draws -- pairs 0 .. n of sk[(k0 + k) * NP + .], contiguous -- the loss term and dL/dscore of every
// pair.  A group of G lanes per interaction (G: slk_softmax_group(NP), a function of n alone), lane t taking pairs t, t + G,
// ...: the lanes of a group read consecutive floats, the groups of a wavefront consecutive interactions.  NP <= 64 is one pair
// per lane, kept in a register; above, the wavefront strides and re-reads its pairs from the cache (the scores of one
// interaction are at most 4 KB).  The order of the max and of the sums is the one the header states: per lane in pair order,
// then the xor butterfly G/2 .. 1 -- grid, bm and chunking do not enter, and there is no other form of this kernel.
// Every entry of this minibatch's gk is written (no memset before the launch); w / wsum as in k_adaptive_select.
// ---------------------------------------------------------------------------------------
static inline int slk_softmax_group(int NP) {
    int g = 2;
    while (g < NP && g < 64) g <<= 1;
    return g;
}

template <int G>
__global__ __launch_bounds__(256) void k_softmax_loss(const float *sk, float *gk, uint32_t k0, uint32_t bm, int nn, float inv_b,
                                                      double *loss_partial, const float *w, const double *wsum) {
    __shared__ double red[256];
    constexpr uint32_t GPB = 256 / G;
    const int NP = nn + 1;
    const int lane = (int)(threadIdx.x % G);
    const uint32_t grp = threadIdx.x / G;
    const float inv_W = w ? 1.0f / (float)*wsum : 0.0f;
    double lsum = 0.0;
    // (every group of a workgroup makes the same number of trips: the shuffles inside are taken by whole wavefronts)
    for (uint32_t base = blockIdx.x * GPB; base < bm; base += gridDim.x * GPB) {
        const uint32_t k = base + grp;
        const bool on = k < bm;
        const size_t at0 = (size_t)(k0 + (on ? k : 0u)) * NP;
        const float s_own = (on && lane < NP) ? sk[at0 + lane] : 0.0f;  // this lane's first pair
        float m = -INFINITY;
        if (on)
            for (int j = lane; j < NP; j += G) m = fmaxf(m, j == lane ? s_own : sk[at0 + j]);
#pragma unroll
        for (int x = G / 2; x >= 1; x >>= 1) m = fmaxf(m, __shfl_xor(m, x, G));
        float zn = 0.0f, e_own = 0.0f;
        if (on)
            for (int j = lane; j < NP; j += G) {
                const float e = expf((j == lane ? s_own : sk[at0 + j]) - m);
                if (j == lane) e_own = e;
                if (j > 0) zn += e;
            }
#pragma unroll
        for (int x = G / 2; x >= 1; x >>= 1) zn += __shfl_xor(zn, x, G);
        const float e0 = __shfl(e_own, 0, G), s0 = __shfl(s_own, 0, G);
        if (!on) continue;
        const float Z = e0 + zn;
        const float wc = w ? w[k0 + k] : 1.0f;
        for (int j = lane; j < NP; j += G) {
            const float e = j == lane ? e_own : expf(sk[at0 + j] - m);
            const float unit = j == 0 ? zn / Z : e / Z;
            const float g = w ? slk_weight_scale(unit, wc, inv_W) : unit * inv_b;
            gk[at0 + j] = j == 0 ? -g : g;
        }
        if (lane == 0) {
            const float l = logf(Z) - (s0 - m);
            lsum += w ? (double)wc * (double)l : (double)l;
        }
    }
    const double tot = slk_block_sum_256(lsum, red);
    // (weighted: the partials leave already divided by the weight sum -- the item pass's finalisation then runs with inv_b = 1)
    if (threadIdx.x == 0) loss_partial[blockIdx.x] = w ? tot * (double)inv_W : tot;
}

typedef void (*slk_softmax_fn)(const float *, float *, uint32_t, uint32_t, int, float, double *, const float *, const double *);
static slk_softmax_fn softmax_loss_fn(int g) {
    switch (g) {
        case 2: return k_softmax_loss<2>;
        case 4: return k_softmax_loss<4>;
        case 8: return k_softmax_loss<8>;
        case 16: return k_softmax_loss<16>;
        case 32: return k_softmax_loss<32>;
        default: return k_softmax_loss<64>;
    }
}

// ---------------------------------------------------------------------------------------
// explicit feedback (spotlight/factorization/explicit.py:223-234, losses.py:169-244): per interaction
// the loss of its ONE predicted score against the observed rating and dL/dscore, formed in fp32
// operation by operation as autograd forms them.  One thread per interaction of the minibatch.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_explicit_loss(const float *sk, const float *ratings, float *gk, uint32_t k0,
                                                       uint32_t bm, int loss_kind, float inv_b, double *loss_partial) {
    __shared__ double red[256];
    double lsum = 0.0;
    for (uint32_t c = blockIdx.x * 256 + threadIdx.x; c < bm; c += gridDim.x * 256) {
        const float sc = sk[k0 + c], r = ratings[k0 + c];
        float l, g;
        slk_explicit_loss(loss_kind, sc, r, inv_b, bm, l, g);
        gk[k0 + c] = g;
        lsum += (double)l;
    }
    const double tot = slk_block_sum_256(lsum, red);
    if (threadIdx.x == 0) loss_partial[blockIdx.x] = tot;
}

// ---------------------------------------------------------------------------------------
// interaction weights (slk_bilinear_train_weighted): L = sum(w_i l_i) / sum(w_i) per minibatch
// ---------------------------------------------------------------------------------------
// W_m = sum of the weights of minibatch m, in float64, in an order fixed by the minibatch's length alone: segment j of the
// minibatch (SLK_WSEG consecutive weights) is summed by ONE workgroup -- thread t adds elements t, t + 256, ... of the segment
// in turn, then the block tree (slk_block_sum_256) -- and the segments' sums are added the same way by one workgroup per
// minibatch.  Which workgroup takes which segment, the grid and the chunk the minibatch falls in do not enter.
#define SLK_WSEG 8192u
__global__ __launch_bounds__(256) void k_weight_partials(const float *w, uint32_t nc, uint32_t per_mb, uint32_t segs_per_mb,
                                                         double *wpart) {
    __shared__ double red[256];
    const uint32_t n_mb = (nc + per_mb - 1) / per_mb;
    for (uint32_t i = blockIdx.x; i < n_mb * segs_per_mb; i += gridDim.x) {
        const uint32_t mb = i / segs_per_mb, seg = i - mb * segs_per_mb;
        const uint32_t w0 = mb * per_mb, w1 = (nc - w0 < per_mb) ? nc : w0 + per_mb;
        // (a short last minibatch has empty segments: they are written as 0.0 and add nothing)
        const uint32_t s0 = (w1 - w0 > seg * SLK_WSEG) ? w0 + seg * SLK_WSEG : w1, s1 = (w1 - s0 < SLK_WSEG) ? w1 : s0 + SLK_WSEG;
        double x = 0.0;
        for (uint32_t e = s0 + threadIdx.x; e < s1; e += 256) x += (double)w[e];
        const double tot = slk_block_sum_256(x, red);
        if (threadIdx.x == 0) wpart[i] = tot;
    }
}

__global__ __launch_bounds__(256) void k_weight_sums(const double *wpart, uint32_t n_mb, uint32_t segs_per_mb, double *wsum) {
    __shared__ double red[256];
    for (uint32_t mb = blockIdx.x; mb < n_mb; mb += gridDim.x) {
        double x = 0.0;
        for (uint32_t j = threadIdx.x; j < segs_per_mb; j += 256) x += wpart[(size_t)mb * segs_per_mb + j];
        const double tot = slk_block_sum_256(x, red);
        if (threadIdx.x == 0) wsum[mb] = tot;
    }
}

// The pair losses (pointwise, bpr, hinge) behind k_score_pass with NP == 2: one thread per interaction of the minibatch, in
// the shape of k_explicit_loss.  sk / gk / w are chunk-local (k0 = the minibatch's first interaction); *wsum = W of this
// minibatch.  The loss partials leave already divided by W: the item pass's finalisation runs with inv_b = 1.
__global__ __launch_bounds__(256) void k_pair_loss_weighted(const float *sk, const float *w, float *gk, uint32_t k0, uint32_t bm,
                                                            int loss_kind, const double *wsum, double *loss_partial) {
    __shared__ double red[256];
    const float inv_W = 1.0f / (float)*wsum;
    double lsum = 0.0;
    for (uint32_t c = blockIdx.x * 256 + threadIdx.x; c < bm; c += gridDim.x * 256) {
        const size_t at = 2 * (size_t)(k0 + c);
        const float wc = w[k0 + c];
        float l, gp, gn;
        slk_pair_loss(loss_kind, sk[at], sk[at + 1], 1.0f, l, gp, gn);  // (x * 1.0f is x: the factors without their 1 / B)
        gk[at] = slk_weight_scale(gp, wc, inv_W);
        gk[at + 1] = slk_weight_scale(gn, wc, inv_W);
        lsum += (double)wc * (double)l;
    }
    const double tot = slk_block_sum_256(lsum, red);
    if (threadIdx.x == 0) loss_partial[blockIdx.x] = tot * (double)inv_W;
}

__global__ __launch_bounds__(256) void k_explicit_loss_weighted(const float *sk, const float *ratings, const float *w, float *gk,
                                                                uint32_t k0, uint32_t bm, int loss_kind, const double *wsum,
                                                                double *loss_partial) {
    __shared__ double red[256];
    const float Wf = (float)*wsum, inv_W = 1.0f / Wf;
    double lsum = 0.0;
    for (uint32_t c = blockIdx.x * 256 + threadIdx.x; c < bm; c += gridDim.x * 256) {
        const float wc = w[k0 + c];
        float l, g;
        slk_explicit_loss_weighted(loss_kind, sk[k0 + c], ratings[k0 + c], wc, inv_W, Wf, l, g);
        gk[k0 + c] = g;
        lsum += (double)wc * (double)l;
    }
    const double tot = slk_block_sum_256(lsum, red);
    if (threadIdx.x == 0) loss_partial[blockIdx.x] = tot * (double)inv_W;
}

// ---------------------------------------------------------------------------------------
// dense sweeps (reference default optimizer: Adam with weight_decay = l2 over EVERY row)
// ---------------------------------------------------------------------------------------

// One launch sweeps up to four tables: block b belongs to the table t with first[t] <= b < first[t + 1]
// and strides over that table with the blocks of its own range (a minibatch of the reference's default
// optimizer is then user pass + item pass + ONE sweep launch instead of four).
struct slk_sweep_all_args {
    float *p[4], *s1[4], *s2[4], *g[4];
    size_t numel[4];
    unsigned first[5];
    int adam;
    slk_opt_coef coef;
    slk_opt_hyper hyper;
};

// One element: consume (and re-zero) its gradient, then the optimizer's rule in place on memory -- the state's stores are
// issued where the rule assigns them, ahead of the parameter's division chain.
template <int KIND>
__device__ __forceinline__ void slk_dense_sweep_elem(const slk_sweep_all_args &a, float *p, float *s1, float *s2, float *g, size_t e) {
    const float gv = g[e];
    g[e] = 0.0f;
    float none = 0.0f;
    slk_opt_step<KIND>(a.hyper, a.coef, p[e], s1[e], slk_opt_has_s2(KIND) ? s2[e] : none, gv);
}

__global__ __launch_bounds__(256) void k_dense_sweep_all(slk_sweep_all_args a) {
    int t = 0;
    while (t < 3 && blockIdx.x >= a.first[t + 1]) ++t;
    const size_t local = blockIdx.x - a.first[t], nblk = a.first[t + 1] - a.first[t];
    float *p = a.p[t], *s1 = a.s1[t], *s2 = a.s2[t], *g = a.g[t];
    const size_t numel = a.numel[t];
    if (a.adam) {
        for (size_t e = local * 256 + threadIdx.x; e < numel; e += nblk * 256) slk_dense_sweep_elem<SLK_OPT_ADAM_DENSE>(a, p, s1, s2, g, e);
    } else {
        for (size_t e = local * 256 + threadIdx.x; e < numel; e += nblk * 256) slk_dense_sweep_elem<SLK_OPT_ADAGRAD_DENSE>(a, p, s1, s2, g, e);
    }
}

// ---------------------------------------------------------------------------------------
// prep kernels
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_i64_to_u32(const int64_t *in, uint32_t *out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = (uint32_t)in[i];
}

__global__ __launch_bounds__(256) void k_u32_to_i64(const uint32_t *in, int64_t *out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = (int64_t)in[i];
}

__global__ __launch_bounds__(256) void k_pack_items(const uint32_t *uk, const int64_t *items,
                                                    const uint32_t *neg32, uint32_t nc, int nn, uint32_t *uit) {
    const int NP = nn + 1;
    for (uint32_t q = blockIdx.x * 256 + threadIdx.x; q < nc; q += gridDim.x * 256) {
        const uint32_t k = uk[q];
        uit[(size_t)q * NP] = (uint32_t)items[k];
        for (int r = 0; r < nn; ++r) uit[(size_t)q * NP + 1 + r] = neg32[(size_t)k * nn + r];
    }
}

// adaptive hinge, live occurrences only: qk[uk[q]] = q
__global__ __launch_bounds__(256) void k_invert_perm(const uint32_t *uk, uint32_t nc, uint32_t *qk) {
    for (uint32_t q = blockIdx.x * 256 + threadIdx.x; q < nc; q += gridDim.x * 256) qk[uk[q]] = q;
}

// keys of one minibatch's live list (k_adaptive_select): entry e -> (item of occurrence live[e], live[e]);
// with a BloomEmbedding item layer (ib.n_hash > 0, hashed = true) entry e*H + h -> (row_h(item), live[e]).
// Dead entries get the all-ones key: they sort to the end and the item pass skips them.
__global__ __launch_bounds__(256) void k_build_live_keys(const uint32_t *live, const uint32_t *uit, uint32_t n_live,
                                                         slk_bloom_dev ib, bool hashed, uint32_t *key, uint32_t *val) {
    const uint32_t H = hashed ? (uint32_t)ib.n_hash : 1u;
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < n_live * H; e += gridDim.x * 256) {
        const uint32_t l = e / H, h = e - l * H;
        const uint32_t r = live[l];
        uint32_t k = 0xffffffffu;
        if (r != 0xffffffffu) k = hashed ? slk_bloom_row(ib, uit[r], (int)h) : uit[r];
        key[e] = k;
        val[e] = r;
    }
}

// BloomEmbedding item layer: occurrence r contributes to the n_hash hashed rows of its item:
// key[r*H + h] = (minibatch, row_h(item)), value = r (same record as the plain occurrence)
__global__ __launch_bounds__(256) void k_build_item_bloom_keys(const uint32_t *uit, uint32_t nocc, int NP,
                                                               uint32_t bsz, unsigned cbits, slk_bloom_dev ib,
                                                               uint32_t *key, uint32_t *val) {
    const uint32_t H = (uint32_t)ib.n_hash;
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < nocc * H; e += gridDim.x * 256) {
        const uint32_t r = e / H, h = e - r * H;
        const uint32_t q = r / (uint32_t)NP;
        key[e] = ((q / bsz) << cbits) | slk_bloom_row(ib, uit[r], (int)h);
        val[e] = r;
    }
}

// BloomEmbedding user layer: the head position p of every user segment contributes its summed
// gradient record to the n_hash hashed rows of the user; non-head positions get the sentinel
// row `ub.rows` (never updated).  value = p.
__global__ __launch_bounds__(256) void k_build_user_bloom_keys(const uint32_t *ukey, uint32_t umask, uint32_t nc,
                                                               uint32_t bsz, unsigned cbits, slk_bloom_dev ub,
                                                               uint32_t *key, uint32_t *val) {
    const uint32_t H = (uint32_t)ub.n_hash;
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < nc * H; e += gridDim.x * 256) {
        const uint32_t p = e / H, h = e - p * H;
        const uint32_t mb = p / bsz;
        const bool head = (p % bsz == 0) || ukey[p - 1] != ukey[p];
        key[e] = (mb << cbits) | (head ? slk_bloom_row(ub, ukey[p] & umask, (int)h) : ub.rows);
        val[e] = p;
    }
}

// ---------------------------------------------------------------------------------------
// predict
// ---------------------------------------------------------------------------------------
template <int VEC, int G>
__global__ __launch_bounds__(256) void k_predict(const float *U, const float *V, const float *bu,
                                                 const float *bi, int D, slk_bloom_dev ub, slk_bloom_dev ib,
                                                 const int64_t *users, int64_t n_users, const int64_t *items,
                                                 int64_t n, float *out) {
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const int d0 = lane * VEC;
    const bool on = d0 < D;
    for (int64_t k = (int64_t)blockIdx.x * GPB + grp; k < n; k += (int64_t)gridDim.x * GPB) {
        const int64_t u = users[n_users == 1 ? 0 : k];
        const int64_t i = items ? items[k] : k;
        const slk_vec<VEC> a = slk_emb_vec<VEC>(U, ub, (uint32_t)u, D, d0, on);
        const slk_vec<VEC> b = slk_emb_vec<VEC>(V, ib, (uint32_t)i, D, d0, on);
        const float s = (slk_chain_dot<VEC, G>(a, b) + bu[u]) + bi[i];  // the score's definition: slk_kernels.h, slk_eval.hip
        if (lane == 0) out[k] = s;
    }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
typedef slk_pass_fn pass_fn;

template <int VEC, int G, bool BLOOM>
static pass_fn user_pass_fn2(int upd, int umode) {
    if (umode == 2) {
        if (upd == SLK_UPD_ADAGRAD) return k_user_pass<VEC, G, SLK_UPD_ADAGRAD, 2, BLOOM>;
        if (upd == SLK_UPD_SPARSE_ADAM) return k_user_pass<VEC, G, SLK_UPD_SPARSE_ADAM, 2, BLOOM>;
        if (upd == SLK_UPD_SGD) return k_user_pass<VEC, G, SLK_UPD_SGD, 2, BLOOM>;
        return k_user_pass<VEC, G, SLK_UPD_GRAD_ONLY, 2, BLOOM>;
    }
    if (umode == 1) {
        if (upd == SLK_UPD_ADAGRAD) return k_user_pass<VEC, G, SLK_UPD_ADAGRAD, 1, BLOOM>;
        if (upd == SLK_UPD_SPARSE_ADAM) return k_user_pass<VEC, G, SLK_UPD_SPARSE_ADAM, 1, BLOOM>;
        if (upd == SLK_UPD_SGD) return k_user_pass<VEC, G, SLK_UPD_SGD, 1, BLOOM>;
        return k_user_pass<VEC, G, SLK_UPD_GRAD_ONLY, 1, BLOOM>;
    }
    if (upd == SLK_UPD_ADAGRAD) return k_user_pass<VEC, G, SLK_UPD_ADAGRAD, 0, BLOOM>;
    if (upd == SLK_UPD_SPARSE_ADAM) return k_user_pass<VEC, G, SLK_UPD_SPARSE_ADAM, 0, BLOOM>;
    if (upd == SLK_UPD_SGD) return k_user_pass<VEC, G, SLK_UPD_SGD, 0, BLOOM>;
    return k_user_pass<VEC, G, SLK_UPD_GRAD_ONLY, 0, BLOOM>;
}

// the latency-bound form of the pair-mode user pass over plain tables (k_user_pass<..., LAT = true>)
template <int VEC, int G, bool ULONG = false>
static pass_fn user_pass_lat_fn(int upd) {
    if (upd == SLK_UPD_ADAGRAD) return k_user_pass<VEC, G, SLK_UPD_ADAGRAD, 0, false, true, ULONG>;
    if (upd == SLK_UPD_SPARSE_ADAM) return k_user_pass<VEC, G, SLK_UPD_SPARSE_ADAM, 0, false, true, ULONG>;
    if (upd == SLK_UPD_SGD) return k_user_pass<VEC, G, SLK_UPD_SGD, 0, false, true, ULONG>;
    return k_user_pass<VEC, G, SLK_UPD_GRAD_ONLY, 0, false, true, ULONG>;
}

// inside a user-row ping-pong scope (pair mode, plain tables, row-sparse optimizers): the four forms of the pass and the stitch
template <int VEC, int G, bool LAT, bool ULONG>
static pass_fn user_pass_pp_fn(int upd) {
    if (upd == SLK_UPD_ADAGRAD) return k_user_pass<VEC, G, SLK_UPD_ADAGRAD, 0, false, LAT, ULONG, true>;
    if (upd == SLK_UPD_SPARSE_ADAM) return k_user_pass<VEC, G, SLK_UPD_SPARSE_ADAM, 0, false, LAT, ULONG, true>;
    return k_user_pass<VEC, G, SLK_UPD_SGD, 0, false, LAT, ULONG, true>;
}
// ... with the single-occurrence fast path (Adagrad, the bandwidth-bound form) and the item pass that skips what it covered
template <int VEC, int G>
static pass_fn user_pass_sgl_fn() {
    return k_user_pass<VEC, G, SLK_UPD_ADAGRAD, 0, false, false, false, true, true>;
}
template <int VEC, int G>
static slk_item_fns item_pass_sgl_fn() {
    return {k_item_pass<VEC, G, SLK_UPD_ADAGRAD, SLK_ITEM_SNAPPPS>, k_item_stitch<VEC, G, SLK_UPD_ADAGRAD, SLK_PART_BOTH>,
            k_item_pass<VEC, G, SLK_UPD_ADAGRAD, SLK_ITEM_SNAPPPS, SLK_PART_BOTH, false>,
            k_item_pass<VEC, G, SLK_UPD_ADAGRAD, SLK_ITEM_SNAPPPS, SLK_PART_BOTH, false, 4>};
}
template <int VEC, int G>
static pass_fn user_stitch_pp_fn(int upd) {
    if (upd == SLK_UPD_ADAGRAD) return k_user_stitch<VEC, G, SLK_UPD_ADAGRAD, true>;
    if (upd == SLK_UPD_SPARSE_ADAM) return k_user_stitch<VEC, G, SLK_UPD_SPARSE_ADAM, true>;
    return k_user_stitch<VEC, G, SLK_UPD_SGD, true>;
}
template <int VEC, int G>
static slk_item_fns item_pass_pp_fn(int upd) {
    if (upd == SLK_UPD_ADAGRAD)
        return {k_item_pass<VEC, G, SLK_UPD_ADAGRAD, SLK_ITEM_SNAPPP>, k_item_stitch<VEC, G, SLK_UPD_ADAGRAD, SLK_PART_BOTH>,
                k_item_pass<VEC, G, SLK_UPD_ADAGRAD, SLK_ITEM_SNAPPP, SLK_PART_BOTH, false>,
                k_item_pass<VEC, G, SLK_UPD_ADAGRAD, SLK_ITEM_SNAPPP, SLK_PART_BOTH, false, 4>};
    if (upd == SLK_UPD_SPARSE_ADAM)
        return {k_item_pass<VEC, G, SLK_UPD_SPARSE_ADAM, SLK_ITEM_SNAPPP>, k_item_stitch<VEC, G, SLK_UPD_SPARSE_ADAM, SLK_PART_BOTH>,
                k_item_pass<VEC, G, SLK_UPD_SPARSE_ADAM, SLK_ITEM_SNAPPP, SLK_PART_BOTH, false>,
                k_item_pass<VEC, G, SLK_UPD_SPARSE_ADAM, SLK_ITEM_SNAPPP, SLK_PART_BOTH, false, 4>};
    return {k_item_pass<VEC, G, SLK_UPD_SGD, SLK_ITEM_SNAPPP>, k_item_stitch<VEC, G, SLK_UPD_SGD, SLK_PART_BOTH>,
            k_item_pass<VEC, G, SLK_UPD_SGD, SLK_ITEM_SNAPPP, SLK_PART_BOTH, false>,
            k_item_pass<VEC, G, SLK_UPD_SGD, SLK_ITEM_SNAPPP, SLK_PART_BOTH, false, 4>};
}

// plain tables, minibatches that hold a long user run (k_user_pass<..., ULONG = true>) and the stitch kernel behind it
template <int VEC, int G, int UMODE>
static pass_fn user_pass_long_fn1(int upd) {
    if (upd == SLK_UPD_ADAGRAD) return k_user_pass<VEC, G, SLK_UPD_ADAGRAD, UMODE, false, false, true>;
    if (upd == SLK_UPD_SPARSE_ADAM) return k_user_pass<VEC, G, SLK_UPD_SPARSE_ADAM, UMODE, false, false, true>;
    if (upd == SLK_UPD_SGD) return k_user_pass<VEC, G, SLK_UPD_SGD, UMODE, false, false, true>;
    return k_user_pass<VEC, G, SLK_UPD_GRAD_ONLY, UMODE, false, false, true>;
}
template <int VEC, int G>
static pass_fn user_pass_long_fn(int upd, int umode) {
    if (umode == 2) return user_pass_long_fn1<VEC, G, 2>(upd);
    if (umode == 1) return user_pass_long_fn1<VEC, G, 1>(upd);
    return user_pass_long_fn1<VEC, G, 0>(upd);
}
template <int VEC, int G>
static pass_fn user_stitch_fn(int upd) {
    if (upd == SLK_UPD_ADAGRAD) return k_user_stitch<VEC, G, SLK_UPD_ADAGRAD>;
    if (upd == SLK_UPD_SPARSE_ADAM) return k_user_stitch<VEC, G, SLK_UPD_SPARSE_ADAM>;
    if (upd == SLK_UPD_SGD) return k_user_stitch<VEC, G, SLK_UPD_SGD>;
    return k_user_stitch<VEC, G, SLK_UPD_GRAD_ONLY>;
}

template <int VEC, int G>
static pass_fn user_pass_fn(int upd, int umode, bool bloom) {
    return bloom ? user_pass_fn2<VEC, G, true>(upd, umode) : user_pass_fn2<VEC, G, false>(upd, umode);
}


int slk_check_tables(slk_ctx *ctx, const slk_tables *t, unsigned table_mask, int *vec, int *g, bool shadow_ok, bool pingpong_ok) {
    if (!t) return slk_fail(ctx, SLK_EINVAL, "tables is NULL");
    for (int i = 0; i < 4; ++i)
        if (((table_mask >> i) & 1u) && !t->d_param[i])
            return slk_fail(ctx, SLK_EINVAL, "tables->d_param[%d] is NULL", i);
    if (!shadow_ok && (table_mask & 8u) && ctx->shadow_active && t->d_param[3] == ctx->shadow_src_p)
        return slk_fail(ctx, SLK_EINVAL, "the item biases of these tables are shadowed (slk_bias_shadow_begin): the array is stale until "
                                         "slk_bias_shadow_end, and only slk_bilinear_train indexes the shadow");
    if (!pingpong_ok && (table_mask & 1u) && ctx->pp_active && t->d_param[0] == ctx->pp_src_u)
        return slk_fail(ctx, SLK_EINVAL, "the user rows of these tables are ping-ponged (slk_user_pingpong_begin): the array holds only "
                                         "some of the current rows until slk_user_pingpong_end, and only slk_bilinear_train reads both copies");
    if (((table_mask & 5u) && (t->num_users < 1 || t->num_users >= ((int64_t)1 << 31))) || t->num_items < 1 ||
        t->num_items >= ((int64_t)1 << 31))
        return slk_fail(ctx, SLK_EINVAL, "table rows must be in [1, 2^31): users %lld items %lld",
                        (long long)t->num_users, (long long)t->num_items);
    if (!slk_pick_layout(t->dim, vec, g))
        return slk_fail(ctx, SLK_EINVAL,
                        "embedding dim %d unsupported (need dim %% 4 == 0 and <= 256, or dim <= 64)", t->dim);
    const slk_bloom *bl[2] = {(table_mask & 1u) ? t->user_bloom : nullptr, (table_mask & 2u) ? t->item_bloom : nullptr};
    for (int side = 0; side < 2; ++side) {
        const slk_bloom *b = bl[side];
        if (!b) continue;
        if (b->n_hash < 1 || b->n_hash > 8 || b->rows < 1 || b->rows >= ((int64_t)1 << 30) || b->skip_row >= b->rows ||
            b->skip_row < -1 || b->padding_idx < -1)
            return slk_fail(ctx, SLK_EINVAL, "bad BloomEmbedding descriptor: rows %lld n_hash %d skip_row %lld",
                            (long long)b->rows, b->n_hash, (long long)b->skip_row);
    }
    return SLK_OK;
}

int slk_check_optim(slk_ctx *ctx, const slk_optim *optim, unsigned table_mask) {
    if (!optim) return slk_fail(ctx, SLK_EINVAL, "optim is NULL");
    if (optim->kind < SLK_OPT_ADAGRAD || optim->kind > SLK_OPT_SGD)
        return slk_fail(ctx, SLK_EINVAL, "unknown optimizer kind %d", optim->kind);
    if (optim->kind == SLK_OPT_SGD) {  // stateless
        if (optim->weight_decay != 0.0) return slk_fail(ctx, SLK_EINVAL, "SGD: weight_decay must be 0 (a full-table sweep per step is not built)");
        return SLK_OK;
    }
    const bool need_s2 = slk_opt_has_s2(optim->kind);
    for (int i = 0; i < 4; ++i) {
        if (!((table_mask >> i) & 1u)) continue;
        if (!optim->d_state1[i]) return slk_fail(ctx, SLK_EINVAL, "optim->d_state1[%d] is NULL", i);
        if (need_s2 && !optim->d_state2[i]) return slk_fail(ctx, SLK_EINVAL, "optim->d_state2[%d] is NULL", i);
    }
    if (optim->kind == SLK_OPT_ADAGRAD && optim->weight_decay != 0.0)
        return slk_fail(ctx, SLK_EINVAL, "row-sparse Adagrad requires weight_decay == 0 (use ADAGRAD_DENSE)");
    return SLK_OK;
}

int slk_ensure_dgrad(slk_ctx *ctx, const size_t elems[4], unsigned table_mask, hipStream_t s) {
    for (int t = 0; t < 4; ++t) {
        if (!((table_mask >> t) & 1u)) continue;
        if (ctx->dgrad_elems[t] != elems[t] || !ctx->dgrad[t].p) {
            int rc = slk_ensure(ctx, ctx->dgrad[t], elems[t] * 4);
            if (rc) return rc;
            SLK_HIP(ctx, hipMemsetAsync(ctx->dgrad[t].p, 0, elems[t] * 4, s));
            ctx->dgrad_elems[t] = elems[t];
        }
    }
    return SLK_OK;
}

// Reference default optimizer (Adam + l2) / dense Adagrad with weight decay: sweep every row of
// the tables in `table_mask`, consuming (and re-zeroing) the dense gradient buffers.
int slk_dense_sweeps(slk_ctx *ctx, float *const params[4], const slk_optim *optim, unsigned table_mask,
                     hipStream_t s) {
    slk_prof_begin(ctx, SLK_K_DENSE_SWEEP, s);
    slk_sweep_all_args w;
    memset(&w, 0, sizeof(w));
    w.adam = optim->kind == SLK_OPT_ADAM_DENSE;
    w.coef = slk_opt_coef_at(optim, optim->step + 1);
    w.hyper = slk_opt_hyper_of(optim);
    unsigned blocks = 0;
    for (int t = 0; t < 4; ++t) {
        w.first[t] = blocks;
        if (!((table_mask >> t) & 1u)) continue;
        w.p[t] = params[t];
        w.s1[t] = optim->d_state1[t];
        w.s2[t] = optim->d_state2[t];
        w.g[t] = (float *)ctx->dgrad[t].p;
        w.numel[t] = ctx->dgrad_elems[t];
        blocks += slk_grid_for(ctx, w.numel[t], 256);
    }
    w.first[4] = blocks;
    if (blocks) {
        hipLaunchKernelGGL(k_dense_sweep_all, dim3(blocks), dim3(256), 0, s, w);
        SLK_LAUNCH_CHECK(ctx, "k_dense_sweep_all");
    }
    slk_prof_end(ctx, s);
    return SLK_OK;
}

int slk_launch_i64_to_u32(slk_ctx *ctx, const int64_t *in, uint32_t *out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_i64_to_u32, dim3(slk_grid_for(ctx, n, 256)), dim3(256), 0, s, in, out, n);
    SLK_LAUNCH_CHECK(ctx, "k_i64_to_u32");
    return SLK_OK;
}

int slk_prep_given_negatives(slk_ctx *ctx, const int64_t *neg_in, int64_t *neg_out, size_t n, slk_prep_bufs &pb, hipStream_t s) {
    int rc;
    slk_prof_begin(ctx, SLK_K_SAMPLE, s);
    if ((rc = slk_launch_i64_to_u32(ctx, neg_in, (uint32_t *)pb.neg32.p, n, s))) return rc;
    if (neg_out) SLK_HIP(ctx, hipMemcpyAsync(neg_out, neg_in, n * 8, hipMemcpyDeviceToDevice, s));
    slk_prof_end(ctx, s);
    return SLK_OK;
}

void slk_fill_table_args(slk_pass_args &a, const slk_ctx *ctx, const slk_tables *tables, const slk_optim *optim, bool dense) {
    for (int t = 0; t < 4; ++t) {
        a.P[t] = tables->d_param[t];
        a.S1[t] = dense ? (float *)ctx->dgrad[t].p : optim->d_state1[t];
        a.S2[t] = optim->d_state2[t];
    }
}

SLK_EXPORT int slk_bilinear_predict(slk_ctx *ctx, const slk_tables *tables, const int64_t *d_users,
                                    int64_t n_users, const int64_t *d_items, int64_t n, float *d_out,
                                    void *stream) {
    if (!ctx) return SLK_EINVAL;
    int vec, g, rc;
    if ((rc = slk_check_tables(ctx, tables, 15u, &vec, &g))) return rc;
    if (n < 0 || !d_users || (n > 0 && !d_out)) return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_predict: bad arguments");
    if (n_users != 1 && n_users != n)
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_predict: n_users must be 1 or n (%lld vs %lld)",
                        (long long)n_users, (long long)n);
    if (n == 0) return SLK_OK;
    SLK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    ctx->last_stream = s;
    slk_prof_begin(ctx, SLK_K_SCORE, s);
    if (n_users == 1 && !d_items) {
        // one user against EVERY item: the item table streams through the matrix cores (slk_eval.hip), same scores bit for bit
        if (n != tables->num_items)
            return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_predict: d_items == NULL scores all %lld items, n is %lld",
                            (long long)tables->num_items, (long long)n);
        const float *rep, *rbias;
        const int64_t *gmap;
        if ((rc = slk_eval_user_rep(ctx, tables, vec, g, d_users, &rep, &rbias, &gmap, s))) return rc;
        rc = slk_eval_predict_all(ctx, tables, rep, rbias, gmap, d_out, s);
        slk_prof_end(ctx, s);
        return rc;
    }
#define SLK_PREDICT(V_, G_)                                                                          \
    hipLaunchKernelGGL((k_predict<V_, G_>), dim3(slk_grid_for(ctx, (size_t)n, 256 / G_)), dim3(256), 0, s, \
                       (const float *)tables->d_param[0], (const float *)tables->d_param[1],          \
                       (const float *)tables->d_param[2], (const float *)tables->d_param[3],          \
                       (int)tables->dim, ubd, ibd, d_users, n_users, d_items, n, d_out)
    slk_bloom_dev ubd, ibd;
    slk_bloom_to_dev(tables->user_bloom, &ubd);
    slk_bloom_to_dev(tables->item_bloom, &ibd);
    SLK_FOR_LAYOUT(vec, g, SLK_PREDICT);
#undef SLK_PREDICT
    SLK_LAUNCH_CHECK(ctx, "k_predict");
    slk_prof_end(ctx, s);
    return SLK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The training driver.  A call is (1) taken down as given (train_call), (2) planned: every derived value and every refusal,
// before any GPU work (plan_training), (3) given its scratch (ensure_scratch; slk_bilinear_reserve stops behind it), (4) its
// kernels (pick_kernels), and (5) scheduled: chunk by chunk, the value-independent prep of a chunk (prep_sample, prep_sort)
// and its minibatches (run_chunk: score_stage, user_stage, item_stage) in line (run_inline), one chunk ahead
// (run_pipelined), or the first chunk a whole call ahead (prefetch_first_chunk).
// ---------------------------------------------------------------------------------------------------------------------------
struct train_call {  // the arguments as given (ratings: explicit feedback, and only it; weights: slk_bilinear_train_weighted, and only it)
    enum { TRAIN, RESERVE, PREFETCH } mode;
    const slk_tables *tables;
    slk_optim *optim;
    const int64_t *users, *items;
    const float *ratings;
    const int64_t *neg_in;
    int64_t *neg_out;
    float *mb_loss;
    int64_t n, batch_size;
    int32_t loss, n_neg;
    hipStream_t s;
    const float *weights;
};

struct train_plan {  // everything derived from a call and the ctx's options before any GPU work
    int vec, g, D;
    // RS: record = the pre-step user row (16-B granular; D = 64: two aligned 128-B lines); RSU: user-bloom gradient record (+ an
    // unused bias slot); hot users (k_user_pass<..., ULONG>): two partials of UPS floats per tile of SLK_USER_TILE positions
    int RS, RSU, UPS;
    size_t utiles;
    unsigned ubits, ibits, ucbits, icbits;
    slk_bloom_dev ubd, ibd;  // BloomEmbedding layers (layers.py:74-244): keys of the row-owner passes are hashed rows
    int Hu, Hi;
    // expl: explicit feedback (ratings, no negatives); fused: ... whose user pass forms score, loss and dL/dscore itself (option
    // "explicit_fused"); pre: dL/dscore is computed before the user pass; weighted: interaction weights -- every loss staged
    // (`pre`, never `fused`, never the persistent route), the pair losses with their NP = 2 through k_pair_loss_weighted
    bool bloom, adaptive, multi, expl, fused, pre, dense, late, weighted;
    int nn, NP, umode, nsets;
    int64_t bsz, mb_per_chunk, chunk_cap, occ_mult;
    // chunk ck is [ck * chunk_cap, min(n, (ck + 1) * chunk_cap)): nc_max interactions in the largest (= the first); 0 chunks: an empty call
    size_t nc_max, n_chunks;
    // one_draw: the negatives of the WHOLE call are one draw of the sampler, not one per chunk; epoch_route: as planned -- the
    // persistent route may still refuse its first launch (train_run)
    bool side, pingpong, sgl_on, shadowed, one_draw, epoch_route;
    size_t dense_elems[4];  // the *_DENSE optimizers' gradient buffers
};

struct train_run {  // what changes while a call runs
    const uint32_t *neg_all;  // negatives of the whole call drawn ahead (ctx->pf_neg, ctx->call_neg): the chunks read theirs from it
    int64_t mb_global;        // minibatches done
    bool epoch_route;         // false from the first chunk on whose cooperative launch was refused
};

struct train_kernels {
    pass_fn upass, spass, upass_lat, upass_long, upass_lat_long, ustitch, upass_sgl;
    slk_item_fns ipass, ipass_rows, ipass_bias, rpass_rows, ipass_sgl;
    unsigned gpb;
    int occ_user, occ_sgl;
};

static inline uint32_t *u32p(const slk_buf &b) { return (uint32_t *)b.p; }
static inline float *f32p(const slk_buf &b) { return (float *)b.p; }
static inline int64_t chunk_begin(const train_plan &p, size_t ck) { return (int64_t)ck * p.chunk_cap; }
static inline uint32_t chunk_len(const train_plan &p, const train_call &c, size_t ck) {
    const int64_t c1 = chunk_begin(p, ck + 1);
    return (uint32_t)((c1 < c.n ? c1 : c.n) - chunk_begin(p, ck));
}

static inline uint32_t weight_segs(const train_plan &p) { return (uint32_t)(((size_t)p.bsz + SLK_WSEG - 1) / SLK_WSEG); }

static int run_training(slk_ctx *ctx, const train_call &c);

SLK_EXPORT int slk_bilinear_train(slk_ctx *ctx, const slk_tables *tables, slk_optim *optim,
                                  const int64_t *d_users, const int64_t *d_items, int64_t n,
                                  int64_t batch_size, int32_t loss, int32_t n_neg, const int64_t *d_neg_in,
                                  int64_t *d_neg_out, float *d_mb_loss, void *stream) {
    return run_training(ctx, {train_call::TRAIN, tables, optim, d_users, d_items, nullptr, d_neg_in, d_neg_out, d_mb_loss, n,
                              batch_size, loss, n_neg, (hipStream_t)stream});
}

SLK_EXPORT int slk_bilinear_reserve(slk_ctx *ctx, const slk_tables *tables, const slk_optim *optim, int64_t n,
                                    int64_t batch_size, int32_t loss, int32_t n_neg, void *stream) {
    slk_optim o;
    if (!optim) return slk_fail(ctx, SLK_EINVAL, "optim is NULL");
    o = *optim;
    return run_training(ctx, {train_call::RESERVE, tables, &o, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n, batch_size,
                              loss, n_neg, (hipStream_t)stream});
}

// The FIRST chunk of the next slk_bilinear_train call with these very arguments, prepared now: its negatives and sorts go to
// the ctx's prep stream, beside whatever the caller's stream still holds (the passes of the epoch before).  fit() calls it as
// soon as the next epoch's shuffled ids exist; h_key / pos (optional): the MT19937 state the call's draws start from, written
// without waiting for the ctx's stream (the caller has waited for the last draw: slk_rng_get_state_sampled).  A no-op for
// calls that would not pipeline their prep (a single chunk, minibatches below "overlap_min_batch", the persistent route).
SLK_EXPORT int slk_bilinear_prefetch(slk_ctx *ctx, const slk_tables *tables, const slk_optim *optim, const int64_t *d_users,
                                     const int64_t *d_items, int64_t n, int64_t batch_size, int32_t loss, int32_t n_neg,
                                     const uint32_t *h_key, int32_t pos, void *stream) {
    if (!ctx) return SLK_EINVAL;
    if (!optim) return slk_fail(ctx, SLK_EINVAL, "optim is NULL");
    if (h_key) {
        if (pos < 0 || pos > 624) return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_prefetch: pos %d outside [0, 624]", pos);
        SLK_HIP(ctx, hipSetDevice(ctx->device));
        if (ctx->sampled_valid && ctx->ev_sampled) SLK_HIP(ctx, hipEventSynchronize(ctx->ev_sampled));
        int rc = slk_rng_write_state(ctx, h_key, pos);
        if (rc) return rc;
    }
    slk_optim o = *optim;
    return run_training(ctx, {train_call::PREFETCH, tables, &o, d_users, d_items, nullptr, nullptr, nullptr, nullptr, n, batch_size,
                              loss, n_neg, (hipStream_t)stream});
}

// ExplicitFactorizationModel.fit's minibatch loop (spotlight/factorization/explicit.py:213-236): the same
// passes with ONE pair per interaction, dL/dscore from k_explicit_loss (the PRE route of the user pass)
SLK_EXPORT int slk_bilinear_train_explicit(slk_ctx *ctx, const slk_tables *tables, slk_optim *optim,
                                           const int64_t *d_users, const int64_t *d_items, const float *d_ratings,
                                           int64_t n, int64_t batch_size, int32_t loss, float *d_mb_loss,
                                           void *stream) {
    if (ctx && !slk_loss_is_explicit(loss))
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_train_explicit: loss kind %d%s is not regression/poisson/logistic", loss,
                        loss == SLK_LOSS_WARP ? " (warp)" : (loss == SLK_LOSS_SOFTMAX ? " (softmax)" : ""));
    if (ctx && n > 0 && !d_ratings) return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_train_explicit: d_ratings is NULL");
    return run_training(ctx, {train_call::TRAIN, tables, optim, d_users, d_items, d_ratings, nullptr, nullptr, d_mb_loss, n,
                              batch_size, loss, 0, (hipStream_t)stream});
}

// Interaction weights (include/spotlight_hip.h): either loss family with L = sum(w_i l_i) / sum(w_i) per minibatch.  Every
// loss takes the staged route -- k_score_pass, a weighted loss kernel, the user pass reading dL/dscore (UMODE 1) -- so that
// neither hot pass knows of the weights.  The weights' VALUES are the caller's responsibility, as ids are.
SLK_EXPORT int slk_bilinear_train_weighted(slk_ctx *ctx, const slk_tables *tables, slk_optim *optim, const int64_t *d_users,
                                           const int64_t *d_items, const float *d_weights, const float *d_ratings, int64_t n,
                                           int64_t batch_size, int32_t loss, int32_t n_neg, const int64_t *d_neg_in,
                                           int64_t *d_neg_out, float *d_mb_loss, void *stream) {
    if (ctx && n > 0 && !d_weights) return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_train_weighted: d_weights is NULL");
    // (n == 0: a no-op like every training call; a non-NULL stand-in keeps the plan a weighted one, so the refusals are the same)
    static const float none = 1.0f;
    return run_training(ctx, {train_call::TRAIN, tables, optim, d_users, d_items, d_ratings, d_neg_in, d_neg_out, d_mb_loss, n,
                              batch_size, loss, d_ratings ? 0 : n_neg, (hipStream_t)stream, d_weights ? d_weights : &none});
}

// Every derived value of a call and every refusal, in the order the rules have always been checked in (where a call breaks
// several, the first one answers).  Touches nothing on the GPU; of the ctx only the current device and the noted stream.
static int plan_training(slk_ctx *ctx, const train_call &c, train_plan *plan) {
    train_plan &p = *plan;
    const slk_tables *tables = c.tables;
    const slk_optim *optim = c.optim;
    const bool reserve = c.mode == train_call::RESERVE, prefetch = c.mode == train_call::PREFETCH;
    const int64_t n = c.n;
    int rc;
    p.n_chunks = 0;
    if ((rc = slk_check_tables(ctx, tables, 15u, &p.vec, &p.g, /*shadow_ok=*/true, /*pingpong_ok=*/true))) return rc;
    if ((rc = slk_check_optim(ctx, optim, 15u))) return rc;
    if (n < 0 || c.batch_size < 1) return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_train: n %lld batch_size %lld",
                                                   (long long)n, (long long)c.batch_size);
    if (c.loss < SLK_LOSS_POINTWISE || c.loss > SLK_LOSS_SOFTMAX)
        return slk_fail(ctx, SLK_EINVAL, "unknown loss kind %d", c.loss);
    // (`adaptive`: a COLUMN loss -- adaptive hinge or warp; they differ in k_adaptive_select's rule alone.  `multi`: n_neg draws
    // per positive, all scored ahead of the user pass -- the column losses and sampled softmax, whose 1 + n occurrences are ALL
    // live: never `late`, never the persistent route)
    p.adaptive = slk_loss_is_column(c.loss);
    p.multi = slk_loss_is_multi(c.loss);
    p.expl = slk_loss_is_explicit(c.loss);
    if (p.expl != (c.ratings != nullptr) && !reserve)
        return slk_fail(ctx, SLK_EINVAL, "ratings go with (and only with) the regression/poisson/logistic losses");
    p.weighted = c.weights != nullptr;
    p.fused = p.expl && ctx->opt_explicit_fused && !p.weighted;
    p.pre = p.multi || p.expl || p.weighted;
    p.umode = p.fused ? 2 : (p.pre ? 1 : 0);
    p.nn = p.multi ? c.n_neg : (p.expl ? 0 : 1);
    if (!p.expl && (p.nn < 1 || p.nn > 1024)) return slk_fail(ctx, SLK_EINVAL, "num_negative_samples %d outside [1, 1024]", p.nn);
    p.NP = p.nn + 1;
    p.dense = slk_opt_is_dense(optim->kind);
    if (n == 0) return SLK_OK;
    if (!reserve && (!c.users || !c.items || (!c.mb_loss && !prefetch)))
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_train: NULL id/loss pointer");
    if (c.batch_size * (int64_t)p.NP >= ((int64_t)1 << 31))
        return slk_fail(ctx, SLK_EINVAL, "batch_size * (1 + negatives) must be < 2^31");
    SLK_HIP(ctx, hipSetDevice(ctx->device));
    ctx->last_stream = c.s;

    p.D = tables->dim;
    p.ubits = slk_bits_for((uint64_t)tables->num_users - 1);
    p.ibits = slk_bits_for((uint64_t)tables->num_items - 1);
    unsigned idbits = p.ubits > p.ibits ? p.ubits : p.ibits;
    slk_bloom_to_dev(tables->user_bloom, &p.ubd);
    slk_bloom_to_dev(tables->item_bloom, &p.ibd);
    p.bloom = p.ubd.n_hash || p.ibd.n_hash;
    const int Hu = p.Hu = p.ubd.n_hash, Hi = p.Hi = p.ibd.n_hash;
    p.ucbits = Hu ? slk_bits_for((uint64_t)p.ubd.rows) : 0;  // + the non-head sentinel row
    p.icbits = Hi ? slk_bits_for((uint64_t)p.ibd.rows - 1) : 0;
    if (p.ucbits > idbits) idbits = p.ucbits;
    if (p.icbits > idbits) idbits = p.icbits;
    p.occ_mult = (int64_t)p.NP * (Hi ? Hi : 1) > (int64_t)(Hu ? Hu : 1) ? (int64_t)p.NP * (Hi ? Hi : 1) : (int64_t)(Hu ? Hu : 1);
    // minibatches per chunk: keys must fit 32 bits, occurrences must fit 2^31, and scratch
    // stays bounded (~8M interactions).
    const int64_t bsz = p.bsz = c.batch_size < n ? c.batch_size : n;
    int64_t mb_per_chunk = (int64_t)1 << (32 - idbits);
    // ~8M interactions per chunk (option "chunk_interactions"): large enough for the sorts and the
    // MT19937 jump-ahead sampler to fill the GPU, small enough to bound the scratch
    const int64_t cap_inter = ctx->opt_chunk_interactions;
    if (mb_per_chunk * bsz > cap_inter) mb_per_chunk = cap_inter / bsz;
    while (mb_per_chunk > 1 && mb_per_chunk * bsz * p.occ_mult >= ((int64_t)1 << 31)) mb_per_chunk >>= 1;
    if (mb_per_chunk < 1) mb_per_chunk = 1;
    if (bsz * p.occ_mult >= ((int64_t)1 << 31))
        return slk_fail(ctx, SLK_EINVAL, "batch_size * lookups per interaction must be < 2^31");
    // the persistent route (slk_epoch.hip) keeps per-(minibatch, workgroup) loss partials and counts barriers in 32 bits:
    // at most 2^13 minibatches per launch (16 MB of partials at 256 workgroups)
    const bool maybe_epoch = ctx->opt_epoch_kernel && !ctx->epoch_refused && bsz <= ctx->opt_epoch_max_batch && !p.weighted &&
                            c.loss != SLK_LOSS_SOFTMAX;
    if (maybe_epoch && mb_per_chunk > ((int64_t)1 << 13)) mb_per_chunk = (int64_t)1 << 13;
    p.mb_per_chunk = mb_per_chunk;
    // chunks of chunk_cap.  Chunking is value-neutral: the negatives of a call are one contiguous draw however
    // it is cut.  (Ramped chunks and a short first chunk for the overlapped prep were measured in round 3 and lost at every
    // call length -- small chunks pay the sampler's jump-ahead and the sorts' fixed costs again: profiles/r03_c_*, r03_w_*.)
    p.chunk_cap = mb_per_chunk * bsz;
    p.nc_max = (size_t)(p.chunk_cap < n ? p.chunk_cap : n);
    p.n_chunks = (size_t)((n + p.chunk_cap - 1) / p.chunk_cap);

    // Adaptive hinge: only the positive and the selected negative of a column carry a gradient, so
    // the item-side owner passes run over 2 live occurrences per interaction (sorted per minibatch,
    // after the selection) instead of all 1+n.  Not for SparseAdam, which also decays the moments
    // of looked-up rows whose gradient is zero.
    // Below `adaptive_late_min_batch` interactions per minibatch the per-minibatch sort of the live occurrences (half a dozen
    // small launches) costs more than the dead occurrences it removes from the item pass: all 1+n are sorted once per chunk.
    p.late = p.adaptive && optim->kind != SLK_OPT_SPARSE_ADAM && (Hi > 0 || bsz >= ctx->opt_adaptive_late_min_batch);
    // Two buffer sets whenever a call has more than one chunk: chunk c + 1 is prepared (negatives, sorts) BEFORE chunk c's passes are
    // enqueued.  `side`: that preparation goes to the ctx's second stream and runs BESIDE the passes (option "overlap_prep", what
    // fit() sets).  Otherwise (a bare ctx; round 6) it goes to the caller's own stream, one chunk ahead: still one stream, every
    // kernel alone on the GPU -- but the host's one wait per chunk (the long-run flags of prep_sort) now falls while the GPU works on
    // the next chunk's prep instead of idling (a bubble of ~40 us per chunk of 8 minibatches in rounds 1-5).
    p.side = ctx->opt_overlap_prep && p.n_chunks > 1 && bsz >= ctx->opt_overlap_min_batch;
    p.nsets = p.n_chunks > 1 ? 2 : 1;
    // The negatives of the WHOLE call in ONE draw (it is one contiguous draw however the call is chunked): the generator's
    // jump-ahead, ~130 us whatever the draw's length, is paid once per call instead of once per chunk (round 6: 0.0135 -> 0.0065
    // ms per C2 step at 20 minibatches per call).  Calls of >= 2^30 draws and calls that are handed their negatives keep
    // drawing / converting by chunk.
    p.one_draw = !c.neg_in && p.nn > 0 && p.n_chunks > 1 && (uint64_t)n * (uint64_t)p.nn < ((uint64_t)1 << 30);
    p.RS = (p.D + 3) / 4 * 4;
    p.UPS = p.RS + 4;
    p.utiles = ((size_t)bsz + SLK_USER_TILE - 1) / SLK_USER_TILE;
    p.RSU = p.D + 4;
    // user-row ping-pong of a training scope (slk_user_pingpong_begin): pair mode over plain tables with a row-sparse optimizer on
    // the launch path -- the user pass writes the updated row to the other copy and no record, the item pass gathers the pre-step
    // row from the copy the user pass read.  A call the scope cannot serve is refused, not trained beside it.
    p.pingpong = ctx->pp_active && ctx->pp_src_u == tables->d_param[0];
    if (ctx->pp_active && !p.pingpong && !reserve)
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_train: a user-row ping-pong (slk_user_pingpong_begin) is open on this ctx for OTHER "
                                         "tables; close it (slk_user_pingpong_end / _abort) before training another model");
    if (p.pingpong && p.weighted)
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_train_weighted: the user rows are ping-ponged (slk_user_pingpong_begin): a call "
                                         "with interaction weights forms dL/dscore ahead of the user pass and does not train inside the scope");
    if (p.pingpong && (p.pre || p.bloom || p.dense || tables->num_users != ctx->pp_rows || p.D != ctx->pp_dim))
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_train: the user rows are ping-ponged (slk_user_pingpong_begin): only the pair losses "
                                         "(pointwise, bpr, hinge) over plain tables of the scope's shape with a row-sparse optimizer train inside the scope");
    // The single-occurrence fast path (k_user_pass<..., SGL>): inside a ping-pong scope, row-sparse Adagrad, item tables of at
    // least "item_single_min_items" rows (default 2^24: a catalogue far larger than a minibatch, where nearly every occurrence is
    // the only one of its item; at C2 -- two occurrences per item on average -- 12 % qualify and the flags would cost more)
    // (a call that got here with `pingpong` has a pair loss, plain tables and a row-sparse optimizer: the refusal above)
    p.sgl_on = p.pingpong && optim->kind == SLK_OPT_ADAGRAD && ctx->opt_item_single_min_items > 0 &&
               tables->num_items >= ctx->opt_item_single_min_items;
    // the item-bias shadow of a training scope (slk_bias_shadow_begin): the launch path's kernels index it, the persistent
    // kernel does not -- a call whose biases are shadowed takes the launches
    p.shadowed = ctx->shadow_active && ctx->shadow_src_p == tables->d_param[3] && !p.dense &&
                 optim->kind == SLK_OPT_ADAGRAD && ctx->shadow_src_s == optim->d_state1[3];
    if (ctx->shadow_active && !p.shadowed && ctx->shadow_src_p == tables->d_param[3])
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_train: the item biases are shadowed (slk_bias_shadow_begin) for another optimizer state");
    // One scope per ctx, and the scope is a TRAINING scope of ONE model (ABI 11): a training call on other tables while it is
    // open is a caller that has lost track of the scope -- refused, not trained beside it (the scope's _end would otherwise
    // write through pointers whose owner may have moved on).  slk_bilinear_reserve allocates only and stays allowed.
    if (ctx->shadow_active && !p.shadowed && !reserve)
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_train: an item-bias shadow (slk_bias_shadow_begin) is open on this ctx for OTHER "
                                         "tables; close it (slk_bias_shadow_end / _abort) before training another model");
    // minibatches of a few thousand interactions: every minibatch of a chunk inside ONE persistent launch (slk_epoch.hip)
    p.epoch_route = !p.weighted && !p.shadowed && !p.pingpong && (!p.pre || p.adaptive || p.fused) &&
                    slk_epoch_eligible(ctx, tables, optim, bsz, c.loss, p.bloom);
    p.dense_elems[0] = (size_t)(Hu ? p.ubd.rows : tables->num_users) * p.D;
    p.dense_elems[1] = (size_t)(Hi ? p.ibd.rows : tables->num_items) * p.D;
    p.dense_elems[2] = (size_t)tables->num_users;
    p.dense_elems[3] = (size_t)tables->num_items;
    return SLK_OK;
}

static int ensure_dense_buffers(slk_ctx *ctx, const train_plan &p, hipStream_t s) { return slk_ensure_dgrad(ctx, p.dense_elems, 15u, s); }

// scratch.  With the "overlap_prep" option the value-independent part of a chunk (negatives,
// sort by user, sort by item) is prepared on a second HIP stream while the previous chunk's
// passes run, and those buffers exist twice (ctx->pb[0|1]).  What fit() sets for its epochs (profiles/r03_a_*, r03_b_*: with
// two of the user pass's eight workgroups per CU left to the prep stream the steady state of a run of training calls gains
// 1.5-4 %; round 1 had measured no gain with the pass holding every wave slot); off on a bare ctx (slk_common.h).
static int ensure_scratch(slk_ctx *ctx, const train_plan &p, hipStream_t s) {
    const size_t nc_max = p.nc_max, NP = (size_t)p.NP, Hi = (size_t)p.Hi, Hu = (size_t)p.Hu, bsz = (size_t)p.bsz;
    const bool late = p.late;
    int rc;
    for (int st = 0; st < p.nsets; ++st) {
        slk_prep_bufs &pb = ctx->pb[st];
        if ((rc = slk_ensure(ctx, pb.neg32, nc_max * p.nn * 4))) return rc;
        for (int b = 0; b < 2; ++b) {
            if ((rc = slk_ensure(ctx, pb.ukey[b], nc_max * 4))) return rc;
            if ((rc = slk_ensure(ctx, pb.uval[b], nc_max * 8))) return rc;
            // `late`: the item-side lists are built per minibatch from the live occurrences only;
            // ipay[0] then holds the interaction -> sorted-position map of the chunk
            if (!late && (rc = slk_ensure(ctx, pb.ikey[b], nc_max * NP * 4))) return rc;
            if (!(late && b == 1) && (rc = slk_ensure(ctx, pb.ipay[b], late ? nc_max * 4 : nc_max * NP * 4))) return rc;
            if (!late && Hi && (rc = slk_ensure(ctx, pb.bik[b], nc_max * NP * Hi * 4))) return rc;
            if (!late && Hi && (rc = slk_ensure(ctx, pb.bip[b], nc_max * NP * Hi * 4))) return rc;
            if (Hu && (rc = slk_ensure(ctx, pb.buk[b], nc_max * Hu * 4))) return rc;
            if (Hu && (rc = slk_ensure(ctx, pb.bup[b], nc_max * Hu * 4))) return rc;
        }
        if (p.pre && (rc = slk_ensure(ctx, pb.uit, nc_max * NP * 4))) return rc;
        if (p.sgl_on && (rc = slk_ensure(ctx, pb.mflag, nc_max * NP + 16))) return rc;    // "occurs more than once" per occurrence: by payload,
        if (p.sgl_on && (rc = slk_ensure(ctx, pb.msorted, nc_max * NP + 16))) return rc;  //   in item-sorted order
        if ((rc = slk_ensure(ctx, pb.lflags, 2 * (size_t)p.mb_per_chunk * 4))) return rc;  // long-run flags of a chunk: items, users
    }
    if ((rc = slk_ensure(ctx, ctx->snap, bsz * p.RS * 4))) return rc;
    // dL/dscore per (position, pair); ping-pong: {dL/dscore, src} per (position, pair)
    if ((rc = slk_ensure(ctx, ctx->extra[BL_GSN], bsz * NP * (p.pingpong ? 8 : 4)))) return rc;
    const unsigned max_grid = (unsigned)ctx->num_cus * (unsigned)(ctx->opt_user_grid_mult > 8 ? ctx->opt_user_grid_mult : 8);
    if ((rc = slk_ensure(ctx, ctx->losspart, (size_t)max_grid * 8))) return rc;
    if (p.pre) {
        if ((rc = slk_ensure(ctx, ctx->gk, nc_max * NP * 4))) return rc;
        if ((rc = slk_ensure(ctx, ctx->sk, nc_max * NP * 4))) return rc;
    }
    // the weight sums of a chunk's minibatches and their per-segment partials (k_weight_partials): a few KB, so a plan of
    // ANY kind holds them -- slk_bilinear_reserve does not know whether the call it stands for carries weights
    {
        const size_t n_mb = (nc_max + bsz - 1) / bsz;
        if ((rc = slk_ensure(ctx, ctx->extra[BL_WSUM], n_mb * 8))) return rc;
        if ((rc = slk_ensure(ctx, ctx->extra[BL_WPART], n_mb * weight_segs(p) * 8))) return rc;
    }
    if (late) {
        // (the live lists are sorted per minibatch on the PASSES' stream; with the overlapped prep another chunk's sorts run on
        // the prep stream at the same time, so these sorts have temporary storage of their own: BL_LATE_SORT, not ctx->sort_tmp)
        const size_t nl = 2 * bsz, nlh = nl * (Hi ? Hi : 1);
        if ((rc = slk_ensure(ctx, ctx->extra[BL_LIVE], nl * 4))) return rc;
        for (int b = 0; b < 4; ++b)
            if ((rc = slk_ensure(ctx, ctx->extra[BL_LK0 + b], nlh * 4))) return rc;
    }
    if (!p.bloom) {
        if ((rc = slk_ensure(ctx, ctx->extra[BL_UPART], 2 * p.utiles * (size_t)p.UPS * 4))) return rc;
        const size_t meta_bytes = 2 * p.utiles * 8 + 64;
        if (meta_bytes > ctx->upart_meta.cap) {
            if ((rc = slk_ensure(ctx, ctx->upart_meta, meta_bytes))) return rc;
            SLK_HIP(ctx, hipMemsetAsync(ctx->upart_meta.p, 0, ctx->upart_meta.cap, s));  // stamp 0 is never used
        }
    }
    if (Hu && (rc = slk_ensure(ctx, ctx->extra[BL_UREC], bsz * p.RSU * 4))) return rc;
    if (p.dense && !p.epoch_route && (rc = ensure_dense_buffers(ctx, p, s))) return rc;
    return SLK_OK;
}

// One tiny prep on the prep stream, ordered against the caller's stream by the pipeline's own events: whatever the
// runtime sets up the first time these kernels (sampler, sorts) run on a stream and the first time two
// streams wait for each other's events then happens here and not inside the first overlapped training call
// (measured: that call ran 0.81-0.87 instead of 0.75-0.77 ms per step; a prior overlapped call of two minibatches
// removes it, profiles/r03_p_*).  The RNG state is put back afterwards.
static int warm_prep_stream(slk_ctx *ctx, const train_plan &p, const train_call &c) {
    hipStream_t s = c.s, ps = ctx->prep_stream;
    slk_prep_bufs &pb = ctx->pb[1];
    int rc;
    if ((rc = slk_ensure(ctx, ctx->extra[BL_LIVE], sizeof(slk_rng_dev) + 64))) return rc;
    SLK_HIP(ctx, hipEventRecord(ctx->ev_start, s));
    SLK_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_start, 0));
    SLK_HIP(ctx, hipMemcpyAsync(ctx->extra[BL_LIVE].p, ctx->d_rng, sizeof(slk_rng_dev), hipMemcpyDeviceToDevice, ps));
    if ((rc = slk_sample_u32(ctx, c.tables->num_items, 4096, u32p(pb.neg32), nullptr, ps))) return rc;
    SLK_HIP(ctx, hipMemcpyAsync(ctx->d_rng, ctx->extra[BL_LIVE].p, sizeof(slk_rng_dev), hipMemcpyDeviceToDevice, ps));
    SLK_HIP(ctx, hipMemsetAsync(pb.ukey[0].p, 0, 4096 * 4, ps));
    if ((rc = slk_sort_pairs_u32_u64(ctx, u32p(pb.ukey[0]), u32p(pb.ukey[1]), (const uint64_t *)pb.uval[0].p, (uint64_t *)pb.uval[1].p,
                                     4096, 20, ps)))
        return rc;
    if (!p.late) {
        SLK_HIP(ctx, hipMemsetAsync(pb.ikey[0].p, 0, 4096 * 4, ps));
        if ((rc = slk_sort_pairs_u32_u32(ctx, u32p(pb.ikey[0]), u32p(pb.ikey[1]), u32p(pb.ipay[0]), u32p(pb.ipay[1]), 4096, 20, ps)))
            return rc;
    }
    SLK_HIP(ctx, hipEventRecord(ctx->ev_prep[1], ps));
    SLK_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_prep[1], 0));
    SLK_HIP(ctx, hipEventRecord(ctx->ev_done[1], s));
    SLK_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_done[1], 0));
    SLK_HIP(ctx, hipStreamSynchronize(ps));
    SLK_HIP(ctx, hipStreamSynchronize(s));
    ctx->last_stream = s;
    ctx->sampled_valid = false;
    ctx->prep_warmed = true;
    return SLK_OK;
}

// slk_bilinear_reserve: what a training call of this plan would otherwise allocate or set up on its way
static int reserve_extras(slk_ctx *ctx, const train_plan &p, const train_call &c) {
    int rc;
    if (p.side && (rc = slk_prep_stream_init(ctx))) return rc;
    // the pinned read-back buffers and events of the long-run flags, per buffer set: hipHostMalloc inside a training call
    // costs a device synchronisation (measured: the first overlapped call of a process 0.85 instead of 0.745 ms per step)
    for (int st = 0; st < p.nsets; ++st)
        if ((rc = slk_lflags_reserve(ctx, ctx->pb[st], 2 * (size_t)p.mb_per_chunk))) return rc;
    if (p.side && !ctx->prep_warmed && p.nn > 0 && p.nc_max >= 4096 && (rc = warm_prep_stream(ctx, p, c))) return rc;
    const uint32_t n_mb = (uint32_t)((p.nc_max + p.bsz - 1) / p.bsz);
    if (p.epoch_route && (rc = slk_epoch_reserve(ctx, c.tables, c.optim, n_mb, p.bsz, (int)c.loss, p.NP))) return rc;
    // sampler and sort scratch for the largest chunk (the whole call when its negatives are one draw), so that the training
    // call allocates nothing
    if (p.one_draw && (rc = slk_ensure(ctx, ctx->call_neg, (size_t)c.n * p.nn * 4))) return rc;
    if ((rc = slk_sample_reserve(ctx, c.tables->num_items, p.one_draw ? c.n * (int64_t)p.nn : (int64_t)p.nc_max * p.nn))) return rc;
    return slk_sort_reserve(ctx, p.nc_max * (size_t)p.occ_mult);
}

static void pick_kernels(slk_ctx *ctx, const train_plan &p, const slk_optim *optim, train_kernels *kernels) {
    train_kernels &k = *kernels;
    const int upd = slk_upd_for(optim->kind), umode = p.umode;
    const bool bloom = p.bloom;
    // sampled softmax over a plain item table: every occurrence of the item pass is live (a bloom item table keeps the
    // SLK_ITEM_SNAP forms of its bias and row passes)
    const bool all_live = p.multi && !p.adaptive;
    k = train_kernels{};
#define SLK_PICK(V_, G_)                                                                    \
    do {                                                                                    \
        k.upass = user_pass_fn<V_, G_>(upd, umode, bloom);                                  \
        if (umode == 0 && !bloom) k.upass_lat = user_pass_lat_fn<V_, G_>(upd);              \
        if (umode == 0 && !bloom) k.upass_lat_long = user_pass_lat_fn<V_, G_, true>(upd);   \
        if (!bloom) k.upass_long = user_pass_long_fn<V_, G_>(upd, umode);                   \
        if (!bloom) k.ustitch = user_stitch_fn<V_, G_>(upd);                                \
        k.ipass = slk_item_pass_fn<V_, G_, SLK_ITEM_SNAP>(upd);                             \
        if (all_live) k.ipass = slk_item_pass_fn<V_, G_, SLK_ITEM_SNAPALL>(upd);            \
        k.spass = k_score_pass<V_, G_>;                                                     \
        if (p.pingpong) {                                                                   \
            k.upass = user_pass_pp_fn<V_, G_, false, false>(upd);                           \
            k.upass_lat = user_pass_pp_fn<V_, G_, true, false>(upd);                        \
            k.upass_long = user_pass_pp_fn<V_, G_, false, true>(upd);                       \
            k.upass_lat_long = user_pass_pp_fn<V_, G_, true, true>(upd);                    \
            k.ustitch = user_stitch_pp_fn<V_, G_>(upd);                                     \
            k.ipass = item_pass_pp_fn<V_, G_>(upd);                                         \
            if (p.sgl_on) {                                                                 \
                k.upass_sgl = user_pass_sgl_fn<V_, G_>();                                   \
                k.ipass_sgl = item_pass_sgl_fn<V_, G_>();                                   \
            }                                                                               \
        }                                                                                   \
        if (bloom) {                                                                        \
            k.ipass_rows = slk_item_pass_fn<V_, G_, SLK_ITEM_SNAP, SLK_PART_ROWS>(upd);     \
            k.ipass_bias = slk_item_pass_fn<V_, G_, SLK_ITEM_SNAP, SLK_PART_BIAS>(upd);     \
            k.rpass_rows = slk_item_pass_fn<V_, G_, SLK_ITEM_ROW, SLK_PART_ROWS>(upd);      \
        }                                                                                   \
    } while (0)
    SLK_FOR_LAYOUT(p.vec, p.g, SLK_PICK);
#undef SLK_PICK
    k.gpb = 256u / (unsigned)p.g;
    // The user pass is a grid-stride kernel: workgroups beyond what a CU holds RESIDENT start when others finish and unbalance
    // the pass.  Its grid is therefore capped at the kernel's own occupancy (slk_occupancy_of: the SparseAdam form needs 72
    // VGPRs = 7 workgroups per CU; launched 8 per CU it ran 0.58 ms, capped 0.44; Adagrad's 59 VGPRs hold 8).
    // (one cap for the forms a minibatch may take -- plain, latency-bound, long runs: the grid also counts the loss partials)
    k.occ_user = slk_occupancy_of(ctx, k.upass);
    for (pass_fn f : {k.upass_lat, k.upass_long, k.upass_lat_long}) {
        const int o = slk_occupancy_of(ctx, f);
        if (o < k.occ_user) k.occ_user = o;
    }
    // (the single-occurrence form holds more registers than the four whose smallest occupancy caps the others: a cap of its own)
    k.occ_sgl = p.sgl_on ? slk_occupancy_of(ctx, k.upass_sgl) : k.occ_user;
}

// ---- prep of one chunk into buffer set `pb` (value-independent: ids only), in two halves:
// the negatives (ALU/latency-bound MT19937 generator), then the sorts (HBM-bound)
static int prep_sample(slk_ctx *ctx, const train_plan &p, const train_call &c, const train_run &run, size_t ck, slk_prep_bufs &pb, hipStream_t s) {
    const int64_t c0 = chunk_begin(p, ck);
    const size_t nneg = (size_t)chunk_len(p, c, ck) * p.nn;
    if (run.neg_all) return SLK_OK;

    // ---- negatives (sampling.py:34, one randint per minibatch == one contiguous draw)
    if (p.nn == 0) return SLK_OK;  // explicit feedback draws none
    if (c.neg_in) return slk_prep_given_negatives(ctx, c.neg_in + c0 * p.nn, c.neg_out ? c.neg_out + c0 * p.nn : nullptr, nneg, pb, s);
    return slk_sample_u32(ctx, c.tables->num_items, (int64_t)nneg, u32p(pb.neg32), c.neg_out ? c.neg_out + c0 * p.nn : nullptr, s);
}

// The single-occurrence flags of a chunk's item-sorted list: which occurrences are NOT the only one of their item in their
// minibatch (ids only).  Behind the item sort of the chunk, on the same stream or one that waits for it.
static int prep_single_flags(slk_ctx *ctx, const train_plan &p, const train_call &c, slk_prep_bufs &pb, size_t ck, hipStream_t s) {
    const uint32_t nocc = chunk_len(p, c, ck) * (uint32_t)p.NP;
    SLK_HIP(ctx, hipMemsetAsync(pb.mflag.p, 0, (size_t)nocc, s));
    hipLaunchKernelGGL(k_item_multi_flags, dim3(slk_grid_for(ctx, nocc, 256)), dim3(256), 0, s, (const uint32_t *)pb.ikey[1].p,
                       (const uint32_t *)pb.ipay[1].p, nocc, (uint32_t)p.bsz * (uint32_t)p.NP, (uint8_t *)pb.msorted.p, (uint8_t *)pb.mflag.p);
    SLK_LAUNCH_CHECK(ctx, "k_item_multi_flags");
    return SLK_OK;
}

static int prep_sort(slk_ctx *ctx, const train_plan &p, const train_call &c, const train_run &run, size_t ck, slk_prep_bufs &pb, hipStream_t s) {
    int rc;
    const int64_t c0 = chunk_begin(p, ck);
    const uint32_t nc = chunk_len(p, c, ck), nocc = nc * (uint32_t)p.NP, bsz = (uint32_t)p.bsz;
    const int64_t *cu = c.users + c0, *ci = c.items + c0;
    const uint32_t *neg32 = run.neg_all ? run.neg_all + (size_t)c0 * p.nn : u32p(pb.neg32);
    const int Hi = p.Hi, Hu = p.Hu;

    // ---- prep: sort interactions by (minibatch, user), occurrences by (minibatch, item)
    slk_prof_begin(ctx, SLK_K_PREP, s);
    const unsigned mbbits = slk_bits_for((uint64_t)((nc - 1) / bsz));
    uint32_t *const ukey = u32p(pb.ukey[1]);
    const uint32_t *uit, *uk = nullptr;
    uint32_t *const ukeys[2] = {u32p(pb.ukey[0]), ukey};
    if (!p.pre) {
        // (keys and the fat (positive, negative) payload are formed by the sort's first pass from the id arrays)
        uint64_t *const uvals[2] = {(uint64_t *)pb.uval[0].p, (uint64_t *)pb.uval[1].p};
        if ((rc = slk_sort_user_fat(ctx, cu, ci, neg32, nc, (size_t)bsz, p.ubits, mbbits, (size_t)c.tables->num_users, ukeys, uvals,
                                    s)))
            return rc;
        uit = u32p(pb.uval[1]);  // little-endian (pos, neg) pairs
    } else {
        uint32_t *const uvals[2] = {u32p(pb.uval[0]), u32p(pb.uval[1])};
        if ((rc = slk_sort_user_idx(ctx, cu, nc, (size_t)bsz, p.ubits, mbbits, (size_t)c.tables->num_users, ukeys, uvals, s))) return rc;
        uk = u32p(pb.uval[1]);
        hipLaunchKernelGGL(k_pack_items, dim3(slk_grid_for(ctx, nc, 256)), dim3(256), 0, s, uk, ci, neg32, nc, p.nn, u32p(pb.uit));
        SLK_LAUNCH_CHECK(ctx, "k_pack_items");
        uit = u32p(pb.uit);
    }
    if (p.late) {
        hipLaunchKernelGGL(k_invert_perm, dim3(slk_grid_for(ctx, nc, 256)), dim3(256), 0, s, uk, nc, u32p(pb.ipay[0]));
        SLK_LAUNCH_CHECK(ctx, "k_invert_perm");
    } else {
        uint32_t *const ikeys[2] = {u32p(pb.ikey[0]), u32p(pb.ikey[1])};
        uint32_t *const ivals[2] = {u32p(pb.ipay[0]), u32p(pb.ipay[1])};
        if ((rc = slk_sort_item_occ(ctx, uit, nocc, (size_t)bsz, p.NP, p.ibits, mbbits, (size_t)c.tables->num_items, ikeys, ivals, s)))
            return rc;
        if (p.sgl_on && (rc = prep_single_flags(ctx, p, c, pb, ck, s))) return rc;
    }
    // which minibatches hold a LONG run (an item run that wholly covers a tile of the item pass, [0, n_mb); a user run that
    // wholly covers a tile of the user pass, [n_mb, 2 n_mb)): ids only, so the answer is fetched once per chunk and the usual
    // minibatch (none) gets the plain passes with no stitch kernel behind them
    if (!run.epoch_route) {  // (the persistent route walks the runs itself; its fall-back takes the long forms, run_passes)
        const uint32_t n_mb_c = (nc + bsz - 1) / bsz;
        const unsigned gpb = 256u / (unsigned)p.g;
        if ((rc = slk_ensure(ctx, pb.lflags, 2 * (size_t)n_mb_c * 4))) return rc;
        SLK_HIP(ctx, hipMemsetAsync(pb.lflags.p, 0, 2 * (size_t)n_mb_c * 4, s));
        if (!p.late) {
            hipLaunchKernelGGL(k_item_long_flags, dim3(slk_grid_for(ctx, nocc / (4 * gpb) + n_mb_c, 256)), dim3(256), 0, s,
                               (const uint32_t *)pb.ikey[1].p, nocc, bsz * (uint32_t)p.NP, 4u * gpb,
                               (uint32_t)((1ull << p.ibits) - 1), 0xffffffffu, 0xffffffffu, (int *)pb.lflags.p);
            SLK_LAUNCH_CHECK(ctx, "k_item_long_flags");
        }
        if (!p.bloom) {
            hipLaunchKernelGGL(k_user_long_flags, dim3(slk_grid_for(ctx, nc / SLK_USER_TILE + n_mb_c, 256)), dim3(256), 0, s,
                               (const uint32_t *)ukey, nc, bsz, (int *)pb.lflags.p + n_mb_c);
            SLK_LAUNCH_CHECK(ctx, "k_user_long_flags");
        }
        if ((rc = slk_lflags_readback(ctx, pb, 2 * (size_t)n_mb_c, s))) return rc;
    } else {
        pb.h_lflags_n = 0;  // no flags for this chunk: every pass of a fall-back takes the partial-writing form
    }
    if (Hi && !p.late) {
        hipLaunchKernelGGL(k_build_item_bloom_keys, dim3(slk_grid_for(ctx, (size_t)nocc * Hi, 256)), dim3(256), 0, s,
                           uit, nocc, p.NP, bsz, p.icbits, p.ibd, u32p(pb.bik[0]), u32p(pb.bip[0]));
        SLK_LAUNCH_CHECK(ctx, "k_build_item_bloom_keys");
        if ((rc = slk_sort_pairs_u32_u32(ctx, u32p(pb.bik[0]), u32p(pb.bik[1]), u32p(pb.bip[0]), u32p(pb.bip[1]), (size_t)nocc * Hi,
                                         p.icbits + mbbits, s, true)))
            return rc;
    }
    if (Hu) {
        hipLaunchKernelGGL(k_build_user_bloom_keys, dim3(slk_grid_for(ctx, (size_t)nc * Hu, 256)), dim3(256), 0, s,
                           (const uint32_t *)ukey, (uint32_t)((1ull << p.ubits) - 1), nc, bsz, p.ucbits, p.ubd,
                           u32p(pb.buk[0]), u32p(pb.bup[0]));
        SLK_LAUNCH_CHECK(ctx, "k_build_user_bloom_keys");
        if ((rc = slk_sort_pairs_u32_u32(ctx, u32p(pb.buk[0]), u32p(pb.buk[1]), u32p(pb.bup[0]), u32p(pb.bup[1]), (size_t)nc * Hu,
                                         p.ucbits + mbbits, s, true)))
            return rc;
    }
    slk_prof_end(ctx, s);
    return SLK_OK;
}

// ---- the minibatches of one prepared chunk, in order, on the caller's stream
struct minibatch {
    uint32_t b0, b1, bm;  // chunk-local interactions [b0, b1)
    slk_pass_args a;
    int ugm;              // workgroups per CU of the user pass's grid ...
    unsigned ugrid;       // ... and that grid, capped at the smallest occupancy of the four forms
    bool item_may_long, user_may_long;  // the chunk's long-run flags (prep_sort) do not rule a long run out
    bool sgl;             // the user pass also updates the items that occur once in the minibatch (the item pass skips them)
};

// What every pass of chunk `ck` is handed, whichever its minibatch.
static void chunk_pass_args(slk_ctx *ctx, const train_plan &p, const train_call &c, size_t ck, const slk_prep_bufs &pb, slk_pass_args *args) {
    slk_pass_args &a = *args;
    const slk_tables *tables = c.tables;
    const slk_optim *optim = c.optim;
    memset(&a, 0, sizeof(a));
    slk_fill_table_args(a, ctx, tables, optim, p.dense);
    if (p.shadowed) {
        a.P[3] = f32p(ctx->bias_shadow);
        a.S1[3] = f32p(ctx->bias_shadow) + 1;
        a.bsh3 = 1u;
    }
    if (p.pingpong) {
        a.P0alt = f32p(ctx->pp_alt);
        a.uflag = (uint8_t *)ctx->pp_flags.p;
    }
    a.D = p.D;
    a.NP = p.NP;
    a.ukey = u32p(pb.ukey[1]);
    a.umask = (uint32_t)((1ull << p.ubits) - 1);
    a.uit = p.pre ? u32p(pb.uit) : u32p(pb.uval[1]);
    a.uk = p.pre ? u32p(pb.uval[1]) : nullptr;
    a.gk = f32p(ctx->gk);
    a.sk = f32p(ctx->sk);
    a.snap = f32p(ctx->snap);
    a.RS = p.RS;
    a.gsn = f32p(ctx->extra[BL_GSN]);
    a.ikey = u32p(pb.ikey[1]);
    a.imask = (uint32_t)((1ull << p.ibits) - 1);
    a.ipay = u32p(pb.ipay[1]);
    a.loss_partial = (double *)ctx->losspart.p;
    a.loss_kind = c.loss;
    a.pad_item = a.pad_item2 = 0xffffffffu;
    a.ub = p.ubd;
    a.ib = p.ibd;
    a.urec = f32p(ctx->extra[BL_UREC]);
    a.RSU = p.RSU;
    // user biases the caller vouches are all zero, a loss whose user-bias gradient is exactly zero, an update for which a
    // zero gradient is an exact no-op: nothing of the table is read or written by the pair-mode user pass
    a.ubz = (tables->flags & SLK_TABLES_USER_BIAS_ZERO) && (c.loss == SLK_LOSS_BPR || c.loss == SLK_LOSS_HINGE) && !p.bloom &&
            slk_opt_zero_is_noop(optim->kind) && ctx->opt_user_bias_zero_hint;
    a.ubg0 = c.loss == SLK_LOSS_SOFTMAX;
    a.nt = ctx->opt_nt;
    if (p.fused) a.ratings = c.ratings + chunk_begin(p, ck);  // the user pass forms score, loss and dL/dscore itself (one pair per interaction)
}

// this minibatch's live occurrences (k_adaptive_select), as item ids or as their hashed rows, sorted: BL_LK1 / BL_LV1
static int sort_live_list(slk_ctx *ctx, const train_plan &p, const minibatch &mb, bool hashed, hipStream_t s) {
    const uint32_t n = 2 * mb.bm * (hashed ? (uint32_t)p.Hi : 1u);
    hipLaunchKernelGGL(k_build_live_keys, dim3(slk_grid_for(ctx, n, 256)), dim3(256), 0, s, (const uint32_t *)ctx->extra[BL_LIVE].p,
                       mb.a.uit, 2 * mb.bm, p.ibd, hashed, u32p(ctx->extra[BL_LK0]), u32p(ctx->extra[BL_LV0]));
    SLK_LAUNCH_CHECK(ctx, hashed ? "k_build_live_keys<hashed>" : "k_build_live_keys");
    return slk_sort_pairs_u32_u32_in(ctx, ctx->extra[BL_LATE_SORT], u32p(ctx->extra[BL_LK0]), u32p(ctx->extra[BL_LK1]),
                                     u32p(ctx->extra[BL_LV0]), u32p(ctx->extra[BL_LV1]), n, (hashed ? p.icbits : p.ibits) + 1, s,
                                     true);  // + the dead entries' bit
}

// dL/dscore where the user pass does not form it itself: explicit feedback (staged), adaptive hinge and its late live list
static int score_stage(slk_ctx *ctx, const train_plan &p, const train_call &c, const train_kernels &k, size_t ck, const slk_prep_bufs &pb, minibatch &mb, hipStream_t s) {
    slk_pass_args &a = mb.a;
    int rc;
    a.n_loss_partial = (int)mb.ugrid;
    if (!p.pre || p.fused) return SLK_OK;
    slk_prof_begin(ctx, SLK_K_SCORE, s);
    hipLaunchKernelGGL(k.spass, dim3(mb.ugrid), dim3(256), 0, s, a);
    SLK_LAUNCH_CHECK(ctx, "k_score_pass");
    unsigned sgrid = slk_grid_for(ctx, mb.bm, 256);
    // interaction weights: chunk-local as the ratings are; this minibatch's W in the chunk's sums (weight_sums)
    const float *const wts = p.weighted ? c.weights + chunk_begin(p, ck) : nullptr;
    const double *const wsum = p.weighted ? (const double *)ctx->extra[BL_WSUM].p + mb.b0 / (uint32_t)p.bsz : nullptr;
    if (p.weighted && p.expl) {
        hipLaunchKernelGGL(k_explicit_loss_weighted, dim3(sgrid), dim3(256), 0, s, (const float *)ctx->sk.p,
                           c.ratings + chunk_begin(p, ck), wts, f32p(ctx->gk), mb.b0, mb.bm, (int)c.loss, wsum,
                           (double *)ctx->losspart.p);
        SLK_LAUNCH_CHECK(ctx, "k_explicit_loss_weighted");
    } else if (p.weighted && !p.multi) {
        hipLaunchKernelGGL(k_pair_loss_weighted, dim3(sgrid), dim3(256), 0, s, (const float *)ctx->sk.p, wts, f32p(ctx->gk), mb.b0,
                           mb.bm, (int)c.loss, wsum, (double *)ctx->losspart.p);
        SLK_LAUNCH_CHECK(ctx, "k_pair_loss_weighted");
    } else if (p.expl) {
        hipLaunchKernelGGL(k_explicit_loss, dim3(sgrid), dim3(256), 0, s, (const float *)ctx->sk.p, c.ratings + chunk_begin(p, ck),
                           f32p(ctx->gk), mb.b0, mb.bm, (int)c.loss, a.inv_b, (double *)ctx->losspart.p);
        SLK_LAUNCH_CHECK(ctx, "k_explicit_loss");
    } else if (!p.adaptive) {  // sampled softmax: a lane group per interaction
        const int sg = slk_softmax_group(p.NP);
        sgrid = slk_grid_for(ctx, mb.bm, 256u / (unsigned)sg);
        hipLaunchKernelGGL(softmax_loss_fn(sg), dim3(sgrid), dim3(256), 0, s, (const float *)ctx->sk.p, f32p(ctx->gk), mb.b0, mb.bm,
                           p.nn, a.inv_b, (double *)ctx->losspart.p, wts, wsum);
        SLK_LAUNCH_CHECK(ctx, "k_softmax_loss");
    } else {
        hipLaunchKernelGGL(k_adaptive_select<0>, dim3(sgrid), dim3(256), 0, s, (const float *)ctx->sk.p, f32p(ctx->gk), mb.b0, mb.bm,
                           p.nn, a.inv_b, (double *)ctx->losspart.p, p.late ? (const uint32_t *)pb.ipay[0].p : (const uint32_t *)nullptr,
                           p.late ? u32p(ctx->extra[BL_LIVE]) : (uint32_t *)nullptr, wts, wsum, (int)c.loss,
                           (uint32_t)c.tables->num_items);
        SLK_LAUNCH_CHECK(ctx, "k_adaptive_select");
    }
    a.n_loss_partial = (int)sgrid;
    slk_prof_end(ctx, s);
    if (p.late) {
        // this minibatch's live occurrences, sorted by item (biases; rows of a plain table)
        slk_prof_begin(ctx, SLK_K_PREP, s);
        if ((rc = sort_live_list(ctx, p, mb, false, s))) return rc;
        slk_prof_end(ctx, s);
        a.ikey = u32p(ctx->extra[BL_LK1]);
        a.ipay = u32p(ctx->extra[BL_LV1]);
        a.imask = 0xffffffffu;
        a.ibegin = 0;
        a.iend = 2 * mb.bm;
        // a.pad_item2 == ~0u: the dead entries' all-ones key is never updated
    }
    return SLK_OK;
}

// The user pass in the form this minibatch takes
static int user_stage(slk_ctx *ctx, const train_plan &p, const train_kernels &k, const slk_prep_bufs &pb, minibatch &mb, hipStream_t s) {
    slk_pass_args &a = mb.a;
    slk_prof_begin(ctx, SLK_K_USER_PASS, s);
    const bool lat = k.upass_lat && (int64_t)mb.bm <= ctx->opt_user_lat_max_batch;
    // the single-occurrence fast path rides on the plain (bandwidth-bound) form only: a minibatch that takes the latency-bound
    // or the long-run form leaves every item to the item pass
    const bool sgl = mb.sgl = p.sgl_on && k.upass_sgl && !mb.user_may_long && !lat;
    if (sgl) {
        a.mflag = (const uint8_t *)pb.mflag.p;
        a.msorted = (const uint8_t *)pb.msorted.p;
        ++ctx->stat_single;
    }
    const pass_fn uform = sgl ? k.upass_sgl : (mb.user_may_long ? (lat ? k.upass_lat_long : k.upass_long) : (lat ? k.upass_lat : k.upass));
    unsigned ugrid_form = mb.ugrid;
    // Option "user_grid_own_occ" (off): the grid of the form that is launched capped at THAT form's occupancy instead of the
    // smallest of the four forms' -- measured in round 6 and not kept (slk_common.h); the single-occurrence form always is
    if (ctx->opt_user_grid_own_occ || sgl) {
        const int occ_form = sgl ? k.occ_sgl : slk_occupancy_of(ctx, uform);
        ugrid_form = slk_grid_for(ctx, mb.bm, k.gpb, mb.ugm < occ_form ? mb.ugm : occ_form);
        if (!p.pre || p.fused) a.n_loss_partial = (int)ugrid_form;  // (the pass writes one loss partial per workgroup)
    }
    if (mb.user_may_long) {
        if (ctx->upart_gen >= 0x0ffffffeu) {  // the 28-bit stamp wraps: forget every old partial
            SLK_HIP(ctx, hipMemsetAsync(ctx->upart_meta.p, 0, ctx->upart_meta.cap, s));
            ctx->upart_gen = 0u;
        }
        ++ctx->upart_gen;
        a.upart = f32p(ctx->extra[BL_UPART]);
        a.upart_meta = u32p(ctx->upart_meta);
        a.upart_count = a.upart_meta + 4 * p.utiles;
        a.upart_gen = ctx->upart_gen;
        a.UPS = p.UPS;
        SLK_HIP(ctx, hipMemsetAsync(a.upart_count, 0, 4, s));
        hipLaunchKernelGGL(uform, dim3(ugrid_form), dim3(256), 0, s, a);
        SLK_LAUNCH_CHECK(ctx, "k_user_pass<ULONG>");
        ++ctx->stat_user_long;
        hipLaunchKernelGGL(k.ustitch, dim3(slk_grid_for(ctx, ((size_t)mb.bm + SLK_USER_TILE - 1) / SLK_USER_TILE, k.gpb)), dim3(256), 0, s, a);
        SLK_LAUNCH_CHECK(ctx, "k_user_stitch");
    } else {
        hipLaunchKernelGGL(uform, dim3(ugrid_form), dim3(256), 0, s, a);
        SLK_LAUNCH_CHECK(ctx, "k_user_pass");
    }
    slk_prof_end(ctx, s);
    return SLK_OK;
}

// The row-owner passes over the item side: plain tables in one pass; a compressed item table as a bias pass over the plain
// occurrence list and a row pass over the hashed one; a compressed user table's rows behind them
static int item_stage(slk_ctx *ctx, const train_plan &p, const train_call &c, const train_kernels &k, const slk_prep_bufs &pb, minibatch &mb, hipStream_t s) {
    slk_pass_args &a = mb.a;
    const int Hi = p.Hi, Hu = p.Hu, g = p.g;
    int rc;
    slk_prof_begin(ctx, SLK_K_ITEM_PASS, s);
    if (!Hi) {
        if ((rc = slk_launch_item_pass(ctx, mb.sgl ? k.ipass_sgl : k.ipass, a, g, s, "k_item_pass", mb.item_may_long))) return rc;
    } else {
        // item biases are indexed by the item id: plain occurrence list, bias only ...
        if ((rc = slk_launch_item_pass(ctx, k.ipass_bias, a, g, s, "k_item_pass<BIAS>", mb.item_may_long))) return rc;
        // ... while every occurrence feeds the n_hash hashed rows of the compressed table
        slk_pass_args r = a;
        r.mb_loss_out = nullptr;
        r.ikey = u32p(pb.bik[1]);
        r.ipay = u32p(pb.bip[1]);
        r.ibegin = a.ibegin * (uint32_t)Hi;
        r.iend = a.iend * (uint32_t)Hi;
        r.imask = (uint32_t)((1ull << p.icbits) - 1);
        if (p.late) {
            // the live occurrences' hashed rows (the bias pass above has consumed LK1/LV1:
            // same stream, so the buffers can be reused)
            if ((rc = sort_live_list(ctx, p, mb, true, s))) return rc;
            r.ikey = u32p(ctx->extra[BL_LK1]);
            r.ipay = u32p(ctx->extra[BL_LV1]);
            r.ibegin = 0;
            r.iend = 2 * mb.bm * (uint32_t)Hi;
            r.imask = 0xffffffffu;
        }
        r.pad_item = c.tables->item_bloom->skip_row < 0 ? 0xffffffffu : (uint32_t)c.tables->item_bloom->skip_row;
        if ((rc = slk_launch_item_pass(ctx, k.ipass_rows, r, g, s, "k_item_pass<ROWS>"))) return rc;
    }
    if (Hu) {
        // owner pass over the hashed USER rows: table slot 1 of the pass is remapped onto
        // the user embedding table, records are the segment gradients parked by the user pass
        slk_pass_args r = a;
        r.mb_loss_out = nullptr;
        r.P[1] = a.P[0];
        r.S1[1] = a.S1[0];
        r.S2[1] = a.S2[0];
        r.snap = a.urec;
        r.RS = p.RSU;
        r.ikey = u32p(pb.buk[1]);
        r.ipay = u32p(pb.bup[1]);
        r.ibegin = mb.b0 * (uint32_t)Hu;
        r.iend = mb.b1 * (uint32_t)Hu;
        r.imask = (uint32_t)((1ull << p.ucbits) - 1);
        r.pad_item = c.tables->user_bloom->skip_row < 0 ? 0xffffffffu : (uint32_t)c.tables->user_bloom->skip_row;
        r.pad_item2 = p.ubd.rows;  // sentinel of non-head positions
        if ((rc = slk_launch_item_pass(ctx, k.rpass_rows, r, g, s, "k_item_pass<ROW,ROWS>"))) return rc;
    }
    slk_prof_end(ctx, s);
    return SLK_OK;
}

// W_m of every minibatch of chunk `ck` (BL_WSUM), once per chunk, on the passes' stream ahead of the chunk's first score stage
static int weight_sums(slk_ctx *ctx, const train_plan &p, const train_call &c, size_t ck, hipStream_t s) {
    const uint32_t nc = chunk_len(p, c, ck), bsz = (uint32_t)p.bsz, n_mb = (nc + bsz - 1) / bsz, segs = weight_segs(p);
    double *const wpart = (double *)ctx->extra[BL_WPART].p, *const wsum = (double *)ctx->extra[BL_WSUM].p;
    slk_prof_begin(ctx, SLK_K_SCORE, s);
    hipLaunchKernelGGL(k_weight_partials, dim3(slk_grid_for(ctx, (size_t)n_mb * segs * 256, 256)), dim3(256), 0, s,
                       c.weights + chunk_begin(p, ck), nc, bsz, segs, wpart);
    SLK_LAUNCH_CHECK(ctx, "k_weight_partials");
    hipLaunchKernelGGL(k_weight_sums, dim3(slk_grid_for(ctx, (size_t)n_mb * 256, 256)), dim3(256), 0, s, (const double *)wpart, n_mb,
                       segs, wsum);
    SLK_LAUNCH_CHECK(ctx, "k_weight_sums");
    slk_prof_end(ctx, s);
    return SLK_OK;
}

static int run_passes(slk_ctx *ctx, const train_plan &p, const train_call &c, const train_kernels &k, train_run &run, size_t ck, slk_prep_bufs &pb, hipStream_t s) {
    int rc;
    const uint32_t nc = chunk_len(p, c, ck), bsz = (uint32_t)p.bsz;
    const uint32_t n_mb_c = (nc + bsz - 1) / bsz;
    slk_pass_args chunk_args;
    chunk_pass_args(ctx, p, c, ck, pb, &chunk_args);
    // overlapped prep: the user pass is a grid-stride kernel whose workgroups hold their wave slots for the whole run; two
    // of the eight per CU are left to the prep stream's kernels (measured, profiles/r03_a_*: 8 -> 6 costs the pass
    // nothing by itself and gives the overlap 2 % more)
    const int ugm = p.side && ctx->opt_user_grid_mult > 6 ? 6 : ctx->opt_user_grid_mult;
    minibatch mb;
    mb.ugm = ugm;
    if (p.weighted && (rc = weight_sums(ctx, p, c, ck, s))) return rc;
    for (uint32_t b0 = 0; b0 < nc; b0 += bsz, ++run.mb_global) {
        const uint32_t b1 = (nc - b0 < bsz) ? nc : b0 + bsz, bm = b1 - b0;
        mb.b0 = b0, mb.b1 = b1, mb.bm = bm;
        slk_pass_args &a = mb.a = chunk_args;
        a.begin = b0;
        a.end = b1;
        a.ibegin = b0 * (uint32_t)p.NP;
        a.iend = b1 * (uint32_t)p.NP;
        // (weighted: the loss kernels of score_stage divide by the minibatch's weight sum themselves -- dL/dscore and the loss
        // partials alike -- and nothing else of a staged call reads inv_b but the finalisation of d_mb_loss in the item pass)
        a.inv_b = p.weighted ? 1.0f : 1.0f / (float)bm;
        a.mb_loss_out = c.mb_loss + run.mb_global;
        slk_set_opt_coeffs(a, c.optim);
        // Round 6 (profiles/r06_mall_ab.jsonl): a minibatch whose records are as large as the Infinity Cache (2^20 x 256 B
        // = 256 MB) cannot keep them there until the item pass reads them -- written with plain stores they only evict the
        // item table, which the user pass re-reads twice per interaction.  Non-temporal record stores: C2 step -0.9 %
        // (item pass 0.3165 -> 0.3122 ms), C5 shard -0.2 %; a minibatch of 65 536 (16 MB of records: they DO stay) +4 %, so
        // only above "record_nt_min_bytes".
        if (ctx->opt_record_nt_min_bytes > 0 && (int64_t)bm * p.RS * 4 >= ctx->opt_record_nt_min_bytes) a.nt |= 16;
        mb.ugrid = slk_grid_for(ctx, bm, k.gpb, ugm < k.occ_user ? ugm : k.occ_user);
        if ((rc = score_stage(ctx, p, c, k, ck, pb, mb, s))) return rc;

        // the chunk's long-run flags (prep_sort): ONE host wait per chunk, before the first user pass.  The flags are produced by
        // the chunk's sorts, long before the previous chunk's passes are through: the GPU has work queued while the host waits
        // for the read-back
        if (b0 == 0 && pb.ev_lflags && pb.h_lflags_n) SLK_HIP(ctx, hipEventSynchronize(pb.ev_lflags));
        const uint32_t mb_c = b0 / bsz;
        const bool have_flags = pb.h_lflags_n >= 2 * (size_t)n_mb_c;
        mb.item_may_long = p.late || !ctx->opt_item_long_gate || !have_flags || pb.h_lflags[mb_c] != 0;
        mb.user_may_long = !p.bloom && (!ctx->opt_item_long_gate || !have_flags || pb.h_lflags[n_mb_c + mb_c] != 0);

        if ((rc = user_stage(ctx, p, k, pb, mb, s))) return rc;
        if ((rc = item_stage(ctx, p, c, k, pb, mb, s))) return rc;
        if (p.dense && (rc = slk_dense_sweeps(ctx, c.tables->d_param, c.optim, 15u, s))) return rc;
        c.optim->step += 1;
    }
    return SLK_OK;
}

static int run_chunk(slk_ctx *ctx, const train_plan &p, const train_call &c, const train_kernels &k, train_run &run, size_t ck, slk_prep_bufs &pb, hipStream_t s) {
    if (!run.epoch_route) return run_passes(ctx, p, c, k, run, ck, pb, s);
    const int64_t c0 = chunk_begin(p, ck);
    const uint32_t nc = chunk_len(p, c, ck);
    int rc = slk_epoch_run_chunk(ctx, c.tables, c.optim, pb, nc, p.bsz, p.ubits, p.ibits, (int)c.loss, p.NP, p.RS, f32p(ctx->snap),
                                 f32p(ctx->extra[BL_GSN]), c.mb_loss + run.mb_global, p.expl ? c.ratings + c0 : nullptr, s);
    if (rc == SLK_EAGAIN_EPOCH) {  // cooperative launch refused: nothing ran; per-minibatch launches from here on
        run.epoch_route = false;
        if (p.dense && (rc = ensure_dense_buffers(ctx, p, s))) return rc;
        return run_passes(ctx, p, c, k, run, ck, pb, s);
    }
    run.mb_global += (nc + p.bsz - 1) / p.bsz;
    return rc;
}

// slk_bilinear_prefetch: the first chunk of the call these arguments describe, on the prep stream, and the record of it (ctx->pf)
static int prefetch_first_chunk(slk_ctx *ctx, const train_plan &p, const train_call &c, train_run &run) {
    int rc;
    hipStream_t s = c.s;
    ctx->pf.valid = false;
    if (!p.side || run.epoch_route || c.neg_in) return SLK_OK;  // such a call prepares in line: nothing to run ahead
    if ((rc = slk_prep_stream_init(ctx))) return rc;
    hipStream_t ps = ctx->prep_stream;
    // the set the call before did NOT finish on: its last reader were the passes two chunks back (ev_done of that set)
    const int set = ctx->last_pipe_set >= 0 ? (ctx->last_pipe_set ^ 1) : 0;
    // What the prepared chunk waits for (it used to wait for everything the caller's stream held -- every pass of
    // the epoch before -- and so ran BEHIND those passes, not beside them): the id arrays are complete when this call is made
    // (the header says so; fit() has read the shuffle's RNG state back, which synchronises the lane that wrote them); buffer
    // set `set` was last read by the passes two chunks back (ev_done); the sampler's and the sorts' scratch and, with
    // "overlap_prep" 1, the earlier readers of pf_neg (the sorts of the running call's later chunks) live on the prep stream
    // itself.  Only with "overlap_prep" 2 do sorts that read pf_neg run on the caller's stream: then, and only then, the
    // new draw waits for that stream's tail.
    //  That holds for a ctx whose last training call was a pipelined one.  After an IN-LINE call (one buffer
    // set, "overlap_prep" 0 / 2: sampler, sorts and buffer set 0 were used on the caller's stream -- ctx->last_pipe_set < 0)
    // the new draw waits for that stream's tail; after an in-line slk_sample_items it waits for that draw's own event.
    if (ctx->opt_overlap_prep != 1 || ctx->opt_prefetch_wait || ctx->last_pipe_set < 0) {
        SLK_HIP(ctx, hipEventRecord(ctx->ev_start, s));
        SLK_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_start, 0));
    } else if (ctx->sampled_valid && ctx->ev_sampled) {
        SLK_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_sampled, 0));  // (recorded on the prep stream itself in the steady state: free)
    }
    SLK_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_done[set], 0));
    // The negatives of the WHOLE call in one draw: the stream position behind them -- where the NEXT epoch's shuffle starts --
    // is then known an epoch ahead (slk_rng_get_state_sampled), and the training call itself draws nothing.
    if (p.one_draw) {
        if ((rc = slk_ensure(ctx, ctx->pf_neg, (size_t)c.n * p.nn * 4))) return rc;
        if ((rc = slk_sample_u32(ctx, c.tables->num_items, c.n * (int64_t)p.nn, u32p(ctx->pf_neg), nullptr, ps))) return rc;
        run.neg_all = u32p(ctx->pf_neg);
    } else if ((rc = prep_sample(ctx, p, c, run, 0, ctx->pb[set], ps))) {
        return rc;
    }
    if (ctx->opt_overlap_prep == 1 && (rc = prep_sort(ctx, p, c, run, 0, ctx->pb[set], ps))) return rc;
    SLK_HIP(ctx, hipEventRecord(ctx->ev_prep[set], ps));
    ctx->pf = {true, set, c.users, c.items, c.n, p.bsz, (int64_t)p.nc_max, (int)c.loss, p.nn, p.one_draw, p.sgl_on};
    return SLK_OK;
}

// one chunk: everything in order on the caller's stream
static int run_inline(slk_ctx *ctx, const train_plan &p, const train_call &c, const train_kernels &k, train_run &run) {
    int rc;
    if ((rc = prep_sample(ctx, p, c, run, 0, ctx->pb[0], c.s))) return rc;
    if ((rc = prep_sort(ctx, p, c, run, 0, ctx->pb[0], c.s))) return rc;
    if ((rc = run_chunk(ctx, p, c, k, run, 0, ctx->pb[0], c.s))) return rc;
    ctx->last_stream = c.s;
    ctx->last_pipe_set = -1;
    return SLK_OK;
}

// pipeline: prep(c + 1) is enqueued before passes(c) -- on ctx->prep_stream, beside them (`side`), or on the caller's own
// stream, ahead of them.  `have0`: chunk 0 was prepared ahead by slk_bilinear_prefetch (ctx->pf).
static int run_pipelined(slk_ctx *ctx, const train_plan &p, const train_call &c, const train_kernels &k, train_run &run, bool have0) {
    int rc;
    hipStream_t s = c.s;
    const bool side = p.side;
    // overlap_prep = 1: negatives and sorts; = 2: only the negatives (the generator is ALU-bound and
    // shares the chip with the HBM-bound passes; the sorts stay in line on the caller's stream)
    const bool sort_ahead = !side || ctx->opt_overlap_prep == 1;
    if (side && (rc = slk_prep_stream_init(ctx))) return rc;
    hipStream_t ps = side ? ctx->prep_stream : s;
    if (side) {
        SLK_HIP(ctx, hipEventRecord(ctx->ev_start, s));      // inputs produced on the caller's stream
        SLK_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_start, 0));
    }
    int set = have0 ? ctx->pf.set : 0;
    if (have0) ++ctx->stat_prefetched;
    if (have0 && ctx->pf.all) run.neg_all = u32p(ctx->pf_neg);
    // A chunk prepared ahead of slk_user_pingpong_begin was sorted without the single-occurrence flags this call reads: they
    // are made below, behind the chunk's sorts.  (The opposite mismatch needs nothing: the flags are simply not read.)
    const bool flags0 = have0 && sort_ahead && p.sgl_on && !ctx->pf.sgl_on;
    if (!have0) {
        if (p.one_draw) {  // what slk_bilinear_prefetch does for fit()'s epochs
            if ((rc = slk_ensure(ctx, ctx->call_neg, (size_t)c.n * p.nn * 4))) return rc;
            if ((rc = slk_sample_u32(ctx, c.tables->num_items, c.n * (int64_t)p.nn, u32p(ctx->call_neg), c.neg_out, ps))) return rc;
            run.neg_all = u32p(ctx->call_neg);
        } else if ((rc = prep_sample(ctx, p, c, run, 0, ctx->pb[set], ps))) {
            return rc;
        }
        if (sort_ahead && (rc = prep_sort(ctx, p, c, run, 0, ctx->pb[set], ps))) return rc;
        if (side) SLK_HIP(ctx, hipEventRecord(ctx->ev_prep[set], ps));
    }
    for (size_t ck = 0; ck < p.n_chunks; ++ck, set ^= 1) {
        if (side) SLK_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_prep[set], 0));
        if (ck == 0 && flags0) {
            slk_prof_begin(ctx, SLK_K_PREP, s);
            if ((rc = prep_single_flags(ctx, p, c, ctx->pb[set], 0, s))) return rc;
            slk_prof_end(ctx, s);
        }
        if (ck == 0 && have0 && run.neg_all && c.neg_out) {  // the caller wants the draws: they were made ahead, as uint32
            const size_t nneg = (size_t)c.n * p.nn;
            hipLaunchKernelGGL(k_u32_to_i64, dim3(slk_grid_for(ctx, nneg, 256)), dim3(256), 0, s, run.neg_all, c.neg_out, nneg);
            SLK_LAUNCH_CHECK(ctx, "k_u32_to_i64");
        }
        if (!sort_ahead && (rc = prep_sort(ctx, p, c, run, ck, ctx->pb[set], s))) return rc;
        if (ck + 1 < p.n_chunks) {
            // the other buffer set was last read by the passes of the previous chunk (with a chunk prepared ahead: by the last
            // passes of the call before this one)
            if (side && (ck > 0 || have0)) SLK_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_done[set ^ 1], 0));
            if (!sort_ahead) {
                // "overlap_prep" 2: the next chunk's draw starts behind THIS chunk's sorts, i.e. beside its passes.  Started
                // together with the sorts (round 4) the generator's workgroups -- whole CUs by their LDS -- took the sorts'
                // CUs: the in-line sorts ran 17 % longer and the overlap gained nothing (profiles/r05_b_sweep_overlap_prep.jsonl)
                SLK_HIP(ctx, hipEventRecord(ctx->ev_start, s));
                SLK_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_start, 0));
            }
            if ((rc = prep_sample(ctx, p, c, run, ck + 1, ctx->pb[set ^ 1], ps))) return rc;
            if (sort_ahead && (rc = prep_sort(ctx, p, c, run, ck + 1, ctx->pb[set ^ 1], ps))) return rc;
            if (side) {
                SLK_HIP(ctx, hipEventRecord(ctx->ev_prep[set ^ 1], ps));
                ++ctx->stat_overlapped;
            }
        }
        if ((rc = run_chunk(ctx, p, c, k, run, ck, ctx->pb[set], s))) return rc;
        if (side) SLK_HIP(ctx, hipEventRecord(ctx->ev_done[set], s));
    }
    // not `side`: everything ran on the caller's stream -- in-line semantics for what follows (slk_bilinear_prefetch); else the
    // set of the last chunk (the loop's last increment undone)
    ctx->last_pipe_set = side ? (set ^ 1) : -1;
    ctx->last_stream = s;  // every prep is ordered before the tail of the caller's stream
    return SLK_OK;
}

static int run_training(slk_ctx *ctx, const train_call &c) {
    if (!ctx) return SLK_EINVAL;
    train_plan p;
    int rc;
    if ((rc = plan_training(ctx, c, &p))) return rc;
    if (p.n_chunks == 0) return SLK_OK;
    const bool training = c.mode == train_call::TRAIN;
    if (p.shadowed && training) ++ctx->stat_shadowed;
    if (p.pingpong && training) ++ctx->stat_pingpong;
    if ((rc = ensure_scratch(ctx, p, c.s))) return rc;
    if (c.mode == train_call::RESERVE) return reserve_extras(ctx, p, c);
    train_kernels k;
    pick_kernels(ctx, p, c.optim, &k);
    train_run run = {nullptr, 0, p.epoch_route};
    if (!training) return prefetch_first_chunk(ctx, p, c, run);

    // a chunk prepared ahead by slk_bilinear_prefetch: it must be THIS call's first chunk (its negatives are already drawn)
    // (a call that draws nothing -- negatives handed in, explicit feedback -- cannot be confused with the prepared one: it drops
    // the chunk instead of refusing; fit() of another model after one that left its loop by an exception)
    if (ctx->pf.valid && (c.neg_in || p.expl || p.weighted)) ctx->pf.valid = false;  // (a weighted call is never the prepared one)
    const bool have0 = ctx->pf.valid;
    ctx->pf.valid = false;
    if (have0 && (!p.side || p.epoch_route || ctx->pf.users != (const void *)c.users || ctx->pf.items != (const void *)c.items ||
                  ctx->pf.n != c.n || ctx->pf.bsz != p.bsz || ctx->pf.loss != (int)c.loss || ctx->pf.nn != p.nn ||
                  ctx->pf.nc0 != (int64_t)p.nc_max || c.neg_in))
        return slk_fail(ctx, SLK_EINVAL, "slk_bilinear_train: a chunk was prepared ahead (slk_bilinear_prefetch) for another call; its "
                                         "draws are consumed -- set the RNG state again");
    return p.nsets == 1 ? run_inline(ctx, p, c, k, run) : run_pipelined(ctx, p, c, k, run, have0);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Item-bias shadow (round 5).  On tables of 10^8 rows a minibatch's item biases share no cache line: the owner pass pays a
// 128-byte read and a 64-byte write for the 4-byte bias AND again for its 4-byte Adagrad accumulator -- a quarter of the C5
// shard's item-pass requests (profiles/r04_ea_c5_pmc.md).  For the duration of a training scope (a fit(): thousands of
// minibatches) the two arrays are held interleaved, {bias, sum} per item, so an occurrence touches ONE line; torch's own
// tensors are stale inside the scope and rewritten by slk_bias_shadow_end.  The reference has no counterpart (its biases are
// an nn.Embedding of dim 1: spotlight/factorization/representations.py:80-91).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bias_shadow_pack(const float *p, const float *s1, float2 *sh, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) sh[i] = make_float2(p[i], s1[i]);
}

__global__ __launch_bounds__(256) void k_bias_shadow_unpack(const float2 *sh, float *p, float *s1, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float2 v = sh[i];
        p[i] = v.x;
        s1[i] = v.y;
    }
}

SLK_EXPORT int slk_bias_shadow_begin(slk_ctx *ctx, const slk_tables *tables, const slk_optim *optim, void *stream) {
    if (!ctx || !tables || !optim) return SLK_EINVAL;
    SLK_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->shadow_active) return slk_fail(ctx, SLK_EINVAL, "slk_bias_shadow_begin: a shadow is already active on this ctx");
    if (optim->kind != SLK_OPT_ADAGRAD || !tables->d_param[3] || !optim->d_state1[3] || tables->item_bloom || tables->num_items < 1)
        return slk_fail(ctx, SLK_EINVAL, "slk_bias_shadow_begin: row-sparse Adagrad over a plain item table only");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = slk_ensure(ctx, ctx->bias_shadow, (size_t)tables->num_items * 8))) return rc;
    hipLaunchKernelGGL(k_bias_shadow_pack, dim3(slk_grid_for(ctx, (size_t)tables->num_items, 256)), dim3(256), 0, s,
                       (const float *)tables->d_param[3], (const float *)optim->d_state1[3], (float2 *)ctx->bias_shadow.p,
                       (size_t)tables->num_items);
    SLK_LAUNCH_CHECK(ctx, "k_bias_shadow_pack");
    ctx->shadow_src_p = tables->d_param[3];
    ctx->shadow_src_s = optim->d_state1[3];
    ctx->shadow_rows = tables->num_items;
    ctx->shadow_active = true;
    ctx->last_stream = s;
    return SLK_OK;
}

SLK_EXPORT int slk_bias_shadow_end(slk_ctx *ctx, void *stream) {
    if (!ctx) return SLK_EINVAL;
    if (!ctx->shadow_active) return SLK_OK;
    // Whatever happens below the scope is CLOSED when this call returns (an error return used to leave it open and
    // every later _begin / predict on that ctx refused); on an error the caller's arrays hold what they held at _begin.
    float *const dst_p = ctx->shadow_src_p, *const dst_s = ctx->shadow_src_s;
    const int64_t rows = ctx->shadow_rows;
    ctx->shadow_active = false;
    ctx->shadow_src_p = ctx->shadow_src_s = nullptr;
    SLK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bias_shadow_unpack, dim3(slk_grid_for(ctx, (size_t)rows, 256)), dim3(256), 0, s,
                       (const float2 *)ctx->bias_shadow.p, dst_p, dst_s, (size_t)rows);
    SLK_LAUNCH_CHECK(ctx, "k_bias_shadow_unpack");
    ctx->last_stream = s;
    return SLK_OK;
}

// Closes the scope WITHOUT writing back (ABI 11): for a caller whose bias / accumulator arrays no longer exist (the model was
// deleted inside the scope).  What the scope trained is lost; the arrays -- if they still exist -- keep their _begin values.
SLK_EXPORT int slk_bias_shadow_abort(slk_ctx *ctx) {
    if (!ctx) return SLK_EINVAL;
    ctx->shadow_active = false;
    ctx->shadow_src_p = ctx->shadow_src_s = nullptr;
    return SLK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// User-row ping-pong (round 6).  The two ownership passes of a minibatch each need the OTHER side's pre-step rows.  Rounds 1-6
// saved the user side: the user pass wrote every position's pre-step user row into a record (4D bytes per interaction: 13 % of
// the pass's real traffic at C2) and the item pass gathered it from there.  With 288 GB of HBM the user table can simply exist
// twice: a user's updated row is written to the copy that does NOT hold its current row, one byte per user says which copy is
// current, and the pre-step row stays where it was for the item pass to gather -- the same 4D-byte random read the record cost,
// and no record write.  The caller's table is the union of both copies until _end copies the rows whose current copy is the
// ctx's back.  Same arithmetic in the same order: tables bit-identical to training without it.  The reference has no
// counterpart (autograd keeps the pre-step rows alive as saved tensors: spotlight/factorization/representations.py:61-91).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pingpong_merge(float *P0, const float *alt, const uint8_t *flag, size_t rows, int D) {
    if (D % 4 == 0) {
        const size_t per = (size_t)D / 4, n = rows * per;
        for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256)
            if (flag[e / per]) reinterpret_cast<float4 *>(P0)[e] = reinterpret_cast<const float4 *>(alt)[e];
    } else {
        const size_t n = rows * (size_t)D;
        for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256)
            if (flag[e / (size_t)D]) P0[e] = alt[e];
    }
}

SLK_EXPORT int slk_user_pingpong_begin(slk_ctx *ctx, const slk_tables *tables, const slk_optim *optim, void *stream) {
    if (!ctx) return SLK_EINVAL;
    if (!tables || !optim) return slk_fail(ctx, SLK_EINVAL, "slk_user_pingpong_begin: NULL tables / optim");
    if (ctx->pp_active) return slk_fail(ctx, SLK_EINVAL, "slk_user_pingpong_begin: a ping-pong is already active on this ctx");
    if (tables->user_bloom || tables->item_bloom || !tables->d_param[0] ||
        (optim->kind != SLK_OPT_ADAGRAD && optim->kind != SLK_OPT_SPARSE_ADAM && optim->kind != SLK_OPT_SGD))
        return slk_fail(ctx, SLK_EINVAL, "slk_user_pingpong_begin: plain tables and a row-sparse optimizer (Adagrad, SparseAdam, SGD) only");
    int vec, g, rc;
    if ((rc = slk_check_tables(ctx, tables, 15u, &vec, &g, /*shadow_ok=*/true))) return rc;
    SLK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)tables->num_users;
    if ((rc = slk_ensure(ctx, ctx->pp_alt, rows * (size_t)tables->dim * 4))) return rc;
    if ((rc = slk_ensure(ctx, ctx->pp_flags, (rows + 15) / 16 * 16))) return rc;
    SLK_HIP(ctx, hipMemsetAsync(ctx->pp_flags.p, 0, (rows + 15) / 16 * 16, s));  // every current row is the caller's
    ctx->pp_src_u = tables->d_param[0];
    ctx->pp_rows = tables->num_users;
    ctx->pp_dim = tables->dim;
    ctx->pp_active = true;
    ctx->last_stream = s;
    return SLK_OK;
}

SLK_EXPORT int slk_user_pingpong_end(slk_ctx *ctx, void *stream) {
    if (!ctx) return SLK_EINVAL;
    if (!ctx->pp_active) return SLK_OK;
    // closed on every return (as slk_bias_shadow_end): a failed launch leaves the caller's table a mix of rows, and says so
    float *const dst = ctx->pp_src_u;
    const int64_t rows = ctx->pp_rows;
    const int D = ctx->pp_dim;
    ctx->pp_active = false;
    ctx->pp_src_u = nullptr;
    SLK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pingpong_merge, dim3(slk_grid_for(ctx, (size_t)rows * (size_t)((D + 3) / 4), 256)), dim3(256), 0, s, dst,
                       (const float *)ctx->pp_alt.p, (const uint8_t *)ctx->pp_flags.p, (size_t)rows, D);
    SLK_LAUNCH_CHECK(ctx, "k_pingpong_merge");
    ctx->last_stream = s;
    return SLK_OK;
}

SLK_EXPORT int slk_user_pingpong_abort(slk_ctx *ctx) {
    if (!ctx) return SLK_EINVAL;
    ctx->pp_active = false;
    ctx->pp_src_u = nullptr;
    return SLK_OK;
}
