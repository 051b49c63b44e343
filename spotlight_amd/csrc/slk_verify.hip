// slk_verify.hip -- verified negatives (include/spotlight_hip.h: slk_verify_negatives): of the `tries` candidates drawn up
// front for every negative slot, the first one that is not in the user's history.
//
// A minibatch of bm positives owns a candidate block [tries][n_neg][bm] (the reference's view(rows, bm) of ONE draw of
// tries * n_neg * bm values) and an output block [n_neg][bm]; the blocks of successive minibatches follow each other, so the
// candidate block of the minibatch that starts at interaction m0 starts at m0 * n_neg * tries and its output block at
// m0 * n_neg.  One thread per output slot, column fastest: the user ids, the candidates of one attempt row and the outputs
// of a wavefront are consecutive addresses.  Per attempt a binary search of the user's segment of the CSR; the first unseen
// candidate ends the thread's work.  Every loop is bounded by a constant (16 attempts, 64 halvings) whatever the CSR holds.
#include "slk_common.h"

#define SLK_VERIFY_TRIES_MAX 16
#define SLK_VERIFY_HALVINGS 64

struct slk_verify_args {
    const int64_t *users, *cand, *seen_off, *seen_items;
    unsigned long long slots;    // n * n_neg output slots
    unsigned long long full;     // batch_size * n_neg: the output slots of a full minibatch
    unsigned long long n, bsz, num_users;
    int nn, tries;
    int64_t *out;
    unsigned long long *counts;  // NULL: not counted
};

// is x in the ascending range items[lo, hi)?  (lower bound in at most SLK_VERIFY_HALVINGS steps, then one comparison)
__device__ __forceinline__ bool verify_seen(const int64_t *items, unsigned long long lo, unsigned long long hi, int64_t x) {
    const unsigned long long end = hi;
    for (int step = 0; step < SLK_VERIFY_HALVINGS && lo < hi; ++step) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if (items[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && items[lo] == x;
}

__global__ __launch_bounds__(256) void k_verify_negatives(slk_verify_args a) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = g < a.slots;
    bool replaced = false, unresolved = false;
    if (live) {
        const unsigned long long mb = g / a.full, m0 = mb * a.bsz;
        const unsigned long long bm = a.n - m0 < a.bsz ? a.n - m0 : a.bsz;
        const unsigned long long rem = g - mb * a.full, r = rem / bm, c = rem - r * bm;
        const int64_t *cand = a.cand + m0 * (unsigned long long)a.nn * (unsigned long long)a.tries + r * bm + c;
        const unsigned long long row = (unsigned long long)a.nn * bm;  // candidates of one attempt
        // the user's segment, held inside the items array whatever the offsets say (the last offset is its length); a user id
        // outside [0, num_users) has no history
        const unsigned long long u = (unsigned long long)a.users[m0 + c];
        unsigned long long lo = 0, hi = 0;
        if (u < a.num_users) {
            const unsigned long long total = (unsigned long long)a.seen_off[a.num_users];
            lo = (unsigned long long)a.seen_off[u];
            hi = (unsigned long long)a.seen_off[u + 1];
            if (hi > total) hi = total;
            if (lo > hi) lo = hi;
        }
        const int64_t first = cand[0];
        int64_t pick = first;
        unresolved = true;
        for (int t = 0; t < SLK_VERIFY_TRIES_MAX && t < a.tries; ++t) {
            const int64_t x = t ? cand[(unsigned long long)t * row] : first;
            if (!verify_seen(a.seen_items, lo, hi, x)) {
                pick = x;
                unresolved = false;
                replaced = t > 0;
                break;
            }
        }
        a.out[g] = pick;
    }
    if (a.counts) {  // (uniform over the grid: every lane of a wavefront votes)
        const unsigned long long n_rep = (unsigned long long)__popcll(__ballot(replaced));
        const unsigned long long n_unr = (unsigned long long)__popcll(__ballot(unresolved));
        const int lane = threadIdx.x & 63;
        // one atomic instruction per wavefront: lane 0 adds `replaced`, lane 1 `unresolved`
        if (lane < 2 && (n_rep | n_unr)) atomicAdd(a.counts + lane, lane ? n_unr : n_rep);
    }
}

SLK_EXPORT int slk_verify_negatives(slk_ctx *ctx, const int64_t *d_users, int64_t n, int64_t batch_size, int32_t n_neg, int32_t tries,
                                    const int64_t *d_cand, const int64_t *d_seen_off, const int64_t *d_seen_items, int64_t num_users,
                                    int64_t *d_neg_out, int64_t *d_counts, void *stream) {
    if (!ctx) return SLK_EINVAL;
    if (tries < 1 || tries > SLK_VERIFY_TRIES_MAX)
        return slk_fail(ctx, SLK_EINVAL, "slk_verify_negatives: tries %d outside [1, %d]", (int)tries, SLK_VERIFY_TRIES_MAX);
    if (n_neg < 1) return slk_fail(ctx, SLK_EINVAL, "slk_verify_negatives: n_neg %d < 1", (int)n_neg);
    if (batch_size < 1) return slk_fail(ctx, SLK_EINVAL, "slk_verify_negatives: batch_size %lld < 1", (long long)batch_size);
    if (n < 0) return slk_fail(ctx, SLK_EINVAL, "slk_verify_negatives: negative n");
    if (num_users < 0) return slk_fail(ctx, SLK_EINVAL, "slk_verify_negatives: negative num_users");
    if (n == 0) return SLK_OK;
    if (!d_users || !d_cand || !d_seen_off || !d_seen_items || !d_neg_out)
        return slk_fail(ctx, SLK_EINVAL, "slk_verify_negatives: d_users, d_cand, d_seen_off, d_seen_items or d_neg_out is NULL");
    if (n > (int64_t)1 << 40) return slk_fail(ctx, SLK_EINVAL, "slk_verify_negatives: n %lld too large for one call", (long long)n);
    if (batch_size > n) batch_size = n;  // one (short) minibatch either way
    const unsigned long long slots = (unsigned long long)n * (unsigned long long)n_neg;
    const unsigned long long blocks = (slots + 255) / 256;
    if (blocks > 0x7fffffffull) return slk_fail(ctx, SLK_EINVAL, "slk_verify_negatives: n * n_neg too large for one call");
    // the output of a slot is written while other slots still read their candidates
    const uintptr_t c0 = (uintptr_t)d_cand, c1 = c0 + (uintptr_t)(slots * (unsigned long long)tries * 8);
    const uintptr_t o0 = (uintptr_t)d_neg_out, o1 = o0 + (uintptr_t)(slots * 8);
    if (o0 < c1 && c0 < o1) return slk_fail(ctx, SLK_EINVAL, "slk_verify_negatives: d_neg_out overlaps d_cand");
    int rc;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SAMPLE))) return rc;
    slk_verify_args a;
    a.users = d_users;
    a.cand = d_cand;
    a.seen_off = d_seen_off;
    a.seen_items = d_seen_items;
    a.slots = slots;
    a.full = (unsigned long long)batch_size * (unsigned long long)n_neg;
    a.n = (unsigned long long)n;
    a.bsz = (unsigned long long)batch_size;
    a.num_users = (unsigned long long)num_users;
    a.nn = n_neg;
    a.tries = tries;
    a.out = d_neg_out;
    a.counts = (unsigned long long *)d_counts;
    hipLaunchKernelGGL(k_verify_negatives, dim3((unsigned)blocks), dim3(256), 0, call.s, a);
    SLK_LAUNCH_CHECK(ctx, "k_verify_negatives");
    return SLK_OK;
}
