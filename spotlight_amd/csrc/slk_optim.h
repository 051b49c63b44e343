// slk_optim.h -- ONE optimizer step, written once: the per-kind predicates, the per-step coefficients (host) and the update
// rule on one element (device).  Every training route -- the per-minibatch passes (slk_apply_vec_pre, slk_kernels.h), the
// dense sweep (k_dense_sweep_all), the persistent epoch kernel (slk_epoch_update), the row-sharded path, PoolNet and fold-in --
// calls slk_opt_step; a route owns only how it loads and stores what the rule reads and writes.  The build keeps
// -ffp-contract=off, so the inlined rule performs the same operations, in the same order, in every caller: the routes agree
// bit for bit.  (oracle/slk_oracle.c and the numpy bounds of the tests state the same rules independently, on purpose.)
#pragma once
#include <math.h>

#include "slk_common.h"

// ---- what an optimizer kind (enum slk_opt) needs -----------------------------------------------------------------------
constexpr int SLK_OPT_NONE = -1;  // no rule: SLK_UPD_GRAD_ONLY of the fused passes (slk_kernels.h); every predicate is false

// first state rows (S1): Adagrad's sum, Adam's exp_avg.  SGD is stateless
constexpr bool slk_opt_has_s1(int kind) {
    return kind == SLK_OPT_ADAGRAD || kind == SLK_OPT_SPARSE_ADAM || kind == SLK_OPT_ADAM_DENSE || kind == SLK_OPT_ADAGRAD_DENSE;
}
// second state rows (S2): Adam's exp_avg_sq
constexpr bool slk_opt_has_s2(int kind) { return kind == SLK_OPT_SPARSE_ADAM || kind == SLK_OPT_ADAM_DENSE; }
// EVERY row is updated every step (weight decay, decaying moments): a full-table sweep, not only the looked-up rows
constexpr bool slk_opt_is_dense(int kind) { return kind == SLK_OPT_ADAM_DENSE || kind == SLK_OPT_ADAGRAD_DENSE; }
// a zero summed gradient leaves the row exactly as it is (no write needed): Adagrad (sum += 0, p -= 0) and SGD (p -= 0)
constexpr bool slk_opt_zero_is_noop(int kind) { return kind == SLK_OPT_ADAGRAD || kind == SLK_OPT_SGD; }

// ---- coefficients --------------------------------------------------------------------------------------------------------
// what depends on the step count (bias corrections, lr decay)
struct slk_opt_coef {
    float c0;  // Adagrad (sparse / dense): clr.  SparseAdam: lr * sqrt(bc2) / bc1.  Adam dense: lr / bc1.  SGD: lr
    float c1;  // Adam dense: sqrt(bc2); else 0
};
// what does not
struct slk_opt_hyper {
    float eps, omb1, omb2, beta2, wd;  // omb = 1 - beta; wd = weight_decay
};

// Formed in double and rounded to fp32 exactly as torch does (its hyper-parameters are Python floats).
// step_no: the number of the step being taken, from 1 (torch state['step'] after its increment).
static inline slk_opt_coef slk_opt_coef_at(const slk_optim *optim, int64_t step_no) {
    const double step = (double)step_no;
    slk_opt_coef c = {0.0f, 0.0f};
    if (optim->kind == SLK_OPT_SGD) {
        c.c0 = (float)optim->lr;
    } else if (optim->kind == SLK_OPT_ADAGRAD || optim->kind == SLK_OPT_ADAGRAD_DENSE) {
        c.c0 = (float)(optim->lr / (1.0 + (step - 1.0) * optim->lr_decay));
    } else {
        const double bc1 = 1.0 - pow(optim->beta1, step), bc2 = 1.0 - pow(optim->beta2, step);
        if (optim->kind == SLK_OPT_SPARSE_ADAM) {
            c.c0 = (float)(optim->lr * sqrt(bc2) / bc1);
        } else {
            c.c0 = (float)(optim->lr / bc1);
            c.c1 = (float)sqrt(bc2);
        }
    }
    return c;
}

static inline slk_opt_hyper slk_opt_hyper_of(const slk_optim *optim) {
    slk_opt_hyper h;
    h.eps = (float)optim->eps;
    h.omb1 = (float)(1.0 - optim->beta1);
    h.omb2 = (float)(1.0 - optim->beta2);
    h.beta2 = (float)optim->beta2;
    h.wd = (float)optim->weight_decay;
    return h;
}

// ---- the rule --------------------------------------------------------------------------------------------------------------
// One element's step: parameter p, its state s1 / s2 (untouched where the kind has none), summed gradient g.  No loads, no
// stores: the caller's.  A row that is touched at every step gets the same update from the sparse and the dense form of an
// optimizer up to weight decay, lr_decay (in c0) and the two Adam roundings.
template <int KIND>
__device__ __forceinline__ void slk_opt_step(const slk_opt_hyper &h, const slk_opt_coef &c, float &p, float &s1, float &s2, float g) {
    static_assert(KIND >= SLK_OPT_ADAGRAD && KIND <= SLK_OPT_SGD, "an optimizer kind of enum slk_opt");
    if (KIND == SLK_OPT_ADAGRAD) {
        // torch/optim/adagrad.py:360-385: sum += g^2; p += -clr * (g / (sqrt(sum) + eps))
        s1 += g * g;
        p += -c.c0 * (g / (sqrtf(s1) + h.eps));
    } else if (KIND == SLK_OPT_SPARSE_ADAM) {
        // torch/optim/_functional.py:61-84
        const float mu = (g - s1) * h.omb1;
        const float vu = (g * g - s2) * h.omb2;
        s1 = mu + s1;
        s2 = vu + s2;
        p += -c.c0 * (s1 / (sqrtf(s2) + h.eps));
    } else if (KIND == SLK_OPT_SGD) {
        // torch/optim/sgd.py (momentum 0, weight_decay 0): param.add_(grad, alpha=-lr)
        p += -c.c0 * g;
    } else if (KIND == SLK_OPT_ADAM_DENSE) {
        // torch/optim/adam.py:414-546 (single-tensor): g += wd*p; m.lerp_(g, 1-b1);
        // v = b2*v + (1-b2) g^2; p += -(lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
        const float gv = g + h.wd * p;
        const float m = s1 + h.omb1 * (gv - s1);
        const float v = s2 * h.beta2 + h.omb2 * (gv * gv);
        s1 = m;
        s2 = v;
        p += -c.c0 * (m / (sqrtf(v) / c.c1 + h.eps));
    } else {
        // torch/optim/adagrad.py:350-385 dense branch with weight_decay
        const float gv = g + h.wd * p;
        const float s = s1 + gv * gv;
        s1 = s;
        p += -c.c0 * (gv / (sqrtf(s) + h.eps));
    }
}
