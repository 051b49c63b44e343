"""The loss functions of spotlight/losses.py:18-244 as plain torch functions, for code that
imports them directly (custom training loops, tests).  The models of this package do NOT call
these: their forward, loss, backward and update are fused in the gfx950 kernels
(csrc/slk_kernels.h: slk_pair_loss, csrc/slk_bilinear.hip: k_adaptive_select / k_explicit_loss),
which follow the same formulas operation by operation.

Implicit-feedback losses take (positive_predictions, negative_predictions[, mask]); with a mask
(sequence models: mask = sequence != 0) the mean is over the unmasked entries only.

`weights` (not in the reference; every loss, default None = the reference's mean): one weight per interaction, the loss is
sum(w_i * l_i) / sum(w_i) over the per-interaction terms l_i -- what fit() of a model built with use_weights=True minimises
(include/spotlight_hip.h: slk_bilinear_train_weighted).  Under adaptive hinge the weight of a column is the weight of its positive.
"""
import torch
import torch.nn.functional as F

from spotlight_amd.torch_utils import assert_no_grad


def _masked_mean(values, mask, weights=None):
    if mask is None and weights is None:
        return values.mean()
    if weights is None:
        weights = mask.float()
    elif mask is not None:
        weights = weights * mask.float()
    return (values * weights).sum() / weights.sum()


def pointwise_loss(positive_predictions, negative_predictions, mask=None, weights=None):
    """Logistic loss: (1 - sigmoid(pos)) + sigmoid(neg)   (losses.py:18-50)."""
    return _masked_mean((1.0 - torch.sigmoid(positive_predictions)) + torch.sigmoid(negative_predictions), mask, weights)


def bpr_loss(positive_predictions, negative_predictions, mask=None, weights=None):
    """Spotlight's BPR variant: 1 - sigmoid(pos - neg) -- not -log sigmoid   (losses.py:53-90)."""
    return _masked_mean(1.0 - torch.sigmoid(positive_predictions - negative_predictions), mask, weights)


def hinge_loss(positive_predictions, negative_predictions, mask=None, weights=None):
    """max(0, neg - pos + 1)   (losses.py:93-124)."""
    return _masked_mean(torch.clamp(negative_predictions - positive_predictions + 1.0, 0.0), mask, weights)


def adaptive_hinge_loss(positive_predictions, negative_predictions, mask=None, weights=None):
    """Hinge loss against the highest-scoring of several sampled negatives: negative_predictions has the
    candidates along dim 0   (losses.py:127-166)."""
    hardest, _ = negative_predictions.max(0)
    return hinge_loss(positive_predictions, hardest.squeeze(), mask=mask, weights=weights)


def warp_loss(positive_predictions, negative_predictions, num_items, mask=None, weights=None):
    """WARP (WSABIE; LightFM's loss='warp'; not in the reference): the hinge against the FIRST of the sampled negatives
    that violates the margin, scaled by a weight from how many tries it took.  negative_predictions has the candidates
    along dim 0, in draw order, as for adaptive_hinge_loss.  Per column, with x_r = neg_r - pos + 1:

        t = the smallest r with x_r > 0 (strict; a NaN does not violate); none: the column's term is 0, no gradient
        w = log(max(1, (num_items - 1) // (t + 1)))         -- LightFM's rank estimate floor((I - 1) / tries)
        l = w * x_t

    The weight is a constant of the backward pass: d l / d pos = -w, d l / d neg_t = +w, every other candidate 0.
    All candidates are scored (no early stop).  The estimate assumes uniform draws; under
    negative_sampling='popularity' it is a popularity-weighted rank   (include/spotlight_hip.h: SLK_LOSS_WARP)."""
    x = negative_predictions - positive_predictions.unsqueeze(0) + 1.0
    viol = x > 0
    n = x.shape[0]
    rows = torch.arange(n, device=x.device).view((n,) + (1,) * (x.dim() - 1)).expand_as(x)
    first = torch.where(viol, rows, torch.full_like(rows, n)).min(0)[0]
    hit = first < n
    t = first.clamp(max=n - 1)
    rank = torch.div(torch.full_like(t, int(num_items) - 1), t + 1, rounding_mode='floor').clamp(min=1)
    w = torch.log(rank.to(x.dtype))  # fp32 predictions: logf of the fp32 rank, as the kernels form it
    x_t = x.gather(0, t.unsqueeze(0)).squeeze(0)
    terms = torch.where(hit, w * x_t, torch.zeros_like(x_t))
    return _masked_mean(terms, mask, weights)


def softmax_loss(positive_predictions, negative_predictions, mask=None, weights=None):
    """Sampled softmax (InfoNCE; not in the reference): -log of the positive's share of the softmax over the positive and its
    OWN sampled negatives.  negative_predictions is [n, B]: column c holds the n negatives drawn FOR positive c (the same
    user) -- not the reference's view(n, B) of a user-major draw, whose column c holds other users' draws.  Per column

        l = logsumexp([pos; neg_1 .. neg_n]) - pos

    Every candidate carries a gradient, softmax(.)_j, the positive softmax(.)_0 - 1.  A negative equal to the positive is not
    masked; no logQ correction under negative_sampling='popularity'   (include/spotlight_hip.h: SLK_LOSS_SOFTMAX)."""
    scores = torch.cat([positive_predictions.unsqueeze(0), negative_predictions], 0)
    return _masked_mean(torch.logsumexp(scores, 0) - positive_predictions, mask, weights)


def regression_loss(observed_ratings, predicted_ratings, weights=None):
    """Mean squared error   (losses.py:169-191)."""
    assert_no_grad(observed_ratings)
    return _masked_mean((observed_ratings - predicted_ratings) ** 2, None, weights)


def poisson_loss(observed_ratings, predicted_ratings, weights=None):
    """Poisson negative log-likelihood up to a constant: pred - obs * log(pred)   (losses.py:194-216)."""
    assert_no_grad(observed_ratings)
    return _masked_mean(predicted_ratings - observed_ratings * torch.log(predicted_ratings), None, weights)


def logistic_loss(observed_ratings, predicted_ratings, weights=None):
    """Binary cross-entropy with logits; observed ratings are -1 / +1   (losses.py:219-244)."""
    assert_no_grad(observed_ratings)
    targets = torch.clamp(observed_ratings, 0, 1)
    if weights is None:
        return F.binary_cross_entropy_with_logits(predicted_ratings, targets, reduction='mean')
    return _masked_mean(F.binary_cross_entropy_with_logits(predicted_ratings, targets, reduction='none'), None, weights)
