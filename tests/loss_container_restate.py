"""float64 restatement of the reference's loss container (ndsis/modules/loss.py Loss.forward :101-191), with the crossed RPN
weights spelled out, and the error bounds the tests hold kernel and fixtures to.

    terms       t = (rpn_score, rpn_bbox, class, mask, segmentation)
    log-weights w = (rpn_class, rpn_bbox, class, mask, segmentation)
    rpn_score is scaled by exp(-w[rpn_bbox]) and rpn_bbox by exp(-w[rpn_class]); class, mask and segmentation by their own.

Bound: each of at most 5 products carries exp (<= 2 ulp) and one multiplication, at most 10 additions carry half an ulp of the
running sum each: 16 units of 2^-24 times the quantity's scale S cover the worst case.
"""
import numpy as np

TERM_NAMES = ("rpn_score", "rpn_bbox", "class", "mask", "segmentation")
WEIGHT_NAMES = ("rpn_class", "rpn_bbox", "class", "mask", "segmentation")
RPN_SCORE, RPN_BBOX, CLASS, MASK, SEGMENTATION = range(5)
W_RPN_CLASS, W_RPN_BBOX, W_CLASS, W_MASK, W_SEGMENTATION = range(5)
WEIGHT_OF_TERM = {RPN_SCORE: W_RPN_BBOX, RPN_BBOX: W_RPN_CLASS, CLASS: W_CLASS, MASK: W_MASK, SEGMENTATION: W_SEGMENTATION}
UNITS = 16
EPS = 2.0 ** -24


def combine(terms, present, log_weights, scale=1.0):
    """terms [5] (entries of absent terms ignored), present [5] bool, log_weights [5] -> dict of float64 results for the
    upstream gradient `scale`: total, total_multitask, term_grad [5], weight_grad [5] (0 where the term is absent),
    weight_used [5] bool, and the scales S_total, S_multitask, S_term_grad [5], S_weight_grad [5] of the bounds."""
    t = np.asarray(terms, np.float64)
    w = np.asarray(log_weights, np.float64)
    total = extra = 0.0
    s_total = s_extra = 0.0
    term_grad, weight_grad = np.zeros(5), np.zeros(5)
    s_term, s_weight = np.zeros(5), np.zeros(5)
    used = np.zeros(5, bool)
    for i in range(5):
        if not present[i]:
            continue
        j = WEIGHT_OF_TERM[i]
        c = np.exp(-w[j])
        total += t[i] * c
        extra += w[j]
        s_total += abs(t[i] * c)
        s_extra += abs(w[j])
        term_grad[i] = scale * c
        weight_grad[j] = scale * (1.0 - t[i] * c)
        s_term[i] = abs(scale) * abs(c)
        s_weight[j] = abs(scale) * (1.0 + abs(t[i] * c))
        used[j] = True
    return dict(total=total, total_multitask=total + extra, term_grad=term_grad, weight_grad=weight_grad, weight_used=used,
                S_total=s_total, S_multitask=s_total + s_extra, S_term_grad=s_term, S_weight_grad=s_weight)


def bound(scale, units=UNITS):
    return units * EPS * np.asarray(scale, np.float64)


def plain_sum_f32(terms, present):
    """((0 + t_0) + t_1) + ... over the present terms in fp32: what `_total_` must equal bit for bit when every weight is 1."""
    acc = np.float32(0.0)
    for i in range(5):
        if present[i]:
            acc = np.float32(acc + np.float32(terms[i]))
    return acc
