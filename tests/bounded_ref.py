"""Plain references of the bounded critic update's rules in include/kinova_rollout.h (kr_critic_grad_bounded, kr_grad_sqnorm,
kr_adam_step_clipped), written from the header's rules - not from the kernels - in the manner of tests/glue_ref.py and tests/td3_ref.py:
float64 arithmetic on float32 inputs widened exactly, except where a float32 operation IS the rule (the clamp of the bootstrap, which is
exact in the input's type, and the three float32 operations of the clip coefficient).

tests/test_bounded_reference_cpu.py checks these functions against float64 autograd of ddpgfd.DDPGfD / TD3fD with the options set and
against torch.nn.utils.clip_grad_norm_; tests/test_gpu_bounded_kernels.py then holds every kernel to them."""
import math

import numpy as np

from tests import glue_ref as gr
from tests import td3_ref as tr

NORM_PARTS = 64            # KR_NORM_PARTS
NORM_STRIDE = 64 * NORM_PARTS


def bound(x, lo, hi):
    """x < lo ? lo : (x > hi ? hi : x) in x's own type (the bounds are converted to it first): exact, a NaN passes through"""
    x = np.asarray(x)
    t = x.dtype.type
    with np.errstate(invalid="ignore"):
        return tr.clamp(x, t(lo), t(hi)).astype(x.dtype)


def rho(e, d):
    """twice the Huber function: e^2 where not |e| > d, d (2 |e| - d) otherwise; a NaN takes the square branch and stays NaN"""
    if d == np.inf:                                   # |e| > inf holds for no e
        return e * e
    a = np.abs(e)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(a > d, d * (2.0 * a - d), e * e)


def huber_clip(e, d):
    """rho's derivative over 2: e where not |e| > d, else d with e's sign"""
    if d == np.inf:
        return e
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(e) > d, np.sign(e) * d, e)


def bootstrap(tq1_a, tq1_b, tqn_a, tqn_b, lo, hi):
    """(b1, bn): the minimum of the two target critics (one critic: tq*_b None), then the clamp - both exact in the inputs' type"""
    m1 = np.asarray(tq1_a) if tq1_b is None else tr.nan_min(np.asarray(tq1_a), np.asarray(tq1_b))
    mn = np.asarray(tqn_a) if tqn_b is None else tr.nan_min(np.asarray(tqn_a), np.asarray(tqn_b))
    return bound(m1, lo, hi), bound(mn, lo, hi)


def critic_grad_bounded_ref(q1, q2, tq1_a, tq1_b, tqn_a, tqn_b, reward, weight, wsum, discount, lo, hi, delta):
    """One critic (q2, tq1_b, tqn_b None) or two.  b1, bn as bootstrap(); targets from them as glue_ref.critic_targets; per critic k
        e1 = q_k - target_Q, en = q_k - target_QN;   dq_k = w / wsum (2 c(e1) + c(en));   L1 = sum w rho(e1) / wsum, LN likewise,
        loss = L1 + 0.5 LN;   wsum <= 0: dq and losses are 0 (tboot is formed all the same).
    Returns dq1, dq2 (None for one critic), tboot [2R] in the inputs' type, losses (three or six floats)."""
    b1, bn = bootstrap(tq1_a, tq1_b, tqn_a, tqn_b, lo, hi)
    t1, tn = gr.critic_targets(b1, bn, reward, discount)
    dqs, losses = [], ()
    for q in (q1, q2):
        if q is None:
            dqs.append(None)
            continue
        q = gr.wide(q)
        w = np.ones_like(q) if weight is None else gr.wide(weight)
        if wsum <= 0:
            dqs.append(np.zeros_like(q))
            losses += (0.0, 0.0, 0.0)
            continue
        e1, en = q - t1, q - tn
        l1, ln = float((w * rho(e1, delta)).sum() / wsum), float((w * rho(en, delta)).sum() / wsum)
        dqs.append(w / wsum * (2.0 * huber_clip(e1, delta) + huber_clip(en, delta)))
        losses += (l1 + 0.5 * ln, l1, ln)
    return dqs[0], dqs[1], np.concatenate([b1, bn]), losses


def part_indices(count, b):
    """the elements workgroup b of kr_grad_sqnorm adds: i = 64 b + l + 4096 k for its 64 lanes l and k = 0, 1, ..."""
    i = np.arange(count)
    return i[(i % NORM_STRIDE) // 64 == b]


def sqnorm_ref(g):
    """the sum of the squares, correctly rounded to float64: the square of a widened float32 is exact in float64, math.fsum adds exactly"""
    g = gr.wide(np.asarray(g).reshape(-1))
    return math.fsum((g * g).tolist())


def sqnorm_parts_ref(g):
    """sqnorm_ref of each workgroup's own elements, [NORM_PARTS]"""
    g = np.asarray(g).reshape(-1)
    return np.array([sqnorm_ref(g[part_indices(g.size, b)]) for b in range(NORM_PARTS)])


def clip_coef_f32(total, max_norm):
    """the header's three float32 operations on the float64 total: norm = sqrtf((float)total); coef = max_norm / (norm + 1e-6f);
    coef = coef > 1 ? 1 : coef (a NaN stays NaN).  Returns (norm, coef) as float32."""
    f = np.float32
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        norm = np.sqrt(f(total), dtype=f)
        coef = f(f(max_norm) / f(norm + f(1e-6)))
    return norm, (f(1.0) if coef > f(1.0) else coef)


def adam_clipped_ref(p, g, m, v, step, every, coef, lr, b1, b2, eps, wd):
    """td3_ref.adam_every_ref (glue_ref.adam_ref behind the gate on step and every) on g * coef; the scaling comes before the weight-decay
    term, where clip_grad_norm_ acts.  Returns (p', m', v') in float64."""
    return tr.adam_every_ref(p, gr.wide(g) * float(coef), m, v, step, every, lr, b1, b2, eps, wd)
