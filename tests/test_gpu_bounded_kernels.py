"""The three kernels of the bounded critic update (kr_critic_grad_bounded, kr_grad_sqnorm, kr_adam_step_clipped of csrc/ks_rollout.hip) on
their own against the references of tests/bounded_ref.py (which tests/test_bounded_reference_cpu.py checks on the host), by the method
of tests/test_gpu_glue_kernels.py, whose buffers, bounds and inputs are used here: 0xA5 guards around every writable buffer, U = 2^-24
per rounding of the header's expression, nothing in a bound taken from the kernel's output, an exact case beside each bounded one.
Printed lines starting with GLUE carry the measured worst errors (profiles/bounded_critic.txt is collected from them)."""
import math

import numpy as np
import pytest

from tests import bounded_ref as br
from tests import glue_ref as gr
from tests.test_gpu_glue_kernels import (ADAM_SETS, BETAS, COUNTS, E_POWF, FLOOR, KS_ERR_INVALID, ROWS, SECOND, U, Buf, P, _lib, _rng, _stream,
                                         adam_bounds, adam_inputs, assert_bits, check_bound, critic_bounds, critic_inputs, f32, is_f32, sent, ulp32,
                                         weights_for)
from tests.test_gpu_td3_kernels import run_adam, run_twin, twin_inputs

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
U64 = 2.0 ** -53
LO, HI, DELTA = -1.5, 2.0, 3.0          # exact in float32; inside the inputs' spread (targets ~ 3 N(0, 1), errors of several units)


# ---- kr_critic_grad_bounded ------------------------------------------------------------------------------------------
def run_bounded(R, n, q1, q2, ta1, tb1, tan, tbn, rw, wb, ws, disc, lo, hi, delta):
    twin = q2 is not None
    dq1, dq2 = Buf(sent(R, np.float32)), (Buf(sent(R, np.float32)) if twin else None)
    tboot, ls = Buf(sent(2 * R, np.float32)), Buf(sent(6 if twin else 3, np.float32))
    ins = [None if x is None else Buf(x) for x in (q1, q2, ta1, tb1, tan, tbn, rw)]
    assert _lib().kr_critic_grad_bounded(R, n, *[P(b) for b in ins], P(wb), P(ws), disc, lo, hi, delta, P(dq1), P(dq2), P(tboot), P(ls), _stream()) == 0
    out = dq1.get(), (dq2.get() if twin else None), tboot.get(), ls.get()
    assert all(b is None or b.unchanged() for b in ins)
    return out


def form_inputs(twin, R, n, r):
    q1, q2, ta1, tb1, tan, tbn, rw = twin_inputs(R, n, r)
    return (q1, q2, ta1, tb1, tan, tbn, rw) if twin else (q1, None, ta1, None, tan, None, rw)


def bounded_bounds(q, b1, bn, rw, w, wsum, disc, delta):
    """critic_bounds on (q, b1, bn) - the clamp is exact, c() is 1-Lipschitz and rho's slope is at most the square's, so the roundings of
    the targets and errors carry into dq and the loss terms no further than into kr_critic_grad's, and a term whose computed error falls on
    the other side of |e| = delta than the reference's differs from its own branch by (|e| - delta)^2 <= de^2, which the carried term
    holds - plus ONE more rounding per Huber-branch loss term: fl(w fl(delta fl(fl(2 |e|) - delta))) has three roundings (2 |e| is exact)
    where fl(fl(w e) e) has two, so U w rho(e) / wsum is added per such row."""
    bdq, (_, bl1, bln) = critic_bounds(q, b1, bn, rw, w, wsum, disc)
    if wsum <= 0:
        return bdq, (bl1 + 0.5 * bln, bl1, bln)
    wv = np.ones(q.shape[0]) if w is None else gr.wide(w)
    t1, tn = gr.critic_targets(b1, bn, rw, disc)
    extra = []
    for e in (gr.wide(q) - t1, gr.wide(q) - tn):
        huber = np.abs(e) > delta
        extra.append(U * float((wv * np.where(huber, br.rho(e, delta), 0.0)).sum() / wsum) * SECOND)
    bl1, bln = bl1 + extra[0], bln + extra[1]
    return bdq, (bl1 + 0.5 * bln, bl1, bln)


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("kind", ["01", "null", "zero"])
@pytest.mark.parametrize("twin", [False, True], ids=["single", "twin"])
def test_critic_grad_bounded_within_its_roundings(R, n, kind, twin):
    """wsum from kr_update_prologue's launch on the same weights.  tboot is the reference's clamped bootstrap in every bit; dq_k and the
    loss triples stay within bounded_bounds (kr_critic_grad's roundings on (q_k, b1, bn) + one per Huber-branch loss term);
    losses[0] = fl(losses[1] + fl(0.5 losses[2])) in every bit, likewise 3..5."""
    r = _rng("bounded", R, n, kind, twin)
    disc = float(np.float32(0.995))
    q1, q2, ta1, tb1, tan, tbn, rw = form_inputs(twin, R, n, r)
    w = weights_for(kind, R, r)
    wb = None if w is None else Buf(w)
    ws = Buf(sent(1, np.float32))
    assert _lib().kr_update_prologue(R, n, P(wb), P(ws), P(Buf(sent(R * n, np.float32))), P(Buf(np.zeros(1, np.int64))), P(Buf(np.zeros(1, np.int64))), 0,
                                     _stream()) == 0
    wsum = gr.prologue_ref(R, n, w, 0, 0, 0)[0]
    assert_bits(ws.get(), np.array([wsum]), "weight_sum")
    dq1, dq2, tboot, ls = run_bounded(R, n, q1, q2, ta1, tb1, tan, tbn, rw, wb, ws, disc, LO, HI, DELTA)
    r1, r2, rboot, rls = br.critic_grad_bounded_ref(q1, q2, ta1, tb1, tan, tbn, rw, w, wsum, disc, LO, HI, DELTA)
    assert_bits(tboot, rboot, "tboot")
    case = f"R {R} n {n} weights {kind} {'twin' if twin else 'single'}"
    if R >= 64:
        m1 = ta1 if not twin else np.minimum(ta1, tb1)
        t1, tn = gr.critic_targets(rboot[:R], rboot[R:], rw, disc)
        e = np.concatenate([gr.wide(q1) - t1, gr.wide(q1) - tn])
        assert (m1 < LO).any() and (m1 > HI).any() and ((m1 > LO) & (m1 < HI)).any() and (rboot == np.float32(LO)).any() and (rboot == np.float32(HI)).any()
        assert (e > DELTA).any() and (e < -DELTA).any() and (np.abs(e) < DELTA).any()
    for k, (q, dq, rdq) in enumerate(((q1, dq1, r1), (q2, dq2, r2))[:2 if twin else 1]):
        bdq, bls = bounded_bounds(q, rboot[:R], rboot[R:], rw, w, wsum, disc, DELTA)
        check_bound(dq, rdq, bdq, "kr_critic_grad_bounded", case, f"dq{k + 1}")
        check_bound(ls[3 * k:3 * k + 3], np.array(rls[3 * k:3 * k + 3]), np.array(bls), "kr_critic_grad_bounded", case, f"losses of critic {k + 1}")
        assert_bits(ls[3 * k:3 * k + 1], np.array([ls[3 * k + 1] + np.float32(0.5) * ls[3 * k + 2]], np.float32), "loss = L1 + 0.5 LN")
    if kind == "zero":
        assert not dq1.any() and not ls.any() and (dq2 is None or not dq2.any())


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("kind", ["01", "null"])
@pytest.mark.parametrize("twin", [False, True], ids=["single", "twin"])
def test_critic_grad_bounded_degenerate_zero_weight_sum_and_nan(R, n, kind, twin):
    """q_lo = -inf, q_hi = +inf, huber_delta = +inf: every output bit is kr_critic_grad's (single; tboot = (tq1, tqn)) or
    kr_twin_critic_grad's (twin; tboot = tmin).  wsum = 0 handed in: dq and the losses are 0, tboot is written all the same.  A NaN in one
    target: NaN in that row's tboot and dq, the other rows as without it."""
    r = _rng("bounded0", R, n, kind, twin)
    disc = float(np.float32(0.995))
    q1, q2, ta1, tb1, tan, tbn, rw = form_inputs(twin, R, n, r)
    w = weights_for(kind, R, r)
    wb = None if w is None else Buf(w)
    wsum = gr.prologue_ref(R, n, w, 0, 0, 0)[0]
    ws = Buf(np.array([wsum], np.float32))
    # degenerate
    d1, d2, tb, ls = run_bounded(R, n, q1, q2, ta1, tb1, tan, tbn, rw, wb, ws, disc, -INF, INF, INF)
    if twin:
        e1, e2, tmin, l6 = run_twin(R, n, q1, q2, ta1, tb1, tan, tbn, rw, wb, ws, disc)
        assert_bits(d1, e1, "dq1 = kr_twin_critic_grad's")
        assert_bits(d2, e2, "dq2 = kr_twin_critic_grad's")
        assert_bits(tb, tmin, "tboot = tmin")
        assert_bits(ls, l6, "losses = kr_twin_critic_grad's")
    else:
        dq, l3 = Buf(sent(R, np.float32)), Buf(sent(3, np.float32))
        assert _lib().kr_critic_grad(R, n, P(Buf(q1)), P(Buf(ta1)), P(Buf(tan)), P(Buf(rw)), P(wb), P(ws), disc, P(dq), P(l3), _stream()) == 0
        assert_bits(d1, dq.get(), "dq = kr_critic_grad's")
        assert_bits(tb, np.concatenate([ta1, tan]), "tboot = (tq1, tqn)")
        assert_bits(ls, l3.get(), "losses = kr_critic_grad's")
    # wsum = 0
    d1, d2, tb, ls = run_bounded(R, n, q1, q2, ta1, tb1, tan, tbn, rw, wb, Buf(np.zeros(1, np.float32)), disc, LO, HI, DELTA)
    assert not d1.any() and not ls.any() and (d2 is None or not d2.any())
    assert_bits(tb, np.concatenate(br.bootstrap(ta1, tb1, tan, tbn, LO, HI)), "tboot with wsum 0")
    # NaN
    clean = run_bounded(R, n, q1, q2, ta1, tb1, tan, tbn, rw, wb, ws, disc, LO, HI, DELTA)
    i, j = 0, R - 1
    ta1n, tlast = ta1.copy(), (tbn if twin else tan).copy()
    ta1n[i], tlast[j] = np.nan, np.nan
    d1, d2, tm, _ = run_bounded(R, n, q1, q2, ta1n, tb1, tlast if not twin else tan, tlast if twin else None, rw, wb, ws, disc, LO, HI, DELTA)
    bad = np.zeros(R, bool)
    bad[[i, j]] = True
    assert np.isnan(tm[i]) and np.isnan(tm[R + j])
    assert np.isnan(d1[bad]).all() and (d2 is None or np.isnan(d2[bad]).all())          # (a padding row too: 0 * NaN)
    keep = np.ones(2 * R, bool)
    keep[[i, R + j]] = False
    if R > 1:
        assert_bits(tm[keep], clean[2][keep], "tboot of the other rows")
        assert_bits(d1[~bad], clean[0][~bad], "dq1 of the other rows")
        if twin:
            assert_bits(d2[~bad], clean[1][~bad], "dq2 of the other rows")


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("twin", [False, True], ids=["single", "twin"])
def test_critic_grad_bounded_exact_on_dyadic_inputs(R, n, twin):
    """discount 0.5, q, targets and rewards in {-2, ..., 2}, bounds +-1, delta 1, a power-of-two count of 0 / 1 weights: the bootstrap is in
    {-1, 0, 1}, targets and errors on the grid 2^-n, the squares (|e| <= 1) on 2^-2n, the Huber terms 2 |e| - 1 on 2^-n, every partial sum
    below 2^24 grid units in any order (asserted) - every output is the reference in every bit.  Rows with |e| = delta exactly are there."""
    r = _rng("boundedx", R, n, twin)
    five = lambda *s: f32(r.randint(-2, 3, s))
    q1, q2, ta1, tb1, tan, tbn, rw = five(R), five(R), five(R), five(R), five(R), five(R), five(R, n)
    if not twin:
        q2 = tb1 = tbn = None
    ones = 1 << (R.bit_length() - 1)
    w = np.zeros(R, np.float32)
    w[r.permutation(R)[:ones]] = 1.0
    wsum = float(ones)
    r1, r2, rboot, rls = br.critic_grad_bounded_ref(q1, q2, ta1, tb1, tan, tbn, rw, w, wsum, 0.5, -1.0, 1.0, 1.0)
    t1, tn = gr.critic_targets(rboot[:R], rboot[R:], rw, 0.5)
    on_edge = False
    for q in (q1, q2)[:2 if twin else 1]:
        for e in (gr.wide(q) - t1, gr.wide(q) - tn):
            terms = br.rho(e, 1.0)
            assert is_f32(e) and is_f32(terms) and terms.sum() * 4.0 ** n < 2.0 ** 24
            on_edge = on_edge or bool((np.abs(e) == 1.0).any())
    assert on_edge or R < 64
    assert is_f32(r1) and (r2 is None or is_f32(r2)) and is_f32(np.array(rls)) and set(np.unique(rboot)) <= {-1.0, 0.0, 1.0}
    dq1, dq2, tboot, ls = run_bounded(R, n, q1, q2, ta1, tb1, tan, tbn, rw, Buf(w), Buf(np.array([wsum], np.float32)), 0.5, -1.0, 1.0, 1.0)
    assert_bits(dq1, r1, "dq1 on dyadic inputs")
    if twin:
        assert_bits(dq2, r2, "dq2 on dyadic inputs")
    assert_bits(tboot, rboot, "tboot on dyadic inputs")
    assert_bits(ls, np.array(rls), "losses on dyadic inputs")


# ---- kr_grad_sqnorm --------------------------------------------------------------------------------------------------
NORM_COUNTS = (1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5, 155401)       # the last: the 400-300 critic


def run_sqnorm(g, offset=0):
    """g: the whole buffer; the call sees g[offset:]"""
    gb, pb = Buf(g), Buf(sent(br.NORM_PARTS, np.float64))
    assert _lib().kr_grad_sqnorm(g.size - offset, P(gb, 4 * offset), P(pb), _stream()) == 0
    parts = pb.get()
    assert gb.unchanged()
    return parts, pb


def butterfly(parts):
    """the 64-lane xor butterfly of kr_adam_step_clipped in float64: a + b = b + a, so every lane holds the same bits after every stage"""
    x, lane = np.asarray(parts, np.float64).copy(), np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[lane ^ o]
    assert (x == x[0]).all() or np.isnan(x).all()
    return float(x[0])


@pytest.mark.parametrize("count", NORM_COUNTS)
@pytest.mark.parametrize("offset", [0, 1])
def test_grad_sqnorm_against_the_exact_sum(count, offset):
    """Every term is an exact non-negative float64 square.  A lane adds ceil(count / 4096) of them, the butterfly has 6 stages: partials[b]
    is within (ceil(count / 4096) + 6) 2^-53 (relative) of the exact sum over its own index set; adding the 64 partials by a second
    butterfly gives the total within (ceil(count / 4096) + 12) 2^-53 of the exact sum of squares, so (float)total is within one float32
    ulp of the correctly rounded one.  offset 1: the gradient is a view that is only 4-byte aligned.  The same call twice gives the same
    64 doubles in every bit."""
    r = _rng("sqnorm", count, offset)
    g = f32(r.standard_normal(count + offset) * 10.0 ** r.randint(-3, 2, count + offset))
    parts, _ = run_sqnorm(g, offset)
    seen = g[offset:]
    trips = -(-count // br.NORM_STRIDE)
    ref_parts = br.sqnorm_parts_ref(seen)
    check_bound(parts, ref_parts, (trips + 6) * U64 * ref_parts * SECOND, "kr_grad_sqnorm", f"count {count} offset {offset}", "partials")
    assert (parts[ref_parts == 0] == 0).all()
    total, ref = butterfly(parts), br.sqnorm_ref(seen)
    assert abs(total - ref) <= (trips + 12) * U64 * ref * SECOND
    assert abs(float(np.float32(total)) - float(np.float32(ref))) <= float(ulp32(ref))
    again, _ = run_sqnorm(g, offset)
    assert_bits(again, parts, "the same call twice")


def test_grad_sqnorm_huge_and_zero_gradients():
    """One element of 1e18 among small ones: its square 1e36 is finite in float32 too, the norm is 1e18 and the coefficient max_norm / 1e18.
    One element of 3e19: the float64 sum (9e38) is finite, its conversion to float32 (maximum 3.4e38) is +inf, the norm +inf, the
    coefficient 0 and the step that of a zero gradient.  An all-zero gradient: norm 0, coefficient 1."""
    count = 4097
    r = _rng("sqnorm-huge")
    for big, inf_norm in ((1e18, False), (3e19, True)):
        g = f32(r.standard_normal(count))
        g[777] = big
        parts, pb = run_sqnorm(g)
        total = butterfly(parts)
        assert math.isfinite(total) and abs(total - br.sqnorm_ref(g)) <= (2 + 12) * U64 * total * SECOND
        (pb_, gb, mb, vb), clip = run_clipped(count, f32(r.standard_normal(count)), g, np.zeros(count, np.float32), np.zeros(count, np.float32), 1, 1, pb, 10.0, 1e-3, 0.0)
        norm, coef = clip
        if inf_norm:
            assert norm == np.float32(np.inf) and coef == 0.0 and not mb.get().any() and not vb.get().any() and pb_.unchanged()
        else:
            assert abs(float(norm) - 1e18) <= 4 * U * 1e18 and abs(float(coef) - 1e-17) <= 8 * U * 1e-17 and np.isfinite(pb_.get()).all()
    g = np.zeros(count, np.float32)
    parts, pb = run_sqnorm(g)
    assert not parts.any()
    (pb_, gb, mb, vb), clip = run_clipped(count, f32(r.standard_normal(count)), g, np.zeros(count, np.float32), np.zeros(count, np.float32), 1, 1, pb, 10.0, 1e-3, 0.0)
    assert clip.tolist() == [0.0, 1.0] and pb_.unchanged()


# ---- kr_adam_step_clipped --------------------------------------------------------------------------------------------
def run_clipped(count, p, g, m, v, step, every, parts, max_norm, lr, wd, clip_out=True):
    """parts: a Buf of 64 doubles (kr_grad_sqnorm's output buffer, or given values).  Returns the four buffers and clip_out's content."""
    b1, b2 = BETAS
    lr32, eps, wd32 = float(np.float32(lr)), float(np.float32(1e-8)), float(np.float32(wd))
    bufs = [Buf(x) for x in (p, g, m, v)] + [Buf(np.array([step], np.int64))]
    cb = Buf(sent(2, np.float32)) if clip_out else None
    before = parts.get()
    rc = _lib().kr_adam_step_clipped(count, *[P(b) for b in bufs], every, P(parts), max_norm, lr32, b1, b2, eps, wd32, P(cb), _stream())
    assert rc == 0
    clip = cb.get() if clip_out else None
    assert bufs[4].unchanged() and bufs[1].unchanged() and parts.get().tobytes() == before.tobytes()      # step, grad and the partials are only read
    return bufs[:4], clip


def clipped_adam_bounds(p, g, m, v, step, coef, lr, b1, b2, eps, wd):
    """adam_bounds on the reference's own gradient g c, widened by what the kernel's gradient fl(g c^) carries.  c^ is the float32
    coefficient: (float)total (0.5 U on the norm after the root; the float64 sum's own error is below 1e-3 U), sqrtf (U), + 1e-6f (U; the
    constant's own representation error is relative to 1e-6, far below U of the norm), the division (U) - at most 4 U, rounded up - and the
    product g c^ one more:  |dg0| <= 5 U |g c|.  It enters as a perturbation of the gradient BEFORE the weight-decay term, so by
    adam_bounds' own expressions:  dm += (1 - b1) dg0;  dv += (1 - b2)(2 |g'| dg0 + dg0^2);  and the step carries the widened dm and dv
    exactly as it carries adam_bounds' (the terms (lr / bc1) dm / denom and |D| d(sqrt v') / sqrt(bc2) / denom)."""
    gc = gr.wide(g) * coef
    (p1, m1, v1), (delta, bd, bm, bv) = adam_bounds(p, gc, m, v, step, lr, b1, b2, eps, wd)
    pw = gr.wide(p)
    gi = gc + wd * pw if wd != 0 else gc
    dg0 = 5 * U * np.abs(gc) * SECOND
    bm2 = bm + (1.0 - b1) * dg0 * SECOND
    bv2 = bv + (1.0 - b2) * (2 * np.abs(gi) * dg0 + dg0 * dg0) * SECOND
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    ss, bc2s, sq = lr / bc1, np.sqrt(bc2), np.sqrt(v1)
    denom = sq / bc2s + eps
    dsq = np.minimum(bv2 / np.maximum(sq + np.sqrt(np.maximum(v1 - bv2, 0.0)), 1e-300), np.sqrt(bv2))
    rel = 9 * U + E_POWF * U / bc1 + E_POWF * U / (2 * bc2)
    bd2 = np.abs(delta) * (rel + dsq / bc2s / denom) * SECOND + ss * bm2 / denom * SECOND + ulp32(np.maximum(np.abs(pw), np.abs(p1))) + FLOOR
    assert (bd2 >= bd).all() and (bm2 >= bm).all() and (bv2 >= bv).all()
    return (p1, m1, v1), (delta, bd2, bm2, bv2)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("lr,wd", ADAM_SETS)
def test_adam_step_clipped_within_its_roundings(count, lr, wd):
    """kr_grad_sqnorm + kr_adam_step_clipped at steps 1, 2, 12, 1000 with max_norm = 0.3 x the gradient's norm (coef ~ 0.3): clip_out against
    the three float32 operations on the butterfly total of the partials (norm: U for sqrtf; coef: the norm's U, + 1e-6f, the division),
    the three moved buffers within clipped_adam_bounds of bounded_ref.adam_clipped_ref with the float64 coefficient; grad is not written."""
    r = _rng("clipped", count, lr)
    b1, b2 = BETAS
    lr32, eps, wd32 = float(np.float32(lr)), float(np.float32(1e-8)), float(np.float32(wd))
    p, g, m, v = adam_inputs(count, r)
    if count < 4:
        g = f32(r.standard_normal(count) + 3.0)          # (a norm well above the 1e-6 of the coefficient's denominator)
    parts, pb = run_sqnorm(g)
    sq = br.sqnorm_ref(g)
    max_norm = float(np.float32(0.3 * math.sqrt(sq)))
    coef64 = min(max_norm / (math.sqrt(sq) + 1e-6), 1.0)
    assert 0.25 < coef64 < 0.35
    total = butterfly(parts)
    exact_norm = math.sqrt(float(np.float32(total)))
    exact_coef = max_norm / (exact_norm + float(np.float32(1e-6)))
    for step in (1, 2, 12, 1000):
        (pb_, gb, mb, vb), clip = run_clipped(count, p, g, m, v, step, 1, pb, max_norm, lr, wd)
        assert abs(float(clip[0]) - exact_norm) <= U * exact_norm * SECOND and abs(float(clip[1]) - exact_coef) <= 3 * U * exact_coef * SECOND
        ref = br.adam_clipped_ref(p, g, m, v, step, 1, coef64, lr32, b1, b2, eps, wd32)
        (p1, m1, v1), (delta, bd, bm, bv) = clipped_adam_bounds(p, g, m, v, step, coef64, lr32, b1, b2, eps, wd32)
        assert np.array_equal(ref[0], p1) and np.array_equal(ref[1], m1) and np.array_equal(ref[2], v1)
        case = f"count {count} step {step} lr {lr} wd {wd}"
        check_bound(mb.get(), m1, bm, "kr_adam_step_clipped", case, "exp_avg")
        check_bound(vb.get(), v1, bv, "kr_adam_step_clipped", case, "exp_avg_sq")
        check_bound(gr.wide(pb_.get()) - gr.wide(p), delta, bd, "kr_adam_step_clipped", case, "param step")


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("lr,wd", ADAM_SETS)
def test_adam_step_clipped_with_an_infinite_max_norm_is_adam_step_every(count, lr, wd):
    """max_norm = +inf (coef = 1, the product exact): kr_adam_step_every's four buffers in every bit for every = 1 and 2 at open gates
    (steps 1, 2, 12, 1000 / 2, 24) and closed ones (0 / 0, 1, 3), where nothing but clip_out is written - and clip_out is written there too"""
    r = _rng("clipped-inf", count, lr)
    p, g, m, v = adam_inputs(count, r)
    parts, pb = run_sqnorm(g)
    norm = math.sqrt(float(np.float32(butterfly(parts))))
    for every, steps in ((1, (0, 1, 2, 12, 1000)), (2, (0, 1, 2, 3, 24))):
        for step in steps:
            want = run_adam(count, p, g, m, v, step, every, lr, wd)
            got, clip = run_clipped(count, p, g, m, v, step, every, pb, INF, lr, wd)
            for name, a, b in zip(("param", "grad", "exp_avg", "exp_avg_sq"), got, want):
                assert_bits(a.get(), b.get(), f"every {every}, step {step}: {name}")
            open_gate = step > 0 and step % every == 0
            assert open_gate or all(b.unchanged() for b in got), (every, step)
            assert not open_gate or count < 255 or not got[0].unchanged(), (every, step)
            assert abs(float(clip[0]) - norm) <= U * norm * SECOND and clip[1] == 1.0, (every, step, clip)
    got, clip = run_clipped(count, p, g, m, v, 2, 1, pb, INF, lr, wd, clip_out=False)            # clip_out is optional
    for a, b in zip(got, run_adam(count, p, g, m, v, 2, 1, lr, wd)):
        assert_bits(a.get(), b.get(), "without clip_out")


def test_adam_step_clipped_nan_gradient_reaches_every_parameter():
    """one NaN element: its square makes one partial NaN, the total, norm and coef NaN (a NaN fails coef > 1 and stays), and every
    parameter and moment becomes NaN - what clip_grad_norm_ (error_if_nonfinite=False) and torch.optim.Adam do"""
    count = 4097 + 300
    r = _rng("clipped-nan")
    p, g, m, v = adam_inputs(count, r)
    g[4100] = np.nan
    parts, pb = run_sqnorm(g)
    assert np.isnan(parts).sum() == 1 and np.isnan(parts[(4100 % br.NORM_STRIDE) // 64])
    (pb_, gb, mb, vb), clip = run_clipped(count, p, g, m, v, 3, 1, pb, 10.0, 1e-3, 1e-4)
    assert np.isnan(clip).all() and np.isnan(pb_.get()).all() and np.isnan(mb.get()).all() and np.isnan(vb.get()).all()
    import torch
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy(g.copy())
    opt = torch.optim.Adam([tp], lr=1e-3, weight_decay=1e-4)
    assert torch.isnan(torch.nn.utils.clip_grad_norm_([tp], 10.0))
    opt.step()
    assert torch.isnan(tp).all()


def test_adam_step_clipped_reads_given_partials_lane_by_lane():
    """64 given partials 2^b / 2^40 (their sum is exact in any order): norm and coef are the three float32 operations on that sum in every
    bit - every partial is read once, by its own lane"""
    count = 300
    r = _rng("clipped-given")
    p, g, m, v = adam_inputs(count, r)
    parts = 2.0 ** (np.arange(64) - 40.0)
    pb = Buf(parts)
    total = float(parts.sum())
    assert total == (2.0 ** 64 - 1) / 2.0 ** 40 and butterfly(parts) == total
    _, clip = run_clipped(count, p, g, m, v, 1, 1, pb, 100.0, 1e-3, 0.0)
    norm, coef = br.clip_coef_f32(total, 100.0)
    assert_bits(clip[:1], np.array([norm]), "norm")
    assert abs(float(clip[1]) - float(coef)) <= 2 * U * float(coef) and float(coef) < 1.0


# ---- refusals --------------------------------------------------------------------------------------------------------
def _valid_calls():
    n, ns = 3, 5
    fz = lambda *s: Buf(np.zeros(s, np.float32))
    one = lambda: Buf(np.ones(1, np.float32))
    c = {}
    c["kr_critic_grad_bounded"] = [n, ns, fz(n), fz(n), fz(n), fz(n), fz(n), fz(n), fz(n, ns), fz(n), one(), 0.5, -1.0, 1.0, 2.0, fz(n), fz(n), fz(2 * n), fz(6)]
    c["kr_critic_grad_bounded/single"] = [n, ns, fz(n), None, fz(n), None, fz(n), None, fz(n, ns), None, one(), 0.5, 0.0, 0.0, INF, fz(n), None, fz(2 * n), fz(3)]
    c["kr_grad_sqnorm"] = [n, fz(n), Buf(np.zeros(br.NORM_PARTS, np.float64))]
    c["kr_adam_step_clipped"] = [n, fz(n), fz(n), fz(n), fz(n), Buf(np.ones(1, np.int64)), 1, Buf(np.ones(br.NORM_PARTS, np.float64)), 10.0, 1e-3, 0.9, 0.999,
                                 1e-8, 0.0, fz(2)]
    return c


# optional pointers, and those of the second critic, whose absence one by one is a mixture (below)
OPTIONAL = {"kr_critic_grad_bounded": {3, 5, 7, 9, 16}, "kr_critic_grad_bounded/single": set(), "kr_adam_step_clipped": {14}}


def _refusal_cases():
    cases = []
    for name, args in _valid_calls().items():
        cases += [(name, 0, 0, "count 0"), (name, 0, -1, "count -1")]
        for k, a in enumerate(args):
            if isinstance(a, Buf) and k not in OPTIONAL.get(name, ()):
                cases.append((name, k, None, f"NULL argument {k}"))
    for name in ("kr_critic_grad_bounded", "kr_critic_grad_bounded/single"):
        cases += [(name, 1, 0, "n_steps 0"), (name, 12, NAN, "q_lo NaN"), (name, 13, NAN, "q_hi NaN"), (name, 12, 1.5, "q_lo > q_hi"),
                  (name, 14, 0.0, "huber_delta 0"), (name, 14, -1.0, "huber_delta negative"), (name, 14, NAN, "huber_delta NaN")]
    # a mixture of the two forms: one of the second critic's four pointers missing, or only one of them given
    cases += [("kr_critic_grad_bounded", k, None, f"twin without argument {k}") for k in (3, 5, 7, 16)]
    cases += [("kr_critic_grad_bounded/single", k, "buffer", f"single with argument {k}") for k in (3, 5, 7, 16)]
    cases += [("kr_adam_step_clipped", 6, 0, "every 0"), ("kr_adam_step_clipped", 6, -2, "every -2"), ("kr_adam_step_clipped", 8, 0.0, "max_norm 0"),
              ("kr_adam_step_clipped", 8, -1.0, "max_norm negative"), ("kr_adam_step_clipped", 8, NAN, "max_norm NaN")]
    return cases


REFUSALS = _refusal_cases()


@pytest.mark.parametrize("name,index,value,label", REFUSALS, ids=[f"{c[0].replace('/', '-')}-{c[3].replace(' ', '_')}" for c in REFUSALS])
def test_refusals_return_invalid_and_write_nothing(name, index, value, label):
    """every KS_ERR_INVALID of the three entry points - the return code, and no buffer of the call has changed"""
    args = _valid_calls()[name]
    bufs = [a for a in args if isinstance(a, Buf)]
    if value == "buffer":
        value = Buf(np.zeros(3, np.float32))
        bufs.append(value)
    args[index] = value
    rc = getattr(_lib(), name.split("/")[0])(*[P(a) if isinstance(a, Buf) else a for a in args], _stream())
    assert rc == KS_ERR_INVALID, (name, label, rc)
    assert all(b.unchanged() for b in bufs), (name, label)


def test_the_valid_calls_of_the_refusal_cases_run():
    for name, args in _valid_calls().items():
        assert getattr(_lib(), name.split("/")[0])(*[P(a) if isinstance(a, Buf) else a for a in args], _stream()) == 0, name
    # equal bounds and the optional pointers left out are valid calls too
    args = _valid_calls()["kr_critic_grad_bounded"]
    args[12], args[13], args[9] = 1.0, 1.0, None
    assert _lib().kr_critic_grad_bounded(*[P(a) if isinstance(a, Buf) else a for a in args], _stream()) == 0
    args = _valid_calls()["kr_adam_step_clipped"]
    args[14] = None
    assert _lib().kr_adam_step_clipped(*[P(a) if isinstance(a, Buf) else a for a in args], _stream()) == 0
    import torch
    torch.cuda.synchronize()
