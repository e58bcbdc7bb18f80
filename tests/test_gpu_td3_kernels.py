"""The three TD3fD kernels of csrc/ks_rollout.hip (kr_target_smooth, kr_twin_critic_grad, kr_adam_step_every) on their own against
the references of tests/td3_ref.py (which tests/test_td3_reference_cpu.py checks on the host), by the method of
tests/test_gpu_glue_kernels.py, whose buffers, bounds and inputs are used here: 0xA5 guards around every writable buffer, U = 2^-24
per rounding of the header's expression, nothing in a bound taken from the kernel's output, an exact case beside each bounded one.
Printed lines starting with GLUE / TD3 carry the measured worst errors (profiles/td3fd.txt is collected from them)."""
import numpy as np
import pytest

from tests import glue_ref as gr
from tests import philox_ref
from tests import td3_ref as tr
from tests.test_gpu_glue_kernels import (ADAM_SETS, BETAS, COUNTS, KS_ERR_INVALID, ROWS, SECOND, U, Buf, P, _lib, _rng, _stream, adam_inputs,
                                         assert_bits, check_bound, critic_bounds, critic_inputs, f32, is_f32, sent, weights_for)

pytestmark = pytest.mark.gpu

NOISE_TOL = 6e-6          # tests/test_gpu_actor_versions.py: the same __logf / __sincosf / Box-Muller code


# ---- kr_target_smooth ------------------------------------------------------------------------------------------------
SMOOTH_SETS = [(0.08, 0.2, 0.8), (0.125, 0.25, 1.0), (0.0, 0.2, 0.8), (0.08, 0.0, 0.8)]       # (sigma, clip, max_action); the second is dyadic


def smooth_inputs(rows, sigma, clip, max_action, r):
    """actions over [0, max_action] with both ends, noise that lands below, inside and above the clip and on both its edges, sums below 0,
    inside, above max_action and on both ends, NaN in either input"""
    f = np.float32
    a = f32(r.rand(rows, 4) * max_action)
    z = f32(r.standard_normal((rows, 4)) * (3.0 if sigma == 0 else 1.5 * clip / sigma + 0.5))
    edge = f(clip) / f(sigma) if sigma > 0 else f(1.0)
    pick = r.rand(rows, 4)
    a[pick < 0.10], a[(pick >= 0.10) & (pick < 0.20)] = 0.0, f(max_action)
    z[(pick >= 0.15) & (pick < 0.25)] = 0.0                          # the sum on an end exactly (with the ends above)
    z[(pick >= 0.25) & (pick < 0.30)], z[(pick >= 0.30) & (pick < 0.35)] = edge, -edge
    a[(pick >= 0.35) & (pick < 0.40)], z[(pick >= 0.35) & (pick < 0.40)] = f(clip), -edge * 2        # clip - clip: the lower end from above
    a[(pick >= 0.40) & (pick < 0.43)] = np.nan
    z[(pick >= 0.42) & (pick < 0.45)] = np.nan
    z[(pick >= 0.45) & (pick < 0.47)] = np.inf
    return a, z


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 3200])
@pytest.mark.parametrize("sigma,clip,max_action", SMOOTH_SETS)
def test_target_smooth_with_given_noise_is_the_float32_rule_in_every_bit(rows, sigma, clip, max_action):
    """two roundings (sigma z, action + e) and two exact clamps: the kernel's output is td3_ref.target_smooth_f32, NaN where either input
    is NaN; the noise is not written"""
    r = _rng("smooth", rows, sigma, clip)
    s32, c32, m32 = (float(np.float32(x)) for x in (sigma, clip, max_action))
    a, z = smooth_inputs(rows, s32, c32, m32, r)
    ab, zb = Buf(a), Buf(z)
    assert _lib().kr_target_smooth(rows, P(ab), P(zb), 0, None, s32, c32, m32, _stream()) == 0
    ref = tr.target_smooth_f32(a, z, s32, c32, m32)
    got = ab.get()
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(a) | np.isnan(z) | (np.isinf(z) & (s32 == 0))) and np.array_equal(np.isnan(got), nan)
    assert_bits(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), ref), "smoothed action")
    assert zb.unchanged()
    if rows >= 255:
        fin = ref[~nan]
        assert (fin == 0).any() and (fin == np.float32(m32)).any() and ((fin > 0) & (fin < np.float32(m32))).any()
        with np.errstate(invalid="ignore"):
            e = np.float32(s32) * z
        assert s32 == 0 or ((e < -c32).any() and (e > c32).any())
        # on both edges of the clip exactly: where fl(sigma z) can be the clip (the dyadic set; 0.08 z steps over 0.2)
        assert (sigma, clip) != (0.125, 0.25) or ((e == np.float32(c32)).any() and (e == -np.float32(c32)).any())
    wide = tr.target_smooth_ref(a, z, s32, c32, m32)
    assert np.abs(wide[~nan] - gr.wide(ref[~nan])).max() <= 2 * U * (m32 + c32)       # the float32 rule against the float64 one


def _drawn(rows, seed, draw, sigma, base):
    a = np.full((rows, 4), base, np.float32)
    ab, db = Buf(a), Buf(np.array([draw], np.uint64).view(np.int64))
    assert _lib().kr_target_smooth(rows, P(ab), None, seed, P(db), sigma, 0.2, 0.8, _stream()) == 0
    assert db.unchanged()
    return ab.get()


def test_target_smooth_in_kernel_noise_equals_the_tagged_fp64_reference():
    """rows clear of both clamps (action 0.4, sigma 0.03: |e| < 0.2 for every draw the generator can make): the implied draw
    (out - in) / sigma against td3_ref.normal4_tagged within NOISE_TOL + the two roundings U |sigma z| and U |in + sigma z|, over sigma.
    Seeds and counters that differ in their high words only give their own streams; the same call twice the same bits; the next counter
    and the exploration noise of the same (seed, step, row) other draws."""
    rows, base = 3203, np.float32(0.4)
    sigma = float(np.float32(0.03))
    rid = np.arange(rows, dtype=np.uint64)
    worst, outs = 0.0, {}
    for seed in (0x9E3779B97F4A7C15, 0x9E3779B97F4A7C15 ^ (1 << 40)):
        for draw in (7, 7 + (1 << 32), 8):
            out = _drawn(rows, seed, draw, sigma, base)
            outs[seed, draw] = out
            ref = tr.normal4_tagged(np.uint64(seed), np.uint64(draw), rid, tr.TAG_TARGET_SMOOTH)
            assert np.abs(sigma * ref).max() < 0.19
            implied = (gr.wide(out) - float(base)) / sigma
            tol = NOISE_TOL + (U * np.abs(sigma * ref) + U * np.abs(float(base) + sigma * ref)) / sigma * SECOND
            err = np.abs(implied - ref)
            worst = max(worst, float(err.max()))
            assert (err <= tol).all(), (hex(seed), hex(draw), float(err.max()), float(tol.max()))
            explore = philox_ref.normal4(np.uint64(seed), np.uint64(draw), rid)
            assert (np.abs(implied - explore) > 1e-3).mean() > 0.99               # not the exploration noise's stream
    print(f"\nTD3 kr_target_smooth in-kernel noise vs fp64 tagged reference: max |z - z_ref| = {worst:.3e} over {6 * rows * 4} draws "
          f"(tolerance {NOISE_TOL:.0e} + two roundings)")
    keys = list(outs)
    for i, k in enumerate(keys):
        for j in keys[i + 1:]:
            assert not np.array_equal(outs[k], outs[j]), (k, j)
    again = _drawn(rows, keys[0][0], keys[0][1], sigma, base)
    assert_bits(again, outs[keys[0]], "the same (seed, draw) twice")
    z = (gr.wide(np.concatenate([o.reshape(-1) for o in outs.values()])) - float(base)) / sigma
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02


# ---- kr_twin_critic_grad ---------------------------------------------------------------------------------------------
def twin_inputs(R, n, r):
    q1, ta1, tan, rw = critic_inputs(R, n, r)
    q2, tb1, tbn, _ = critic_inputs(R, n, r)
    return q1, q2, ta1, tb1, tan, tbn, rw


def run_twin(R, n, q1, q2, ta1, tb1, tan, tbn, rw, wb, ws, disc):
    dq1, dq2, tmin, ls = Buf(sent(R, np.float32)), Buf(sent(R, np.float32)), Buf(sent(2 * R, np.float32)), Buf(sent(6, np.float32))
    ins = [Buf(x) for x in (q1, q2, ta1, tb1, tan, tbn, rw)]
    assert _lib().kr_twin_critic_grad(R, n, *[P(b) for b in ins], P(wb), P(ws), disc, P(dq1), P(dq2), P(tmin), P(ls), _stream()) == 0
    out = dq1.get(), dq2.get(), tmin.get(), ls.get()
    assert all(b.unchanged() for b in ins)
    return out


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("kind", ["01", "null", "zero"])
def test_twin_critic_grad_within_its_roundings(R, n, kind):
    """wsum from kr_update_prologue's launch on the same weights.  tmin is the reference's minimum in every bit; from it, dq_k and the
    loss triple of critic k carry kr_critic_grad's roundings (test_critic_grad_within_its_roundings: the bounds of critic_bounds on
    (q_k, m1, mn)); losses[0] = fl(losses[1] + fl(0.5 losses[2])) and likewise for 3..5 in every bit."""
    r = _rng("twin", R, n, kind)
    disc = float(np.float32(0.995))
    q1, q2, ta1, tb1, tan, tbn, rw = twin_inputs(R, n, r)
    w = weights_for(kind, R, r)
    wb = None if w is None else Buf(w)
    ws = Buf(sent(1, np.float32))
    assert _lib().kr_update_prologue(R, n, P(wb), P(ws), P(Buf(sent(R * n, np.float32))), P(Buf(np.zeros(1, np.int64))), P(Buf(np.zeros(1, np.int64))), 0,
                                     _stream()) == 0
    wsum = gr.prologue_ref(R, n, w, 0, 0, 0)[0]
    assert_bits(ws.get(), np.array([wsum]), "weight_sum")
    dq1, dq2, tmin, ls = run_twin(R, n, q1, q2, ta1, tb1, tan, tbn, rw, wb, ws, disc)
    r1, r2, rmin, rls = tr.twin_critic_grad_ref(q1, q2, ta1, tb1, tan, tbn, rw, w, wsum, disc)
    assert_bits(tmin, rmin, "tmin")
    assert R < 64 or ((ta1 < tb1).any() and (tb1 < ta1).any())
    case = f"R {R} n {n} weights {kind}"
    for k, (q, dq, rdq) in enumerate(((q1, dq1, r1), (q2, dq2, r2))):
        bdq, bls = critic_bounds(q, rmin[:R], rmin[R:], rw, w, wsum, disc)
        check_bound(dq, rdq, bdq, "kr_twin_critic_grad", case, f"dq{k + 1}")
        check_bound(ls[3 * k:3 * k + 3], np.array(rls[3 * k:3 * k + 3]), np.array(bls), "kr_twin_critic_grad", case, f"losses of critic {k + 1}")
        assert_bits(ls[3 * k:3 * k + 1], np.array([ls[3 * k + 1] + np.float32(0.5) * ls[3 * k + 2]], np.float32), "loss = L1 + 0.5 LN")
    if kind == "zero":
        assert not dq1.any() and not dq2.any() and not ls.any()


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("kind", ["01", "null"])
def test_twin_critic_grad_zero_weight_sum_nan_and_degenerate_case(R, n, kind):
    """wsum = 0 handed in: dq and the six losses are 0, tmin is written all the same.  A NaN in one target: NaN in that row's tmin and
    both dq, the other rows as without it.  q2 = q1, tq1_b = tq1_a, tqn_b = tqn_a: both halves are kr_critic_grad's output on the same
    buffers in every bit."""
    r = _rng("twin0", R, n, kind)
    disc = float(np.float32(0.995))
    q1, q2, ta1, tb1, tan, tbn, rw = twin_inputs(R, n, r)
    w = weights_for(kind, R, r)
    wb = None if w is None else Buf(w)
    dq1, dq2, tmin, ls = run_twin(R, n, q1, q2, ta1, tb1, tan, tbn, rw, wb, Buf(np.zeros(1, np.float32)), disc)
    assert not dq1.any() and not dq2.any() and not ls.any()
    assert_bits(tmin, np.concatenate([np.minimum(ta1, tb1), np.minimum(tan, tbn)]), "tmin with wsum 0")
    # NaN
    wsum = gr.prologue_ref(R, n, w, 0, 0, 0)[0]
    ws = Buf(np.array([wsum], np.float32))
    clean = run_twin(R, n, q1, q2, ta1, tb1, tan, tbn, rw, wb, ws, disc)
    i, j = 0, R - 1
    ta1n, tbnn = ta1.copy(), tbn.copy()
    ta1n[i], tbnn[j] = np.nan, np.nan
    d1, d2, tm, _ = run_twin(R, n, q1, q2, ta1n, tb1, tan, tbnn, rw, wb, ws, disc)
    bad = np.zeros(R, bool)
    bad[[i, j]] = True
    assert np.isnan(tm[i]) and np.isnan(tm[R + j]) and np.isnan(d1[bad]).all() and np.isnan(d2[bad]).all()
    keep = np.ones(2 * R, bool)
    keep[[i, R + j]] = False
    if R > 1:                                      # (R = 1: its only row holds both NaNs)
        assert_bits(tm[keep], clean[2][keep], "tmin of the other rows")
        assert_bits(d1[~bad], clean[0][~bad], "dq1 of the other rows")
        assert_bits(d2[~bad], clean[1][~bad], "dq2 of the other rows")
    # degenerate
    d1, d2, tm, l6 = run_twin(R, n, q1, q1, ta1, ta1, tan, tan, rw, wb, ws, disc)
    dq, l3 = Buf(sent(R, np.float32)), Buf(sent(3, np.float32))
    assert _lib().kr_critic_grad(R, n, P(Buf(q1)), P(Buf(ta1)), P(Buf(tan)), P(Buf(rw)), P(wb), P(ws), disc, P(dq), P(l3), _stream()) == 0
    assert_bits(d1, dq.get(), "dq1 = kr_critic_grad's dq")
    assert_bits(d2, dq.get(), "dq2 = kr_critic_grad's dq")
    assert_bits(l6, np.concatenate([l3.get(), l3.get()]), "both loss triples = kr_critic_grad's")
    assert_bits(tm, np.concatenate([ta1, tan]), "tmin of equal targets")


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("n", [1, 5])
def test_twin_critic_grad_exact_on_dyadic_inputs(R, n):
    """discount 0.5, values in {-1, 0, 1}, a power-of-two count of 0 / 1 weights (test_critic_grad_exact_on_dyadic_inputs' case for two
    critics): every output is the reference in every bit"""
    r = _rng("twinx", R, n)
    tri = lambda *s: f32(r.randint(-1, 2, s))
    q1, q2, ta1, tb1, tan, tbn, rw = tri(R), tri(R), tri(R), tri(R), tri(R), tri(R), tri(R, n)
    ones = 1 << (R.bit_length() - 1)
    w = np.zeros(R, np.float32)
    w[r.permutation(R)[:ones]] = 1.0
    wsum = float(ones)
    r1, r2, rmin, rls = tr.twin_critic_grad_ref(q1, q2, ta1, tb1, tan, tbn, rw, w, wsum, 0.5)
    t1, tn = gr.critic_targets(rmin[:R], rmin[R:], rw, 0.5)
    for q in (q1, q2):
        e1, en = gr.wide(q) - t1, gr.wide(q) - tn
        assert is_f32(e1 * e1) and is_f32(en * en) and max((e1 * e1).sum(), (en * en).sum()) * 4.0 ** n < 2.0 ** 24
    assert is_f32(r1) and is_f32(r2) and is_f32(np.array(rls))
    dq1, dq2, tmin, ls = run_twin(R, n, q1, q2, ta1, tb1, tan, tbn, rw, Buf(w), Buf(np.array([wsum], np.float32)), 0.5)
    assert_bits(dq1, r1, "dq1 on dyadic inputs")
    assert_bits(dq2, r2, "dq2 on dyadic inputs")
    assert_bits(tmin, rmin, "tmin on dyadic inputs")
    assert_bits(ls, np.array(rls), "losses on dyadic inputs")


# ---- kr_adam_step_every ----------------------------------------------------------------------------------------------
def run_adam(count, p, g, m, v, step, every, lr, wd):
    b1, b2 = BETAS
    lr32, eps, wd32 = float(np.float32(lr)), float(np.float32(1e-8)), float(np.float32(wd))
    bufs = [Buf(x) for x in (p, g, m, v)] + [Buf(np.array([step], np.int64))]
    if every is None:
        rc = _lib().kr_adam_step(count, *[P(b) for b in bufs], lr32, b1, b2, eps, wd32, _stream())
    else:
        rc = _lib().kr_adam_step_every(count, *[P(b) for b in bufs], every, lr32, b1, b2, eps, wd32, _stream())
    assert rc == 0 and bufs[4].unchanged()
    return bufs[:4]


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("lr,wd", ADAM_SETS)
def test_adam_step_every_is_adam_step_on_its_steps_and_nothing_between(count, lr, wd):
    """every = 1: kr_adam_step's four buffers in every bit at steps 1, 2, 12, 1000 (kr_adam_step itself is held to its roundings by
    tests/test_gpu_glue_kernels.py).  every = 2: steps 0, 1 and 3 leave the four buffers untouched, steps 2 and 24 are kr_adam_step at
    steps 1 and 12."""
    r = _rng("every", count, lr)
    p, g, m, v = adam_inputs(count, r)
    plain = {}
    for step in (1, 2, 12, 1000):
        plain[step] = [b.get() for b in run_adam(count, p, g, m, v, step, None, lr, wd)]
        got = run_adam(count, p, g, m, v, step, 1, lr, wd)
        for name, a, b in zip(("param", "grad", "exp_avg", "exp_avg_sq"), got, plain[step]):
            assert_bits(a.get(), b, f"every 1, step {step}: {name}")
        assert not np.array_equal(plain[step][0], p) and got[1].unchanged()
    for step in (0, 1, 3):
        assert all(b.unchanged() for b in run_adam(count, p, g, m, v, step, 2, lr, wd)), step
    for step, t in ((2, 1), (24, 12)):
        got = run_adam(count, p, g, m, v, step, 2, lr, wd)
        for name, a, b in zip(("param", "grad", "exp_avg", "exp_avg_sq"), got, plain[t]):
            assert_bits(a.get(), b, f"every 2, step {step}: {name}")


# ---- refusals --------------------------------------------------------------------------------------------------------
def _valid_calls():
    n, ns = 3, 5
    fz = lambda *s: Buf(np.zeros(s, np.float32))
    c = {}
    c["kr_target_smooth"] = [n, fz(n, 4), fz(n, 4), 5, None, 0.08, 0.2, 0.8]
    c["kr_twin_critic_grad"] = [n, ns, fz(n), fz(n), fz(n), fz(n), fz(n), fz(n), fz(n, ns), fz(n), Buf(np.ones(1, np.float32)), 0.5, fz(n), fz(n), fz(2 * n),
                                fz(6)]
    c["kr_adam_step_every"] = [n, fz(n), fz(n), fz(n), fz(n), Buf(np.ones(1, np.int64)), 1, 1e-3, 0.9, 0.999, 1e-8, 0.0]
    return c


OPTIONAL = {"kr_twin_critic_grad": {9}, "kr_target_smooth": {2}}        # (kr_target_smooth's noise: its own cases below)
NAN = float("nan")


def _refusal_cases():
    cases = []
    for name, args in _valid_calls().items():
        cases += [(name, 0, 0, "count 0"), (name, 0, -1, "count -1")]
        for k, a in enumerate(args):
            if isinstance(a, Buf) and k not in OPTIONAL.get(name, ()):
                cases.append((name, k, None, f"NULL argument {k}"))
    cases += [("kr_twin_critic_grad", 1, 0, "n_steps 0"), ("kr_adam_step_every", 6, 0, "every 0"), ("kr_adam_step_every", 6, -2, "every -2"),
              ("kr_target_smooth", 2, None, "neither noise nor draw"), ("kr_target_smooth", 4, "draw", "both noise and draw"),
              ("kr_target_smooth", 1, "misaligned", "misaligned action"), ("kr_target_smooth", 2, "misaligned", "misaligned noise"),
              ("kr_target_smooth", 5, -0.1, "sigma negative"), ("kr_target_smooth", 5, NAN, "sigma NaN"), ("kr_target_smooth", 6, -0.1, "clip negative"),
              ("kr_target_smooth", 6, NAN, "clip NaN"), ("kr_target_smooth", 7, 0.0, "max_action 0"), ("kr_target_smooth", 7, -0.8, "max_action negative"),
              ("kr_target_smooth", 7, NAN, "max_action NaN")]
    return cases


REFUSALS = _refusal_cases()


@pytest.mark.parametrize("name,index,value,label", REFUSALS, ids=[f"{c[0]}-{c[3].replace(' ', '_')}" for c in REFUSALS])
def test_refusals_return_invalid_and_write_nothing(name, index, value, label):
    """every KS_ERR_INVALID of the three entry points - the return code, and no buffer of the call has changed"""
    args = _valid_calls()[name]
    bufs = [a for a in args if isinstance(a, Buf)]
    conv = [P(a) if isinstance(a, Buf) else a for a in args]
    if value == "draw":
        bufs.append(Buf(np.ones(1, np.int64)))
        conv[index] = P(bufs[-1])
    elif value == "misaligned":
        conv[index] = P(args[index], 4)
    else:
        conv[index] = value
    rc = getattr(_lib(), name)(*conv, _stream())
    assert rc == KS_ERR_INVALID, (name, label, rc)
    assert all(b.unchanged() for b in bufs), (name, label)


def test_the_valid_calls_of_the_refusal_cases_run():
    for name, args in _valid_calls().items():
        assert getattr(_lib(), name)(*[P(a) if isinstance(a, Buf) else a for a in args], _stream()) == 0, name
