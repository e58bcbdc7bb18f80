"""kr_bc_actor_grad (csrc/ks_rollout.hip; contract: include/kinova_rollout.h) on its own against tests/bc_ref.py, by the method of
tests/test_gpu_glue_kernels.py: every writable buffer between two 0xA5 guard regions, rows the kernel must not store compared bit for bit,
the rest within bounds counted from the header's roundings on the reference's own float64 intermediates (U = 2^-24 per rounding, second
order terms in SECOND, an absolute FLOOR where an fp32 intermediate can be denormal) - nothing in a bound comes from the kernel's output.

The roundings.  With d = pi - demo, dd = pi / m, s1 = 1 - dd, g = 2 c (-dq) d and T = g pi s1 (all exact, float64):
    d'   = fl(pi - demo):                                   |d' - d| <= U |d|
    sq   = four products fl(d' d') (2 U from d', 1 from the product) and three sums of non-negative terms (U of the total each):
                                                            |sq' - sq| <= 6 U sq
    g'   = fl(fl(2 c * -dq) * d'):  three roundings         |g' - g| <= 3 U |g|
    t'   = fl(g' * fl(pi * fl(1 - fl(pi / m)))):  kr_sigmoid_scale_backward's count, U |g pi| (|dd| + 3 |s1|), plus g's own:
                                                            |t' - T| <= U |g pi| (|dd| + 3 |s1|) + 3 U |T|
    dz3' = fl(dz3 + t'):                                    |dz3' - (dz3 + T)| <= |t' - T| + U |dz3 + T|
Printed lines starting with GLUE carry the worst error and worst error / bound per case (profiles/bc_loss.txt is collected from them)."""
import ctypes

import numpy as np
import pytest
import torch

from kinovagrasping_amd import sim as ks
from tests import bc_ref as bc
from tests.test_gpu_glue_kernels import ROWS, Buf, U, check_bound, sent
from tests.test_gpu_glue_kernels import assert_bits as _assert_bits

pytestmark = pytest.mark.gpu

FLOOR = 4 * 2.0 ** -149
SECOND = 1.0 + 1e-5
KS_ERR_INVALID = -1
M = float(np.float32(0.8))
C = float(np.float32(1.7))
N_STEPS = 5
DEV = torch.device("cuda", 0)


def assert_bits(got, ref, what):
    """assert_bits of tests/test_gpu_glue_kernels.py; a selection of no rows has nothing to compare"""
    if np.asarray(got).size or np.asarray(ref).size:
        _assert_bits(got, ref, what)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _rng(*key):
    import zlib
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def P(b, offset=0):
    return None if b is None else b.at(offset)


f32 = lambda x: np.asarray(x, np.float32)


def demo_froms(R):
    return sorted({0, R // 3 + 1 if R > 2 else 0, R})


def inputs(R, r, filt):
    """R rows (states): pi and demo in [0, 0.8] with both ends and rows of d = 0; dq as kr_update_prologue forms it for 0 / 1 weights (exact zeros
    on padding rows); with the filter Q values that hold equal pairs and NaNs on either side"""
    pi = np.minimum(f32(r.rand(R, 4)) * np.float32(0.8), np.float32(0.8))
    pi[::7, 0], pi[3::11, 1] = 0.0, np.float32(0.8)                  # both ends of the sigmoid's range
    demo = np.minimum(f32(r.rand(R, 4)) * np.float32(0.8), np.float32(0.8))
    demo[5::13] = pi[5::13]                                          # d = 0 exactly
    w = f32(r.rand(R) < 0.7)
    w[R - 1] = 1.0
    dq = f32(-w / np.float32(max(w.sum(), 1.0) * N_STEPS))
    q_demo = q_pi = None
    if filt:
        q_demo, q_pi = f32(r.standard_normal(R)), f32(r.standard_normal(R))
        q_pi[2::9] = q_demo[2::9]                                    # equal: the comparison is strict, f = 0
        q_demo[4::17], q_pi[6::19] = np.nan, np.nan                  # a NaN on either side: f = 0
    dz3 = f32(r.standard_normal((R, 4)) * 0.01)
    return pi, demo, q_demo, q_pi, dq, dz3


def bounds(pi, demo, dq, dz3, c, m):
    pi, demo, dq, dz3 = (bc.wide(x) for x in (pi, demo, dq.reshape(-1), dz3))
    d = pi - demo
    dd = pi / m
    g = (2.0 * c * -dq)[:, None] * d
    T = g * pi * (1.0 - dd)
    bt = U * np.abs(g * pi) * (np.abs(dd) + 3 * np.abs(1.0 - dd)) + 3 * U * np.abs(T)
    return (bt + U * np.abs(dz3 + T)) * SECOND + FLOOR, 6 * U * (d * d).sum(1) * SECOND + FLOOR


def run(R, demo_from, pi, demo, q_demo, q_pi, dq, dz3, c=C, m=M):
    b = dict(pi=Buf(pi), demo=Buf(demo), q_demo=None if q_demo is None else Buf(q_demo), q_pi=None if q_pi is None else Buf(q_pi), dq=Buf(dq),
             dz3=Buf(dz3), sq=Buf(sent(R, np.float32)), passed=Buf(sent(R, np.float32)))
    rc = ks.load_library().kr_bc_actor_grad(R, demo_from, P(b["pi"]), P(b["demo"]), P(b["q_demo"]), P(b["q_pi"]), P(b["dq"]), c, m, P(b["dz3"]),
                                            P(b["sq"]), P(b["passed"]), _stream())
    assert rc == 0, rc
    out = {k: b[k].get() for k in ("dz3", "sq", "passed")}
    assert all(b[k] is None or b[k].unchanged() for k in ("pi", "demo", "q_demo", "q_pi", "dq")), "an input was written"
    return out


def plant(dz3, written, r):
    """a -0.0 and a NaN in dz3 rows the kernel must not store"""
    idle = np.flatnonzero(~written)
    for row in idle[::2]:
        dz3[row] = f32([-0.0, np.nan, 1.5, -0.0])
    return idle


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("filt", [False, True], ids=["nofilter", "filter"])
def test_bc_actor_grad_within_its_roundings(R, filt):
    """every demo_from of {0, one that is no multiple of 64, rows}: pass and sq's zeros exact, dz3 and sq within the counted bounds, and the
    rows that receive nothing - below demo_from, f = 0 (q_demo <= q_pi, equal, a NaN on either side), dq = 0 - keep every bit of dz3, the
    -0.0 and the NaN planted there included; demo_from = rows leaves dz3 untouched and zeroes sq and pass; the inputs are unchanged"""
    for demo_from in demo_froms(R):
        assert demo_from in (0, R) or demo_from % 64 != 0
        r = _rng("bc", R, filt, demo_from)
        pi, demo, q_demo, q_pi, dq, dz3 = inputs(R, r, filt)
        _, _, f, written = bc.bc_actor_grad_ref(demo_from, pi, demo, q_demo, q_pi, dq, C, M, dz3)
        idle = plant(dz3, written, r)
        ref, sq, f, written = bc.bc_actor_grad_ref(demo_from, pi, demo, q_demo, q_pi, dq, C, M, dz3)
        got = run(R, demo_from, pi, demo, q_demo, q_pi, dq, dz3)
        case = f"R {R} demo_from {demo_from} filter {int(filt)}"
        assert_bits(got["passed"], f, f"{case}: pass")
        assert_bits(got["sq"][f == 0], np.zeros(int((f == 0).sum())), f"{case}: sq where f = 0")
        assert_bits(got["dz3"][idle], dz3[idle], f"{case}: dz3 rows that receive nothing")
        bz, bs = bounds(pi, demo, dq, np.where(written[:, None], dz3, 0.0), C, M)
        if written.any():
            check_bound(got["dz3"][written], ref[written], bz[written], "kr_bc_actor_grad", case, "dz3")
            assert (got["dz3"][written] != dz3[written]).any()
        if (f == 1).any():
            check_bound(got["sq"][f == 1], sq[f == 1], bs[f == 1], "kr_bc_actor_grad", case, "sq")
        if demo_from == R:
            assert not written.any() and not f.any() and got["dz3"].tobytes() == dz3.tobytes()
            assert_bits(got["sq"], np.zeros(R), "sq with demo_from = rows")
        elif filt and R >= 63:
            assert 0 < f[demo_from:].sum() < R - demo_from          # both outcomes of the filter
        if R >= 63:
            assert idle.size > 0 and (demo_from == R or written.any())


def test_bc_actor_grad_on_a_second_grid_trip():
    """2048 * 256 + 261 rows: the capped grid's first threads take a second trip; filter on, demo_from in the middle of a wave"""
    R = 2048 * 256 + 261
    demo_from = 100003
    r = _rng("bc-large")
    pi, demo, q_demo, q_pi, dq, dz3 = inputs(R, r, True)
    ref, sq, f, written = bc.bc_actor_grad_ref(demo_from, pi, demo, q_demo, q_pi, dq, C, M, dz3)
    got = run(R, demo_from, pi, demo, q_demo, q_pi, dq, dz3)
    assert_bits(got["passed"], f, "pass")
    assert_bits(got["dz3"][~written], dz3[~written], "dz3 rows that receive nothing")
    assert_bits(got["sq"][f == 0], np.zeros(int((f == 0).sum())), "sq where f = 0")
    bz, bs = bounds(pi, demo, dq, dz3, C, M)
    assert written[2048 * 256:].any()
    check_bound(got["dz3"][written], ref[written], bz[written], "kr_bc_actor_grad", f"R {R} demo_from {demo_from} filter 1", "dz3")
    check_bound(got["sq"][f == 1], sq[f == 1], bs[f == 1], "kr_bc_actor_grad", f"R {R} demo_from {demo_from} filter 1", "sq")


@pytest.mark.parametrize("filt", [False, True], ids=["nofilter", "filter"])
def test_a_nan_in_pi_reaches_its_own_row_only(filt):
    """one NaN component of pi in a row with f = 1 and dq != 0: that row's sq and that component of its dz3 are NaN, every other element is
    what it is without the NaN - bit for bit; the same NaN in a row with f = 0 (an agent row) reaches nothing"""
    R, demo_from = 130, 41
    r = _rng("bc-nan", filt)
    pi, demo, q_demo, q_pi, dq, dz3 = inputs(R, r, filt)
    _, _, f, written = bc.bc_actor_grad_ref(demo_from, pi, demo, q_demo, q_pi, dq, C, M, dz3)
    row = int(np.flatnonzero(written)[3])
    clean = run(R, demo_from, pi, demo, q_demo, q_pi, dq, dz3)
    bad = pi.copy()
    bad[row, 2] = np.nan
    bad[7, 1] = np.nan                                              # an agent row
    got = run(R, demo_from, bad, demo, q_demo, q_pi, dq, dz3)
    assert np.isnan(got["sq"][row]) and np.isnan(got["dz3"][row, 2]) and not np.isnan(got["dz3"][row, [0, 1, 3]]).any()
    keep = np.ones((R, 4), bool)
    keep[row, 2] = False
    assert_bits(got["dz3"][keep], clean["dz3"][keep], "dz3 beside the NaN")
    rows = np.arange(R) != row
    assert_bits(got["sq"][rows], clean["sq"][rows], "sq beside the NaN")
    assert_bits(got["passed"], clean["passed"], "pass")


@pytest.mark.parametrize("filt", [False, True], ids=["nofilter", "filter"])
def test_bc_weight_zero_leaves_dz3_untouched(filt):
    R, demo_from = 130, 41
    r = _rng("bc-zero", filt)
    pi, demo, q_demo, q_pi, dq, dz3 = inputs(R, r, filt)
    dz3[demo_from + 1::3] = f32([-0.0, np.nan, 1.5, -0.0])
    _, sq, f, written = bc.bc_actor_grad_ref(demo_from, pi, demo, q_demo, q_pi, dq, 0.0, M, dz3)
    assert not written.any()
    got = run(R, demo_from, pi, demo, q_demo, q_pi, dq, dz3, c=0.0)
    assert got["dz3"].tobytes() == dz3.tobytes()
    assert_bits(got["passed"], f, "pass")
    check_bound(got["sq"], sq, bounds(pi, demo, dq, dz3, 0.0, M)[1], "kr_bc_actor_grad", f"bc_weight 0 filter {int(filt)}", "sq")


def _valid():
    R = 6
    fz = lambda *s: Buf(np.zeros(s, np.float32))
    # (the [rows, 4] buffers have a spare row, so that a pointer 4 bytes in still has its rows behind it)
    return [R, 2, fz(R + 1, 4), fz(R + 1, 4), fz(R), fz(R), Buf(np.full(R, -0.1, np.float32)), 1.0, M, fz(R + 1, 4), Buf(sent(R, np.float32)),
            Buf(sent(R, np.float32))]


NAN = float("nan")
REFUSALS = [("rows 0", {0: 0}), ("rows -1", {0: -1}), ("demo_from -1", {1: -1}), ("demo_from rows + 1", {1: 7})] + \
           [(f"NULL {name}", {k: None}) for k, name in ((2, "pi"), (3, "demo"), (6, "dq"), (9, "dz3"), (10, "sq"), (11, "pass"))] + \
           [(f"misaligned {name}", {k: 4}) for k, name in ((2, "pi"), (3, "demo"), (9, "dz3"))] + \
           [("q_demo without q_pi", {5: None}), ("q_pi without q_demo", {4: None}), ("bc_weight -1", {7: -1.0}), ("bc_weight NaN", {7: NAN}),
            ("max_action 0", {8: 0.0}), ("max_action -1", {8: -1.0}), ("max_action NaN", {8: NAN})]


@pytest.mark.parametrize("label,change", REFUSALS, ids=[c[0].replace(" ", "_") for c in REFUSALS])
def test_refusals_return_invalid_and_write_nothing(label, change):
    args = _valid()
    bufs = [a for a in args if isinstance(a, Buf)]
    conv = []
    for k, a in enumerate(args):
        if k in change and label.startswith("misaligned"):
            conv.append(P(a, change[k]))
        elif k in change:
            conv.append(change[k])
        else:
            conv.append(P(a) if isinstance(a, Buf) else a)
    assert ks.load_library().kr_bc_actor_grad(*conv, _stream()) == KS_ERR_INVALID, label
    assert all(b.unchanged() for b in bufs), label


def test_the_valid_call_of_the_refusal_cases_runs():
    args = _valid()
    assert ks.load_library().kr_bc_actor_grad(*[P(a) if isinstance(a, Buf) else a for a in args], _stream()) == 0
    assert_bits(args[11].get(), f32([0, 0, 0, 0, 0, 0]), "pass: q_demo = q_pi everywhere")
    assert args[9].unchanged()
