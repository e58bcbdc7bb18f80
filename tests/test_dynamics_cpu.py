"""The aimed contact-free states of tests/dynamics_states.py, without a GPU: what the sets must offer (from the oracle and the blob alone), the
oracle's own outputs against the bound's ingredients, and the host lane of the kernel source (tests/native_build.Lane: one lane, fp64 and fp32)
against the bounds of tests/dynamics_ref.py.  tests/test_gpu_dynamics.py holds the compiled gfx950 kernels to the same bounds.
Run with -s for the table (recorded in profiles/dynamics_parity.txt)."""
import numpy as np
import pytest

from kinovagrasping_amd import scenarios
from tests import dynamics_ref as dr, dynamics_states as ds
from tests.native_build import Lane

CASES = ds.cases()
case_id = lambda v: str(v)
SHARE_FACTOR, SHARE_CAP = 100.0, 0.90
AIMED_CLASSES = ("free_flight", "finger_swing", "tendon", "actuator") + ds.LIMIT_CLASSES


@pytest.mark.parametrize("cls,shape", CASES, ids=case_id)
def test_states_offer_what_their_class_names(cls, shape):
    s = ds.states(cls, shape)
    n = len(s.tag)
    assert 100 <= n <= 300, (cls, shape, n)
    for a in (s.qpos, s.qvel, s.warm, s.ctrl, s.action, s.hq, s.mass):
        assert np.isfinite(a).all() and np.array_equal(a, ds.f32(a)), "every input is an fp32 number"
    refs = dr.reference(s)
    assert all(r.ncon == 0 for r in refs), "a contact"
    assert (s.clear[:, 0] >= ds.CLEAR).all() and (s.clear[:, 1] >= ds.OBJECT_AWAY).all(), "the generator's certificate (ds.clearance)"
    for i in range(0, n, 17):                                 # and once more from the stored state
        ncon, clear, obj = ds.clearance(shape, s.hq[:, i], s.qpos[:, i])
        assert ncon == 0 and (clear, obj) == tuple(s.clear[i]), (cls, i, ncon, clear, obj)
    assert all(r.converged and r.iters < ds.SOLVER_ITERATIONS for r in refs), "the oracle's Newton cap"
    c = dr.conditions(s)
    print(f"{cls:13s} {shape:8s} states {n:3d} dropped {c['dropped']:.3f} draws set aside {c['redrawn'][0]} + {c['redrawn'][1]} undecidable {c['undecidable']:.3f} aimed {c['aimed']:3d} ({c['aimed'] / n:.2f} of the class) "
          f"carrying the term at {SHARE_FACTOR:.0f} x the fp32 bound {c['carried']:.3f} (median {c['median']:.3g} x)")
    assert c["dropped"] <= ds.DROP_CAP and c["undecidable"] <= ds.UNDECIDABLE_CAP
    if cls in AIMED_CLASSES:
        assert c["aimed"] >= (20 if cls == "actuator" else 30) and c["carried"] >= SHARE_CAP, c


def test_every_limit_is_met_active_and_absent():
    """each limited joint, each end (but the hinges' upper end): states with the row active (the oracle's efc_force != 0), states beyond the range whose row carries no force,
    and states inside the range; every regime of impedance() on a limit row and on a tendon row"""
    M = ds.model(ds.HAND_SHAPE)
    width = ds.constants(M)["width"]
    seen = {}
    for cls in ("limits_slide", "limits_hinge"):
        s = ds.states(cls)
        for i, ref in enumerate(dr.reference(s)):
            (j, side, depth, vel), = s.tag[i][s.tag[i].index("limit") + 1]
            rows = ref.efc_type == 1
            assert rows.sum() == (depth > 0), (cls, i, "a limit row exactly where the joint is beyond its range")
            kind = "inside" if depth < 0 else ("active" if ref.efc_force[rows][0] != 0 else "idle")
            x = depth / width
            regime = 0 if x <= 0.5 else (1 if x < 1 else 2)
            seen.setdefault((j, side), set()).add((kind, regime if kind == "active" else -1))
            if rows.any():
                assert np.sign(ref.efc_J[rows][0][ds.LIMIT_DOF[j]]) == (1 if side == 0 else -1)
    for j in range(6):
        for side in (0, 1):
            got = seen[j, side]
            if j >= 3 and side == 1:
                # the upper end of a hinge is contact-free only with the tendon 3 rad off its rest (dynamics_states.UPPER_DISTAL), which pulls the
                # joint back with 7900 rad/s^2: the row is there and never carries force.  `sign = -1` carries force on the slides' upper ends.
                assert {("inside", -1), ("idle", -1)} <= got, (j, side, got)
                continue
            assert {("inside", -1), ("active", 0), ("active", 1), ("active", 2)} <= got, (j, side, got)
    assert any(("idle", -1) in g for g in seen.values())
    s = ds.states("tendon")
    x = np.array([abs(t[t.index("x") + 1]) for t in s.tag])
    assert (x <= 0.5).sum() >= 30 and ((x > 0.5) & (x < 1)).sum() >= 30 and (x >= 1).sum() >= 30
    multi = [len(t[t.index("limit") + 1]) for t in ds.states("limits_multi").tag]
    assert multi.count(2) >= 30 and multi.count(3) >= 30 and sum(1 for t in ds.states("limits_multi").tag if "x" in t) >= 30


def test_actuator_states_cross_every_clamp():
    s = ds.states("actuator")
    clamp = ds.act_clamps(ds.model(ds.HAND_SHAPE))
    for k in range(9):
        v = np.array([s.ctrl[k, i] for i, t in enumerate(s.tag) if t[t.index("ctrl") + 1] == k]) / clamp[k]
        for m in ds.ACT_MULTIPLES:
            assert np.isclose(v, m, atol=1e-6).any(), (k, m)
        one = np.float32(clamp[k])
        inside, outside = float(np.nextafter(one, np.float32(0))) / clamp[k], float(np.nextafter(one, np.float32(9))) / clamp[k]
        assert {inside, outside, -inside, -outside} <= set(v.tolist()), (k, "one fp32 step inside and outside either clamp")
    assert ((np.abs(s.ctrl[1:6:2]) > 0.05).sum(0) >= 2).all(), "feed-forward controls non-zero (but the one under test at 0 x)"


def test_warm_starts_are_what_they_are_named():
    s = ds.states("warm_start")
    refs = dr.reference(s)
    kinds = [t[t.index("warm") + 1] for t in s.tag]
    assert all(kinds.count(k) >= 60 for k in ds.WARM_KINDS)
    for i in range(0, len(kinds), 4):                       # the four starts of one state: one solution
        assert kinds[i:i + 4] == list(ds.WARM_KINDS)
        a = refs[i].qacc
        assert np.abs(s.warm[:, i + 1]).max() == 0 and np.abs(s.warm[:, i + 3]).max() >= 50 * np.abs(a).max()
        for r in refs[i + 1:i + 4]:
            assert np.abs(r.qacc - a).max() <= 1e-9 * (1 + np.abs(a).max()), (i, "the oracle's solution depends on its start")


@pytest.mark.parametrize("cls,shape", CASES, ids=case_id)
def test_oracle_solution_solves_the_system_of_its_active_set(cls, shape):
    """H a = rhs on the active set the oracle reports: what ties the bound's ingredients (M, efc_J, efc_R, efc_aref, the forces) to its outputs;
    and its Euler step from those ingredients"""
    s = ds.states(cls, shape)
    worst = 0.0
    for mode in ("substep", "step") if cls != "actuator" else ("substep",):
        for i, ref in enumerate(dr.reference(s, mode)):
            res, scale = dr.newton_residual(ref)
            worst = max(worst, res / scale)
            assert res <= 1e-12 * scale, (cls, mode, i, res, scale)
            Md = ref.M + ref.h * np.diag(ref.damping)
            qa = np.linalg.solve(Md, ref.passive - ref.bias + ref.actuator + ref.efc_J.T @ ref.efc_force)
            assert np.abs(s.qvel[:, i] + ref.h * qa - ref.qvel).max() <= 1e-12 * (1 + np.abs(ref.qvel).max()), (cls, mode, i)
    print(f"{cls:13s} {shape:8s} worst |H a - rhs| / scale {worst:.2g}")


_lanes = {}


def lane(shape, precision):
    if (shape, precision) not in _lanes:
        _lanes[shape, precision] = Lane(scenarios.model_blob(shape), precision, multi_geom=shape == ds.MG_SHAPE)
    return _lanes[shape, precision]


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("cls,shape", CASES, ids=case_id)
def test_host_lane_meets_the_bounds(cls, shape, precision):
    s = ds.states(cls, shape)
    T = dr.Tally(s, "substep", precision, f"host lane fp{precision}")
    L = lane(shape, precision)
    for i in range(len(s.tag)):
        q, v, w, ncon, _, status = L.substep(s.qpos[:, i], s.qvel[:, i], s.warm[:, i], s.ctrl[:, i], s.hq[:, i], obj_mass=s.mass[i])
        T.add(i, dict(qpos=q, qvel=v, warm=w), ncon, status)
    print(T.line())
    T.check()
