"""The plane-pair contacts without a GPU: the numpy reference of tests/plane_ref.py against the oracle's C records on the aimed poses of
tests/plane_poses.py (which ties the reference's vertex indices to the oracle), the generator's conditions from oracle and reference alone, and the
host lane of the kernel source (tests/native/ks_lanecheck.cpp: Team<1>, the serial fallbacks of the scans and of the merge), fp64 and fp32, under the
assertions tests/test_gpu_plane_contacts.py makes of the compiled gfx950 kernels (plane_poses.Tally).
Run with -s for the table."""
import numpy as np
import pytest

from kinovagrasping_amd import scenarios
from tests import contact_poses as cp, plane_poses as pp, plane_ref as pr
from tests.native_build import Lane

CASES = [(s, c) for s in pp.SHAPES for c in pp.classes(s)]
ZERO15, ZERO9 = np.zeros(15), np.zeros(9)
_lanes = {}


def lane(shape, precision):
    if (shape, precision) not in _lanes:
        _lanes[shape, precision] = Lane(scenarios.model_blob(shape), precision, multi_geom=cp.on_mg_library(shape))
    return _lanes[shape, precision]


@pytest.mark.parametrize("shape,cls", CASES)
def test_pose_sets_meet_the_generators_conditions(shape, cls):
    ps = pp.poses(shape, cls)
    sd = 1 - np.mean([d for per in ps.set_decidable for d in per.values()])
    print(f"{shape:10s} {cls:11s} poses {len(ps.expected):4d} plane pairs undecidable {pp.undecidable_share(ps):.3f} set-undecidable {sd:.3f} "
          f"largest expected list {int(ps.total.max()):3d} poses beyond the capacity {int((ps.dropped > 0).sum()):3d}")
    pp.check_conditions(ps)


@pytest.mark.parametrize("shape,cls", CASES)
def test_reference_equals_the_oracles_records(shape, cls):
    """same pairs, same order, dist and pos to 1e-12 - at the library's capacity, with the oracle's own count of dropped contacts"""
    ps, orc = pp.poses(shape, cls), cp._oracle(shape)
    for i, exp in enumerate(ps.expected):
        hq, q = ps.hand_quat[:, i], ps.qpos[:, i]
        ref = orc.contacts(hq, q)                               # the oracle at the library's capacity
        assert orc.sim(hq).s.ncon_max == pp.capacity(shape)
        assert orc.sim(hq).s.ncon_dropped == ps.dropped[i] == ps.oracle_dropped[i], (i, orc.sim(hq).s.ncon_dropped, ps.dropped[i])
        assert np.array_equal(ref["pairs"], exp["pairs"]), (i, ref["pairs"].tolist(), exp["pairs"].tolist())
        if len(exp["dist"]):
            assert np.abs(ref["dist"] - exp["dist"]).max() <= 1e-12 and np.abs(ref["pos"] - exp["pos"]).max() <= 1e-12, i
            assert np.array_equal(ref["normal"][exp["vertex"] >= 0], np.tile(pr.E_Z, (int((exp["vertex"] >= 0).sum()), 1)))
        # the recovery the GPU tests use names the reference's vertices on the oracle's records
        for g, pc in ps.per_geom[i].items():
            k, idx, d1, d2 = pr.recover_vertices(ref, orc.M, ps.xmat[i], ps.xpos[i], g)
            assert idx.tolist() == pc.idx[:len(k)].tolist() and (len(k) == len(pc.idx) or ps.dropped[i] > 0), (i, g)
            assert not len(k) or d1.max() < 1e-12


def test_reference_rule_on_hand_made_hulls():
    """the rule's edges on tables small enough to do by hand: the tie band, the spacing threshold's `more than`, the sphere cull, the cap at four"""
    I, V = np.eye(3), np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0], [2, 2, 0.5]], dtype=float)
    p = np.array([0.0, 0.0, -0.01])
    assert pr.plane_pair(I, p, V, 1.0, 0.0).idx.tolist() == [0, 1, 2, 3]            # five tied: the lowest index first, index order, four kept
    assert pr.plane_pair(I, p, V[::-1].copy(), 1.0, 0.0).idx.tolist() == [1, 2, 3, 4]
    W = V.copy()
    W[3, 2] = -2e-12                                                                # deeper by more than the band: first
    assert pr.plane_pair(I, p, W, 1.0, 0.0).idx.tolist() == [3, 0, 1, 2]
    W[3, 2] = -5e-13                                                                # within the band: vertex 0 stays first
    assert pr.plane_pair(I, p, W, 1.0, 0.0).idx.tolist() == [0, 1, 2, 3]
    assert pr.plane_pair(I, p, V, 1.0 / 0.3, 0.0).idx.tolist() == [0, 3]            # threshold 1: at exactly 1 is too close, sqrt 2 is not
    assert pr.plane_pair(I, p, V, 5.0, 0.0).idx.tolist() == [0]
    assert len(pr.plane_pair(I, [0, 0, 1.002], V, 1.0, 1e-3).idx) == 0              # sphere cull
    assert len(pr.plane_pair(I, [0, 0, 2e-3], V, 1.0, 1e-3).idx) == 0               # nothing within the margin
    up = pr.plane_pair(I, [0, 0, 5e-4], V, 1.0, 1e-3)
    assert up.idx.tolist() == [0, 1, 2, 3] and np.allclose(up.dist, 5e-4) and np.allclose(up.pos[1], [1, 0, 2.5e-4])
    assert pr.BAND == cp.BAND
    assert pr.probes(I, p, V, 1.0, 0.0) == (False, True) and pr.probes(I, p, V[:1], 1.0, 0.0) == (True, True)


def test_conditions_fail_when_only_the_hands_lowest_hull_is_aimed(monkeypatch):
    """the conditions bite: with its own lowest vertex on the rungs the palm never has more than 64 vertices within the margin (132 poses, so the
    pose count is not what fails)"""
    monkeypatch.setattr(pp, "ALSO_AIMED", 0.0)
    ps = pp.poses.__wrapped__("CubeS", "hand_floor")
    assert len(ps.expected) >= 100
    with pytest.raises(AssertionError, match="palm vertices within the margin"):
        pp.check_conditions(ps)


@pytest.mark.parametrize("shape,cls", CASES)
def test_host_lane_plane_contacts_match_the_reference(shape, cls):
    ps, M = pp.poses(shape, cls), cp._oracle(shape).M
    for precision in (64, 32):
        ln = lane(shape, precision)
        if precision == 32:
            ln.set_warm(False)
        tally = pp.Tally(ps, precision, f"host lane fp{precision}")
        for i in range(len(ps.expected)):
            _, _, _, nc, con, st = ln.substep(ps.qpos[:, i], ZERO15, ZERO15, ZERO9, ps.hand_quat[:, i])
            tally.add(i, cp.records(M, nc, con), st)
        print(tally.line())
        tally.check()
