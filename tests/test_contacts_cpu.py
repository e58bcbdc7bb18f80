"""The narrow phase of the kernel source (gjk_distance, mpr_penetration_sm, and in the multi-geom build the fp64 distance query) against the
fp64 oracle on the aimed contact poses of tests/contact_poses.py, without a GPU: the host lane (tests/native/ks_lanecheck.cpp), fp64 and
fp32, cold and with the lane's pair memory carried over - from the previous pose, from every other pose, and from ANOTHER OBJECT.  The
compiled gfx950 kernels meet the same poses and bounds in tests/test_gpu_contacts.py.

Bounds (tests/contact_poses.py BOUNDS): on decidable poses the contact count and the ordered pair list equal the oracle's; fp64 point and
distance 1e-9, normal 1e-7; fp32 distance 2e-6, normal 2e-4, point 1e-4; no exception on gap_ladder and feature; on parallel (a face flat on
a face: the documented tie) the point is reported only, and so are the fp32 normal and point on the few poses where the oracle's own
normal is not settled (contact_poses.py: CONDITIONED).  The generator's own conditions are checked against the oracle alone.
Run with -s for the table."""
import numpy as np
import pytest

from kinovagrasping_amd import scenarios
from tests import contact_poses as cp
from tests.native_build import Lane

CASES = [(s, c) for s in cp.SHAPES for c in cp.OBJECT_CLASSES] + [(s, "hand_margin") for s in cp.HAND_MARGIN_SHAPES]
ZERO15, ZERO9 = np.zeros(15), np.zeros(9)
_lanes = {}


def lane(shape, precision):
    if (shape, precision) not in _lanes:
        _lanes[shape, precision] = Lane(scenarios.model_blob(shape), precision, multi_geom=cp.on_mg_library(shape))
    return _lanes[shape, precision]


def query(ln, M, ps, i):
    """the lane's contact list at pose i (the contacts of a substep are those of the state it starts from)"""
    _, _, _, nc, con, st = ln.substep(ps.qpos[:, i], ZERO15, ZERO15, ZERO9, ps.hand_quat[:, i])
    assert st & 6 == 0, (ps.shape, ps.cls, i, st)
    return cp.records(M, nc, con)


@pytest.mark.parametrize("shape,cls", CASES)
def test_pose_sets_meet_the_generators_conditions(shape, cls):
    ps = cp.poses(shape, cls)
    print(f"{shape} {cls}: {len(ps.ref)} poses, {int((~ps.decidable).sum())} undecidable, {int((~ps.conditioned).sum())} with an unsettled record, {int(ps.near.sum())} with the aimed pair apart by < 1e-5 m")
    cp.check_conditions(ps)
    assert np.abs(np.linalg.norm(ps.qpos[12:16], axis=0) - 1).max() < 1e-12 and np.isfinite(ps.qpos).all()
    assert set(np.unique(ps.rung)) == set(cp.MARGIN_RUNGS if cls == "hand_margin" else cp.RUNGS)


def test_pose_sets_are_reproducible():
    cp.poses.cache_clear(); cp.seeds.cache_clear()
    a = cp.poses("CubeS", "feature")
    cp.poses.cache_clear(); cp.seeds.cache_clear()
    b = cp.poses("CubeS", "feature")
    assert np.array_equal(a.qpos, b.qpos) and np.array_equal(a.decidable, b.decidable)


def test_conditions_fail_on_a_ladder_without_its_fine_rungs(monkeypatch):
    """the conditions bite: a ladder that stays 300 um away from touching has no pose within 1e-5 m of it"""
    monkeypatch.setattr(cp, "RUNGS", (-3e-3, -3e-4, -3e-5, -3e-6, 3e-4, 1e-3))
    ps = cp.poses.__wrapped__("CubeS", "gap_ladder")
    with pytest.raises(AssertionError, match="apart by less than"):
        cp.check_conditions(ps)


@pytest.mark.parametrize("shape,cls", CASES)
def test_host_lane_contacts_match_the_oracle(shape, cls):
    """cold fp64, cold fp32, and fp32 with the pair memory of the previous pose of the set (neighbouring rungs of a ladder: the warm start the
    stepping kernels make from substep to substep)"""
    ps, M = cp.poses(shape, cls), cp._oracle(shape).M
    failures = []
    for precision, warm, path in ((64, False, "host lane fp64"), (32, False, "host lane fp32 cold"), (32, True, "host lane fp32 previous pose's memory")):
        ln = lane(shape, precision)
        if precision == 32:
            ln.set_warm(warm)
        tally = cp.Tally(ps, precision, path)
        for i in range(len(ps.ref)):
            tally.add(i, query(ln, M, ps, i))
        print(tally.line())
        failures += [(path,) + f for f in tally.failures]
        assert tally.compared >= 0.85 * tally.poses
    lane(shape, 32).set_warm(False)
    assert not failures, failures[:10]


@pytest.mark.parametrize("shape", ["CubeS", "CylinderB", "BottleS"])
def test_pair_memory_of_every_other_pose_of_the_same_object(shape):
    """(a) 32 poses of the gap ladder, each queried with the memory every other one of them left behind (992 evaluations): within the oracle
    bounds, and on the pairs without margin of decidable poses bit for bit what the cold query returns"""
    ps, M = cp.poses(shape, "gap_ladder"), cp._oracle(shape).M
    ln = lane(shape, 32)
    pick = np.linspace(0, len(ps.ref) - 1, 32).round().astype(int)
    ln.set_warm(False)
    cold = {i: query(ln, M, ps, i) for i in pick}
    memory = {}
    for i in pick:
        ln.set_warm(True)
        query(ln, M, ps, i)
        memory[i] = ln.get_warm()
    assert any(m.any() for m in memory.values())
    tally, differs, n = cp.Tally(ps, 32, "host lane fp32 another pose's memory"), [], 0
    for j in pick:
        for i in pick:
            if i == j:
                continue
            ln.put_warm(memory[j])
            got = query(ln, M, ps, i)
            tally.add(i, got)
            n += 1
            if ps.decidable[i] and not cp.same_bits(cp.margin0(M, got), cp.margin0(M, cold[i])):
                differs.append((int(j), int(i)))
    ln.set_warm(False)
    assert ln.ids_out_of_range() == 0
    print(tally.line(), f"| {n} evaluations, {len(differs)} differ from the cold query on pairs without margin")
    assert n == 992 and not tally.failures and not differs, (tally.failures[:5], differs[:5])


def test_pair_memory_of_another_object_names_vertices_beyond_the_hull_tables():
    """(b) The memory a lane holds after CylinderB poses (object hull: 142 vertices) handed to CubeS poses (24 vertices).  RAW - what the stepping
    kernels met after ks_reset_objects gave an env another object, before that call cleared the env's block - gjk_distance is asked to rebuild
    simplices from vertex ids beyond the table (this build counts them and substitutes vertex 0; the product would read out of range).  By the
    product's rule - the block cleared when the env's object changes - it is not, and the queries are the cold ones bit for bit."""
    src, dst = cp.poses("CylinderB", "gap_ladder"), cp.poses("CubeS", "gap_ladder")
    Ms, Md = cp._oracle("CylinderB").M, cp._oracle("CubeS").M
    a, b = lane("CylinderB", 32), lane("CubeS", 32)
    n = min(len(src.ref), len(dst.ref))
    b.set_warm(False)
    cold = [query(b, Md, dst, i) for i in range(n)]
    b.ids_out_of_range()
    raw, cleared, tally = 0, 0, cp.Tally(dst, 32, "host lane fp32 CylinderB's memory")
    for i in range(n):
        a.set_warm(True)
        query(a, Ms, src, i)
        memory = a.get_warm()
        assert a.ids_out_of_range() == 0                  # the object's own memory is in range
        b.put_warm(memory)
        tally.add(i, query(b, Md, dst, i))
        raw += b.ids_out_of_range()
        b.put_warm(np.zeros_like(memory))               # ks_reset_objects: k_store_init clears the env's block
        assert cp.same_bits(query(b, Md, dst, i), cold[i])
        cleared += b.ids_out_of_range()
    a.set_warm(False); b.set_warm(False)
    print(tally.line(), f"| out-of-range ids: raw {raw}, cleared {cleared}")
    assert raw > 0 and cleared == 0
    assert not tally.failures, tally.failures[:5]
