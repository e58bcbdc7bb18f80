"""The rangefinder pose generator (tests/ray_poses.py) and the tolerances of tests/test_gpu_rays.py, held on the REFERENCE path without
a GPU: the host lane of the kernel source (serial rangefinder(): RayWalk with LocalStack / OwnBound, fp64 and fp32) against the fp64
oracle, which tests every triangle, on every asserted pose class.  That the reference path meets the caps is what makes them conditions
for the GPU paths rather than guesses; the coverage floors (how many rays hit anything, how many hit the OBJECT) come from the oracle
alone.  Run with -s for the table (recorded in profiles/ray_parity.txt)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from kinovagrasping_amd import scenarios
from tests import ray_poses as rp
from tests.native_build import Lane

N_ENVS = 2040           # 17 x 120: every ray is the aimed one in 120 envs; 34 680 rays per (shape, class)


@pytest.fixture(scope="module")
def pose_sets():
    cache = {}

    def get(shape, cls):
        if (shape, cls) not in cache:
            cache[shape, cls] = rp.poses(shape, cls, N_ENVS)
        return cache[shape, cls]
    return get


def lane_rays(shape, precision, ps):
    lane = Lane(scenarios.model_blob(shape), precision, multi_geom=rp.is_multi_geom(shape))
    with ThreadPoolExecutor(rp.threads()) as pool:
        return np.stack(list(pool.map(lambda i: lane.reset_obs(ps.qpos0[:, i], ps.hand_quat[:, i])[1], range(ps.qpos0.shape[1]), chunksize=64)))


@pytest.mark.parametrize("cls", rp.ASSERTED_CLASSES)
@pytest.mark.parametrize("shape", rp.SHAPES)
def test_host_lane_rays_match_the_oracle_and_the_poses_cover_the_object(shape, cls, pose_sets):
    ps = pose_sets(shape, cls)
    assert ps.rays.shape == (N_ENVS, rp.NRAY) and np.isfinite(ps.rays).all() and ((ps.rays >= 0) | (ps.rays == -1)).all()
    rp.check_coverage(ps)
    for precision in (64, 32):
        got = lane_rays(shape, precision, ps)
        beyond, n_rays, worst = rp.compare(ps, got, precision, f"host lane fp{precision}")
        assert beyond <= rp.allowed_beyond(precision, n_rays), (shape, cls, precision, beyond)


def test_poses_are_reproducible_and_a_prefix_of_a_longer_draw():
    """env i's pose depends on (seed, shape, class, i) only: the GPU tests slice one long draw for their small contexts"""
    a, b = rp.poses("CubeS", "aimed", 40), rp.poses("CubeS", "aimed", 23)
    assert np.array_equal(a.qpos0[:, :23], b.qpos0) and np.array_equal(a.hand_quat[:, :23], b.hand_quat) and np.array_equal(a.rays[:23], b.rays)
    c = rp.poses("CubeS", "aimed", 23, seed=1)
    assert not np.array_equal(c.qpos0, b.qpos0)
    assert np.abs(np.linalg.norm(a.qpos0[12:16], axis=0) - 1).max() < 1e-12 and np.abs(np.linalg.norm(a.hand_quat, axis=0) - 1).max() < 1e-12


def test_object_share_floor_fails_when_the_object_is_out_of_the_rays_reach(monkeypatch):
    """the floors bite: with the object placed 0.5 - 0.6 m along the ray instead of 2 - 12 cm, hardly a ray has it as nearest hit"""
    monkeypatch.setattr(rp, "AIM_T", (0.5, 0.6))
    ps = rp.poses("CubeS", "aimed", 340)
    with pytest.raises(AssertionError, match="object share"):
        rp.check_coverage(ps)


@pytest.mark.parametrize("shape", ["CubeS", "Vase1S", "BowlS"])
def test_object_hit_slots_agree_with_moving_the_object_away(shape):
    """object_hit_slots (hit point on a triangle of the object: what the whole-observation GPU tests print) against the generator's
    own answer (the oracle's distance changes when the object is moved away) - a ray that ends where the object touches the hand or
    the ground belongs to both, hence the allowance of a few slots"""
    from kinovagrasping_amd import model_compiler as mc
    from kinovagrasping_amd.sim import SOLVER_ITERATIONS
    from oracle import ko_py as ko
    blob = scenarios.model_blob(shape)
    M, model = mc.read_blob(blob), ko.OracleModel(blob)
    ps = rp.poses(shape, "aimed", 170)
    got = np.zeros_like(ps.obj_hit)
    for i in range(170):
        o = ko.OracleSim(model, ps.hand_quat[:, i], solver_iterations=SOLVER_ITERATIONS)
        o.env_reset(ps.qpos0[:, i])
        got[i] = rp.object_hit_slots(M, o)
    assert ps.obj_hit.sum() >= 170 and (got != ps.obj_hit).sum() <= 3, (int(ps.obj_hit.sum()), int((got != ps.obj_hit).sum()))


def test_compare_counts_flips_and_errors_beyond_the_tolerance():
    ps = rp.poses("CubeS", "aimed", 34)
    lines = []
    assert rp.compare(ps, ps.rays.copy(), 64, "self", out=lines.append)[0] == 0
    got = ps.rays.copy()
    h, m = np.argwhere(got >= 0)[0], np.argwhere(got < 0)[0]
    got[h[0], h[1]] += 5e-9                          # beyond the fp64 tolerance, far within the fp32 one
    assert rp.compare(ps, got, 64, "x", out=lines.append)[0] == 1 and rp.compare(ps, got, 32, "x", out=lines.append)[0] == 0
    got[m[0], m[1]] = 0.05                           # a miss reported as a hit
    assert rp.compare(ps, got, 32, "x", out=lines.append)[0] == 1
    got[h[0], h[1]] = -1.0                           # a hit reported as a miss
    assert rp.compare(ps, got, 32, "x", out=lines.append)[0] == 2
    assert sum("BEYOND" in l for l in lines) == 4
    assert rp.allowed_beyond(64, 10 ** 6) == 0 and rp.allowed_beyond(32, 1999) == 0 and rp.allowed_beyond(32, 34680) == 17
    assert np.array_equal(rp.from_obs([6.0, 0.5, 5.9]), [-1.0, 0.5, 5.9])
