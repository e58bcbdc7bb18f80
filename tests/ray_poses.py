"""Seeded poses for the rangefinder tests (tests/test_rays_cpu.py, tests/test_gpu_rays.py) with the fp64 oracle's answer for each.

The suite's other ray checks use the start tables in the three named hand poses, where most rays miss, hit the ground or hit the hand
itself.  The classes below put the OBJECT onto the rays, beside its mesh features and into the branches of the box test that random
directions never take:

  table          the start tables in the three named poses (what the rest of the suite uses)
  aimed          random hand posture; the centre of the geom named `object` (the body origin of every single-geom object) is placed on ray
                 (env % 17), up to 4 cm beside it, random object orientation
  near_feature   as aimed, but a vertex / an edge midpoint / a face centre (in turn) of a random triangle of the object's ray mesh is
                 brought onto the ray and then moved 20 - 200 um sideways
  axis_aligned   hand and object orientations from the 24 rotations of the cube, joints zero, the object on the point of a 1 cm grid (origin
                 off the round numbers) nearest to a point on ray (env % 17): direction components that are exactly zero (the par[]
                 branch of bvh_box_entry_inv, rays parallel to box slabs)
  exact_feature  near_feature WITHOUT the sideways move.  No oracle answer: the oracle holds the fp64 mesh, the kernels its fp32
                 rounding, and a ray through a vertex falls into different cracks of the two.  Used for cross-path comparisons only.

`poses(shape, cls, n)` returns a PoseSet: qpos0 [16, n], hand_quat [4, n], rays [n, 17] (the oracle's sensordata[9:], -1 = miss;
None for exact_feature) and obj_hit [n, 17] (the object is the ray's nearest hit: the oracle's answer changes when the object is
moved to (5, 5, 5))."""
from __future__ import annotations

import os
import zlib
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from itertools import permutations, product

import numpy as np

from kinovagrasping_amd import model_compiler as mc, scenarios
from kinovagrasping_amd.sim import SOLVER_ITERATIONS
from oracle import ko_py as ko

NRAY = 17
STANDARD_SHAPES = ("CubeS", "Vase1S", "CylinderB", "bcyl")          # libkinova_sim.so
MULTI_GEOM_SHAPES = ("BowlS", "BottleS")                            # libkinova_sim_mg.so (16 geom slots per ray)
SHAPES = STANDARD_SHAPES + MULTI_GEOM_SHAPES
ASSERTED_CLASSES = ("table", "aimed", "near_feature", "axis_aligned")
CLASSES = ASSERTED_CLASSES + ("exact_feature",)
NAMED_POSES = ("normal", "rotated", "top")
FAR = np.array([5.0, 5.0, 5.0])
AIM_T = (0.02, 0.12)            # distance along the ray at which the object's origin is placed (aimed)
FEATURE_T = (0.02, 0.10)        # ... at which the mesh feature is placed (near_feature, exact_feature)
GRID = 0.01                     # axis_aligned: the object sits on a 1 cm grid ...
# ... whose origin is off the round numbers: the hand's sites and the objects' faces sit at round tenths of a millimetre, so with the grid
# through (0, 0, 0) axis-parallel rays run IN the plane of a face or through a symmetry axis of the mesh (measured: CubeS ray 2 at local
# x = -1e-20, Vase1S rays within 7 um of its rim plane; the fp64 oracle and the fp32 lane then fall into different cracks, and a 10 um nudge
# of the object makes all three agree again).  Those are exact_feature poses, not what this class is for (direction components of exactly 0).
GRID_ORIGIN = np.array([0.00137, 0.00271, 0.00433])

PoseSet = namedtuple("PoseSet", "shape cls qpos0 hand_quat rays obj_hit")


def threads():
    return max(1, min(16, os.cpu_count() or 1))


def _unit_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def cube_rotation_quats():
    """the 24 proper rotations of the cube (signed permutation matrices of determinant +1) as unit quaternions"""
    out = []
    for perm in permutations(range(3)):
        for signs in product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if np.linalg.det(R) > 0:
                out.append(mc.mat_to_quat(R))
    assert len(out) == 24
    return np.array(out)


def _perpendicular(rng, vec):
    a = rng.normal(size=3)
    a -= vec * (a @ vec)
    return a / np.linalg.norm(a)


def _oracle_reset(model, hq, q0):
    """(rays [17], site_xpos [17, 3], site z axes [17, 3]) of the oracle's reset at q0"""
    o = ko.OracleSim(model, hq, solver_iterations=SOLVER_ITERATIONS)
    o.env_reset(q0)
    xmat = o.view("site_xmat").reshape(-1, 9)
    return o.view("sensordata")[9:9 + NRAY].copy(), o.view("site_xpos").reshape(-1, 3)[:NRAY].copy(), xmat[:NRAY][:, [2, 5, 8]].copy()


def _hand_posture(rng, M, q):
    """slides uniform in +-0.02, the six finger joints uniform in [0, 1.2], both clipped to the model's joint ranges"""
    sl = rng.uniform(-0.02, 0.02, 3)
    q[0:3] = np.clip(sl, M["slide_range"][:, 0], M["slide_range"][:, 1])
    fj = rng.uniform(0.0, 1.2, 6)
    lim = M["hinge_limited"].astype(bool)
    q[3:9] = np.where(lim, np.clip(fj, M["hinge_range"][:, 0], M["hinge_range"][:, 1]), fj)


def _table_start(shape, i):
    """env i of the table class: named pose i % 3, a row of its start table (the reference's empty-file rule where it ships none),
    the reference reset's 5 cm correction for objects whose meshes carry a CAD origin"""
    pose = NAMED_POSES[i % 3]
    if scenarios.has_start_table(shape, pose):
        tab = scenarios.start_coord_table(shape, pose)
        xyz = tab[(131 * (i // 3) + 7) % len(tab)]
    else:
        xyz = scenarios.fallback_start(shape, pose, np.random.RandomState(1000 + i))
    q = np.zeros(16)
    q[9:12] = scenarios.reset_body_position(shape, xyz)
    q[12] = 1.0
    return q, scenarios.hand_quat_for(pose)


def _draw(shape, cls, i, rng, M, cube_q):
    """the part of env i's pose that does not depend on where its ray is: (qpos0 with the object far away, hand quaternion)"""
    q = np.zeros(16)
    q[9:12], q[12] = FAR, 1.0
    if cls == "table":
        return _table_start(shape, i)
    if cls == "axis_aligned":
        hq = cube_q[rng.integers(24)]
        q[12:16] = cube_q[rng.integers(24)]
        return q, hq
    _hand_posture(rng, M, q)
    hq = scenarios.hand_quat_for(NAMED_POSES[(i // 2) % 3]) if i % 2 == 0 else _unit_quat(rng)
    q[12:16] = _unit_quat(rng)
    return q, hq


def _place(cls, i, rng, M, q, pnt, vec):
    """object position of env i, given the origin and direction of its ray (i % 17) with the object out of the way"""
    r = i % NRAY
    p, v = pnt[r], vec[r]
    Ro = mc.quat_to_mat(q[12:16])
    centre = Ro @ M["geom_pos"][8]          # of the geom named `object`, from the body origin (README shapes: < 2 um; the bottles' CAD origin: 0.19 m)
    if cls == "aimed":
        return p + rng.uniform(*AIM_T) * v + rng.uniform(0.0, 0.04) * _perpendicular(rng, v) - centre
    if cls == "axis_aligned":
        # the grid point nearest to a point on the ray: with a fixed box of grid points in front of the hand fewer than 3 % of the rays
        # have the object as nearest hit, and the primitive cylinder's model not even 10 % hits of any kind
        cell = np.round((p + rng.uniform(*AIM_T) * v - centre - GRID_ORIGIN) / GRID)
        return GRID_ORIGIN + cell * GRID
    # near_feature / exact_feature: a feature of a random triangle of a random piece's ray mesh (geom frame)
    g = int(rng.integers(8, len(M["geom_body"])))
    tri = M[f"mesh{int(M['geom_mesh'][g])}_tri"].astype(np.float64).reshape(-1, 3, 3)
    t3, k = tri[rng.integers(len(tri))], int(rng.integers(3))
    kind = (i // NRAY) % 3
    feat = t3[k] if kind == 0 else (0.5 * (t3[k] + t3[(k + 1) % 3]) if kind == 1 else t3.mean(0))
    world = Ro @ (M["geom_pos"][g] + mc.quat_to_mat(M["geom_quat"][g]) @ feat)
    pos = p + rng.uniform(*FEATURE_T) * v - world
    lat, s = _perpendicular(rng, v), rng.uniform(20e-6, 200e-6)
    return pos + s * lat if cls == "near_feature" else pos


def _one(shape, cls, i, seed, model, M, cube_q):
    rng = np.random.default_rng([seed, zlib.crc32(shape.encode()), CLASSES.index(cls), i])
    q, hq = _draw(shape, cls, i, rng, M, cube_q)
    far = q.copy()
    far[9:12] = FAR
    rays_far, pnt, vec = _oracle_reset(model, hq, far)
    if cls != "table":
        q[9:12] = _place(cls, i, rng, M, q, pnt, vec)
    if cls == "exact_feature":
        return q, hq, None, None
    rays = _oracle_reset(model, hq, q)[0]
    return q, hq, rays, rays != rays_far


def poses(shape: str, cls: str, n: int, seed: int = 0) -> PoseSet:
    assert cls in CLASSES
    blob = scenarios.model_blob(shape)
    model, M, cube_q = ko.OracleModel(blob), mc.read_blob(blob), cube_rotation_quats()
    with ThreadPoolExecutor(threads()) as pool:
        out = list(pool.map(lambda i: _one(shape, cls, i, seed, model, M, cube_q), range(n), chunksize=max(1, n // (4 * threads()))))
    q0, hq = np.stack([o[0] for o in out], 1), np.stack([o[1] for o in out], 1)
    if cls == "exact_feature":
        return PoseSet(shape, cls, q0, hq, None, None)
    return PoseSet(shape, cls, q0, hq, np.stack([o[2] for o in out]), np.stack([o[3] for o in out]))


def object_hit_slots(M, o, tol=2e-6):
    """[17] bool, from an oracle sim's CURRENT fields (site and geom poses and sensordata of one mj_forward: after env_reset, or after
    env_step - the forward at the start of its last substep): the rays whose distance ends on a triangle of the object's ray meshes
    (geoms 8 ..; M = model_compiler.read_blob of the model).  For the summaries of tests that compare whole observations: what did
    their ray slots hit?  (poses() asks the oracle itself, by moving the object away - this is the cheap form for a stepped state.)"""
    d = o.view("sensordata")[9:9 + NRAY]
    pnt = o.view("site_xpos").reshape(-1, 3)[:NRAY]
    vec = o.view("site_xmat").reshape(-1, 9)[:NRAY][:, [2, 5, 8]]
    gp, gm = o.view("geom_xpos").reshape(-1, 3), o.view("geom_xmat").reshape(-1, 3, 3)
    out = np.zeros(NRAY, dtype=bool)
    for g in range(8, len(M["geom_body"])):
        tri = M[f"mesh{int(M['geom_mesh'][g])}_tri"].astype(np.float64).reshape(-1, 3, 3)
        v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        nrm = np.cross(e1, e2)
        nn = np.linalg.norm(nrm, axis=1)
        ok = nn > 0
        for r in np.flatnonzero((d >= 0) & ~out):
            x = gm[g].T @ (pnt[r] + d[r] * vec[r] - gp[g]) - v0              # hit point in the geom frame, from each triangle's first vertex
            off = np.abs((x * nrm).sum(1)) / np.where(ok, nn, 1.0)
            # barycentric coordinates of the projection
            d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
            x1, x2 = (x * e1).sum(1), (x * e2).sum(1)
            det = np.where(ok, d11 * d22 - d12 * d12, 1.0)
            u, v = (d22 * x1 - d12 * x2) / det, (d11 * x2 - d12 * x1) / det
            slack = tol / np.sqrt(np.minimum(d11, d22).clip(1e-30))
            out[r] = bool((ok & (off <= tol) & (u >= -slack) & (v >= -slack) & (u + v <= 1 + slack)).any())
    return out


def is_multi_geom(shape: str) -> bool:
    return shape in MULTI_GEOM_SHAPES


# ---- the comparison both test files make -------------------------------------------------------------------------------------
FP64_TOL = 1e-9          # the project's fp64 tolerance, absolute
FP32_TOL = 2e-4          # |got - ref| <= FP32_TOL * (1 + |ref|): the observation tolerance of tests/test_gpu_obs_contacts.py
FP32_CAP = 0.0005        # share of a (shape, class, path)'s rays that may be beyond FP32_TOL; none below CAP_MIN_RAYS rays
CAP_MIN_RAYS = 2000


def from_obs(slots):
    """observation slots 50-66 -> ray distances: the observation stores a miss (-1) as 6"""
    r = np.array(slots, dtype=np.float64)
    r[r == 6.0] = -1.0
    return r


def compare(ps: PoseSet, got, precision: int, path: str, out=print):
    """`got` [n, 17] (-1 = miss) against the oracle's rays of ps.  Prints every ray beyond the tolerance and one summary line; returns
    (number beyond, rays, worst error among the rays within the tolerance).  A hit / miss flip counts as beyond."""
    ref = ps.rays
    assert got.shape == ref.shape
    flip = (got < 0) != (ref < 0)
    err = np.where(flip, np.inf, np.abs(got - ref))
    tol = FP64_TOL if precision == 64 else FP32_TOL * (1 + np.abs(ref))
    beyond = err > tol
    for e, r in np.argwhere(beyond):
        out(f"  BEYOND {ps.shape} {ps.cls} {path}: env {e} ray {r} got {got[e, r]!r} oracle {ref[e, r]!r} object nearest {bool(ps.obj_hit[e, r])}")
    worst = float(err[~beyond].max()) if (~beyond).any() else 0.0
    out(f"{ps.shape:10s} {ps.cls:13s} {path:28s} rays {ref.size:6d} hit {np.mean(ref >= 0):.3f} object {ps.obj_hit.mean():.3f} "
        f"beyond {int(beyond.sum()):3d} worst within {worst:.2e}")
    return int(beyond.sum()), ref.size, worst


def allowed_beyond(precision: int, n_rays: int) -> int:
    """fp64: none.  fp32: 0.05 % of the rays, none in a set of fewer than 2 000 - the reference path (the host lane of the kernel source)
    needs 0.0017 % at worst, so the cap leaves room for edge grazes that round differently on the GPU and is 20 x below the 1 % of the
    whole-observation tests."""
    if precision == 64 or n_rays < CAP_MIN_RAYS:
        return 0
    return int(FP32_CAP * n_rays)


def check_coverage(ps: PoseSet):
    """coverage floors from the oracle alone (a wrong kernel cannot meet them)"""
    hit = (ps.rays >= 0).mean()
    if ps.cls in ("aimed", "near_feature"):
        assert ps.obj_hit.mean() >= 0.10, (ps.shape, ps.cls, "object share", ps.obj_hit.mean())
        per_ray = ps.obj_hit.mean(0)                                                   # ray r over all envs
        assert per_ray.min() >= 0.02, (ps.shape, ps.cls, "per-ray object share", per_ray)
    if ps.cls in ("table", "aimed", "near_feature"):
        assert hit >= 0.20 and 1 - hit >= 0.10, (ps.shape, ps.cls, "hit share", hit)
    if ps.cls == "axis_aligned":
        assert hit >= 0.10 and 1 - hit >= 0.10, (ps.shape, ps.cls, "hit share", hit)
