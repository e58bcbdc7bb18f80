"""Aimed snapshots for the observation stage (build_obs of csrc/ks_obs.h and its callers in csrc/ks_api.hip) - the analogue of
tests/dynamics_states.py for the stage between the physics and the learner.  tests/obs_ref.py has the reference and the bound.

Every class starts from the oracle's body poses (its forward kinematics at a qpos and hand quaternion, both fp32 numbers) in the three named
hand poses and is then edited.  Every input - the 105-value snapshot and the 17 rays - is rounded to fp32 before kernel or reference sees it.
Fixed seeds; 100 - 300 states per (class, shape).

  lift_band        the object body placed so that the reference's geom-centre z is 0.19, 0.195 -+ 1, 4, 64 fp32 ulps and -+ 1e-5, 0.1999,
                   0.2 -+ 1 ulp, 0.21; upright (turned about z) and randomly rotated.  CubeS, Cone1S (geom centre 12 mm off the body origin),
                   Vase1S (the shape whose rollout contexts run the workgroup and queue forms); BottleS on the multi-geom library (0.2 m
                   off).  The heights within 4 ulps of 0.195 are undecidable by construction and hold NEAR of the LIFT_EACH states that
                   every other height holds: under the 5 % cap.
  palm_rays        all 32 subsets of the five palm rays below the threshold; members at 0, 0.03, nextafter(0.06f, 0), the others at
                   nextafter(0.06f, 1), 0.1 and -1 (a miss beside a hit), the other twelve rays mixed hits and misses
  on_threshold     (the named sub-class of palm_rays) one palm ray exactly 0.06f = 0.05999999865889549: the fp64 reference counts it, an fp32
                   comparison with 0.06f does not.  Every state is undecidable by construction; fp64 paths must equal the reference, fp32
                   paths the reference with that ray left out.
  palm_object      (the in-step form of palm_rays) the object 2 - 8 cm along a palm ray in front of the palm, up to 3 cm beside it, at random
                   orientations, fingers open: the ORACLE's palm rays end on it on either side of 0.06.  Of 900 seeded draws those are kept
                   whose five palm rays are all decidable (a miss, or farther from 0.06 than the ray tolerance), at most PALM_EACH per
                   subset of rays below the threshold: 28 of the 32 subsets, every count nh = 0 .. 5 (tests/test_obs_cpu.py asserts both)
  gravity_axis     hand and object turned rigidly about the hand's origin so that each component of g (slots 67-69) is the largest, with
                   either sign; near ties of the two largest at 1e-2, 1e-4, 1e-6
  finger_fans      the oracle's kinematics along a ladder of finger closures over the whole joint range, symmetric, and one finger ahead of
                   the others: both orders of total1 / total2, front areas down to the smallest the ranges allow
  object_bearing   the object in the wrist frame at ol[0] or ol[2] = 1e-7 .. 1e-1 beside the centre line, at ol[1] < 0, and at |ol[1]| <= 1e-6:
                   angles near 0, pi / 2 and pi
  twentieth_power  hand and object moved so that d of dot_product20 sweeps 0.05 .. 1 (the slot 1e-26 .. 1), the hand's origin 1 mm, 1 cm and
                   10 cm from the world z axis
  ranges           every ray -1, every ray 0, rays at 5.99 and 6.0

States that lift_band, palm_object, gravity_axis, finger_fans and object_bearing hold are a qpos and a hand quaternion (the snapshot is the oracle's
kinematics of them): the in-step GPU paths reach them through ks_reset.  The other classes edit the snapshot or the rays directly."""
from __future__ import annotations

import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

from kinovagrasping_amd import model_compiler as mc, scenarios
from tests import contact_poses as cp
from tests.obs_ref import F06, f32

POSES = cp.NAMED_POSES
CLASSES = ("lift_band", "palm_rays", "on_threshold", "palm_object", "gravity_axis", "finger_fans", "object_bearing", "twentieth_power", "ranges")
QPOS_CLASSES = ("lift_band", "palm_object", "gravity_axis", "finger_fans", "object_bearing")       # expressible as qpos + hand quaternion
SHAPES = {"lift_band": ("CubeS", "Cone1S", "Vase1S", "BottleS"), "object_bearing": ("CubeS", "BottleS"), "twentieth_power": ("CubeS", "BottleS")}
MG_SHAPE = "BottleS"
UNDECIDABLE_CAP, DROP_CAP, BRANCH_FLOOR = 0.05, 0.02, 30
ULP195 = float(np.spacing(np.float32(0.195)))
ULP2 = float(np.spacing(np.float32(0.2)))
Z195, Z2 = float(np.float32(0.195)), float(np.float32(0.2))
LIFT_HEIGHTS = ([("0.19", 0.19), ("0.195-1e-5", 0.195 - 1e-5), ("0.195+1e-5", 0.195 + 1e-5), ("0.195-64ulp", Z195 - 64 * ULP195), ("0.195+64ulp", Z195 + 64 * ULP195),
                 ("0.1999", 0.1999), ("0.2-1ulp", Z2 - ULP2), ("0.2+1ulp", Z2 + ULP2), ("0.21", 0.21)],
                [("0.195-1ulp", Z195 - ULP195), ("0.195+1ulp", Z195 + ULP195), ("0.195-4ulp", Z195 - 4 * ULP195), ("0.195+4ulp", Z195 + 4 * ULP195)])
LIFT_EACH, NEAR = 30, 3                      # states per height: 9 x 30 + 4 x 3 = 282, of which 12 (4.3 %) within 4 ulps of the threshold
BELOW, ABOVE = float(np.nextafter(np.float32(0.06), np.float32(0))), float(np.nextafter(np.float32(0.06), np.float32(1)))
MEMBER_VALUES, OTHER_VALUES = (0.0, 0.03, BELOW), (ABOVE, 0.1, -1.0)
PALM_DRAWS, PALM_EACH = 900, 12
PALM_T, PALM_BESIDE = (0.02, 0.08), 0.03     # the object's centre along a palm ray and beside it
TIES = (1e-2, 1e-4, 1e-6)
BEARING_SIDES = tuple(10.0 ** -k for k in range(7, 0, -1))
JPOS_ORDER = (0, 1, 2, 3, 5, 7, 4, 6, 8)     # the nine jointpos sensors: slides, proximal 1-3, distal 1-3

States = namedtuple("States", "cls shape M snap rays qpos hq tag")       # snap [105, n], rays [17, n] fp32 numbers; qpos [16, n], hq [4, n] or None


def rng_for(cls, shape):
    return np.random.default_rng([zlib.crc32(f"obs/{cls}/{shape}".encode()), 11])


def model(shape):
    return cp._oracle(shape).M


def unit_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def z_turn(a):
    return np.array([np.cos(a / 2), 0.0, 0.0, np.sin(a / 2)])


def snapshot(shape, hq, qpos):
    """the oracle's snapshot [105] (float64, NOT rounded) of a state: poses of bodies 2..9 and the nine jointpos sensors"""
    o = cp._oracle(shape).sim(hq)
    o.set_state(qpos, np.zeros(15), np.zeros(15))
    o.forward()
    xp, xm = o.view("xpos").reshape(-1, 3), o.view("xmat").reshape(-1, 9)
    s = np.zeros(105)
    for b in range(2, 10):
        s[(b - 2) * 12:(b - 2) * 12 + 9], s[(b - 2) * 12 + 9:(b - 2) * 12 + 12] = xm[b], xp[b]
    s[96:105] = np.asarray(qpos)[list(JPOS_ORDER)]
    return s


def base_state(shape, pose, rng, closure=None):
    """(qpos, hq) fp32 numbers: the named pose's start row with the fingers at a drawn closure (distal joints near tendon rest)"""
    hq = f32(scenarios.hand_quat_for(pose))
    tab = scenarios.start_coord_table("CubeS", pose)
    q = np.zeros(16)
    q[12] = 1.0
    q[9:12] = tab[int(rng.integers(len(tab)))]
    q[0:3] = scenarios.hand_slide_offsets(pose, "CubeS", "pose")
    c = rng.uniform(0.0, 1.2, 3) if closure is None else np.asarray(closure, dtype=np.float64)
    q[3:9:2], q[4:9:2] = c, np.clip(c / 2 + rng.uniform(-0.1, 0.1, 3), 0.0, 2.0)
    return f32(q), hq


def body(s, b):
    o = (b - 2) * 12
    return s[o:o + 9].reshape(3, 3).copy(), s[o + 9:o + 12].copy()


def put_body(s, b, R, p):
    o = (b - 2) * 12
    s[o:o + 9], s[o + 9:o + 12] = np.asarray(R).ravel(), p


def wrist_frame(M, s):
    """(T3, wrist) of a snapshot in float64, as obs_ref.evaluate forms them"""
    R7, p7 = body(s, 2)
    q = np.asarray(M["geom_quat"][1], dtype=np.float64)
    Rp = R7 @ mc.quat_to_mat(q / np.linalg.norm(q))
    T3 = np.stack([-Rp[:, 1], -Rp[:, 2], Rp[:, 0]])
    return T3, p7 + R7 @ M["geom_pos"][1] + T3.T @ np.array([-0.009, 0.048, 0.0])


def mixed_rays(rng, n):
    """[17, n] rays, hits and misses mixed, none of the palm's five below the threshold"""
    r = np.where(rng.random((17, n)) < 0.4, -1.0, rng.uniform(0.07, 3.0, (17, n)))
    return f32(r)


def _finish(cls, shape, snaps, rays, qpos, hq, tags):
    snap = f32(np.stack(snaps, 1))
    n = snap.shape[1]
    rays = mixed_rays(rng_for(cls + "/rays", shape), n) if rays is None else f32(np.stack(rays, 1))
    return States(cls, shape, model(shape), snap, rays, None if qpos is None else np.stack(qpos, 1), None if hq is None else np.stack(hq, 1), tags)


def _place_z(M, q, target):
    """qpos[11] (an fp32 number) that puts the object's geom centre at height `target` in the reference"""
    Ro = mc.quat_to_mat(q[12:16] / np.linalg.norm(q[12:16]))
    q[11] = float(np.float32(target - (Ro @ M["geom_pos"][8])[2]))
    return q


def lift_band(shape):
    rng, M = rng_for("lift_band", shape), model(shape)
    snaps, qs, hqs, tags = [], [], [], []
    for group, each in zip(LIFT_HEIGHTS, (LIFT_EACH, NEAR)):
        for name, z in group:
            for i in range(each):
                q, hq = base_state(shape, POSES[i % 3], rng)
                q[12:16] = f32(z_turn(rng.uniform(0, 2 * np.pi)) if i % 2 == 0 else unit_quat(rng))
                q = _place_z(M, q, z)
                snaps.append(snapshot(shape, hq, q)); qs.append(q); hqs.append(hq); tags.append((name, POSES[i % 3], z))
    s = _finish("lift_band", shape, snaps, None, qs, hqs, tags)
    # the snapshot's rotation was rounded after the height was set: with the geom centre 0.2 m off the origin that moves the centre by an
    # ulp.  The rounded snapshot's own origin height is set again, so that its centre is within half a spacing of that height of the target.
    for i, t in enumerate(tags):
        s.snap[95, i] = float(np.float32(t[2] - s.snap[90:93, i] @ M["geom_pos"][8]))
    return s


def _palm_states(cls, shape, n):
    rng = rng_for(cls, shape)
    return rng, [snapshot(shape, *reversed(base_state(shape, POSES[i % 3], rng))) for i in range(n)]


def palm_rays(shape="CubeS"):
    rng, snaps = _palm_states("palm_rays", shape, 32 * 6)
    rays, tags = [], []
    for sub in range(32):
        for k in range(6):
            r = mixed_rays(rng, 1)[:, 0]
            for i in range(5):
                r[i] = (MEMBER_VALUES if sub >> i & 1 else OTHER_VALUES)[(k + i + sub) % 3]
            rays.append(r); tags.append(("subset", sub))
    return _finish("palm_rays", shape, snaps, rays, None, None, tags)


def on_threshold(shape="CubeS"):
    rng, snaps = _palm_states("on_threshold", shape, 100)
    rays, tags = [], []
    for k in range(100):
        r = mixed_rays(rng, 1)[:, 0]
        for i in range(5):
            r[i] = (MEMBER_VALUES + OTHER_VALUES)[int(rng.integers(6))]
        r[k % 5] = F06
        if k >= 50:                                  # ... and alone: without it the sensor reads "none"
            r[:5] = [ABOVE, 0.1, -1.0, 0.1, ABOVE]
            r[k % 5] = F06
        rays.append(r); tags.append(("ray", k % 5, "alone" if k >= 50 else "among others"))
    return _finish("on_threshold", shape, snaps, rays, None, None, tags)


def palm_ray_decidable(rays):
    """[n] bool of rays [17, n]: every palm ray is a miss or farther from 0.06 than the fp32 ray tolerance of tests/ray_poses.py"""
    from tests import ray_poses as rp
    pr = np.asarray(rays)[:5]
    return ((pr < 0) | (np.abs(pr - 0.06) > rp.FP32_TOL * 1.06)).all(0)


def palm_subset(rays):
    """[n] int of rays [17, n]: bit i set where palm ray i is a hit below 0.06"""
    pr = np.asarray(rays)[:5]
    return (((pr >= 0) & (pr < 0.06)) * (1 << np.arange(5))[:, None]).sum(0)


def palm_object(shape="CubeS"):
    from oracle import ko_py as ko
    from tests import ray_poses as rp
    rng, mdl = rng_for("palm_object", shape), ko.OracleModel(scenarios.model_blob(shape))
    snaps, qs, hqs, tags, held = [], [], [], [], {}
    for i in range(PALM_DRAWS):
        q, hq = base_state(shape, POSES[i % 3], rng, closure=rng.uniform(0.0, 0.5, 3))
        far = q.copy()
        far[9:12] = cp.FAR
        _, pnt, vec = rp._oracle_reset(mdl, hq, far)
        k = i % 5
        beside = rng.normal(size=3)
        beside -= vec[k] * (beside @ vec[k])
        q[12:16] = f32(unit_quat(rng))
        q[9:12] = f32(pnt[k] + rng.uniform(*PALM_T) * vec[k] + rng.uniform(0.0, PALM_BESIDE) * beside / np.linalg.norm(beside))
        rays = rp._oracle_reset(mdl, hq, q)[0][:, None]
        sub = int(palm_subset(rays)[0])
        if not palm_ray_decidable(rays)[0] or held.get(sub, 0) >= PALM_EACH:
            continue
        held[sub] = held.get(sub, 0) + 1
        snaps.append(snapshot(shape, hq, q)); qs.append(q); hqs.append(hq); tags.append(("subset", sub, "along ray", k))
    return _finish("palm_object", shape, snaps, None, qs, hqs, tags)


def _rotation_onto(a, b):
    """the rotation that takes unit vector a to unit vector b"""
    v, c = np.cross(a, b), float(a @ b)
    if c < -1 + 1e-12:
        p = np.cross(a, [1.0, 0, 0] if abs(a[0]) < 0.9 else [0, 1.0, 0])
        p /= np.linalg.norm(p)
        return 2 * np.outer(p, p) - np.eye(3)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + K + K @ K / (1 + c)


def gravity_axis(shape="CubeS"):
    """the hand quaternion turned so that g = T3 (0, 0, -1) is the drawn direction, the object carried along (same pose relative to the hand);
    the slides then move the hand along turned axes, and the kinematics are the oracle's"""
    rng, M = rng_for("gravity_axis", shape), model(shape)
    targets = []
    for a in range(3):
        for s in (-1.0, 1.0):
            for i in range(20):
                g = rng.uniform(-0.6, 0.6, 3)
                g[a] = s
                targets.append((g, ("clear", a, s)))
            for b in range(3):
                if b != a:
                    for tie in TIES:
                        for i in range(2):
                            g = rng.uniform(-0.3, 0.3, 3)
                            g[a], g[b] = s, (1 - tie) * (1 if i else -1)
                            targets.append((g, ("tie", a, b, tie)))
    snaps, qs, hqs, tags = [], [], [], []
    for i, (g, tag) in enumerate(targets):
        q, hq = base_state(shape, POSES[i % 3], rng)
        s0 = snapshot(shape, hq, q)
        T3, _ = wrist_frame(M, s0)
        R7, p7 = body(s0, 2)
        Q = mc.quat_to_mat(z_turn(rng.uniform(0, 2 * np.pi))) @ _rotation_onto(T3.T @ (g / np.linalg.norm(g)), np.array([0.0, 0, -1]))
        hq2 = f32(mc.mat_to_quat(Q @ mc.quat_to_mat(hq / np.linalg.norm(hq))))
        q[0:3] = 0.0                                  # the hand's origin stays where the slides' zero puts it
        s1 = snapshot(shape, hq2, q)
        R7b, p7b = body(s1, 2)
        Qe = R7b @ R7.T                               # the turn the fp32 quaternion realises
        Ro, po = body(s0, 9)
        q[9:12] = p7b + Qe @ (po - p7)
        q[12:16] = mc.mat_to_quat(Qe @ Ro)
        q = f32(q)
        snaps.append(snapshot(shape, hq2, q)); qs.append(q); hqs.append(hq2); tags.append(tag)
    return _finish("gravity_axis", shape, snaps, None, qs, hqs, tags)


def finger_fans(shape="CubeS"):
    rng = rng_for("finger_fans", shape)
    closures = []
    for c in np.linspace(0.0, 2.0, 21):
        closures.append(((c, c, c), ("symmetric", round(float(c), 2))))
    for f in range(3):
        for c in np.linspace(0.0, 1.5, 7):
            for ahead in (0.05, 0.2, 0.5):
                cl = [c, c, c]
                cl[f] = min(2.0, c + ahead)
                closures.append((tuple(cl), ("ahead", f, round(float(c), 2), ahead)))
    for f in range(3):                               # the extremes of the range, one finger against the other two
        for lo, hi in ((0.0, 2.0), (2.0, 0.0)):
            cl = [lo, lo, lo]
            cl[f] = hi
            closures.append((tuple(cl), ("extreme", f, lo, hi)))
    snaps, qs, hqs, tags = [], [], [], []
    for i, (cl, tag) in enumerate(closures):
        for pose in POSES:
            q, hq = base_state(shape, pose, rng, closure=cl)
            if i % 2:
                q[4:9:2] = f32(rng.uniform(0.0, 2.0, 3))          # the distal joints anywhere in their range
            snaps.append(snapshot(shape, hq, q)); qs.append(q); hqs.append(hq); tags.append(tag + (pose,))
    return _finish("finger_fans", shape, snaps, None, qs, hqs, tags)


def object_bearing(shape):
    rng, M = rng_for("object_bearing", shape), model(shape)
    spots = []
    for side in BEARING_SIDES:
        for comp in (0, 2):
            for sgn in (-1.0, 1.0):
                for k in range(2):
                    ol = np.array([0.0, rng.uniform(0.03, 0.12), 0.0])
                    ol[comp], ol[2 - comp] = sgn * side, rng.uniform(-0.04, 0.04)
                    spots.append((ol, ("beside", comp, side)))
    for y in (-0.01, -0.05, -0.1):
        for k in range(12):
            spots.append((np.array([rng.uniform(-0.05, 0.05), y, rng.uniform(-0.05, 0.05)]), ("behind", y)))
        for side in (1e-6, 1e-4):                    # ... and on the centre line behind the palm: both angles near pi
            spots.append((np.array([side, y, -side]), ("behind on the line", y, side)))
    for y in (0.0, 1e-7, -1e-7, 1e-6, -1e-6):
        for k in range(8):
            spots.append((np.array([rng.choice([-1, 1]) * rng.uniform(0.03, 0.08), y, rng.choice([-1, 1]) * rng.uniform(0.03, 0.08)]), ("abreast", y)))
    snaps, qs, hqs, tags = [], [], [], []
    for i, (ol, tag) in enumerate(spots):
        q, hq = base_state(shape, POSES[i % 3], rng)
        T3, wrist = wrist_frame(M, snapshot(shape, hq, q))
        q[12:16] = f32(unit_quat(rng))
        Ro = mc.quat_to_mat(q[12:16] / np.linalg.norm(q[12:16]))
        q[9:12] = f32(wrist + T3.T @ ol - Ro @ M["geom_pos"][8])
        snaps.append(snapshot(shape, hq, q)); qs.append(q); hqs.append(hq); tags.append(tag)
    return _finish("object_bearing", shape, snaps, None, qs, hqs, tags)


def twentieth_power(shape):
    """snapshot edits: hand and object translated in x, y (a rigid move of the scene, then the object on its own)"""
    rng, M = rng_for("twentieth_power", shape), model(shape)
    snaps, tags = [], []
    for r in (1e-3, 1e-2, 1e-1):
        for d in np.concatenate([np.linspace(0.05, 0.95, 19), [0.99, 0.999, 1.0]]):
            for k in range(3):
                q, hq = base_state(shape, POSES[k], rng)
                q[12:16] = f32(unit_quat(rng))
                s = snapshot(shape, hq, q)
                _, p7 = body(s, 2)
                gap = np.arccos(d)
                beta = rng.uniform(0.0, np.pi / 2 - gap)
                alpha = beta + gap
                if rng.random() < 0.5:
                    alpha, beta = beta, alpha
                sg = rng.choice([-1.0, 1.0], 4)
                hand = r * np.array([np.cos(beta) * sg[0], np.sin(beta) * sg[1]])
                shift = hand - p7[:2]
                for b in range(2, 9):
                    s[(b - 2) * 12 + 9:(b - 2) * 12 + 11] += shift
                Ro, po = body(s, 9)
                ow = po + Ro @ M["geom_pos"][8]
                rho = rng.uniform(0.03, 0.15)
                want = hand + rho * np.array([np.cos(alpha) * sg[2], np.sin(alpha) * sg[3]])
                po[:2] += want - ow[:2]
                put_body(s, 9, Ro, po)
                snaps.append(s); tags.append(("r", r, "d", round(float(d), 3)))
    return _finish("twentieth_power", shape, snaps, None, None, None, tags)


def ranges(shape="CubeS"):
    rng, snaps = _palm_states("ranges", shape, 120)
    rays, tags = [], []
    for k in range(120):
        kind = ("all miss", "all zero", "5.99 and 6", "mixed with 5.99 and 6")[k % 4]
        r = {0: np.full(17, -1.0), 1: np.zeros(17), 2: np.where(rng.random(17) < 0.5, 5.99, 6.0), 3: mixed_rays(rng, 1)[:, 0]}[k % 4]
        if k % 4 == 3:
            r[rng.integers(17, size=4)] = [5.99, 6.0, 5.99, 6.0]
        rays.append(r); tags.append((kind,))
    return _finish("ranges", shape, snaps, rays, None, None, tags)


@lru_cache(maxsize=None)
def oracle_rays(cls, shape):
    """[17, n]: the oracle's rangefinder distances (-1 = miss) at the states of a class that holds qpos and hand quaternion"""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import ko_py as ko
    from tests import ray_poses as rp
    s = states(cls, shape)
    assert s.qpos is not None
    mdl = ko.OracleModel(scenarios.model_blob(shape))
    with ThreadPoolExecutor(rp.threads()) as pool:
        out = list(pool.map(lambda i: rp._oracle_reset(mdl, s.hq[:, i], s.qpos[:, i])[0], range(s.qpos.shape[1])))
    return np.stack(out, 1)


def exact_snapshots(cls, shape):
    """[105, n] float64, NOT rounded: the oracle's kinematics of the class's qpos and hand quaternion - what an in-step path is held to"""
    s = states(cls, shape)
    return np.stack([snapshot(shape, s.hq[:, i], s.qpos[:, i]) for i in range(s.qpos.shape[1])], 1)


_BUILDERS = dict(lift_band=lift_band, palm_rays=palm_rays, palm_object=palm_object, on_threshold=on_threshold, gravity_axis=gravity_axis, finger_fans=finger_fans,
                 object_bearing=object_bearing, twentieth_power=twentieth_power, ranges=ranges)


def shapes_of(cls):
    return SHAPES.get(cls, ("CubeS",))


@lru_cache(maxsize=None)
def states(cls, shape) -> States:
    assert shape in shapes_of(cls), (cls, shape)
    return _BUILDERS[cls](shape)


def all_sets(multi_geom=None):
    """[(class, shape)]; multi_geom None: all, False / True: those of that library"""
    out = [(c, s) for c in CLASSES for s in shapes_of(c)]
    return [cs for cs in out if multi_geom is None or (cs[1] == MG_SHAPE) == multi_geom]
