"""Aimed contact poses for the narrow-phase tests (tests/test_contacts_cpu.py, tests/test_gpu_contacts.py) with the fp64 oracle's contact
list for each - the analogue of tests/ray_poses.py for gjk_distance / mpr_penetration_sm / mpr_penetration_pair / gjk_distance_f64.

The rest of the suite meets the narrow phase in the states one scripted grasp happens to visit.  The classes below put ONE hand-object hull
pair (the aimed pair) at a chosen signed gap and on a chosen feature of the object's hull:

  gap_ladder   a state of the oracle's close-and-lift grasp in which a hand geom touches the object; the object is slid along that
               contact's normal until the aimed pair's signed gap is each rung of RUNGS (millimetres of penetration, through +-3 um, to
               a few hundred um of separation)
  feature      the same ladder after the object has been turned about the contact point so that a vertex / an edge midpoint / a face
               centre tilted 1 - 3 degrees away from parallel (in turn) of its hull meets the link
  parallel     a face of the object's hull exactly parallel to a face of the link's hull (the pad), centre on centre: the documented tie
               class - MPR ends on one triangle of a flat Minkowski facet and rounding decides which (tests/test_kernel_source_cpu.py:
               same_contact_points) - so the contact POINT is reported, not asserted
  hand_margin  no object in reach: the fingers closed until two HAND geoms (finger against finger, finger against palm: pairs with the 1 mm
               geom margin) stand at each rung of MARGIN_RUNGS, set by bisection on the finger joints.  The object pairs have no margin, so
               their distance query only decides separated / overlap; these pairs' margin-zone records are what the fp32 build reads off
               gjk_distance's final simplex (distance, normal, point) - the only use of its termination test's absolute floor KS_GJK_GAP.
               Asserted: pair list and distance (2e-6); the POINT is reported (two finger pads side by side are near-parallel faces: the closest
               pair of points is not unique); the NORMAL of a margin-zone record (dist > 0) of the standard build to 3.5e-3 = 0.2 degrees, the
               figure tests/test_gpu_obs_contacts.py records for the closest-feature normals of near-touching pairs (the fp32 query stops on a
               distance test - 1e-6 relative + KS_GJK_GAP - which settles the distance, not the direction between two near-parallel pads;
               measured here: 1.4e-3 on the MI355X, 1.8e-3 on the host lane); the multi-geom build (fp64 distance query) and every penetrating
               record keep 2e-4.  The set does not depend on the object (parked far away): the tests run it on one shape per library.

Seeds: per hand pose (normal / top / rotated) SEEDS states of the in-hand grasp script of tests/test_multi_geom_cpu.py; a hand pose whose
script touches the object in too few states is filled up with the `normal` pose's seeds carried over rigidly (the object keeps its pose
relative to the palm).  Negative rungs are set by iterating on the oracle's own distance of the aimed pair; a positive rung g is the -3 um
pose moved (3 um + g) further out, because a margin-0 pair has no contact record once it is apart.

A pose is DECIDABLE when the oracle returns the same pair list at the pose and with the object moved +-2e-6 m along the approach normal:
2e-6 is the project's fp32 contact-distance tolerance, and a distance error within it can flip a contact's presence only inside that band.
Pair lists and counts are asserted on decidable poses only.

UNSETTLED records.  Every pose also carries the oracle's contact lists with the object moved +-1e-7 m along the approach normal and two tangents
(`alts`; hand_margin: every finger joint moved by what changes the aimed gap by 1e-7 m).  1e-7 m is what single precision leaves of a geom's pose:
2^-24 relative on coordinates of a few tenths of a metre, through a handful of chained transforms.  A record whose oracle normal moves by more than the
fp32 normal bound (2e-4) under such a move is unsettled - the oracle itself gives another answer on the pose an fp32 kernel sees:
  * a shallow penetration or a margin-zone record a few um deep / apart: the normal turns continuously with a sideways move, by about 1e-7 / |dist|
    (measured on the oracle: 3e-3 at 30 um, 7e-3 at 10 um, 2e-2 at 3 um, on the bottle's pieces and the lemon);
  * the origin ray of the penetration query on an edge between two Minkowski facets (seen: Vase1S, a face tilted 2 degrees at 30 um depth, normal
    3e-3 away after 0.1 um) - the tie of the `parallel` class one facet over.
An fp32 record beyond the plain bounds there must be within the bounds (normal 2e-4, point 1e-4) of the oracle's record at one of the moved poses, or
within the plain bound PLUS the largest change of the oracle's own record over the moves; otherwise it fails.  The allowance is per record: a settled
record of the same pose (the aimed object contact beside a jumping hand-hand normal, say) keeps the plain bounds.
Settled records (all but 0 - 3 % of a set) are held to the plain bounds; fp64 paths are held to the plain bounds everywhere.  `conditioned` [n]
(no unsettled record in the pose) is a statistic, capped at 15 % of a set like the undecidable share.

`poses(shape, cls)` returns a ContactPoses: qpos [16, n], hand_quat [4, n], ref (per pose the oracle's contacts: pairs [nc, 2], dist, normal
[nc, 3], pos [nc, 3]), decidable [n], conditioned [n], alts (per pose the oracle's lists at the moved poses that keep the pair list), near [n] (the aimed pair is apart by less than 1e-5 m: absent here, present 1e-5 further in - or a
margin-zone record with 0 < dist < 1e-5), aimed [n, 2] (its geoms), rung [n] and kind [n]."""
from __future__ import annotations

import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

from kinovagrasping_amd import model_compiler as mc, scenarios
from kinovagrasping_amd.sim import SOLVER_ITERATIONS
from oracle import ko_py as ko

RUNGS = (-3e-3, -3e-4, -3e-5, -1e-5, -3e-6, 3e-6, 1e-5, 3e-5, 3e-4)
STANDARD_SHAPES = ("CubeS", "CylinderB", "Cone1S", "Vase1S")        # libkinova_sim.so
MULTI_GEOM_SHAPES = ("BowlS", "BottleS")                            # libkinova_sim_mg.so: welded pieces, margin-zone contacts
MG_SINGLE_GEOM = "LemonS"                                           # one geom, but a 2434-vertex hull: libkinova_sim_mg.so, ids beyond the 10-bit pair memory
MG_LIBRARY_SHAPES = MULTI_GEOM_SHAPES + (MG_SINGLE_GEOM,)
SHAPES = STANDARD_SHAPES + MG_LIBRARY_SHAPES
OBJECT_CLASSES = ("gap_ladder", "feature", "parallel")
CLASSES = OBJECT_CLASSES + ("hand_margin",)
MARGIN_RUNGS = (-3e-4, -3e-5, -3e-6, 3e-6, 1e-5, 3e-5, 1e-4, 3e-4, 8e-4)
FAR = (5.0, 5.0, 5.0)
NAMED_POSES = ("normal", "top", "rotated")
SEEDS = 7                       # per hand pose: 3 x 7 x len(RUNGS) = 189 poses per (shape, class)
BAND = 2e-6                     # decidability band = the fp32 contact-distance tolerance
PROBE = 1e-7                    # what fp32 leaves of a geom pose (see CONDITIONED above)
NEAR = 1e-5
UNDECIDABLE_CAP = 0.15
NCON_MAX_MG = 40                # contact records libkinova_sim_mg.so keeps for every model it loads

ContactPoses = namedtuple("ContactPoses", "shape cls qpos hand_quat ref decidable conditioned alts near aimed rung kind")


def on_mg_library(shape: str) -> bool:
    return shape in MG_LIBRARY_SHAPES


class Oracle:
    """one oracle sim per hand pose of a shape, rays off: contacts of a pose = set_state; forward; contacts"""

    def __init__(self, shape):
        self.shape = shape
        blob = scenarios.model_blob(shape)
        self.model, self.M = ko.OracleModel(blob), mc.read_blob(blob)
        self.sims = {}

    def sim(self, hq):
        key = tuple(np.asarray(hq, dtype=np.float64))
        if key not in self.sims:
            o = ko.OracleSim(self.model, np.array(key), solver_iterations=SOLVER_ITERATIONS, ncon_max=NCON_MAX_MG if on_mg_library(self.shape) else None)
            o.s.rays_enabled = 0
            self.sims[key] = o
        return self.sims[key]

    def contacts(self, hq, qpos):
        o = self.sim(hq)
        o.set_state(qpos, np.zeros(15), np.zeros(15))
        o.forward()
        cs = o.contacts()
        return dict(pairs=np.array([(c["geom1"], c["geom2"]) for c in cs], dtype=int).reshape(-1, 2), dist=np.array([c["dist"] for c in cs]),
                    normal=np.array([c["frame"][:3] for c in cs]).reshape(-1, 3), pos=np.array([c["pos"] for c in cs]).reshape(-1, 3))

    def geom_pose(self, hq, qpos, g):
        o = self.sim(hq)
        o.set_state(qpos, np.zeros(15), np.zeros(15))
        o.forward()
        return o.view("geom_xmat").reshape(-1, 3, 3)[g].copy(), o.view("geom_xpos").reshape(-1, 3)[g].copy()


def pair_dist(ref, pair):
    """distance of the (first) record of `pair` in an oracle contact list, None when the pair has none"""
    hit = np.flatnonzero((ref["pairs"] == pair).all(1)) if len(ref["pairs"]) else []
    return float(ref["dist"][hit[0]]) if len(hit) else None


def hand_object(ref):
    """indices of the hull contacts between a hand geom (1 - 7) and the object or one of its pieces (8 ..)"""
    return np.flatnonzero((ref["pairs"][:, 0] >= 1) & (ref["pairs"][:, 1] >= 8)) if len(ref["pairs"]) else np.zeros(0, dtype=int)


def moved(qpos, t, n):
    q = qpos.copy()
    q[9:12] += t * n
    return q


# ---- seeds -----------------------------------------------------------------------------------------------------------------------
def _grasp_states(orc, pose):
    """(qpos, contact index) of the in-hand close-and-lift script's states with a hand-object hull contact, every 5th substep"""
    M, hq = orc.M, scenarios.hand_quat_for(pose)
    q0 = np.zeros(16)
    q0[12] = 1.0
    q0[9:12] = -M["geom_pos"][8] * np.array([1.0, 1.0, 0.0])
    q0[0:3] = scenarios.hand_slide_offsets(pose, orc.shape, "pose")
    o = ko.OracleSim(orc.model, hq, solver_iterations=SOLVER_ITERATIONS)
    o.s.rays_enabled = 0
    o.set_state(q0)
    o.forward()
    ctrl = np.zeros(9)
    ctrl[6:9] = 0.6
    out = []
    for i in range(320):
        if i == 200:
            ctrl[4] = 0.4
        o.step(ctrl)
        if i % 5 == 4 and np.abs(o.view("qvel")[9:12]).max() < 1.0:
            q = o.view("qpos").copy()
            if len(hand_object(orc.contacts(hq, q))):
                out.append(q)
    return hq, out


def _carry_over(orc, q, hq_from, hq_to):
    """the state q of hand pose hq_from in hand pose hq_to: same joints, the object in the same pose relative to the palm"""
    Ra, pa = orc.geom_pose(hq_from, q, 1)
    Rb, pb = orc.geom_pose(hq_to, q, 1)
    Q = Rb @ Ra.T
    out = q.copy()
    out[9:12] = pb + Q @ (q[9:12] - pa)
    out[12:16] = mc.mat_to_quat(Q @ mc.quat_to_mat(q[12:16]))
    return out


@lru_cache(maxsize=None)
def _oracle(shape):
    return Oracle(shape)


@lru_cache(maxsize=None)
def seeds(shape):
    """[(hand pose name, hand quaternion, qpos, aimed contact of the oracle's list at qpos)] - SEEDS per hand pose, the aimed contact
    taking the hand-object contacts of a state in turn"""
    orc = _oracle(shape)
    own = {pose: _grasp_states(orc, pose) for pose in NAMED_POSES}
    out = []
    for pose in NAMED_POSES:
        hq, states = own[pose]
        if len(states) < SEEDS:
            hq_n, st_n = own["normal"]
            states = states + [_carry_over(orc, q, hq_n, hq) for q in st_n]
        states = [q for q in states if len(hand_object(orc.contacts(hq, q)))]
        assert len(states) >= SEEDS, (shape, pose, len(states))
        for k, j in enumerate(np.linspace(0, len(states) - 1, SEEDS).round().astype(int)):
            ref = orc.contacts(hq, states[j])
            ho = hand_object(ref)
            out.append((pose, hq, states[j], int(ho[k % len(ho)])))
    return out


# ---- placing the aimed pair at a signed gap --------------------------------------------------------------------------------------
def _calibrate(orc, hq, q, n, pair, target, t=0.0):
    """t such that the oracle's distance of `pair` at moved(q, t, n) is `target` (< 0), or None: the distance changes by dt when the
    object moves dt along the contact normal, so a few corrections by the residual land on it"""
    d, tries = pair_dist(orc.contacts(hq, moved(q, t, n)), pair), 0
    while d is None and tries < 60:                 # apart: move in until the pair has a record
        t -= 2e-4
        tries += 1
        d = pair_dist(orc.contacts(hq, moved(q, t, n)), pair)
    if d is None:
        return None
    for _ in range(8):
        if abs(d - target) < 1e-9:
            break
        t2 = t + (target - d)
        d2 = pair_dist(orc.contacts(hq, moved(q, t2, n)), pair)
        if d2 is None:
            t2 = t + 0.5 * (target - d)
            d2 = pair_dist(orc.contacts(hq, moved(q, t2, n)), pair)
            if d2 is None:
                return None
        t, d = t2, d2
    return t if abs(d - target) < 2e-7 else None


def _ladder(orc, hq, q, n, pair):
    """{rung: qpos} for the rungs that could be set"""
    out, t, t3 = {}, 0.0, None
    for g in sorted(r for r in RUNGS if r < 0):
        tt = _calibrate(orc, hq, q, n, pair, g, t)
        if tt is not None:
            out[g], t = moved(q, tt, n), tt
            t3 = tt if g == -3e-6 else t3
    if t3 is not None:
        for g in (r for r in RUNGS if r > 0):
            out[g] = moved(q, t3 + 3e-6 + g, n)
    return out


# ---- hull features ---------------------------------------------------------------------------------------------------------------
def _hull(M, g):
    s = int(M["geom_mesh"][g])
    V = np.asarray(M[f"mesh{s}_vert"], dtype=np.float64)[:, :3]
    return V, np.asarray(M[f"mesh{s}_adj_off"]), np.asarray(M[f"mesh{s}_adj"])


def _neighbours(off, adj, v):
    return [int(w) for w in adj[off[v]:off[v + 1]]]


def _faces_at(V, off, adj, v):
    """triangles (v, a, b) of mutually adjacent hull vertices with their outward unit normal and centre"""
    c0, nb, out = V.mean(0), _neighbours(off, adj, v), []
    for i, a in enumerate(nb):
        for b in nb[i + 1:]:
            if b in _neighbours(off, adj, a):
                nrm = np.cross(V[a] - V[v], V[b] - V[v])
                if np.linalg.norm(nrm) > 1e-14:
                    nrm /= np.linalg.norm(nrm)
                    ctr = (V[v] + V[a] + V[b]) / 3
                    out.append((nrm if nrm @ (ctr - c0) > 0 else -nrm, ctr))
    return out


def _rotation_onto(a, b):
    """the smallest rotation taking unit vector a onto unit vector b"""
    v, c = np.cross(a, b), float(a @ b)
    if np.linalg.norm(v) < 1e-12:
        if c > 0:
            return np.eye(3)
        p = np.cross(a, [1.0, 0, 0] if abs(a[0]) < 0.9 else [0, 1.0, 0])
        p /= np.linalg.norm(p)
        return 2 * np.outer(p, p) - np.eye(3)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + K + K @ K / (1 + c)


def _turned(q, Q, feat_world, target):
    """the object turned by Q and moved so that its point feat_world comes to lie on `target`"""
    out = q.copy()
    out[12:16] = mc.mat_to_quat(Q @ mc.quat_to_mat(q[12:16]))
    out[12:16] /= np.linalg.norm(out[12:16])
    out[9:12] = target - Q @ (feat_world - q[9:12])
    return out


def _feature_pose(orc, hq, q, ref, ci, kind, rng):
    """(qpos, approach normal): the object's hull feature nearest to contact ci - kind 0 vertex, 1 edge midpoint, 2 face centre tilted
    1 - 3 degrees - turned to face the link along the contact normal and put on the contact point"""
    g2, n, pc = int(ref["pairs"][ci, 1]), ref["normal"][ci], ref["pos"][ci]
    V, off, adj = _hull(orc.M, g2)
    Rg, pg = orc.geom_pose(hq, q, g2)
    v = int(np.argmin(((V - Rg.T @ (pc - pg)) ** 2).sum(1)))
    c0 = V.mean(0)
    if kind == 0:
        feat = V[v]
        u = (feat - c0) / np.linalg.norm(feat - c0)
    elif kind == 1:
        feat = 0.5 * (V[v] + V[_neighbours(off, adj, v)[0]])
        u = (feat - c0) / np.linalg.norm(feat - c0)
    else:
        faces = _faces_at(V, off, adj, v)
        if not faces:
            return None
        u, feat = faces[0]
        axis = np.cross(u, rng.normal(size=3))
        axis /= np.linalg.norm(axis)
        ang = np.deg2rad(rng.uniform(1.0, 3.0))
        u = u * np.cos(ang) + np.cross(axis, u) * np.sin(ang)
    Q = _rotation_onto(Rg @ u, -n)
    return _turned(q, Q, pg + Rg @ feat, pc), n


def _parallel_pose(orc, hq, q, ref, ci):
    """(qpos, approach normal = the link face's outward normal): a face of the object's hull parallel to the face of the link's hull that
    looks along the contact normal, centre on centre"""
    g1, g2, n, pc = int(ref["pairs"][ci, 0]), int(ref["pairs"][ci, 1]), ref["normal"][ci], ref["pos"][ci]
    Vh, offh, adjh = _hull(orc.M, g1)
    Rh, ph = orc.geom_pose(hq, q, g1)
    near = np.argsort(((Vh - Rh.T @ (pc - ph)) ** 2).sum(1))[:6]
    link = [f for v in near for f in _faces_at(Vh, offh, adjh, int(v))]
    V, off, adj = _hull(orc.M, g2)
    Rg, pg = orc.geom_pose(hq, q, g2)
    obj = _faces_at(V, off, adj, int(np.argmin(((V - Rg.T @ (pc - pg)) ** 2).sum(1))))
    if not link or not obj:
        return None
    m, cl = max(link, key=lambda f: float((Rh @ f[0]) @ n))
    m, cl = Rh @ m, ph + Rh @ cl
    uo, fo = max(obj, key=lambda f: float(-(Rg @ f[0]) @ n))
    Q = _rotation_onto(Rg @ uo, -m)
    return _turned(q, Q, pg + Rg @ fo, cl), m


def _alts(orc, hq, q, n, ref):
    """the oracle's contact lists with the object moved +-PROBE along n and two tangents, those that keep the pair list"""
    a = np.cross(n, [1.0, 0, 0] if abs(n[0]) < 0.9 else [0, 1.0, 0])
    a /= np.linalg.norm(a)
    out = [orc.contacts(hq, moved(q, s, v)) for v in (n, a, np.cross(n, a)) for s in (-PROBE, PROBE)]
    return [r for r in out if np.array_equal(r["pairs"], ref["pairs"])]


def spread(ref, alts, key="normal"):
    """per record the largest change of the oracle's own normal (or point) over the moved poses"""
    if not len(ref["dist"]) or not alts:
        return np.zeros(len(ref["dist"]))
    return np.max([np.abs(r[key] - ref[key]).max(1) for r in alts], axis=0)


def _settled(ref, alts):
    return bool((spread(ref, alts) <= BOUNDS[32]["normal"]).all())


# ---- hand against hand ------------------------------------------------------------------------------------------------------------
def hand_hand(ref):
    return np.flatnonzero((ref["pairs"][:, 0] >= 1) & (ref["pairs"][:, 1] <= 7)) if len(ref["pairs"]) else np.zeros(0, dtype=int)


def _fingers(a, b):
    q = np.zeros(16)
    q[12], q[9:12] = 1.0, FAR
    q[3:9] = [a, b, a, b, a, b]
    return q


def _hand_margin_poses(orc):
    """[(hq, qpos, pair, rung, slope)]: per hand pose, up to SEEDS brackets of the proximal angle a (distal angle b fixed) across which a hand-hand
    pair goes from apart (or absent) to overlapping; every rung by bisection on a.  slope = d gap / d a at the pose (m / rad), measured on the oracle
    over +-1e-5 rad (about 5e-7 m of gap: no rung is that close to touching)."""
    out = []
    for pose in NAMED_POSES:
        hq, brackets = scenarios.hand_quat_for(pose), []
        for b in np.linspace(0.0, 2.0, 11):
            grid = np.linspace(0.6, 1.9, 27)
            lists = [orc.contacts(hq, _fingers(a, b)) for a in grid]
            for k in range(len(grid) - 1):
                for ci in hand_hand(lists[k + 1]):
                    pair = lists[k + 1]["pairs"][ci]
                    d0, d1 = pair_dist(lists[k], pair), lists[k + 1]["dist"][ci]
                    if d1 < -3e-4 and (d0 is None or d0 > 8e-4) and not any((pair == p).all() and bb == b for _, _, bb, p in brackets):
                        brackets.append((grid[k], grid[k + 1], b, pair))
        pick = [brackets[j] for j in np.linspace(0, len(brackets) - 1, min(SEEDS, len(brackets))).round().astype(int)] if brackets else []
        for a0, a1, b, pair in pick:
            for g in MARGIN_RUNGS:
                lo, hi = a0, a1                               # dist(lo) > g (or no record), dist(hi) < g
                for _ in range(60):
                    mid = 0.5 * (lo + hi)
                    d = pair_dist(orc.contacts(hq, _fingers(mid, b)), pair)
                    lo, hi = (mid, hi) if (d is None or d > g) else (lo, mid)
                d = pair_dist(orc.contacts(hq, _fingers(hi, b)), pair)
                dm, dp = (pair_dist(orc.contacts(hq, _fingers(hi + s, b)), pair) for s in (-1e-5, 1e-5))
                if d is not None and abs(d - g) < 2e-7 and dm is not None and dp is not None and abs(dp - dm) > 1e-8:
                    out.append((hq, _fingers(hi, b), pair, g, (dp - dm) / 2e-5))
    return out


def _hand_margin_set(shape):
    orc = _oracle(shape)
    rows = _hand_margin_poses(orc)
    assert rows, (shape, "no hand-hand bracket")
    qs, hqs, refs, dec, cond, alts, near, aimed, rung = [], [], [], [], [], [], [], [], []
    proximal = np.r_[np.zeros(3), [1, 0, 1, 0, 1, 0], np.zeros(7)]
    for hq, q, pair, g, slope in rows:
        ref = orc.contacts(hq, q)
        # +-BAND of the aimed gap through the proximal joints (the bisection's variable); +-PROBE of it through every finger joint in turn
        lists = [orc.contacts(hq, q + s / abs(slope) * proximal)["pairs"] for s in (-BAND, BAND)]
        alt = []
        for j in range(3, 9):
            for s in (-PROBE / abs(slope), PROBE / abs(slope)):
                qq = q.copy()
                qq[j] += s
                r = orc.contacts(hq, qq)
                if np.array_equal(r["pairs"], ref["pairs"]):
                    alt.append(r)
        d = pair_dist(ref, pair)
        qs.append(q); hqs.append(hq); refs.append(ref); aimed.append(pair); rung.append(g); alts.append(alt)
        dec.append(all(np.array_equal(l, ref["pairs"]) for l in lists)); cond.append(_settled(ref, alt)); near.append(d is not None and 0 < d < NEAR)
    return ContactPoses(shape, "hand_margin", np.stack(qs, 1), np.stack(hqs, 1), refs, np.array(dec), np.array(cond), alts, np.array(near), np.array(aimed),
                        np.array(rung), np.zeros(len(qs), dtype=int))


# ---- the pose sets ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def poses(shape: str, cls: str) -> ContactPoses:
    assert cls in CLASSES and shape in SHAPES
    if cls == "hand_margin":
        return _hand_margin_set(shape)
    orc = _oracle(shape)
    qs, hqs, refs, dec, cond, alts, near, aimed, rung, kinds = [], [], [], [], [], [], [], [], [], []
    for k, (pose, hq, q, ci) in enumerate(seeds(shape)):
        rng = np.random.default_rng([zlib.crc32(shape.encode()), CLASSES.index(cls), k])
        ref0 = orc.contacts(hq, q)
        pair = ref0["pairs"][ci].copy()
        kind = k % 3
        if cls == "gap_ladder":
            placed = (q, ref0["normal"][ci])
        elif cls == "feature":
            placed = _feature_pose(orc, hq, q, ref0, ci, kind, rng)
        else:
            placed = _parallel_pose(orc, hq, q, ref0, ci)
        if placed is None:
            continue
        base, n = placed
        for g, qq in _ladder(orc, hq, base, n, pair).items():
            ref = orc.contacts(hq, qq)
            lists = [orc.contacts(hq, moved(qq, s, n))["pairs"] for s in (-BAND, BAND)]
            d, d_in = pair_dist(ref, pair), pair_dist(orc.contacts(hq, moved(qq, -NEAR, n)), pair)
            qs.append(qq); hqs.append(hq); refs.append(ref); aimed.append(pair); rung.append(g); kinds.append(kind)
            dec.append(all(np.array_equal(l, ref["pairs"]) for l in lists))
            alts.append(_alts(orc, hq, qq, n, ref))
            cond.append(_settled(ref, alts[-1]))
            near.append((d is None and d_in is not None) or (d is not None and 0 < d < NEAR))
    assert qs, (shape, cls, "no pose could be set")
    return ContactPoses(shape, cls, np.stack(qs, 1), np.stack(hqs, 1), refs, np.array(dec), np.array(cond), alts, np.array(near), np.array(aimed), np.array(rung), np.array(kinds))


def check_conditions(ps: ContactPoses):
    """what a pose set must offer, from the oracle alone (a wrong kernel cannot meet or miss them)"""
    n = len(ps.ref)
    assert n >= (60 if ps.cls == "hand_margin" else 100), (ps.shape, ps.cls, "poses", n)
    assert (~ps.decidable).mean() <= UNDECIDABLE_CAP, (ps.shape, ps.cls, "undecidable", int((~ps.decidable).sum()), n)
    assert (~ps.conditioned).mean() <= UNDECIDABLE_CAP, (ps.shape, ps.cls, "ill-conditioned", int((~ps.conditioned).sum()), n)
    which = hand_hand if ps.cls == "hand_margin" else hand_object
    deep = sum(int((r["dist"][which(r)] < 0).sum()) for r in ps.ref)
    assert deep >= 1, (ps.shape, ps.cls, "no penetrating hull contact of the aimed kind")
    assert ps.near.any(), (ps.shape, ps.cls, "no pose with the aimed pair apart by less than 1e-5 m")
    if ps.cls == "hand_margin":
        zone = sum(int((r["dist"][hand_hand(r)] > 0).sum()) for r in ps.ref)
        assert zone >= 0.5 * n, (ps.shape, ps.cls, "margin-zone hand-hand contacts", zone)
    elif ps.shape in MULTI_GEOM_SHAPES:
        zone = sum(int((r["dist"][hand_object(r)] > 0).sum()) for r in ps.ref)
        assert zone >= 1, (ps.shape, ps.cls, "no margin-zone contact")


# ---- the comparison both test files make -----------------------------------------------------------------------------------------
# fp64: tests/test_kernel_source_cpu.py same_contact_points; fp32: the header of tests/test_gpu_obs_contacts.py (distance 2e-6, normal 2e-4) and the
# bound under which that file calls two contact points the same (1e-4)
BOUNDS = {64: dict(dist=1e-9, normal=1e-7, point=1e-9), 32: dict(dist=2e-6, normal=2e-4, point=1e-4)}
MARGIN_ZONE_NORMAL_F32 = 3.5e-3     # 0.2 degrees: margin-zone normals of the fp32 distance query (hand_margin, standard build; see the module docstring)
HAND_MARGIN_SHAPES = ("CubeS", "BottleS")       # one per library: the class does not depend on the object


def records(M, ncon, con):
    """a kernel's contact records (rows of CON_STRIDE words: point, normal, distance, .., word 8 = bodies + 256 x pair index) as the oracle's dict"""
    c = np.asarray(con, dtype=np.float64)[:ncon]
    pi = (c[:, 8].astype(np.int64) // 256) if ncon else np.zeros(0, dtype=np.int64)
    return dict(pairs=np.asarray(M["pairs"])[pi, :2].astype(int).reshape(-1, 2), dist=c[:, 6].copy(), normal=c[:, 3:6].copy(), pos=c[:, 0:3].copy())


def margin0(M, rec):
    """the records of pairs without margin (the explicit object pairs: GJK only decides separated / overlap, the point comes from a cold MPR)"""
    pairs = np.asarray(M["pairs"])
    margin = {(int(a), int(b)): m for a, b, m in zip(pairs[:, 0], pairs[:, 1], pairs[:, 4])}
    keep = np.array([margin[tuple(p)] == 0 for p in rec["pairs"].tolist()], dtype=bool)
    return {k: v[keep] for k, v in rec.items()}


def same_bits(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in ("pairs", "dist", "normal", "pos"))


class Tally:
    """errors of one (shape, class, path) against the oracle; `failures` collects what the bounds of the class forbid"""

    def __init__(self, ps: ContactPoses, precision: int, path: str):
        self.ps, self.precision, self.path, self.b = ps, precision, path, BOUNDS[precision]
        self.dist, self.normal, self.point, self.failures = [], [], [], []
        self.poses = self.compared = self.hull = self.ties = self.list_differs = self.ill = 0

    def add(self, i, got):
        ps, b, ref = self.ps, self.b, self.ps.ref[i]
        self.poses += 1
        same = np.array_equal(got["pairs"], ref["pairs"])
        if not same:
            self.list_differs += 1
            if ps.decidable[i]:
                self.failures.append((i, "pair list", got["pairs"].tolist(), ref["pairs"].tolist(), float(ps.rung[i])))
            return
        if not np.isfinite(np.concatenate([got["dist"], got["normal"].ravel(), got["pos"].ravel()])).all():
            self.failures.append((i, "not finite"))
            return
        self.compared += 1
        self.hull += len(hand_object(ref)) + len(hand_hand(ref))
        if not len(ref["dist"]):
            return
        ed, en, ep = np.abs(got["dist"] - ref["dist"]), np.abs(got["normal"] - ref["normal"]).max(1), np.abs(got["pos"] - ref["pos"]).max(1)
        self.dist += ed.tolist(); self.normal += en.tolist(); self.point += ep.tolist()
        if ed.max() > b["dist"]:
            self.failures.append((i, "distance", float(ed.max()), float(ps.rung[i]), int(ps.kind[i])))
        point_reported = ps.cls in ("parallel", "hand_margin")                  # the tie classes: the point is counted, not asserted
        bn = np.full(len(en), b["normal"])
        if ps.cls == "hand_margin" and self.precision == 32 and not on_mg_library(ps.shape):
            bn[ref["dist"] > 0] = MARGIN_ZONE_NORMAL_F32
        bad = (en > bn) | ((ep > b["point"]) & (not point_reported))
        self.ties += int((ep > b["point"]).any())
        if bad.any() and self.precision == 32:
            # unsettled records (see the module docstring): the oracle's own answer on the pose an fp32 kernel sees
            alts = ps.alts[i]
            sn, sp = spread(ref, alts), spread(ref, alts, "pos")
            for k in np.flatnonzero(bad & (sn > b["normal"])):
                ok = (en[k] <= bn[k] + sn[k] and (point_reported or ep[k] <= b["point"] + sp[k])) or \
                     any(np.abs(got["normal"][k] - r["normal"][k]).max() <= b["normal"] and
                         (point_reported or np.abs(got["pos"][k] - r["pos"][k]).max() <= b["point"]) for r in alts)
                if ok:
                    bad[k] = False
                    self.ill += 1
        for k in np.flatnonzero(bad):
            self.failures.append((i, "normal / point", ref["pairs"][k].tolist(), float(ref["dist"][k]), float(en[k]), float(ep[k]), float(ps.rung[i]), int(ps.kind[i])))

    def line(self):
        f = lambda a: (f"{max(a):.1e}/{np.percentile(a, 99):.1e}" if a else "-")
        return (f"{self.ps.shape:10s} {self.ps.cls:10s} {self.path:34s} poses {self.poses:4d} decidable {self.ps.decidable.mean():.3f} lists equal {self.compared:4d} "
                f"hull contacts {self.hull:4d} worst/p99 dist {f(self.dist)} normal {f(self.normal)} point {f(self.point)} point beyond {self.ties / max(1, self.compared):.3f} "
                f"poses with an unsettled record {(~self.ps.conditioned).mean():.3f} (records passed on the oracle's moved poses: {self.ill})")
