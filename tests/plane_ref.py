"""The plane-hull contact rule of the fp64 oracle (oracle/ko_physics.c collide_plane_hull) restated in numpy float64, for the plane-pair tests
(tests/plane_poses.py, tests/test_plane_cpu.py, tests/test_gpu_plane_contacts.py).  Written from the rule, not from the kernels:

  ground plane z = 0, normal e_z; hull vertex v of a geom with world pose (R, p):  d(v) = p_z + (R^T e_z) . v
  1. sphere cull: p_z > rbound + margin -> no contact
  2. the deepest vertex; none within the margin -> no contact
  3. the first contact is the LOWEST-INDEX vertex within TIE_EPS = 1e-12 of the deepest
  4. one walk over all indices from 0: a vertex with d <= margin that is MORE than 0.3 rbound from every accepted vertex is accepted, until 4
  5. per contact: dist = d(v), pos = R v + p - 0.5 d e_z, normal e_z

`plane_pair` returns the ordered vertex indices with dist and pos; `probes` says whether that answer survives what single precision can
do to the inputs (DECIDABLE: the ordered list, SET-DECIDABLE: the set); `expected_env` merges the plane pairs of this reference with the hull
pairs of the oracle's own list in pair order and cuts at the library's capacity.  Nothing here reads a kernel's output."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

PLANE_MESH_TOL = 0.3
TIE_EPS = 1e-12
BAND = 2e-6                 # the fp32 contact-distance tolerance (= contact_poses.BAND: tests/test_plane_cpu.py)
TILT = 2e-7                 # rad: what fp32 leaves of a rotation (entries of magnitude <= 1 at 2^-24 relative, a few chained products)
SPACING = 1e-5              # relative: the fp32 error of |v - w|^2 against (0.3 rbound)^2 is a few 2^-24; 1e-5 is two orders above it
E_Z = np.array([0.0, 0.0, 1.0])

PlaneContacts = namedtuple("PlaneContacts", "idx dist pos")
EMPTY = PlaneContacts(np.zeros(0, dtype=int), np.zeros(0), np.zeros((0, 3)))


def vertex_dist(R, p, V):
    """signed distance of every hull vertex to the plane"""
    return p[2] + V @ R[2]


def select(d, V, rbound, margin, spacing_scale=1.0):
    """steps 2 - 4 on the vertex distances d: the ordered vertex indices (at most 4)"""
    bd = d.min()
    if bd > margin:
        return []
    chosen = [int(np.flatnonzero(d <= bd + TIE_EPS)[0])]
    thr2 = (PLANE_MESH_TOL * rbound * spacing_scale) ** 2
    for i in np.flatnonzero(d <= margin):                       # the walk over all indices; only those within the margin can be accepted
        if len(chosen) == 4:
            break
        if all(((V[i] - V[c]) ** 2).sum() > thr2 for c in chosen):
            chosen.append(int(i))
    return chosen


def plane_pair(R, p, V, rbound, margin, spacing_scale=1.0) -> PlaneContacts:
    """the contacts of the ground plane with the hull V [nv, 3] of a geom at world pose (R [3, 3], p [3])"""
    R, p, V = np.asarray(R, dtype=np.float64), np.asarray(p, dtype=np.float64), np.asarray(V, dtype=np.float64)
    if p[2] > rbound + margin:
        return EMPTY
    d = vertex_dist(R, p, V)
    idx = select(d, V, rbound, margin, spacing_scale)
    if not idx:
        return EMPTY
    idx = np.array(idx, dtype=int)
    dist = d[idx]
    pos = V[idx] @ R.T + p - 0.5 * dist[:, None] * E_Z
    return PlaneContacts(idx, dist, pos)


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]]) if axis == 0 else np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def probes(R, p, V, rbound, margin):
    """(decidable, set_decidable) of a plane pair: its ordered vertex list / its vertex set from `plane_pair` unchanged with
    p_z +- BAND, R tilted by +- TILT about both horizontal axes (about the geom's origin), and the spacing threshold scaled by 1 +- SPACING"""
    R, p = np.asarray(R, dtype=np.float64), np.asarray(p, dtype=np.float64)
    base = plane_pair(R, p, V, rbound, margin).idx.tolist()
    moved = [plane_pair(R, p + s * BAND * E_Z, V, rbound, margin) for s in (-1, 1)]
    moved += [plane_pair(_rot(ax, s * TILT) @ R, p, V, rbound, margin) for ax in (0, 1) for s in (-1, 1)]
    moved += [plane_pair(R, p, V, rbound, margin, 1 + s * SPACING) for s in (-1, 1)]
    lists = [m.idx.tolist() for m in moved]
    return all(l == base for l in lists), all(set(l) == set(base) for l in lists)


def plane_pairs_of(M):
    """[(pair index, geom)] of the model's plane pairs, in pair order"""
    P = np.asarray(M["pairs"])
    return [(k, int(P[k, 1])) for k in range(len(P)) if int(P[k, 0]) == 0]


def hull_of(M, g):
    return np.asarray(M[f"mesh{int(M['geom_mesh'][g])}_vert"], dtype=np.float64)[:, :3]


def expected_env(M, xmat, xpos, oracle_list, capacity):
    """The expected ordered record list of an env: the plane pairs from this reference on the oracle's geom poses (xmat [ngeom, 3, 3], xpos
    [ngeom, 3]), the hull pairs from the oracle's own list `oracle_list` (contact_poses.Oracle.contacts of a sim that dropped nothing),
    merged in pair order and cut at `capacity`.  Returns (records as the oracle's dict with `vertex` [n] added - the hull vertex of a
    plane record, -1 on a hull record -, number dropped, {geom: PlaneContacts} uncut)."""
    P = np.asarray(M["pairs"])
    rows, per_geom = [], {}
    for k in range(len(P)):
        g1, g2 = int(P[k, 0]), int(P[k, 1])
        if g1 == 0:
            pc = plane_pair(xmat[g2], xpos[g2], hull_of(M, g2), float(M["geom_rbound"][g2]), float(P[k, 4]))
            per_geom[g2] = pc
            rows += [((0, g2), pc.dist[j], E_Z, pc.pos[j], int(pc.idx[j])) for j in range(len(pc.idx))]
        else:
            hit = np.flatnonzero((oracle_list["pairs"] == (g1, g2)).all(1)) if len(oracle_list["pairs"]) else []
            rows += [((g1, g2), oracle_list["dist"][j], oracle_list["normal"][j], oracle_list["pos"][j], -1) for j in hit]
    dropped = max(0, len(rows) - capacity)
    rows = rows[:capacity]
    rec = dict(pairs=np.array([r[0] for r in rows], dtype=int).reshape(-1, 2), dist=np.array([r[1] for r in rows], dtype=np.float64),
               normal=np.array([r[2] for r in rows], dtype=np.float64).reshape(-1, 3), pos=np.array([r[3] for r in rows], dtype=np.float64).reshape(-1, 3),
               vertex=np.array([r[4] for r in rows], dtype=int))
    return rec, dropped, per_geom


def recover_vertices(rec, M, xmat, xpos, g):
    """The hull vertices a contact list names for plane pair (0, g): per record of that pair the vertex nearest to pos + 0.5 dist e_z under
    the oracle's pose, with the distance to it and to the second-nearest (what makes a record attributable: plane_poses.ATTRIBUTE)"""
    V = hull_of(M, g)
    k = np.flatnonzero((rec["pairs"] == (0, g)).all(1)) if len(rec["pairs"]) else np.zeros(0, dtype=int)
    idx, d1, d2 = [], [], []
    for j in k:
        local = xmat[g].T @ (rec["pos"][j] + 0.5 * rec["dist"][j] * E_Z - xpos[g])
        r = np.sqrt(((V - local) ** 2).sum(1))
        o = np.argpartition(r, 1)[:2]
        o = o[np.argsort(r[o])]
        idx.append(int(o[0])); d1.append(float(r[o[0]])); d2.append(float(r[o[1]]))
    return k, np.array(idx, dtype=int), np.array(d1), np.array(d2)
