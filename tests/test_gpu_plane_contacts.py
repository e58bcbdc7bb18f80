"""The plane-pair contacts of every stepping path of the compiled gfx950 kernels - collide_plane_hull as the 16-lane team runs it (the masked first
scan, the DPP arg-min, the tie rule rebuilt from the lanes' masks, the walk over the candidate bits, the ballot walk of hulls above 1024 vertices,
the four staging lanes, the dynamic staging slots of the multi-geom build), the plane culls in front of it and the row-scan merge behind it -
against the numpy restatement of the oracle's rule (tests/plane_ref.py) on the aimed poses of tests/plane_poses.py.  tests/test_plane_cpu.py holds
the reference to the oracle's C records and the host lane (the serial fallbacks) to the same assertions.

Contexts run with contact_tap, horizon 0 and frame_skip 1; per env set_state(qpos, 0, 0), ONE step, get_state(contacts=True): the contacts of a
step are those of the state it starts from.  All classes of a shape share one context per path (env e holds pose e of the concatenated sets; a
context with fewer envs than poses takes every k-th).

  fp64 ks_substep, fp64 ks_step       ordered vertex list of every plane pair equal to the reference, ties included; dist, pos 1e-9; the whole
                                      record list, its count and the overflow bit equal to the expected merged list
  fp32 ks_substep, ks_step 275 / 4099 ordered list on decidable pairs, vertex set on set-decidable pairs, on every pair the invariants no tie
                                      can touch (plane_poses.Tally); dist 2e-6, pos 1e-4; normal (0, 0, 1) bit for bit; |pos_z - 0.5 dist|;
                                      where every plane pair of the env is decidable the record list is the first `capacity` of the expected
                                      list and status bit 1 is set exactly when the expected list is longer
  all                                 status bit 1 on no env outside the overflow class, bits 2 and 4 never, everything finite
  across                              275 and 4099 envs return the same bits per pose; an env given another object by ks_reset_objects equals a
                                      fresh context of that object bit for bit
Run with -s for the table (recorded in profiles/plane_parity.txt)."""
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import contact_poses as cp, plane_poses as pp

pytestmark = pytest.mark.gpu

N_SHORT, N_LONG = 275, 4099
ACTION = (0.1, 0.3, -0.2, 0.4)           # any action: the contacts of the first substep precede its effect
Path = namedtuple("Path", "name precision kind n")
SUB64, STEP64 = Path("fp64 ks_substep", 64, "substep", 0), Path("fp64 ks_step", 64, "step", 0)
SUB32, SHORT, LONG = Path("fp32 ks_substep", 32, "substep", 0), Path("fp32 ks_step", 32, "step", N_SHORT), Path("fp32 ks_step", 32, "step", N_LONG)
PATHS = (SUB64, STEP64, SUB32, SHORT, LONG)
CASES = [(s, p) for s in pp.SHAPES for p in PATHS]
case_id = lambda v: f"{v.name} n{v.n}".replace(" ", "_") if isinstance(v, Path) else str(v)
_results = {}


def pose_list(shape, classes=None):
    """[(class, index in its set)] of the concatenated sets of a shape"""
    return [(c, i) for c in (classes or pp.classes(shape)) for i in range(len(pp.poses(shape, c).expected))]


def tiled(total, n):
    """index into the pose list of every env: one env per pose (n = 0), every k-th pose (n < total), or the list over and over"""
    n = n or total
    return np.arange(n) * total // n if n < total else np.arange(n) % total


def state_of(shape, plist, idx):
    q = np.stack([pp.poses(shape, plist[j][0]).qpos[:, plist[j][1]] for j in idx], 1)
    hq = np.stack([pp.poses(shape, plist[j][0]).hand_quat[:, plist[j][1]] for j in idx], 1)
    return torch.as_tensor(q), torch.as_tensor(hq)


def put(sim, q, hq, **kw):
    sim.reset(q, hq, **kw)


def zeros(k):
    return torch.zeros((15, k), dtype=torch.float64)


def tap(sim, M):
    """per env (contact records as contact_poses.records, status word); state finite"""
    st = sim.get_state(contacts=True)
    torch.cuda.synchronize()
    status, ncon = st["status"].cpu().numpy(), st["ncon"].cpu().numpy()
    con = st["contact"].double().cpu().numpy()
    assert np.isfinite(st["qpos"].double().cpu().numpy()).all() and np.isfinite(st["qvel"].double().cpu().numpy()).all()
    return [(cp.records(M[e] if isinstance(M, list) else M, int(ncon[e]), con[:, :, e]), int(status[e])) for e in range(sim.n_envs)]


def advance(sim, kind, n):
    if kind == "substep":
        sim.substep(torch.zeros((9, n), dtype=torch.float64))
    else:
        sim.step(torch.as_tensor(np.repeat(np.array(ACTION)[:, None], n, 1)))


def run_path(shape, path):
    if (shape, path) in _results:
        return _results[shape, path]
    from kinovagrasping_amd.sim import KinovaSim
    plist, M = pose_list(shape), cp._oracle(shape).M
    idx = tiled(len(plist), path.n)
    n = len(idx)
    sim = KinovaSim(n, shape, precision=path.precision, frame_skip=1, horizon=0, contact_tap=True)
    assert sim.multi_geom == cp.on_mg_library(shape) and sim.ncon_max == pp.capacity(shape)
    q, hq = state_of(shape, plist, idx)
    put(sim, q, hq)
    sim.set_state(q, zeros(n), zeros(n))
    advance(sim, path.kind, n)
    out = (idx, tap(sim, M))
    sim.close()
    _results[shape, path] = out
    return out


def compare(shape, plist, idx, got, precision, name):
    """every pose once (its first env) against the reference; the other envs of the pose must hold the same bits"""
    tallies = {c: pp.Tally(pp.poses(shape, c), precision, name) for c in dict.fromkeys(c for c, _ in plist)}
    first = {}
    for e, j in enumerate(idx):
        if j in first:
            assert cp.same_bits(got[e][0], got[first[j]][0]) and got[e][1] == got[first[j]][1], (name, "envs of one pose differ", int(e), first[j])
            continue
        first[j] = e
        c, i = plist[j]
        tallies[c].add(i, *got[e])
    for t in tallies.values():
        print(t.line())
    return tallies


@pytest.mark.parametrize("shape,path", CASES, ids=case_id)
def test_plane_contacts_of_every_gpu_path_match_the_reference(shape, path):
    plist = pose_list(shape)
    idx, got = run_path(shape, path)
    tallies = compare(shape, plist, idx, got, path.precision, f"{path.name} n={len(idx)}")
    for c, t in tallies.items():
        if path.n == 0 or path.n >= len(plist):
            assert t.poses == len(pp.poses(shape, c).expected)
        t.check()
    assert sum(t.overflowed for t in tallies.values()) >= (5 if shape in pp.STANDARD_SHAPES else 0)


@pytest.mark.parametrize("shape", pp.SHAPES)
def test_short_and_long_contexts_return_the_same_bits(shape):
    plist = pose_list(shape)
    (ia, a), (ib, b) = run_path(shape, SHORT), run_path(shape, LONG)
    where = {int(j): e for e, j in reversed(list(enumerate(ib)))}
    for e, j in enumerate(ia):
        assert cp.same_bits(a[e][0], b[where[int(j)]][0]) and a[e][1] == b[where[int(j)]][1], (plist[j], e, where[int(j)])


@pytest.mark.parametrize("shapes", [("CylinderB", "CubeS"), ("BottleS", "BowlS")], ids=lambda s: "-".join(s))
def test_envs_given_another_object_scan_that_objects_hull(shapes):
    """A mixed-object context steps the first object's poses; ks_reset_objects then gives every third env the second object.  Those envs' plane
    pair of the object must scan the SECOND object's hull table (142 against 24 vertices, 1546 against at most 533): they equal a fresh context
    of the second object bit for bit and meet the reference; the envs beside them keep meeting the reference of the first."""
    from kinovagrasping_amd.sim import KinovaSim
    first, second = shapes
    la, lb = pose_list(first, pp.OBJECT_CLASSES), pose_list(second, pp.OBJECT_CLASSES)
    Ma, Mb = cp._oracle(first).M, cp._oracle(second).M
    n = N_SHORT
    ia = tiled(len(la), n)
    ids = np.arange(0, n, 3, dtype=np.int32)
    ib = tiled(len(lb), len(ids))
    act = torch.as_tensor(np.repeat(np.array(ACTION)[:, None], n, 1))
    qa, ha = state_of(first, la, ia)
    qb, hb = state_of(second, lb, ib)
    mixed = KinovaSim(n, list(shapes), frame_skip=1, horizon=0, contact_tap=True)
    put(mixed, qa, ha)
    mixed.set_state(qa, zeros(n), zeros(n))
    mixed.step(act)
    put(mixed, qa, ha)
    put(mixed, qb, hb, env_ids=torch.as_tensor(ids), object_id=np.ones(len(ids), dtype=np.int32))
    q = qa.clone()
    q[:, torch.as_tensor(ids.astype(np.int64))] = qb
    mixed.set_state(q, zeros(n), zeros(n))
    alone = KinovaSim(len(ids), second, frame_skip=1, horizon=0, contact_tap=True)
    put(alone, qb, hb)
    alone.set_state(qb, zeros(len(ids)), zeros(len(ids)))
    mixed.step(act)
    alone.step(act[:, :len(ids)])
    models = [Mb if e in set(ids.tolist()) else Ma for e in range(n)]
    got_m, got_a = tap(mixed, models), tap(alone, Mb)
    mixed.close(); alone.close()
    for k, e in enumerate(ids):
        assert cp.same_bits(got_m[e][0], got_a[k][0]) and got_m[e][1] == got_a[k][1], int(e)
    keep = np.setdiff1d(np.arange(n), ids)
    tb = compare(second, lb, ib, [got_m[e] for e in ids], 32, f"fp32 ks_step given {second} after {first}")
    ta = compare(first, la, ia[keep], [got_m[e] for e in keep], 32, f"fp32 ks_step beside them ({first})")
    for t in list(tb.values()) + list(ta.values()):
        t.check()
