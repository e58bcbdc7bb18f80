"""The hull-pair narrow phase of every stepping path of the compiled gfx950 kernels against the fp64 oracle on the aimed contact poses of
tests/contact_poses.py (gap ladders from millimetres of penetration through +-3 um to separation; vertex / edge / tilted-face features;
parallel faces).  tests/test_contacts_cpu.py holds the same bounds on the host lane of the kernel source and the generator's conditions on
the oracle alone.

Contexts run with contact_tap, horizon 0 and frame_skip 1.  Per env: set_state(qpos, 0, 0), ONE step, get_state(contacts=True): the contacts
of a step are those of the state it starts from, so they are the set pose's - the fp64 paths confirm it by meeting the oracle to round-off.

  path                               reached by
  fp64 ks_substep / fp64 ks_step     precision-64 context (template queries, cold)
  fp32 ks_substep                    k_substep: the one-lane penetration query (mpr_penetration_sm), cold
  fp32 ks_step, 275 / 4099 envs      k_env_step_f32: two-lane penetration query (mpr_penetration_pair), GJK warm-started from pair memory;
                                     a partly filled workgroup, and at 4099 more workgroups than compute units
  ... fresh / pair_memory=False / stale
                                     a new context; one that never remembers; one that first stepped the pose set shifted by half its length,
                                     so that every env remembers ANOTHER pose when it meets its own (memory carried across ks_reset and ks_set_state)
  ... after ks_reset_objects         a mixed-object context whose envs held another object (test_envs_given_another_object_*)
  the multi-geom build of all these  BowlS, BottleS, LemonS on libkinova_sim_mg.so (one-lane query, margin-zone contacts from the fp64 distance
                                     query, hull tables in global memory)

Bounds (tests/contact_poses.py): decidable poses - contact count and ordered pair list equal the oracle's; fp64 point and distance 1e-9, normal
1e-7, no exception; fp32 distance 2e-6, normal 2e-4, point 1e-4 on every record of gap_ladder and feature - except records the ORACLE marks
unsettled (its own normal moves by more than 2e-4 under a 0.1 um move of the object): those must be within the bounds of the oracle's record at one
of the moved poses, or within the bound plus the oracle's own change, record by record; parallel: list, distance and normal, the share of differing
points printed; hand_margin (CubeS and BottleS: one shape per library): list, distance, normal (margin-zone records of the standard build 3.5e-3).
Status bits non-finite and ray-pool time-out never set, everything finite.
Run with -s for the table (recorded in profiles/contact_parity.txt)."""
import time
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import contact_poses as cp

pytestmark = pytest.mark.gpu

N_SHORT, N_LONG = 275, 4099
ACTION = (0.1, 0.3, -0.2, 0.4)           # any action: the contacts of the first substep precede its effect
Path = namedtuple("Path", "name precision kind n memory")        # kind: "substep" | "step"; memory: "fresh" | "off" | "stale"
SUB64 = Path("fp64 ks_substep", 64, "substep", 0, "fresh")
STEP64 = Path("fp64 ks_step", 64, "step", 0, "fresh")
SUB32 = Path("fp32 ks_substep", 32, "substep", 0, "fresh")
FRESH = Path("fp32 ks_step fresh", 32, "step", N_SHORT, "fresh")
LONG = Path("fp32 ks_step fresh", 32, "step", N_LONG, "fresh")
NOMEM = Path("fp32 ks_step pair_memory=False", 32, "step", N_SHORT, "off")
STALE = Path("fp32 ks_step stale memory", 32, "step", N_SHORT, "stale")
PATHS = (SUB64, STEP64, SUB32, FRESH, LONG, NOMEM, STALE)
CASES = [(s, p) for s in cp.SHAPES for p in PATHS]
case_id = lambda v: f"{v.name} n{v.n}".replace(" ", "_") if isinstance(v, Path) else str(v)
_results, _t0 = {}, time.time()


def classes(shape):
    """hand_margin does not depend on the object: one shape per library carries it"""
    return cp.OBJECT_CLASSES + (("hand_margin",) if shape in cp.HAND_MARGIN_SHAPES else ())


def tiled(ps, n):
    """pose index of every env: env e holds pose e % len(poses); n = 0: one env per pose"""
    return np.arange(n or len(ps.ref)) % len(ps.ref)


def tap(sim, M):
    """per env the contact records of the last step as contact_poses.records, after the status checks (M: the model, or one per env: a record
    names its pair by the index in its env's own pair table)"""
    st = sim.get_state(contacts=True)
    torch.cuda.synchronize()
    status, ncon = st["status"].cpu().numpy(), st["ncon"].cpu().numpy()
    con = st["contact"].double().cpu().numpy()
    assert (status & 6 == 0).all(), ("status", np.flatnonzero(status & 6)[:10], status[status & 6 != 0][:10])
    assert np.isfinite(st["qpos"].double().cpu().numpy()).all() and np.isfinite(st["qvel"].double().cpu().numpy()).all()
    return [cp.records(M[e] if isinstance(M, list) else M, int(ncon[e]), con[:, :, e]) for e in range(sim.n_envs)]


def advance(sim, path, n):
    if path.kind == "substep":
        sim.substep(torch.zeros((9, n), dtype=torch.float64))
    else:
        sim.step(torch.as_tensor(np.repeat(np.array(ACTION)[:, None], n, 1)))


def put(sim, ps, idx):
    q, hq = torch.as_tensor(ps.qpos[:, idx].copy()), torch.as_tensor(ps.hand_quat[:, idx].copy())
    sim.reset(q, hq)
    sim.set_state(q, torch.zeros((15, len(idx)), dtype=torch.float64), torch.zeros((15, len(idx)), dtype=torch.float64))


def run_path(shape, path, cls):
    """per env the tapped contact records of `path` on the poses of (shape, cls) - cached: the cross-path test compares what the per-path tests
    compared with the oracle"""
    if (shape, path, cls) in _results:
        return _results[shape, path, cls]
    from kinovagrasping_amd.sim import KinovaSim
    ps, M = cp.poses(shape, cls), cp._oracle(shape).M
    idx = tiled(ps, path.n)
    n = len(idx)
    sim = KinovaSim(n, shape, precision=path.precision, frame_skip=1, horizon=0, contact_tap=True, pair_memory=path.memory != "off")
    assert sim.multi_geom == cp.on_mg_library(shape)
    if path.memory == "stale":
        put(sim, ps, (idx + len(ps.ref) // 2 + 1) % len(ps.ref))
        advance(sim, path, n)
    put(sim, ps, idx)
    advance(sim, path, n)
    out = tap(sim, M)
    sim.close()
    _results[shape, path, cls] = out
    return out


def compare(ps, idx, got, precision, name):
    tally = cp.Tally(ps, precision, name)
    for e, i in enumerate(idx):
        tally.add(int(i), got[e])
    print(tally.line())
    return tally


@pytest.mark.parametrize("shape,path", CASES, ids=case_id)
def test_contacts_of_every_gpu_path_match_the_oracle(shape, path):
    failures = []
    for cls in classes(shape):
        ps = cp.poses(shape, cls)
        cp.check_conditions(ps)
        idx = tiled(ps, path.n)
        tally = compare(ps, idx, run_path(shape, path, cls), path.precision, f"{path.name} n={len(idx)}")
        failures += [(cls,) + f for f in tally.failures]
        assert tally.compared >= 0.85 * tally.poses, (cls, tally.compared, tally.poses)
    print(f"  (tests/test_gpu_contacts.py: {time.time() - _t0:.0f} s since the module was loaded)")
    assert not failures, (len(failures), failures[:10])


@pytest.mark.parametrize("shape", cp.SHAPES)
def test_fresh_memoryless_and_stale_contexts_return_the_same_contacts(shape):
    """Standard library: the records of the pairs without margin (every object pair: GJK only decides separated / overlap there - a true
    certificate whatever simplex it started from - and the penetration query is cold) are bit for bit the same on decidable poses whether the
    context is new, never remembers, or remembers another pose.  Multi-geom library: a margin-zone contact is read off the remembered simplex'
    successor, so the three are held to the oracle bounds each (test_contacts_of_every_gpu_path_match_the_oracle) and the differences counted."""
    M, differs, total = cp._oracle(shape).M, [], 0
    for cls in classes(shape):
        ps = cp.poses(shape, cls)
        idx = tiled(ps, N_SHORT)
        fresh, others = run_path(shape, FRESH, cls), {p.name: run_path(shape, p, cls) for p in (NOMEM, STALE)}
        for name, got in others.items():
            for e, i in enumerate(idx):
                if ps.decidable[i]:
                    total += 1
                    if not cp.same_bits(cp.margin0(M, got[e]), cp.margin0(M, fresh[e])):
                        differs.append((cls, name, e))
    print(f"{shape}: {total} comparisons with the fresh context on pairs without margin, {len(differs)} differ")
    if not cp.on_mg_library(shape):
        assert not differs, (len(differs), differs[:10])


@pytest.mark.parametrize("shapes", [("CylinderB", "CubeS"), ("BottleS", "BowlS")], ids=lambda s: "-".join(s))
def test_envs_given_another_object_start_like_a_fresh_context_of_it(shapes):
    """A mixed-object context steps poses of its first object (every env's pair memory then names vertices of THAT object's hulls: 142 against 24
    for CylinderB / CubeS, up to 1546 against at most 533 for BottleS / BowlS); ks_reset_objects then gives every third env the second object.
    ks_reset_objects clears the pair memory of the envs whose object it changes, so they continue bit for bit like a new context of the second object alone -
    contact records of the first step, and contacts and state over three further steps - and meet the oracle; the other envs (stale memory of
    their own object) meet the oracle as well."""
    from kinovagrasping_amd.sim import KinovaSim
    first, second = shapes
    pa, pb = cp.poses(first, "gap_ladder"), cp.poses(second, "gap_ladder")
    Ma, Mb = cp._oracle(first).M, cp._oracle(second).M
    n = N_SHORT
    ia = tiled(pa, n)
    ids = np.arange(0, n, 3, dtype=np.int32)
    ib = tiled(pb, len(ids))
    zeros = lambda k: torch.zeros((15, k), dtype=torch.float64)
    act = torch.as_tensor(np.repeat(np.array(ACTION)[:, None], n, 1))
    mixed = KinovaSim(n, list(shapes), frame_skip=1, horizon=0, contact_tap=True)
    put(mixed, pa, (ia + len(pa.ref) // 2 + 1) % len(pa.ref))
    mixed.step(act)
    mixed.step(act)
    # the second object for every third env, then every env on its pose
    qb, hb = torch.as_tensor(pb.qpos[:, ib].copy()), torch.as_tensor(pb.hand_quat[:, ib].copy())
    q = pa.qpos[:, ia].copy()
    q[:, ids] = pb.qpos[:, ib]
    mixed.reset(torch.as_tensor(pa.qpos[:, ia].copy()), torch.as_tensor(pa.hand_quat[:, ia].copy()))
    mixed.reset(qb, hb, env_ids=torch.as_tensor(ids), object_id=np.ones(len(ids), dtype=np.int32))
    mixed.set_state(torch.as_tensor(q), zeros(n), zeros(n))
    alone = KinovaSim(len(ids), second, frame_skip=1, horizon=0, contact_tap=True)
    alone.reset(qb, hb)
    alone.set_state(qb, zeros(len(ids)), zeros(len(ids)))
    keep = np.setdiff1d(np.arange(n), ids)
    models = [Mb if e in set(ids.tolist()) else Ma for e in range(n)]
    for t in range(4):
        mixed.step(act)
        alone.step(act[:, :len(ids)])
        sm, sa = mixed.get_state(contacts=True), alone.get_state(contacts=True)
        torch.cuda.synchronize()
        dev_ids = torch.as_tensor(ids.astype(np.int64), device=sm["qpos"].device)
        for k in ("qpos", "qvel", "qacc_warmstart"):
            assert torch.equal(sm[k][:, dev_ids], sa[k]), (t, k)
        assert torch.equal(sm["ncon"][dev_ids], sa["ncon"]), t
        got_m, got_a = tap(mixed, models), tap(alone, Mb)
        for k, e in enumerate(ids):
            assert cp.same_bits(got_m[e], got_a[k]), (t, int(e))
        if t == 0:
            tb = compare(pb, ib, [got_m[e] for e in ids], 32, f"fp32 ks_step after ks_reset_objects ({first} -> {second})")
            ta = compare(pa, ia[keep], [got_m[e] for e in keep], 32, f"fp32 ks_step stale memory beside them ({first})")
            assert not tb.failures and not ta.failures, (tb.failures[:5], ta.failures[:5])
    mixed.close(); alone.close()
