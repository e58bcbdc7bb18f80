"""An env's step does not depend on which envs share its wave.

The four envs of a wave of k_env_step_f32 run the constraint solver in lock step: a wave-uniform branch (a ballot, a loop that runs until the
slowest team is done) is taken for all of them or for none.  Whatever such a branch skips or repeats must leave an env's numbers alone - an env
with more than 16 contacts (its second contact slot per lane in use) beside envs without any is the case where the four teams want different
things.

One context per arrangement: CubeS, frame_skip 8, 16 envs (four waves), one reset, set_env_params, set_state, ONE ks_step, get_state.

  the overflow state   tests/plane_poses.poses("CubeS", "overflow"): the hand pressed into the floor, the pose with the longest contact list (30
                       against a capacity of 24); zero velocity, zero action.  The oracle keeps 18 contacts at the end of the 8 substeps
                       (test_the_oracle_counts_of_the_two_states, no GPU).
  the free state       tests/dynamics_states.states("free_flight", "CubeS")[0]: hand parked in the air, the object flying; no contact

  arrangements         the overflow state at envs i % 4 == 0 | at i % 4 == 3 (every wave mixed) | in waves 0 and 2 (every wave of one kind)
  references           all 16 envs hold the overflow state | all 16 hold the free state

Every env's qpos / qvel / qacc_warmstart / ncon / status is bit-equal to the SAME env of the reference that holds its state.  Asserted from the
runs themselves: in the two mixed arrangements every wave holds an env that reports ncon > 16 and one that reports ncon <= 16; no status bit but
the contact-overflow bit (1) is set anywhere."""
from functools import lru_cache

import numpy as np
import pytest

N, FRAME_SKIP, WAVE = 16, 8, 4
OUTPUTS = (("qpos", "qpos"), ("qvel", "qvel"), ("warm", "qacc_warmstart"))
ARRANGEMENTS = {"first_team": np.arange(N) % WAVE == 0, "last_team": np.arange(N) % WAVE == 3, "whole_waves": (np.arange(N) // WAVE) % 2 == 0}


@lru_cache(maxsize=None)
def two_states():
    """[overflow, free]: dict(qpos [16], qvel [15], warm [15], action [4], hq [4], mass), every input rounded to fp32"""
    from tests import dynamics_states as ds, plane_poses as pp
    ps = pp.poses("CubeS", "overflow")
    i = int(np.argmax(ps.total))
    assert ps.total[i] >= 21
    over = dict(qpos=ds.f32(ps.qpos[:, i]), qvel=np.zeros(15), warm=np.zeros(15), action=np.zeros(4), hq=ds.f32(ps.hand_quat[:, i]),
                mass=float(ds.f32(ds.model("CubeS")["body_mass"][9])))
    s = ds.states("free_flight", "CubeS")
    free = dict(qpos=s.qpos[:, 0], qvel=s.qvel[:, 0], warm=s.warm[:, 0], action=s.action[:, 0], hq=s.hq[:, 0], mass=float(s.mass[0]))
    return over, free


def test_the_oracle_counts_of_the_two_states():
    """(no GPU) what the arrangement relies on, from the oracle alone: the overflow state keeps more than 16 contacts to the end of the env-step,
    the free state has none"""
    from kinovagrasping_amd.sim import SOLVER_ITERATIONS
    from oracle import ko_py as ko
    from tests import contact_poses as cp
    counts = []
    for st in two_states():
        o = ko.OracleSim(cp._oracle("CubeS").model, st["hq"], solver_iterations=SOLVER_ITERATIONS, ncon_max=24)
        o.s.rays_enabled = 0
        o.env_reset(st["qpos"])
        o.set_state(st["qpos"], st["qvel"], st["warm"])
        o.env_step(st["action"], frame_skip=FRAME_SKIP)
        assert np.isfinite(o.view("qpos")).all()
        counts.append(int(o.s.ncon))
    print("oracle ncon after the env-step: overflow state", counts[0], "free state", counts[1])
    assert counts[0] > 16 and counts[1] == 0


def run_context(is_over):
    """env e holds the overflow state where is_over[e], the free state elsewhere: {output: [k, 16] float32}, ncon, status"""
    import torch
    from kinovagrasping_amd.sim import KinovaSim
    over, free = two_states()
    col = lambda k: np.stack([np.asarray((over if o else free)[k], dtype=np.float64) for o in is_over], 1)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a))
    sim = KinovaSim(N, "CubeS", precision=32, frame_skip=FRAME_SKIP, horizon=0)
    assert not sim.multi_geom
    sim.reset(t(col("qpos")), t(col("hq")))
    sim.set_env_params(obj_mass=torch.as_tensor(np.array([(over if o else free)["mass"] for o in is_over])))
    sim.set_state(t(col("qpos")), t(col("qvel")), t(col("warm")))
    sim.step(t(col("action")))
    st = sim.get_state()
    torch.cuda.synchronize()
    out = {k: st[name].cpu().numpy().astype(np.float32) for k, name in OUTPUTS}
    ncon, status = st["ncon"].cpu().numpy().astype(np.int64), st["status"].cpu().numpy().astype(np.int64)
    sim.close()
    return out, ncon, status


@lru_cache(maxsize=None)
def references():
    return run_context(np.ones(N, dtype=bool)), run_context(np.zeros(N, dtype=bool))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ARRANGEMENTS))
def test_an_env_steps_the_same_whoever_shares_its_wave(name):
    is_over = ARRANGEMENTS[name]
    ref_over, ref_free = references()
    out, ncon, status = run_context(is_over)
    print(name, "ncon", ncon.tolist(), "status", status.tolist(), "| all overflow: ncon", ref_over[1].tolist(), "status", ref_over[2].tolist())
    for o, n, s in (ref_over, ref_free, (out, ncon, status)):
        assert all(np.isfinite(v).all() for v in o.values())
        assert ((s & ~1) == 0).all(), ("a status bit other than contact overflow", s.tolist())
    assert (ref_free[1] == 0).all() and (ref_over[1] > 16).all(), (ref_free[1].tolist(), ref_over[1].tolist())
    waves = [(ncon[w:w + WAVE] > 16).any() and (ncon[w:w + WAVE] <= 16).any() for w in range(0, N, WAVE)]
    if name == "whole_waves":
        assert not any(waves) and (ncon > 16).any() and (ncon <= 16).any(), ncon.tolist()
    else:
        assert all(waves), ("every wave holds an env beyond 16 contacts and one within", ncon.tolist())
    for e in range(N):
        ro, rn, rs = ref_over if is_over[e] else ref_free
        for k in out:
            assert np.array_equal(out[k][:, e].view(np.uint32), ro[k][:, e].view(np.uint32)), (name, "env", e, k, "differs from the env among its own kind")
        assert ncon[e] == rn[e] and status[e] == rs[e], (name, "env", e, "ncon / status", int(ncon[e]), int(rn[e]), int(status[e]), int(rs[e]))
