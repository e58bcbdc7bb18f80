"""The in-step rays with batched leaf loads (ks_api.hip: wg_rays, RayWalk<..., WG_LEAF_BATCH>) at the smallest size that has both of
its forms: ONE context of 20 CubeS envs - a full 16-env workgroup and a quarter-filled one; in ks_rollout's free-running form five waves
of four envs (wg_rays<true>, 64 lanes share a wave's walks), in ks_step the two workgroups and the ray pool (wg_rays<false>).

frame_skip = 1 isolates the rays from the physics (tests/test_gpu_rays.py): after one env-step from a fresh ks_reset the ray slots of the
observation belong to the reset pose.  The poses are the first 20 of the `aimed` class, seed 0 (tests/ray_poses.py).

  * ks_rollout's ray slots equal ks_step's bit for bit: the minimum over the same fp32 triangle hits, whoever loads them in whatever order;
  * both are within 2e-4 * (1 + |oracle|) of the fp64 oracle in EVERY ray.  The 0.05 % allowance of the large sets does not apply to 340 rays;
    on this draw the reference path (the host lane of the kernel source, a triangle at a time) has no ray beyond the tolerance and its worst
    error is 3.4e-7 - 600 times inside it (checked without a GPU when the draw was chosen), so nothing here grazes an edge."""
import numpy as np
import pytest
import torch

from tests import ray_poses as rp
from tests.test_gpu_rays import ACTION, no_pool_timeout, ray_slots, rollout_engine

pytestmark = pytest.mark.gpu

N = 20


def test_wave_form_rays_equal_ks_step_bit_for_bit_and_both_match_the_oracle(monkeypatch):
    from kinovagrasping_amd.sim import KinovaSim
    for k in ("KS_RAYS_IN_STEP", "KS_RAY_POOL", "KS_OBS_IN_STEP", "KS_ROLLOUT_WAVES", "KS_ROLLOUT_WGS", "KS_ROLLOUT_DEAL", "KS_ROLLOUT_PHASE_DEAL"):
        monkeypatch.delenv(k, raising=False)
    ps = rp.poses("CubeS", "aimed", N)
    assert (ps.rays >= 0).mean() > 0.5 and ps.obj_hit.mean() > 0.2, ((ps.rays >= 0).mean(), ps.obj_hit.mean())        # the oracle's own: most rays hit, a third the cube
    sim = KinovaSim(N, "CubeS", precision=32, frame_skip=1, horizon=30, auto_reset=True)

    def terminal_or_current():
        # an env that finished (an aimed object may start above the lift height) was restarted: its terminal observation is in final_obs
        return ray_slots(torch.where(sim.done.bool()[:, None], sim.final_obs, sim.obs))

    q0, hq = torch.as_tensor(ps.qpos0.copy()), torch.as_tensor(ps.hand_quat.copy())
    sim.reset(q0, hq)
    sim.step(torch.as_tensor(np.repeat(np.array(ACTION)[:, None], N, 1)))
    torch.cuda.synchronize()
    lock = terminal_or_current()
    no_pool_timeout(sim, "ks_step")

    obs0 = sim.reset(q0, hq)
    torch.cuda.synchronize()
    tr, eng, replay = rollout_engine(sim, obs0)
    assert sim.rollout_plan()[0] == "waves" == tr.rollout_plan, sim.rollout_plan()
    eng.start(obs0)
    sim.rollout(1, tr.args)
    replay.commit_published()
    torch.cuda.synchronize()
    waves = terminal_or_current()
    no_pool_timeout(sim, "ks_rollout")
    sim.close()

    for name, got in (("ks_step n=20", lock), ("wg_rays<true> ks_rollout n=20", waves)):
        beyond, n_rays, worst = rp.compare(ps, got, 32, name)
        assert n_rays == N * rp.NRAY and beyond == 0, (name, beyond, worst)
    differ = np.argwhere(waves != lock)
    assert np.array_equal(waves, lock), ("ks_rollout against ks_step: (env, ray)", differ[:10].tolist(), waves[waves != lock][:10], lock[waves != lock][:10])
