"""Every GPU path that casts rangefinder rays, each against the fp64 oracle on poses that put the OBJECT onto the rays (tests/ray_poses.py;
tests/test_rays_cpu.py holds the same tolerances on the host lane of the kernel source, and the coverage floors on the oracle alone).

The rays are isolated from the physics by frame_skip = 1: the ray snapshot is what mj_forward saw at the START of the last substep
(ks_env.h, above lane_env_step), so after ONE ks_step / one env-step of ks_rollout from a fresh ks_reset the ray slots of the observation
(50-66, a miss stored as 6) belong to exactly the reset pose - whatever the action, however deeply an aimed object sits in a finger.

  path                                   reached by
  k_rays<double>                         precision-64 context: ks_reset, and ks_step (no in-step rays in fp64)
  k_rays<float>                          precision-32 context: ks_reset; ks_step with KS_RAYS_IN_STEP=0
  wg_rays<false>, own rays               ks_step with KS_RAY_POOL=0
  wg_rays<false> + wg_ray_pool           ks_step, default
  wg_rays<true> (free waves)             ks_rollout, one env-step, plan "waves" (275 and 4096 envs; Vase1S / CylinderB, 15 envs per workgroup:
                                         wg_rays<false> from the "workgroups" / "queue" forms of k_rollout)
  ray_lane_f64 in k_rollout_f64          ks_rollout on a precision-64 context
  the multi-geom build of all of these   BowlS, BottleS on libkinova_sim_mg.so (16 geom slots per ray; its ks_rollout is fp32 only)

Tolerances (tests/ray_poses.py): fp64 paths 1e-9 absolute, no hit / miss flip, no exception; fp32 paths 2e-4 * (1 + |oracle|), at most 0.05 % of
the rays of a (shape, class, path) beyond it (none in a set of fewer than 2 000 rays), every one of them printed.  Cross-path
(test_paths_that_cast_the_same_pose_return_the_same_bits): paths that cast the same fp32 snapshot with the same compiled arithmetic return
the same bits, k_rollout_f64 the bits of k_rays<double>; the poses of class exact_feature (rays through mesh vertices and edges) are compared
this way only.
Env counts 275 and 4099: partly filled ray groups, a partly filled stepping workgroup, and at 4099 more workgroups than compute units.
Run with -s for the table (recorded in profiles/ray_parity.txt)."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import ray_poses as rp

pytestmark = pytest.mark.gpu

N_LONG, N_SHORT, N_WAVES = 4099, 275, 4096
ACTION = (0.1, 0.3, -0.2, 0.4)           # any action: the ray snapshot of the first substep precedes its effect

# kind "lock": ks_reset then one ks_step; "rollout": ks_reset then one env-step of ks_rollout
Path = namedtuple("Path", "name kind precision n env")
STEP64 = Path("k_rays<double> ks_step", "lock", 64, N_LONG, ())
POOL = Path("wg_rays<false> + pool", "lock", 32, N_LONG, ())
POOL_SHORT = Path("wg_rays<false> + pool", "lock", 32, N_SHORT, ())
SEPARATE = Path("k_rays<float> ks_step", "lock", 32, N_LONG, (("KS_RAYS_IN_STEP", "0"),))
OWN = Path("wg_rays<false> own rays", "lock", 32, N_LONG, (("KS_RAY_POOL", "0"),))
OWN_SHORT = Path("wg_rays<false> own rays", "lock", 32, N_SHORT, (("KS_RAY_POOL", "0"),))
WAVES_SHORT = Path("wg_rays ks_rollout", "rollout", 32, N_SHORT, ())
WAVES = Path("wg_rays ks_rollout", "rollout", 32, N_WAVES, ())
ROLLOUT64 = Path("ray_lane_f64 ks_rollout", "rollout", 64, N_SHORT, ())
LOCK_PATHS = (STEP64, POOL, POOL_SHORT, SEPARATE, OWN, OWN_SHORT)
STANDARD_PATHS = LOCK_PATHS + (WAVES_SHORT, WAVES, ROLLOUT64)
MULTI_GEOM_PATHS = LOCK_PATHS + (WAVES_SHORT,)         # (libkinova_sim_mg.so refuses ks_rollout on precision-64 contexts)
CASES = [(s, p) for s in rp.STANDARD_SHAPES for p in STANDARD_PATHS] + [(s, p) for s in rp.MULTI_GEOM_SHAPES for p in MULTI_GEOM_PATHS]
case_id = lambda v: f"{v.name} fp{v.precision} n{v.n}".replace(" ", "_") if isinstance(v, Path) else str(v)

# fp32 ks_rollout: the free waves (wg_rays<true>) need one full 16-env group per workgroup and no more groups than compute units.  The hull
# tables of Vase1S and CylinderB leave LDS for 15 envs per workgroup: their contexts run the barrier-joined workgroups at 275 envs and the
# ready queue at 4096 (274 groups) - both cast with wg_rays<false>.  fp64 contexts (k_rollout_f64) have the workgroup form only.
ROLLOUT_PLAN = {"Vase1S": ("workgroups", "queue"), "CylinderB": ("workgroups", "queue")}
SWITCHES = ("KS_RAYS_IN_STEP", "KS_RAY_POOL", "KS_OBS_IN_STEP", "KS_ROLLOUT_WAVES", "KS_ROLLOUT_WGS", "KS_ROLLOUT_DEAL", "KS_ROLLOUT_PHASE_DEAL")
_poses, _results = {}, {}


def pose_set(shape, cls):
    """one draw of N_LONG envs per (shape, class); the smaller contexts take its first envs"""
    if (shape, cls) not in _poses:
        _poses[shape, cls] = rp.poses(shape, cls, N_LONG)
    return _poses[shape, cls]


def head(ps, n):
    cut = lambda a: None if a is None else a[:n]
    return rp.PoseSet(ps.shape, ps.cls, ps.qpos0[:, :n], ps.hand_quat[:, :n], cut(ps.rays), cut(ps.obj_hit))


def ray_slots(obs):
    return rp.from_obs(obs.double().cpu().numpy()[:, 50:67])


def no_pool_timeout(sim, what):
    status = sim.get_state()["status"].cpu().numpy()
    assert (status & 4 == 0).all(), (what, "ray-pool wait ran out in envs", np.flatnonzero(status & 4)[:10])


def run_path(shape, path):
    """{class: {"reset": rays [n, 17] of ks_reset (lock-step contexts), "step": rays after the one env-step}} - cached: the cross-path test
    compares what the per-path tests compared with the oracle"""
    if (shape, path) in _results:
        return _results[shape, path]
    from kinovagrasping_amd.sim import KinovaSim
    with pytest.MonkeyPatch.context() as mp:                 # the switches are read when the context is created
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in path.env:
            mp.setenv(k, v)
        rollout = path.kind == "rollout"
        sim = KinovaSim(path.n, shape, precision=path.precision, frame_skip=1, horizon=30 if rollout else 0, auto_reset=rollout)
        assert {k: os.environ[k] for k in SWITCHES if k in os.environ} == dict(path.env)          # which path this context runs
    assert sim.multi_geom == rp.is_multi_geom(shape) and sim.dtype == (torch.float64 if path.precision == 64 else torch.float32)
    tr = None
    out = {}
    for cls in rp.CLASSES:
        ps = head(pose_set(shape, cls), path.n)
        obs0 = sim.reset(torch.as_tensor(ps.qpos0.copy()), torch.as_tensor(ps.hand_quat.copy()))
        torch.cuda.synchronize()
        res = {"reset": ray_slots(obs0)}
        if not rollout:
            obs = sim.step(torch.as_tensor(np.repeat(np.array(ACTION)[:, None], path.n, 1)))[0]
            torch.cuda.synchronize()
            res["step"] = ray_slots(obs)
        else:
            if tr is None:
                tr, eng, replay = rollout_engine(sim, obs0)
                plan = sim.rollout_plan()
                want = "workgroups" if path.precision == 64 else ROLLOUT_PLAN.get(shape, ("waves", "waves"))[path.n == N_WAVES]
                assert plan[0] == want == tr.rollout_plan, (plan, want)
                print(f"{shape} {path.name} n={path.n}: rollout plan {plan}")
            eng.start(obs0)
            sim.rollout(1, tr.args)
            replay.commit_published()
            torch.cuda.synchronize()
            # an env that finished (an aimed object may start above the lift height) was restarted: its terminal observation is in final_obs
            done = sim.done.bool()
            res["step"] = ray_slots(torch.where(done[:, None], sim.final_obs, sim.obs))
        no_pool_timeout(sim, (shape, cls, path.name))
        out[cls] = res
    sim.close()
    _results[shape, path] = out
    return out


def rollout_engine(sim, obs0):
    """the free-running rollout's plumbing, as tests/test_gpu_async.py sets it up"""
    import warnings
    from kinovagrasping_amd.ddpgfd import DDPGfD
    from kinovagrasping_amd.pipeline import AsyncTrainer
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from kinovagrasping_amd.rollout import RolloutEngine
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=64, hidden=(256, 256), device=sim.device)
    replay = DeviceEpisodeReplay(sim.n_envs, capacity=8 * sim.n_envs, horizon=30, device=sim.device)
    eng = RolloutEngine(sim, policy, replay, expl_noise=0.1)
    eng.start(obs0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=16)
    return tr, eng, replay


@pytest.mark.parametrize("shape,path", CASES, ids=case_id)
def test_rays_of_every_gpu_path_match_the_oracle(shape, path):
    got = run_path(shape, path)
    failures = []
    for cls in rp.ASSERTED_CLASSES:
        ps = head(pose_set(shape, cls), path.n)
        rp.check_coverage(pose_set(shape, cls))
        stages = [("step", f"{path.name} n={path.n}")]
        if path.kind == "lock" and not path.env:            # ks_reset runs k_rays<T> in every context: compared once per precision and size
            stages.insert(0, ("reset", f"k_rays<{'double' if path.precision == 64 else 'float'}> ks_reset n={path.n}"))
        for stage, name in stages:
            beyond, n_rays, _ = rp.compare(ps, got[cls][stage], path.precision, name)
            if beyond > rp.allowed_beyond(path.precision, n_rays):
                failures.append((cls, name, beyond, rp.allowed_beyond(path.precision, n_rays)))
    assert not failures, failures


def ulps(a, b, precision):
    """largest difference in units of the last place between two arrays of non-negative distances (and -1 for a miss)"""
    if a.size == 0:
        return 0
    it, ft = (np.int64, np.float64) if precision == 64 else (np.int32, np.float32)
    return int(np.abs(a.astype(ft).view(it).astype(np.int64) - b.astype(ft).view(it).astype(np.int64)).max())


def difference(a, b, precision):
    """(rays that differ, hit / miss flips, largest difference in ulp and absolute among the others, rays beyond the fp32 tolerance - flips included)"""
    flip = (a < 0) != (b < 0)
    d = np.where(flip, 0.0, np.abs(a - b))
    beyond = flip | (d > rp.FP32_TOL * (1 + np.abs(b)))
    return int((a != b).sum()), int(flip.sum()), ulps(a[~flip], b[~flip], precision), float(d.max()), int(beyond.sum())


@pytest.mark.parametrize("shape", rp.SHAPES)
def test_paths_that_cast_the_same_pose_return_the_same_bits(shape):
    """All classes, exact_feature included; smaller contexts hold the first envs of the same draw.

    Bit for bit (the minimum over the same fp32 triangle hits does not depend on who visits them):
      * k_rays<T> of ks_reset in every context, whatever its size and switches;
      * the in-step rays of every stepping form - own rays, pooled, 275 or 4099 envs, ks_rollout's free waves / workgroups / queue;
      * fp64: ks_step's and k_rollout_f64's rays against ks_reset's (which also confirms that with frame_skip = 1 the step's ray
        snapshot IS the reset pose).
    Rounding pairs (fp32) - the same pose, but not the same bits going in or the same compiled arithmetic:
      * k_rays<float> after ks_step (KS_RAYS_IN_STEP=0) against the in-step rays: the same snapshot; ray_origin / ray_to_geom / ray_tri are
        compiled into two kernels that contract multiply-adds differently (tests/test_gpu_parity.py: test_in_step_rays_equal_the_separate_ray_kernel);
      * k_rays<float> after ks_step against k_rays<float> after ks_reset: the same kernel, but the snapshot comes from k_reset's one-lane
        kinematics in one case and from the stepping kernel's team kinematics in the other - body poses that differ in their last bits.
      A difference of the last bits of a pose or of a dot product is amplified without bound where a ray grazes a surface, so no ulp figure
      bounds these pairs (measured: profiles/ray_parity.txt).  They are held to what each of them is held to against the oracle: 2e-4 * (1 + |d|),
      at most 0.05 % of the rays beyond it, a hit / miss flip counting as beyond - on the asserted classes; on exact_feature (rays through
      vertices and edges, where the last bit of the pose decides which triangle is hit) the figures are printed only."""
    paths = MULTI_GEOM_PATHS if rp.is_multi_geom(shape) else STANDARD_PATHS
    got = {p: run_path(shape, p) for p in paths}
    bit_pairs = [(p, "reset", POOL if p.precision == 32 else STEP64, "reset") for p in paths]
    bit_pairs += [(p, "step", OWN, "step") for p in paths if p.precision == 32 and p not in (OWN, SEPARATE)]
    bit_pairs += [(p, "step", STEP64, "reset") for p in paths if p.precision == 64]
    rounding_pairs = [(SEPARATE, "step", OWN, "step"), (SEPARATE, "step", SEPARATE, "reset")]
    failures = []
    for cls in rp.CLASSES:
        for p, ps_, q, qs in bit_pairs:
            a, b = got[p][cls][ps_], got[q][cls][qs][:p.n]
            if not np.array_equal(a, b):
                failures.append((cls, p.name, p.n, ps_, "against", q.name, qs) + difference(a, b, p.precision))
        for p, ps_, q, qs in rounding_pairs:
            a, b = got[p][cls][ps_], got[q][cls][qs]
            n_diff, flips, ulp, dmax, beyond = difference(a, b, 32)
            print(f"{shape:10s} {cls:13s} {p.name} {ps_} vs {q.name} {qs}: {n_diff} of {a.size} rays differ, {flips} flips, largest {ulp} ulp / {dmax:.2e}, "
                  f"beyond tolerance {beyond}")
            if cls in rp.ASSERTED_CLASSES and beyond > rp.allowed_beyond(32, a.size):
                failures.append((cls, p.name, p.n, ps_, "against", q.name, qs, n_diff, flips, ulp, dmax, beyond))
    for f in failures:
        print("  DIFFERS", shape, f)
    print(f"{shape}: {len(bit_pairs)} bit-for-bit pairs and {len(rounding_pairs)} rounding pairs x {len(rp.CLASSES)} classes: {'ok' if not failures else 'FAILED'}")
    assert not failures, failures
