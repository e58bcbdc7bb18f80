"""The scripted demonstrators inside the kernels (csrc/ks_controller.h): kr_controller_select against the torch expressions of
demonstrators.py on the same device, the lock-step RolloutEngine(controller=...) against the Python loop run_controller_episodes, the
free-running ks_rollout with a controller set (ks_set_rollout_controller) against the lock-step calls - bit for bit, in the scheduling
forms a small context can be put in, both precisions, both libraries, with a start pool and an episode log -, switching between
controller and actor on one context, the error paths, and demonstrators.run_controller_free_running against a lock-step run.
Starts: scenarios.draw_start_pool(["CubeS"] * n, "normal", k, RandomState(13)), as tests/test_gpu_episode_log.py's _eval_setup draws them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from kinovagrasping_amd import scenarios
from tests.test_controller_cpu import GOLDEN_TOL, golden_cases
from tests.test_gpu_start_pool import _ring_episodes, _sim

pytestmark = pytest.mark.gpu

K = 6
POOL_SEED = 21
KS_ERR_INVALID, KS_ERR_STATE = -1, -5


@functools.lru_cache(maxsize=None)
def _starts(kind, n):
    if kind == "multi-geom":            # the bottle above the closing hand, at K jittered places (tests/test_gpu_start_pool.py: _rollout_setup)
        from tests.test_gpu_multi_geom import in_hand_start
        rng = np.random.RandomState(13)
        q = np.repeat(np.repeat(in_hand_start("BottleS")[None, :, None], K, 0), n, 2)
        q[:, 9] += rng.uniform(-0.02, 0.02, (K, n))
        q[:, 10] += rng.uniform(-0.01, 0.01, (K, n))
        hq = np.repeat(np.repeat(scenarios.hand_quat_for("normal")[None, :, None], K, 0), n, 2)
        return q, hq, None
    return scenarios.draw_start_pool(["CubeS"] * n, "normal", K, np.random.RandomState(13))


def _setup(kind, n, horizon, mode, rule, pool=False, log=False, auto_reset=True, with_replay=True, policy=None):
    """a context at the start of an episode (entry 0 of the drawn starts, or the whole pool), a replay and a controller engine on it"""
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from kinovagrasping_amd.rollout import RolloutEngine
    q, hq, classes = _starts(kind, n)
    sim = _sim(n, "BottleS" if kind == "multi-geom" else "CubeS", horizon=horizon, auto_reset=auto_reset, precision=64 if kind == "fp64" else 32)
    assert sim.multi_geom == (kind == "multi-geom")
    if pool:
        obs0 = sim.set_start_pool(torch.as_tensor(q), torch.as_tensor(hq), POOL_SEED).clone()
    else:
        obs0 = sim.reset(torch.as_tensor(q[0]), torch.as_tensor(hq[0])).clone()
    if log:
        sim.set_episode_log(8 * n)
    replay = DeviceEpisodeReplay(n, capacity=8 * n, horizon=horizon, device=sim.device) if with_replay else None
    eng = RolloutEngine(sim, policy, replay, controller=mode, lift_rule=rule)
    eng.start(obs0)
    return sim, replay, eng, obs0


def _words(rec):
    xy = rec["start_xy"].contiguous().view(torch.int32)
    w = torch.stack([rec["env"], rec["object"], rec["start_index"], rec["steps"], rec["done"], xy[:, 0], xy[:, 1], rec["episode"]], 1).cpu().numpy()
    return w[np.lexsort((w[:, 7], w[:, 0]))]


@functools.lru_cache(maxsize=None)
def _lock_step(kind, n, horizon, mode, rule, steps, pool=False, log=False):
    """the reference: `steps` env-steps of kr_controller_select -> ks_step -> kr_store_transition"""
    sim, replay, eng, obs0 = _setup(kind, n, horizon, mode, rule, pool, log)
    lifted = torch.zeros((), dtype=torch.long, device=sim.device)
    timed = torch.zeros_like(lifted)
    lift_steps = torch.zeros_like(lifted)
    for _ in range(steps):
        eng.step()
        lift_steps += eng.lifting.sum()
        lifted += ((sim.done & 1) != 0).sum()
        timed += (((sim.done & 2) != 0) & ((sim.done & 1) == 0)).sum()
    torch.cuda.synchronize()
    st = sim.get_state()
    out = dict(obs0=obs0.float().cpu(), obs=eng.obs.clone(), prev=eng.prev_obs.clone(), t=eng.t.clone(), ready=eng.ready.clone(), init=eng.init.clone(),
               action=eng.action.clone(), qpos=st["qpos"].clone(), status=st["status"].clone(), eps=_ring_episodes(replay), count=replay.count,
               lifted=int(lifted), timed=int(timed), lift_steps=int(lift_steps), words=_words(sim.episode_log()) if log else None)
    sim.close()
    return out


def _free_args(sim, eng, replay, policy=None, pub=None, pub_ver=None):
    from kinovagrasping_amd.pipeline import rollout_args
    if replay is not None:
        replay.enable_async()
    steps_total = torch.zeros(sim.n_envs, dtype=torch.long, device=sim.device)
    counters = torch.zeros(8 + 4 * 512 + 8, dtype=torch.long, device=sim.device)
    return rollout_args(sim, policy, eng, pub, pub_ver, steps_total, counters, replay=replay), steps_total, counters


def _free_running_equals_lock_step(kind, n, horizon, mode, rule, per, chunks, plan, pool=False, log=False):
    ref = _lock_step(kind, n, horizon, mode, rule, per * chunks, pool, log)
    x0 = ref["obs0"][:, 21]
    print(f"lock step {kind} n={n} {mode}/{rule} horizon {horizon}, {per * chunks} env-steps: {ref['lifted']} episodes lifted, {ref['timed']} ran into the time "
          f"limit, {ref['lift_steps']} lift steps, ring {ref['count']}; starts: {(x0.abs() <= 0.03).sum()} centre, {(x0 > 0.03).sum()} right, {(x0 < -0.03).sum()} left")
    if kind != "multi-geom" and not pool:
        # the reference run's starts reach all three PD branches
        assert (x0.abs() <= 0.03).any() and (x0 > 0.03).any() and (x0 < -0.03).any()
    if horizon == 30 and per * chunks >= 2 * horizon:
        assert ref["lifted"] >= 1 and ref["timed"] >= 1
    sim, replay, eng, _ = _setup(kind, n, horizon, mode, rule, pool, log)
    sim.set_rollout_controller(mode, rule)
    if plan is not None:
        assert sim.rollout_plan()[0] == plan, sim.rollout_plan()
    args, steps_total, counters = _free_args(sim, eng, replay)
    assert not args.actor_pub and not args.actor_ver and args.h1 == 0
    for _ in range(chunks):
        sim.rollout(per, args)
        replay.commit_published()
    torch.cuda.synchronize()
    st = sim.get_state()
    c = counters[:4].tolist()
    print(f"free-running: plan {sim.rollout_plan()}, counters {c}, ring {replay.count}")
    assert c[3] == 0                                                         # no episode is dropped
    assert c[0] == ref["lifted"] + ref["timed"] and c[1] == ref["lifted"]
    assert torch.equal(st["qpos"], ref["qpos"]) and torch.equal(st["status"], ref["status"])
    assert torch.equal(eng.obs, ref["obs"]) and torch.equal(eng.prev_obs, ref["prev"]) and torch.equal(eng.t, ref["t"]) and torch.equal(eng.ready, ref["ready"])
    assert torch.equal(eng.action, ref["action"])
    assert torch.equal(sim.rollout_controller_init(), ref["init"])
    assert torch.equal(steps_total, torch.full_like(steps_total, per * chunks))
    assert replay.count == ref["count"] == min(c[2], replay.capacity) and _ring_episodes(replay) == ref["eps"]
    if log:
        assert np.array_equal(_words(sim.episode_log()), ref["words"]) and len(ref["words"]) == c[0]
    sim.close()


@pytest.mark.parametrize("mode,rule,horizon,per,chunks", [("naive", "expert", 30, 13, 5), ("combined", "expert", 30, 13, 5), ("combined", "train", 12, 5, 8)])
def test_free_running_controller_equals_the_lock_step_calls(mode, rule, horizon, per, chunks):
    """n = 272 (17 workgroups, the wave form).  horizon 30, 5 launches of 13 env-steps: long enough for the expert rule's t > 10 lifts and a second
    episode; lift rule train at horizon 12 in launches of 5 (an episode of that rule has at least 6 steps: no env can finish two in one launch)"""
    _free_running_equals_lock_step("fp32", 272, horizon, mode, rule, per, chunks, "waves")


def test_free_running_controller_with_a_start_pool_and_an_episode_log():
    """the pool's draws and the log's records per (env, episode) are the lock-step ones"""
    _free_running_equals_lock_step("fp32", 272, 30, "combined", "expert", 13, 5, "waves", pool=True, log=True)


def test_free_running_controller_in_the_barrier_joined_workgroup_form(monkeypatch):
    monkeypatch.setenv("KS_ROLLOUT_WAVES", "0")
    _free_running_equals_lock_step("fp32", 272, 30, "position-dependent", "expert", 13, 3, "workgroups")


def test_free_running_controller_in_the_exact_mode():
    """precision 64: the controller reads the fp32 rounding of the fp64 observation; 2 launches of 8 env-steps (fewer than the fp32 cases: no
    grasp has latched by then - the lifts of this path's shared code are the fp32 cases')"""
    _free_running_equals_lock_step("fp64", 272, 30, "combined", "expert", 8, 2, "workgroups")


def test_free_running_controller_on_the_multi_geom_library():
    _free_running_equals_lock_step("multi-geom", 64, 12, "combined", "train", 5, 3, None, pool=True)


def _torch_engine_like(eng, mode, rule, force_ready=None):
    """a second engine on the same context whose pre() runs the torch expressions (the checker path of RolloutEngine), in `eng`'s state;
    force_ready: envs whose grasp counts as latched already, whatever the run has seen"""
    from kinovagrasping_amd.rollout import RolloutEngine
    ref = RolloutEngine(eng.sim, None, None, controller=mode, lift_rule=rule)
    ref.native = False
    for k in ("obs", "prev_obs", "has_prev", "t", "ready", "init"):
        getattr(ref, k).copy_(getattr(eng, k))
    if force_ready is not None:
        ref.ready |= force_ready
    return ref


def test_kr_controller_select_equals_the_torch_expressions_on_the_device(golden_dir):
    """272 envs, the observations of real env-steps 0, 1, 2, 6, 10, 11, 12, 16, 20, 24 and 28 of a combined-controller episode, as the run left
    them and once more with every other env's grasp latched (so that lifting rows, and rows that are latched while the expert rule still waits
    for t > 10, occur whenever the run itself latches): actions, ready, lifting and init of the three modes and both lift rules are the bits
    of the torch expressions (demonstrators.controller_action, the rules as RolloutEngine's torch path states them) on the same device; then
    the 600 golden cases: the bits of torch, and the reference's fp64 answers within the CPU test's bound"""
    n = 272
    sim, _, eng, _ = _setup("fp32", n, 30, "combined", "expert", with_replay=False)
    every_other = (torch.arange(n, device=sim.device) % 2) == 0
    seen_lift = seen_hold = own_lift = 0
    for step in range(29):
        if step in (0, 1, 2, 6, 10, 11, 12, 16, 20, 24, 28):
            for mode in ("naive", "position-dependent", "combined"):
                for rule in ("expert", "train"):
                    for forced in (None, every_other):
                        a, b = _torch_engine_like(eng, mode, rule, forced), _torch_engine_like(eng, mode, rule, forced)
                        b.native = True
                        a.pre()
                        b.pre()
                        for k in ("action", "action_t", "ready", "lifting", "init"):
                            assert torch.equal(getattr(a, k), getattr(b, k)), (step, mode, rule, forced is not None, k)
                        seen_lift += int(b.lifting.sum())
                        seen_hold += int((b.ready & ~b.lifting).sum())
                        own_lift += int(b.lifting.sum()) if forced is None else 0
        eng.step()
    print(f"kr_controller_select on real observations: {seen_lift} lifting rows ({own_lift} without the forced latch), {seen_hold} rows latched but not yet "
          f"lifting (expert rule, t <= 10)")
    assert seen_lift > 0 and seen_hold > 0
    # the golden cases: t = 1 (the start values are read, not written), lift rule train with ready = the case's lift flag and no previous observation
    g, obs, ix, idot, lift = golden_cases()
    dev, m = sim.device, len(obs)
    lib, P = sim.lib, lambda t: C.c_void_p(t.data_ptr())
    from kinovagrasping_amd.demonstrators import controller_action
    d = lambda a: torch.as_tensor(a).to(dev)
    obs_d, init_d, lift_d = d(obs), torch.stack([d(ix), d(idot)]).contiguous(), d(lift)
    for code, (mode, key) in enumerate((("naive", "action_naive"), ("position-dependent", "action_position_dependent"), ("combined", "action_combined")), 1):
        ready, lifting = lift_d.clone(), torch.zeros(m, dtype=torch.bool, device=dev)
        has_prev, t = torch.zeros(m, dtype=torch.bool, device=dev), torch.ones(m, dtype=torch.long, device=dev)
        action, action_t, init = torch.zeros(m, 4, device=dev), torch.zeros(4, m, device=dev), init_d.clone()
        rc = lib.kr_controller_select(m, code, 0, P(obs_d), P(obs_d), P(has_prev), P(t), P(ready), P(init), 6, P(action), P(action_t), P(lifting), None)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(lifting, lift_d) and torch.equal(init, init_d) and torch.equal(action_t, action.t())
        assert torch.equal(action, controller_action(mode, obs_d, init_d[0], init_d[1], lift_d))
        err = np.abs(action.double().cpu().numpy() - g[key]).max(1)
        print(f"{mode}: max |kr_controller_select - fp64 golden| over {m} cases {err.max():.3e}")
        assert (err < GOLDEN_TOL).all(), (mode, float(err.max()))
    sim.close()


def test_lock_step_engine_equals_the_python_loop():
    """RolloutEngine(controller="combined", lift_rule="expert") on a context without auto-reset against run_controller_episodes over one 30-step
    episode of 64 envs: the same action in every step of every env whose episode is running, the same success and steps"""
    from kinovagrasping_amd.demonstrators import run_controller_episodes
    n, horizon = 64, 30
    sim, _, eng, obs0 = _setup("fp32", n, horizon, "combined", "expert", auto_reset=False, with_replay=False)
    acts, step = [], sim.step
    sim.step = lambda a: (acts.append(a.clone()), step(a))[1]
    out = run_controller_episodes(sim, obs0.clone(), None, horizon, "combined", "expert")
    sim.step = step
    q, hq, _ = _starts("fp32", n)
    eng.start(sim.reset(torch.as_tensor(q[0]), torch.as_tensor(hq[0])))
    alive = torch.ones(n, dtype=torch.bool, device=sim.device)
    success, steps = torch.zeros_like(alive), torch.zeros(n, dtype=torch.long, device=sim.device)
    for t in range(horizon):
        eng.pre()
        assert torch.equal(eng.action_t[:, alive], acts[t][:, alive]), t
        sim.step(eng.action_t)
        eng.post()
        done = (sim.done != 0) & alive
        steps += alive.long()
        success |= done & ((sim.done & 1) != 0)
        alive &= ~done
    print(f"python loop / engine: {int(out['success'].sum())} of {n} lifted, steps {out['steps'].min().item()} .. {out['steps'].max().item()}")
    assert torch.equal(success, out["success"]) and torch.equal(steps, out["steps"])
    sim.close()


def _actor_setup(n, horizon):
    from kinovagrasping_amd.ddpgfd import DDPGfD
    from kinovagrasping_amd.rollout import RolloutEngine
    q, hq, _ = _starts("fp32", n)
    sim = _sim(n, "CubeS", horizon=horizon, auto_reset=True)
    obs0 = sim.reset(torch.as_tensor(q[0]), torch.as_tensor(hq[0])).clone()
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=64, hidden=(256, 256), device=sim.device)
    eng = RolloutEngine(sim, policy, None, expl_noise=0.1)
    eng.start(obs0)
    flat = policy._flat_params["actor"]
    pub = torch.zeros(3, (flat.numel() + 3) // 4 * 4, device=sim.device)
    pub[0, :flat.numel()].copy_(flat)
    pub_ver = torch.zeros(1, dtype=torch.long, device=sim.device)
    args, steps_total, counters = _free_args(sim, eng, None, policy, pub, pub_ver)
    return sim, eng, args, (policy, pub, pub_ver, steps_total, counters)


def test_switching_between_controller_and_actor_on_one_context():
    """(a) controller set and cleared again: the actor-path run behind it is a fresh context's; (b) a ks_rollout captured in a graph BEFORE
    ks_set_rollout_controller acts by the controller when it is replayed after the call - the record is read when the kernel runs"""
    n, horizon, per = 64, 30, 5
    sim, eng, args, keep = _actor_setup(n, horizon)
    sim.rollout(2 * per, args)
    torch.cuda.synchronize()
    fresh = dict(obs=eng.obs.clone(), action=eng.action.clone(), qpos=sim.get_state()["qpos"].clone(), t=eng.t.clone())
    sim.close()
    sim, eng, args, keep = _actor_setup(n, horizon)
    sim.set_rollout_controller("combined", "expert")
    sim.set_rollout_controller(None)
    sim.rollout(2 * per, args)
    torch.cuda.synchronize()
    assert torch.equal(eng.obs, fresh["obs"]) and torch.equal(eng.action, fresh["action"]) and torch.equal(sim.get_state()["qpos"], fresh["qpos"])
    sim.close()
    # (b)
    ref = _lock_step("fp32", n, horizon, "naive", "expert", per)
    sim, eng, args, keep = _actor_setup(n, horizon)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):     # (k_rollout has run in this process: part (a))
        sim.rollout(per, args)
    sim.set_rollout_controller("naive", "expert")
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eng.action, ref["action"]) and torch.equal(eng.obs, ref["obs"]) and torch.equal(sim.get_state()["qpos"], ref["qpos"])
    assert not torch.equal(eng.action, fresh["action"])
    sim.close()


def test_error_paths():
    from kinovagrasping_amd.sim import KsConfig, load_library
    sim, _, eng, _ = _setup("fp32", 64, 30, "combined", "expert", with_replay=False)
    lib = sim.lib
    for mode, rule in ((4, 0), (-1, 1), (1, 2), (3, -1)):
        assert lib.ks_set_rollout_controller(sim.ctx, mode, rule, None) == KS_ERR_INVALID
    with pytest.raises(ValueError):
        sim.set_rollout_controller("pid")
    with pytest.raises(ValueError):
        sim.set_rollout_controller("naive", "eval")
    P = lambda t: C.c_void_p(t.data_ptr())
    for mode, rule in ((0, 0), (4, 1), (1, 2)):
        assert lib.kr_controller_select(64, mode, rule, P(eng.obs), P(eng.prev_obs), P(eng.has_prev), P(eng.t), P(eng.ready), P(eng.init), 6, P(eng.action),
                                        P(eng.action_t), P(eng.lifting), None) == KS_ERR_INVALID
    # null actor pointers are accepted only while a controller is set
    args, _, _ = _free_args(sim, eng, None)
    assert lib.ks_rollout(sim.ctx, 1, C.byref(args), None) == KS_ERR_INVALID
    sim.set_rollout_controller("naive")
    assert lib.ks_rollout(sim.ctx, 1, C.byref(args), sim._stream()) == 0
    sim.set_rollout_controller(None)
    torch.cuda.synchronize()
    assert lib.ks_rollout(sim.ctx, 1, C.byref(args), None) == KS_ERR_INVALID
    sim.close()
    # before a model is loaded
    L = load_library()
    cfg = KsConfig()
    L.ks_default_config(C.byref(cfg))
    cfg.n_envs = 64
    ctx = C.c_void_p()
    assert L.ks_create(C.byref(cfg), 0, C.byref(ctx)) == 0
    assert L.ks_set_rollout_controller(ctx, 1, 1, None) == KS_ERR_STATE
    assert b"ks_load_model" in L.ks_last_error(ctx)
    L.ks_destroy(ctx)


def test_run_controller_free_running_equals_a_lock_step_run():
    """n = 272, a pool of 6 starts, 2 episodes per env: every env has exactly two counted episodes whose success and steps are the lock-step
    engine's for the same (env, episode), and the expert ring filled beside it holds the lock-step run's episodes"""
    from kinovagrasping_amd.demonstrators import run_controller_free_running
    n, horizon, E = 272, 30, 2
    sim, replay, _, _ = _setup("fp32", n, horizon, "combined", "expert", pool=True)
    _, _, classes = _starts("fp32", n)
    out = run_controller_free_running(sim, replay, episodes_per_env=E, mode="combined", lift_rule="expert", classes=classes, object_names=["CubeS"])
    torch.cuda.synchronize()
    assert out["env_steps"] % n == 0 and out["episodes_dropped"] == 0
    steps_run = out["env_steps"] // n
    assert tuple(out["success"].shape) == tuple(out["steps"].shape) == (n, E) and (out["steps"] > 0).all() and (out["start_index"] >= 0).all()
    assert len(out["success_coords"]["x"]) + len(out["fail_coords"]["x"]) == n * E and out["num_success"] == int(out["success"].sum())
    ref = _lock_step("fp32", n, horizon, "combined", "expert", steps_run, True, True)
    w = ref["words"]
    w = w[w[:, 7] < E]
    assert len(w) == n * E
    e, j = w[:, 0], w[:, 7]
    assert np.array_equal(out["success"].cpu().numpy()[e, j], (w[:, 4] & 1) != 0) and np.array_equal(out["steps"].cpu().numpy()[e, j], w[:, 3])
    assert np.array_equal(out["start_index"].cpu().numpy()[e, j], w[:, 2])
    print(f"run_controller_free_running: {steps_run} env-steps per env, {out['num_success']} of {n * E} counted episodes lifted, ring {replay.count} (lock step {ref['count']})")
    assert replay.count == ref["count"] and _ring_episodes(replay) == ref["eps"]
    # the controller and the log are cleared behind the run
    with pytest.raises(RuntimeError):
        sim.episode_log_raw()
    args, _, _ = _free_args(sim, _setup_engine_only(sim), None)
    assert sim.lib.ks_rollout(sim.ctx, 1, C.byref(args), None) == KS_ERR_INVALID
    sim.close()


def _setup_engine_only(sim):
    from kinovagrasping_amd.rollout import RolloutEngine
    return RolloutEngine(sim, None, None, controller="naive")
