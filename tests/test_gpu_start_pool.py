"""The start pool (ks_set_start_pool, include/kinova_sim.h): every env holds K prepared starts and each AUTO-RESET inside the stepping
kernels (ks_step: k_obs / wg_obs; ks_rollout: k_rollout, k_rollout_f64) draws one of them with a counter-based generator instead of
replaying the one stored initial state.  Pinned here: the draw against the host Philox reference, the restarted episodes against a
second context that is host-reset to the drawn entry (bit for bit), no pool / K = 1 against today's behaviour, the free-running
kernels against the lock-step calls with a pool on both sides, and curriculum.run_stage without host resets between rounds."""
import functools

import numpy as np
import pytest
import torch

from kinovagrasping_amd import scenarios
from tests.test_start_pool_cpu import start_index_reference

pytestmark = pytest.mark.gpu

N, K, HORIZON, STEPS = 64, 8, 5, 40
ACTION = (0.0, 0.3, 0.25, 0.35)                     # the fingers close, the wrist stays: no lift, every episode runs into the time limit


def _sim(*a, **k):
    from kinovagrasping_amd.sim import KinovaSim
    return KinovaSim(*a, **k)


def _entries(pool, idx, envs):
    """pool [K, F, N] -> [F, len(envs)]: entry idx[i] of env envs[i]"""
    return pool[torch.as_tensor(np.asarray(idx), dtype=torch.long), :, torch.as_tensor(np.asarray(envs), dtype=torch.long)].t().contiguous()


def _pick_seed(n=N, k=K, episodes=STEPS // HORIZON, distinct=3):
    """the first seed for which - by the host reference alone - every env uses at least `distinct` different entries in its first
    `episodes` episodes (40 steps at horizon 5: episodes 0..7 are run, the draw of episode 8 is made by the last step)"""
    for seed in range(1, 1000):
        idx = start_index_reference(seed, np.arange(n)[:, None], np.arange(episodes)[None], k)
        if min(len(set(row.tolist())) for row in idx) >= distinct:
            return seed, idx
    raise AssertionError("no seed found")


@functools.lru_cache(maxsize=None)
def _pool_run(precision, orientation):
    """64 CubeS envs with a pool of 8 starts, 40 lock-step ks_steps with a fixed action at horizon 5 - beside a second context WITHOUT a pool
    that is host-reset (ks_reset of the envs concerned) to the entry the first one drew whenever an episode of the first restarts, and
    stepped with the same actions.  Returns everything both produced."""
    seed, host_idx = _pick_seed()
    q, hq, classes = scenarios.draw_start_pool(["CubeS"] * N, orientation, K, np.random.RandomState(7), hand_offsets="pose")
    sim = _sim(N, "CubeS", horizon=HORIZON, auto_reset=True, precision=precision)
    ref = _sim(N, "CubeS", horizon=HORIZON, auto_reset=True, precision=precision)
    dt = sim.dtype
    tq, thq = torch.as_tensor(q), torch.as_tensor(hq)
    # what ks_reset to entry j returns, for every entry (second context)
    entry_obs = torch.stack([ref.reset(tq[j], thq[j]).clone() for j in range(K)])               # [K, N, 82]
    obs0 = sim.set_start_pool(tq, thq, seed).clone()
    idx, ep = (t.cpu().numpy() for t in sim.start_index())
    rec = dict(seed=seed, host_idx=host_idx, q=q, hq=hq, classes=classes, entry_obs=entry_obs.cpu().numpy(), obs0=obs0.cpu().numpy(), idx0=idx.copy(),
               ep0=ep.copy(), steps=[], dtype=dt)
    # the second context starts every env at the first one's draw for episode 0
    ref.reset(_entries(tq, idx, np.arange(N)), _entries(thq, idx, np.arange(N)))
    a = torch.tensor(ACTION, dtype=dt).unsqueeze(1).expand(4, N).contiguous()
    for t in range(STEPS):
        obs, rew, done, _ = sim.step(a)
        robs, rrew, rdone, _ = ref.step(a)
        torch.cuda.synchronize()
        idx, ep = (x.cpu().numpy() for x in sim.start_index())
        st = sim.get_state()
        d = done.cpu().numpy()
        rec["steps"].append(dict(obs=obs.cpu().numpy().copy(), final=sim.final_obs.cpu().numpy().copy(), rew=rew.cpu().numpy().copy(), done=d.copy(),
                                 robs=robs.cpu().numpy().copy(), rfinal=ref.final_obs.cpu().numpy().copy(), rrew=rrew.cpu().numpy().copy(),
                                 rdone=rdone.cpu().numpy().copy(), idx=idx.copy(), ep=ep.copy(), qpos=st["qpos"].cpu().numpy().copy(),
                                 qvel=st["qvel"].cpu().numpy().copy(), status=st["status"].cpu().numpy().copy()))
        fin = np.nonzero(d)[0]
        if len(fin):                                     # the host reset of the second context to the entries the first one drew
            ids = torch.as_tensor(fin, dtype=torch.int32)
            ref.reset(_entries(tq, idx[fin], fin), _entries(thq, idx[fin], fin), env_ids=ids)
    sim.close()
    ref.close()
    return rec


@pytest.mark.parametrize("precision", [32, 64])
def test_known_answers_of_the_draw(precision):
    """after every step start_index() is the host Philox sequence; after a restart obs is, bit for bit, what ks_reset to that entry returns on a
    second context, and the state is the entry"""
    r = _pool_run(precision, "normal")
    seed, host_idx = r["seed"], r["host_idx"]
    # by the host reference alone: every env uses at least 3 distinct entries in the episodes this run starts (a constant index cannot pass)
    assert min(len(set(row.tolist())) for row in host_idx) >= 3
    e = np.arange(N)
    npdt = np.float32 if precision == 32 else np.float64
    assert (r["ep0"] == 0).all() and (r["idx0"] == host_idx[:, 0]).all()
    assert np.array_equal(r["obs0"], r["entry_obs"][r["idx0"], e])
    episode = np.zeros(N, dtype=np.int64)
    used = [set([int(i)]) for i in r["idx0"]]
    restarts = 0
    for t, s in enumerate(r["steps"]):
        fin = s["done"] != 0
        assert (fin == ((t + 1) % HORIZON == 0)).all(), t              # this action never lifts: time limits only
        episode += fin
        want = start_index_reference(seed, e, episode, K)
        assert np.array_equal(s["ep"], episode) and np.array_equal(s["idx"], want), t
        assert (s["status"] & 2 == 0).all()
        if fin.any():
            f = np.nonzero(fin)[0]
            restarts += len(f)
            assert np.array_equal(s["obs"][f], r["entry_obs"][want[f], f]), t                    # the cached observation of the entry = ks_reset's
            assert np.array_equal(s["qpos"][:, f], r["q"][want[f], :, f].T.astype(npdt)), t      # the state is the entry
            assert (s["qvel"][:, f] == 0).all()
            assert np.abs(s["final"][f] - s["obs"][f]).max() > 1e-4                              # the terminal observation went to final_obs
            for i in f:
                used[i].add(int(want[i]))
    assert restarts == N * (STEPS // HORIZON)
    assert min(len(u) for u in used) >= 3 and (episode == STEPS // HORIZON).all()


def _assert_episodes_equal_host_resets(r):
    for t, s in enumerate(r["steps"]):
        fin = s["done"] != 0
        assert np.array_equal(s["done"], s["rdone"]) and np.array_equal(s["rew"], s["rrew"]), t
        # envs inside an episode: the observation; envs whose episode ended: the terminal observation (obs already holds the next start's)
        assert np.array_equal(s["obs"][~fin], s["robs"][~fin]), t
        assert np.array_equal(s["final"][fin], s["rfinal"][fin]), t
    return sum(int((s["done"] != 0).sum()) for s in r["steps"])


@pytest.mark.parametrize("precision", [32, 64])
def test_episodes_are_the_ones_a_host_reset_gives(precision):
    """every episode of the run above equals, bit for bit and step by step (obs, reward, done), the episode of a second context that was
    host-reset to the drawn entry and stepped with the same actions - as test_time_limit_done_and_auto_reset holds for the stored state"""
    r = _pool_run(precision, "normal")
    assert _assert_episodes_equal_host_resets(r) == N * (STEPS // HORIZON)
    # the pool's starts differ: so do the episodes of an env (the check above is not comparing constants)
    first = np.stack([s["obs"] for s in r["steps"][:HORIZON - 1]])
    second = np.stack([s["obs"] for s in r["steps"][HORIZON:2 * HORIZON - 1]])
    changed = r["steps"][HORIZON - 1]["idx"] != r["idx0"]
    assert changed.sum() > N // 2 and (np.abs(first - second).max(axis=(0, 2))[changed] > 1e-5).all()


@pytest.mark.parametrize("precision", [32, 64])
def test_the_hand_orientation_changes_with_the_drawn_entry(precision):
    """a pool drawn with the 'random' orientation rule: after a restart the env runs with the drawn entry's hand quaternion - its next
    steps' observations are those of a context host-reset to that entry (a stale per-step hand_quat would keep the last episode's)"""
    r = _pool_run(precision, "random")
    assert set(np.unique(r["classes"]).tolist()) == {"normal", "rotated", "top"}
    _assert_episodes_equal_host_resets(r)
    e = np.arange(N)
    prev_idx, prev_cls = r["idx0"], r["classes"][r["idx0"], e]
    switched = np.zeros(N, dtype=bool)
    for t, s in enumerate(r["steps"]):
        fin = s["done"] != 0
        if fin.any() and t + 1 < STEPS:
            cls = r["classes"][s["idx"], e]
            sw = fin & (cls != prev_cls)
            switched |= sw
            # the step right after the restart, for the envs whose orientation class changed with the draw
            nxt = r["steps"][t + 1]
            assert np.array_equal(nxt["obs"][sw], nxt["robs"][sw]), t
            # ... and it is not what the old orientation gives: the entries' reset observations differ between the classes
            assert (np.abs(r["entry_obs"][s["idx"], e] - r["entry_obs"][prev_idx, e]).max(axis=1)[sw] > 1e-3).all()
            prev_idx, prev_cls = np.where(fin, s["idx"], prev_idx), np.where(fin, cls, prev_cls)
    assert switched.sum() > N // 2


@pytest.mark.parametrize("precision", [32, 64])
def test_one_entry_equal_to_the_reset_start_is_no_pool_and_clearing_restores_it(precision):
    """K = 1 with the entry = the ks_reset start: bit-equal to a context without a pool over 70 steps (two auto-resets per env and the lifts'
    early ones); set_start_pool(k = 0) and ks_reset_objects with object_id clear the pool: today's behaviour again"""
    n = 64
    q0, hq = scenarios.config2_states(n)
    acts = torch.as_tensor(np.abs(scenarios.config_actions(n, 70)))            # positive: the hands close and lift, some episodes end early
    plain = _sim(n, "CubeS", horizon=30, auto_reset=True, precision=precision)
    pooled = _sim(n, "CubeS", horizon=30, auto_reset=True, precision=precision)
    with pytest.raises(RuntimeError, match="no start pool"):
        pooled.start_index()
    o0 = plain.reset(torch.as_tensor(q0), torch.as_tensor(hq)).clone()
    o1 = pooled.set_start_pool(torch.as_tensor(q0)[None], torch.as_tensor(hq)[None], seed=9).clone()
    assert torch.equal(o0, o1)

    def run_both(a_sim, b_sim, steps):
        dones = 0
        for t in range(steps):
            ra = [x.clone() for x in a_sim.step(acts[t])] + [a_sim.final_obs.clone()]
            rb = [x.clone() for x in b_sim.step(acts[t])] + [b_sim.final_obs.clone()]
            assert all(torch.equal(x, y) for x, y in zip(ra, rb)), t
            dones += int((ra[2] != 0).sum())
        sa, sb = a_sim.get_state(), b_sim.get_state()
        assert all(torch.equal(sa[k], sb[k]) for k in sa)
        return dones

    assert run_both(plain, pooled, 70) >= 2 * n
    idx, ep = pooled.start_index()
    assert (idx == 0).all() and (ep >= 2).all()
    # a pool of 8 different starts, then k = 0: every env keeps the start of its running episode as the stored initial state
    q, hq8, _ = scenarios.draw_start_pool(["CubeS"] * n, "normal", 8, np.random.RandomState(1))
    pooled.set_start_pool(torch.as_tensor(q), torch.as_tensor(hq8), seed=4)
    idx = pooled.start_index()[0].cpu().numpy()
    assert pooled.set_start_pool(None) is None
    with pytest.raises(RuntimeError, match="no start pool"):
        pooled.start_index()
    e = np.arange(n)
    plain.reset(torch.as_tensor(q[idx, :, e].T), torch.as_tensor(hq8[idx, :, e].T))
    run_both(plain, pooled, 35)
    # ks_reset_objects with object_id ends a pool
    pooled.set_start_pool(torch.as_tensor(q), torch.as_tensor(hq8), seed=5)
    ob = pooled.reset(torch.as_tensor(q0), torch.as_tensor(hq), object_id=np.zeros(n, dtype=np.int32)).clone()
    with pytest.raises(RuntimeError, match="no start pool"):
        pooled.start_index()
    assert torch.equal(ob, plain.reset(torch.as_tensor(q0), torch.as_tensor(hq)))
    run_both(plain, pooled, 35)
    # ... while a plain ks_reset of some envs keeps it: they run the caller's start, their next auto-reset draws again
    pooled.set_start_pool(torch.as_tensor(q), torch.as_tensor(hq8), seed=5)
    some = torch.arange(0, n, 2, dtype=torch.int32)
    pooled.reset(torch.as_tensor(q0[:, ::2]), torch.as_tensor(hq[:, ::2]), env_ids=some)
    st = pooled.get_state()["qpos"].cpu().numpy()
    assert np.array_equal(st[:, ::2], q0[:, ::2].astype(st.dtype))
    for t in range(30):
        pooled.step(torch.zeros(4, n))
    idx, ep = (x.cpu().numpy() for x in pooled.start_index())
    assert (ep == 1).all() and np.array_equal(idx, start_index_reference(5, e, 1, 8))
    assert np.array_equal(pooled.get_state()["qpos"].cpu().numpy(), q[idx, :, e].T.astype(st.dtype))
    plain.close()
    pooled.close()


def _ring_episodes(replay):
    key = lambda e: (len(e["reward"]), e["state"].tobytes(), e["action"].tobytes(), e["next_state"].tobytes(), e["reward"].tobytes(), e["not_done"].tobytes())
    return sorted(key(e) for e in replay.host_episodes())


def _rollout_setup(kind, n, horizon, k=6, pool_seed=21):
    from kinovagrasping_amd.ddpgfd import DDPGfD
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from kinovagrasping_amd.rollout import RolloutEngine
    rng = np.random.RandomState(13)
    if kind == "mixed":                 # BASELINE config 5's start states: 14 objects x 3 hand poses x mass / friction in one context
        oid, _, q0, hq, mf = scenarios.config5_states(n, seed=5)
        sim = _sim(n, scenarios.SHAPES, horizon=horizon, auto_reset=True)
        sim.reset(torch.as_tensor(q0), torch.as_tensor(hq), object_id=oid, mass_friction=mf)
        q, hqp, _ = scenarios.draw_start_pool([scenarios.SHAPES[i] for i in oid], "random", k, rng, hand_offsets="pose")
    elif kind == "multi-geom":          # one multi-geom shape on libkinova_sim_mg.so: the bottle above the closing hand, at k jittered places
        from tests.test_gpu_multi_geom import in_hand_start
        sim = _sim(n, "BottleS", horizon=horizon, auto_reset=True)
        assert sim.multi_geom
        q = np.repeat(np.repeat(in_hand_start("BottleS")[None, :, None], k, 0), n, 2)
        q[:, 9] += rng.uniform(-0.02, 0.02, (k, n))
        q[:, 10] += rng.uniform(-0.01, 0.01, (k, n))
        hqp = np.repeat(np.repeat(scenarios.hand_quat_for("normal")[None, :, None], k, 0), n, 2)
    else:
        sim = _sim(n, "CubeS", horizon=horizon, auto_reset=True, precision=64 if kind == "fp64" else 32)
        q, hqp, _ = scenarios.draw_start_pool(["CubeS"] * n, "normal", k, rng)
    obs0 = sim.set_start_pool(torch.as_tensor(q), torch.as_tensor(hqp), pool_seed)
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=64, hidden=(256, 256), device=sim.device)
    with torch.no_grad():                       # wrist ~ 0, fingers ~ 0.6: the hand closes, check_grasp fires, the scripted lift ends episodes early
        policy.actor.l3.bias.add_(torch.tensor([-6.0, 1.0, 0.8, 1.2], device=sim.device))
    replay = DeviceEpisodeReplay(n, capacity=8 * n, horizon=horizon, device=sim.device)
    eng = RolloutEngine(sim, policy, replay, expl_noise=0.1)
    eng.start(obs0)
    return sim, policy, replay, eng, k, pool_seed


@pytest.mark.parametrize("kind,n,plan,horizon,per,chunks", [("fp32", 272, "waves", 12, 9, 4), ("fp32", 4096, "waves", 12, 9, 4), ("fp32", 272, "waves", 30, 13, 5),
                                                            ("mixed", 272, None, 12, 9, 4), ("fp64", 272, "workgroups", 12, 9, 4),
                                                            ("multi-geom", 208, None, 12, 9, 4)])
def test_free_running_rollout_equals_the_lock_step_calls_with_a_pool(kind, n, plan, horizon, per, chunks):
    """test_free_running_rollout_equals_the_lock_step_calls' comparison with a start pool set on both sides: the draw lives in obs_finish, the one place
    k_obs, wg_obs (k_env_step, k_rollout) and obs_epilogue_f64 (k_rollout_f64) share - per env the same entries, the same bits, the same replay rows.
    horizon 12: three time limits per env in 36 env-steps; horizon 30, 65 env-steps: the actor closes the hand, the scripted lift ends episodes
    early - restarts that come from the lift, at different times in different envs"""
    from kinovagrasping_amd.pipeline import AsyncTrainer
    import warnings
    min_episodes = chunks * per // horizon
    sim, policy, replay, eng, k, pool_seed = _rollout_setup(kind, n, horizon)
    for _ in range(chunks * per):
        eng.step()
    torch.cuda.synchronize()
    st = sim.get_state()
    idx, ep = sim.start_index()
    ref = dict(obs=eng.obs.clone(), prev=eng.prev_obs.clone(), t=eng.t.clone(), ready=eng.ready.clone(), qpos=st["qpos"].clone(), status=st["status"].clone(),
               eps=_ring_episodes(replay), count=replay.count, idx=idx.clone(), ep=ep.clone())
    sim.close()
    # every env drew what the host reference says for its episode count, and the pool was used: most envs moved to another entry
    assert (ref["ep"] >= min_episodes).all()
    assert np.array_equal(ref["idx"].cpu().numpy(), start_index_reference(pool_seed, np.arange(n), ref["ep"].cpu().numpy(), k))
    sim, policy, replay, eng, k, pool_seed = _rollout_setup(kind, n, horizon)
    idx0 = sim.start_index()[0].clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=16)
    if plan is not None:
        assert sim.rollout_plan()[0] == plan, sim.rollout_plan()
    for _ in range(chunks):
        sim.rollout(per, tr.args)
        replay.commit_published()
    torch.cuda.synchronize()
    st, c = sim.get_state(), tr.counts()
    idx, ep = sim.start_index()
    print(f"free-running with a pool, {kind} n={n}: plan {sim.rollout_plan()}, {c}, ring {replay.count} episodes; lock step ring {ref['count']}")
    assert c["episodes_dropped"] == 0 and c["episodes_finished"] >= min_episodes * n and int(ep.sum()) == c["episodes_finished"]
    if horizon == 30:
        assert c["lifted"] > 0.05 * n and eng.t.unique().numel() > 1          # lifts ended episodes early: the envs' episode clocks are apart
    assert torch.equal(st["qpos"], ref["qpos"]) and torch.equal(st["status"], ref["status"])
    assert torch.equal(eng.obs, ref["obs"]) and torch.equal(eng.prev_obs, ref["prev"]) and torch.equal(eng.t, ref["t"]) and torch.equal(eng.ready, ref["ready"])
    assert torch.equal(tr.steps_total, torch.full_like(tr.steps_total, chunks * per))
    assert replay.count == ref["count"] and _ring_episodes(replay) == ref["eps"]
    assert torch.equal(idx, ref["idx"]) and torch.equal(ep, ref["ep"])
    assert (idx != idx0).float().mean().item() > 0.5
    sim.close()


def test_run_stage_with_a_start_pool_needs_no_host_reset_between_rounds(tmp_path):
    """curriculum.run_stage(starts_per_env=4): an auto-reset context whose envs draw their starts in the stepping kernel; two rounds see more
    distinct starts than there are envs"""
    from kinovagrasping_amd import curriculum
    from kinovagrasping_amd.ddpgfd import DDPGfD
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=8, hidden=(64, 64), device=torch.device("cuda", 0))
    plan = curriculum.experiment_plan(3, root=tmp_path)                  # `orientations`: CubeS in all three orientation classes
    assert plan["requested_shapes"] == ["CubeS"] and plan["requested_orientation"] == "random"
    out = curriculum.run_stage(plan, policy, n_envs=64, rounds=2, updates_per_round=2, load_previous=False, save=False, starts_per_env=4)
    print("run_stage with a pool:", {k: out[k] for k in ("distinct_starts", "updates", "num_success", "orientation_counts")})
    assert out["num_total"] == 64 and out["updates"] == 4
    assert 64 < out["distinct_starts"] <= 64 * 4
    # without a pool the stage runs the code as it stood: one host reset of every env per round
    out0 = curriculum.run_stage(plan, policy, n_envs=64, rounds=2, updates_per_round=1, load_previous=False, save=False)
    assert out0["distinct_starts"] == 128 and out0["updates"] == 2
