"""The in-kernel episode log (ks_set_episode_log / ks_get_episode_log, include/kinova_sim.h): one record per episode that ends and restarts
inside the stepping kernels, written in obs_finish - the place k_obs, wg_obs (k_env_step, k_rollout) and the fp64 rollout share.  Pinned
here: the records of lock-step runs against known answers and against a ledger the host keeps from the per-step outputs, the free-running
kernels against the lock-step calls (bit for bit in every word), the ring's wrap, that a log changes nothing else, a ks_step captured
before the log was set, evaluate.eval_policy_free_running against a lock-step evaluation, and curriculum.run_stage's per-shape fold."""
import functools
import warnings

import numpy as np
import pytest
import torch

from kinovagrasping_amd import scenarios
from tests.test_gpu_start_pool import ACTION, HORIZON, K, N, STEPS, _pool_run, _ring_episodes, _rollout_setup, _sim
from tests.test_start_pool_cpu import start_index_reference

pytestmark = pytest.mark.gpu

EPISODES = STEPS // HORIZON


def _words(rec):
    """episode_log()'s fields back as the records' 8 words, int32 [m, 8]"""
    xy = rec["start_xy"].contiguous().view(torch.int32)
    return torch.stack([rec["env"], rec["object"], rec["start_index"], rec["steps"], rec["done"], xy[:, 0], xy[:, 1], rec["episode"]], 1).cpu().numpy()


def _by_env_episode(words):
    return words[np.lexsort((words[:, 7], words[:, 0]))]


@functools.lru_cache(maxsize=None)
def _lock_step_log(precision, capacity):
    """_pool_run's case with an episode log: 64 CubeS envs, a pool of 8 starts, horizon 5, 40 ks_steps with the fixed action that never lifts"""
    r = _pool_run(precision, "normal")
    sim = _sim(N, "CubeS", horizon=HORIZON, auto_reset=True, precision=precision)
    obs0 = sim.set_start_pool(torch.as_tensor(r["q"]), torch.as_tensor(r["hq"]), r["seed"]).clone()
    sim.set_episode_log(capacity)
    a = torch.tensor(ACTION, dtype=sim.dtype).unsqueeze(1).expand(4, N).contiguous()
    steps = []
    for t in range(STEPS):
        obs, rew, done, _ = sim.step(a)
        steps.append(dict(obs=obs.cpu().numpy().copy(), final=sim.final_obs.cpu().numpy().copy(), rew=rew.cpu().numpy().copy(), done=done.cpu().numpy().copy()))
    ring, written = sim.episode_log_raw()
    rec = sim.episode_log()
    st = sim.get_state()
    out = dict(rec=rec, words=_words(rec), ring=ring.cpu().numpy(), written=int(written.item()), obs0=obs0.cpu().numpy(), steps=steps,
               qpos=st["qpos"].cpu().numpy())
    sim.close()
    return out


@pytest.mark.parametrize("precision", [32, 64])
def test_lock_step_records_are_the_known_answers(precision):
    """exactly 64 x 8 records; per env the ordinals 0..7 in ticket order, 5 steps, time limit, object 0, the pool entry the host Philox reference
    gives for that episode, and the start coordinates = columns 21, 22 of what ks_reset to that entry returns (fp64: rounded to fp32 once)"""
    r = _pool_run(precision, "normal")
    log = _lock_step_log(precision, N * EPISODES)
    w = log["words"]
    assert log["written"] == N * EPISODES and log["rec"]["lost"] == 0 and w.shape == (N * EPISODES, 8)
    for e in range(N):
        mine = w[w[:, 0] == e]
        assert mine[:, 7].tolist() == list(range(EPISODES)), e                     # ticket order = episode order for one env
    assert (w[:, 3] == HORIZON).all() and (w[:, 4] == 2).all() and (w[:, 1] == 0).all()
    want = start_index_reference(r["seed"], w[:, 0].astype(np.int64), w[:, 7].astype(np.int64), K)
    assert np.array_equal(w[:, 2], want)
    assert min(len(set(w[w[:, 0] == e][:, 2].tolist())) for e in range(N)) >= 3     # (the pool was used: no constant index passes)
    xy = r["entry_obs"][w[:, 2], w[:, 0]][:, 21:23].astype(np.float32)              # ks_reset to that entry, second context
    assert np.array_equal(w[:, 5:7], xy.view(np.int32))
    assert np.abs(xy).max() > 1e-3 and len(np.unique(xy[:, 0])) > N
    # ... and the run is, step by step, the run without a log (_pool_run)
    assert np.array_equal(log["obs0"], r["obs0"])
    for t, (s, s0) in enumerate(zip(log["steps"], r["steps"])):
        assert all(np.array_equal(s[k], s0[k]) for k in ("obs", "final", "rew", "done")), t
    assert np.array_equal(log["qpos"], r["steps"][-1]["qpos"])


def _engine_log_run(kind, n, horizon, steps):
    """`steps` lock-step eng.step()s of _rollout_setup's engine with a log; returns the log's records, the ledger the host builds from the engine's
    per-step outputs and start_index(), and the run's end state"""
    sim, policy, replay, eng, k, pool_seed = _rollout_setup(kind, n, horizon)
    sim.set_episode_log(n * steps)
    obj = np.zeros(n, dtype=np.int64)
    if kind == "mixed":
        obj = np.asarray(scenarios.config5_states(n, seed=5)[0]).astype(np.int64)
    start_xy = sim.obs[:, 21:23].float().cpu().numpy().copy()                  # the observation the running episode began with
    length, ordinal = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    host = []
    for t in range(steps):
        idx = sim.start_index()[0].cpu().numpy()                                # the entry every running episode started from
        reward, done_b = eng.step()
        torch.cuda.synchronize()
        d, rew = sim.done.cpu().numpy().astype(np.int64), sim.reward.cpu().numpy()
        assert np.array_equal(d != 0, done_b.cpu().numpy()) and np.array_equal((d & 1) != 0, rew > 25)
        length += 1
        now = sim.obs[:, 21:23].float().cpu().numpy()
        for e in np.nonzero(d)[0]:
            host.append((e, obj[e], idx[e], length[e], d[e]) + tuple(start_xy[e].view(np.int32).tolist()) + (ordinal[e],))
            ordinal[e] += 1
            length[e] = 0
            start_xy[e] = now[e]
    rec = sim.episode_log()
    st = sim.get_state()
    out = dict(words=_words(rec), lost=rec["lost"], written=rec["written"], host=np.asarray(host, dtype=np.int64).reshape(-1, 8).astype(np.int32),
               obs=eng.obs.clone(), qpos=st["qpos"].clone(), eps=_ring_episodes(replay), count=replay.count)
    sim.close()
    return out


def test_lock_step_engine_records_equal_a_host_ledger():
    """272 envs, horizon 30, 65 env-steps of the engine whose actor closes the hand: lifts end episodes early, at different times in different envs"""
    out = _engine_log_run("fp32", 272, 30, 65)
    host = out["host"]
    lifted = host[(host[:, 4] & 1) != 0]
    # by the host ledger alone: lifts, time limits, and lifted episodes of different lengths
    assert len(lifted) > 0 and (host[:, 4] == 2).any() and len(np.unique(lifted[:, 3])) >= 2, (len(lifted), np.unique(host[:, 4]), np.unique(lifted[:, 3]))
    assert out["lost"] == 0 and out["written"] == len(host)
    assert np.array_equal(_by_env_episode(out["words"]), _by_env_episode(host))


@pytest.mark.parametrize("kind,n,plan,horizon,per,chunks", [("fp32", 272, "waves", 12, 9, 4), ("fp32", 4096, "waves", 12, 9, 4), ("fp32", 272, "waves", 30, 13, 5),
                                                            ("mixed", 272, None, 12, 9, 4), ("fp64", 272, "workgroups", 12, 9, 4),
                                                            ("multi-geom", 208, None, 12, 9, 4)])
def test_free_running_records_equal_the_lock_step_ones(kind, n, plan, horizon, per, chunks):
    """the six cases of test_free_running_rollout_equals_the_lock_step_calls_with_a_pool: the records of the ks_rollout run, sorted by (env, episode), are
    those of the lock-step engine run in every word; as many as counters[0] finished episodes, counters[1] of them lifted"""
    from kinovagrasping_amd.pipeline import AsyncTrainer
    ref = _engine_log_run(kind, n, horizon, chunks * per)
    assert ref["lost"] == 0 and np.array_equal(_by_env_episode(ref["words"]), _by_env_episode(ref["host"]))
    sim, policy, replay, eng, k, pool_seed = _rollout_setup(kind, n, horizon)
    sim.set_episode_log(n * chunks * per)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=16)
    if plan is not None:
        assert sim.rollout_plan()[0] == plan, sim.rollout_plan()
    for _ in range(chunks):
        sim.rollout(per, tr.args)
        replay.commit_published()
    torch.cuda.synchronize()
    rec, c = sim.episode_log(), tr.counts()
    w = _words(rec)
    print(f"episode log, free-running {kind} n={n}: {len(w)} records, {int((w[:, 4] & 1).sum())} lifted, counters {c}")
    assert rec["lost"] == 0 and rec["written"] == len(w) == c["episodes_finished"] and len(w) >= (chunks * per // horizon) * n
    assert int(((w[:, 4] & 1) != 0).sum()) == c["lifted"]
    if kind == "mixed":
        assert len(np.unique(w[:, 1])) > 1                                     # the records name the envs' objects
    if horizon == 30:
        assert c["lifted"] > 0
    assert np.array_equal(_by_env_episode(w), _by_env_episode(ref["words"]))
    assert torch.equal(sim.get_state()["qpos"], ref["qpos"]) and torch.equal(eng.obs, ref["obs"])
    sim.close()


@pytest.mark.parametrize("capacity", [3 * N, 2 * N + N // 2])
def test_the_ring_wraps_and_keeps_the_last_records(capacity):
    """a ring smaller than the run's 512 episodes (a whole number of lock-step launches, and two and a half): `written` is the true total, the ring
    holds exactly the last `capacity` tickets - a launch of this run takes 64 consecutive tickets, so ticket t belongs to episode t // 64 -, and every
    survivor is the record of the un-wrapped run"""
    full = _lock_step_log(32, N * EPISODES)
    log = _lock_step_log(32, capacity)
    total = N * EPISODES
    assert log["written"] == total and log["rec"]["lost"] == total - capacity
    w = log["words"]
    assert w.shape == (capacity, 8)
    tickets = np.arange(total - capacity, total)
    assert np.array_equal(w[:, 7], tickets // N)                                # oldest first, and nothing older than the last `capacity`
    assert np.array_equal(log["ring"][tickets % capacity][:, 7], tickets // N)  # slot = ticket % capacity
    for e in range(N):
        o = w[w[:, 0] == e][:, 7]
        assert (np.diff(o) == 1).all() and o[-1] == EPISODES - 1, e
    ref = {(r[0], r[7]): r for r in full["words"]}
    assert len({(r[0], r[7]) for r in w}) == capacity
    assert all(np.array_equal(r, ref[(r[0], r[7])]) for r in w)


def test_a_log_changes_nothing_else_and_the_error_paths():
    """the same free-running run with and without a log: bit-equal outputs, state and replay ring; capacity 0 clears the log; ks_get_episode_log
    without a log and ks_set_episode_log without auto_reset return KS_ERR_STATE (-5)"""
    from kinovagrasping_amd.pipeline import AsyncTrainer
    runs = []
    for with_log in (False, True):
        sim, policy, replay, eng, k, pool_seed = _rollout_setup("fp32", 272, 30)
        if with_log:
            sim.set_episode_log(272 * 65)
        else:
            with pytest.raises(RuntimeError, match=r"error -5.*no episode log"):
                sim.episode_log()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=16)
        for _ in range(5):
            sim.rollout(13, tr.args)
            replay.commit_published()
        torch.cuda.synchronize()
        st = sim.get_state()
        runs.append(dict(obs=sim.obs.clone(), final=sim.final_obs.clone(), reward=sim.reward.clone(), done=sim.done.clone(), eobs=eng.obs.clone(),
                         qpos=st["qpos"].clone(), qvel=st["qvel"].clone(), warm=st["qacc_warmstart"].clone(), status=st["status"].clone(),
                         idx=sim.start_index()[0].clone(), ep=sim.start_index()[1].clone(), eps=_ring_episodes(replay), count=replay.count, c=tr.counts()))
        if with_log:
            rec = sim.episode_log()
            assert rec["written"] > 272 and rec["lost"] == 0
            assert rec["written"] == int(runs[-1]["ep"].sum())                  # every auto-reset since the pool was set was logged
            # the log survives the pool being cleared and a host reset, which logs nothing ...
            sim.set_start_pool(None)
            q0, hq = scenarios.config2_states(272)
            sim.reset(torch.as_tensor(q0), torch.as_tensor(hq))
            assert sim.episode_log()["written"] == rec["written"]
            for _ in range(30):
                sim.step(torch.zeros(4, 272))
            more = sim.episode_log()
            assert more["written"] >= rec["written"] + 272 and (more["start_index"] == -1).all() and (more["episode"] >= 1).all()
            # ... capacity 0 clears it, and a new log starts from nothing
            sim.set_episode_log(0)
            with pytest.raises(RuntimeError, match=r"error -5.*no episode log"):
                sim.episode_log()
            for _ in range(30):
                sim.step(torch.zeros(4, 272))
            sim.set_episode_log(272)
            assert sim.episode_log()["written"] == 0
            for _ in range(30):
                sim.step(torch.zeros(4, 272))
            again = sim.episode_log()
            assert again["written"] >= 272 and (again["episode"] == 0).sum() == 272
            with pytest.raises(RuntimeError, match=r"error -1"):
                sim.set_episode_log(271)                                        # fewer records than envs
        sim.close()
    a, b = runs
    for key in ("obs", "final", "reward", "done", "eobs", "qpos", "qvel", "warm", "status", "idx", "ep"):
        assert torch.equal(a[key], b[key]), key
    assert a["count"] == b["count"] and a["eps"] == b["eps"] and a["c"] == b["c"]
    plain = _sim(64, "CubeS", horizon=HORIZON, auto_reset=False)
    with pytest.raises(RuntimeError, match=r"error -5.*auto_reset"):
        plain.set_episode_log(64)
    plain.close()


def test_a_step_captured_before_the_log_is_set_logs_when_replayed():
    """the log's descriptor lives in device memory: a ks_step captured in a HIP graph while the context held no log writes records once one is set"""
    n = 256
    q0, hq = scenarios.config2_states(n)
    sim = _sim(n, "CubeS", auto_reset=True, horizon=HORIZON)
    sim.reset(torch.as_tensor(q0), torch.as_tensor(hq))
    act = torch.tensor(ACTION, device=sim.device).unsqueeze(1).expand(4, n).contiguous()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sim.step(act)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        sim.step(act)
    for _ in range(HORIZON):                                                   # replays without a log: nothing is written anywhere
        g.replay()
    sim.set_episode_log(4 * n)
    dones = 0
    for _ in range(2 * HORIZON):
        g.replay()
        dones += int((sim.done != 0).sum())
    rec = sim.episode_log()
    assert dones >= 2 * n - n and rec["written"] == dones and rec["lost"] == 0
    assert (rec["start_index"] == -1).all() and (rec["object"] == 0).all() and (rec["steps"] <= HORIZON).all()
    for e in (0, n - 1):
        assert rec["episode"][rec["env"] == e].tolist() == list(range(int((rec["env"] == e).sum())))
    sim.close()


def _eval_setup(n=272, k=6, horizon=30):
    from kinovagrasping_amd.ddpgfd import DDPGfD
    q, hq, classes = scenarios.draw_start_pool(["CubeS"] * n, "normal", k, np.random.RandomState(13))        # _rollout_setup's pool
    sim = _sim(n, "CubeS", horizon=horizon, auto_reset=True)
    obs0 = sim.set_start_pool(torch.as_tensor(q), torch.as_tensor(hq), 21).clone()
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=64, hidden=(256, 256), device=sim.device)
    with torch.no_grad():                       # as _rollout_setup: the hand closes, check_grasp fires, the scripted lift ends episodes early
        policy.actor.l3.bias.add_(torch.tensor([-6.0, 1.0, 0.8, 1.2], device=sim.device))
    return sim, policy, obs0, q, hq, classes


def test_free_running_evaluation_equals_a_lock_step_one(tmp_path):
    """eval_policy_free_running (ks_rollout, sigma 0, nothing stored, the log read back) against one episode per env of the lock-step RolloutEngine
    without noise on the same pool: per env the same outcome and the same number of steps"""
    from kinovagrasping_amd import metrics
    from kinovagrasping_amd.evaluate import eval_policy, eval_policy_free_running
    from kinovagrasping_amd.rollout import RolloutEngine
    n, horizon = 272, 30
    sim, policy, obs0, q, hq, classes = _eval_setup(n, horizon=horizon)
    idx0 = sim.start_index()[0].cpu().numpy()
    eng = RolloutEngine(sim, policy, None, expl_noise=0.0)
    eng.start(obs0)
    success, steps = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    for t in range(horizon):
        eng.step()
        torch.cuda.synchronize()
        d = sim.done.cpu().numpy()
        first = (d != 0) & (steps == 0)
        success[first], steps[first] = (d[first] & 1) != 0, t + 1
    sim.close()
    assert (steps > 0).all()
    assert success.any() and len(np.unique(steps)) >= 2                         # the comparison has lifts, and episodes of different lengths
    sim, policy, obs0, q, hq, classes = _eval_setup(n, horizon=horizon)
    res = eval_policy_free_running(sim, policy, obs0=obs0, classes=classes)
    with pytest.raises(RuntimeError, match="no episode log"):                  # its own log is cleared behind it
        sim.episode_log()
    sim.close()
    assert np.array_equal(res["success"].cpu().numpy(), success) and np.array_equal(res["steps"].cpu().numpy(), steps)
    assert np.array_equal(res["start_index"].cpu().numpy(), idx0)
    assert res["num_success"] == int(success.sum()) and res["avg_reward"] == pytest.approx(50.0 * success.mean())
    assert res["avg_rewards"]["lift_reward"] == res["avg_reward"] and res["avg_rewards"]["finger_reward"] == 0.0
    assert res["per_object"] == {0: {"attempts": n, "successes": int(success.sum()), "mean_steps": steps.sum() / n}}
    e = np.arange(n)
    assert sorted(res["success_coords"]["orientation"]) == sorted(classes[idx0, e][success].tolist())
    assert np.array_equal(np.sort(np.asarray(res["success_coords"]["x"], dtype=np.float32)), np.sort(obs0[:, 21].cpu().numpy()[success]))
    text = metrics.save_heatmap_coords(res["success_coords"], res["fail_coords"], 0, tmp_path)
    assert f"Total # Success: {int(success.sum())}" in text and f"Total # Fail: {int((~success).sum())}" in text
    assert (tmp_path / "heatmap_info.txt").exists()
    # for the record only (torch actor, not bit-equal to the in-kernel MFMA actor): eval_policy on a context host-reset to the same starts
    plain = _sim(n, "CubeS", horizon=horizon, auto_reset=False)
    tq, thq = torch.as_tensor(q), torch.as_tensor(hq)
    o = plain.reset(tq[torch.as_tensor(idx0).long(), :, torch.as_tensor(e)].t().contiguous(), thq[torch.as_tensor(idx0).long(), :, torch.as_tensor(e)].t().contiguous())
    host = eval_policy(plain, policy, o, horizon=horizon)
    plain.close()
    print(f"evaluation of {n} starts: eval_policy_free_running success rate {res['num_success'] / n:.4f}, eval_policy (torch actor) {host['num_success'] / n:.4f}, "
          f"per-env outcomes that differ: {int((host['success'].cpu().numpy() != success).sum())}")


def _count_done_flags(monkeypatch):
    """the done flags the round loop of run_stage sees: every RolloutEngine.step() of the stage adds its done_out (the final evaluation steps the
    simulator itself, not the engine)"""
    from kinovagrasping_amd.rollout import RolloutEngine
    seen = {"flags": torch.zeros((), dtype=torch.long, device="cuda:0"), "steps": 0}
    step = RolloutEngine.step

    def counting_step(self, *a, **kw):
        out = step(self, *a, **kw)
        seen["flags"] += (self.done_out != 0).sum()
        seen["steps"] += 1
        return out
    monkeypatch.setattr(RolloutEngine, "step", counting_step)
    return seen


def test_run_stage_returns_the_per_shape_fold(tmp_path, monkeypatch):
    """curriculum.run_stage(starts_per_env=4): per_shape_success' attempts sum to `episodes`, the number of done flags the round loop saw"""
    from kinovagrasping_amd import curriculum
    from kinovagrasping_amd.ddpgfd import DDPGfD
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=8, hidden=(64, 64), device=torch.device("cuda", 0))
    plan = curriculum.experiment_plan(3, root=tmp_path)
    seen = _count_done_flags(monkeypatch)
    out = curriculum.run_stage(plan, policy, n_envs=64, rounds=2, updates_per_round=2, load_previous=False, save=False, starts_per_env=4)
    flags = int(seen["flags"])
    print("run_stage with a log:", {k: out[k] for k in ("episodes", "per_shape_success", "distinct_starts")}, "done flags seen:", flags)
    per = out["per_shape_success"]
    assert list(per) == ["CubeS"] and seen["steps"] == 2 * 30
    assert sum(v["attempts"] for v in per.values()) == out["episodes"] == flags >= 2 * 64
    assert 0 <= per["CubeS"]["successes"] <= per["CubeS"]["attempts"] and 0 < per["CubeS"]["mean_steps"] <= 30
    # what the stage returned before is still there, and nothing but the two keys was added; without a pool there is no log and no new key
    assert out["num_total"] == 64 and out["updates"] == 4 and 64 < out["distinct_starts"] <= 64 * 4
    out0 = curriculum.run_stage(plan, policy, n_envs=64, rounds=1, updates_per_round=1, load_previous=False, save=False)
    assert "per_shape_success" not in out0 and "episodes" not in out0
    assert set(out) - set(out0) == {"per_shape_success", "episodes"}


def test_run_stage_counts_every_shape_of_a_two_shape_stage(tmp_path, monkeypatch):
    """a stage of two shapes with a pool: every env runs - and its records name - its own shape's object.  64 envs, 32 per shape, two rounds of
    30 env-steps at horizon 30: every env ends at least one episode per round, so each shape has at least 2 x 32 attempts"""
    from kinovagrasping_amd import curriculum
    from kinovagrasping_amd.ddpgfd import DDPGfD
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=8, hidden=(64, 64), device=torch.device("cuda", 0))
    plan = dict(curriculum.experiment_plan(3, root=tmp_path), requested_shapes=["CubeS", "CylinderS"])
    seen = _count_done_flags(monkeypatch)
    out = curriculum.run_stage(plan, policy, n_envs=64, rounds=2, updates_per_round=2, load_previous=False, save=False, starts_per_env=4)
    flags = int(seen["flags"])
    per = out["per_shape_success"]
    print("run_stage, two shapes:", {k: out[k] for k in ("episodes", "per_shape_success")}, "done flags seen:", flags)
    assert list(per) == ["CubeS", "CylinderS"] and out["shapes"] == ["CubeS", "CylinderS"]
    assert all(v["attempts"] >= 2 * 32 for v in per.values()), per
    assert sum(v["attempts"] for v in per.values()) == out["episodes"] == flags
    assert all(0 <= v["successes"] <= v["attempts"] and 0 < v["mean_steps"] <= 30 for v in per.values())
