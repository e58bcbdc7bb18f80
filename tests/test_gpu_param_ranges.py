"""Per-episode parameter ranges (ks_set_param_ranges / ks_get_env_params, include/kinova_sim.h): every AUTO-RESET inside the stepping
kernels (ks_step: k_obs / wg_obs; ks_rollout: k_rollout, k_rollout_f64) draws the env's object mass and object-hand friction from the
env's ranges with a counter-based generator.  Pinned here: the draw against the host reference (scenarios.param_draw_reference) bit for
bit, the episodes against a second context whose parameters the HOST writes (ks_set_env_params) before the steps, one episode against
the fp64 oracle with the drawn values, the free-running kernels against the lock-step calls, the interactions with ks_set_env_params /
ks_reset_objects / clearing, a graph captured before the call, and curriculum.run_stage."""
import functools

import numpy as np
import pytest
import torch

from kinovagrasping_amd import scenarios
from tests.test_gpu_start_pool import ACTION, _ring_episodes, _rollout_setup

pytestmark = pytest.mark.gpu

N, HORIZON, STEPS = 64, 5, 40
EPISODES = STEPS // HORIZON


def _sim(*a, **k):
    from kinovagrasping_amd.sim import KinovaSim
    return KinovaSim(*a, **k)


def _starts(n=N):
    """CubeS starts beside the closing fingers: the first n rows of the reference's start table with |x| + y > 0.055.  There the fixed
    action's fingers reach the cube within an episode of five env-steps, so its mass and the finger friction show in the trajectory
    (rows in the middle of the table are not touched in five steps: their episodes would not depend on the parameters at all)."""
    tab = scenarios.start_coord_table("CubeS")
    rows = tab[np.abs(tab[:, 0]) + tab[:, 1] > 0.055][:n]
    assert len(rows) == n
    q = np.zeros((16, n))
    q[9:12], q[12] = rows.T, 1.0
    return q, np.repeat(scenarios.hand_quat_for("normal")[:, None], n, 1)


def _range_rows(n, dtype):
    r = scenarios.config5_param_ranges(n)
    return np.stack([r["mass"][0], r["mass"][1], r["mu"][0], r["mu"][1]]).astype(dtype)


def _pick_seed(n=N, episodes=EPISODES, span=0.4):
    """the first seed for which - by the host reference alone - every env's first `episodes` mass draws span at least `span` of its range"""
    rows = _range_rows(n, np.float64)
    for seed in range(1, 1000):
        mass, _ = scenarios.param_draw_reference(seed, np.arange(n)[:, None], np.arange(episodes)[None], rows, np.float64)
        if ((mass.max(1) - mass.min(1)) / (rows[1] - rows[0])).min() >= span:
            return seed
    raise AssertionError("no seed found")


def _params(sim):
    return tuple(x.cpu().numpy().copy() for x in sim.env_params())


@functools.lru_cache(maxsize=None)
def _ranges_run(precision):
    """64 CubeS envs with config 5's ranges, 40 lock-step ks_steps with a fixed action at horizon 5 - beside a second context WITHOUT
    ranges into which the host writes (ks_set_env_params) the values of the host reference before every step.  Returns everything both
    produced."""
    seed = _pick_seed()
    npdt = np.float32 if precision == 32 else np.float64
    q0, hq = _starts()
    sim = _sim(N, "CubeS", horizon=HORIZON, auto_reset=True, precision=precision)
    ref = _sim(N, "CubeS", horizon=HORIZON, auto_reset=True, precision=precision)
    sim.reset(torch.as_tensor(q0), torch.as_tensor(hq))
    ref.reset(torch.as_tensor(q0), torch.as_tensor(hq))
    nominal = _params(sim)
    ranges = sim.set_param_ranges(seed=seed, **scenarios.config5_param_ranges(N)).cpu().numpy()
    rec = dict(seed=seed, ranges=ranges, q0=q0, hq=hq, nominal=nominal, params0=_params(sim), steps=[], npdt=npdt)
    e = np.arange(N)
    episode = np.zeros(N, dtype=np.int64)
    a = torch.tensor(ACTION, dtype=sim.dtype).unsqueeze(1).expand(4, N).contiguous()
    for t in range(STEPS):
        ref.set_env_params(*scenarios.param_draw_reference(seed, e, episode, ranges, npdt))      # the host's write, from the host's reference
        obs, rew, done, _ = sim.step(a)
        robs, rrew, rdone, _ = ref.step(a)
        torch.cuda.synchronize()
        d = done.cpu().numpy().copy()
        st = sim.get_state()
        rec["steps"].append(dict(obs=obs.cpu().numpy().copy(), final=sim.final_obs.cpu().numpy().copy(), rew=rew.cpu().numpy().copy(), done=d,
                                 robs=robs.cpu().numpy().copy(), rfinal=ref.final_obs.cpu().numpy().copy(), rrew=rrew.cpu().numpy().copy(),
                                 rdone=rdone.cpu().numpy().copy(), params=_params(sim), qpos=st["qpos"].cpu().numpy().copy(),
                                 status=st["status"].cpu().numpy().copy()))
        episode += d != 0
    sim.close()
    ref.close()
    return rec


@pytest.mark.parametrize("precision", [32, 64])
def test_known_answers_of_the_draw_and_host_equivalence(precision):
    """after the call and after every step env_params() is the host reference, bit for bit, and `episode` the count of the env's dones;
    every step equals (obs, final obs, reward, done: bit for bit) the step of a context whose parameters the host wrote"""
    seed = _pick_seed()
    rows64 = _range_rows(N, np.float64)
    e = np.arange(N)
    # by the host reference alone: every env's first 8 mass draws span at least 40 % of its range (constants cannot pass)
    mass_ref, _ = scenarios.param_draw_reference(seed, e[:, None], np.arange(EPISODES)[None], rows64, np.float64)
    assert ((mass_ref.max(1) - mass_ref.min(1)) / (rows64[1] - rows64[0])).min() >= 0.4
    r = _ranges_run(precision)
    npdt, ranges = r["npdt"], r["ranges"]
    assert r["seed"] == seed and np.array_equal(ranges, _range_rows(N, npdt))
    m0, u0 = scenarios.param_draw_reference(seed, e, 0, ranges, npdt)
    assert np.array_equal(r["params0"][0], m0) and np.array_equal(r["params0"][1], u0) and (r["params0"][2] == 0).all()
    assert not np.array_equal(r["nominal"][0], m0) and (r["nominal"][2] == 0).all()
    episode = np.zeros(N, dtype=np.int64)
    for t, s in enumerate(r["steps"]):
        fin = s["done"] != 0
        assert (fin == ((t + 1) % HORIZON == 0)).all(), t              # this action never lifts: time limits only
        episode += fin
        mass, mu = scenarios.param_draw_reference(seed, e, episode, ranges, npdt)
        assert np.array_equal(s["params"][0], mass) and np.array_equal(s["params"][1], mu) and np.array_equal(s["params"][2], episode), t
        assert (s["status"] & 2 == 0).all()
        # the second context: the host wrote the same values before the step
        assert np.array_equal(s["done"], s["rdone"]) and np.array_equal(s["rew"], s["rrew"]), t
        assert np.array_equal(s["obs"], s["robs"]), t
        assert np.array_equal(s["final"][fin], s["rfinal"][fin]), t
    assert (episode == EPISODES).all()
    # the episodes of one env differ from each other (same start, other parameters): the check above is not comparing constants
    first = np.stack([s["obs"] for s in r["steps"][:HORIZON - 1]])
    second = np.stack([s["obs"] for s in r["steps"][HORIZON:2 * HORIZON - 1]])
    diff = np.abs(first - second).max(axis=(0, 2))
    print(f"precision {precision}: max |obs difference| between an env's first two episodes: median {np.median(diff):.2e}, envs > 1e-5: {(diff > 1e-5).sum()} of {N}")
    assert (diff > 1e-5).sum() > N // 2


def test_the_draw_reaches_the_physics():
    """16 envs of the run above, their second episode (the first that starts with an in-kernel draw), four env-steps after the restart:
    the state tracks the fp64 oracle whose obj_mass / obj_mu are the DRAWN values within test_gpu_config5's check (b) - median relative
    qpos error <= 5e-6, at least 90 % of the envs <= 2e-4 - and the same oracle with the model's nominal mass / friction is outside 2e-4
    on at least one env.
    The exact-mode run (precision 64) is the one compared: whether the physics used the drawn pair is then not blurred by what fp32
    rounding grows to over 60 contact-rich substeps; the fp32 kernels are tied to the same values by the test above (bit-equal to a
    context whose parameters ks_set_env_params wrote, the path test_gpu_config5 pins against the oracle)."""
    from kinovagrasping_amd.sim import SOLVER_ITERATIONS
    from oracle import ko_py as ko
    r = _ranges_run(64)
    envs = np.arange(0, N, N // 16)
    seed, ranges = r["seed"], r["ranges"]
    mass, mu = scenarios.param_draw_reference(seed, envs, 1, ranges, np.float64)
    assert np.array_equal(r["steps"][HORIZON - 1]["params"][0][envs], mass)          # what the kernel drew at the restart
    qg = r["steps"][2 * HORIZON - 2]["qpos"][:, envs]                                # four steps into episode 1
    model = ko.OracleModel(scenarios.model_blob("CubeS"))

    def oracle(params):
        out = []
        for k, i in enumerate(envs):
            o = ko.OracleSim(model, r["hq"][:, i].copy(), solver_iterations=SOLVER_ITERATIONS)
            if params is not None:
                o.s.obj_mass, o.s.obj_mu = params[0][k], params[1][k]
            o.env_reset(r["q0"][:, i].copy())
            for t in range(HORIZON - 1):
                o.env_step(np.array(ACTION))
            out.append(o.view("qpos").copy())
        return np.stack(out, 1)

    rel = lambda qo: np.abs(qg - qo).max(0) / np.maximum(1e-3, np.abs(qo).max(0))
    drawn, nominal = rel(oracle((mass, mu))), rel(oracle(None))
    print(f"episode 1 of 16 envs against the oracle: drawn values median rel qpos {np.median(drawn):.2e}, max {drawn.max():.2e}; "
          f"nominal values median {np.median(nominal):.2e}, max {nominal.max():.2e}")
    assert np.isfinite(qg).all()
    assert np.median(drawn) <= 5e-6 and (drawn <= 2e-4).mean() >= 0.9
    assert (nominal > 2e-4).any()


def _set_ranges(sim, n, seed):
    return sim.set_param_ranges(seed=seed, **scenarios.config5_param_ranges(n)).cpu().numpy()


@pytest.mark.parametrize("kind,n,plan", [("fp32", 272, "waves"), ("mixed", 272, None), ("fp64", 64, "workgroups"), ("multi-geom", 64, None)])
def test_free_running_rollout_equals_the_lock_step_calls_with_ranges_and_a_pool(kind, n, plan):
    """test_free_running_rollout_equals_the_lock_step_calls_with_a_pool's comparison with parameter ranges set on both sides, behind the
    pool: the draw lives in obs_finish, the one place k_obs, wg_obs (k_env_step, k_rollout) and obs_epilogue_f64 (k_rollout_f64) share - per
    env the same parameters, the same bits, the same replay rows.  horizon 12: three time limits per env in 36 env-steps"""
    from kinovagrasping_amd.pipeline import AsyncTrainer
    import warnings
    horizon, per, chunks, range_seed = 12, 9, 4, 33
    min_episodes = chunks * per // horizon
    npdt = np.float64 if kind == "fp64" else np.float32
    sim, policy, replay, eng, k, pool_seed = _rollout_setup(kind, n, horizon)
    before = _params(sim)
    ranges = _set_ranges(sim, n, range_seed)
    for _ in range(chunks * per):
        eng.step()
    torch.cuda.synchronize()
    st = sim.get_state()
    ref = dict(obs=eng.obs.clone(), prev=eng.prev_obs.clone(), t=eng.t.clone(), ready=eng.ready.clone(), qpos=st["qpos"].clone(), status=st["status"].clone(),
               eps=_ring_episodes(replay), count=replay.count, params=_params(sim), pool=[x.clone() for x in sim.start_index()])
    sim.close()
    # every env drew what the host reference says for its episode count (the pool's count: both are bumped at every auto-reset)
    mass, mu, ep = ref["params"]
    assert (ep >= min_episodes).all() and np.array_equal(ep, ref["pool"][1].cpu().numpy())
    want = scenarios.param_draw_reference(range_seed, np.arange(n), ep, ranges, npdt)
    assert np.array_equal(mass, want[0]) and np.array_equal(mu, want[1])
    assert not np.array_equal(mass, before[0])
    sim, policy, replay, eng, k, pool_seed = _rollout_setup(kind, n, horizon)
    assert np.array_equal(_set_ranges(sim, n, range_seed), ranges)
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
    got = _params(sim)
    print(f"free-running with ranges and a pool, {kind} n={n}: plan {sim.rollout_plan()}, {c}, ring {replay.count} episodes; lock step ring {ref['count']}")
    assert c["episodes_dropped"] == 0 and c["episodes_finished"] >= min_episodes * n and int(got[2].sum()) == c["episodes_finished"]
    assert torch.equal(st["qpos"], ref["qpos"]) and torch.equal(st["status"], ref["status"])
    assert torch.equal(eng.obs, ref["obs"]) and torch.equal(eng.prev_obs, ref["prev"]) and torch.equal(eng.t, ref["t"]) and torch.equal(eng.ready, ref["ready"])
    assert replay.count == ref["count"] and _ring_episodes(replay) == ref["eps"]
    assert all(np.array_equal(x, y) for x, y in zip(got, ref["params"]))
    assert all(torch.equal(x, y) for x, y in zip(sim.start_index(), ref["pool"]))
    sim.close()


@pytest.mark.parametrize("precision", [32, 64])
def test_constant_ranges_clearing_host_writes_and_object_changes(precision):
    n, seed = 64, 11
    npdt = np.float32 if precision == 32 else np.float64
    e = np.arange(n)
    q0, hq = _starts(n)
    tq, thq = torch.as_tensor(q0), torch.as_tensor(hq)
    a = torch.tensor(ACTION, dtype=torch.float64).unsqueeze(1).expand(4, n).contiguous()
    plain = _sim(n, "CubeS", horizon=HORIZON, auto_reset=True, precision=precision)
    sim = _sim(n, "CubeS", horizon=HORIZON, auto_reset=True, precision=precision)
    nominal = _params(plain)
    assert (nominal[0] == nominal[0][0]).all() and (nominal[2] == 0).all()
    # ranges with lo == hi == the current values: a run bit-equal to a context without ranges
    m5, u5 = scenarios.config5_env_params(n)
    for s in (plain, sim):
        s.set_env_params(m5, u5)
        s.reset(tq, thq)
    cur = sim.env_params()
    assert np.array_equal(cur[0].cpu().numpy(), m5.astype(npdt))
    sim.set_param_ranges(mass=(cur[0], cur[0]), mu=(cur[1], cur[1]), seed=seed)
    for t in range(2 * HORIZON + 2):
        ra = [x.clone() for x in plain.step(a)] + [plain.final_obs.clone()]
        rb = [x.clone() for x in sim.step(a)] + [sim.final_obs.clone()]
        assert all(torch.equal(x, y) for x, y in zip(ra, rb)), t
    sa, sb = plain.get_state(), sim.get_state()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    p = _params(sim)
    assert np.array_equal(p[0], m5.astype(npdt)) and np.array_equal(p[1], u5.astype(npdt)) and (p[2] == 2).all()
    # None for one parameter keeps it constant at the envs' current values
    sim.reset(tq, thq)
    ranges = sim.set_param_ranges(mass=(0.05, 0.15), seed=seed).cpu().numpy()
    assert np.array_equal(ranges[2], u5.astype(npdt)) and np.array_equal(ranges[3], u5.astype(npdt))
    for t in range(HORIZON):
        sim.step(a)
    p = _params(sim)
    want = scenarios.param_draw_reference(seed, e, 1, ranges, npdt)
    assert np.array_equal(p[0], want[0]) and np.array_equal(p[1], u5.astype(npdt)) and (p[2] == 1).all()
    assert np.unique(p[0]).size > n // 2
    # ks_set_env_params mid-episode holds until the env's next done, then the draw resumes at the right episode number; ks_reset keeps the ranges
    ranges = _set_ranges(sim, n, seed)
    sim.reset(tq, thq)
    sim.step(a)
    sim.step(a)
    sim.set_env_params(np.full(n, 0.123), np.full(n, 0.77))
    for t in range(2):
        sim.step(a)
        p = _params(sim)
        assert (p[0] == npdt(0.123)).all() and (p[1] == npdt(0.77)).all() and (p[2] == 0).all()
    _, _, done, _ = sim.step(a)
    assert (done != 0).all()
    p = _params(sim)
    want = scenarios.param_draw_reference(seed, e, 1, ranges, npdt)
    assert np.array_equal(p[0], want[0]) and np.array_equal(p[1], want[1]) and (p[2] == 1).all()
    # clearing keeps the running values, and nothing is drawn afterwards
    assert sim.set_param_ranges(None) is None
    for t in range(HORIZON + 1):
        sim.step(a)
    q = _params(sim)
    assert all(np.array_equal(x, y) for x, y in zip(p, q))
    # ks_reset_objects with object_id clears the ranges: the object's own values, no draw at the next auto-reset
    _set_ranges(sim, n, seed)
    assert not np.array_equal(_params(sim)[0], nominal[0])
    sim.reset(tq, thq, object_id=np.zeros(n, dtype=np.int32))
    for t in range(HORIZON + 1):
        sim.step(a)
    p = _params(sim)
    assert np.array_equal(p[0], nominal[0]) and np.array_equal(p[1], nominal[1])
    # ... while mass_friction alone behaves like ks_set_env_params: the running episode's values, the next auto-reset draws again
    ranges = _set_ranges(sim, n, seed)
    sim.reset(tq, thq, mass_friction=np.stack([np.full(n, 0.11), np.full(n, 0.9)]))
    p = _params(sim)
    assert (p[0] == npdt(0.11)).all() and (p[1] == npdt(0.9)).all()
    for t in range(HORIZON):
        sim.step(a)
    p = _params(sim)
    want = scenarios.param_draw_reference(seed, e, 1, ranges, npdt)
    assert np.array_equal(p[0], want[0]) and np.array_equal(p[1], want[1]) and (p[2] == 1).all()
    plain.close()
    sim.close()


def test_ranges_need_auto_reset():
    sim = _sim(16, "CubeS", horizon=HORIZON, auto_reset=False)
    with pytest.raises(RuntimeError, match="auto_reset"):
        sim.set_param_ranges(mass=(0.05, 0.15), mu=(0.5, 1.0))
    with pytest.raises(ValueError, match="lo > hi"):
        sim.set_param_ranges(mass=(0.15, 0.05), mu=(0.5, 1.0))
    mass, mu, ep = sim.env_params()                                  # ks_get_env_params needs no ranges
    assert (mass > 0).all() and (mu > 0).all() and (ep == 0).all()
    sim.close()


def test_a_step_captured_before_the_call_draws_when_replayed_after_it():
    """the ranges' record lives in device memory and is written by the stream: a ks_step graph captured on a context without ranges draws
    once ranges are set (default queue settings, a single-branch graph)"""
    n, seed = 64, 17
    q0, hq = _starts(n)
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
    nominal = _params(sim)
    for _ in range(HORIZON):                                         # replays without ranges: nothing is drawn
        g.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(_params(sim), nominal))
    sim.reset(torch.as_tensor(q0), torch.as_tensor(hq))
    ranges = _set_ranges(sim, n, seed)
    e = np.arange(n)
    for episode in range(1, 4):
        for _ in range(HORIZON):
            g.replay()
        torch.cuda.synchronize()
        assert (sim.done != 0).all()
        mass, mu, ep = _params(sim)
        want = scenarios.param_draw_reference(seed, e, episode, ranges, np.float32)
        assert (ep == episode).all() and np.array_equal(mass, want[0]) and np.array_equal(mu, want[1]), episode
    sim.close()


def test_run_stage_with_parameter_ranges(tmp_path):
    """curriculum.run_stage(starts_per_env=4, param_ranges=config 5's): every episode of the rounds is counted in the (mass, friction)
    table; without a pool the ranges have nothing to draw at"""
    from kinovagrasping_amd import curriculum
    from kinovagrasping_amd.ddpgfd import DDPGfD
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=8, hidden=(64, 64), device=torch.device("cuda", 0))
    plan = curriculum.experiment_plan(3, root=tmp_path)
    out = curriculum.run_stage(plan, policy, n_envs=64, rounds=2, updates_per_round=2, load_previous=False, save=False, starts_per_env=4,
                               param_ranges=scenarios.config5_param_ranges(64))
    ps = out["param_success"]
    attempts, successes = np.asarray(ps["attempts"]), np.asarray(ps["successes"])
    print("run_stage with ranges:", out["episodes"], "episodes;", attempts.tolist(), successes.tolist())
    assert out["episodes"] >= 2 * 64 and attempts.sum() == out["episodes"]
    assert attempts.shape == (4, 4) and (successes <= attempts).all() and (attempts > 0).sum() >= 8
    assert successes.sum() == sum(v["successes"] for v in out["per_shape_success"].values())
    assert np.allclose(ps["mass_edges"], np.linspace(np.float32(0.05), np.float32(0.15), 5)) and np.allclose(ps["mu_edges"], np.linspace(0.5, 1.0, 5))
    with pytest.raises(ValueError, match="starts_per_env"):
        curriculum.run_stage(plan, policy, n_envs=64, rounds=1, updates_per_round=1, load_previous=False, save=False,
                             param_ranges=scenarios.config5_param_ranges(64))
