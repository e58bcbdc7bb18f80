"""Observation, reward, done and the episode bookkeeping of every GPU path (build_obs of csrc/ks_obs.h; obs_write / obs_finish / wg_obs /
obs_epilogue_f64 / k_obs of csrc/ks_api.hip) against the fp64 reference and the derived bound of tests/obs_ref.py on the aimed states of
tests/obs_states.py.  tests/test_obs_cpu.py holds the host lane of the same source to the same bounds and checks the classes' conditions.

  snapshot path   every class through ks_obs_from_snapshot (k_obs mode 2) in precision 64 and 32, in both layouts of the observation: the
                  slot-major result is the transpose of the env-major one bit for bit; a mixed-object context of three shapes
  in-step paths   the classes that a qpos and a hand quaternion express, ks_reset then ONE env-step with frame_skip = 1 (the snapshot of
                  the only substep is the reset pose, whatever the action: tests/test_gpu_rays.py): ks_step (wg_obs<false>, four waves),
                  KS_OBS_IN_STEP=0 (k_obs mode 0), fp64 ks_step, ks_rollout's free waves (wg_obs<true>), its workgroup form, the queue form
                  (Vase1S, 4096 envs), k_rollout_f64.  Non-ray slots: the bound plus the kinematic term (obs_ref.py); the reference takes the
                  path's own rays, which follow the ray tolerance of tests/ray_poses.py against the oracle's.  All fp32 in-step paths return
                  the same bits per state, k_rollout_f64 those of fp64 ks_step, and four placements (the list rotated by 0 - 3 envs) too.
  bookkeeping     obs_finish against a Python model: horizon 3, auto_reset on and off, both layouts, five steps, final_obs filled with a
                  sentinel before every step; one case of 4099 envs in the slot-major layout.
Run with -s for the table (recorded in profiles/obs_parity.txt)."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import ko_py as ko
from kinovagrasping_amd import scenarios
from kinovagrasping_amd.sim import SOLVER_ITERATIONS
from tests import obs_ref as orf, obs_states as ost, ray_poses as rp

pytestmark = pytest.mark.gpu
N = 275
ACTION = (0.1, 0.3, -0.2, 0.4)            # any action: the snapshot of the first substep precedes its effect
SWITCHES = ("KS_RAYS_IN_STEP", "KS_RAY_POOL", "KS_OBS_IN_STEP", "KS_ROLLOUT_WAVES", "KS_ROLLOUT_WGS", "KS_ROLLOUT_DEAL", "KS_ROLLOUT_PHASE_DEAL")
SENTINEL = -7.25
_bounds, _instep = {}, {}


def make_sim(n, model, env=(), **kw):
    """a context created under exactly the switches of `env` (they are read when the context is created)"""
    from kinovagrasping_amd.sim import KinovaSim
    with pytest.MonkeyPatch.context() as mp:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in env:
            mp.setenv(k, v)
        sim = KinovaSim(n, model, **kw)
        assert {k: os.environ[k] for k in SWITCHES if k in os.environ} == dict(env)
    return sim


def rows(sim, t):
    """an observation buffer of the context as float64 [N, 82], whatever its layout"""
    a = t.double().cpu().numpy()
    return a.copy() if sim.obs_env_major else a.T.copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def batches(n_states, n_env):
    """index arrays [n_env]: the states in order, the last batch wrapped round to the first states"""
    return [(start + np.arange(n_env)) % n_states for start in range(0, n_states, n_env)]


def bound_of(cls, shape):
    if (cls, shape) not in _bounds:
        s = ost.states(cls, shape)
        _bounds[cls, shape] = orf.bound(s.M, s.snap, s.rays)
    return _bounds[cls, shape]


# ---- the snapshot path ---------------------------------------------------------------------------------------------------------------
def from_snapshot(sim, snap, rays):
    """(obs [n, 82], reward, done, info [n, 3], the raw observation buffers per batch) of ks_obs_from_snapshot on snapshots [105, n]"""
    n = snap.shape[1]
    obs, rew, done, info, raw = np.zeros((n, 82)), np.zeros(n), np.zeros(n, dtype=int), np.zeros((n, 3)), []
    for idx in batches(n, sim.n_envs):
        o, r, d, f = sim.obs_from_snapshot(torch.as_tensor(snap[:, idx].copy()), torch.as_tensor(rays[:, idx].copy()))
        torch.cuda.synchronize()
        raw.append(o.cpu().numpy().copy())
        obs[idx], rew[idx], done[idx], info[idx] = rows(sim, o), r.double().cpu().numpy(), d.cpu().numpy(), f.double().cpu().numpy().T
    return obs, rew, done, info, raw


@pytest.mark.parametrize("precision", (64, 32))
@pytest.mark.parametrize("shape", ("CubeS", "Cone1S", "Vase1S", "BottleS"))
def test_every_class_through_the_snapshot_kernel_in_both_layouts(shape, precision):
    sets = [cs for cs in ost.all_sets() if cs[1] == shape]
    sims = {major: make_sim(N, shape, precision=precision, obs_env_major=major) for major in (True, False)}
    assert sims[True].multi_geom == (shape == ost.MG_SHAPE)
    failures = []
    for cls, _ in sets:
        s, bd = ost.states(cls, shape), bound_of(cls, shape)
        out = {major: from_snapshot(sims[major], s.snap, s.rays) for major in (True, False)}
        for a, b in zip(out[True][4], out[False][4]):
            assert a.shape == (N, 82) and b.shape == (82, N)
            if not np.array_equal(bits(a), bits(b.T)):
                failures.append((cls, "the slot-major observation is not the transpose of the env-major one", np.argwhere(bits(a) != bits(b.T))[:5].tolist()))
        for major in (True, False):
            obs, rew, done, info, _ = out[major]
            t = orf.Tally(cls, shape, f"k_obs mode 2 fp{precision} {'env' if major else 'slot'}-major", precision, s.M, s.snap, s.rays, bd)
            t.add_all(obs, rew, done, info)
            failures += t.failures + orf.exact_failures(s, obs, precision)
            if (done & ~1).any():
                failures.append((cls, "done bits beyond bit 0 on the snapshot path"))
            if major:
                print(t.line())
    for sim in sims.values():
        sim.close()
    assert not failures, (len(failures), failures[:6])


def test_a_mixed_object_context_follows_each_envs_own_model():
    """three shapes in one context (ks_reset_objects): slots 33-35 and 73-74 come from the env's own model, both precisions"""
    shapes = ["CubeS", "Cone1S", "Vase1S"]
    s = ost.states("ranges", "CubeS")
    idx = np.arange(N) % s.snap.shape[1]
    oid = np.arange(N) % 3
    Ms = [ost.model(shapes[k]) for k in oid]
    snap, rays = s.snap[:, idx], s.rays[:, idx]
    bd = orf.bound(Ms, snap, rays)
    assert len({tuple(m["obj_size_obs"]) for m in Ms}) == 3
    q0, hq = scenarios.config2_states(N)
    for precision in (64, 32):
        sim = make_sim(N, shapes, precision=precision)
        sim.reset(torch.as_tensor(q0), torch.as_tensor(hq), object_id=torch.as_tensor(oid, dtype=torch.int32))
        obs, rew, done, info, _ = from_snapshot(sim, snap, rays)
        t = orf.Tally("ranges", "mixed", f"k_obs mode 2 fp{precision} three shapes", precision, Ms, snap, rays, bd)
        t.add_all(obs, rew, done, info)
        print(t.line())
        size = np.array([m["obj_size_obs"] for m in Ms], dtype=np.float64)
        np.testing.assert_array_equal(obs[:, 33:36], orf.f32(size) if precision == 32 else size)
        t.check()
        sim.close()


# ---- the in-step paths ---------------------------------------------------------------------------------------------------------------
Path = namedtuple("Path", "name kind precision n env shape")
STEP32 = Path("ks_step wg_obs<false>", "lock", 32, N, (), "CubeS")
KOBS32 = Path("ks_step k_obs mode 0", "lock", 32, N, (("KS_OBS_IN_STEP", "0"),), "CubeS")
STEP64 = Path("ks_step fp64", "lock", 64, N, (), "CubeS")
WAVES = Path("ks_rollout waves wg_obs<true>", "rollout", 32, N, (), "CubeS")
WGS = Path("ks_rollout workgroups", "rollout", 32, N, (("KS_ROLLOUT_WAVES", "0"),), "CubeS")
ROLL64 = Path("k_rollout_f64", "rollout", 64, N, (), "CubeS")
CUBE_PATHS = (STEP32, KOBS32, STEP64, WAVES, WGS, ROLL64)
QUEUE = Path("ks_rollout queue", "rollout", 32, 4096, (), "Vase1S")            # 15 envs per workgroup: 274 groups, the ready queue
VASE_STEP32 = STEP32._replace(shape="Vase1S")
CONE_PATHS = tuple(p._replace(shape="Cone1S") for p in (STEP32, STEP64, WAVES))
MG_PATHS = tuple(p._replace(shape="BottleS") for p in (STEP32, KOBS32, STEP64, WAVES))   # (the multi-geom library's ks_rollout is fp32 only)
PLANS = {WAVES.name: "waves", WGS.name: "workgroups", ROLL64.name: "workgroups", QUEUE.name: "queue"}
IN_STEP = [(p, c) for p in CUBE_PATHS for c in ost.QPOS_CLASSES] + [(p, "lift_band") for p in (QUEUE, VASE_STEP32) + CONE_PATHS] + \
          [(p, c) for p in MG_PATHS for c in ("lift_band", "object_bearing")]
step_id = lambda v: f"{v.name} fp{v.precision} n{v.n} {v.shape}".replace(" ", "_") if isinstance(v, Path) else str(v)
_sims, _runs = {}, {}


@pytest.fixture(scope="module", autouse=True)
def contexts():
    yield
    for sim, *_ in _sims.values():
        sim.close()
    _sims.clear()


def path_sim(path):
    if path not in _sims:
        rollout = path.kind == "rollout"
        sim = make_sim(path.n, path.shape, path.env, precision=path.precision, frame_skip=1, horizon=30 if rollout else 0, auto_reset=rollout)
        _sims[path] = [sim, None]
    return _sims[path]


def one_env_step(path, qpos, hq):
    """(observation after the one env-step [n, 82] - a finished env's terminal one from final_obs -, reward, done, info or None, ks_reset's
    observation) of the states qpos [16, n], hq [4, n] placed in env order"""
    entry = path_sim(path)
    sim = entry[0]
    obs0 = sim.reset(torch.as_tensor(qpos.copy()), torch.as_tensor(hq.copy()))
    torch.cuda.synchronize()
    first = rows(sim, obs0)
    if path.kind == "lock":
        obs, rew, done, info = sim.step(torch.as_tensor(np.repeat(np.array(ACTION)[:, None], path.n, 1)))
        torch.cuda.synchronize()
        return rows(sim, obs), rew.double().cpu().numpy(), done.cpu().numpy().astype(int), info.double().cpu().numpy().T, first
    from tests.test_gpu_rays import rollout_engine
    if entry[1] is None:
        entry[1] = rollout_engine(sim, obs0)
        plan = sim.rollout_plan()
        assert plan[0] == PLANS[path.name] == entry[1][0].rollout_plan, (path.name, plan)
    tr, eng, replay = entry[1]
    eng.start(obs0)
    sim.rollout(1, tr.args)
    replay.commit_published()
    torch.cuda.synchronize()
    done = sim.done.bool()
    obs = torch.where(done[:, None], sim.final_obs, sim.obs)
    return rows(sim, obs), sim.reward.double().cpu().numpy(), sim.done.cpu().numpy().astype(int), None, first


def run(path, cls, shift=0):
    """the class's states through the path, each state i in env (i + shift) of its batch: per state (obs, reward, done, info)"""
    key = (path, cls, shift)
    if key not in _runs:
        s = ost.states(cls, path.shape)
        n = s.qpos.shape[1]
        obs, rew, done, info = np.zeros((n, 82)), np.zeros(n), np.zeros(n, dtype=int), np.zeros((n, 3))
        for idx in batches(n, path.n):
            idx = np.roll(idx, shift)
            o, r, d, f, _ = one_env_step(path, s.qpos[:, idx], s.hq[:, idx])
            obs[idx], rew[idx], done[idx] = o, r, d
            info[idx] = np.stack([0 * r, 0 * r, r], 1) if f is None else f
        status = path_sim(path)[0].get_state()["status"].cpu().numpy()
        assert (status & 4 == 0).all(), (path.name, cls, "ray-pool wait ran out")
        _runs[key] = (obs, rew, done, info)
    return _runs[key]


def instep_reference(cls, shape):
    """(exact snapshots [105, n], oracle rays [17, n], Bound with the kinematic term, at the oracle's rays)"""
    if (cls, shape) not in _instep:
        s = ost.states(cls, shape)
        snap, rays = ost.exact_snapshots(cls, shape), ost.oracle_rays(cls, shape)
        _instep[cls, shape] = (snap, rays, orf.bound(s.M, snap, rays, kinematics=True))
    return _instep[cls, shape]


@pytest.mark.parametrize("path,cls", IN_STEP, ids=step_id)
def test_one_env_step_of_every_path_meets_the_bound(path, cls):
    s = ost.states(cls, path.shape)
    snap, orays, bd = instep_reference(cls, path.shape)
    obs, rew, done, info = run(path, cls)
    n = obs.shape[0]
    # the rays: tests/ray_poses.py's tolerance against the oracle's, a hit / miss flip counting as beyond
    got = rp.from_obs(obs[:, 50:67]).T
    flip = (got < 0) != (orays < 0)
    err = np.where(flip, np.inf, np.abs(got - orays))
    beyond = err > (rp.FP64_TOL if path.precision == 64 else rp.FP32_TOL * (1 + np.abs(orays)))
    assert beyond.sum() <= rp.allowed_beyond(path.precision, beyond.size), (path.name, cls, int(beyond.sum()), np.argwhere(beyond)[:5].tolist())
    # everything else: the reference at the path's own rays; slots 70-72 where the oracle's palm rays are decidably on one side of 0.06
    # and the path's rays are on that side
    tol = rp.FP32_TOL * 1.06
    decidable = ((orays[:5] < 0) | (np.abs(orays[:5] - 0.06) > tol)).all(0)
    X = orf.pack(s.M, snap, got)
    y, z, dec, _ = orf.evaluate(X, s.M["site_body"])
    same = (dec.member == bd.dec.member).all(0)
    assert same[decidable & ~beyond[:5].any(0)].all(), (path.name, cls, "palm rays on the other side of 0.06 than the oracle's")
    skip = np.zeros((n, 82), dtype=bool)
    skip[~(decidable & same)] |= np.isin(np.arange(82), orf.PALM_SLOTS)
    bdk = bd._replace(ref=y.T, dec=dec, ray_ok=np.ones(n, dtype=bool))
    t = orf.Tally(cls, path.shape, f"{path.name} n={path.n}", path.precision, s.M, snap, got, bdk, extra=bd.kin[:, :82])
    t.add_all(obs, rew, done, info, skip=skip)
    print(t.line() + f"; rays beyond {int(beyond.sum())} of {beyond.size}; palm slots asserted in {int((decidable & same).sum())}")
    if path.kind == "lock" and path.env == ():
        assert (done & ~1 == 0).all()
    t.check()


BASE = {32: STEP32, 64: STEP64}
BIT_PAIRS = [(p, c) for p, c in IN_STEP if p.name not in (STEP32.name, STEP64.name) and (BASE[p.precision]._replace(shape=p.shape), c) in IN_STEP]


@pytest.mark.parametrize("path,cls", BIT_PAIRS, ids=step_id)
def test_in_step_paths_return_the_same_bits_per_state(path, cls):
    """every fp32 in-step path the bits of ks_step's four waves, k_rollout_f64 the bits of fp64 ks_step: the parts of build_obs - dealt to
    waves, to the lanes of a DPP row, or run by one lane - are the same arithmetic on the same snapshot and rays.

    k_obs mode 0 (KS_OBS_IN_STEP=0) is a second compiled copy of build_obs.  It holds only because k_obs writes a step's observation as wg_obs
    does, part by part with a run-time part: with part = -1 known at compile time the compiler contracted the multiply-adds of the wrist
    frame differently, and 900 - 1 850 of a class's 11 000 - 23 000 values came out an ulp apart (at most 3.5e-6, on slot 81) - this test
    found that, and fails again if the two copies drift apart."""
    a, b = run(path, cls), run(BASE[path.precision]._replace(shape=path.shape), cls)
    failures = []
    for k, name in enumerate(("obs", "reward", "done", "info")):
        if not np.array_equal(bits(a[k]), bits(b[k])):
            where = np.argwhere(bits(a[k]) != bits(b[k]))
            d = np.abs(a[k] - b[k])
            per_slot = {int(j): float(d[:, j].max()) for j in sorted(set(where[:, 1].tolist()))} if d.ndim == 2 else {}
            print(f"  DIFFERS {path.shape} {path.name} against {BASE[path.precision].name} {cls} {name}: {len(where)} of {a[k].size} values; largest per slot "
                  + " ".join(f"{j}:{v:.2e}" for j, v in per_slot.items()))
            failures.append((name, len(where), float(d.max())))
    assert not failures, (path.name, cls, failures)


@pytest.mark.parametrize("cls", ost.QPOS_CLASSES)
def test_four_placements_return_the_same_bits_per_state(cls):
    """the list rotated by 0 - 3 envs: every state in every team slot of a wave, the last workgroup partly filled"""
    base = run(STEP32, cls)
    for shift in (1, 2, 3):
        got = run(STEP32, cls, shift)
        for k, name in enumerate(("obs", "reward", "done", "info")):
            assert np.array_equal(bits(got[k]), bits(base[k])), (cls, shift, name, np.argwhere(got[k] != base[k])[:5].tolist())


# ---- the bookkeeping of obs_finish -----------------------------------------------------------------------------------------------------
HORIZON, STEPS = 3, 5
RISE = 0.5                                   # m/s upwards: 4.0 and 3.0 mm in the first two substeps (dt 0.01, semi-implicit Euler)
AWAY = (0.4, -0.4)                           # where the rising objects fly, clear of the hand in every pose


def bookkeeping_states(n):
    """qpos [16, n], qvel [15, n], hq [4, n]: lift_band states at rest, resting starts, and objects that rise into the band between the
    first and second and between the second and third step"""
    lb = ost.states("lift_band", "CubeS")
    q0, hq0 = scenarios.config2_states(n)
    qpos, qvel, hq = np.zeros((16, n)), np.zeros((15, n)), np.zeros((4, n))
    kind = np.arange(n) % 4
    for i in range(n):
        if kind[i] == 0:
            j = (i // 4 * 7) % lb.qpos.shape[1]
            qpos[:, i], hq[:, i] = lb.qpos[:, j], lb.hq[:, j]
        else:
            qpos[:, i], hq[:, i] = q0[:, i], orf.f32(hq0[:, i])
            if kind[i] >= 2:
                qpos[9:12, i] = [AWAY[0], AWAY[1], 0.195 - (2e-3 if kind[i] == 2 else 5.5e-3)]
                qvel[11, i] = RISE
    return orf.f32(qpos), orf.f32(qvel), hq, kind


_book = {}


def oracle_lift(n):
    """per env: the oracle's (lifted, margin decidable) at steps 1 .. STEPS from the start state, and from the reset pose at rest"""
    if n not in _book:
        qpos, qvel, hq, kind = bookkeeping_states(min(n, N))
        from tests import contact_poses as cp
        model, kin = ko.OracleModel(scenarios.model_blob("CubeS")), cp._oracle("CubeS")
        out = np.zeros((2, qpos.shape[1], STEPS, 2), dtype=bool)
        for i in range(qpos.shape[1]):
            for k, v in enumerate((qvel[:, i], np.zeros(15))):
                o = ko.OracleSim(model, hq[:, i], solver_iterations=SOLVER_ITERATIONS)
                o.s.rays_enabled = 0
                o.set_state(qpos[:, i], v, np.zeros(15))
                o.forward()
                for t in range(STEPS):
                    z = kin.geom_pose(hq[:, i], o.view("qpos").copy(), 8)[1][2]       # the snapshot of step t + 1: the kinematics at its start
                    out[k, i, t] = (abs(z - 0.2) < 0.005 or z >= 0.2, abs(z - 0.195) > 1e-4)
                    o.env_step(np.array(ACTION), frame_skip=1)
        _book[n] = (qpos, qvel, hq, kind, out)
    return _book[n]


def model_steps(lift, auto_reset):
    """the Python model of obs_finish for one env: per step (done, reward, restart, decidable); lift [2, STEPS, 2] from oracle_lift"""
    out, sc, traj, t0 = [], 0, 0, 0
    for t in range(STEPS):
        lifted, sure = lift[traj, t - t0]
        sc += 1
        d = (1 if lifted else 0) | (2 if HORIZON > 0 and sc >= HORIZON else 0)
        restart = bool(d) and auto_reset
        out.append((d, 50.0 if lifted else 0.0, restart, bool(sure)))
        if restart:
            sc, traj, t0 = 0, 1, t + 1
    return out


def run_bookkeeping(n, auto_reset, env_major, at_rest=False):
    """five steps of a context; per step (obs, final_obs [n, 82], reward, done, info [n, 3], state dict), and ks_reset's observation and state.
    at_rest: every env starts from its reset pose at rest - what an env restarts into"""
    qpos, qvel, hq, kind, _ = oracle_lift(n)
    idx = np.arange(n) % qpos.shape[1]
    sim = make_sim(n, "CubeS", precision=32, frame_skip=1, horizon=HORIZON, auto_reset=auto_reset, obs_env_major=env_major)
    state = lambda: {k: v.cpu().numpy().copy() for k, v in sim.get_state().items() if k in ("qpos", "qvel", "qacc_warmstart")}
    first = rows(sim, sim.reset(torch.as_tensor(qpos[:, idx].copy()), torch.as_tensor(hq[:, idx].copy())))
    torch.cuda.synchronize()
    fresh = state()
    if not at_rest:
        sim.set_state(qvel=torch.as_tensor(qvel[:, idx].copy()))
    steps = []
    for t in range(STEPS):
        sim.final_obs.fill_(SENTINEL)
        obs, rew, done, info = sim.step(torch.as_tensor(np.repeat(np.array(ACTION)[:, None], n, 1)))
        torch.cuda.synchronize()
        assert tuple(sim.final_obs.shape) == ((n, 82) if env_major else (82, n))
        steps.append((rows(sim, obs), rows(sim, sim.final_obs), rew.double().cpu().numpy(), done.cpu().numpy().astype(int), info.double().cpu().numpy().T, state()))
    sim.close()
    return first, fresh, steps, idx


_checked, _rest = {}, {}
# what the pair memory of an env's earlier episode may leave in a later one (the state itself restarts bit for bit): the figures that
# test_step_finished_inside_the_stepping_kernel_equals_the_separate_observation_launch (tests/test_gpu_obs_contacts.py) allows two runs of the
# same source that differ in such last bits - 1e-6 absolute and relative, 5e-5 on slots 73-81
LATER_TOL = np.where(np.arange(82) >= 73, 5e-5, 1e-6)


def rest_twin(env_major):
    """per step the obs of a context without auto_reset whose envs all start from their reset pose at rest"""
    if env_major not in _rest:
        _rest[env_major] = [st[0] for st in run_bookkeeping(N, False, env_major, at_rest=True)[2]]
    return _rest[env_major]


def check_bookkeeping(n, auto_reset, env_major, twin=None):
    for with_twin in ((True,) if twin is not None else (True, False)):          # (a run checked without its twin does not stand for one with it)
        if (n, auto_reset, env_major, with_twin) in _checked:
            return _checked[n, auto_reset, env_major, with_twin]
    qpos, qvel, hq, kind, lift = oracle_lift(n)
    first, fresh, steps, idx = run_bookkeeping(n, auto_reset, env_major)
    models = [model_steps(lift[:, j], auto_reset) for j in range(qpos.shape[1])]
    later, later_same = [0, 0], [0, 0]
    seen, failures, finished_before, restarted_at = set(), [], np.zeros(n, dtype=bool), np.full(n, -1)
    for t, (obs, fin, rew, done, info, st) in enumerate(steps):
        want = [models[j][t] for j in idx]
        sure = np.array([all(m[3] for m in models[j][:t + 1]) for j in idx])
        d, r, restart = np.array([w[0] for w in want]), np.array([w[1] for w in want]), np.array([w[2] for w in want])
        seen |= set(done[sure].tolist())
        if not (np.array_equal(done[sure], d[sure]) and np.array_equal(rew[sure], r[sure])):
            failures.append((t, "done / reward", np.flatnonzero(sure & ((done != d) | (rew != r)))[:5].tolist()))
        if not (np.isin(rew, (0.0, 50.0)).all() and np.array_equal(info, np.stack([0 * rew, 0 * rew, rew], 1))):
            failures.append((t, "info rows are not (0, 0, reward)"))
        untouched = (bits(fin.astype(np.float32)) == bits(np.full_like(fin, SENTINEL, dtype=np.float32))).all(1)
        if auto_reset:
            ended = done != 0
            if not np.array_equal(untouched, ~ended):
                failures.append((t, "final_obs rows: written for an unfinished env, or left for a finished one", np.flatnonzero(untouched == ended)[:5].tolist()))
            if not np.array_equal(bits(obs[ended].astype(np.float32)), bits(first[ended].astype(np.float32))):
                failures.append((t, "obs of a restarted env is not ks_reset's"))
            for k in fresh:
                if not np.array_equal(bits(st[k][:, ended]), bits(fresh[k][:, ended])):
                    failures.append((t, "state of a restarted env is not a fresh reset's", k))
            if twin is not None:
                # until its first finish an env of this context is in the state of its twin without auto_reset: its terminal observation
                # (final_obs here) is the twin's obs of that step bit for bit
                rowsel = ended & ~finished_before
                if not np.array_equal(bits(fin[rowsel].astype(np.float32)), bits(twin[t][0][rowsel].astype(np.float32))):
                    failures.append((t, "final_obs is not the terminal observation", np.flatnonzero(rowsel)[:5].tolist()))
                # a later finish: the env restarted into its reset pose at rest `since` steps ago, so its terminal observation is what a
                # context started there holds after `since` steps - bit for bit one step on (with frame_skip = 1 that observation is the
                # reset pose's, untouched by the step), within LATER_TOL further on
                rest = rest_twin(env_major)
                for i in np.flatnonzero(ended & finished_before):
                    since = t - restarted_at[i]
                    want = rest[since - 1][i]
                    same = np.array_equal(bits(fin[i].astype(np.float32)), bits(want.astype(np.float32)))
                    if not same and (since == 1 or (np.abs(fin[i] - want) > LATER_TOL * (1 + np.abs(want))).any()):
                        failures.append((t, "final_obs of a later finish is not the terminal observation", int(i), int(since)))
                    later[min(since, 2) - 1] += 1
                    later_same[min(since, 2) - 1] += int(same)
            finished_before |= ended
            restarted_at[ended] = t
        elif not untouched.all():
            failures.append((t, "final_obs written without auto_reset"))
    if auto_reset and twin is not None:
        print(f"bookkeeping {'env' if env_major else 'slot'}-major: later finishes one step after the restart {later[0]} (bit-equal to the context started at rest: {later_same[0]}), "
              f"further on {later[1]} (bit-equal {later_same[1]})")
        assert later[0] >= 30 and later[1] >= 30, later
    if auto_reset:
        # the time limit comes again three steps later: an env that restarted at step t and is not lifted at rest is done = 2 at t + 3
        again = [j for j in range(qpos.shape[1]) if any(models[j][t][2] and t + HORIZON < STEPS and models[j][t + HORIZON][0] == 2 for t in range(STEPS))]
        assert len(again) >= 30, len(again)
    assert {0, 1, 2, 3} <= seen, seen
    assert not failures, (n, auto_reset, env_major, failures[:6])
    _checked[n, auto_reset, env_major, twin is not None] = steps
    return steps


@pytest.mark.parametrize("env_major", (True, False), ids=("env-major", "slot-major"))
def test_episode_bookkeeping_follows_the_model_of_obs_finish(env_major):
    """without auto_reset obs holds the terminal observation and final_obs stays untouched; with it final_obs holds that observation (the
    twin context's obs, bit for bit) and obs, state and counter are a fresh reset's"""
    twin = check_bookkeeping(N, False, env_major)
    # the twin's own observation is held to the reference through the in-step tests: its envs that hold a lift_band state return, in the
    # first step, the bits that ks_step returns for that state there (test_one_env_step_of_every_path_meets_the_bound asserts the bound on them)
    held = run(STEP32, "lift_band")[0]
    n_lb = ost.states("lift_band", "CubeS").qpos.shape[1]
    for i in range(0, N, 4):
        assert np.array_equal(bits(twin[0][0][i]), bits(held[(i // 4 * 7) % n_lb])), ("the twin's first observation is not ks_step's of that state", i)
    check_bookkeeping(N, True, env_major, twin)


@pytest.mark.parametrize("auto_reset", (False, True))
def test_the_two_layouts_return_the_same_bits_over_an_episode(auto_reset):
    for a, b in zip(check_bookkeeping(N, auto_reset, True), check_bookkeeping(N, auto_reset, False)):
        for k in range(5):
            assert np.array_equal(bits(a[k]), bits(b[k])), ("the two layouts differ", k)


def test_episode_bookkeeping_at_4099_envs_in_the_slot_major_layout():
    """the stride is 4099: no multiple of a wave, a team or a cache line; env i holds state i mod 275 and returns that state's bits"""
    steps = check_bookkeeping(4099, True, False)
    small = check_bookkeeping(N, True, False)
    idx = np.arange(4099) % N
    for a, b in zip(steps, small):
        for k in range(5):
            assert np.array_equal(bits(a[k]), bits(b[k][idx])), ("4099 envs differ from 275", k)
