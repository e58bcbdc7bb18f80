"""What the host side of libkinova_sim.so refuses (csrc/ks_api.hip: Ctx<T>): for every call below the return code and the exact
ks_last_error text, and that a context which has refused is as usable as before.  Every case differs from a valid call in one argument
or in one property of its context, and is turned down by a check on the host: no kernel sees a bad argument.  (One refusal comes late:
hidden widths 48-48 pass every check of the arguments and are turned down where the kernel is chosen, behind the copy of the launch's
records and the slot sort - both of them launches with valid arguments, repeated by the next valid call.)"""
import ctypes as C

import pytest
import torch

from kinovagrasping_amd import scenarios

pytestmark = pytest.mark.gpu

N = 16
OK, INVALID, STATE = 0, -1, -5          # KS_OK, KS_ERR_INVALID, KS_ERR_STATE (include/kinova_sim.h)
NULL_ARGUMENT = "ks_rollout: NULL argument"
NEEDS_WAVES = "ks_rollout: a time budget needs the wave form of the rollout kernel (ks_rollout_plan: KS_PLAN_WAVES)"
POOL_ARGUMENTS = "ks_set_start_pool: 1 <= k <= 1024 starts per env (0 clears the pool), qpos0 and hand_quat required"


class Contexts:
    """fp32 with auto_reset (and the engine, policy and replay of a valid ks_rollout record), fp32 without auto_reset, fp64 with
    auto_reset, and fp32 with auto_reset created under KS_ROLLOUT_WAVES=0 (the switch is read when a context is created)"""

    def __init__(self, monkeypatch):
        from kinovagrasping_amd.ddpgfd import DDPGfD
        from kinovagrasping_amd.pipeline import rollout_args
        from kinovagrasping_amd.replay import DeviceEpisodeReplay
        from kinovagrasping_amd.rollout import RolloutEngine
        from kinovagrasping_amd.sim import KinovaSim
        q0, hq = (torch.as_tensor(x) for x in scenarios.config2_states(N))
        self.q0, self.hq = q0, hq
        self.f32 = KinovaSim(N, "CubeS", horizon=30, auto_reset=True)
        self.plain = KinovaSim(N, "CubeS", horizon=30, auto_reset=False)
        self.f64 = KinovaSim(N, "CubeS", horizon=30, auto_reset=True, precision=64)
        monkeypatch.setenv("KS_ROLLOUT_WAVES", "0")
        self.joined = KinovaSim(N, "CubeS", horizon=30, auto_reset=True)
        monkeypatch.delenv("KS_ROLLOUT_WAVES")
        for sim in (self.plain, self.f64, self.joined):
            sim.reset(q0, hq)
        sim = self.f32
        obs0 = sim.reset(q0, hq)
        torch.manual_seed(2)
        self.policy = DDPGfD(82, 4, 0.8, 5, batch_size=64, hidden=(256, 256), device=sim.device)
        self.replay = DeviceEpisodeReplay(N, capacity=8 * N, horizon=30, device=sim.device)
        self.eng = RolloutEngine(sim, self.policy, self.replay, expl_noise=0.1)
        self.eng.start(obs0)
        self.replay.enable_async()
        flat = self.policy._flat_params["actor"]
        self.pub = torch.zeros(3, (flat.numel() + 3) // 4 * 4, device=sim.device)
        self.pub[0, :flat.numel()].copy_(flat)
        self.pub_ver = torch.zeros(1, dtype=torch.long, device=sim.device)
        self.steps_total = torch.zeros(N, dtype=torch.long, device=sim.device)
        self.counters = torch.zeros(8 + 4 * 512 + 8 + N, dtype=torch.long, device=sim.device)
        self.args = rollout_args(sim, self.policy, self.eng, self.pub, self.pub_ver, self.steps_total, self.counters, replay=self.replay)
        self.q0d, self.hqd = q0.to(sim.device, torch.float32).contiguous(), hq.to(sim.device, torch.float32).contiguous()
        self.action = torch.full((4, N), 0.3, device=sim.device)
        self.ranges = torch.ones(4, N, device=sim.device)
        assert sim.rollout_plan()[0] == "waves" and self.joined.rollout_plan()[0] == "workgroups"
        torch.cuda.synchronize()

    def close(self):
        torch.cuda.synchronize()
        for sim in (self.f32, self.plain, self.f64, self.joined):
            sim.close()


@pytest.fixture(scope="module")
def ctxs():
    mp = pytest.MonkeyPatch()
    c = Contexts(mp)
    yield c
    c.close()
    mp.undo()


def _rollout(which, n_iter=1, **changed):
    """ks_rollout of the valid record with the given fields changed, on context `which`"""
    def call(c):
        sim = getattr(c, which)
        a = type(c.args).from_buffer_copy(c.args)
        for k, v in changed.items():
            setattr(a, k, v)
        return sim, sim.lib.ks_rollout(sim.ctx, n_iter, C.byref(a), sim._stream())
    return call


def _call(which, fn, *args):
    """fn(ctx, *args, stream) on context `which`; an argument that is a string names a tensor of the fixture"""
    def call(c):
        sim = getattr(c, which)
        ptr = lambda a: C.c_void_p(getattr(c, a).data_ptr()) if isinstance(a, str) else a
        return sim, getattr(sim.lib, fn)(sim.ctx, *[ptr(a) for a in args], sim._stream())
    return call


def _load_again(c):
    blob = bytes(scenarios.model_blob("CubeS"))
    return c.f32, c.f32.lib.ks_load_model(c.f32.ctx, blob, len(blob))


CASES = {
    "rollout n_iter = 0": (_rollout("f32", n_iter=0), INVALID, NULL_ARGUMENT),
    "rollout obs NULL": (_rollout("f32", obs=None), INVALID, NULL_ARGUMENT),
    "rollout replay horizon <= n_steps": (_rollout("f32", horizon=5, n_steps=5), INVALID, "ks_rollout: replay buffers"),
    "rollout h1 = 258": (_rollout("f32", h1=258), INVALID, "ks_rollout: hidden widths must be multiples of 4"),
    "rollout off_w2 = 2": (_rollout("f32", off_w2=2), INVALID, "ks_rollout: weight offsets must be multiples of 4 floats"),
    "rollout hidden 48-48": (_rollout("f32", h1=48, h2=48), INVALID, "ks_rollout: hidden widths must be 256-256, 400-300, 128-128 or 64-64"),
    "rollout budget_ticks = -1": (_rollout("f32", budget_ticks=-1), STATE, NEEDS_WAVES),
    "rollout budget without free waves": (_rollout("joined", budget_ticks=100000), STATE, NEEDS_WAVES),
    "rollout budget on fp64": (_rollout("f64", budget_ticks=100000), STATE, NEEDS_WAVES + "; fp64 contexts have none"),
    "rollout without auto_reset": (_rollout("plain"), STATE, "ks_rollout needs the in-kernel observation path, env-major observations and auto_reset"),
    "start pool k = 1025": (_call("f32", "ks_set_start_pool", 1025, "q0d", "hqd", 0, None), INVALID, POOL_ARGUMENTS),
    "start pool qpos0 NULL": (_call("f32", "ks_set_start_pool", 1, None, "hqd", 0, None), INVALID, POOL_ARGUMENTS),
    "start index without a pool": (_call("f32", "ks_get_start_index", None, None), STATE, "ks_get_start_index: the context holds no start pool (ks_set_start_pool)"),
    "episode log capacity = n_envs - 1": (_call("f32", "ks_set_episode_log", N - 1), INVALID,
                                          "ks_set_episode_log: n_envs <= capacity <= 16777216 records (0 clears the log)"),
    "episode log without auto_reset": (_call("plain", "ks_set_episode_log", 64), STATE,
                                       "ks_set_episode_log: the log is written where an episode restarts inside the stepping kernels - the context needs auto_reset"),
    "episode log read without a log": (_call("f32", "ks_get_episode_log", None, None), STATE, "ks_get_episode_log: the context holds no episode log (ks_set_episode_log)"),
    "param ranges without auto_reset": (_call("plain", "ks_set_param_ranges", "ranges", 0), STATE,
                                        "ks_set_param_ranges: the parameters are drawn where an episode restarts inside the stepping kernels - the context needs auto_reset"),
    "controller mode 7": (_call("f32", "ks_set_rollout_controller", 7, 0), INVALID,
                          "ks_set_rollout_controller: mode 0 (none), 1 (naive), 2 (position-dependent) or 3 (combined); lift rule 0 (train) or 1 (expert)"),
    "reset n = 0": (_call("f32", "ks_reset", None, 0, "q0d", "hqd", None), INVALID, "ks_reset: bad arguments"),
    "step action NULL": (_call("f32", "ks_step", None, None, None, None, None, None), INVALID, "ks_step: action is NULL"),
    "obs_from_snapshot snap NULL": (_call("f32", "ks_obs_from_snapshot", None, "ranges", "ranges", None, None, None), INVALID,
                                    "ks_obs_from_snapshot: snapshot, rays and obs are required"),
    "second ks_load_model": (_load_again, STATE, "ks_load_model: a context loads its model(s) once"),
}


def _refused(c, name):
    call, code, text = CASES[name]
    sim, rc = call(c)
    assert (rc, sim.lib.ks_last_error(sim.ctx).decode()) == (code, text), name


@pytest.mark.parametrize("name", list(CASES))
def test_the_host_refuses(ctxs, name):
    _refused(ctxs, name)


def test_a_context_that_has_refused_steps_and_rolls_out(ctxs):
    c = ctxs
    for name in CASES:
        _refused(c, name)
    sim = c.f32
    rc = sim.lib.ks_step(sim.ctx, C.c_void_p(c.action.data_ptr()), *(C.c_void_p(t.data_ptr()) for t in (sim.obs, sim.reward, sim.done, sim.info, sim.final_obs)),
                         sim._stream())
    assert rc == OK, sim.lib.ks_last_error(sim.ctx).decode()
    rc = sim.lib.ks_rollout(sim.ctx, 1, C.byref(c.args), sim._stream())
    assert rc == OK, sim.lib.ks_last_error(sim.ctx).decode()
    torch.cuda.synchronize()
    assert torch.equal(c.steps_total, torch.ones_like(c.steps_total)) and torch.isfinite(sim.obs).all()
    assert (sim.get_state()["status"] & 2).sum().item() == 0
