"""The free-running waves' actor forward on 4-row MFMA blocks (csrc/ks_mlp_tile.h: mlp3_rows_wave on v_mfma_f32_4x4x1_16B_f32) equals the
lock-step calls bit for bit: 21 CubeS envs (one workgroup whose waves hold 4 and 1 envs), frame_skip 1, ONE ks_rollout launch of 2 env-steps
in the free-wave form against kr_actor_select -> ks_step -> kr_store_transition per env - action, next observation and the stored rows of
both env-steps.  What that rests on is that the 16x16x4 fp32 MFMA of the reference is, per output, the k-ordered fma chain of its four k.

Widths: 256-256, 392-292 (partial groups, the 400-300 instantiation), 128-128, 120-116, 64-64, 60-52 - those of
tests/test_gpu_actor_weight_stream.py.  In every case the published parameters lie between NaN words (every matrix and bias on its own,
at least 4 on either side) and everything that comes out must be finite: a guard word that reached an MFMA would show as NaN.

* dense random: weights N(0, 1/sqrt(fan_in)), biases N(0, 0.1), fixed seeds; an fp64 forward of the same parameters has at least a quarter
  of every hidden layer's units on either side of the ReLU, so both the sums and the zeros are exercised.  (Dyadic inputs, as the older
  exact tests use, are exact in any order; these are not.)
* layout: one-hot W1 / W2 / W3 (a single 1.0 per feature row at column (7 f + 3) mod K, zero biases), no exploration noise.  Nothing is
  ever added to a nonzero value, so every output is exactly one gathered input word.  The only output of the kernel is the action
  0.8 / (1 + exp(-z)), which cannot tell integers beyond ~15 apart, so the inputs are the distinct integers 1 + k + 82 env scaled by
  2^-9 (0 < x < 3.4: neighbours are > 40 ulp of the action apart): the logit of the first env-step's stored action, times 2^9, must
  round to the integer the three gathers name - a wrong lane, quad or env shows as another integer - and the bits must be the lock-step
  call's.

The file's name sorts behind test_gpu_actor_versions.py on purpose: the first case of that file counts forwards that overlap a burst of
publications and finds none - with the 16-column form as well, measured - when a test that builds a trainer (this file, or
test_gpu_actor_weight_stream.py) has run before it in the same process."""
import math

import pytest
import torch

from kinovagrasping_amd import scenarios

pytestmark = pytest.mark.gpu

N, H, STEPS = 21, 6, 2
WIDTHS = [(256, 256), (392, 292), (128, 128), (120, 116), (64, 64), (60, 52)]


def dense_layers(hw, seed=None):
    g = torch.Generator().manual_seed(hw[0] * 1000 + hw[1] if seed is None else seed)
    dims = [(hw[0], 82), (hw[1], hw[0]), (4, hw[1])]
    return [(torch.randn(o, i, generator=g) / i ** 0.5, 0.1 * torch.randn(o, generator=g)) for o, i in dims]


def one_hot_layers(hw):
    layers = []
    for o, i in [(hw[0], 82), (hw[1], hw[0]), (4, hw[1])]:
        w = torch.zeros(o, i)
        w[torch.arange(o), (7 * torch.arange(o) + 3) % i] = 1.0
        layers.append((w, torch.zeros(o)))
    return layers


def relu_balance(layers, obs):
    """per hidden layer, the fraction of (env, unit) pairs in front of the ReLU that are positive (fp64)"""
    x, out = obs.double(), []
    for w, b in layers[:2]:
        z = x @ w.double().T + b.double()
        out.append(float((z > 0).double().mean()))
        x = z.clamp(min=0)
    return out


def _setup(monkeypatch, hw, layers, sigma, obs):
    from kinovagrasping_amd import learner_native
    from kinovagrasping_amd.ddpgfd import DDPGfD
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from kinovagrasping_amd.rollout import RolloutEngine
    from kinovagrasping_amd.sim import KinovaSim

    class RolloutOnly(learner_native.NativeDDPGfDUpdate):       # (the trainer is built for the rollout's argument record only, as in
        def __init__(self, *a, **kw):                           # test_gpu_actor_weight_stream.py: no update ever runs)
            super().__init__(*a, **kw)
            self.lds_free = True

    monkeypatch.setattr(learner_native, "NativeDDPGfDUpdate", RolloutOnly)
    q0, hq = scenarios.config2_states(N)
    sim = KinovaSim(N, "CubeS", frame_skip=1, horizon=H, auto_reset=True)
    obs0 = sim.reset(torch.as_tensor(q0), torch.as_tensor(hq))
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=64, hidden=hw, device=sim.device)
    with torch.no_grad():
        for lin, (w, b) in zip((policy.actor.l1, policy.actor.l2, policy.actor.l3), layers):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
    replay = DeviceEpisodeReplay(N, capacity=8 * N, horizon=H, device=sim.device)
    eng = RolloutEngine(sim, policy, replay, expl_noise=sigma)
    eng.start(obs0)
    if obs is not None:
        eng.obs.copy_(obs)
    return sim, policy, replay, eng, obs0


def _guarded_block(layers, dev):
    """W1, b1, W2, b2, W3, b3 in ONE buffer of NaN, each at a multiple of 4 floats with at least 4 NaN words on either side: the published
    block [3, stride] (buffers 1 and 2 are NaN throughout) inside a pool with NaN in front and behind, and the offsets"""
    flat = [t for wb in layers for t in wb]
    up4 = lambda k: (k + 3) // 4 * 4
    stride = sum(up4(t.numel()) + 8 for t in flat) + 8
    pool = torch.full((3 * stride + 16,), float("nan"), device=dev)
    assert pool.data_ptr() % 16 == 0
    pub = pool[8:8 + 3 * stride].view(3, stride)
    offs, at = [], 8
    for t in flat:
        pub[0, at:at + t.numel()].copy_(t.reshape(-1))
        offs.append(at)
        at += up4(t.numel()) + 8
    assert int(torch.isnan(pool).sum()) == pool.numel() - sum(t.numel() for t in flat)
    return pool, pub, offs


def run_both(monkeypatch, hw, layers, sigma=0.1, obs=None):
    """the same parameters and start states through the lock-step calls and through one free-running launch: two dicts of what they leave"""
    from kinovagrasping_amd.pipeline import AsyncTrainer, rollout_args
    # lock step
    sim, policy, replay, eng, obs0 = _setup(monkeypatch, hw, layers, sigma, obs)
    for _ in range(STEPS):
        eng.step()
    torch.cuda.synchronize()
    lock = dict(action=eng.action.clone(), obs=eng.obs.clone(), state=replay.cur_state[:, :STEPS].clone(), next=replay.cur_next[:, :STEPS].clone(),
                stored_action=replay.cur_action[:, :STEPS].clone(), reward=replay.cur_reward[:, :STEPS].clone(),
                not_done=replay.cur_not_done[:, :STEPS].clone(), len=replay.cur_len.clone(), obs0=obs0.clone())
    sim.close()
    # free running: one launch
    sim, policy, replay, eng, _ = _setup(monkeypatch, hw, layers, sigma, obs)
    tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=16)
    assert sim.rollout_plan()[0] == "waves" == tr.rollout_plan
    pool, pub, offs = _guarded_block([(w.to(sim.device), b.to(sim.device)) for w, b in layers], sim.device)
    args = rollout_args(sim, policy, eng, pub, tr.pub_ver, tr.steps_total, tr.counters, replay=replay, repeats=tr.repeats)
    args.off_w1, args.off_b1, args.off_w2, args.off_b2, args.off_w3, args.off_b3 = offs
    sim.rollout(STEPS, args)
    torch.cuda.synchronize()
    assert torch.equal(tr.steps_total, torch.full_like(tr.steps_total, STEPS)) and int(tr.repeats) == 0
    assert torch.equal(replay.a_sel, torch.zeros_like(replay.a_sel))                    # nobody finished an episode: buffer 0 is the open one
    free = dict(action=eng.action.clone(), obs=eng.obs.clone(), state=replay.a_state[0, :, :STEPS].clone(), next=replay.a_next[0, :, :STEPS].clone(),
                stored_action=replay.a_action[0, :, :STEPS].clone(), reward=replay.a_reward[0, :, :STEPS].clone(),
                not_done=replay.a_not_done[0, :, :STEPS].clone(), len=replay.a_len[0].clone())
    sim.close()
    del pool
    return lock, free


def assert_bit_equal(lock, free):
    for k, v in free.items():
        assert torch.isfinite(v.float()).all(), k
        bad = (v != lock[k]).reshape(N, -1).any(1).nonzero().flatten().tolist()
        assert torch.equal(v, lock[k]), (k, "envs", bad)
    assert torch.equal(free["len"], torch.full_like(free["len"], STEPS))
    assert free["stored_action"].std() > 0


@pytest.mark.parametrize("hw", WIDTHS, ids=lambda hw: f"{hw[0]}-{hw[1]}")
def test_dense_random_actor_in_the_free_waves_equals_the_lock_step_calls(monkeypatch, hw):
    layers = dense_layers(hw)
    lock, free = run_both(monkeypatch, hw, layers)
    for frac in relu_balance(layers, lock["obs0"].cpu()) + relu_balance(layers, lock["obs"].cpu()):
        assert 0.25 <= frac <= 0.75, frac
    assert_bit_equal(lock, free)


@pytest.mark.parametrize("hw", WIDTHS, ids=lambda hw: f"{hw[0]}-{hw[1]}")
def test_one_hot_layers_gather_the_named_input_word_of_the_named_env(monkeypatch, hw):
    x_int = 1 + torch.arange(82)[None, :] + 82 * torch.arange(N)[:, None]             # distinct per (env, k)
    lock, free = run_both(monkeypatch, hw, one_hot_layers(hw), sigma=0.0, obs=x_int.float() / 512)
    col = lambda f, k: (7 * f + 3) % k
    a = free["stored_action"][:, 0].double().cpu()                                   # the first env-step acted on x
    got = torch.round(torch.log(a / (0.8 - a)) * 512).long()
    for o in range(4):
        k = col(col(col(o, hw[1]), hw[0]), 82)                                       # output o <- h2 unit <- h1 unit <- input word
        assert got[:, o].tolist() == x_int[:, k].tolist(), (o, k, got[:, o].tolist())
    assert torch.equal(free["state"][:, 0].cpu(), x_int.float() / 512)
    assert_bit_equal(lock, free)
