"""The references of tests/glue_ref.py against independent implementations of the same rules, on the host: torch.optim.Adam in
float64, float64 autograd of DDPGfD's own losses, and the torch paths (native = False) of DeviceEpisodeReplay / RolloutEngine on the
random stream of test_gpu_parity.py::test_rollout_kernels_equal_torch_bookkeeping.  tests/test_gpu_glue_kernels.py holds the kr_*
kernels to these references; this file is what the references themselves stand on."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import glue_ref as gr


def _rel(a, b):
    """the largest element-wise relative error (floor 1e-300 absolute: exact zeros compare as equal)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max()) if (a != b).any() else 0.0


@pytest.mark.parametrize("lr,wd", [(1e-4, 0.0), (1e-3, 1e-4)])
def test_adam_ref_equals_torch_adam_in_float64(lr, wd):
    """12 steps of torch.optim.Adam (float64) on one tensor, the reference fed with the same gradients and its own state"""
    g = torch.Generator().manual_seed(3)
    p = torch.randn(257, generator=g, dtype=torch.float64).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, weight_decay=wd)
    rp, rm, rv = p.detach().numpy().copy(), np.zeros(257), np.zeros(257)
    for step in range(1, 13):
        grad = torch.randn(257, generator=g, dtype=torch.float64) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=g))
        grad[::7] = 0
        p.grad = grad.clone()
        opt.step()
        rp, rm, rv = gr.adam_ref(rp, grad.numpy(), rm, rv, step, lr, 0.9, 0.999, 1e-8, wd)
        st = opt.state[p]
        assert _rel(rp, p.detach().numpy()) <= 1e-12 and _rel(rm, st["exp_avg"].numpy()) <= 1e-12 and _rel(rv, st["exp_avg_sq"].numpy()) <= 1e-12, step
    kept = gr.adam_ref(rp, rp, rm, rv, 0, lr, 0.9, 0.999, 1e-8, wd)
    assert all(np.array_equal(a, b) for a, b in zip(kept, (rp, rm, rv)))


class _Table(torch.nn.Module):
    """a network that returns its own parameter whatever it is given: its gradient is dLoss/dOutput"""

    def __init__(self, values):
        super().__init__()
        self.out = torch.nn.Parameter(values.clone())

    def forward(self, *inputs):
        return self.out


class _Second(torch.nn.Module):
    def forward(self, state, action):
        return action


class _NoStep:
    def step(self):
        pass

    def zero_grad(self):
        pass


def _policy(n):
    from kinovagrasping_amd.ddpgfd import DDPGfD
    torch.manual_seed(7)
    p = DDPGfD(82, 4, 0.8, n, hidden=(8, 8), device="cpu")
    p._disc = p._disc.double()          # (the fp64 learner check of test_gpu_mlp_fp64.py does the same)
    return p


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("weights", ["none", "masked", "all_zero"])
def test_critic_grad_and_prologue_refs_equal_float64_autograd(n, weights):
    """DDPGfD.phase_critic / phase_actor in float64 with table networks in the critic's, the targets' and the actor's place: the
    three losses, dLoss/dQ of the critic loss and dLoss/dQ of the actor loss"""
    R = 37
    g = torch.Generator().manual_seed(11 + n)
    f32 = lambda *s: torch.randn(*s, generator=g).float()
    q, tq, rw = f32(R, 1) * 3, f32(2 * R, 1) * 3, torch.rand(R, n, generator=g).float() * 5
    w = {"none": None, "masked": (torch.rand(R, generator=g) < 0.7).float(), "all_zero": torch.zeros(R)}[weights]
    p = _policy(n)
    disc = float(np.float32(p.discount))
    p.discount = disc
    p._disc = torch.tensor([disc ** i for i in range(n)], dtype=torch.float64)
    p.critic, p.critic_target, p.actor_target = _Table(q.double()), _Table(tq.double()), _Table(torch.zeros(1).double())
    p.critic_optimizer = _NoStep()
    w64 = None if w is None else w.double()
    state = torch.zeros(R, n, 82, dtype=torch.float64)
    losses = p.phase_critic(state, torch.zeros(R, n, 4, dtype=torch.float64), state, rw.double(), w64)
    wsum, dqa, it, it_head = gr.prologue_ref(R, n, None if w is None else w.numpy(), 4, 2, 1)
    assert (it, it_head) == (5, 5) and gr.prologue_ref(R, n, None, 4, 2, 0)[2:] == (5, 2)
    assert wsum == (R if w is None else max(float(w.sum()), 1.0))
    dq, ref_losses = gr.critic_grad_ref(q[:, 0].numpy(), tq[:R, 0].numpy(), tq[R:, 0].numpy(), rw.numpy(), None if w is None else w.numpy(), wsum, disc)
    for a, b in zip(ref_losses, losses):
        assert abs(a - b.item()) <= 1e-13 * max(1.0, abs(b.item())), (ref_losses, losses)
    assert np.abs(dq - p.critic.out.grad[:, 0].numpy()).max() <= 1e-13 * max(1.0, float(p.critic.out.grad.abs().max()))
    # the actor loss -mean_w Q(s, pi(s)) with Q = the actor's own table: its gradient is dLoss/dQ
    p.actor, p.critic = _Table(torch.randn(R, n, 1, generator=g, dtype=torch.float64)), _Second()
    p.actor_optimizer = _NoStep()
    p.phase_actor(state, w64)
    got = p.actor.out.grad.reshape(-1).numpy()
    assert np.abs(dqa - got).max() <= 1e-15, np.abs(dqa - got).max()
    if weights == "all_zero":
        assert wsum == 1.0 and not dq.any() and not dqa.any() and ref_losses == (0.0, 0.0, 0.0)
        assert gr.critic_grad_ref(q[:, 0].numpy(), tq[:R, 0].numpy(), tq[R:, 0].numpy(), rw.numpy(), None, 0.0, disc)[1] == (0.0, 0.0, 0.0)


def test_soft_update_ref_equals_phase_targets_across_call_10():
    """12 calls of DDPGfD.phase_targets on float64 parameters that move between the calls: the targets change on call 10 only"""
    p = _policy(5)
    g = torch.Generator().manual_seed(5)
    p.actor_optimizer = _NoStep()
    p._flat_params = {k: torch.randn(300, generator=g, dtype=torch.float64) for k in ("critic", "critic_target", "actor", "actor_target")}
    ref = {k: v.numpy().copy() for k, v in p._flat_params.items()}
    changed = []
    for call in range(1, 13):
        for k in ("critic", "actor"):
            p._flat_params[k] += 0.1 * torch.randn(300, generator=g, dtype=torch.float64)
        before = p._flat_params["critic_target"].clone()
        p.phase_targets()
        for k in ("critic", "actor"):
            ref[k + "_target"] = gr.soft_update_ref(p._flat_params[k].numpy(), ref[k + "_target"], p.tau, call, p.network_repl_freq)
            assert _rel(ref[k + "_target"], p._flat_params[k + "_target"].numpy()) <= 1e-15, (call, k)
        if not torch.equal(before, p._flat_params["critic_target"]):
            changed.append(call)
    assert changed == [10]
    tp = ref["critic_target"]
    assert np.array_equal(gr.soft_update_ref(ref["critic"], tp, p.tau, 0, 1), tp) and not np.array_equal(gr.soft_update_ref(ref["critic"], tp, p.tau, 3, 1), tp)


def test_elementwise_refs():
    a = np.array([0.0, -0.0, 1e-40, -1e-40, -1.0, 2.0], np.float32)
    g = np.array([1.0, 2.0, 3.0, 4.0, 5.0, -0.0], np.float32)
    out = gr.relu_backward_ref(a, g)
    assert out.view(np.uint32).tolist() == np.array([0, 0, 3.0, 0, 0, -0.0], np.float32).view(np.uint32).tolist()
    z = torch.linspace(-4, 4, 33, dtype=torch.float64, requires_grad=True)
    act = 0.8 * torch.sigmoid(z)
    up = torch.linspace(-1, 2, 33, dtype=torch.float64)
    act.backward(up)
    ref = gr.sigmoid_scale_backward_ref(act.detach().numpy(), 0.8, up.numpy())
    assert np.abs(ref - z.grad.numpy()).max() <= 1e-15


# ---- the ring rules against the torch paths ---------------------------------------------------------------------------
N_ENVS, HORIZON, N_STEPS, CAPACITY, T_STEPS = 193, 30, 5, 256, 75


class _FakeSim:
    def __init__(self, n, dev):
        self.n_envs, self.device = n, dev
        self.cfg = SimpleNamespace(auto_reset=1)
        self.obs, self.final_obs = torch.zeros(n, 82), torch.zeros(n, 82)
        self.reward, self.done = torch.zeros(n), torch.zeros(n, dtype=torch.uint8)


def _np(t):
    a = t.detach().cpu().numpy()
    return a.astype(np.uint8) if a.dtype == np.bool_ else a.copy()


def _ring_of(rep):
    return dict(count=rep.count, head=rep.head, capacity=rep.capacity, ep_len=_np(rep.ep_len), state=_np(rep.ep_state), next=_np(rep.ep_next),
                action=_np(rep.ep_action), reward=_np(rep.ep_reward), not_done=_np(rep.ep_not_done))


def _assert_same_batch(ref, got, what):
    for k, (a, b) in enumerate(zip(ref[:6], got)):
        assert np.array_equal(a.view(np.uint32), _np(b).view(np.uint32)), (what, k)


@pytest.fixture(scope="module")
def stream_run():
    """the random stream of test_rollout_kernels_equal_torch_bookkeeping on the CPU device: the torch engine and replay take every
    step; the references keep a replay of their own from the first step on (engine state is re-read after pre(), whose action
    selection is not under test here) and are compared after every step."""
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from kinovagrasping_amd.rollout import RolloutEngine
    dev, n, H = torch.device("cpu"), N_ENVS, HORIZON
    g = torch.Generator().manual_seed(5)
    W1 = torch.randn(82, 4, generator=g) * 0.05
    policy = SimpleNamespace(actor=lambda o: 0.8 * torch.sigmoid(o @ W1))
    sim = _FakeSim(n, dev)
    rep = DeviceEpisodeReplay(n, capacity=CAPACITY, horizon=H, device=dev)
    eng = RolloutEngine(sim, policy, rep, expl_noise=0.1, generator=torch.Generator().manual_seed(11))
    assert not rep.native and not eng.native
    eng.start(torch.randn(n, 82, generator=g) * 0.1)
    z = lambda *s: np.zeros(s, np.float32)
    cur = dict(cur_state=z(n, H, 82), cur_next=z(n, H, 82), cur_action=z(n, H, 4), cur_reward=z(n, H), cur_not_done=z(n, H),
               cur_len=np.zeros(n, np.int64), keep=np.zeros(n, np.uint8))
    ep = dict(state=z(CAPACITY, H, 82), next=z(CAPACITY, H, 82), action=z(CAPACITY, H, 4), reward=z(CAPACITY, H), not_done=z(CAPACITY, H))
    ep_len, head, count = np.zeros(CAPACITY, np.int64), 0, 0
    age = torch.zeros(n, dtype=torch.long)
    seen = dict(lift_end=0, dropped=0, early_batches=[])
    for step in range(T_STEPS):
        nobs = torch.randn(n, 82, generator=g) * 0.1
        frozen = torch.rand(n, generator=g) < 0.3
        nobs[:, 9:17] = torch.where(frozen.unsqueeze(1), eng.obs[:, 9:17], nobs[:, 9:17])
        fin = torch.randn(n, 82, generator=g)
        rew = torch.rand(n, generator=g) * 50
        age += 1
        done = (torch.rand(n, generator=g) < 0.04) | (age >= 30)
        age = torch.where(done, torch.zeros_like(age), age)
        eng.pre()
        sim.obs.copy_(nobs); sim.final_obs.copy_(fin); sim.reward.copy_(rew); sim.done.copy_(done.to(torch.uint8) * 3)
        e = {k: _np(getattr(eng, k)) for k in ("obs", "prev_obs", "has_prev", "t", "ready", "lifting", "action", "reward_out", "done_out")}
        s = dict(obs=_np(sim.obs), final_obs=_np(sim.final_obs), reward=_np(sim.reward), done=_np(sim.done))
        for i in range(n):
            seen["lift_end"] += int(s["done"][i] != 0 and e["lifting"][i] != 0)
            gr.store_transition_ref(i, H, N_STEPS, 1, s, e, cur)
        keep_torch = _np(done & (rep.cur_len + (~eng.lifting).long() * (rep.cur_len < H).long() - N_STEPS > 1))
        eng.post()
        rank, total = gr.rank_ref(cur["keep"])
        assert np.array_equal(rank, torch.cumsum(torch.as_tensor(cur["keep"]).long(), 0).numpy()) and np.array_equal(cur["keep"], keep_torch)
        seen["dropped"] += int((s["done"] != 0).sum()) - total
        gr.commit_ref(cur["keep"], rank, head, CAPACITY, {f: cur["cur_" + f] for f in gr.RING_FIELDS}, cur["cur_len"], ep, ep_len)
        head, count, cur["cur_len"] = gr.advance_ref(total, head, count, CAPACITY, e["done_out"], cur["cur_len"])
        for k in ("obs", "prev_obs", "has_prev", "t", "ready", "reward_out", "done_out"):
            assert np.array_equal(e[k], _np(getattr(eng, k))), (step, k)
        for k in ("cur_state", "cur_next", "cur_action", "cur_reward", "cur_not_done", "cur_len"):
            assert np.array_equal(cur[k], _np(getattr(rep, k))), (step, k)
        assert (head, count) == (rep.head, rep.count), step
        # (row `capacity` of the torch ring is its trash row, where episodes that are not kept go: not part of the rule)
        assert np.array_equal(ep_len, _np(rep.ep_len[:CAPACITY])), step
        if count <= 2 and count not in seen["early_batches"]:
            seen["early_batches"].append(count)
            u = torch.rand(4 * (H - N_STEPS + 1), generator=torch.Generator().manual_seed(step))
            ring = dict(count=count, head=head, capacity=CAPACITY, ep_len=ep_len, **ep)
            _assert_same_batch(gr.sample_windows_ref(4, H, N_STEPS, ring, u[:4].numpy(), u[4:].numpy()), rep.sample_batch_nstep(4, uniforms=u), ("early", step))
    for f in gr.RING_FIELDS:
        assert np.array_equal(ep[f], _np(getattr(rep, "ep_" + f)[:CAPACITY])), f
    return rep, dict(count=count, head=head, capacity=CAPACITY, ep_len=ep_len, **ep), seen


def test_store_rank_commit_advance_refs_equal_the_torch_bookkeeping(stream_run):
    """(the comparisons run step by step inside the fixture) the stream wrapped the ring and met the rows the rules differ on"""
    rep, ring, seen = stream_run
    assert ring["count"] == CAPACITY and rep.count == CAPACITY, "the ring never filled"
    assert seen["lift_end"] > 0 and seen["dropped"] > 0, seen
    assert 0 in seen["early_batches"], seen


def test_sample_windows_ref_equals_the_torch_sampler(stream_run):
    """every row of the batch, padding rows included (the torch path gathers them by the same rule), on the wrapped ring and with
    uniforms at 0 and just below 1"""
    rep, ring, _ = stream_run
    B, W = 64, HORIZON - N_STEPS
    u = torch.rand(B * (W + 1), generator=torch.Generator().manual_seed(9))
    u[0], u[1], u[B], u[B + 1] = 0.0, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24, 0.0
    ref = gr.sample_windows_ref(B, HORIZON, N_STEPS, ring, u[:B].numpy(), u[B:].numpy())
    _assert_same_batch(ref, rep.sample_batch_nstep(B, uniforms=u), "one ring")
    newest = (ring["head"] - 1) % CAPACITY
    assert all(slot != newest for slot, _ in ref[6])
    assert 0 < ref[5].sum() < B * W


def test_sample_windows_ref_two_rings_equals_sample_mixed(stream_run):
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    rep, ring, _ = stream_run
    g = torch.Generator().manual_seed(21)
    ex = DeviceEpisodeReplay(4, capacity=7, horizon=HORIZON, device="cpu")
    for name in ("ep_state", "ep_next", "ep_action", "ep_reward", "ep_not_done"):
        getattr(ex, name).copy_(torch.randn(getattr(ex, name).shape, generator=g))
    ex.ep_len[:7] = torch.tensor([30, 6, 7, 12, 5, 4, 30])
    B, W = 10, HORIZON - N_STEPS
    u = torch.rand(B * (W + 1), generator=g)
    # (5, 2): wrapped in a ring that was refilled, slots 4, 5, 6, 0, 1; counts 0, 1 and 2 - which the stream passes in one step - on their own
    for count, head in ((5, 2), (0, 0), (1, 1), (2, 2)):
        ex._count.fill_(count); ex._head.fill_(head)
        for prob, b_agent in ((0.3, 7), (1.0, 0), (0.0, 10)):
            ref = gr.sample_windows_ref(B, HORIZON, N_STEPS, ring, u[:B].numpy(), u[B:].numpy(), expert=_ring_of(ex), batch_agent=b_agent)
            _assert_same_batch(ref, rep.sample_mixed(ex, B, prob=prob, uniforms=u), (count, prob))
            assert count >= 2 or not ref[5].reshape(B, W)[b_agent:].any()
        _assert_same_batch(gr.sample_windows_ref(B, HORIZON, N_STEPS, _ring_of(ex), u[:B].numpy(), u[B:].numpy()), ex.sample_batch_nstep(B, uniforms=u), count)


@pytest.mark.parametrize("auto_reset", [0, 1])
@pytest.mark.parametrize("H", [30, 7])
def test_store_transition_ref_equals_the_torch_path_on_the_edge_rows(H, auto_reset):
    """the enumerated rows of glue_ref.store_cases - open episodes at and beyond H - 1, a lift that ends with nothing stored, lengths
    on both sides of the keep rule - which the random stream above never meets (it never stores into an open episode that holds H - 1 transitions)"""
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from kinovagrasping_amd.rollout import RolloutEngine
    sim_in, e, cur = gr.store_cases(H, N_STEPS, seed=H)
    n = len(sim_in["done"])
    sim = _FakeSim(n, torch.device("cpu"))
    sim.cfg.auto_reset = auto_reset
    rep = DeviceEpisodeReplay(n, capacity=CAPACITY, horizon=H, device="cpu")
    eng = RolloutEngine(sim, SimpleNamespace(actor=None), rep, generator=torch.Generator())
    for k in ("obs", "prev_obs", "has_prev", "t", "ready", "lifting", "action"):
        getattr(eng, k).copy_(torch.as_tensor(e[k]).to(getattr(eng, k).dtype))
    for k in ("cur_state", "cur_next", "cur_action", "cur_reward", "cur_not_done", "cur_len"):
        getattr(rep, k).copy_(torch.as_tensor(cur[k]))
    sim.obs.copy_(torch.as_tensor(sim_in["obs"])); sim.final_obs.copy_(torch.as_tensor(sim_in["final_obs"]))
    sim.reward.copy_(torch.as_tensor(sim_in["reward"])); sim.done.copy_(torch.as_tensor(sim_in["done"]))
    eng.post()
    for i in range(n):
        gr.store_transition_ref(i, H, N_STEPS, auto_reset, sim_in, e, cur)
    for k in ("obs", "prev_obs", "has_prev", "t", "ready", "reward_out", "done_out"):
        assert np.array_equal(e[k], _np(getattr(eng, k))), k
    for k in ("cur_state", "cur_next", "cur_action", "cur_reward", "cur_not_done"):
        assert np.array_equal(cur[k].view(np.uint32), _np(getattr(rep, k)).view(np.uint32)), k
    # the torch path has committed the kept episodes already: the same through the references
    rank, total = gr.rank_ref(cur["keep"])
    z = lambda *s: np.zeros(s, np.float32)
    ep = dict(state=z(CAPACITY, H, 82), next=z(CAPACITY, H, 82), action=z(CAPACITY, H, 4), reward=z(CAPACITY, H), not_done=z(CAPACITY, H))
    ep_len = np.zeros(CAPACITY, np.int64)
    gr.commit_ref(cur["keep"], rank, 0, CAPACITY, {f: cur["cur_" + f] for f in gr.RING_FIELDS}, cur["cur_len"], ep, ep_len)
    head, count, cur_len = gr.advance_ref(total, 0, 0, CAPACITY, e["done_out"], cur["cur_len"])
    assert total > 0 and (head, count) == (rep.head, rep.count) and np.array_equal(cur_len, _np(rep.cur_len))
    assert np.array_equal(ep_len, _np(rep.ep_len[:CAPACITY]))
    for f in gr.RING_FIELDS:
        assert np.array_equal(ep[f], _np(getattr(rep, "ep_" + f)[:CAPACITY])), f
