"""TD3fD through the native update and the trainers (GPU): one update against float64 autograd of ddpgfd.TD3fD in the three forms of
learner_native (LDS-free, lean, library GEMMs), the degenerate TD3fD that must be the DDPGfD update, the delayed actor, the trainers'
captures and the priorities written from the target the update used."""
import warnings

import numpy as np
import pytest
import torch

from tests import priority_ref as pr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FORMS = [((256, 256), None), ((400, 300), True), ((200, 100), None)]          # LDS-free, lean, library GEMMs
FORM_IDS = ["ldsfree-256", "lean-400-300", "library-200-100"]
NETS = ("actor", "critic", "critic2", "actor_target", "critic_target", "critic2_target")


class _NoStep:
    def step(self):
        pass

    def zero_grad(self):
        pass


def _batch(R=37, n=5, seed=11):
    g = torch.Generator(device=DEV).manual_seed(seed)
    st = torch.randn(R, n, 82, device=DEV, generator=g) * 0.3
    ns = torch.randn(R, n, 82, device=DEV, generator=g) * 0.3
    ac = torch.rand(R, n, 4, device=DEV, generator=g) * 0.8
    rw = torch.rand(R, n, device=DEV, generator=g) * 5
    w = (torch.rand(R, device=DEV, generator=g) < 0.7).float()
    w[:3] = 0
    w[3] = 1
    z = torch.randn(2 * R, 4, device=DEV, generator=g) * 2
    return st, ac, ns, rw, w, z


def _check_form(nat, hidden, lean):
    if hidden == (256, 256):
        assert nat.lds_free and not nat.lean_kernels
    elif lean:
        assert nat.lds_free and nat.lean_kernels
    else:
        assert not nat.lds_free and not nat.lean_kernels


@pytest.mark.parametrize("hidden,lean", FORMS, ids=FORM_IDS)
def test_td3_update_against_fp64_autograd(hidden, lean):
    """The batch and the criterion of test_lean_learner_update_against_fp64_autograd (R = 37 masked rows, n = 5; per tensor the native
    error is at most 4 x that of fp32 torch autograd on the same data, or 1e-6 of the tensor's largest entry), with given smoothing
    draws of which some lie beyond the clip: the six losses, both critics' gradients, the actor's gradient."""
    from kinovagrasping_amd.ddpgfd import TD3fD
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate

    def make():
        torch.manual_seed(7)
        return TD3fD(82, 4, 0.8, 5, hidden=hidden, device=DEV)

    p32, pn, p64 = make(), make(), make()
    for name in NETS:
        getattr(p64, name).double()
    p64._disc = p64._disc.double()
    nat = NativeDDPGfDUpdate(pn, lean=lean)
    _check_form(nat, hidden, lean)
    assert nat.td3 and nat.losses.numel() == 6
    st, ac, ns, rw, w, z = _batch()
    assert 0 < w.sum().item() < w.numel() and (pn.policy_noise * z.abs() > pn.noise_clip).any() and (pn.policy_noise * z.abs() < pn.noise_clip).any()

    def compare(native, t32, t64, what):
        for k, (a, b, c) in enumerate(zip(native, t32, t64)):
            a, b, c = a.double(), b.double(), c.double()
            e_nat, e_32 = (a - c).abs().max().item(), (b - c).abs().max().item()
            print(f"{what}[{k}]: native error {e_nat:.3g}, fp32 autograd error {e_32:.3g}, largest entry {c.abs().max().item():.3g}")
            assert e_nat <= max(4 * e_32, 1e-6 * c.abs().max().item()), (what, k, e_nat, e_32, c.abs().max().item())

    l32 = p32.phase_critic(st, ac, ns, rw, w, z)
    l64 = p64.phase_critic(st.double(), ac.double(), ns.double(), rw.double(), w.double(), z.double())
    ln = nat.phase_critic(st, ac, ns, rw, w, target_noise=z)
    torch.cuda.synchronize()
    assert len(ln) == 6
    one = lambda ls: [x.reshape(1) for x in ls]
    compare(one(ln), one(l32), one(l64), "critic losses")
    grads = lambda m: [p.grad for p in m.parameters()]
    nat_grads = lambda net: [t for pair in zip(net.gW, net.gb) for t in pair]
    compare(nat_grads(nat.critic), grads(p32.critic), grads(p64.critic), "critic gradient")
    compare(nat_grads(nat.critic2), grads(p32.critic2), grads(p64.critic2), "critic2 gradient")
    # actor phase: the reference critic takes the native critic's parameters after its Adam step
    before2 = nat.critic2.flat.clone()
    nat.phase_actor(st, w)
    torch.cuda.synchronize()
    assert not torch.equal(before2, nat.critic2.flat)                   # the second critic has stepped too
    p32._flat_params["critic"].copy_(nat.critic.flat)
    for q, src in zip(p64.critic.parameters(), pn.critic.parameters()):
        q.data.copy_(src.data.double())
    for p in (p32, p64):
        p.critic_optimizer, p.critic2_optimizer = _NoStep(), _NoStep()
    p32.phase_actor(st, w)
    p64.phase_actor(st.double(), w.double())
    compare(nat_grads(nat.actor), grads(p32.actor), grads(p64.actor), "actor gradient")


def _degenerate(hidden, lean):
    """NativeDDPGfDUpdate on a DDPGfD and, from the same seed, on a TD3fD without noise and delay whose second critic copies the first"""
    from kinovagrasping_amd.ddpgfd import DDPGfD, TD3fD
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    torch.manual_seed(7)
    ddpg = DDPGfD(82, 4, 0.8, 5, hidden=hidden, device=DEV)
    torch.manual_seed(7)
    td3 = TD3fD(82, 4, 0.8, 5, hidden=hidden, device=DEV, policy_noise=0.0, policy_freq=1)
    for k in ("critic", "critic_target"):
        td3._flat_params[k.replace("critic", "critic2")].copy_(td3._flat_params[k])
    return NativeDDPGfDUpdate(ddpg, lean=lean), NativeDDPGfDUpdate(td3, lean=lean)


@pytest.mark.parametrize("hidden,lean", FORMS, ids=FORM_IDS)
def test_degenerate_td3_update_is_the_ddpgfd_update(hidden, lean):
    """3 updates each (the smoothing on its in-kernel stream, at sigma 0): actor, critic, both targets and their Adam moments are equal in
    every bit on the LDS-free and lean kernels, within 1e-6 on the library path; the copied critic stays a copy"""
    a, b = _degenerate(hidden, lean)
    _check_form(b, hidden, lean)
    for it in range(3):
        st, ac, ns, rw, w, _ = _batch(R=75, seed=20 + it)
        la, lb = a.train_on_batch(st, ac, ns, rw, w), b.train_on_batch(st, ac, ns, rw, w)
    torch.cuda.synchronize()
    pairs = [(f"flat {k}", a.p._flat_params[k], b.p._flat_params[k]) for k in ("actor", "critic", "actor_target", "critic_target")]
    for name in ("actor", "critic"):
        na, nb = getattr(a, name), getattr(b, name)
        pairs += [(f"{name} exp_avg", na.exp_avg, nb.exp_avg), (f"{name} exp_avg_sq", na.exp_avg_sq, nb.exp_avg_sq)]
    pairs += [(f"loss {k}", la[k], lb[k]) for k in range(3)] + [(f"loss2 {k}", la[k], lb[3 + k]) for k in range(3)]
    pairs += [("critic2", b.critic.flat, b.critic2.flat), ("critic2 target", b.critic_t.flat, b.critic2_t.flat), ("critic2 exp_avg", b.critic.exp_avg, b.critic2.exp_avg)]
    for what, x, y in pairs:
        if b.lds_free:
            assert torch.equal(x, y), (what, (x - y).abs().max().item())
        else:
            assert (x - y).abs().max().item() <= 1e-6, (what, (x - y).abs().max().item())
    assert int(a.it.item()) == int(b.it.item()) == 3 and a.p.total_it == b.p.total_it == 3


@pytest.mark.parametrize("form", ["eager", "pipelined"])
def test_the_actor_steps_on_every_second_update_only(form):
    """policy_freq = 2, through phase_targets (eager) and through phase_head (pipelined: the step of update k is applied by the head of
    update k + 1, the last one by finish_pending): the actor's weights and both moments are bit-unchanged by updates 1 and 3 and changed
    by 2 and 4, the critics step every time; the exported actor optimizer is at step 2 after update 4, the critics' at 4"""
    from kinovagrasping_amd.ddpgfd import TD3fD
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    torch.manual_seed(5)
    pol = TD3fD(82, 4, 0.8, 5, hidden=(64, 64), device=DEV, policy_freq=2)
    nat = NativeDDPGfDUpdate(pol)
    nat.pipelined = form == "pipelined"
    snap = lambda: tuple(t.clone() for t in (nat.actor.flat, nat.actor.exp_avg, nat.actor.exp_avg_sq))
    states, critics = [snap()], [nat.critic2.flat.clone()]
    for k in range(1, 5):
        st, ac, ns, rw, w, _ = _batch(R=50, seed=40 + k)
        if form == "eager":
            nat.train_on_batch(st, ac, ns, rw, w)
        else:
            nat.phase_head()                         # applies update k - 1's actor step
            torch.cuda.synchronize()
            if k > 1:
                states.append(snap())
            nat.phase_critic(st, ac, ns, rw, w)
            nat.phase_actor(st, w)
        if form == "eager":
            torch.cuda.synchronize()
            states.append(snap())
        critics.append(nat.critic2.flat.clone())
    if form == "pipelined":
        nat.finish_pending()
        torch.cuda.synchronize()
        states.append(snap())
    same = [all(torch.equal(x, y) for x, y in zip(states[k - 1], states[k])) for k in range(1, 5)]
    assert same == [True, False, True, False], same
    assert not any(torch.equal(x, y) for x, y in zip(states[1], states[2])) and not any(torch.equal(x, y) for x, y in zip(states[3], states[4]))
    assert all(not torch.equal(critics[k - 1], critics[k]) for k in range(1, 5))
    nat.export_optimizer_state()
    steps = lambda opt: {float(s["step"]) for s in opt.state.values()}
    assert steps(pol.actor_optimizer) == {2.0} and steps(pol.critic_optimizer) == {4.0} and steps(pol.critic2_optimizer) == {4.0}
    nat.import_optimizer_state()
    assert int(nat.it.item()) == 4


def test_capturable_autograd_gate_equals_the_host_gate():
    """TD3fD(capturable=True): the delayed step and the soft update gated on the device give what the host-gated phases give"""
    from kinovagrasping_amd.ddpgfd import TD3fD
    pols = []
    for cap in (False, True):
        torch.manual_seed(9)
        pol = TD3fD(82, 4, 0.8, 5, hidden=(32, 32), device=DEV, capturable=cap, policy_freq=2)
        pol.network_repl_freq = 3
        pols.append(pol)
    for k in range(1, 5):
        st, ac, ns, rw, w, z = _batch(R=20, seed=60 + k)
        before = [p._flat_params["actor"].clone() for p in pols]
        for p in pols:
            p.train_on_batch(st, ac, ns, rw, w, z)
        for p, b in zip(pols, before):
            assert torch.equal(p._flat_params["actor"], b) == (k % 2 == 1), k
    for name in NETS:
        assert (pols[0]._flat_params[name] - pols[1]._flat_params[name]).abs().max().item() <= 1e-6, name
    assert {float(s["step"]) for s in pols[1].actor_optimizer.state.values()} == {2.0}


def test_the_fork_form_refuses_a_td3fd_policy(monkeypatch):
    from kinovagrasping_amd.ddpgfd import TD3fD
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    monkeypatch.setenv("KS_LEARNER_FORK", "1")
    torch.manual_seed(1)
    with pytest.raises(ValueError):
        NativeDDPGfDUpdate(TD3fD(82, 4, 0.8, 5, hidden=(256, 256), device=DEV))


def test_a_replayed_captured_td3_update_equals_the_eager_one_bit_for_bit():
    """the pattern of test_forked_update_equals_the_single_stream_update_bit_for_bit: 4 updates eager and 4 replays of one captured
    update on the same batches (in-kernel smoothing noise, keyed by the update count in both) - all six networks, three gradient and
    moment sets equal in every bit"""
    from kinovagrasping_amd.ddpgfd import TD3fD
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    bs = [_batch(R=80, seed=70 + k)[:5] for k in range(4)]

    def fresh():
        torch.manual_seed(7)
        return TD3fD(82, 4, 0.8, 5, hidden=(64, 64), device=DEV)

    def run(graph):
        pol = fresh()
        nat = NativeDDPGfDUpdate(pol)
        if not graph:
            for b in bs:
                nat.train_on_batch(*b)
        else:
            static = [t.clone() for t in bs[0]]
            s = torch.cuda.Stream(DEV)
            s.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(s):
                nat.train_on_batch(*static)                                   # warm-up outside the capture
            torch.cuda.current_stream(DEV).wait_stream(s)
            torch.cuda.synchronize()
            pol2 = fresh()
            for k in pol._flat_params:
                pol._flat_params[k].copy_(pol2._flat_params[k])
            for net in (nat.actor, nat.critic, nat.critic2):
                net.grad.zero_(); net.exp_avg.zero_(); net.exp_avg_sq.zero_()
            nat.it.zero_(); nat.it_head.zero_(); pol.total_it = 0
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                nat.train_on_batch(*static)
            for b in bs:
                for dst, src in zip(static, b):
                    dst.copy_(src)
                g.replay()
        torch.cuda.synchronize()
        return ({k: v.clone() for k, v in pol._flat_params.items()},
                [(n.grad.clone(), n.exp_avg.clone(), n.exp_avg_sq.clone()) for n in (nat.actor, nat.critic, nat.critic2)], nat.losses.clone())

    ref_p, ref_o, ref_l = run(False)
    p, o, l = run(True)
    assert set(p) == set(NETS)
    for k in ref_p:
        assert torch.equal(p[k], ref_p[k]), (k, (p[k] - ref_p[k]).abs().max().item())
    for a, b in zip(o, ref_o):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(l, ref_l) and torch.isfinite(l).all()


# ---- the trainers ------------------------------------------------------------------------------------------------------------------------
def _setup(n=64, horizon=12):
    from kinovagrasping_amd import scenarios
    from kinovagrasping_amd.ddpgfd import TD3fD
    from kinovagrasping_amd.multi_shape import MultiShapeSim
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from kinovagrasping_amd.rollout import RolloutEngine
    rng = np.random.RandomState(4)
    sim = MultiShapeSim(n, ["CubeS"], device=0, auto_reset=True, horizon=horizon)
    qp, hqp, _ = scenarios.draw_start_pool(["CubeS"] * n, "normal", 4, rng)
    sim.reset(torch.as_tensor(qp[0]), torch.as_tensor(hqp[0]), object_id=sim.shape_of_env)
    obs0 = sim.set_start_pool(torch.as_tensor(qp), torch.as_tensor(hqp), seed=2)
    torch.manual_seed(2)
    policy = TD3fD(82, 4, 0.8, 5, batch_size=8, hidden=(64, 64), device=sim.device)
    replay = DeviceEpisodeReplay(n, capacity=8 * n, horizon=horizon, device=sim.device)
    eng = RolloutEngine(sim, policy, replay, expl_noise=0.1)
    eng.start(obs0)
    return sim, policy, replay, eng


def _learner_state(tr):
    nat = tr.native
    out = {k: v.clone() for k, v in tr.policy._flat_params.items()}
    for name in ("actor", "critic", "critic2"):
        net = getattr(nat, name)
        out[name + ".exp_avg"], out[name + ".exp_avg_sq"] = net.exp_avg.clone(), net.exp_avg_sq.clone()
    out["it"], out["it_head"] = nat.it.clone(), nat.it_head.clone()
    return out


def _check_trained(tr, before, updates):
    torch.cuda.synchronize()
    nat = tr.native
    assert (tr.updates == updates if isinstance(updates, int) else tr.updates >= updates[0]) and int(nat.it.item()) == tr.updates and int(nat.it_head.item()) == 0
    assert nat.losses.numel() == 6 and torch.isfinite(nat.losses).all()
    after = _learner_state(tr)
    assert all(torch.isfinite(v).all() for v in after.values())
    for k in NETS + ("critic2.exp_avg", "critic2.exp_avg_sq", "actor.exp_avg"):
        assert not torch.equal(after[k], before[k]), k


def test_graphed_trainer_trains_a_td3fd_policy():
    """64 envs, lock step: capture() leaves the six networks, the three moment sets and the counters as before its warm-up; 45 env-steps
    then count their updates (more than 10: the targets move at update 10), six finite losses, and critic2 and its target have moved"""
    from kinovagrasping_amd.pipeline import GraphedTrainer
    sim, policy, replay, eng = _setup()
    tr = GraphedTrainer(sim, policy, replay, eng, batch_episodes=8)
    assert tr.native.td3 and tr.native.seed == tr.sample_seed & (2 ** 64 - 1)
    before = _learner_state(tr)
    tr.capture()
    torch.cuda.synchronize()
    for k, v in _learner_state(tr).items():
        assert torch.equal(v, before[k]), k
    for _ in range(45):
        tr.step()
    tr.flush(finish_update=True)
    _check_trained(tr, before, (11,))
    sim.close()


def test_async_trainer_trains_a_td3fd_policy():
    """the free-running form on the same set-up: three launches of 13 env-steps with captured graphs"""
    from kinovagrasping_amd.pipeline import AsyncTrainer
    sim, policy, replay, eng = _setup()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=8)
    before = _learner_state(tr)
    tr.capture()
    torch.cuda.synchronize()
    for k, v in _learner_state(tr).items():
        assert torch.equal(v, before[k]), k
    for _ in range(3):
        tr.run(13)
        tr.flush()
    tr.flush(finish_update=True)
    _check_trained(tr, before, 39)
    c = tr.counts()
    assert c["pacing_timeouts"] == 0 and c["episodes_kept"] == replay.count
    sim.close()


def test_priorities_come_from_the_first_critic_and_the_twin_minimum():
    """GraphedTrainer(prioritized=True) with a TD3fD policy, one eager update on a filled ring: the callback receives q1 and tmin [2R],
    and per_delta is tests/priority_ref.py's delta on exactly those in every bit"""
    from kinovagrasping_amd.pipeline import GraphedTrainer
    sim, policy, replay, eng = _setup()
    tr = GraphedTrainer(sim, policy, replay, eng, batch_episodes=8, overlap=False, prioritized=True, per_alpha=0.6, per_beta=0.4, per_eps=1e-3)
    for _ in range(26):
        eng.step()
    torch.cuda.synchronize()
    assert replay.count >= 2 * 64
    seen = {}
    inner = tr._update_priorities

    def record(q, tq1, reward, weight):
        seen.update(q=q.clone(), tq1=tq1.clone(), reward=reward.clone(), weight=weight.clone())
        inner(q, tq1, reward, weight)

    tr._update_priorities = record
    tr._learn_eager()
    torch.cuda.synchronize()
    B, n = 8, replay.n_steps
    W = replay.horizon - n
    R = B * W
    assert tuple(seen["tq1"].shape) == (2 * R,) and tuple(seen["q"].shape) == (R, 1)
    host = {k: v.cpu().numpy() for k, v in seen.items()}
    ref = pr.episode_deltas_ref(B, W, n, host["q"], host["tq1"][:R], host["reward"], host["weight"], policy.discount)
    got = tr.per_delta.cpu().numpy()
    assert np.isfinite(got).all() and (got >= 0).all() and got.tobytes() == ref.tobytes(), (got, ref)
    sim.close()
