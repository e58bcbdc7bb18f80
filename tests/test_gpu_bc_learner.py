"""The behaviour-cloning term of the actor loss with its Q-filter (ddpgfd: bc_weight, q_filter; kr_bc_actor_grad) through the native update and
the trainers (GPU), by the method of tests/test_gpu_bounded_learner.py: one and ten updates against float64 autograd of the same policy
in the forms of learner_native (LDS-free, lean, library GEMMs) for DDPGfD and TD3fD, on windows and on episode tables, bc_weight = 0 as the
update it was in launches and bits, and the trainers' captures.

The Q-filter is a comparison of two critic outputs, and a demonstration state whose two values lie within float32's error of each other
passes in one evaluation and fails in another; the criterion of _compare is about arithmetic, not about which side of the threshold a
float32 sum lands on.  Such states are treated like the rows near a ReLU kink: a window row with a demonstration state whose float64 margin
|Q(s, a) - Q(s, pi(s))| is below tau gets weight 0 in all three evaluations, tau = 16 x the worst |Q of fp32 autograd - Q of float64| on
the batch - computed from the two references only.  From the float64 policy alone the tests assert that at most 2 % of the demonstration
rows go that way and that both outcomes of the filter occur among the rest."""
import warnings

import numpy as np
import pytest
import torch

from tests.test_gpu_bounded_learner import FORM_IDS, FORMS, _batch, _check_form, _compare, _double, _kink_rows, _make, _NoStep, _Recorder, _state, _sync

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
B, W, N, H = 8, 25, 5, 30
DEMO_FROM = 5 * W                       # int(8 * (1 - 0.3)) = 5 agent episodes, 3 expert ones
BC = dict(bc_weight=2.0)
# The batch of the one-update tests (tests/test_gpu_bounded_learner.py's _batch at this seed), chosen on the host from the float64 policy
# alone: in all eight (form, learner) cases no demonstration state's margin |Q(s, a) - Q(s, pi(s))| is below 5e-5 - several tau - and at
# most one row has a state below 1e-4, while both outcomes of the filter occur (pass shares 0.4 to 0.6).  The table batch's seed likewise:
# every margin is above 20 tau.
BATCH_SEED = 19


def _margins(p32, p64, st, ac, demo_from):
    """from the two autograd policies (their critics as stepped): tau, the window rows r >= demo_from with a state inside the margin, and
    the float64 filter [R, n]"""
    with torch.no_grad():
        s64, a64 = st.double(), ac.double()
        qa64, qp64 = p64.critic(s64, a64), p64.critic(s64, p64.actor(s64))
        qa32, qp32 = p32.critic(st, ac), p32.critic(st, p32.actor(st))
        tau = 16 * max((qa32.double() - qa64).abs().max().item(), (qp32.double() - qp64).abs().max().item())
        near = ((qa64 - qp64).abs() < tau).squeeze(-1).any(1)
        near[:demo_from] = False
        return tau, near, (qa64 > qp64).squeeze(-1)


def _table_batch(seed=31):
    """the 8 x 25 x 5 batch as episode tables: 5 agent and 3 expert episodes of H = 30 from two filled rings (explicit uniforms), states
    and rewards scaled as tests/test_gpu_bounded_learner.py's batch; one agent and one expert episode are short (padding rows)"""
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from tests import tables_ref as tr
    rings = []
    for k, cap in enumerate((8, 6)):
        rep = tr.fill_ring(DeviceEpisodeReplay(2, cap, horizon=H, n_steps=N, device=DEV), cap - 1, cap - 1, seed=seed + k)
        rep.ep_state.sub_(0.5).mul_(1.0)
        rep.ep_next.sub_(0.5).mul_(1.0)
        rep.ep_action.mul_(0.8)
        rep.ep_reward.mul_(5.0)
        rep.ep_len.fill_(H)
        rep.ep_len[1] = 12
        rings.append(rep)
    u = torch.rand(B * (W + 1), generator=torch.Generator(device="cpu").manual_seed(seed))
    tb = rings[0].sample_tables(rings[1], B, 0.3, uniforms=u.to(DEV), next_ends=True)
    assert tb.weight.shape[0] == B * W and tb.horizon == H and tb.n_steps == N
    return tb


def _bc_update(nats, p32, p64, k, batch, td3, demo_from):
    """Update k + 1 of every native learner of `nats` - pairs (learner, TableBatch or None for the window form), all in the same state -
    checked against float64 autograd as tests/test_gpu_bounded_learner.py's _checked_update does for the actor phase: both autograd
    policies start from the native state, the rows near a ReLU kink and the demonstration rows inside the filter's margin are padding in
    all evaluations, and for the actor phase both take the native critics as stepped.  Compared by _compare: the actor's gradient and the
    three tracked losses (actor loss, its behaviour-cloning part, the filter's pass share).  Returns what the callers assert on."""
    st, ac, ns, rw, w0, z = batch
    d = lambda t: t.double()
    e32, e64 = ((z,), (d(z),)) if td3 else ((), ())
    n, R = st.shape[1], st.shape[0]
    grads = lambda m: [q.grad.clone() for q in m.parameters()]
    nat_grads = lambda net: [t for pair in zip(net.gW, net.gb) for t in pair]
    critics = ("critic", "critic2") if td3 else ("critic",)
    first = nats[0][0]
    _sync(p64, first, td3, k)
    _sync(p32, first, td3, k)
    rows_c = _kink_rows(p64, d(st), d(ac), td3)[0]
    w_c = torch.where(rows_c, torch.zeros_like(w0), w0)
    p64.phase_critic(d(st), d(ac), d(ns), d(rw), d(w_c), *e64)
    p32.phase_critic(st, ac, ns, rw, w_c, *e32)
    for nat, tb in nats:
        nat.track_actor_loss = True
        if tb is None:
            nat.phase_critic(st, ac, ns, rw, w_c, **(dict(target_noise=z) if td3 else {}))
        else:
            nat.phase_critic_tables(tb._replace(weight=w_c), target_noise=z if td3 else None)
    # the autograd policies' own critic steps show the actor phase's rows near a kink and the filter's margins
    p64.phase_actor(d(st), d(w_c), d(ac), demo_from)
    p32.phase_actor(st, w_c, ac, demo_from)
    rows_a = _kink_rows(p64, d(st), d(ac), td3)[1]
    tau, near = 0.0, torch.zeros_like(rows_a)
    if p64.q_filter:
        tau, near, f64 = _margins(p32, p64, st, ac, demo_from)
        assert int(near.sum()) <= 0.02 * (R - demo_from), (int(near.sum()), R - demo_from, tau)
        live = f64[demo_from:][((w_c > 0) & ~rows_a & ~near)[demo_from:]]
        assert live.any() and not live.all(), "both outcomes of the filter must occur on the batch"
    w_a = torch.where(rows_a | near, torch.zeros_like(w_c), w_c)
    assert w_a.sum() > 0.5 * w0.sum() and w_a[demo_from:].sum() > 0.5 * w0[demo_from:].sum()
    wsum = w_a.sum().clamp_min(1.0)
    scale = -1.0 / (wsum * float(n))
    for nat, tb in nats:
        # the prologue's outputs rewritten for w_a, as the prologue forms them
        nat.weight = w_a
        nat.wsum.copy_(wsum.view(1))
        if tb is None:
            nat.dq_actor.copy_((w_a * scale).repeat_interleave(n).view_as(nat.dq_actor))
            nat.phase_actor(st, w_a, ac, demo_from)
        else:
            nat.dq_table.copy_((tb.slot_weight * scale).repeat_interleave(tb.horizon).view_as(nat.dq_table))
            idx = tb.row_table.long().unsqueeze(1) + torch.arange(n, device=DEV)
            idx[w_a == 0] = -1
            nat.row_index.copy_(idx.reshape(-1).int())
            nat.phase_actor_tables(tb, demo_from)
    keep = {}
    for pol in (p32, p64):
        for name in critics:
            pol._flat_params[name].copy_(getattr(first, name).flat)
            keep[pol, name] = getattr(pol, name + "_optimizer")
            setattr(pol, name + "_optimizer", _NoStep())
    t64 = p64.phase_actor(d(st), d(w_a), d(ac), demo_from)
    a64, l64 = grads(p64.actor), [t64, p64.bc_loss, p64.bc_pass]
    t32 = p32.phase_actor(st, w_a, ac, demo_from)
    a32, l32 = grads(p32.actor), [t32, p32.bc_loss, p32.bc_pass]
    for (pol, name), opt in keep.items():
        setattr(pol, name + "_optimizer", opt)
    for nat, _ in nats:
        nat.phase_targets()
    torch.cuda.synchronize()
    one = lambda ls: [x.reshape(1) for x in ls]
    for nat, tb in nats:
        form = "tables" if tb is not None else "windows"
        _compare(nat_grads(nat.actor), a32, a64, f"update {k + 1} ({form}): actor gradient")
        _compare(one([nat.actor_loss, nat.bc_loss, nat.bc_pass]), one(l32), one(l64), f"update {k + 1} ({form}): actor loss, BC loss, pass share")
    return dict(tau=tau, near=int(near.sum()), share=p64.bc_pass.item(), bc=p64.bc_loss.item(), masked=int(((rows_c | rows_a | near) & (w0 > 0)).sum()))


def _three(td3, hidden, **kw):
    p32, pn, p64 = (_make(td3, hidden, **kw) for _ in range(3))
    return p32, pn, _double(p64, td3)


@pytest.mark.parametrize("q_filter", [False, True], ids=["nofilter", "filter"])
@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS, ids=FORM_IDS)
def test_one_update_on_windows_against_fp64_autograd(hidden, lean, td3, q_filter):
    """the first update on the 8 x 25 x 5 batch with demo_from = 5 * 25, in the four forms"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    p32, pn, p64 = _three(td3, hidden, q_filter=q_filter, **BC)
    nat = NativeDDPGfDUpdate(pn, lean=lean)
    _check_form(nat, hidden, lean)
    assert nat.bc_weight == 2.0 and nat.q_filter == q_filter and nat.td3 == td3
    info = _bc_update([(nat, None)], p32, p64, 0, _batch(seed=BATCH_SEED), td3, DEMO_FROM)
    print("window form:", info)
    assert info["bc"] > 0 and ((0 < info["share"] < 1) if q_filter else info["share"] == 1.0)
    assert int(nat.it.item()) == 1 and pn.total_it == 1


@pytest.mark.parametrize("q_filter", [False, True], ids=["nofilter", "filter"])
@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS[:3], ids=FORM_IDS[:3])
def test_one_update_on_tables_against_fp64_autograd_and_the_window_form(hidden, lean, td3, q_filter):
    """the same batch shape drawn as episode tables (the LDS-free forms): phase_actor_tables against float64 autograd on tb.windows(), and
    equal to phase_actor on tb.windows() bit for bit - the actor's gradient buffer and the three losses"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    p32, pn, p64 = _three(td3, hidden, q_filter=q_filter, **BC)
    tab, win = NativeDDPGfDUpdate(pn, lean=lean), NativeDDPGfDUpdate(_make(td3, hidden, q_filter=q_filter, **BC), lean=lean)
    _check_form(tab, hidden, lean)
    tb = _table_batch()
    st, ac, ns, rw, nd, w = tb.windows()
    z = (torch.randn(2 * w.shape[0], 4, generator=torch.Generator().manual_seed(4)) * 2).to(DEV)
    info = _bc_update([(tab, tb), (win, None)], p32, p64, 0, (st, ac, ns, rw, w, z), td3, DEMO_FROM)
    print("table form:", info)
    assert info["bc"] > 0 and ((0 < info["share"] < 1) if q_filter else info["share"] == 1.0)
    assert np.array_equal(tab.actor.grad.cpu().numpy(), win.actor.grad.cpu().numpy()) and tab.actor.grad.abs().max().item() > 0
    for name in ("actor_loss", "bc_loss", "bc_pass"):
        assert torch.equal(getattr(tab, name), getattr(win, name)), name
    assert torch.equal(tab.actor.flat, win.actor.flat)


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS, ids=FORM_IDS)
def test_ten_updates_against_fp64_autograd(hidden, lean, td3):
    """ten consecutive native updates on ten batches without the filter, each checked from the native state it starts in"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    p32, pn, p64 = _three(td3, hidden, **BC)
    nat = NativeDDPGfDUpdate(pn, lean=lean)
    _check_form(nat, hidden, lean)
    infos = [_bc_update([(nat, None)], p32, p64, k, _batch(seed=100 + k), td3, DEMO_FROM) for k in range(10)]
    print("rows masked per update:", [i["masked"] for i in infos], "BC loss:", ["%.4f" % i["bc"] for i in infos])
    assert all(i["share"] == 1.0 and i["bc"] > 0 for i in infos)
    assert int(nat.it.item()) == 10 and pn.total_it == 10


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS[:3], ids=FORM_IDS[:3])
def test_bc_weight_zero_is_the_update_as_it_was(hidden, lean, td3):
    """three native updates of a policy built with bc_weight=0, q_filter=False (actions and demo_from handed in) against a policy built
    without the arguments: the same launches, entry point by entry point, none of them kr_bc_actor_grad, and every parameter, gradient,
    moment and loss equal in every bit; with the term set the kernel runs once per update"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    a = NativeDDPGfDUpdate(_make(td3, hidden), lean=lean)
    b = NativeDDPGfDUpdate(_make(td3, hidden, bc_weight=0.0, q_filter=False), lean=lean)
    c = NativeDDPGfDUpdate(_make(td3, hidden, bc_weight=1.0, q_filter=True), lean=lean)
    _check_form(b, hidden, lean)
    for nat in (a, b, c):
        nat.lib = _Recorder(nat.lib)
    for it in range(3):
        st, ac, ns, rw, w, _ = _batch(seed=20 + it)
        a.train_on_batch(st, ac, ns, rw, w)
        b.train_on_batch(st, ac, ns, rw, w, demo_from=DEMO_FROM)
        c.train_on_batch(st, ac, ns, rw, w, demo_from=DEMO_FROM)
    torch.cuda.synchronize()
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert a.lib.calls == b.lib.calls and "kr_bc_actor_grad" not in b.lib.calls
    assert c.lib.calls["kr_bc_actor_grad"] == 3 and {k: v for k, v in c.lib.calls.items() if k != "kr_bc_actor_grad"} == a.lib.calls
    assert not torch.equal(_state(c)["actor"], sa["actor"]) and torch.isfinite(_state(c)["actor"]).all()
    with pytest.raises(ValueError):
        c.phase_actor(st, w)


# ---- the trainers ------------------------------------------------------------------------------------------------------------------------
def _trainer_setup(td3, **opts):
    """tests/test_gpu_bounded_learner.py's 64 envs at hidden 64-64, and a small expert ring filled from a fixed tensor"""
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from tests import tables_ref as tr
    from tests.test_gpu_bounded_learner import _setup
    sim, policy, replay, eng = _setup(td3, **opts)
    expert = tr.fill_ring(DeviceEpisodeReplay(64, capacity=16, horizon=replay.horizon, device=sim.device), 15, 15, seed=8)
    expert.ep_action.mul_(0.8)
    expert.ep_len.fill_(replay.horizon)
    return sim, policy, replay, eng, expert


def _captured_equals_eager(tr, policy):
    """from one learner state on a ring that no longer changes: 5 updates replayed from the trainer's captured graphs and 5 eager ones (the
    sampler is keyed by the update count in both) - networks, gradients, moments and the tracked losses equal in every bit"""
    nat = tr.native
    nets = tr._opt_nets()
    saved = ({k: v.clone() for k, v in policy._flat_params.items()}, [(net.grad.clone(), net.exp_avg.clone(), net.exp_avg_sq.clone()) for net in nets],
             nat.it.clone(), nat.it_head.clone(), policy.total_it)

    def restore():
        for k, v in saved[0].items():
            policy._flat_params[k].copy_(v)
        for net, (g, m, v) in zip(nets, saved[1]):
            net.grad.copy_(g); net.exp_avg.copy_(m); net.exp_avg_sq.copy_(v)
        nat.it.copy_(saved[2]); nat.it_head.copy_(saved[3])
        policy.total_it = saved[4]

    def snapshot():
        nat.finish_pending()
        torch.cuda.synchronize()
        out = _state(nat)
        out.update(it=nat.it.clone(), actor_loss=nat.actor_loss.clone(), bc_loss=nat.bc_loss.clone(), bc_pass=nat.bc_pass.clone())
        return out

    restore()
    for _ in range(5):
        tr.g_head.replay()
        tr.g_learn[0].replay()
    graphed = snapshot()
    restore()
    for _ in range(5):
        tr._learn_eager()
    eager = snapshot()
    for k in graphed:
        assert torch.equal(graphed[k], eager[k]), k
    assert int(graphed["it"].item()) == int(saved[2].item()) + 5 and torch.isfinite(graphed["losses"]).all()
    assert not torch.equal(graphed["actor"], saved[0]["actor"])
    return graphed


@pytest.mark.parametrize("tables", [False, True], ids=["windows", "tables"])
@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
def test_graphed_trainer_captured_equals_eager_in_every_bit(td3, tables):
    """GraphedTrainer on 64 envs with bc_weight = 1 and the filter, 5 agent + 3 expert episodes per batch: 5 updates replayed from the
    captured graphs and, from the same learner state, 5 eager ones - networks, moments and the tracked losses equal in every bit, the pass
    share inside (0, 1)"""
    from kinovagrasping_amd.pipeline import GraphedTrainer
    sim, policy, replay, eng, expert = _trainer_setup(td3, bc_weight=1.0, q_filter=True)
    tr = GraphedTrainer(sim, policy, replay, eng, batch_episodes=8, overlap=False, expert_replay=expert, expert_prob=0.3, tables=tables)
    nat = tr.native
    assert nat.bc_weight == 1.0 and nat.q_filter and tr.tables == tables and tr.demo_from == 5 * (replay.horizon - replay.n_steps)
    nat.track_actor_loss = True
    for _ in range(26):
        eng.step()
    tr.capture()
    torch.cuda.synchronize()
    assert replay.count >= 2 * 64
    graphed = _captured_equals_eager(tr, policy)
    assert 0 < graphed["bc_pass"].item() < 1 and graphed["bc_loss"].item() > 0
    sim.close()


def test_async_trainer_trains_with_the_bc_term(monkeypatch):
    """the free-running form on 64 envs, one launch of 13 env-steps with captured graphs: it runs, drops nothing, and the tracked BC loss
    and pass share are those of a filter that passes some states and rejects others; then, on the ring as the launch left it, its captured
    update equals the eager one in every bit (eager under the wave split AsyncTrainer.capture() bakes into its graphs)"""
    from kinovagrasping_amd.pipeline import AsyncTrainer
    sim, policy, replay, eng, expert = _trainer_setup(True, bc_weight=1.0, q_filter=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=8, expert_replay=expert, expert_prob=0.3)
    tr.native.track_actor_loss = True
    tr.capture()
    tr.run(13)
    tr.flush(finish_update=True)
    torch.cuda.synchronize()
    nat = tr.native
    c = tr.counts()
    assert tr.updates == 13 and int(nat.it.item()) == 13 and int(nat.it_head.item()) == 0
    assert c["pacing_timeouts"] == 0 and c["episodes_kept"] == replay.count
    assert torch.isfinite(nat.losses).all() and torch.isfinite(nat.actor_loss).all()
    assert 0 < nat.bc_pass.item() < 1 and nat.bc_loss.item() > 0
    import os
    monkeypatch.setenv("KS_MLP_SPLIT", os.environ.get("KS_ASYNC_MLP_SPLIT", "0"))
    graphed = _captured_equals_eager(tr, policy)
    assert 0 < graphed["bc_pass"].item() < 1
    sim.close()


@pytest.mark.parametrize("which", ["graphed", "async"])
def test_the_trainers_refuse_the_term_without_demonstrations(which):
    """bc_weight > 0 without an expert ring, or with expert_prob = 0: ValueError at construction"""
    from kinovagrasping_amd.pipeline import AsyncTrainer, GraphedTrainer
    sim, policy, replay, eng, expert = _trainer_setup(False, bc_weight=1.0)
    Trainer = GraphedTrainer if which == "graphed" else AsyncTrainer
    kw = dict(overlap=False) if which == "graphed" else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(ValueError):
            Trainer(sim, policy, replay, eng, batch_episodes=8, **kw)
        with pytest.raises(ValueError):
            Trainer(sim, policy, replay, eng, batch_episodes=8, expert_replay=expert, expert_prob=0.0, **kw)
    sim.close()
