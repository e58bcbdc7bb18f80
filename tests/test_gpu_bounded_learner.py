"""The bounded critic update (q_bounds, huber_delta, max_grad_norm) through the native update and the trainers (GPU): one and ten updates
against float64 autograd of the same policy in the forms of learner_native (LDS-free, lean, library GEMMs) for DDPGfD and TD3fD, the
infinite settings that must be the unset update in every bit, the launch sequences, the fork form's refusal, the trainers' captures and
the priorities written from the bootstrap the update used."""
import warnings

import numpy as np
import pytest
import torch

from tests import priority_ref as pr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FORMS = [((64, 64), None), ((256, 256), None), ((400, 300), True), ((200, 100), None)]          # LDS-free twice, lean, library GEMMs
FORM_IDS = ["ldsfree-64", "ldsfree-256", "lean-400-300", "library-200-100"]
INF = float("inf")
# The batch below has rewards in [0, 5) and freshly initialised critics, whose outputs lie between about -2 and 1 at every width used here
# (for TD3fD's minimum of two: below 0): the bootstrap leaves [-0.5, -0.2] on both sides and stays inside it for some rows, the errors
# (targets up to 25) straddle delta = 2, the critics' gradient norms are between 1 and 30 and the actor's first one is below 0.5 - every
# branch of the three options is taken, which the tests assert from the float64 policy and from native.clip.
OPTS = dict(q_bounds=(-0.5, -0.2), huber_delta=2.0, max_grad_norm=0.5)
NEW = ("kr_critic_grad_bounded", "kr_grad_sqnorm", "kr_adam_step_clipped")
OLD = ("kr_critic_grad", "kr_twin_critic_grad", "kr_adam_step", "kr_adam_step_every")


def _batch(seed=11, B=8, W=25, n=5, device=DEV):
    """8 episodes x 25 windows; drawn on the host, so that the rows are the same wherever the test runs"""
    R = B * W
    g = torch.Generator().manual_seed(seed)
    st = torch.randn(R, n, 82, generator=g) * 0.3
    ns = torch.randn(R, n, 82, generator=g) * 0.3
    ac = torch.rand(R, n, 4, generator=g) * 0.8
    rw = torch.rand(R, n, generator=g) * 5
    w = (torch.rand(R, generator=g) < 0.7).float()
    w[:3] = 0
    w[3] = 1
    z = torch.randn(2 * R, 4, generator=g) * 2
    return tuple(t.to(device) for t in (st, ac, ns, rw, w, z))


def _make(td3, hidden, device=DEV, seed=7, **kw):
    from kinovagrasping_amd.ddpgfd import DDPGfD, TD3fD
    torch.manual_seed(seed)
    return (TD3fD if td3 else DDPGfD)(82, 4, 0.8, 5, hidden=hidden, device=device, **kw)


def _nets(td3):
    return ("actor", "critic", "actor_target", "critic_target") + (("critic2", "critic2_target") if td3 else ())


def _double(p, td3):
    for name in _nets(td3):
        getattr(p, name).double()
    p._disc = p._disc.double()
    # (module.double() re-creates the parameters' storage: the flat buffers of the soft update must be the new parameters again)
    from kinovagrasping_amd.ddpgfd import _flatten_parameters
    for name in _nets(td3):
        p._flat_params[name] = _flatten_parameters(getattr(p, name))
    return p


def _check_form(nat, hidden, lean):
    if hidden in ((64, 64), (256, 256)):
        assert nat.lds_free and not nat.lean_kernels
    elif lean:
        assert nat.lds_free and nat.lean_kernels
    else:
        assert not nat.lds_free and not nat.lean_kernels


def _compare(native, t32, t64, what):
    """tests/test_gpu_td3_learner.py's criterion: per tensor the native error is at most 4 x that of fp32 torch autograd on the same data,
    or 1e-6 of the tensor's largest entry"""
    for k, (a, b, c) in enumerate(zip(native, t32, t64)):
        a, b, c = a.double(), b.double(), c.double()
        e_nat, e_32 = (a - c).abs().max().item(), (b - c).abs().max().item()
        print(f"{what}[{k}]: native error {e_nat:.3g}, fp32 autograd error {e_32:.3g}, largest entry {c.abs().max().item():.3g}")
        assert e_nat <= max(4 * e_32, 1e-6 * c.abs().max().item()), (what, k, e_nat, e_32, c.abs().max().item())


def _branches(p64, st, ac, ns, rw, z, td3):
    """from the float64 policy: is the bootstrap clamped on both sides and left alone somewhere, are both Huber branches taken?"""
    with torch.no_grad():
        R = rw.shape[0]
        nx = torch.cat([ns[:, 0], ns[:, -1]], 0)
        a = p64.actor_target(nx)
        if td3:
            a = (a + (p64.policy_noise * z).clamp(-p64.noise_clip, p64.noise_clip)).clamp(0, p64.max_action)
            tq = torch.min(p64.critic_target(nx, a), p64.critic2_target(nx, a))
        else:
            tq = p64.critic_target(nx, a)
        lo, hi = p64.q_bounds
        b = tq.clamp(lo, hi)
        e1 = p64.critic(st[:, 0], ac[:, 0]) - (rw[:, :1] + p64.discount * b[:R])
    return (tq < lo).any().item() and (tq > hi).any().item() and ((tq > lo) & (tq < hi)).any().item(), \
        (e1.abs() > p64.huber_delta).any().item() and (e1.abs() < p64.huber_delta).any().item()


KINK = 2e-6


def _kink_rows(p64, st, ac, td3):
    """The batch rows on which a ReLU input of the update is within KINK of 0, from the float64 policy: the critics' two hidden layers on
    the critic phase's rows (p64.critic / critic2 as they are when this is called) and, on all n rows of the actor phase, the actor's
    and critic 1's.  A ReLU whose input is within float32's rounding of 0 (about 1e-7 for these inputs of order 1) is on in one
    evaluation and off in another, and one such unit moves a weight gradient by 1e-4; the criterion of _compare is about arithmetic, not
    about which side of a kink a float32 sum lands on.  Such rows get weight 0 in all three evaluations (padding, as the sampler's)."""
    near = lambda z: z.abs().min(-1).values < KINK
    with torch.no_grad():
        x = torch.cat([st[:, 0], ac[:, 0]], -1)
        rows_c = torch.zeros(st.shape[0], dtype=torch.bool, device=st.device)
        for c in (p64.critic,) + ((p64.critic2,) if td3 else ()):
            z1 = c.l1(x)
            rows_c |= near(z1) | near(c.l2(torch.relu(z1)))
        a1 = p64.actor.l1(st)
        a2 = p64.actor.l2(torch.relu(a1))
        z1 = p64.critic.l1(torch.cat([st, p64.actor(st)], -1))
        rows_a = (near(a1) | near(a2) | near(z1) | near(p64.critic.l2(torch.relu(z1)))).any(1)
    return rows_c, rows_a


def _sync(pol, nat, td3, k):
    """pol (an autograd policy of either precision) takes the native learner's state after k updates: every network, and in its
    optimizers the native Adam moments and step counts (the delayed actor's: k // policy_freq)"""
    for name in _nets(td3):
        pol._flat_params[name].copy_(nat.p._flat_params[name])
    pol.total_it = k
    for name in ("actor", "critic") + (("critic2",) if td3 else ()):
        net, opt = getattr(nat, name), getattr(pol, name + "_optimizer")
        step = k // pol.policy_freq if (td3 and name == "actor") else k
        opt.state.clear()
        off = 0
        for q in opt.param_groups[0]["params"]:
            n = q.numel()
            if step > 0:
                opt.state[q] = {"step": torch.tensor(float(step)), "exp_avg": net.exp_avg[off:off + n].view_as(q).to(q.dtype).clone(),
                                "exp_avg_sq": net.exp_avg_sq[off:off + n].view_as(q).to(q.dtype).clone()}
            off += n


class _NoStep:
    def step(self):
        pass

    def zero_grad(self):
        pass


def _checked_update(nat, p32, p64, k, batch, td3):
    """Update k + 1 of the native learner, checked in full.  Both autograd policies start from the native state after k updates (_sync)
    and run their own phase_critic and phase_actor on the same rows:
      * the critic losses, every critic's gradient and the actor's gradient against float64 autograd by the criterion of _compare;
      * every network's clipped Adam step on its own: (norm, coef) in native.clip against bounded_ref on the native gradient, and the
        moved parameters and moments against bounded_ref.adam_clipped_ref - which tests/test_bounded_reference_cpu.py holds to
        clip_grad_norm_ + Adam.step() of these policies - on the native gradient, old parameters and old moments, with the hyper-
        parameters read from the POLICY's optimizers, the step number counted here and coef from the exact norm, within
        clipped_adam_bounds of tests/test_gpu_bounded_kernels.py (adam_bounds, E_POWF included, + the coefficient's roundings).  TD3fD's
        actor is untouched in every bit on the odd updates.
    A single step from a shared state: Adam's float32 scalar factors do not accumulate, and an element whose gradient is a cancelled
    sum is stepped from the SAME gradient on both sides.
    The rows within KINK of a ReLU kink (_kink_rows) are padding: the critic phase's from the state the update starts in, the actor
    phase's from the critics as the float64 policy steps them.  For the actor phase both autograd policies take the native critics as
    stepped, as tests/test_gpu_td3_learner.py does: kr_adam_step's powf may be an ulp off, which docs/kernels.md allows as
    E_POWF U / (2 bc2) - 1e-5 of the second step - and a critic that moves fast carries that into dQ/da (measured: 3e-6 of the actor's
    gradient at update 2 at 256-256 and 400-300).
    Returns what the callers assert on."""
    from tests import bounded_ref as br
    from tests.test_gpu_bounded_kernels import clipped_adam_bounds
    from tests.test_gpu_glue_kernels import SECOND, U, check_bound
    st, ac, ns, rw, w0, z = batch
    d = lambda t: t.double()
    e32, e64 = ((z,), (d(z),)) if td3 else ((), ())
    grads = lambda m: [q.grad.clone() for q in m.parameters()]
    nat_grads = lambda net: [t for pair in zip(net.gW, net.gb) for t in pair]
    critics = ("critic", "critic2") if td3 else ("critic",)
    opt_nets = ("actor",) + critics
    old = {name: tuple(t.cpu().numpy().copy() for t in (getattr(nat, name).flat, getattr(nat, name).exp_avg, getattr(nat, name).exp_avg_sq)) for name in opt_nets}
    # critic phase: the rows near a kink of the critics as they stand are padding (w_c) for all three
    _sync(p64, nat, td3, k)
    _sync(p32, nat, td3, k)
    rows_c = _kink_rows(p64, d(st), d(ac), td3)[0]
    w_c = torch.where(rows_c, torch.zeros_like(w0), w0)
    l64 = p64.phase_critic(d(st), d(ac), d(ns), d(rw), d(w_c), *e64)
    c64 = {name: grads(getattr(p64, name)) for name in critics}
    l32 = p32.phase_critic(st, ac, ns, rw, w_c, *e32)
    c32 = {name: grads(getattr(p32, name)) for name in critics}
    ln = nat.phase_critic(st, ac, ns, rw, w_c, **(dict(target_noise=z) if td3 else {}))
    # actor phase: its rows near a kink are known only behind the critics' steps, which depend on w_c alone.  The float64 policy's own
    # clipped steps show them (the native steps differ from those by Adam's float32 scalar factors: 1e-5 of a step, far inside KINK);
    # the native phase takes its row weights from the prologue's dq_actor, which is rewritten here as the prologue forms it, for w_a.
    p64.phase_actor(d(st), d(w_c))
    rows_a = _kink_rows(p64, d(st), d(ac), td3)[1]
    w_a = torch.where(rows_a, torch.zeros_like(w_c), w_c)
    masked = (rows_c | rows_a) & (w0 > 0)
    assert w_a.sum() > 0.5 * w0.sum(), (int(masked.sum()), "rows near a kink")
    n = st.shape[1]
    nat.dq_actor.copy_((w_a * (-1.0 / (w_a.sum().clamp_min(1.0) * float(n)))).repeat_interleave(n).view_as(nat.dq_actor))
    nat.phase_actor(st, w_a)
    # ... and the autograd policies take the native critics as stepped (their own steps are checked below, on their own)
    keep = {}
    for pol in (p32, p64):
        for name in critics:
            pol._flat_params[name].copy_(getattr(nat, name).flat)
            keep[pol, name] = getattr(pol, name + "_optimizer")
            setattr(pol, name + "_optimizer", _NoStep())
    p64.phase_actor(d(st), d(w_a))
    a64 = grads(p64.actor)
    p32.phase_actor(st, w_a)
    a32 = grads(p32.actor)
    for (pol, name), opt in keep.items():
        setattr(pol, name + "_optimizer", opt)
    nat.phase_targets()
    torch.cuda.synchronize()
    one = lambda ls: [x.reshape(1) for x in ls]
    assert len(ln) == (6 if td3 else 3)
    _compare(one(ln), one(l32), one(l64), f"update {k + 1}: critic losses")
    for name in critics:
        _compare(nat_grads(getattr(nat, name)), c32[name], c64[name], f"update {k + 1}: {name} gradient")
    _compare(nat_grads(nat.actor), a32, a64, f"update {k + 1}: actor gradient")
    # the clipped Adam steps, each on the native gradient
    f32r = lambda x: float(np.float32(x))
    G = f32r(nat.p.max_grad_norm)
    clip = nat.clip.cpu().numpy()
    info = dict(masked=int(masked.sum()), norms64={}, coefs={}, l1=l64[1].item())
    for slot, name in enumerate(opt_nets):
        net, group = getattr(nat, name), getattr(nat.p, name + "_optimizer").param_groups[0]
        lr, b1, b2, eps, wd = f32r(group["lr"]), f32r(group["betas"][0]), f32r(group["betas"][1]), f32r(group["eps"]), f32r(group["weight_decay"])
        g = net.grad.cpu().numpy()
        p0, m0, v0 = old[name]
        new = tuple(t.cpu().numpy() for t in (net.flat, net.exp_avg, net.exp_avg_sq))
        sq = br.sqnorm_ref(g)
        norm64 = float(np.sqrt(sq))
        coef64 = min(G / (norm64 + 1e-6), 1.0)
        assert abs(float(clip[slot, 0]) - norm64) <= 2 * U * norm64 * SECOND and abs(float(clip[slot, 1]) - coef64) <= 4 * U * coef64 * SECOND, (name, clip[slot])
        info["coefs"][name] = coef64
        every = nat.p.policy_freq if (td3 and name == "actor") else 1
        if (k + 1) % every != 0:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(new, old[name])), f"update {k + 1}: the delayed actor moved"
            continue
        step = (k + 1) // every
        (p1, m1, v1), (delta, bd, bm, bv) = clipped_adam_bounds(p0, g, m0, v0, step, coef64, lr, b1, b2, eps, wd)
        ref = br.adam_clipped_ref(p0, g, m0, v0, k + 1, every, coef64, lr, b1, b2, eps, wd)
        assert np.array_equal(ref[0], p1) and np.array_equal(ref[1], m1) and np.array_equal(ref[2], v1)
        case = f"update {k + 1} {name} coef {coef64:.4f}"
        check_bound(new[1], m1, bm, "learner kr_adam_step_clipped", case, "exp_avg")
        check_bound(new[2], v1, bv, "learner kr_adam_step_clipped", case, "exp_avg_sq")
        check_bound(new[0].astype(np.float64) - p0.astype(np.float64), delta, bd, "learner kr_adam_step_clipped", case, "param step")
        assert not np.array_equal(new[0], p0)
    for name in critics:
        info["norms64"][name] = torch.cat([g.reshape(-1) for g in c64[name]]).norm().item()
    info["norms64"]["actor"] = torch.cat([g.reshape(-1) for g in a64]).norm().item()
    return info


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS, ids=FORM_IDS)
def test_one_bounded_update_against_fp64_autograd(hidden, lean, td3):
    """The first update, by _checked_update: losses, every gradient and every clipped step.  The inputs take every branch (asserted from
    the float64 policy): the bootstrap is clamped on both sides and left alone, both Huber branches occur, the critics' coefficient is
    below 1 and the actor's is clamped to 1; native.clip's norms are those of the float64 gradients."""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    p32, pn, p64 = (_make(td3, hidden, **OPTS) for _ in range(3))
    _double(p64, td3)
    nat = NativeDDPGfDUpdate(pn, lean=lean)
    _check_form(nat, hidden, lean)
    assert nat.bounded and nat.max_grad_norm == 0.5 and nat.td3 == td3
    batch = _batch()
    st, ac, ns, rw, w, z = batch
    clamped, both = _branches(p64, st.double(), ac.double(), ns.double(), rw.double(), z.double(), td3)
    assert clamped and both
    info = _checked_update(nat, p32, p64, 0, batch, td3)
    clip = nat.clip.tolist()
    for slot, name in enumerate(("actor", "critic") + (("critic2",) if td3 else ())):
        n64 = info["norms64"][name]
        assert abs(clip[slot][0] - n64) <= 1e-4 * n64, (name, clip[slot], n64)          # (fp32 gradients: their own error is far below 1e-4)
        assert (0 < n64 < 0.5 and clip[slot][1] == 1.0) if name == "actor" else (n64 > 0.5 and clip[slot][1] < 1.0), (name, clip[slot], n64)
    assert int(nat.it.item()) == 1 and pn.total_it == 1


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS, ids=FORM_IDS)
def test_ten_bounded_updates_against_fp64_autograd(hidden, lean, td3):
    """Ten consecutive native updates on ten batches, each by _checked_update from the native state it starts in: losses, the critics' and
    the actor's gradients - formed from the clipped, Huber-shaped dq at step counts 1 to 10 - and every network's clipped Adam step with
    coef < 1 (the critics' throughout, the actor's where its norm has grown past max_grad_norm), the delayed actor's gate on the odd
    updates.  The critic learns on the way (its loss falls), so the share of clamped rows and of rows on the Huber branch changes; the
    targets move at the tenth update.
    Why from the native state each time: on free trajectories kr_adam_step's float32 scalar factors (betas, powf, the bias corrections;
    docs/kernels.md allows them E_POWF U / bc1 + E_POWF U / (2 bc2) on a step) and torch's Python floats make the steps differ by
    about 1e-6 of their size, the critic's output moves by several units in its first updates, and from the third update on the native
    loss of a free trajectory is 1.0e-6 to 1.4e-6 of its value from the float64 one (measured on an MI355X at 256-256 and 400-300:
    3.7e-6 to 4.2e-6 on losses of 2.9 to 3.6; fp32 autograd: 5e-10 to 4e-7).  The step itself is held to the bound that allows for
    exactly that (clipped_adam_bounds), on the native gradient."""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    p32, pn, p64 = (_make(td3, hidden, **OPTS) for _ in range(3))
    _double(p64, td3)
    nat = NativeDDPGfDUpdate(pn, lean=lean)
    _check_form(nat, hidden, lean)
    infos = []
    for k in range(10):
        target_before = pn._flat_params["critic_target"].clone()
        infos.append(_checked_update(nat, p32, p64, k, _batch(seed=100 + k), td3))
        assert torch.equal(target_before, pn._flat_params["critic_target"]) == (k < 9)
    critics = ("critic", "critic2") if td3 else ("critic",)
    assert all(i["coefs"][name] < 1.0 for i in infos for name in critics)
    l1 = [i["l1"] for i in infos]
    assert l1[-1] < 0.9 * l1[0], l1                      # the critic has learnt: the ten states are not one state ten times
    print("rows masked near a kink per update:", [i["masked"] for i in infos], "actor coef:", ["%.3f" % i["coefs"]["actor"] for i in infos])
    assert int(nat.it.item()) == 10 and pn.total_it == 10


def _state(nat):
    out = {k: v.clone() for k, v in nat.p._flat_params.items()}
    for name in ("actor", "critic") + (("critic2",) if nat.td3 else ()):
        net = getattr(nat, name)
        out[name + ".grad"], out[name + ".exp_avg"], out[name + ".exp_avg_sq"] = net.grad.clone(), net.exp_avg.clone(), net.exp_avg_sq.clone()
    out["losses"] = nat.losses.clone()
    return out


class _Recorder:
    """the library handle of a NativeDDPGfDUpdate, counting the kr_* entry points it is asked for"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS[:3], ids=FORM_IDS[:3])
def test_the_infinite_settings_are_the_unset_update_in_every_bit(hidden, lean, td3):
    """5 native updates with q_bounds = (-inf, inf), huber_delta = inf, max_grad_norm = inf against 5 with None, None, None (TD3fD: the
    smoothing on its in-kernel stream), on the hand-written kernels, whose results do not depend on the schedule: networks, targets,
    gradients, moments and losses equal in every bit, through the new kernels on one side and without a single launch of them on the
    other"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    a = NativeDDPGfDUpdate(_make(td3, hidden), lean=lean)
    b = NativeDDPGfDUpdate(_make(td3, hidden, q_bounds=(-INF, INF), huber_delta=INF, max_grad_norm=INF), lean=lean)
    _check_form(b, hidden, lean)
    a.lib, b.lib = _Recorder(a.lib), _Recorder(b.lib)
    ca, cb = a.lib.calls, b.lib.calls
    assert not a.bounded and a.max_grad_norm is None and b.bounded and b.max_grad_norm == INF
    for it in range(5):
        st, ac, ns, rw, w, _ = _batch(seed=20 + it)
        a.train_on_batch(st, ac, ns, rw, w)
        b.train_on_batch(st, ac, ns, rw, w)
    torch.cuda.synchronize()
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (k, (sa[k] - sb[k]).abs().max().item())
    assert torch.isfinite(sa["losses"]).all() and not a.clip.any() and (b.clip[:3 if td3 else 2, 1] == 1.0).all()
    # the launch sequences: the unset policy issues no new kernel, the set one none of those they replace
    assert not any(k in ca for k in NEW) and all(k in cb for k in NEW) and not any(k in cb for k in OLD)
    nets = 3 if td3 else 2
    assert cb["kr_critic_grad_bounded"] == 5 and cb["kr_grad_sqnorm"] == cb["kr_adam_step_clipped"] == 5 * nets
    assert ca["kr_twin_critic_grad" if td3 else "kr_critic_grad"] == 5 and ca["kr_adam_step"] + ca.get("kr_adam_step_every", 0) == 5 * nets
    for k in set(ca) - set(OLD):
        assert ca[k] == cb[k], k


def test_each_option_alone_takes_its_own_launches():
    """q_bounds or huber_delta alone: the bounded loss-gradient launch and the plain Adam steps; max_grad_norm alone: the reverse"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    st, ac, ns, rw, w, _ = _batch(seed=3)
    for kw, want, never in ((dict(q_bounds=(0.0, 50.0)), ("kr_critic_grad_bounded", "kr_adam_step"), ("kr_critic_grad", "kr_grad_sqnorm", "kr_adam_step_clipped")),
                            (dict(huber_delta=10.0), ("kr_critic_grad_bounded", "kr_adam_step"), ("kr_critic_grad", "kr_grad_sqnorm", "kr_adam_step_clipped")),
                            (dict(max_grad_norm=10.0), ("kr_critic_grad", "kr_grad_sqnorm", "kr_adam_step_clipped"), ("kr_critic_grad_bounded", "kr_adam_step"))):
        nat = NativeDDPGfDUpdate(_make(False, (64, 64), **kw))
        nat.lib = _Recorder(nat.lib)
        nat.train_on_batch(st, ac, ns, rw, w)
        torch.cuda.synchronize()
        calls = nat.lib.calls
        assert all(k in calls for k in want) and not any(k in calls for k in never), (kw, calls)
        assert torch.isfinite(nat.losses).all()


@pytest.mark.parametrize("kw", [dict(q_bounds=(0.0, 50.0)), dict(huber_delta=10.0), dict(max_grad_norm=10.0)], ids=["q_bounds", "huber_delta", "max_grad_norm"])
def test_the_fork_form_refuses_a_bounded_policy(monkeypatch, kw):
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    monkeypatch.setenv("KS_LEARNER_FORK", "1")
    with pytest.raises(ValueError):
        NativeDDPGfDUpdate(_make(False, (256, 256), **kw))


@pytest.mark.parametrize("form", ["eager", "pipelined"])
def test_the_delayed_actor_reports_its_norm_on_every_update(form):
    """TD3fD with policy_freq = 2 and the options set: the actor's (norm, coef) is written on every update - the clipped step's gate is
    closed on the odd ones, clip_out is not - and its parameters move on the even updates only"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    pol = _make(True, (64, 64), seed=5, policy_freq=2, **OPTS)
    nat = NativeDDPGfDUpdate(pol)
    nat.pipelined = form == "pipelined"
    moved, reported = [], []
    for k in range(1, 5):
        st, ac, ns, rw, w, _ = _batch(seed=40 + k)
        before = nat.actor.flat.clone()
        nat.clip.zero_()
        if form == "eager":
            nat.train_on_batch(st, ac, ns, rw, w)
        else:
            nat.phase_critic(st, ac, ns, rw, w)
            nat.phase_actor(st, w)
            nat.phase_head()                          # (the next update's head, which applies this update's actor step)
        torch.cuda.synchronize()
        moved.append(not torch.equal(before, nat.actor.flat))
        reported.append(nat.clip[0].tolist())
    assert moved == [False, True, False, True], moved
    assert all(norm > 0 and 0 < coef <= 1 for norm, coef in reported), reported


# ---- the trainers ------------------------------------------------------------------------------------------------------------------------
def _setup(td3, n=64, horizon=12, **opts):
    from kinovagrasping_amd import scenarios
    from kinovagrasping_amd.ddpgfd import DDPGfD, TD3fD
    from kinovagrasping_amd.multi_shape import MultiShapeSim
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from kinovagrasping_amd.rollout import RolloutEngine
    rng = np.random.RandomState(4)
    sim = MultiShapeSim(n, ["CubeS"], device=0, auto_reset=True, horizon=horizon)
    qp, hqp, _ = scenarios.draw_start_pool(["CubeS"] * n, "normal", 4, rng)
    sim.reset(torch.as_tensor(qp[0]), torch.as_tensor(hqp[0]), object_id=sim.shape_of_env)
    obs0 = sim.set_start_pool(torch.as_tensor(qp), torch.as_tensor(hqp), seed=2)
    torch.manual_seed(2)
    policy = (TD3fD if td3 else DDPGfD)(82, 4, 0.8, 5, batch_size=8, hidden=(64, 64), device=sim.device, **opts)
    replay = DeviceEpisodeReplay(n, capacity=8 * n, horizon=horizon, device=sim.device)
    eng = RolloutEngine(sim, policy, replay, expl_noise=0.1)
    eng.start(obs0)
    return sim, policy, replay, eng


# (on the trainers' rewards - at most a few units per episode - these settings bite: a tight range, a small delta, a small norm)
TRAINER_OPTS = dict(q_bounds=(-0.01, 0.01), huber_delta=0.05, max_grad_norm=0.05)


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
def test_graphed_trainer_captured_equals_eager_in_every_bit(td3):
    """GraphedTrainer on 64 envs with the options set, a filled ring that no longer changes: 5 updates replayed from the captured graphs
    and, from the same learner state, 5 eager ones (the sampler is keyed by the update count in both) - networks, moments, losses and
    native.clip equal in every bit"""
    from kinovagrasping_amd.pipeline import GraphedTrainer
    sim, policy, replay, eng = _setup(td3, **TRAINER_OPTS)
    tr = GraphedTrainer(sim, policy, replay, eng, batch_episodes=8, overlap=False)
    nat = tr.native
    assert nat.bounded and nat.max_grad_norm == 0.05 and nat.pipelined
    for _ in range(26):
        eng.step()
    tr.capture()
    torch.cuda.synchronize()
    assert replay.count >= 2 * 64
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
        nat.clip.zero_()

    def snapshot():
        nat.finish_pending()
        torch.cuda.synchronize()
        out = _state(nat)
        out["clip"], out["it"] = nat.clip.clone(), nat.it.clone()
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
    assert not torch.equal(graphed["critic"], saved[0]["critic"]) and not torch.equal(graphed["actor"], saved[0]["actor"])
    assert (graphed["clip"][:3 if td3 else 2, 0] > 0).all() and (graphed["clip"][:3 if td3 else 2, 1] <= 1.0).all()
    sim.close()


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
def test_priorities_come_from_the_bootstrap_the_update_used(td3):
    """GraphedTrainer(prioritized=True) with q_bounds set, one eager update on a filled ring: the callback receives q and tboot [2R] - inside
    the bounds, on both of them somewhere - and per_delta is tests/priority_ref.py's delta on exactly those in every bit"""
    from kinovagrasping_amd.pipeline import GraphedTrainer
    sim, policy, replay, eng = _setup(td3, **TRAINER_OPTS)
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
    lo, hi = np.float32(-0.01), np.float32(0.01)
    assert (host["tq1"] >= lo).all() and (host["tq1"] <= hi).all() and ((host["tq1"] == lo) | (host["tq1"] == hi)).any()
    ref = pr.episode_deltas_ref(B, W, n, host["q"], host["tq1"][:R], host["reward"], host["weight"], policy.discount)
    got = tr.per_delta.cpu().numpy()
    assert np.isfinite(got).all() and (got >= 0).all() and got.tobytes() == ref.tobytes(), (got, ref)
    sim.close()


def test_async_trainer_trains_a_bounded_policy():
    """the free-running form on 64 envs, one launch of 13 env-steps with captured graphs: it runs, drops nothing, and native.clip is finite"""
    from kinovagrasping_amd.pipeline import AsyncTrainer
    sim, policy, replay, eng = _setup(True, **TRAINER_OPTS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=8)
    tr.capture()
    tr.run(13)
    tr.flush(finish_update=True)
    torch.cuda.synchronize()
    nat = tr.native
    c = tr.counts()
    assert tr.updates == 13 and int(nat.it.item()) == 13 and int(nat.it_head.item()) == 0
    assert c["pacing_timeouts"] == 0 and c["episodes_kept"] == replay.count
    assert torch.isfinite(nat.clip).all() and torch.isfinite(nat.losses).all() and (nat.clip[:, 0] >= 0).all()
    sim.close()
