"""Running observation normalisation (ddpgfd: obs_norm; kr_obs_stats_update, kr_obs_normalize, kr_fold_obs_norm) through the native update
(GPU), by the method of tests/test_gpu_bounded_learner.py and tests/test_gpu_bc_learner.py: one and ten updates against float64 autograd
of the same policy in the forms of learner_native (LDS-free, lean, library GEMMs) for DDPGfD and TD3fD, on windows and on episode tables,
the acting copy against the fold kernel after every update, the folded first layer against explicit normalisation, the unset feature as
the update it was in launches and bits, and the settings composed."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import obsnorm_ref as onr
from tests.test_gpu_bc_learner import _table_batch
from tests.test_gpu_bounded_learner import _batch, _check_form, _double, _make, _NoStep, _Recorder, _state, _sync

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FORMS = [((64, 64), None), ((400, 300), True), ((200, 100), None)]          # LDS-free, lean, library GEMMs
FORM_IDS = ["ldsfree-64", "lean-400-300", "library-200-100"]
ON = dict(obs_norm=True)
KINK = 4e-6          # (tests/test_gpu_bounded_learner.py's 2e-6 for inputs of order 0.3; the normalised ones are of order 1 to 3)


def _compare(native, t32, t64, what, floors=None):
    """tests/test_gpu_bounded_learner.py's criterion, the project's: per tensor the native error is at most 4 x that of fp32 torch autograd
    on the same data, or 1e-6 of the tensor's largest entry.  floors (the gradients only): an absolute allowance per tensor, see _sum_floor"""
    for k, (a, b, c) in enumerate(zip(native, t32, t64)):
        a, b, c = a.double(), b.double(), c.double()
        e_nat, e_32 = (a - c).abs().max().item(), (b - c).abs().max().item()
        floor = 0.0 if floors is None else floors[k]
        print(f"{what}[{k}]: native error {e_nat:.3g}, fp32 autograd error {e_32:.3g}, largest entry {c.abs().max().item():.3g}" + (f", floor {floor:.3g}" if floor else ""))
        assert e_nat <= max(4 * e_32, 1e-6 * c.abs().max().item(), floor), (what, k, e_nat, e_32, c.abs().max().item(), floor)


def _sum_floor(terms):
    """A critic's last bias gradient is ONE number, the sum over the R batch rows of dLoss/dQ_r - the weighted mean TD error - and it passes
    through zero while the critic learns, where an error relative to that number alone says nothing about the arithmetic.  Its absolute
    allowance: an fp32 sum of R terms in any order is within (R - 1) 2^-24 sum |terms| of the exact sum, and each term carries one more
    rounding: R 2^-24 sum_r |dLoss/dQ_r|, the terms from the float64 policy."""
    return terms.numel() * 2.0 ** -24 * terms.abs().sum().item()


def _kink_rows(p64, st, ac, td3, kink):
    """tests/test_gpu_bounded_learner.py's _kink_rows with the band as a parameter: the batch rows on which a ReLU input of the update is
    within `kink` of 0 in the float64 policy - the critics' hidden layers on the critic phase's rows, the actor's and critic 1's on all n rows
    of the actor phase"""
    near = lambda z: z.abs().min(-1).values < kink
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


def _scaled(batch):
    """the batch with state columns of very different scale and offset, as the real observation's - what the feature is for"""
    st, ac, ns, rw, w, z = batch
    scale = torch.logspace(-2, 1, 82, device=st.device)
    shift = torch.linspace(-2, 2, 82, device=st.device)
    return st * scale + shift, ac, ns * scale + shift, rw, w, z


def _three(td3, hidden, **kw):
    p32, pn, p64 = (_make(td3, hidden, **kw) for _ in range(3))
    _double(p64, td3)
    p64.refresh_acting()
    return p32, pn, p64


def _sync_all(pol, nat, td3, k):
    _sync(pol, nat, td3, k)
    for dst, src in zip(pol.obs_norm.tensors(), nat.p.obs_norm.tensors()):
        dst.copy_(src)


def _near(p64, st, ac, td3):
    """_kink_rows on the states as p64 normalises them now, at this file's KINK"""
    return _kink_rows(p64, p64._norm(st), ac, td3, KINK)


def _critic_mask(p64, st, ac, w0, k, td3):
    """The critic phase's rows near a ReLU kink are padding - and padding rows do not enter the statistics, which moves the normalised
    states: the mask grows until the statistics it gives leave no unmasked row near a kink (p64's statistics are put back)."""
    saved = [t.clone() for t in p64.obs_norm.tensors()]
    rows = torch.zeros_like(w0, dtype=torch.bool)
    for _ in range(8):
        for t, v in zip(p64.obs_norm.tensors(), saved):
            t.copy_(v)
        p64.obs_norm.update(st[:, 0], torch.where(rows, torch.zeros_like(w0), w0).double(), k)
        new = _near(p64, st, ac, td3)[0] & ~rows
        rows |= new
        if not new.any():
            break
    else:
        raise AssertionError("the kink mask did not settle")
    for t, v in zip(p64.obs_norm.tensors(), saved):
        t.copy_(v)
    return rows


def _fold_kernel(pol):
    """kr_fold_obs_norm on the policy's actor and statistics as they are -> (W1_out, b1_out)"""
    from kinovagrasping_amd import sim as ks
    w, b, on = pol.actor.l1.weight.data, pol.actor.l1.bias.data, pol.obs_norm
    wo, bo = torch.empty_like(w), torch.empty_like(b)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = ks.load_library().kr_fold_obs_norm(w.shape[0], w.shape[1], on.dim, P(w), P(b), P(on.mean32), P(on.inv32), P(wo), P(bo),
                                            ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0
    return wo, bo


def _acting_is_the_fold(pol, what):
    wo, bo = _fold_kernel(pol)
    torch.cuda.synchronize()
    (w1, b1), (w2, b2), (w3, b3) = pol.acting_layers()
    a = pol.actor
    assert torch.equal(w1, wo) and torch.equal(b1, bo), what
    assert all(torch.equal(x, y.data) for x, y in ((w2, a.l2.weight), (b2, a.l2.bias), (w3, a.l3.weight), (b3, a.l3.bias))), what
    n1 = w1.numel() + b1.numel()
    assert torch.equal(pol.acting_flat()[n1:], pol._flat_params["actor"][n1:])


def _checked_update(nats, p32, p64, k, batch, td3):
    """Update k + 1 of every native learner of `nats` - pairs (learner, TableBatch or None for the window form), all in the same state.  Both
    autograd policies start from the native state after k updates, statistics included, and run their own phases on the same raw rows; the
    rows near a ReLU kink of the float64 policy are padding in all evaluations (the critic phase's settle with the statistics, _critic_mask;
    the actor phase's are known behind the critics' steps, and the native prologue's outputs are rewritten for them as the prologue forms
    them, as tests/test_gpu_bc_learner.py does); for the actor phase both autograd policies take the native critics as stepped.
    Compared by _compare: the statistics, the critic losses, every critic's stepped parameters, and behind phase_targets the actor and every
    target network - each network's flat parameter buffer - and, beyond that, every gradient tensor of the trained networks (the critics'
    one-element last bias gradient with the absolute allowance of _sum_floor)."""
    st, ac, ns, rw, w0, z = batch
    d = lambda t: t.double()
    e32, e64 = ((z,), (d(z),)) if td3 else ((), ())
    n = st.shape[1]
    grads = lambda m: [q.grad.clone() for q in m.parameters()]
    nat_grads = lambda net: [t for pair in zip(net.gW, net.gb) for t in pair]
    critics = ("critic", "critic2") if td3 else ("critic",)
    first = nats[0][0]
    for pol in (p32, p64):
        _sync_all(pol, first, td3, k)
    rows_c = _critic_mask(p64, d(st), d(ac), w0, k, td3)
    w_c = torch.where(rows_c, torch.zeros_like(w0), w0)
    dq64, hooks = {}, []
    for name in critics:             # dLoss/dQ per row of each critic, for _sum_floor: its last layer's output keeps its gradient
        def keep_grad(module, inputs, out, name=name):
            out.retain_grad()
            dq64[name] = out
        hooks.append(getattr(p64, name).l3.register_forward_hook(keep_grad))
    l64 = p64.phase_critic(d(st), d(ac), d(ns), d(rw), d(w_c), *e64)
    for h in hooks:
        h.remove()
    floors = {name: [0.0] * 5 + [_sum_floor(dq64[name].grad)] for name in critics}
    c64 = {name: grads(getattr(p64, name)) for name in critics}
    l32 = p32.phase_critic(st, ac, ns, rw, w_c, *e32)
    c32 = {name: grads(getattr(p32, name)) for name in critics}
    assert not _near(p64, d(st), d(ac), td3)[0][w_c > 0].any()
    states, lns = [], []
    for nat, tb in nats:
        if tb is None:
            s_n = st.clone()                           # (normalised in place; the actor phase takes the same buffer)
            lns.append(nat.phase_critic(s_n, ac, ns.clone(), rw, w_c, **(dict(target_noise=z) if td3 else {})))
        else:
            tb = tb._replace(weight=w_c, **{f: getattr(tb, f).clone() for f in ("table_state", "table_next", "state0", "next_ends")})
            s_n = tb
            lns.append(nat.phase_critic_tables(tb, target_noise=z if td3 else None))
        states.append(s_n)
    # the autograd policies' own critic steps: compared with the native ones, and they show the actor phase's rows near a kink
    p64.phase_actor(d(st), d(w_c))
    p32.phase_actor(st, w_c)
    step64 = {name: p64._flat_params[name].clone() for name in critics}
    step32 = {name: p32._flat_params[name].clone() for name in critics}
    rows_a = _near(p64, d(st), d(ac), td3)[1]
    w_a = torch.where(rows_a, torch.zeros_like(w_c), w_c)
    assert w_a.sum() > 0.5 * w0.sum(), (int(rows_c.sum()), int(rows_a.sum()))
    wsum = w_a.sum().clamp_min(1.0)
    scale = -1.0 / (wsum * float(n))
    for (nat, _), s_n in zip(nats, states):
        nat.weight = w_a
        nat.wsum.copy_(wsum.view(1))
        if isinstance(s_n, torch.Tensor):
            nat.dq_actor.copy_((w_a * scale).repeat_interleave(n).view_as(nat.dq_actor))
            nat.phase_actor(s_n, w_a)
        else:
            nat.dq_table.copy_((s_n.slot_weight * scale).repeat_interleave(s_n.horizon).view_as(nat.dq_table))
            idx = s_n.row_table.long().unsqueeze(1) + torch.arange(n, device=DEV)
            idx[w_a == 0] = -1
            nat.row_index.copy_(idx.reshape(-1).int())
            nat.phase_actor_tables(s_n)
    keep = {}
    for pol in (p32, p64):
        for name in critics:
            pol._flat_params[name].copy_(getattr(first, name).flat)
            keep[pol, name] = getattr(pol, name + "_optimizer")
            setattr(pol, name + "_optimizer", _NoStep())
    p64.phase_actor(d(st), d(w_a))
    a64 = grads(p64.actor)
    p32.phase_actor(st, w_a)
    a32 = grads(p32.actor)
    for (pol, name), opt in keep.items():
        setattr(pol, name + "_optimizer", opt)
    p64.phase_targets()
    p32.phase_targets()
    for nat, _ in nats:
        nat.phase_targets()
    torch.cuda.synchronize()
    one = lambda ls: [x.reshape(1) for x in ls]
    stats = lambda pol: list(pol.obs_norm.tensors())
    for (nat, tb), ln in zip(nats, lns):
        form = f"update {k + 1} ({'tables' if tb is not None else 'windows'})"
        assert float(nat.p.obs_norm.count[0]) == float(p64.obs_norm.count[0]) == float(first.p.obs_norm.count[0])
        _compare(stats(nat.p), stats(p32), stats(p64), f"{form}: statistics")
        _compare(one(ln), one(l32), one(l64), f"{form}: critic losses")
        for name in critics:
            _compare(nat_grads(getattr(nat, name)), c32[name], c64[name], f"{form}: {name} gradient", floors[name])
            _compare([getattr(nat, name).flat], [step32[name]], [step64[name]], f"{form}: {name} stepped")
        _compare(nat_grads(nat.actor), a32, a64, f"{form}: actor gradient")
        names = ("actor", "actor_target") + tuple(c + "_target" for c in critics)
        _compare([nat.p._flat_params[x] for x in names], [p32._flat_params[x] for x in names], [p64._flat_params[x] for x in names], f"{form}: {names}")
        _acting_is_the_fold(nat.p, form)
    return dict(masked=int(((rows_c | rows_a) & (w0 > 0)).sum()), count=float(first.p.obs_norm.count[0]), counted=int((w_c != 0).sum()))


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS, ids=FORM_IDS)
def test_one_update_on_windows_against_fp64_autograd(hidden, lean, td3):
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    p32, pn, p64 = _three(td3, hidden, **ON)
    nat = NativeDDPGfDUpdate(pn, lean=lean)
    _check_form(nat, hidden, lean)
    assert nat.obs_norm is pn.obs_norm and torch.equal(pn.acting_flat(), pn._flat_params["actor"])
    info = _checked_update([(nat, None)], p32, p64, 0, _scaled(_batch(seed=19)), td3)
    print("window form:", info)
    assert info["count"] == info["counted"] > 100 and int(nat.it.item()) == 1 and pn.total_it == 1
    assert not torch.equal(pn.acting_flat(), pn._flat_params["actor"])


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS[:2], ids=FORM_IDS[:2])
def test_one_update_on_tables_against_fp64_autograd_and_the_window_form(hidden, lean, td3):
    """8 episodes of horizon 30 drawn as episode tables (padding rows, an expert tail): against float64 autograd on tb.windows(), and equal to
    the window form on tb.windows() in every bit - every network, gradient, moment, loss, the statistics and the acting copy"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    p32, pn, p64 = _three(td3, hidden, **ON)
    tab, win = NativeDDPGfDUpdate(pn, lean=lean), NativeDDPGfDUpdate(_make(td3, hidden, **ON), lean=lean)
    _check_form(tab, hidden, lean)
    tb = _table_batch()
    scale, shift = torch.logspace(-2, 1, 82, device=DEV), torch.linspace(-2, 2, 82, device=DEV)
    tb = tb._replace(**{f: getattr(tb, f) * scale + shift for f in ("table_state", "table_next", "state0", "next_ends")})
    st, ac, ns, rw, nd, w = tb.windows()
    z = (torch.randn(2 * w.shape[0], 4, generator=torch.Generator().manual_seed(4)) * 2).to(DEV)
    info = _checked_update([(tab, tb), (win, None)], p32, p64, 0, (st, ac, ns, rw, w, z), td3)
    print("table form:", info)
    sa, sb = _state(tab), _state(win)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for x, y in zip(tab.p.obs_norm.tensors() + (tab.p.acting_flat(),), win.p.obs_norm.tensors() + (win.p.acting_flat(),)):
        assert torch.equal(x, y)
    assert tab.actor.grad.abs().max().item() > 0


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS, ids=FORM_IDS)
def test_ten_updates_against_fp64_autograd(hidden, lean, td3):
    """ten consecutive native updates on ten batches, each checked from the native state it starts in; the tenth fires the soft update"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    p32, pn, p64 = _three(td3, hidden, **ON)
    nat = NativeDDPGfDUpdate(pn, lean=lean)
    _check_form(nat, hidden, lean)
    infos = [_checked_update([(nat, None)], p32, p64, k, _scaled(_batch(seed=100 + k)), td3) for k in range(10)]
    print("rows masked per update:", [i["masked"] for i in infos])
    assert infos[-1]["count"] == sum(i["counted"] for i in infos) and int(nat.it.item()) == 10
    assert not torch.equal(pn._flat_params["actor_target"], _make(td3, hidden)._flat_params["actor_target"])


def _scaled_tables(seed):
    tb = _table_batch(seed)
    scale, shift = torch.logspace(-2, 1, 82, device=DEV), torch.linspace(-2, 2, 82, device=DEV)
    return tb._replace(**{f: getattr(tb, f) * scale + shift for f in ("table_state", "table_next", "state0", "next_ends")})


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS[:2], ids=FORM_IDS[:2])
def test_ten_updates_on_tables_against_fp64_autograd_and_the_window_form(hidden, lean, td3):
    """ten consecutive updates on ten table batches, the table learner and a window learner on tb.windows() side by side: each update checked
    from the state it starts in, and after the tenth both learners equal in every bit - networks, gradients, moments, losses, statistics and
    the acting copy"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    p32, pn, p64 = _three(td3, hidden, **ON)
    tab, win = NativeDDPGfDUpdate(pn, lean=lean), NativeDDPGfDUpdate(_make(td3, hidden, **ON), lean=lean)
    infos = []
    for k in range(10):
        tb = _scaled_tables(40 + 2 * k)
        st, ac, ns, rw, nd, w = tb.windows()
        z = (torch.randn(2 * w.shape[0], 4, generator=torch.Generator().manual_seed(4 + k)) * 2).to(DEV)
        infos.append(_checked_update([(tab, tb), (win, None)], p32, p64, k, (st, ac, ns, rw, w, z), td3))
    print("rows masked per update:", [i["masked"] for i in infos])
    sa, sb = _state(tab), _state(win)
    for name in sa:
        assert torch.equal(sa[name], sb[name]), name
    for x, y in zip(tab.p.obs_norm.tensors() + (tab.p.acting_flat(),), win.p.obs_norm.tensors() + (win.p.acting_flat(),)):
        assert torch.equal(x, y)
    assert infos[-1]["count"] == sum(i["counted"] for i in infos) and int(tab.it.item()) == 10


def test_acting_copy_follows_a_delayed_actor_and_a_freeze():
    """TD3fD (the actor steps on every second update) with the statistics frozen after two updates, four whole native updates on tables:
    after each the acting copy is the fold kernel's output for the actor and statistics of that moment in every bit; the statistics move on
    the first two updates only, the acting copy's first layer whenever actor or statistics did"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    pn = _make(True, (64, 64), obs_norm=True, obs_norm_freeze_after=2)
    nat = NativeDDPGfDUpdate(pn)
    tb0 = _table_batch()
    seen = []
    for k in range(4):
        tb = tb0._replace(**{f: getattr(tb0, f) * (1.0 + k) + 0.1 * k for f in ("table_state", "table_next", "state0", "next_ends")})
        raw = tb.state0.clone()
        nat.train_on_tables(tb)
        _acting_is_the_fold(pn, f"update {k + 1}")
        seen.append(tuple(t.clone() for t in pn.obs_norm.tensors() + (pn.acting_flat(), pn._flat_params["actor"])))
        on = pn.obs_norm
        assert torch.equal(tb.state0, (raw - on.mean32) * on.inv32)          # in place, by the statistics as this update left them
    counted = int((tb0.weight != 0).sum())
    assert [float(s[0][0]) for s in seen] == [counted, 2 * counted, 2 * counted, 2 * counted]
    assert not torch.equal(seen[0][1], seen[1][1]) and all(torch.equal(x, y) for x, y in zip(seen[1][:5], seen[2][:5]))
    assert all(torch.equal(x, y) for x, y in zip(seen[1][:5], seen[3][:5]))
    moved = [not torch.equal(seen[k][6], seen[k + 1][6]) for k in range(3)]
    assert moved == [True, False, True], moved                       # the delayed actor: updates 2 and 4
    assert torch.equal(seen[1][5], seen[2][5]) and not torch.equal(seen[2][5], seen[3][5])


def test_folded_first_layer_against_explicit_normalisation():
    """the first-layer pre-activation through the acting copy's fp32 weights (as the rollout kernels form it, here in fp64 from those weights)
    against explicit normalisation evaluated in fp64: within (S + 2) 2^-24 sum_k |W1'_jk| (|x_k| + |mu_k|), error / bound <= 1"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    pn = _make(False, (64, 64), **ON)
    nat = NativeDDPGfDUpdate(pn)
    for k in range(3):
        st, ac, ns, rw, w, _ = _scaled(_batch(seed=50 + k))
        nat.train_on_batch(st, ac, ns, rw, w)
    torch.cuda.synchronize()
    x = _scaled(_batch(seed=60))[0][:, 0].cpu()
    (w1, b1), _, _ = pn.acting_layers()
    on = pn.obs_norm
    folded = (x.double() @ w1.cpu().double().t() + b1.cpu().double()).numpy()
    xn = (x.double() - on.mean32.cpu().double()) * on.inv32.cpu().double()
    explicit = (xn @ pn.actor.l1.weight.data.cpu().double().t() + pn.actor.l1.bias.data.cpu().double()).numpy()
    bound = onr.preactivation_bound(w1.cpu().numpy(), x.numpy(), on.mean32.cpu().numpy())
    ratio = (np.abs(folded - explicit) / bound).max()
    print(f"\nGLUE folded first layer | 200 rows x 64 units | pre-activation | worst err {np.abs(folded - explicit).max():.3e} | worst err/bound {ratio:.3f}")
    assert ratio <= 1
    with torch.no_grad():
        assert (pn.select_action(x.to(DEV)) - pn.actor(on.normalize(x.to(DEV)))).abs().max().item() == 0


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("hidden,lean", FORMS, ids=FORM_IDS)
def test_unset_feature_is_the_update_as_it_was(hidden, lean, td3):
    """three native updates of a policy built with obs_norm=False against a policy built without the arguments: the same launches, entry
    point by entry point, none of the three kernels, every parameter, gradient, moment and loss equal in every bit, and the batch buffers
    untouched; with the feature on the three kernels run 1 + 2 + 1 times per update and nothing else changes in the sequence"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    a = NativeDDPGfDUpdate(_make(td3, hidden), lean=lean)
    b = NativeDDPGfDUpdate(_make(td3, hidden, obs_norm=False), lean=lean)
    c = NativeDDPGfDUpdate(_make(td3, hidden, **ON), lean=lean)
    for nat in (a, b, c):
        nat.lib = _Recorder(nat.lib)
    new = ("kr_obs_stats_update", "kr_obs_normalize", "kr_fold_obs_norm")
    for it in range(3):
        st, ac, ns, rw, w, _ = _batch(seed=20 + it)
        keep = st.clone()
        a.train_on_batch(st, ac, ns, rw, w)
        b.train_on_batch(st, ac, ns, rw, w)
        assert torch.equal(st, keep)
        c.train_on_batch(st.clone(), ac, ns.clone(), rw, w)
    torch.cuda.synchronize()
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert a.lib.calls == b.lib.calls and not any(k in b.lib.calls for k in new)
    assert b.p.obs_norm is None and b.p.acting_flat() is b.p._flat_params["actor"]
    assert [c.lib.calls[k] for k in new] == [3, 6, 3] and {k: v for k, v in c.lib.calls.items() if k not in new} == a.lib.calls
    assert torch.isfinite(_state(c)["actor"]).all() and not torch.equal(_state(c)["actor"], sa["actor"])


def test_the_settings_compose():
    """obs_norm with bc_weight, the Q-filter and q_bounds on one policy, one update on tables in the LDS-free form against the window form in
    every bit and against float64 autograd's losses: the normalised states are what the behaviour-cloning term and the filter's critic see"""
    from kinovagrasping_amd.learner_native import NativeDDPGfDUpdate
    kw = dict(obs_norm=True, bc_weight=2.0, q_filter=True, q_bounds=(-0.5, 0.5), huber_delta=2.0)
    tab, win = NativeDDPGfDUpdate(_make(False, (64, 64), **kw)), NativeDDPGfDUpdate(_make(False, (64, 64), **kw))
    p64 = _double(_make(False, (64, 64), **kw), False)
    p64.refresh_acting()
    tb = _table_batch()
    st, ac, ns, rw, nd, w = tb.windows()
    demo_from = 5 * 25
    for nat in (tab, win):
        nat.track_actor_loss = True
    tab.train_on_tables(tb, demo_from=demo_from)
    lw = win.train_on_batch(st.clone(), ac, ns.clone(), rw, w, demo_from=demo_from)
    l64 = p64.train_on_batch(st.double(), ac.double(), ns.double(), rw.double(), w.double(), demo_from=demo_from)
    torch.cuda.synchronize()
    sa, sb = _state(tab), _state(win)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(tab.p.acting_flat(), win.p.acting_flat()) and torch.equal(tab.bc_loss, win.bc_loss)
    # (a composition check, not a parity one - the parts have theirs: fp32 losses of order 10 over 200 rows agree with float64 to 1e-4, and
    # one of the 75 demonstration rows changing sides of the filter moves the term by 1 / 75 of itself)
    for got, ref in zip(lw, l64[1:]):
        assert abs(got.item() - ref.item()) <= 1e-4 * max(1.0, abs(ref.item())), (got.item(), ref.item())
    assert win.bc_loss.item() > 0 and abs(win.bc_loss.item() - p64.bc_loss.item()) <= 2e-2 * p64.bc_loss.item() + 1e-6
    _acting_is_the_fold(win.p, "composed")


def test_composed_with_prioritized_replay_in_the_trainer():
    """GraphedTrainer(prioritized=True) on 64 envs with obs_norm, bc_weight and q_bounds on the policy and an expert ring.  One eager update:
    the priorities callback receives the Q of the NORMALISED window-first states - the critic as it stands on the batch buffer the update
    normalised in place, and not on those states mapped back to raw -, per_delta is tests/priority_ref.py's delta on exactly the callback's
    operands in every bit, and both rings still hold the raw rows in every bit.  Then the capture: its warm-up updates are undone on the
    priorities and on the statistics alike, and five captured steps train with finite losses and move both."""
    from kinovagrasping_amd.pipeline import GraphedTrainer
    from tests import priority_ref as pr
    from tests.test_gpu_bc_learner import _trainer_setup
    sim, policy, replay, eng, expert = _trainer_setup(False, obs_norm=True, bc_weight=1.0, q_bounds=(-0.01, 0.01))
    tr = GraphedTrainer(sim, policy, replay, eng, batch_episodes=8, overlap=False, learn_after=0, expert_replay=expert, expert_prob=0.3,
                        prioritized=True, per_alpha=0.6, per_beta=0.4, per_eps=1e-3)
    assert tr.tables and tr.native.obs_norm is policy.obs_norm and tr.native.bc_weight == 1.0 and tr.native.bounded
    for _ in range(26):
        eng.step()
    torch.cuda.synchronize()
    assert replay.count >= 2 * 64
    rings = [t for r in (replay, expert) for t in (r.ep_state, r.ep_next)]
    raw = [t.clone() for t in rings]
    seen = {}
    inner = tr._update_priorities

    def record(q, tq1, reward, weight):
        tb, on = tr._tb, policy.obs_norm
        with torch.no_grad():
            seen.update(q=q.clone(), tq1=tq1.clone(), reward=reward.clone(), weight=weight.clone(), count=on.count.clone(),
                        q_norm=policy.critic(tb.state0, tb.action0), q_raw=policy.critic(tb.state0 / on.inv32 + on.mean32, tb.action0),
                        q_64=copy.deepcopy(policy.critic).double()(tb.state0.double(), tb.action0.double()))
        inner(q, tq1, reward, weight)

    tr._update_priorities = record
    tr._learn_eager()
    torch.cuda.synchronize()
    B, n = 8, replay.n_steps
    W = replay.horizon - n
    R = B * W
    live = seen["weight"] != 0
    assert float(seen["count"][0]) == int(live.sum()) > 0                   # the statistics moved before the critic's forward
    big = seen["q_64"][live].abs().max().item()
    e_nat, e_32 = ((seen[k].double() - seen["q_64"])[live].abs().max().item() for k in ("q", "q_norm"))
    print(f"priorities' Q on the normalised buffer: native error {e_nat:.3g}, fp32 torch error {e_32:.3g}, largest {big:.3g}")
    assert e_nat <= max(4 * e_32, 1e-6 * big)                               # (_compare's criterion, on the same fp32 inputs)
    assert (seen["q"] - seen["q_raw"])[live].abs().max().item() > 1e3 * max(e_nat, e_32)
    assert all(torch.equal(a, b) for a, b in zip(rings, raw))
    host = {k: seen[k].cpu().numpy() for k in ("q", "tq1", "reward", "weight")}
    ref = pr.episode_deltas_ref(B, W, n, host["q"], host["tq1"][:R], host["reward"], host["weight"], policy.discount)
    got = tr.per_delta.cpu().numpy()
    assert np.isfinite(got).all() and (got >= 0).all() and got.tobytes() == ref.tobytes(), (got, ref)
    # the capture's warm-up updates: undone on the priorities and on the statistics
    tr._update_priorities = inner
    before = [t.clone() for t in (replay.ep_prio, replay.prio_max, expert.ep_prio, expert.prio_max) + policy.obs_norm.tensors() + (policy.acting_flat(),)]
    tr.capture()
    torch.cuda.synchronize()
    after = (replay.ep_prio, replay.prio_max, expert.ep_prio, expert.prio_max) + policy.obs_norm.tensors() + (policy.acting_flat(),)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    count0 = float(policy.obs_norm.count[0])
    for _ in range(5):
        tr.step()
    tr.flush(finish_update=True)
    torch.cuda.synchronize()
    assert tr.updates == 5 and float(policy.obs_norm.count[0]) > count0 and not torch.equal(before[0], replay.ep_prio)
    assert torch.isfinite(tr.native.losses).all() and torch.isfinite(policy._flat_params["actor"]).all()
    _acting_is_the_fold(policy, "trainer")
    sim.close()
