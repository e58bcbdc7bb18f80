"""TD3fD on the host: the references of tests/td3_ref.py against float64 autograd of ddpgfd.TD3fD's phases (table networks, as in
tests/test_glue_reference_cpu.py), the degenerate TD3fD that must be DDPGfD bit for bit, checkpoints, and the gradient exchange of the
second critic over two gloo ranks.  tests/test_gpu_td3_kernels.py holds the kernels to the references checked here."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from kinovagrasping_amd.ddpgfd import DDPGfD, TD3fD
from tests import glue_ref as gr
from tests import td3_ref as tr


class _Table(torch.nn.Module):
    """a network that returns its own parameter whatever it is given: its gradient is dLoss/dOutput"""

    def __init__(self, values):
        super().__init__()
        self.out = torch.nn.Parameter(values.clone())

    def forward(self, *inputs):
        return self.out


class _TablePlusAction(torch.nn.Module):
    """a target critic whose value depends on the action it is given: table + action @ coef"""

    def __init__(self, table, coef):
        super().__init__()
        self.table, self.coef = table, coef

    def forward(self, state, action):
        return self.table + action @ self.coef


class _Second(torch.nn.Module):
    def forward(self, state, action):
        return action


class _Forbidden(torch.nn.Module):
    def forward(self, *inputs):
        raise AssertionError("the actor loss goes through critic 1 only")


class _CountStep:
    def __init__(self):
        self.steps = 0

    def step(self):
        self.steps += 1

    def zero_grad(self):
        pass


@pytest.mark.parametrize("n", [1, 5])
def test_td3_refs_equal_float64_autograd_over_12_calls(n):
    """TD3fD.phase_critic / phase_actor / phase_targets in float64, 12 calls on unmasked, masked and all-padding batches (policy_freq 2:
    the actor steps on the even calls; the targets move on call 10): the six losses, both dLoss/dQ, the smoothed action through target
    critics that depend on it, dLoss/dQ of the actor loss, the delayed Adam step and the three soft updates."""
    R = 37
    g = torch.Generator().manual_seed(23 + n)
    f32 = lambda *s: torch.randn(*s, generator=g).float()
    torch.manual_seed(7)
    p = TD3fD(82, 4, 0.8, n, hidden=(8, 8), device="cpu", policy_freq=2)
    disc = float(np.float32(p.discount))
    p.discount = disc
    p._disc = torch.tensor([disc ** i for i in range(n)], dtype=torch.float64)
    p.policy_noise, p.noise_clip = float(np.float32(p.policy_noise)), float(np.float32(p.noise_clip))
    assert (p.policy_noise, p.noise_clip) == (float(np.float32(0.1 * 0.8)), float(np.float32(0.25 * 0.8)))
    actor = _Table(torch.randn(R, n, 1, generator=g, dtype=torch.float64))
    adam = torch.optim.Adam(actor.parameters(), lr=1e-4)
    rp, rm, rv = actor.out.detach().numpy().reshape(-1).copy(), np.zeros(R * n), np.zeros(R * n)
    names = ("critic", "critic_target", "critic2", "critic2_target", "actor", "actor_target")
    p._flat_params = {k: torch.randn(300, generator=g, dtype=torch.float64) for k in names}
    ref = {k: v.numpy().copy() for k, v in p._flat_params.items()}
    state = torch.zeros(R, n, 82, dtype=torch.float64)
    moved, stepped = [], []
    for call in range(1, 13):
        kind = ("none", "masked", "all_zero")[(call - 1) % 3]
        w = {"none": None, "masked": (torch.rand(R, generator=g) < 0.7).float(), "all_zero": torch.zeros(R)}[kind]
        w64, wn = (None if w is None else w.double()), (None if w is None else w.numpy())
        q1, q2, rw = f32(R, 1) * 3, f32(R, 1) * 3, torch.rand(R, n, generator=g).float() * 5
        a_raw = (torch.rand(2 * R, 4, generator=g).float() * 1.2 - 0.2).clamp(0, 0.8)        # some rows at 0 and at max_action
        z = f32(2 * R, 4) * 2                                                                  # |0.08 z| beyond the clip of 0.2 for some
        ta_tab, tb_tab, ca, cb = f32(2 * R, 1) * 3, f32(2 * R, 1) * 3, f32(4, 1), f32(4, 1)
        p.critic, p.critic2, p.actor_target = _Table(q1.double()), _Table(q2.double()), _Table(a_raw.double())
        p.critic_target, p.critic2_target = _TablePlusAction(ta_tab.double(), ca.double()), _TablePlusAction(tb_tab.double(), cb.double())
        p.critic_optimizer, p.critic2_optimizer = _CountStep(), _CountStep()
        losses = p.phase_critic(state, torch.zeros(R, n, 4, dtype=torch.float64), state, rw.double(), w64, target_noise=z.double())
        wsum, dqa, _, _ = gr.prologue_ref(R, n, wn, call - 1, 0, 0)
        ta = tr.target_smooth_ref(a_raw.numpy(), z.numpy(), p.policy_noise, p.noise_clip, 0.8)
        assert (np.abs(0.08 * z.numpy()) > 0.2).any() and (ta == 0).any() and (ta == 0.8).any()
        tqa = gr.wide(ta_tab.numpy())[:, 0] + ta @ gr.wide(ca.numpy())[:, 0]
        tqb = gr.wide(tb_tab.numpy())[:, 0] + ta @ gr.wide(cb.numpy())[:, 0]
        dq1, dq2, tmin, ref_losses = tr.twin_critic_grad_ref(q1[:, 0].numpy(), q2[:, 0].numpy(), tqa[:R], tqb[:R], tqa[R:], tqb[R:], rw.numpy(), wn, wsum, disc)
        assert len(losses) == 6 and np.array_equal(tmin, np.minimum(tqa, tqb))
        for a, b in zip(ref_losses, losses):
            assert abs(a - b.item()) <= 1e-13 * max(1.0, abs(b.item())), (call, ref_losses, losses)
        for dq, net in ((dq1, p.critic), (dq2, p.critic2)):
            assert np.abs(dq - net.out.grad[:, 0].numpy()).max() <= 1e-13 * max(1.0, float(net.out.grad.abs().max())), call
        if kind == "all_zero":
            assert not dq1.any() and not dq2.any() and ref_losses == (0.0,) * 6
        # the actor loss through critic 1 only; both critics' optimizers step first
        p.actor, p.actor_optimizer, p.critic, p.critic2 = actor, adam, _Second(), _Forbidden()
        p.phase_actor(state, w64)
        assert (p.critic_optimizer.steps, p.critic2_optimizer.steps) == (1, 1)
        got = actor.out.grad.reshape(-1).numpy().copy()
        assert np.abs(dqa - got).max() <= 1e-15, call
        # the delayed actor step and the three soft updates
        for k in ("critic", "critic2", "actor"):
            p._flat_params[k] += 0.1 * torch.randn(300, generator=g, dtype=torch.float64)
        before_t, before_a = p._flat_params["critic2_target"].clone(), actor.out.detach().clone()
        p.phase_targets()
        assert p.total_it == call
        rp, rm, rv = tr.adam_every_ref(rp, got, rm, rv, call, 2, 1e-4, 0.9, 0.999, 1e-8, 0.0)
        assert np.abs(rp - actor.out.detach().numpy().reshape(-1)).max() <= 1e-12, call
        if not torch.equal(before_a, actor.out.detach()):
            stepped.append(call)
        if adam.state:
            st = adam.state[actor.out]
            assert int(st["step"]) == call // 2
            assert np.abs(rm - st["exp_avg"].numpy().reshape(-1)).max() <= 1e-15 and np.abs(rv - st["exp_avg_sq"].numpy().reshape(-1)).max() <= 1e-15
        for k in ("critic", "critic2", "actor"):
            ref[k + "_target"] = gr.soft_update_ref(p._flat_params[k].numpy(), ref[k + "_target"], p.tau, call, p.network_repl_freq)
            assert np.abs(ref[k + "_target"] - p._flat_params[k + "_target"].numpy()).max() <= 1e-15, (call, k)
        if not torch.equal(before_t, p._flat_params["critic2_target"]):
            moved.append(call)
    assert moved == [10]
    # (calls 6 and 12 are all padding: their step is on a zero gradient, which still moves the weights through the moments)
    assert stepped == [2, 4, 6, 8, 10, 12], stepped


def test_td3_refs_edge_rules():
    """the rules the random calls cannot pin: NaN through both clamps and the minimum, the clamps' edges, the gate of the delayed step"""
    f = np.float32
    nan = f("nan")
    a = np.array([0.0, 0.8, 0.3, nan, 0.3, 0.79, 0.01, 0.5], f)
    z = np.array([-1.0, 1.0, nan, 1.0, 100.0, 2.5, -2.5, 0.0], f)
    out = tr.target_smooth_f32(a, z, 0.08, 0.2, 0.8)
    exp = np.array([0.0, 0.8, nan, nan, f(0.3) + f(0.2), 0.8, 0.0, 0.5], f)
    assert out.dtype == f and np.array_equal(out.view(np.uint32)[[0, 1, 4, 5, 6, 7]], exp.view(np.uint32)[[0, 1, 4, 5, 6, 7]]) and np.isnan(out[2:4]).all()
    assert np.array_equal(tr.target_smooth_f32(a[[0, 1, 7]], z[[0, 1, 7]] * 0 + 7, 0.0, 0.2, 0.8), a[[0, 1, 7]])
    wide = tr.target_smooth_ref(a, z, float(f(0.08)), float(f(0.2)), 0.8)
    assert np.isnan(wide[2:4]).all() and np.abs(wide[[0, 1, 4, 5, 6, 7]] - out[[0, 1, 4, 5, 6, 7]].astype(np.float64)).max() <= 2.0 ** -24
    m = tr.nan_min(np.array([1.0, nan, 2.0, -0.5], f), np.array([nan, 1.0, -3.0, 7.0], f))
    assert np.isnan(m[:2]).all() and m[2:].tolist() == [-3.0, -0.5]
    p = np.array([1.0, -2.0], f)
    g, m0, v0 = np.array([0.5, 0.25], f), np.array([0.1, 0.2], f), np.array([0.3, 0.4], f)
    for step in (0, 1, 3, -2):
        kept = tr.adam_every_ref(p, g, m0, v0, step, 2, 1e-3, 0.9, 0.999, 1e-8, 1e-4)
        assert all(np.array_equal(x, y.astype(np.float64)) for x, y in zip(kept, (p, m0, v0)))
    for step, t in ((2, 1), (24, 12)):
        assert all(np.array_equal(x, y) for x, y in zip(tr.adam_every_ref(p, g, m0, v0, step, 2, 1e-3, 0.9, 0.999, 1e-8, 1e-4),
                                                         gr.adam_ref(p, g, m0, v0, t, 1e-3, 0.9, 0.999, 1e-8, 1e-4)))


def test_tagged_normals_are_a_stream_of_their_own():
    """the tagged draw with the exploration noise's tag is philox_ref.normal4; with the smoothing's tag it is another, standard normal, stream"""
    from tests import philox_ref
    rows = np.arange(4096, dtype=np.uint64)
    seed, step = np.uint64(0x123456789ABCDEF), np.uint64(0x100000003)
    assert np.array_equal(tr.normal4_tagged(seed, step, rows, 0x4B52), philox_ref.normal4(seed, step, rows))
    z = tr.normal4_tagged(seed, step, rows, tr.TAG_TARGET_SMOOTH)
    assert tr.TAG_TARGET_SMOOTH not in (0x4B52, 0x5A4D, 0x5A4E)
    assert not np.isclose(z, philox_ref.normal4(seed, step, rows)).any(1).any()
    assert abs(z.mean()) < 0.03 and abs(z.std() - 1.0) < 0.03 and np.abs(z).max() < 6.0
    assert not np.array_equal(z, tr.normal4_tagged(seed, step + np.uint64(1), rows, tr.TAG_TARGET_SMOOTH))
    assert not np.array_equal(z, tr.normal4_tagged(seed, step ^ np.uint64(1 << 32), rows, tr.TAG_TARGET_SMOOTH))
    assert not np.array_equal(z, tr.normal4_tagged(seed ^ np.uint64(1 << 32), step, rows, tr.TAG_TARGET_SMOOTH))


def _batch(seed, rows, n=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, n, 82, generator=g), torch.rand(rows, n, 4, generator=g) * 0.8, torch.randn(rows, n, 82, generator=g),
            torch.rand(rows, n, generator=g) * 5, (torch.rand(rows, generator=g) < 0.8).float())


def _degenerate_pair(hidden=(32, 24)):
    """a DDPGfD and, from the same seed, a TD3fD without noise and delay whose second critic is a copy of the first"""
    torch.manual_seed(31)
    ddpg = DDPGfD(82, 4, 0.8, 5, hidden=hidden)
    torch.manual_seed(31)
    td3 = TD3fD(82, 4, 0.8, 5, hidden=hidden, policy_noise=0.0, policy_freq=1)
    for k in ("critic", "critic_target"):
        td3._flat_params[k.replace("critic", "critic2")].copy_(td3._flat_params[k])
    return ddpg, td3


def test_degenerate_td3fd_is_ddpgfd_bit_for_bit():
    """critic2 = critic, policy_noise 0, policy_freq 1: after 12 train_on_batch calls (fp32) actor, critic and both targets are equal in
    every bit, and the copied critic has stayed a copy"""
    ddpg, td3 = _degenerate_pair()
    for k in ("actor", "critic", "actor_target", "critic_target"):
        assert torch.equal(ddpg._flat_params[k], td3._flat_params[k]), k           # the same seed gives the same first four networks
    for it in range(12):
        b = _batch(200 + it, 24)
        la, lb = ddpg.train_on_batch(*b), td3.train_on_batch(*b)
        assert len(lb) == 7 and all(torch.equal(x, y) for x, y in zip(la, lb[:4])) and all(torch.equal(x, y) for x, y in zip(lb[1:4], lb[4:]))
    for k in ("actor", "critic", "actor_target", "critic_target"):
        assert torch.equal(ddpg._flat_params[k], td3._flat_params[k]), k
    assert torch.equal(td3._flat_params["critic2"], td3._flat_params["critic"]) and torch.equal(td3._flat_params["critic2_target"], td3._flat_params["critic_target"])
    assert (ddpg.total_it, td3.total_it) == (12, 12)


def test_td3fd_defaults_and_independent_second_critic():
    torch.manual_seed(3)
    p = TD3fD(82, 4, 0.8, 5, hidden=(16, 16))
    assert (p.policy_noise, p.noise_clip, p.policy_freq) == (0.1 * 0.8, 0.25 * 0.8, 2)
    assert not torch.equal(p._flat_params["critic2"], p._flat_params["critic"])
    assert torch.equal(p._flat_params["critic2"], p._flat_params["critic2_target"])
    assert p.critic2.l1.weight.data_ptr() == p._flat_params["critic2"].data_ptr()
    a, b = p.critic_optimizer.param_groups[0], p.critic2_optimizer.param_groups[0]
    assert all(a[k] == b[k] for k in ("lr", "betas", "eps", "weight_decay"))
    with pytest.raises(ValueError):
        TD3fD(82, 4, 0.8, 5, hidden=(16, 16), policy_freq=0)
    # without given draws the phase draws its own: two calls on the same batch from the same weights differ, given draws repeat
    b = _batch(5, 8)
    l1 = p.phase_critic(*b[:4], b[4])
    l2 = p.phase_critic(*b[:4], b[4])
    z = torch.randn(16, 4, generator=torch.Generator().manual_seed(1))
    l3, l4 = p.phase_critic(*b[:4], b[4], target_noise=z), p.phase_critic(*b[:4], b[4], target_noise=z)
    assert not torch.equal(l1[0], l2[0]) and torch.equal(l3[0], l4[0])


def _state(p):
    nets = ("actor", "critic", "critic2", "actor_target", "critic_target", "critic2_target")
    out = {k: p._flat_params[k].clone() for k in nets if k in p._flat_params}
    for name in ("actor_optimizer", "critic_optimizer", "critic2_optimizer"):
        opt = getattr(p, name, None)
        if opt is not None:
            for i, q in enumerate(opt.param_groups[0]["params"]):
                for k, v in opt.state[q].items():
                    out[f"{name}.{i}.{k}"] = torch.as_tensor(v).clone()
    return out


def test_td3fd_checkpoints(tmp_path):
    """save -> load restores the six networks' weights (targets with sync_targets) and the three optimizers; the same files load into a
    DDPGfD; the reference's four files load into a TD3fD and leave critic2 alone"""
    torch.manual_seed(41)
    src = TD3fD(82, 4, 0.8, 5, hidden=(16, 12))
    for it in range(3):
        src.train_on_batch(*_batch(300 + it, 8))
    prefix = str(tmp_path / "td3")
    src.save(prefix)
    assert sorted(f.name for f in tmp_path.iterdir()) == sorted("td3_" + s for s in ("actor", "critic", "critic2", "actor_optimizer", "critic_optimizer",
                                                                                   "critic2_optimizer"))
    want = _state(src)
    torch.manual_seed(42)
    dst = TD3fD(82, 4, 0.8, 5, hidden=(16, 12))
    targets_before = {k: dst._flat_params[k].clone() for k in ("actor_target", "critic_target", "critic2_target")}
    dst.load(prefix)
    got = _state(dst)
    for k in want:
        if k.endswith("_target"):
            assert torch.equal(got[k], targets_before[k]), k               # like the reference, loading leaves the targets alone
        else:
            assert torch.equal(got[k], want[k]), k
    assert [float(s["step"]) for s in dst.actor_optimizer.state.values()] == [1.0] * 6       # 3 updates, policy_freq 2
    assert [float(s["step"]) for s in dst.critic2_optimizer.state.values()] == [3.0] * 6
    dst.load(prefix, sync_targets=True)
    for k in ("actor", "critic", "critic2"):
        assert torch.equal(dst._flat_params[k + "_target"], want[k]), k
    # the same files into a DDPGfD
    torch.manual_seed(43)
    plain = DDPGfD(82, 4, 0.8, 5, hidden=(16, 12))
    plain.load(prefix)
    got = _state(plain)
    assert all(torch.equal(got[k], want[k]) for k in got if not k.endswith("_target")) and "critic2" not in got
    # the reference's four files into a TD3fD
    four = str(tmp_path / "four")
    plain.save(four)
    torch.manual_seed(44)
    dst = TD3fD(82, 4, 0.8, 5, hidden=(16, 12))
    keep = {k: dst._flat_params[k].clone() for k in ("critic2", "critic2_target")}
    dst.load(four, sync_targets=True)
    assert torch.equal(dst._flat_params["critic"], want["critic"]) and torch.equal(dst._flat_params["critic_target"], want["critic"])
    assert torch.equal(dst._flat_params["critic2"], keep["critic2"]) and torch.equal(dst._flat_params["critic2_target"], keep["critic2"])
    assert not dst.critic2_optimizer.state


# ---- world-2 gloo: the second critic's gradients are averaged too (the pattern of tests/test_distributed_cpu.py) --------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _full_batch(it):
    st, ac, ns, rw, _ = _batch(100 + it, 32)
    return st, ac, ns, rw, torch.randn(64, 4, generator=torch.Generator().manual_seed(500 + it))


def _nets(pol):
    return {f"{name}.{k}": v for name in ("actor", "critic", "critic2", "actor_target", "critic2_target") for k, v in getattr(pol, name).state_dict().items()}


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(123)                      # identical initial replicas
    pol = TD3fD(82, 4, 0.8, 5, hidden=(64, 48))
    for it in range(12):                        # crosses the soft target update at call 10
        st, ac, ns, rw, z = _full_batch(it)
        rows = slice(rank * 16, (rank + 1) * 16)
        # the draws of the shard's rows: [1-step rows | n-step rows] of the full batch's
        pol.train_on_batch(st[rows], ac[rows], ns[rows], rw[rows], None, torch.cat([z[:32][rows], z[32:][rows]]))
    torch.save(_nets(pol), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_rank_allreduce_averages_the_second_critic_too(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt")
    r1 = torch.load(tmp_path / "rank1.pt")
    for k in r0:
        assert torch.equal(r0[k], r1[k]), k          # replicas stay bit-identical: they trained on different shards
    torch.manual_seed(123)
    pol = TD3fD(82, 4, 0.8, 5, hidden=(64, 48))
    start = {k: v.clone() for k, v in _nets(pol).items()}
    for it in range(12):
        st, ac, ns, rw, z = _full_batch(it)
        pol.train_on_batch(st, ac, ns, rw, None, z)
    ref = _nets(pol)
    for k in ref:
        torch.testing.assert_close(r0[k], ref[k], rtol=1e-4, atol=1e-6)
    assert not torch.equal(ref["critic2.l1.weight"], start["critic2.l1.weight"])
