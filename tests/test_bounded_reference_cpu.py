"""The bounded critic update on the host: the references of tests/bounded_ref.py against float64 autograd of ddpgfd.DDPGfD / TD3fD with
q_bounds, huber_delta and max_grad_norm set (table networks, as in tests/test_td3_reference_cpu.py) and against
torch.nn.utils.clip_grad_norm_; the infinite settings that must be the unset policy bit for bit; validation; checkpoints.
tests/test_gpu_bounded_kernels.py holds the kernels to the references checked here."""
import math

import numpy as np
import pytest
import torch

from kinovagrasping_amd.ddpgfd import DDPGfD, TD3fD
from tests import bounded_ref as br
from tests import glue_ref as gr
from tests.test_td3_reference_cpu import _batch, _state, _Table

INF, NAN = float("inf"), float("nan")
LO, HI, DELTA = 0.0, 4.0, 2.0


class _TablePlusAction(torch.nn.Module):
    """a critic whose value is its own parameter plus the action it is given: its parameter takes a gradient and the actor behind it too"""

    def __init__(self, values):
        super().__init__()
        self.out = torch.nn.Parameter(values.clone())

    def forward(self, state, action):
        return self.out + action


def _rows(R, n, g, twin):
    """float32 inputs of one critic phase.  Rows 0..5 are built by hand (discount * 0 = 0 and discount^n * 0 = 0 are exact):
      row 0: both bootstraps below LO -> 0; rewards 1, 0, ... -> both targets 1; q = 1 + DELTA: |e| = DELTA exactly on both
      row 1: the same targets, q = 1 + 3 DELTA: the Huber branch, e > 0;   row 2: q = 1 - 3 DELTA: the Huber branch, e < 0
      row 3: the same targets, q = 1.5: the square branch
      row 4: both bootstraps above HI;   row 5: both inside [LO, HI]."""
    f = lambda *s: (torch.randn(*s, generator=g) * 3).float()
    q1, q2, rw = f(R), f(R), (torch.rand(R, n, generator=g) * 5).float()
    ta, tb = f(2 * R) + 2, f(2 * R) + 2
    rw[:4] = 0.0
    rw[:4, 0] = 1.0
    for t in (ta, tb):
        t[[0, 1, 2, 3, R, R + 1, R + 2, R + 3]] = -1.5
        t[[4, R + 4]] = 9.0
        t[[5, R + 5]] = 2.5
    tb[[0, R + 1]], tb[[4, R + 4]], ta[[5]] = -7.0, 11.0, 3.0            # the minimum comes from either critic
    for q in (q1, q2):
        q[0], q[1], q[2], q[3] = 1.0 + DELTA, 1.0 + 3 * DELTA, 1.0 - 3 * DELTA, 1.5
    return q1, (q2 if twin else None), ta, (tb if twin else None), rw


def _assert_covered(q1, ta, tb, rw, disc):
    """the inputs provably hold a clamped bootstrap on each side, a row on each Huber branch and one at |e| = DELTA exactly"""
    R = q1.shape[0]
    m = ta if tb is None else np.minimum(ta, tb)
    for half in (m[:R], m[R:]):
        assert (half < LO).any() and (half > HI).any() and ((half > LO) & (half < HI)).any()
    b1, bn = br.bootstrap(ta[:R], None if tb is None else tb[:R], ta[R:], None if tb is None else tb[R:], LO, HI)
    assert (b1 == LO).any() and (b1 == HI).any() and (bn == LO).any() and (bn == HI).any()
    t1, tn = gr.critic_targets(b1, bn, rw, disc)
    for e in (gr.wide(q1) - t1, gr.wide(q1) - tn):
        assert (np.abs(e) == DELTA).any() and (e > DELTA).any() and (e < -DELTA).any() and (np.abs(e) < DELTA).any()


@pytest.mark.parametrize("twin", [False, True], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("n", [1, 5])
def test_bounded_critic_ref_equals_float64_autograd(twin, n):
    """phase_critic in float64 on unmasked, masked and all-padding batches: dq against current_Q.grad, the loss triples, and the rows the
    rule distinguishes are asserted to be there"""
    R = 37
    g = torch.Generator().manual_seed(61 + n + 10 * twin)
    torch.manual_seed(7)
    kw = dict(hidden=(8, 8), q_bounds=(LO, HI), huber_delta=DELTA)
    p = TD3fD(82, 4, 0.8, n, policy_freq=2, **kw) if twin else DDPGfD(82, 4, 0.8, n, **kw)
    disc = float(np.float32(p.discount))
    p.discount, p._disc = disc, torch.tensor([disc ** i for i in range(n)], dtype=torch.float64)
    state = torch.zeros(R, n, 82, dtype=torch.float64)
    for call in range(3):
        w = (None, (torch.rand(R, generator=g) < 0.7).float(), torch.zeros(R))[call]
        if w is not None and call == 1:
            w[:6] = 1.0
        wn = None if w is None else w.numpy()
        q1, q2, ta, tb, rw = _rows(R, n, g, twin)
        _assert_covered(q1.numpy(), ta.numpy(), None if tb is None else tb.numpy(), rw.numpy(), disc)
        p.critic, p.critic_target = _Table(q1.double().view(R, 1)), _Table(ta.double().view(2 * R, 1))
        p.actor_target = _Table(torch.zeros(2 * R, 4, dtype=torch.float64))
        args = (state, torch.zeros(R, n, 4, dtype=torch.float64), state, rw.double(), None if w is None else w.double())
        if twin:
            p.critic2, p.critic2_target = _Table(q2.double().view(R, 1)), _Table(tb.double().view(2 * R, 1))
            losses = p.phase_critic(*args, target_noise=torch.zeros(2 * R, 4, dtype=torch.float64))
        else:
            losses = p.phase_critic(*args)
        wsum = gr.prologue_ref(R, n, wn, 0, 0, 0)[0] if call < 2 else 0.0
        np_ = lambda t: None if t is None else t.numpy()
        dq1, dq2, tboot, ref_losses = br.critic_grad_bounded_ref(q1.numpy(), np_(q2), ta.numpy()[:R], None if tb is None else tb.numpy()[:R], ta.numpy()[R:],
                                                                 None if tb is None else tb.numpy()[R:], rw.numpy(), wn, wsum, disc, LO, HI, DELTA)
        assert tboot.dtype == np.float32 and tboot.min() == LO and tboot.max() == HI
        assert len(losses) == len(ref_losses) == (6 if twin else 3)
        for a, b in zip(ref_losses, losses):
            assert abs(a - b.item()) <= 1e-13 * max(1.0, abs(b.item())), (call, ref_losses, losses)
        for dq, net in ((dq1, p.critic),) + (((dq2, p.critic2),) if twin else ()):
            assert np.abs(dq - net.out.grad[:, 0].numpy()).max() <= 1e-13 * max(1.0, float(net.out.grad.abs().max())), call
        if call == 0:
            # row 0 sits on the edge (gradient 2 DELTA + DELTA either way), rows 1 and 2 are clipped to +-DELTA, row 3 is not
            assert np.allclose(dq1[:4] * R, [3 * DELTA, 3 * DELTA, -3 * DELTA, 3 * 0.5], rtol=1e-12)
        if call == 2:
            assert not dq1.any() and ref_losses == (0.0,) * len(ref_losses)


def test_bounded_ref_edge_rules():
    """what the random rows cannot pin: NaN through the clamp and both Huber functions, the branches' values on the edge, the infinite
    settings, the float32 coefficient's special values"""
    f = np.float32
    x = np.array([-1.0, 0.0, 0.5, 50.0, 50.5, np.nan, -np.inf, np.inf], f)
    b = br.bound(x, 0.0, 50.0)
    assert b.dtype == f and np.isnan(b[5]) and b[[0, 1, 2, 3, 4, 6, 7]].tolist() == [0.0, 0.0, 0.5, 50.0, 50.0, 0.0, 50.0]
    assert np.array_equal(br.bound(x, -INF, INF)[[0, 1, 2, 3, 4, 6, 7]], x[[0, 1, 2, 3, 4, 6, 7]])
    e = np.array([-3.0, -2.0, -1.0, 0.0, 2.0, 2.5, np.nan])
    assert br.rho(e, 2.0)[:6].tolist() == [8.0, 4.0, 1.0, 0.0, 4.0, 6.0] and np.isnan(br.rho(e, 2.0)[6])
    assert br.huber_clip(e, 2.0)[:6].tolist() == [-2.0, -2.0, -1.0, 0.0, 2.0, 2.0] and np.isnan(br.huber_clip(e, 2.0)[6])
    assert np.array_equal(br.rho(e[:6], INF), e[:6] ** 2) and np.array_equal(br.huber_clip(e[:6], INF), e[:6])
    assert br.clip_coef_f32(0.0, 10.0) == (f(0.0), f(1.0))
    norm, coef = br.clip_coef_f32(1e36, 10.0)                        # (one element of 1e18: below float32's maximum of 3.4e38)
    assert abs(float(norm) - 1e18) <= 2.0 ** -23 * 1e18 and abs(float(coef) - 1e-17) <= 2.0 ** -22 * 1e-17
    norm, coef = br.clip_coef_f32(9e38, 10.0)                        # (one element of 3e19: finite in float64, beyond float32)
    assert norm == f(np.inf) and coef == f(0.0)
    norm, coef = br.clip_coef_f32(NAN, 10.0)
    assert np.isnan(norm) and np.isnan(coef)
    assert br.clip_coef_f32(400.0, INF) == (f(20.0), f(1.0)) and br.clip_coef_f32(400.0, 10.0)[0] == f(20.0)
    assert abs(float(br.clip_coef_f32(400.0, 10.0)[1]) - 10.0 / (20.0 + 1e-6)) <= 2.0 ** -24
    # the index sets of the partial sums are a partition, lane-major inside 4096-element trips
    count = 3 * 4096 + 5
    parts = [br.part_indices(count, k) for k in range(br.NORM_PARTS)]
    assert sorted(np.concatenate(parts).tolist()) == list(range(count)) and parts[1][:3].tolist() == [64, 65, 66] and parts[0][64] == 4096
    g = np.arange(count, dtype=f) / f(64)
    assert math.fsum(br.sqnorm_parts_ref(g).tolist()) == br.sqnorm_ref(g)


GRADS = [("large", 30.0), ("small", 1e-3)]          # norms far above and far below max_grad_norm = 10: coef < 1 and coef clamped to 1


@pytest.mark.parametrize("twin", [False, True], ids=["ddpgfd", "td3fd"])
def test_clipped_adam_ref_equals_the_phases_and_clip_grad_norm(twin):
    """phase_actor and phase_targets in float64 with max_grad_norm = 10 over 4 calls whose gradients alternate between a norm far above and
    far below it: sqnorm_ref against clip_grad_norm_'s own norm, g * coef against the gradients it leaves, the float32 coefficient against
    the float64 one, and adam_clipped_ref against the critics' and the (for TD3fD: delayed) actor's parameters after the step"""
    R, n, G = 29, 5, 10.0
    g = torch.Generator().manual_seed(91 + twin)
    torch.manual_seed(7)
    p = TD3fD(82, 4, 0.8, n, hidden=(8, 8), policy_freq=2, max_grad_norm=G) if twin else DDPGfD(82, 4, 0.8, n, hidden=(8, 8), max_grad_norm=G)
    critics = [_TablePlusAction(torch.randn(R, n, 1, generator=g, dtype=torch.float64)) for _ in range(2 if twin else 1)]
    actor = _Table(torch.randn(R, n, 1, generator=g, dtype=torch.float64))
    p.critic, p.actor = critics[0], actor
    p.critic_optimizer = torch.optim.Adam(critics[0].parameters(), lr=1e-3, weight_decay=1e-4)
    p.actor_optimizer = torch.optim.Adam(actor.parameters(), lr=1e-4)
    if twin:
        p.critic2, p.critic2_optimizer = critics[1], torch.optim.Adam(critics[1].parameters(), lr=1e-3, weight_decay=1e-4)
    p._flat_params = {k: torch.zeros(4, dtype=torch.float64) for k in p._flat_params}
    ref = [[c.out.detach().numpy().reshape(-1).copy(), np.zeros(R * n), np.zeros(R * n)] for c in critics]
    ref_a = [actor.out.detach().numpy().reshape(-1).copy(), np.zeros(R * n), np.zeros(R * n)]
    state = torch.zeros(R, n, 82, dtype=torch.float64)
    coefs = []
    for call in range(1, 5):
        scale = GRADS[(call - 1) % 2][1]
        for c, r in zip(critics, ref):
            g32 = (torch.randn(R * n, generator=g) * scale).float().numpy()
            c.out.grad = torch.from_numpy(gr.wide(g32)).view(R, n, 1).clone()
            # clip_grad_norm_ as the checker, on a copy
            probe = torch.nn.Parameter(torch.zeros(R * n, dtype=torch.float64))
            probe.grad = torch.from_numpy(gr.wide(g32)).clone()
            total = float(torch.nn.utils.clip_grad_norm_([probe], G))
            sq = br.sqnorm_ref(g32)
            assert abs(math.sqrt(sq) - total) <= 1e-14 * total
            coef64 = min(G / (math.sqrt(sq) + 1e-6), 1.0)
            assert np.abs(gr.wide(g32) * coef64 - probe.grad.numpy()).max() <= 1e-15 * max(1.0, np.abs(g32).max())
            norm32, coef32 = br.clip_coef_f32(sq, G)
            # (float)total and sqrtf: 1.5 roundings on the norm; + 1e-6f and the division: two more on the coefficient
            assert abs(float(norm32) - math.sqrt(sq)) <= 2 * 2.0 ** -24 * math.sqrt(sq) and abs(float(coef32) - coef64) <= 4 * 2.0 ** -24 * coef64
            coefs.append(coef64)
            r[:] = br.adam_clipped_ref(r[0], g32, r[1], r[2], call, 1, coef64, 1e-3, 0.9, 0.999, 1e-8, 1e-4)
        w = (torch.rand(R, generator=g) < 0.7).double()
        p.phase_actor(state, w)
        for c, r in zip(critics, ref):
            assert np.abs(r[0] - c.out.detach().numpy().reshape(-1)).max() <= 1e-12, call
        # the actor's gradient is dLoss/dQ of the actor loss: tiny on its own, so scale it into both regimes as well
        ga = actor.out.grad.reshape(-1).numpy().copy() * (1e5 if call in (1, 2) else 1.0)
        actor.out.grad = torch.from_numpy(ga).view(R, n, 1).clone()
        sq = math.fsum((ga * ga).tolist())
        coef64 = min(G / (math.sqrt(sq) + 1e-6), 1.0)
        p.phase_targets()
        ref_a[:] = br.adam_clipped_ref(ref_a[0], ga, ref_a[1], ref_a[2], call, 2 if twin else 1, coef64, 1e-4, 0.9, 0.999, 1e-8, 0.0)
        assert np.abs(ref_a[0] - actor.out.detach().numpy().reshape(-1)).max() <= 1e-12, call
        if not twin or call % 2 == 0:
            coefs.append(coef64)
    assert min(coefs) < 0.5 and max(coefs) == 1.0
    assert p.total_it == 4


@pytest.mark.parametrize("cls", [DDPGfD, TD3fD], ids=["ddpgfd", "td3fd"])
def test_the_infinite_settings_are_the_unset_policy_bit_for_bit(cls):
    """q_bounds = (-inf, inf), huber_delta = inf, max_grad_norm = inf against None, None, None: 3 fp32 updates on the CPU, every network and
    every loss equal in every bit (the clamp, rho and the coefficient 1 are exact)"""
    pols = []
    for kw in (dict(), dict(q_bounds=(-INF, INF), huber_delta=INF, max_grad_norm=INF)):
        torch.manual_seed(31)
        pols.append(cls(82, 4, 0.8, 5, hidden=(32, 24), **kw))
    assert pols[0].q_bounds is None and pols[0].huber_delta is None and pols[0].max_grad_norm is None
    assert pols[1].q_bounds == (-INF, INF) and pols[1].huber_delta == INF and pols[1].max_grad_norm == INF
    for it in range(3):
        b = _batch(700 + it, 24)
        extra = (torch.randn(48, 4, generator=torch.Generator().manual_seed(it)),) if cls is TD3fD else ()
        la, lb = (p.train_on_batch(*b, *extra) for p in pols)
        assert all(torch.equal(x, y) for x, y in zip(la, lb)) and all(torch.isfinite(x) for x in la)
    for k in pols[0]._flat_params:
        assert torch.equal(pols[0]._flat_params[k], pols[1]._flat_params[k]), k


def test_the_set_policy_differs_from_the_unset_one():
    """finite settings that bite change the update (the previous test would pass on options that do nothing)"""
    pols = []
    for kw in (dict(), dict(q_bounds=(0.0, 0.01)), dict(huber_delta=0.05), dict(max_grad_norm=1e-3)):
        torch.manual_seed(31)
        pols.append(DDPGfD(82, 4, 0.8, 5, hidden=(32, 24), **kw))
        pols[-1].train_on_batch(*_batch(700, 24))
    for p in pols[1:]:
        assert not torch.equal(p._flat_params["critic"], pols[0]._flat_params["critic"])


BAD = [dict(q_bounds=(1.0, 0.0)), dict(q_bounds=(NAN, 1.0)), dict(q_bounds=(0.0, NAN)), dict(huber_delta=0.0), dict(huber_delta=-1.0),
       dict(huber_delta=NAN), dict(max_grad_norm=0.0), dict(max_grad_norm=-2.0), dict(max_grad_norm=NAN)]


@pytest.mark.parametrize("cls", [DDPGfD, TD3fD], ids=["ddpgfd", "td3fd"])
@pytest.mark.parametrize("kw", BAD, ids=[f"{k}={v}" for d in BAD for k, v in d.items()])
def test_invalid_settings_raise(cls, kw):
    with pytest.raises(ValueError):
        cls(82, 4, 0.8, 5, hidden=(8, 8), **kw)


def test_valid_edge_settings_are_accepted():
    p = TD3fD(82, 4, 0.8, 5, hidden=(8, 8), q_bounds=(2, 2), huber_delta=1e-30, max_grad_norm=INF)
    assert p.q_bounds == (2.0, 2.0) and p.huber_delta == 1e-30 and p.max_grad_norm == INF
    p = DDPGfD(82, 4, 0.8, 5, hidden=(8, 8), q_bounds=[0, 50])
    assert p.q_bounds == (0.0, 50.0) and p.huber_delta is None and p.max_grad_norm is None


@pytest.mark.parametrize("cls", [DDPGfD, TD3fD], ids=["ddpgfd", "td3fd"])
def test_checkpoints_carry_no_new_state(cls, tmp_path):
    """a checkpoint written with the options set loads into a policy without them, and back: the same files, the same state"""
    opts = dict(q_bounds=(0.0, 50.0), huber_delta=10.0, max_grad_norm=10.0)
    extra = lambda it: (torch.randn(16, 4, generator=torch.Generator().manual_seed(it)),) if cls is TD3fD else ()
    torch.manual_seed(41)
    src = cls(82, 4, 0.8, 5, hidden=(16, 12), **opts)
    for it in range(3):
        src.train_on_batch(*_batch(300 + it, 8), *extra(it))
    src.save(str(tmp_path / "set"))
    files = sorted(f.name for f in tmp_path.iterdir())
    assert files == sorted("set_" + s for s in ("actor", "critic", "actor_optimizer", "critic_optimizer") + (("critic2", "critic2_optimizer") if cls is TD3fD else ()))
    torch.manual_seed(42)
    plain = cls(82, 4, 0.8, 5, hidden=(16, 12))
    plain.load(str(tmp_path / "set"), sync_targets=True)
    want, got = _state(src), _state(plain)
    assert set(want) == set(got)
    assert all(torch.equal(got[k], want[k]) for k in want if not k.endswith("_target"))
    plain.train_on_batch(*_batch(400, 8), *extra(9))
    plain.save(str(tmp_path / "plain"))
    torch.manual_seed(43)
    back = cls(82, 4, 0.8, 5, hidden=(16, 12), **opts)
    back.load(str(tmp_path / "plain"))
    want, got = _state(plain), _state(back)
    assert all(torch.equal(got[k], want[k]) for k in want if not k.endswith("_target"))
    assert back.q_bounds == (0.0, 50.0) and plain.q_bounds is None
    back.train_on_batch(*_batch(401, 8), *extra(10))
