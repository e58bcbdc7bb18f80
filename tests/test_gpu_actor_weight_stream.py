"""The in-kernel actor's operands arrive as batches of range-checked buffer loads (csrc/ks_mlp_tile.h).  Nothing of the arithmetic changed, so
(1) the free-running rollout still equals the lock-step calls per env, bit for bit, at every tile pair of k_rollout - at a nominal width and at
one whose last tiles are partial - in the wave form and in the workgroup form, with a group whose waves hold 4, 1, 0 and 0 envs; and (2) a
forward on parameters that lie between NaN words returns the bits of the same forward on ordinary tensors: a guard word that reached an
MFMA would show as NaN."""
import pytest
import torch

from kinovagrasping_amd import mlp, sim as ks
from tests.test_gpu_async import _free_running_equals_lock_step

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("waves", ["waves", "workgroups"])
@pytest.mark.parametrize("hidden", [(128, 128), (244, 244), (120, 116), (60, 52), (392, 292)])
def test_rollout_equals_lock_step_at_nominal_and_partial_tile_widths(monkeypatch, hidden, waves):
    """21 envs: one full group and one of 5 envs (waves with 4, 1, 0, 0 envs); horizon 6, launches of 8 env-steps"""
    if waves == "workgroups":
        monkeypatch.setenv("KS_ROLLOUT_WAVES", "0")
    # The comparison builds an AsyncTrainer for the rollout's argument record and never runs an update.  The trainer refuses widths
    # whose LEARNER has no LDS-free kernels - every width with a partial last tile but 392-292 - which is not what is compared here.
    from kinovagrasping_amd import learner_native

    class RolloutOnly(learner_native.NativeDDPGfDUpdate):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.lds_free = True

    monkeypatch.setattr(learner_native, "NativeDDPGfDUpdate", RolloutOnly)
    _free_running_equals_lock_step(hidden, False, 6, 8, 21, expect_plan=waves)


def _net(hw, g):
    dims = [(hw[0], 82), (hw[1], hw[0]), (4, hw[1])]
    return [(torch.randn(o, i, generator=g) / i ** 0.5, 0.1 * torch.randn(o, generator=g)) for o, i in dims]


def _guarded(layers):
    """the same parameters as 16-byte-aligned views into ONE tensor of NaN: at least 4 NaN words on both sides of every matrix and bias"""
    flat = [t for wb in layers for t in wb]
    up4 = lambda k: (k + 3) // 4 * 4
    pool = torch.full((sum(up4(t.numel()) + 8 for t in flat) + 8,), float("nan"), device=DEV)
    assert pool.data_ptr() % 16 == 0
    views, at = [], 8
    for t in flat:
        v = pool[at:at + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 0 and v.is_contiguous()
        views.append(v)
        at += up4(t.numel()) + 8
    assert int(torch.isnan(pool).sum()) == pool.numel() - sum(t.numel() for t in flat)
    return pool, [(views[0], views[1]), (views[2], views[3]), (views[4], views[5])]


@pytest.mark.parametrize("hw", [(60, 52), (244, 244), (392, 292), (250, 250)])
def test_forward_on_parameters_between_nan_words_returns_the_same_bits(hw):
    n = 17
    g = torch.Generator().manual_seed(hw[0] * 1000 + hw[1])
    plain = [(w.to(DEV), b.to(DEV)) for w, b in _net(hw, g)]
    pool, guarded = _guarded(plain)
    obs = torch.randn(n, 82, generator=g).to(DEV)
    prev = torch.randn(n, 82, generator=g).to(DEV)
    prev[: n // 2, 9:16:3] = obs[: n // 2, 9:16:3]
    has_prev = (torch.rand(n, generator=g) < 0.8).to(DEV)
    t = torch.randint(0, 30, (n,), generator=g).to(DEV)
    noise = torch.randn(n, 4, generator=g).to(DEV)
    ready = (torch.rand(n, generator=g) < 0.1).to(DEV)
    lib, P = ks.load_library(), ks._ptr
    stream = lambda: mlp._stream(obs)

    def forward(layers):
        return mlp.mlp3_forward(layers, obs, act=mlp.ACT_SIGMOID, scale=0.8)

    def select(layers):
        (w1, b1), (w2, b2), (w3, b3) = layers
        r, pi = ready.clone(), torch.full((n, 4), 7.0, device=DEV)
        a, at, lift = torch.full((n, 4), 7.0, device=DEV), torch.full((4, n), 7.0, device=DEV), torch.zeros(n, dtype=torch.bool, device=DEV)
        assert lib.kr_actor_select(n, hw[0], hw[1], P(obs), P(prev), P(has_prev), P(t), P(r), P(w1), P(b1), P(w2), P(b2), P(w3), P(b3), P(noise), 0,
                                   None, 0.08, 0.8, 6, P(pi), P(a), P(at), P(lift), stream()) == 0
        return pi, a, at, lift, r

    out_p, out_g = forward(plain), forward(guarded)
    sel_p, sel_g = select(plain), select(guarded)
    torch.cuda.synchronize()
    assert torch.isfinite(out_g).all() and torch.equal(out_p, out_g)
    assert (out_g > 0).all() and (out_g < 0.8).all() and out_g.std() > 0
    for p, q in zip(sel_p, sel_g):
        assert torch.isfinite(q.float()).all() and torch.equal(p, q)
    assert torch.equal(sel_g[0], out_g)                          # kr_actor_select's actor_out is kr_mlp3_forward's output
