"""Running observation normalisation on the host (ddpgfd.DDPGfD / TD3fD with obs_norm; ddpgfd.ObsNorm): the torch implementation - the
specification of kr_obs_stats_update / kr_obs_normalize / kr_fold_obs_norm - against tests/obsnorm_ref.py and numpy's one-shot mean and
variance, the invariance the feature exists for, the unset feature in every bit, the freeze, checkpoints and the refusals."""
import numpy as np
import pytest
import torch

from kinovagrasping_amd.ddpgfd import DDPGfD, ObsNorm, TD3fD, _flatten_parameters
from tests import obsnorm_ref as onr

S, A, N = 82, 4, 5
HIDDEN = (32, 24)


def _policy(td3=False, seed=3, double=False, **kw):
    torch.manual_seed(seed)
    p = (TD3fD if td3 else DDPGfD)(S, A, 0.8, N, hidden=HIDDEN, **kw)
    if double:
        nets = ("actor", "critic", "actor_target", "critic_target") + (("critic2", "critic2_target") if td3 else ())
        for name in nets:
            getattr(p, name).double()
            p._flat_params[name] = _flatten_parameters(getattr(p, name))
        p._disc = p._disc.double()
        p.refresh_acting()
    return p


def _batch(seed, R=14, dtype=torch.float32, scale=None, shift=None):
    """R windows of n steps; rows 0, 5 and the last are padding (weight 0).  The state columns have very different scales, as the real
    observation's: column k is scale[k] * N(0, 1) + shift[k]"""
    g = torch.Generator().manual_seed(seed)
    scale = torch.logspace(-2, 1, S) if scale is None else scale
    shift = torch.linspace(-3, 3, S) if shift is None else shift
    st = torch.randn(R, N, S, generator=g) * scale + shift
    ns = torch.randn(R, N, S, generator=g) * scale + shift
    ac = torch.rand(R, N, A, generator=g) * 0.8
    rw = torch.rand(R, N, generator=g) * 5
    w = torch.ones(R)
    w[[0, 5, R - 1]] = 0
    return tuple(t.to(dtype) for t in (st, ac, ns, rw, w))


def _stats(p):
    on = p.obs_norm
    return float(on.count[0]), on.mean.numpy().copy(), on.m2.numpy().copy()


def test_statistics_equal_numpys_one_shot_mean_and_variance():
    """After 1, 2 and 7 updates on batches with padding rows count / mean / m2 are numpy's mean and sum of squared deviations over the
    concatenation of the counted window-first states, within obsnorm_ref's bounds of the fp64 merges (error / bound <= 1); the derived
    vectors are the reference's roundings of the state in every bit; the acting copy is the fold of actor and statistics."""
    p = _policy(obs_norm=True)
    assert _stats(p)[0] == 0 and not p.obs_norm.mean32.any() and bool((p.obs_norm.inv32 == 1).all())
    assert torch.equal(p.acting_flat(), p._flat_params["actor"]) and p.acting_flat().data_ptr() != p._flat_params["actor"].data_ptr()
    rows = []
    for k in range(7):
        st, ac, ns, rw, w = _batch(100 + k)
        p.train_on_batch(st, ac, ns, rw, w)
        rows.append(st[:, 0][w != 0].double().numpy())
        if k + 1 not in (1, 2, 7):
            continue
        allrows = np.concatenate(rows)
        count, mean, m2 = _stats(p)
        X = np.abs(allrows).max(0)
        assert count == allrows.shape[0] == 11 * (k + 1)
        for name, got, ref, bound in (("mean", mean, allrows.mean(0), onr.mean_bound(count, k + 1, X)),
                                      ("m2", m2, allrows.var(0) * count, onr.m2_bound(count, k + 1, X))):
            ratio = (np.abs(got - ref) / bound).max()
            print(f"\nOBSNORM after {k + 1} updates | {name} | worst err {np.abs(got - ref).max():.3e} | worst err/bound {ratio:.3f}")
            assert ratio <= 1, (k + 1, name, ratio)
        m32, i32 = onr.derived_ref(count, mean, m2, p.obs_norm.eps)
        assert m32.tobytes() == p.obs_norm.mean32.numpy().tobytes() and i32.tobytes() == p.obs_norm.inv32.numpy().tobytes()
        wf, bf, terms = onr.fold_ref(p.actor.l1.weight.data.numpy(), p.actor.l1.bias.data.numpy(), m32, i32)
        (w1, b1), l2, l3 = p.acting_layers()
        assert w1.numpy().tobytes() == wf.tobytes()
        assert (np.abs(b1.numpy().astype(np.float64) - bf) <= onr.fold_bias_bound(bf, terms, S)).all()
        assert torch.equal(l2[0], p.actor.l2.weight.data) and torch.equal(l3[1], p.actor.l3.bias.data)
    assert torch.isfinite(p._flat_params["actor"]).all()


def test_obsnorm_update_is_the_reference_merge_and_ignores_padding_content():
    """ObsNorm.update against obsnorm_ref.stats_update_ref step by step - NULL weight, mixed zeros, all zeros (nothing changes in any bit), a
    start from nothing and a merge into a long history -, and a padding row holding NaN changes nothing in any bit"""
    r = np.random.RandomState(5)
    on = ObsNorm(S, 1e-2)
    on.count.fill_(1e9)
    on.mean.copy_(torch.from_numpy(r.standard_normal(S)))
    on.m2.copy_(torch.from_numpy(1e9 * (0.5 + r.rand(S))))
    for k, weight in enumerate((None, "mixed", "zero", "mixed")):
        x = torch.from_numpy(r.standard_normal((21, S)).astype(np.float32) * 3 + 1)
        w = None if weight is None else torch.from_numpy((r.rand(21) < 0.6).astype(np.float32)) if weight == "mixed" else torch.zeros(21)
        before = tuple(t.clone() for t in on.tensors())
        ref = onr.stats_update_ref(x.numpy(), None if w is None else w.numpy(), float(on.count[0]), on.mean.numpy().copy(), on.m2.numpy().copy())
        on.update(x, w)
        if weight == "zero":
            assert ref is None and all(torch.equal(a, b) for a, b in zip(before, on.tensors()))
            continue
        nb = ref[0] - float(before[0][0])
        X = np.maximum(np.abs(x.numpy()).max(0), np.abs(before[1].numpy()))
        assert float(on.count[0]) == ref[0]
        assert (np.abs(on.mean.numpy() - ref[1]) <= onr.mean_bound(nb, 1, X)).all()
        assert (np.abs(on.m2.numpy() - ref[2]) <= onr.m2_bound(nb, 1, X, before[2].numpy())).all()
    a, b = ObsNorm(S, 1e-2), ObsNorm(S, 1e-2)
    x = torch.from_numpy(r.standard_normal((9, S)).astype(np.float32))
    w = torch.tensor([1, 0, 1, 1, 0, 1, 1, 1, 0.0])
    a.update(x, w)
    x[1] = float("nan")
    x[4, 7] = float("inf")
    b.update(x, w)
    assert all(torch.equal(s, t) for s, t in zip(a.tensors(), b.tensors())) and float(a.count[0]) == 6


def _dyadic_pair(seed):
    """A base batch and its image under x -> a_k x + c_k per state column, both exact: the base states are multiples of 1/16 in [-4, 4], 16
    rows count, a_k = 2^e with e over -7 .. 7 (0.0078 .. 128: it covers 1e-2 .. 1e2), c_k multiples of 1/4 in [-8, 8].  The statistics are rounded to
    fp32 by design, so two normalisers agree to better than 2^-24 |mean| / sigma only where that rounding commutes with the map - here:
    every mean is a multiple of 2^-15 below 2^10, exact in fp32 (and so is every state, a multiple of 2^-11), and a power of two passes through sqrt, the reciprocal and the rounding."""
    g = torch.Generator().manual_seed(seed)
    R = 19
    grid = lambda *shape: (torch.randint(-64, 65, shape, generator=g).double() / 16)
    st, ns = grid(R, N, S), grid(R, N, S)
    ac = torch.rand(R, N, A, generator=g).double() * 0.8
    rw = torch.rand(R, N, generator=g).double() * 5
    w = torch.ones(R, dtype=torch.float64)
    w[[2, 9, 18]] = 0
    a = 2.0 ** ((torch.arange(S) * 4) % 15 - 7).double()
    c = torch.randint(-32, 33, (S,), generator=g).double() / 4
    return (st, ac, ns, rw, w), (st * a + c, ac, ns * a + c, rw, w), a


def test_invariance_under_a_per_column_affine_map():
    """The property the feature exists for: two float64 policies of one seed, one batch - but one sees every state column mapped
    x -> a_k x + c_k, a_k over four decades.  After one update the actors' outputs on their own inputs and the critic losses agree to 1e-9
    with obs_norm, and differ by more than 1e-3 without."""
    base, mapped, a = _dyadic_pair(17)
    sd = base[0][:, 0][base[4] != 0].std(0, unbiased=False)
    assert float(a.min()) <= 1e-2 and float(a.max()) >= 1e2 and float(sd.min()) >= 1e-2 / float(a.min())       # no column at the floor
    for kw, close in ((dict(obs_norm=True), True), ({}, False)):
        pa, pb = _policy(double=True, **kw), _policy(double=True, **kw)
        la = pa.train_on_batch(*base)
        lb = pb.train_on_batch(*mapped)
        with torch.no_grad():
            d_act = (pa.act(base[0]) - pb.act(mapped[0])).abs().max().item()
        d_loss = max(abs(x.item() - y.item()) for x, y in zip(la[1:], lb[1:]))
        print(f"\nOBSNORM invariance | obs_norm {close} | actor outputs differ by {d_act:.3e}, critic losses by {d_loss:.3e}")
        if close:
            assert d_act <= 1e-9 and d_loss <= 1e-9, (d_act, d_loss)
            assert float(pa.obs_norm.count[0]) == 16
        else:
            assert d_act > 1e-3 and d_loss > 1e-3, (d_act, d_loss)


def test_acting_copy_acts_as_the_normalised_actor():
    """act() on raw observations and the acting copy's plain forward are one function: the first layer through the folded fp32 weights
    against explicit normalisation in fp64 within obsnorm_ref.preactivation_bound"""
    p = _policy(obs_norm=True)
    for k in range(3):
        p.train_on_batch(*_batch(40 + k))
    x = _batch(77)[0][:, 0]
    (w1, b1), _, _ = p.acting_layers()
    folded = (x.double() @ w1.double().t() + b1.double()).numpy()
    on = p.obs_norm
    xn = (x.double() - on.mean32.double()) * on.inv32.double()
    explicit = (xn @ p.actor.l1.weight.data.double().t() + p.actor.l1.bias.data.double()).numpy()
    bound = onr.preactivation_bound(w1.numpy(), x.numpy(), on.mean32.numpy())
    assert (np.abs(folded - explicit) <= bound).all(), (np.abs(folded - explicit) / bound).max()
    assert torch.equal(p.select_action(x), p.actor(on.normalize(x)))
    one = p.select_action(x[0].numpy())
    assert one.shape == (A,) and np.allclose(one, p.select_action(x)[0].numpy(), atol=1e-6)


@pytest.mark.parametrize("td3", [False, True], ids=["ddpgfd", "td3fd"])
def test_unset_feature_is_the_policy_without_the_arguments(td3):
    """obs_norm=False: three updates leave every parameter bit equal to a policy built without the arguments, nothing new exists"""
    pa, pb = _policy(td3), _policy(td3, obs_norm=False, obs_norm_eps=1e-2, obs_norm_freeze_after=None)
    z = torch.randn(2 * 14, A, generator=torch.Generator().manual_seed(1))
    for k in range(3):
        st, ac, ns, rw, w = _batch(60 + k)
        extra = dict(target_noise=z) if td3 else {}
        la, lb = pa.train_on_batch(st, ac, ns, rw, w, **extra), pb.train_on_batch(st, ac, ns, rw, w, **extra)
        assert all(torch.equal(x, y) for x, y in zip(la, lb))
    for name in pa._flat_params:
        assert torch.equal(pa._flat_params[name], pb._flat_params[name]), name
    assert pb.obs_norm is None and pb.acting_flat() is pb._flat_params["actor"]
    assert pb.acting_layers()[0][0].data_ptr() == pb.actor.l1.weight.data_ptr()


def test_freeze_stops_the_statistics_and_not_the_training():
    # the gate itself, on a count held in a tensor as a capturable policy's is: open below N, closed from N on
    on = ObsNorm(S, 1e-2, freeze_after=3)
    x = _batch(8)[0][:, 0]
    for it, count in ((torch.tensor(0), 14), (torch.tensor([2]), 28), (torch.tensor(3), 28), (7, 28)):
        on.update(x, None, it)
        assert float(on.count[0]) == count
    p = _policy(td3=True, obs_norm=True, obs_norm_freeze_after=2)
    seen = []
    for k in range(4):
        before = p._flat_params["critic"].clone()
        p.train_on_batch(*_batch(80 + k))
        seen.append(tuple(t.clone() for t in p.obs_norm.tensors()))
        assert not torch.equal(before, p._flat_params["critic"])
    assert float(seen[0][0][0]) == 11 and float(seen[1][0][0]) == 22
    assert not torch.equal(seen[0][1], seen[1][1])
    for later in seen[2:]:
        assert all(torch.equal(x, y) for x, y in zip(seen[1], later))
    # the acting copy keeps following the actor (TD3fD's steps on every second update)
    wf = p.obs_norm.fold(p.actor.l1.weight.data, p.actor.l1.bias.data)
    assert torch.equal(p.acting_layers()[0][0], wf[0]) and torch.equal(p.acting_layers()[0][1], wf[1])
    assert torch.equal(p.acting_layers()[2][0], p.actor.l3.weight.data)


def test_checkpoint_round_trip(tmp_path):
    p = _policy(obs_norm=True, obs_norm_eps=0.05, obs_norm_freeze_after=9)
    for k in range(2):
        p.train_on_batch(*_batch(20 + k))
    prefix = str(tmp_path / "ck")
    p.save(prefix)
    assert (tmp_path / "ck_obs_norm").exists()
    q = _policy(seed=9, obs_norm=True)
    q.load(prefix)
    assert all(torch.equal(x, y) for x, y in zip(p.obs_norm.tensors(), q.obs_norm.tensors()))
    assert q.obs_norm.eps == 0.05 and q.obs_norm.freeze_after == 9
    assert torch.equal(p.acting_flat(), q.acting_flat()) and torch.equal(p._flat_params["actor"], q._flat_params["actor"])
    x = _batch(5)[0][:, 0]
    assert torch.equal(p.select_action(x), q.select_action(x))
    # a missing statistics file is refused - the weights mean nothing without it - before anything is loaded
    (tmp_path / "ck_obs_norm").unlink()
    r = _policy(seed=11, obs_norm=True)
    before = r._flat_params["actor"].clone()
    with pytest.raises(FileNotFoundError, match="_obs_norm"):
        r.load(prefix)
    assert torch.equal(before, r._flat_params["actor"])
    # ... and what is left is a reference-style 4-file checkpoint, which a policy without the feature loads as ever - and writes
    plain = _policy(seed=13)
    plain.load(prefix)
    assert torch.equal(plain._flat_params["actor"], p._flat_params["actor"])
    plain.save(str(tmp_path / "plain"))
    assert sorted(f.name for f in tmp_path.glob("plain*")) == ["plain_actor", "plain_actor_optimizer", "plain_critic", "plain_critic_optimizer"]


def test_argument_refusals(monkeypatch):
    for kw in (dict(obs_norm=True, obs_norm_eps=0.0), dict(obs_norm=True, obs_norm_eps=-1.0), dict(obs_norm=True, obs_norm_eps=float("nan")),
               dict(obs_norm=True, obs_norm_eps=float("inf")), dict(obs_norm=True, obs_norm_freeze_after=0), dict(obs_norm=True, obs_norm_freeze_after=2.5),
               dict(obs_norm=True, obs_norm_freeze_after=True), dict(obs_norm_eps=0.1), dict(obs_norm_freeze_after=5), dict(obs_norm=False, obs_norm_eps=0.1)):
        for cls in (DDPGfD, TD3fD):
            with pytest.raises(ValueError, match="obs_norm"):
                cls(S, A, 0.8, N, hidden=HIDDEN, **kw)
    assert _policy(obs_norm=True, obs_norm_eps=0.5, obs_norm_freeze_after=1).obs_norm.eps == 0.5
    # per-rank statistics under shared weights: not with more than one rank
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="more than one rank"):
        DDPGfD(S, A, 0.8, N, hidden=HIDDEN, obs_norm=True)
    DDPGfD(S, A, 0.8, N, hidden=HIDDEN)
