"""Prioritized episode replay without a GPU: DeviceEpisodeReplay(device="cpu").sample_prioritized - the torch path, the checker of
kr_sample_windows_prioritized - against the plain loops of tests/priority_ref.py; the priority column through the torch commit and through
load; and the argument checks that must not need a device."""
import types
import zlib

import numpy as np
import pytest
import torch

from kinovagrasping_amd.replay import PRIO_ONE, DeviceEpisodeReplay
from tests import priority_ref as pr

H, N = pr.H, pr.N_STEPS
W = H - N
BETAS = (1.0, 0.4, 0.0)


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def to_replay(ring):
    """a CPU DeviceEpisodeReplay holding the ring dict's rows, counters and priorities"""
    cap = ring["capacity"]
    rep = DeviceEpisodeReplay(4, cap, horizon=H, n_steps=N, device="cpu")
    rep.enable_priorities()
    for name, f in (("ep_state", "state"), ("ep_next", "next"), ("ep_action", "action"), ("ep_reward", "reward"), ("ep_not_done", "not_done")):
        getattr(rep, name)[:cap] = torch.from_numpy(ring[f])
    rep.ep_len[:cap] = torch.from_numpy(ring["ep_len"])
    rep.ep_prio.view(torch.int32)[:cap] = torch.from_numpy(ring["ep_prio"].view(np.int32))
    rep._count.fill_(ring["count"])
    rep._head.fill_(ring["head"])
    return rep


def assert_same(got, ref, what):
    """sample_prioritized's tuple (6 tensors + picked) against priority_ref's: every bit, the weight column against the reference's float64
    power rounded once to fp32 (the torch path takes the power in float64 too)"""
    assert got[-1].dtype == torch.int32 and np.array_equal(got[-1].numpy(), ref[6]), (what, got[-1].tolist(), ref[6].tolist())
    for k, name in enumerate(("state", "action", "next_state", "reward", "not_done")):
        g = got[k].numpy()
        assert g.dtype == np.float32 and g.shape == ref[k].shape, (what, name, g.shape, ref[k].shape)
        assert g.tobytes() == ref[k].tobytes(), f"{what}: {name} differs"
    w = got[5].numpy()
    assert w.dtype == np.float32 and w.tobytes() == ref[5].astype(np.float32).tobytes(), (what, w, ref[5])
    assert ((w >= 0) & (w <= 1)).all()


CASES = [(c, h, name) for c, h in pr.COUNT_HEAD for name in ("equal", "extremes", "random", "near_one")]


@pytest.mark.parametrize("count,head,pattern", CASES, ids=[f"count{c}-head{h}-{p}" for c, h, p in CASES])
def test_torch_path_equals_the_reference(count, head, pattern):
    """rings of 8 slots at count 0, 1, 2, 5, 8 and heads that wrap the eligible range; tables of equal priorities, of 1 and 2^32 - 1 side by side
    (and a stored 0), random ones; u_ep on 0, on 1 - 2^-24 and on and beside the prefix-sum boundaries; one ring and two rings at batch_agent
    0, 4 and 6; beta 1, 0.4 and 0: every output and picked"""
    r = _rng("cpu", count, head, pattern)
    agent = pr.make_ring(pr.CAP, H, count, head, pr.ring_lens(H, N), pr.priority_patterns(pr.CAP, r)[pattern], r)
    expert = pr.make_ring(5, H, 4, 2, [N + 2, H, N + 1, H, N + 3], [3 * PRIO_ONE, 1, PRIO_ONE // 7, pr.U32_MAX, 5], r)
    ra, re = to_replay(agent), to_replay(expert)
    for shift, beta in enumerate(BETAS):
        ue = pr.episode_uniforms(pr.B, agent, shift)
        ue[pr.B_AGENT:] = pr.episode_uniforms(pr.B - pr.B_AGENT, expert, shift)
        us = pr.start_uniforms(pr.B, W, shift)
        u = torch.from_numpy(np.concatenate([ue, us.reshape(-1)]))
        got = ra.sample_prioritized(None, pr.B, beta=beta, uniforms=u)
        assert_same(got, pr.sample_prioritized_ref(pr.B, H, N, agent, ue, us, beta), f"one ring, beta {beta}")
        for prob, b_agent in ((1.0, 0), (0.3, 4), (0.0, pr.B)):
            assert int(pr.B * (1 - prob)) == b_agent
            got = ra.sample_prioritized(re, pr.B, prob, beta=torch.tensor([beta]), uniforms=u)
            ref = pr.sample_prioritized_ref(pr.B, H, N, agent, ue, us, beta, expert=expert, batch_agent=b_agent)
            assert_same(got, ref, f"two rings, batch_agent {b_agent}, beta {beta}")
            if count >= 2:                       # the newest episode is never read
                assert all(p[0] != (head - 1) % pr.CAP for p in ref[8][:b_agent])
            if count < 2:
                assert not got[5][:b_agent * W].any()


@pytest.mark.parametrize("count,head", pr.COUNT_HEAD)
def test_equal_priorities_pick_uniformly_with_unit_weights(count, head):
    """a table of equal priorities: slot b takes age min(hi - 1, floor((double)ue * hi)) over the hi = count - 1 eligible episodes, and every
    real row's weight is exactly 1 whatever beta is"""
    r = _rng("equal", count, head)
    for value in (1, PRIO_ONE, pr.U32_MAX, 0):
        agent = pr.make_ring(pr.CAP, H, count, head, [H] * pr.CAP, np.full(pr.CAP, value, np.uint32), r)
        ra = to_replay(agent)
        ue = np.asarray([0.0, pr.TOP, 0.5, 0.37, 0.99, 1.0 / 3], np.float32)
        u = torch.from_numpy(np.concatenate([ue, pr.start_uniforms(pr.B, W, 0).reshape(-1)]))
        got = ra.sample_prioritized(None, pr.B, beta=0.7, uniforms=u)
        hi = max(count - 1, 1)
        want = [(head - count + min(hi - 1, int(float(x) * hi))) % pr.CAP for x in ue]
        assert got[-1].tolist() == want, (value, got[-1].tolist(), want)
        weight = got[5].numpy()
        assert (weight == (1.0 if count >= 2 else 0.0)).all()                  # (every episode has H - N real rows here)


def test_torch_commit_writes_the_entry_priority_into_the_commit_rules_slots():
    """end_episodes on CPU tensors: kept env i's slot (head + rank - 1) % capacity gets max(prio_max, 1) - priority_ref.commit_priorities_ref -,
    every other slot AND the trash row keep what they held; a ring without priorities has no column at all"""
    n, cap = 5, 4
    for top in (3 * PRIO_ONE + 5, 0, pr.U32_MAX):
        rep = DeviceEpisodeReplay(n, cap, horizon=H, n_steps=N, device="cpu")
        assert rep.ep_prio is None and rep.prio_max is None
        rep.enable_priorities()
        assert rep.ep_prio.dtype == torch.uint32 and rep.ep_prio.shape == (cap + 1,) and rep.prio_max.shape == (1,)
        assert rep.priorities().tolist() == [PRIO_ONE] * (cap + 1) and rep.priority_max() == PRIO_ONE
        before = np.array([11, 12, 13, 14, 15], np.uint32)
        rep.ep_prio.view(torch.int32).copy_(torch.from_numpy(before.view(np.int32)))
        rep.prio_max.view(torch.int32).copy_(torch.from_numpy(np.array([top], np.uint32).view(np.int32)))
        rep._head.fill_(3)
        rep._count.fill_(3)
        rep.cur_len.copy_(torch.tensor([H, 2, H, H, 1]))                         # envs 1 and 4: too short to keep
        mask = torch.tensor([True, True, True, False, True])
        keep = (mask & (rep.cur_len - N > 1)).numpy().astype(np.uint8)
        rank = np.cumsum(keep != 0).astype(np.int64)
        want = pr.commit_priorities_ref(keep, rank, 3, cap, top, before.astype(np.int64).copy())
        assert int(rep.end_episodes(mask)) == 2
        assert rep.priorities().tolist() == want.tolist() and want.tolist() == [max(top, 1), 12, 13, max(top, 1), 15]
        assert rep.priority_max() == top and rep.head == 1 and rep.count == 4


def test_load_gives_loaded_episodes_the_rings_prio_max_and_save_writes_no_priorities(tmp_path):
    """save leaves the bundle's file list as it is without priorities; load tags every loaded episode with the loading ring's prio_max"""
    src = DeviceEpisodeReplay(3, 8, horizon=H, n_steps=N, device="cpu")
    plain = DeviceEpisodeReplay(3, 8, horizon=H, n_steps=N, device="cpu")
    src.enable_priorities()
    g = torch.Generator().manual_seed(3)
    for rep in (src, plain):
        g.manual_seed(3)
        for _ in range(H):
            rep.add(torch.rand(3, 82, generator=g), torch.rand(3, 4, generator=g), torch.rand(3, 82, generator=g), torch.rand(3, generator=g),
                    torch.zeros(3, dtype=torch.bool))
        rep.end_episodes(torch.ones(3, dtype=torch.bool))
    src.save(tmp_path / "a")
    plain.save(tmp_path / "b")
    names = sorted(p.name for p in (tmp_path / "b").iterdir())
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == names
    for name in names:
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    dst = DeviceEpisodeReplay(2, 8, horizon=H, n_steps=N, device="cpu")
    dst.enable_priorities()
    dst.prio_max.view(torch.int32).fill_(5 * PRIO_ONE + 1)
    dst.load(tmp_path / "a")
    assert dst.count == 3 and dst.priorities().tolist() == [5 * PRIO_ONE + 1] * 3 + [PRIO_ONE] * 6
    bare = DeviceEpisodeReplay(2, 8, horizon=H, n_steps=N, device="cpu")
    bare.load(tmp_path / "a")
    assert bare.ep_prio is None and bare.count == 3


def test_arguments_are_checked_before_a_device_is_needed():
    """prioritized together with balanced, a prioritized trainer on a host ring, sample_prioritized / update_priorities on rings without
    priorities, a beta of the wrong kind, set_per_beta on a trainer without priorities, a ring too large for exact sums: ValueError, all of
    them on a machine without a GPU"""
    from kinovagrasping_amd.pipeline import AsyncTrainer, GraphedTrainer
    eng = types.SimpleNamespace(gen=None)
    rep = DeviceEpisodeReplay(2, 8, horizon=H, n_steps=N, device="cpu")
    for cls in (GraphedTrainer, AsyncTrainer):
        with pytest.raises(ValueError, match="balanced"):
            cls(None, None, rep, eng, prioritized=True, balanced=True)
        with pytest.raises(ValueError, match="device ring"):
            cls(None, None, rep, eng, prioritized=True)
    with pytest.raises(ValueError, match="launch_synchronous"):
        AsyncTrainer(None, None, rep, eng, prioritized=True, launch_synchronous=True)
    assert rep.ep_prio is None
    with pytest.raises(ValueError, match="priorities"):
        rep.sample_prioritized(None, 4)
    with pytest.raises(ValueError, match="priorities"):
        rep.update_priorities(None, None, None, None, None, torch.zeros(4, dtype=torch.int32))
    with_prio = DeviceEpisodeReplay(2, 8, horizon=H, n_steps=N, device="cpu")
    with_prio.enable_priorities()
    with pytest.raises(ValueError, match="priorities"):
        with_prio.sample_prioritized(rep, 4)
    with pytest.raises(ValueError, match="beta"):
        with_prio.sample_prioritized(None, 4, beta=torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match="beta"):
        with_prio.sample_prioritized(None, 4, beta=torch.tensor([1.0], dtype=torch.float64))
    with pytest.raises(ValueError, match="device rings"):
        with_prio.update_priorities(None, None, None, None, None, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="prioritized"):
        GraphedTrainer.set_per_beta(types.SimpleNamespace(prioritized=False), 0.5)
    import kinovagrasping_amd.replay as replay_module
    big = types.SimpleNamespace(ep_prio=None, capacity=replay_module.PRIO_MAX_CAPACITY + 1)
    with pytest.raises(ValueError, match="at most"):
        DeviceEpisodeReplay.enable_priorities(big)
