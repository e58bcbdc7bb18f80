"""The class-balanced replay sampler without a GPU: DeviceEpisodeReplay(device="cpu").sample_balanced - the torch path, the checker of
kr_sample_windows_balanced - against the plain loops of tests/balanced_ref.py, bit for bit; the class column through the torch commit and
through save / load; and the argument checks of the trainers and of curriculum.run_stage that must not need a device."""
import json
import types
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

from kinovagrasping_amd.replay import CLASS_SIDECAR, DeviceEpisodeReplay
from tests import balanced_ref as br

H = 12
W = H - br.N_STEPS


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def to_replay(ring, n_classes, H=H):
    """a CPU DeviceEpisodeReplay holding the ring dict's rows, counters and tags"""
    cap = ring["capacity"]
    rep = DeviceEpisodeReplay(4, cap, horizon=H, n_steps=br.N_STEPS, device="cpu")
    rep.set_env_classes(torch.zeros(4, dtype=torch.int32), [f"c{k}" for k in range(n_classes)])
    for name, f in (("ep_state", "state"), ("ep_next", "next"), ("ep_action", "action"), ("ep_reward", "reward"), ("ep_not_done", "not_done")):
        getattr(rep, name)[:cap] = torch.from_numpy(ring[f])
    rep.ep_len[:cap] = torch.from_numpy(ring["ep_len"])
    rep.ep_class[:cap] = torch.from_numpy(ring["ep_class"])
    rep._count.fill_(ring["count"])
    rep._head.fill_(ring["head"])
    return rep


def assert_same(got, ref, what):
    """sample_balanced's tuple (6 tensors + picked) against balanced_ref's, in every bit"""
    for k, name in enumerate(("state", "action", "next_state", "reward", "not_done", "weight")):
        g = got[k].numpy()
        assert g.dtype == np.float32 and g.shape == ref[k].shape, (what, name, g.shape, ref[k].shape)
        assert g.tobytes() == ref[k].tobytes(), f"{what}: {name} differs"
    assert got[-1].dtype == torch.int32 and np.array_equal(got[-1].numpy(), ref[6]), (what, got[-1].tolist(), ref[6].tolist())


SMALL = br.small_cases()


@pytest.mark.parametrize("count,head,nc,pattern,tags", SMALL, ids=[f"count{c[0]}-head{c[1]}-nc{c[2]}-{c[3]}" for c in SMALL])
def test_torch_path_equals_the_reference(count, head, nc, pattern, tags):
    """one ring (expert=None) and two rings at batch_agent 0, between and batch (prob 1, 0.3, 0), the uniforms on 0, on the values whose
    product with a class's population lands on m - 1 or beside an integer, and on nextafter(1, 0); rotation and draw move the classes"""
    r = _rng("cpu", count, head, nc, pattern)
    agent = br.make_ring(br.CAP, H, count, head, br.ring_lens(H, br.N_STEPS), tags, r)
    expert = br.make_ring(5, H, 4, 2, [br.N_STEPS + 2, H, br.N_STEPS + 1, H, br.N_STEPS + 3], [0, nc - 1, -1, 0, nc - 1], r)
    ra, re = to_replay(agent, nc), to_replay(expert, nc)
    pops = br.class_populations(agent, nc) + br.class_populations(expert, nc) + [max(count - 1, 1)]
    for shift, rotation, draw in ((0, 0, None), (1, 2, 3), (3, -4, 0), (5, 1, 2 ** 40 + 1)):
        ue, us = br.episode_uniforms(br.B, pops, shift), br.start_uniforms(br.B, W, shift)
        u = torch.from_numpy(np.concatenate([ue, us.reshape(-1)]))
        dr = None if draw is None else torch.tensor([draw])
        got = ra.sample_balanced(None, br.B, uniforms=u, draw=dr, rotation=rotation)
        assert_same(got, br.sample_balanced_ref(br.B, H, br.N_STEPS, agent, ue, us, nc, rotation, draw), f"one ring, shift {shift}")
        for prob, b_agent in ((1.0, 0), (0.3, 4), (0.0, br.B)):
            assert int(br.B * (1 - prob)) == b_agent
            got = ra.sample_balanced(re, br.B, prob, uniforms=u, draw=dr, rotation=rotation)
            ref = br.sample_balanced_ref(br.B, H, br.N_STEPS, agent, ue, us, nc, rotation, draw, expert=expert, batch_agent=b_agent)
            assert_same(got, ref, f"two rings, batch_agent {b_agent}, shift {shift}")
            if count >= 2:                       # the newest episode is never read, from whichever rule the slot came
                assert all(p[0] != (head - 1) % br.CAP for p in ref[8][:b_agent])


def test_the_reference_takes_the_fallback_and_the_last_of_a_class():
    """what the case list is for, by the reference alone: a class whose only episode is the newest falls back (m_c = 0), u = nextafter(1, 0)
    takes the youngest eligible episode of its class, a -1 tag is in no class"""
    agent = br.make_ring(br.CAP, H, 8, 3, br.ring_lens(H, br.N_STEPS), br.tag_patterns(3, 8, 3)["newest_only"], _rng("ref"))
    top = np.float32(np.nextafter(np.float32(1.0), np.float32(0.0)))
    picks = br.pick_ref(agent, 3, [top] * 3, 3)
    assert [p[1] for p in picks] == [0, 1, 2] and picks[2][2] == 0 and picks[0][2] + picks[1][2] == 7
    first = (3 - 8) % br.CAP
    assert picks[0][0] == (first + 6) % br.CAP and picks[1][0] == (first + 5) % br.CAP         # ages 0 .. 6 alternate 0, 1: the youngest of each
    assert picks[2][0] == (first + 6) % br.CAP                                                # fallback: k = hi - 1 over all eligible
    unknown = br.make_ring(br.CAP, H, 8, 0, br.ring_lens(H, br.N_STEPS), br.tag_patterns(2, 8, 0)["unknown"], _rng("ref"))
    assert sum(br.class_populations(unknown, 2)) == 6


@pytest.mark.parametrize("count,head", [(0, 0), (1, 1), (5, 5), (8, 3)])
def test_one_class_is_sample_mixed(count, head):
    """property (a): n_classes == 1 and every tag 0 - the batch of sample_mixed's torch path in every bit"""
    r = _rng("one", count, head)
    agent = br.make_ring(br.CAP, H, count, head, br.ring_lens(H, br.N_STEPS), np.zeros(br.CAP, np.int32), r)
    expert = br.make_ring(5, H, 4, 2, [br.N_STEPS + 2, H, br.N_STEPS + 1, H, br.N_STEPS + 3], np.zeros(5, np.int32), r)
    ra, re = to_replay(agent, 1), to_replay(expert, 1)
    for shift in (0, 2):
        ue, us = br.episode_uniforms(br.B, [max(count - 1, 1), 3], shift), br.start_uniforms(br.B, W, shift)
        u = torch.from_numpy(np.concatenate([ue, us.reshape(-1)]))
        for prob in (1.0, 0.3, 0.0):
            got, want = ra.sample_balanced(re, br.B, prob, uniforms=u, rotation=shift), ra.sample_mixed(re, br.B, prob, uniforms=u)
            assert len(got) == len(want) + 1
            for g, w_ in zip(got, want):
                assert g.numpy().tobytes() == w_.numpy().tobytes()


def test_class_shares_differ_by_at_most_one_and_rotate():
    """property (b), counted from `picked` on a skewed ring (16 episodes: 11 of class 0, 3 of class 1, 2 of class 2): within a segment the
    classes' slot counts differ by at most 1; over n_classes consecutive draws every class gets exactly the segment's length"""
    cap, nc, batch = 16, 3, 10
    tags = np.array([0] * 11 + [1] * 3 + [2] * 2, np.int32)[_rng("skew").permutation(16)]
    tags[15] = 0                                                              # (head 0: slot 15 is the newest; every class stays eligible)
    agent = br.make_ring(cap, H, 16, 0, [H] * cap, tags, _rng("skew", 1))
    expert = br.make_ring(cap, H, 16, 0, [H] * cap, tags[::-1].copy(), _rng("skew", 2))
    assert min(br.class_populations(agent, nc)) > 0 and min(br.class_populations(expert, nc)) > 0
    ra, re = to_replay(agent, nc), to_replay(expert, nc)
    b_agent = int(batch * 0.7)
    totals = np.zeros((2, nc), np.int64)
    gen = torch.Generator().manual_seed(5)
    for draw in range(nc):
        picked = ra.sample_balanced(re, batch, 0.3, draw=torch.tensor([draw]), generator=gen)[-1].numpy()
        for k, (seg, tg) in enumerate(((picked[:b_agent], tags), (picked[b_agent:], tags[::-1]))):
            per = np.bincount(tg[seg], minlength=nc)
            assert per.max() - per.min() <= 1 and per.sum() == len(seg), (draw, k, per)
            totals[k] += per
    assert (totals[0] == b_agent).all() and (totals[1] == batch - b_agent).all(), totals


def test_torch_commit_tags_the_slots_of_the_commit_rule():
    """end_episodes on CPU tensors: kept env i's class lands in slot (head + rank - 1) % capacity - balanced_ref.commit_classes_ref -, every
    other slot keeps -1 (the trash row aside); a ring without classes has no column at all"""
    n, cap = 5, 4
    rep = DeviceEpisodeReplay(n, cap, horizon=H, n_steps=br.N_STEPS, device="cpu")
    assert rep.ep_class is None
    env_class = torch.tensor([2, 0, 1, 2, 0], dtype=torch.int64)
    rep.set_env_classes(env_class, ["a", "b", "c"])
    assert rep.ep_class.dtype == torch.int32 and rep.ep_class.shape == (cap + 1,) and (rep.ep_class == -1).all()
    rep._head.fill_(3)
    rep._count.fill_(3)
    rep.cur_len.copy_(torch.tensor([H, 2, H, H, 1]))                         # envs 1 and 4: too short to keep
    mask = torch.tensor([True, True, True, False, True])
    keep = (mask & (rep.cur_len - br.N_STEPS > 1)).numpy().astype(np.uint8)
    rank = np.cumsum(keep != 0).astype(np.int64)
    want = br.commit_classes_ref(keep, rank, 3, cap, env_class.numpy().astype(np.int32), np.full(cap, -1, np.int32))
    assert int(rep.end_episodes(mask)) == 2
    assert np.array_equal(rep.ep_class[:cap].numpy(), want) and want.tolist() == [1, -1, -1, 2]
    assert rep.head == 1 and rep.count == 4


def _filled(names, env_class, episodes_of):
    rep = DeviceEpisodeReplay(len(env_class), 8, horizon=H, n_steps=br.N_STEPS, device="cpu")
    if names is not None:
        rep.set_env_classes(torch.tensor(env_class), names)
    g = torch.Generator().manual_seed(3)
    for envs in episodes_of:
        mask = torch.zeros(len(env_class), dtype=torch.bool)
        mask[list(envs)] = True
        for _ in range(H):
            rep.add(torch.rand(len(env_class), 82, generator=g), torch.rand(len(env_class), 4, generator=g), torch.rand(len(env_class), 82, generator=g),
                    torch.rand(len(env_class), generator=g), torch.zeros(len(env_class), dtype=torch.bool))
        rep.end_episodes(mask)
    return rep


def test_save_and_load_carry_the_classes_through_the_sidecar(tmp_path):
    """save with classes writes the reference bundle's files - byte-identical to the same ring's without classes - and the sidecar; load
    maps the sidecar's NAMES onto the loading ring's classes (a name it does not know: -1), class_id overrides, no classes: no column"""
    rounds = [(0, 1, 2), (2,), (1, 2)]
    with_classes = _filled(["CubeS", "CylinderB", "BowlM"], [0, 1, 2], rounds)
    plain = _filled(None, [0, 1, 2], rounds)
    with_classes.save(tmp_path / "a")
    plain.save(tmp_path / "b")
    names = sorted(p.name for p in (tmp_path / "b").iterdir())
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(names + [CLASS_SIDECAR])
    for name in names:
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    side = json.loads((tmp_path / "a" / CLASS_SIDECAR).read_text())
    assert side == {"class_names": ["CubeS", "CylinderB", "BowlM"], "episode_class": [0, 1, 2, 2, 1, 2]}
    other = DeviceEpisodeReplay(2, 8, horizon=H, n_steps=br.N_STEPS, device="cpu")
    other.set_env_classes(None, ["BowlM", "CubeS"])                         # another order, and no CylinderB
    other.load(tmp_path / "a")
    assert other.count == 6 and other.ep_class[:6].tolist() == [1, -1, 0, 0, -1, 0] and (other.ep_class[6:] == -1).all()
    for f in ("ep_state", "ep_action", "ep_reward"):
        assert torch.equal(getattr(other, f)[:6], getattr(with_classes, f)[:6])
    other.load(tmp_path / "b")                                               # no sidecar: unknown; the ring wraps
    assert other.ep_class[[6, 7, 0, 1]].tolist() == [-1] * 4
    other.load(tmp_path / "a", class_id=1)
    assert other.ep_class[[4, 5, 6, 7, 0, 1]].tolist() == [1] * 6 and other.ep_class[[2, 3]].tolist() == [-1, -1]
    with pytest.raises(ValueError):
        other.load(tmp_path / "a", class_id=2)
    bare = DeviceEpisodeReplay(2, 8, horizon=H, n_steps=br.N_STEPS, device="cpu")
    bare.load(tmp_path / "a")
    assert bare.ep_class is None and bare.count == 6


def test_arguments_are_checked_before_a_device_is_needed(tmp_path):
    """run_stage(free_running=True) without a start pool, a trainer with balanced=True on rings without classes, sample_balanced without
    classes and set_env_classes with a wrong tensor: ValueError, all of them on a machine without a GPU"""
    from kinovagrasping_amd import curriculum
    from kinovagrasping_amd.pipeline import AsyncTrainer, GraphedTrainer
    plan = curriculum.experiment_plan(2, root=tmp_path)
    with pytest.raises(ValueError, match="starts_per_env"):
        curriculum.run_stage(plan, None, free_running=True, starts_per_env=0)
    with pytest.raises(ValueError, match="free_running"):
        curriculum.run_stage(plan, None, budget_ms=50.0)
    eng = types.SimpleNamespace(gen=None)
    rep = DeviceEpisodeReplay(2, 8, horizon=H, n_steps=br.N_STEPS, device="cpu")
    for cls in (GraphedTrainer, AsyncTrainer):
        with pytest.raises(ValueError, match="classes"):
            cls(None, None, rep, eng, balanced=True)
    tagged = DeviceEpisodeReplay(2, 8, horizon=H, n_steps=br.N_STEPS, device="cpu")
    tagged.set_env_classes(torch.tensor([0, 1]), ["a", "b"])
    with pytest.raises(ValueError, match="classes"):
        GraphedTrainer(None, None, tagged, eng, balanced=True, expert_replay=rep)
    with pytest.raises(ValueError, match="classes"):
        rep.sample_balanced(None, 4)
    with pytest.raises(ValueError, match="classes"):
        tagged.sample_balanced(rep, 4)
    for bad, names in ((torch.tensor([0, 2]), ["a", "b"]), (torch.tensor([0.0, 1.0]), ["a", "b"]), (torch.tensor([0]), ["a", "b"]),
                       (torch.tensor([0, 1]), []), (torch.tensor([0, 0]), ["a", "a"]), (torch.tensor([0, 0]), [str(k) for k in range(65)])):
        with pytest.raises(ValueError):
            rep.set_env_classes(bad, names)
    assert rep.ep_class is None
