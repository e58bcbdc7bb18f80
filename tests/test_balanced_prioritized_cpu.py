"""The class-balanced prioritized replay sampler without a GPU: DeviceEpisodeReplay(device="cpu").sample_balanced_prioritized - the torch path,
the checker of kr_sample_windows_balanced_prioritized - against the plain loops of tests/balprio_ref.py; its two degenerate equalities against
the torch picks of the two samplers it combines; and the argument checks of the sampler, the trainers and curriculum.run_stage that must not
need a device."""
import types
import zlib

import numpy as np
import pytest
import torch

from kinovagrasping_amd.replay import PRIO_ONE, DeviceEpisodeReplay
from tests import balprio_ref as bp
from tests import priority_ref as pr

H, N = bp.H, bp.N_STEPS
W = H - N
BETAS = (1.0, 0.4, 0.0)


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def to_replay(ring, n_classes):
    """a CPU DeviceEpisodeReplay holding the ring dict's rows, counters, tags and priorities"""
    cap = ring["capacity"]
    rep = DeviceEpisodeReplay(4, cap, horizon=H, n_steps=N, device="cpu")
    rep.set_env_classes(torch.zeros(4, dtype=torch.int32), [f"c{k}" for k in range(n_classes)])
    rep.enable_priorities()
    for name, f in (("ep_state", "state"), ("ep_next", "next"), ("ep_action", "action"), ("ep_reward", "reward"), ("ep_not_done", "not_done")):
        getattr(rep, name)[:cap] = torch.from_numpy(ring[f])
    rep.ep_len[:cap] = torch.from_numpy(ring["ep_len"])
    rep.ep_class[:cap] = torch.from_numpy(ring["ep_class"])
    rep.ep_prio.view(torch.int32)[:cap] = torch.from_numpy(ring["ep_prio"].view(np.int32))
    rep._count.fill_(ring["count"])
    rep._head.fill_(ring["head"])
    return rep


def assert_same(got, ref, what):
    """the sampler's tuple (6 tensors + picked) against balprio_ref's: every bit, the weight column against the reference's float64 power
    rounded once to fp32 (the torch path takes the power in float64 too)"""
    assert got[-1].dtype == torch.int32 and np.array_equal(got[-1].numpy(), ref[6]), (what, got[-1].tolist(), ref[6].tolist())
    for k, name in enumerate(("state", "action", "next_state", "reward", "not_done")):
        g = got[k].numpy()
        assert g.dtype == np.float32 and g.shape == ref[k].shape, (what, name, g.shape, ref[k].shape)
        assert g.tobytes() == ref[k].tobytes(), f"{what}: {name} differs"
    w = got[5].numpy()
    assert w.dtype == np.float32 and w.tobytes() == ref[5].astype(np.float32).tobytes(), (what, w, ref[5])
    assert ((w >= 0) & (w <= 1)).all()


CASES = [(c, h, nc) for c, h in bp.COUNT_HEAD for nc in bp.N_CLASSES]


@pytest.mark.parametrize("count,head,nc", CASES, ids=[f"count{c}-head{h}-nc{nc}" for c, h, nc in CASES])
def test_torch_path_equals_the_reference(count, head, nc):
    """rings of 8 slots at every (count, head) of priority_ref's list, 1, 3 and 64 classes; tags cyclic, with an absent class (the fallback), with
    a class whose only member is the newest episode, with -1 and a value >= n_classes; tables of equal priorities, of 1 and 2^32 - 1 side by
    side (and a stored 0), random ones; u_ep on 0, 1 - 2^-24 and on and beside the classes' prefix-sum boundaries; one ring and two rings at
    batch_agent 0, 4 and 6; rotation -5, 0, 7 and a draw; beta 1, 0.4 and 0: every output and picked"""
    saw_fallback = saw_class = False
    for tname, tags in bp.tag_patterns(nc, count, head).items():
        for pname in ("equal", "extremes", "random"):
            r = _rng("cpu", count, head, nc, tname, pname)
            agent = bp.make_ring(bp.CAP, H, count, head, pr.ring_lens(H, N), tags, pr.priority_patterns(bp.CAP, r)[pname], r)
            expert = bp.expert_ring(r, nc)
            ra, re = to_replay(agent, nc), to_replay(expert, nc)
            for shift, (beta, rotation, draw) in enumerate(zip(BETAS, bp.ROTATIONS, (None, 3, 2 ** 40 + 1))):
                rot = rotation + (draw or 0)
                us = pr.start_uniforms(bp.B, W, shift)
                dr = None if draw is None else torch.tensor([draw])
                ue = bp.episode_uniforms(bp.B, agent, nc, rot, shift)
                u = torch.from_numpy(np.concatenate([ue, us.reshape(-1)]))
                got = ra.sample_balanced_prioritized(None, bp.B, beta=beta, uniforms=u, draw=dr, rotation=rotation)
                ref = bp.sample_ref(bp.B, H, N, agent, ue, us, nc, beta, rotation, draw)
                assert_same(got, ref, f"{tname} {pname} one ring, shift {shift}")
                saw_fallback |= any(p[7] == 0 for p in ref[8])
                saw_class |= any(p[7] > 0 for p in ref[8])
                for prob, b_agent in ((1.0, 0), (0.3, 4), (0.0, bp.B)):
                    assert int(bp.B * (1 - prob)) == b_agent
                    ue[b_agent:] = bp.episode_uniforms(bp.B - b_agent, expert, nc, rot, shift)
                    u = torch.from_numpy(np.concatenate([ue, us.reshape(-1)]))
                    got = ra.sample_balanced_prioritized(re, bp.B, prob, beta=torch.tensor([beta]), uniforms=u, draw=dr, rotation=rotation)
                    ref = bp.sample_ref(bp.B, H, N, agent, ue, us, nc, beta, rotation, draw, expert=expert, batch_agent=b_agent)
                    assert_same(got, ref, f"{tname} {pname} two rings, batch_agent {b_agent}, shift {shift}")
                    for p in ref[8][:b_agent]:
                        if p[7] > 0:                 # a slot whose class has eligible episodes takes one of that class
                            assert int(agent["ep_class"][p[0]]) == p[6]
                        if count >= 2:               # the newest episode is never read, from whichever rule the slot came
                            assert p[0] != (head - 1) % bp.CAP
                    if count < 2:
                        assert not got[5][:b_agent * W].any()
    assert (saw_fallback or nc == 1) and (saw_class or count < 2)


@pytest.mark.parametrize("count,head", bp.COUNT_HEAD)
def test_one_class_or_no_known_tag_is_the_prioritized_pick(count, head):
    """n_classes == 1 with every tag 0, and 3 classes with no eligible tag inside [0, 3): slot and weight of every batch slot are
    _pick_prioritized's, in every bit, whatever rotation and draw are"""
    for pname in ("equal", "extremes", "random", "near_one"):
        r = _rng("as prioritized", count, head, pname)
        prio = pr.priority_patterns(bp.CAP, r)[pname]
        ue = torch.from_numpy(pr.episode_uniforms(bp.B, pr.make_ring(bp.CAP, H, count, head, pr.ring_lens(H, N), prio, r), 1))
        for nc, tags in ((1, np.zeros(bp.CAP, np.int32)), (3, np.array([-1, 3, 7, -2, 64, 3, -1, 100], np.int32))):
            rep = to_replay(bp.make_ring(bp.CAP, H, count, head, pr.ring_lens(H, N), tags, prio, r), nc)
            for beta, rotation, d in ((1.0, 0, 0), (0.4, -5, 2), (0.0, 7, 2 ** 40)):
                b = torch.tensor([beta])
                slot, weight = rep._pick_balanced_prioritized(ue, rotation, d, b)
                want_slot, want_weight = rep._pick_prioritized(ue, b)
                assert torch.equal(slot, want_slot) and weight.numpy().tobytes() == want_weight.numpy().tobytes(), (pname, nc, beta)


@pytest.mark.parametrize("head", [0, 5, 11])
def test_equal_priorities_are_the_balanced_pick_with_unit_weights(head):
    """every priority 65536 on a full ring of 16 slots whose 15 eligible episodes are 8, 4, 2 and 1 of classes 0 .. 3, interleaved
    (balprio_ref.power_of_two_ring): ue * (float)m_c is exact in fp32 for m_c a power of two, so floor((double)ue * m_c) is _pick_balanced's j on
    every uniform; the slot is _pick_balanced's and every weight exactly 1 whatever beta is"""
    r = _rng("as balanced", head)
    ring = bp.power_of_two_ring(H, head, r)
    assert sorted(sum(1 for _, _, tag in bp.eligible(ring) if tag == c) for c in range(4)) == [1, 2, 4, 8]
    rep = to_replay(ring, 4)
    ue = torch.from_numpy(np.concatenate([[0.0, pr.TOP, 0.5, 1.0 / 3, 0.37, 0.99, 0.125, 0.875], r.rand(56)]).astype(np.float32))
    for rotation, d in ((0, 0), (-5, 3), (7, 2 ** 40)):
        slot, weight = rep._pick_balanced_prioritized(ue, rotation, d, torch.tensor([0.7]))
        assert torch.equal(slot, rep._pick_balanced(ue, rotation, d)), (rotation, d)
        assert (weight == 1.0).all()


def test_the_reference_takes_the_class_by_rotation_and_the_episode_by_priority():
    """what the case list is for, by the reference alone: 8 episodes, tags 0 1 2 0 1 2 0 (newest: 2), class 0 with priorities 1, 2^20, 2^20 at
    ages 0, 3, 6: u = 0 takes age 0, the smallest u above 1 / T_c age 3, 1 - 2^-24 age 6; weights (1 / p)^beta; the slot of class 2, whose
    eligible members are ages 2 and 5, never takes the newest; an absent class falls back to all eligible episodes"""
    tags = np.array([0, 1, 2, 0, 1, 2, 0, 2], np.int32)
    prio = np.array([1, 7, 7, 2 ** 20, 7, 9, 2 ** 20, 1], np.uint32)
    ring = bp.make_ring(8, H, 8, 0, [H] * 8, tags, prio, _rng("ref"))
    T = 1 + 2 ** 21
    for u, age, p in ((0.0, 0, 1), (np.nextafter(np.float32(1.0 / T), np.float32(1)), 3, 2 ** 20), (pr.TOP, 6, 2 ** 20)):
        slot, w, got_p, p_min, total, t, c, m_c = bp.pick_ref(ring, 1, [u], 3, 0.5)[0]
        assert (slot, got_p, p_min, total, c, m_c) == (age, p, 1, T, 0, 3)
        assert w == float(np.float32(1) / np.float32(p)) ** 0.5
    picks = bp.pick_ref(ring, 3, [pr.TOP] * 3, 3, 1.0, rotation=-1)
    assert [p[6] for p in picks] == [2, 0, 1] and picks[0][0] == 5 and picks[0][7] == 2 and picks[0][3] == 7
    fallback = bp.pick_ref(ring, 1, [pr.TOP], 5, 1.0, rotation=4)[0]
    assert fallback[7] == 0 and fallback[0] == 6 and fallback[4] == int(prio[:7].astype(np.int64).sum()) and fallback[3] == 1


def test_arguments_are_checked_before_a_device_is_needed():
    """the sampler on rings that lack classes or priorities, or whose class names differ, and a beta of the wrong kind: ValueError, as
    sample_balanced and sample_prioritized; both trainers with both flags on a CPU ring that has classes: the device-ring error, no longer
    'not implemented'; run_stage(prioritized=True) without free_running: ValueError - all of them on a machine without a GPU"""
    from kinovagrasping_amd import curriculum
    from kinovagrasping_amd.pipeline import AsyncTrainer, GraphedTrainer
    new = lambda: DeviceEpisodeReplay(2, 8, horizon=H, n_steps=N, device="cpu")
    bare, only_classes, only_prio, both, other = new(), new(), new(), new(), new()
    only_classes.set_env_classes(None, ["a", "b"])
    only_prio.enable_priorities()
    both.set_env_classes(None, ["a", "b"])
    both.enable_priorities()
    other.set_env_classes(None, ["a", "c"])
    other.enable_priorities()
    for rep, expert, match in ((bare, None, "classes"), (only_prio, None, "classes"), (only_classes, None, "priorities"), (both, only_prio, "classes"),
                               (both, only_classes, "priorities"), (both, other, "class names")):
        with pytest.raises(ValueError, match=match):
            rep.sample_balanced_prioritized(expert, 4)
    short = DeviceEpisodeReplay(2, 8, horizon=H + 1, n_steps=N, device="cpu")
    short.set_env_classes(None, ["a", "b"])
    short.enable_priorities()
    with pytest.raises(ValueError, match="horizon"):
        both.sample_balanced_prioritized(short, 4)
    for beta in (torch.tensor([1.0, 2.0]), torch.tensor([1.0], dtype=torch.float64)):
        with pytest.raises(ValueError, match="beta"):
            both.sample_balanced_prioritized(None, 4, beta=beta)
    eng = types.SimpleNamespace(gen=None)
    for cls in (GraphedTrainer, AsyncTrainer):
        with pytest.raises(ValueError, match="device ring") as err:
            cls(None, None, only_classes, eng, prioritized=True, balanced=True)
        assert "not implemented" not in str(err.value)
        with pytest.raises(ValueError, match="must have classes set"):
            cls(None, None, new(), eng, prioritized=True, balanced=True)
    assert only_classes.ep_prio is None
    with pytest.raises(ValueError, match="free_running"):
        curriculum.run_stage({}, None, prioritized=True)
    with pytest.raises(ValueError, match="free_running"):
        curriculum.run_stage({}, None, prioritized=True, starts_per_env=4)
