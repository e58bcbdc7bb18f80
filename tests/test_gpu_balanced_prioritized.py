"""kr_sample_windows_balanced_prioritized (csrc/ks_rollout.hip: k_pick_balanced_prioritized, k_gather_windows) through the C ABI against the plain
loops of tests/balprio_ref.py, between guard regions (the buffers of tests/test_gpu_glue_kernels.py): which episode a batch slot takes and every
gathered row are pinned to the bit, the importance weight to the powf allowance of tests/test_gpu_priority_sampler.py.  Then the two samplers it
combines on the same inputs, the refusals, and the combined sampler end to end: in the lock-step trainer, in the free-running trainer and in
curriculum.run_stage."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from tests import balprio_ref as bp
from tests import priority_ref as pr
from tests.test_gpu_balanced_sampler import _check_tags, _two_shape_setup, run_balanced
from tests.test_gpu_glue_kernels import Buf, P, S, _lib, _rng, _stream, assert_bits, sent
from tests.test_gpu_priority_sampler import (K_POWF, OUT_ORDER, _call, _host_ring, _refuse, check_entry, check_weights, kr_ring, outputs,
                                             philox_uniforms, run_prioritized)

pytestmark = pytest.mark.gpu

A = 4
FN = "kr_sample_windows_balanced_prioritized"


def upload(ring, prio_offset=0, tag_offset=0, front_tag=0):
    """the ring's buffers; the two tables `prio_offset` / `tag_offset` elements behind a 16-byte boundary, the elements in front of them holding
    priority 2^32 - 1 and the tag `front_tag`"""
    dev = {k: Buf(ring[k]) for k in bp.RING_FIELDS}
    dev.update(count=Buf(np.array([ring["count"]], np.int64)), head=Buf(np.array([ring["head"]], np.int64)), ep_len=Buf(ring["ep_len"]),
               ep_prio=Buf(np.concatenate([np.full(prio_offset, pr.U32_MAX, np.uint32), ring["ep_prio"]])),
               ep_class=Buf(np.concatenate([np.full(tag_offset, front_tag, np.int32), ring["ep_class"]])))
    return dev


def run_combined(batch, b_agent, H, n, agent, da, expert, de, nc, rotation, beta, ue, us, draw, with_picked=True, with_ends=True, seed=0,
                 prio_offset=0, tag_offset=0):
    """one call with explicit uniforms (ue not None) or in-kernel draws; returns the output buffers"""
    out = outputs(batch, H - n, n)
    ra, re = kr_ring(agent, da), kr_ring(expert, de)
    keep = [Buf(ue), Buf(us)] if ue is not None else [None, None]
    dr = None if draw is None else Buf(np.array([draw], np.int64))
    bb = Buf(np.array([beta], np.float32))
    rc = getattr(_lib(), FN)(batch, b_agent, H, n, ctypes.byref(ra), ctypes.byref(re), P(da["ep_class"], 4 * tag_offset), P(de["ep_class"]), nc, rotation,
                             P(da["ep_prio"], 4 * prio_offset), P(de["ep_prio"]), P(bb), P(keep[0]), P(keep[1]), seed, P(dr),
                             *[P(out[k]) for k in OUT_ORDER], P(out["ends"]) if with_ends else None, P(out["picked"]) if with_picked else None, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bb.unchanged() and all(k is None or k.unchanged() for k in keep) and (dr is None or dr.unchanged())
    return out


def check(out, ref, what, with_picked=True, with_ends=True):
    if with_picked:
        assert_bits(out["picked"].get(), ref[6], f"{what}: picked")
    else:
        assert out["picked"].unchanged()
    for k, want in zip(OUT_ORDER[:5], ref[:5]):
        assert_bits(out[k].get(), want, f"{what}: {k}")
    if with_ends:
        assert_bits(out["ends"].get(), ref[7], f"{what}: next_ends")
    else:
        assert out["ends"].unchanged()
    return check_weights(out["weight"].get(), ref[5], what)


def same_outputs(got, want, what, keys=OUT_ORDER + ("ends", "picked")):
    for k in keys:
        assert_bits(got[k].get(), want[k].get(), f"{what}: {k}")


# ---- pick and gather, every row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,head", bp.COUNT_HEAD)
def test_combined_sampler_every_row(count, head):
    """horizon 8, n_steps 3 (W = 5), 6 batch slots, an agent ring of 8 slots at every (count, head) of priority_ref's list and an expert ring of 5;
    1, 3 and 64 classes; tags cyclic, with an absent class (the fallback), with a class whose only member is the newest episode, with -1 and with
    a value >= n_classes; tables of equal priorities, of 1 and 2^32 - 1 side by side with a stored 0, random ones (every tag pattern with one of
    them, in turn); uniforms on 0, on 1 - 2^-24, on and beside the classes' prefix-sum boundaries, and Philox draws; batch_agent 0, 4 and 6;
    rotation -5, 0 and 7; with and without `picked` and next_ends: picked, every output row - the weight-0 rows too - and next_ends equal
    balprio_ref bit for bit, the weights within the powf allowance"""
    H, n, W = bp.H, bp.N_STEPS, bp.H - bp.N_STEPS
    worst, fallbacks, in_class = 0.0, 0, 0
    for nc in bp.N_CLASSES:
        for k, (tname, tags) in enumerate(bp.tag_patterns(nc, count, head).items()):
            pname = ("equal", "extremes", "random")[(k + count + head + nc) % 3]
            r = _rng("balprio rows", count, head, nc, tname)
            agent = bp.make_ring(bp.CAP, H, count, head, pr.ring_lens(H, n), tags, pr.priority_patterns(bp.CAP, r)[pname], r)
            expert = bp.expert_ring(r, nc)
            da, de = upload(agent), upload(expert)
            for shift, (beta, rotation) in enumerate(zip((1.0, 0.4, 0.0), bp.ROTATIONS)):
                us = pr.start_uniforms(bp.B, W, shift)
                what = f"nc {nc} {tname} {pname} beta {beta} rotation {rotation}"
                ue = bp.episode_uniforms(bp.B, agent, nc, rotation, shift)
                out = run_combined(bp.B, bp.B, H, n, agent, da, agent, da, nc, rotation, beta, ue, us, None)
                ref = bp.sample_ref(bp.B, H, n, agent, ue, us, nc, beta, rotation)
                worst = max(worst, check(out, ref, what + " one ring"))
                fallbacks += sum(p[7] == 0 for p in ref[8])
                in_class += sum(p[7] > 0 for p in ref[8])
                for b_agent in ((0, bp.B_AGENT, bp.B) if shift == (k % 3) else (bp.B_AGENT,)):
                    with_picked, with_ends = b_agent != bp.B_AGENT or shift == 1, b_agent != bp.B_AGENT or shift != 2
                    ue[b_agent:] = bp.episode_uniforms(bp.B - b_agent, expert, nc, rotation, shift)
                    out = run_combined(bp.B, b_agent, H, n, agent, da, expert, de, nc, rotation, beta, ue, us, None, with_picked, with_ends)
                    ref = bp.sample_ref(bp.B, H, n, agent, ue, us, nc, beta, rotation, expert=expert, batch_agent=b_agent)
                    worst = max(worst, check(out, ref, what + f" batch_agent {b_agent}", with_picked, with_ends))
            # in-kernel draws: the uniforms are Philox's and the draw counter moves the classes, the batch the reference's on those
            seed, draw = 0x1234567890ABCDEF, 2 ** 40 + 77
            ue, us = philox_uniforms(np.arange(bp.B), 0x5a4d, seed, draw), philox_uniforms(np.arange(bp.B * W), 0x5a4e, seed, draw).reshape(bp.B, W)
            for with_picked in (True, False):
                out = run_combined(bp.B, bp.B_AGENT, H, n, agent, da, expert, de, nc, 7, 0.6, None, None, draw, with_picked, seed=seed)
                ref = bp.sample_ref(bp.B, H, n, agent, ue, us, nc, 0.6, 7, draw, expert=expert, batch_agent=bp.B_AGENT)
                worst = max(worst, check(out, ref, f"nc {nc} {tname} {pname} philox", with_picked))
            assert all(b.unchanged() for b in list(da.values()) + list(de.values()))
    print(f"\nBALPRIO rows count {count} head {head} | worst powf error {worst:.3f} x 2^-23, {in_class} slots from their class, {fallbacks} fell back")
    assert fallbacks > 0 and (in_class > 0 or count < 2)


# ---- long tables: the pick alone, through `picked` ---------------------------------------------------------------------------------------
ELIGIBLE = (1, 2, 3, 255, 256, 257, 767, 768, 769, 1535, 1536, 1537, 2047, 2048, 2049, 4100)
OFFSETS = ((0, 1), (2, 1), (1, 1), (3, 0), (2, 3), (0, 0), (1, 2), (3, 3))          # (priority table, tag table) elements behind a 16-byte boundary


@pytest.mark.parametrize("wrapped", [False, True], ids=["unwrapped", "wrapped"])
@pytest.mark.parametrize("eligible", ELIGIBLE)
def test_combined_pick_on_long_tables(eligible, wrapped):
    """eligible counts around one trip of the walk (256 episodes), around one group of trips of the masked walk (768) and of the unmasked one
    (1536), around 2048, and 4100 (several groups, the last one partial); the eligible range in one piece (head = count) or wrapped into two with
    ragged ends (a full ring, head mid-table); the priority table and the tag table each 0 - 3 elements behind a 16-byte boundary, in unequal
    and equal combinations; 3 and 14 classes, tags random with some -1 and some >= n_classes, and (wrapped) the last class confined to the piece
    behind the wrap; priorities all 1, all 2^32 - 1, random, and 1 with a few 2^32 - 1.  Every slot outside the eligible range - the newest
    episode, the slots beyond count, the elements in front of the tables - holds a wanted tag with priority 2^32 - 1: a walk that reads one
    picks wrongly.  W = 1; compared through `picked`: exact."""
    H, n, batch = 4, 3, 28
    if wrapped:
        cap = count = eligible + 1
        head = (2 * cap) // 3 if cap > 2 else 1
    else:
        cap, count = eligible + 3, eligible + 1
        head = count
    r = _rng("long balprio", eligible, wrapped)
    zeros = {f: np.zeros(s, np.float32) for f, s in dict(state=(cap, H, S), next=(cap, H, S), action=(cap, H, A), reward=(cap, H), not_done=(cap, H)).items()}
    tables = {"ones": np.ones(cap, np.uint32), "max": np.full(cap, pr.U32_MAX, np.uint32),
              "random": r.randint(0, 2 ** 32, cap, dtype=np.uint64).astype(np.uint32),
              "spikes": np.where(r.rand(cap) < 0.01, pr.U32_MAX, 1).astype(np.uint32)}
    ages = (np.arange(cap) - (head - count)) % cap                                  # the age of every slot; >= count - 1: outside
    worst = 0.0
    for k, (name, table) in enumerate(tables.items()):
        for j in range(2):
            nc = (3, 14)[(k + j) % 2]
            p_off, t_off = OFFSETS[(2 * k + j + eligible) % len(OFFSETS)]
            tags = r.randint(0, nc - 1 if wrapped else nc, cap).astype(np.int32)
            tags[r.rand(cap) < 0.05] = -1
            tags[r.rand(cap) < 0.05] = nc + 1
            if wrapped:                                                             # the last class: only in slots [0, head - 1), the younger piece
                behind = np.flatnonzero((np.arange(cap) < head - 1) & (r.rand(cap) < 0.3))
                tags[behind] = nc - 1
            outside = ages >= count - 1
            tags[outside] = np.arange(int(outside.sum())) % 2                       # wanted classes, at the largest priority
            prio = np.where(outside, pr.U32_MAX, table).astype(np.uint32)
            ring = dict(count=count, head=head, capacity=cap, ep_len=np.full(cap, H, np.int64), ep_prio=prio, ep_class=tags, **zeros)
            dev = upload(ring, prio_offset=p_off, tag_offset=t_off, front_tag=j)
            elig = bp.eligible(ring)
            assert len(elig) == eligible
            rotation = int(r.randint(-20, 20))
            ue = r.rand(batch).astype(np.float32)
            ue[:3] = [0.0, pr.TOP, 0.5]
            for i in range(3, 15):                                                  # on and just below a prefix-sum boundary of the slot's class
                qs = [p for _, p, tag in elig if tag == (i + rotation) % nc] or [p for _, p, _ in elig]
                x = np.float32(np.cumsum(qs, dtype=np.float64)[r.randint(0, len(qs))] / sum(qs))
                ue[i] = x if i % 2 else np.nextafter(x, np.float32(0))
            ue = np.where((ue >= 0) & (ue < 1), ue, np.float32(0.25)).astype(np.float32)
            out = run_combined(batch, batch, H, n, ring, dev, ring, dev, nc, rotation, 0.5, ue, np.zeros((batch, 1), np.float32), None, with_ends=False,
                               prio_offset=p_off, tag_offset=t_off)
            picks = bp.pick_ref(ring, batch, ue, nc, 0.5, rotation)
            what = f"eligible {eligible} {name} nc {nc} offsets {p_off}/{t_off}"
            assert_bits(out["picked"].get(), np.asarray([p[0] for p in picks], np.int32), f"{what}: picked")
            worst = max(worst, check_weights(out["weight"].get(), [p[1] for p in picks], what))
            assert dev["ep_prio"].unchanged() and dev["ep_class"].unchanged()
            assert all(ages[p[0]] < count - 1 for p in picks) and all(tags[p[0]] == p[6] for p in picks if p[7] > 0)
            if wrapped and eligible > 255:
                assert any(p[6] == nc - 1 and p[7] > 0 and p[0] < head - 1 for p in picks)
    print(f"\nBALPRIO long eligible {eligible} {'wrapped' if wrapped else 'unwrapped'} | worst powf error {worst:.3f} x 2^-23")


# ---- the two samplers it combines, on the same inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,head", [(2, 2), (5, 5), (8, 3), (8, 7), (5, 3)])
def test_one_class_or_no_known_tag_equals_the_prioritized_sampler(count, head):
    """n_classes == 1 with every tag 0, and 3 classes with no eligible tag inside [0, 3): picked, every row, next_ends - and the weight column,
    the same powf on the same operands - equal kr_sample_windows_prioritized's in every bit; caller's uniforms and Philox draws, batch_agent
    0, 4 and 6, with and without `picked`"""
    H, n, W = bp.H, bp.N_STEPS, bp.H - bp.N_STEPS
    for pname in ("equal", "extremes", "random", "near_one"):
        for nc, tags, etags in ((1, np.zeros(bp.CAP, np.int32), np.zeros(5, np.int32)),
                                (3, np.array([-1, 3, 7, -2, 64, 3, -1, 100], np.int32), np.array([5, -1, 3, 3, -7], np.int32))):
            r = _rng("as prioritized", count, head, pname)
            agent = bp.make_ring(bp.CAP, H, count, head, pr.ring_lens(H, n), tags, pr.priority_patterns(bp.CAP, r)[pname], r)
            expert = bp.expert_ring(r, nc)
            expert["ep_class"] = etags
            da, de = upload(agent), upload(expert)
            ue = pr.episode_uniforms(bp.B, agent, 1)
            us = pr.start_uniforms(bp.B, W, 1)
            for b_agent, rotation, with_picked in ((0, 0, True), (bp.B_AGENT, -5, True), (bp.B, 7, True), (bp.B_AGENT, 7, False)):
                got = run_combined(bp.B, b_agent, H, n, agent, da, expert, de, nc, rotation, 0.4, ue, us, None, with_picked)
                want = run_prioritized(bp.B, b_agent, H, n, agent, da, expert, de, 0.4, ue, us, None, with_picked=with_picked)
                same_outputs(got, want, f"{pname} nc {nc} batch_agent {b_agent}")
            got = run_combined(bp.B, bp.B_AGENT, H, n, agent, da, expert, de, nc, 2, 0.7, None, None, 2 ** 33 + 5, seed=99)
            want = run_prioritized(bp.B, bp.B_AGENT, H, n, agent, da, expert, de, 0.7, None, None, 2 ** 33 + 5, seed=99)
            same_outputs(got, want, f"{pname} nc {nc} philox")


@pytest.mark.parametrize("head", [0, 5, 11])
def test_equal_priorities_equal_the_balanced_sampler_with_unit_weights(head):
    """every priority 65536 on full rings of 16 slots whose 15 eligible episodes are 8, 4, 2 and 1 of four classes (balprio_ref.power_of_two_ring:
    both rules take the same floor on every uniform): picked, every row and next_ends equal kr_sample_windows_balanced's in every bit, and so
    does the weight column - every real weight is exactly 1.0 whatever beta is"""
    H, n, W, batch = bp.H, bp.N_STEPS, bp.H - bp.N_STEPS, 32
    r = _rng("as balanced", head)
    agent, expert = bp.power_of_two_ring(H, head, r), bp.power_of_two_ring(H, (head + 7) % 16, r)
    agent["ep_len"], expert["ep_len"] = np.resize(pr.ring_lens(H, n), 16).astype(np.int64), np.resize(pr.ring_lens(H, n)[::-1], 16).astype(np.int64)
    da, de = upload(agent), upload(expert)
    ue = np.concatenate([[0.0, pr.TOP, 0.5, 1.0 / 3, 0.37, 0.99, 0.125, 0.875], r.rand(batch - 8)]).astype(np.float32)
    us = r.rand(batch, W).astype(np.float32)
    for b_agent, rotation, beta in ((batch, 0, 0.7), (22, -5, 1.0), (0, 7, 0.3)):
        got = run_combined(batch, b_agent, H, n, agent, da, expert, de, 4, rotation, beta, ue, us, None)
        want = run_balanced(batch, b_agent, H, n, agent, da, expert, de, 4, rotation, ue, us, None)
        same_outputs(got, want, f"batch_agent {b_agent} rotation {rotation}")
        weight = got["weight"].get()
        assert set(np.unique(weight).tolist()) <= {0.0, 1.0} and (weight == 1.0).sum() > batch
    got = run_combined(batch, 22, H, n, agent, da, expert, de, 4, 3, 0.5, None, None, 2 ** 35 + 1, seed=7)
    want = run_balanced(batch, 22, H, n, agent, da, expert, de, 4, 3, None, None, 2 ** 35 + 1, seed=7)
    same_outputs(got, want, "philox")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _valid_call():
    H, ns, cap, W = 8, 5, 4, 3
    fz = lambda *s: Buf(np.zeros(s, np.float32))
    fs = lambda *s: Buf(sent(s, np.float32))
    rings = []
    for _ in range(2):
        rings.append(dict(count=Buf(np.array([3], np.int64)), head=Buf(np.array([3], np.int64)), capacity=cap, ep_len=Buf(np.full(cap, H, np.int64)),
                          ep_state=fz(cap, H, S), ep_next=fz(cap, H, S), ep_action=fz(cap, H, A), ep_reward=fz(cap, H), ep_not_done=fz(cap, H)))
    R = 2 * W
    table = lambda: Buf(np.array([5, 1, 70000, 9], np.uint32))
    classes = lambda: Buf(np.array([0, 1, 0, 1], np.int32))
    return [2, 1, H, ns, rings[0], rings[1], classes(), classes(), 2, 0, table(), table(), Buf(np.array([0.5], np.float32)), fz(2), fz(2, W), 5,
            Buf(np.array([2], np.int64)), fs(R, ns, S), fs(R, ns, A), fs(R, ns, S), fs(R, ns), fs(R, ns), fs(R), fs(2 * R, S), Buf(sent(2, np.int32))]


REFUSALS = [("batch 0", 0, 0), ("batch_agent > batch", 1, 3), ("batch_agent -1", 1, -1), ("horizon == n_steps", 2, 5), ("n_steps 65", (2, 3), (70, 65)),
            ("n_steps 0", 3, 0), ("agent ring NULL", 4, None), ("expert ring NULL", 5, None), ("agent_class NULL", 6, None), ("expert_class NULL", 7, None),
            ("n_classes 0", 8, 0), ("n_classes 65", 8, 65), ("n_classes -1", 8, -1), ("agent_prio NULL", 10, None), ("expert_prio NULL", 11, None),
            ("beta NULL", 12, None), ("u_ep without u_start", 14, None), ("u_start without u_ep", 13, None), ("no uniforms and no draw", (13, 14, 16), None)] + \
           [(f"NULL output {k}", k, None) for k in range(17, 23)] + \
           [(f"{which} ring without {f}", (4 if which == "agent" else 5, f), None) for which in ("agent", "expert")
            for f in ("count", "head", "ep_len", "ep_state", "ep_next", "ep_action", "ep_reward", "ep_not_done", "capacity")] + \
           [(f"{which} capacity above 2^20", (4 if which == "agent" else 5, "capacity"), 2 ** 20 + 1) for which in ("agent", "expert")]


@pytest.mark.parametrize("label,index,value", REFUSALS, ids=[c[0].replace(" ", "_") for c in REFUSALS])
def test_combined_sampler_refusals(label, index, value):
    """what kr_sample_windows_mixed refuses, n_classes outside 1 .. 64, a NULL beta, and for a ring that has batch slots a NULL class or priority
    table or a capacity above 2^20: KS_ERR_INVALID, and no buffer of the call - the sentinel-filled outputs among them - has changed"""
    args = _valid_call()
    _refuse(FN, args, args[4:6], label, index, value)


def test_the_valid_call_and_its_optional_arguments():
    """the refusal list's call runs and fills its outputs; so it does without next_ends, without picked, with NULL tables for a ring that has no
    batch slots, with in-kernel draws and without a draw counter"""
    for change in ({}, {23: None}, {24: None}, {23: None, 24: None}, {1: 2, 7: None, 11: None}, {1: 0, 6: None, 10: None}, {13: None, 14: None}, {16: None}):
        args = _valid_call()
        for k, v in change.items():
            args[k] = v
        assert _call(FN, args) == 0, change
        torch.cuda.synchronize()
        for k in range(17, 25):
            if args[k] is not None:
                assert not args[k].unchanged(), (change, k)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_lock_step_trainer_balances_the_classes_and_writes_the_errors_back():
    """GraphedTrainer(balanced=True, prioritized=True), 64 envs, two shapes, horizon 12, batch 8, eager: the ring is filled by the engine's own
    steps, the table set to random priorities, three updates run.  Every update's `picked` and batch rows are balprio_ref's on the table before it
    and the Philox uniforms of (seed, update count), the update count moving the classes, so the two classes' shares of the batch differ by one slot at most (here: 4 and 4); the
    priorities of the picked slots are what priority_ref computes from the q, tq1, reward and weight the update handed to kr_update_priorities,
    within the powf allowance, and every other entry is as before"""
    from kinovagrasping_amd.pipeline import GraphedTrainer
    sim, policy, replay, eng = _two_shape_setup()
    tr = GraphedTrainer(sim, policy, replay, eng, batch_episodes=8, overlap=False, balanced=True, prioritized=True, per_alpha=0.6, per_beta=0.4, per_eps=1e-3)
    assert replay.ep_prio is not None and replay.priority_max() == pr.PRIO_ONE
    for _ in range(26):
        eng.step()
    torch.cuda.synchronize()
    cnt, cap = replay.count, replay.capacity
    assert 2 * 64 <= cnt <= cap and (replay.priorities() == pr.PRIO_ONE).all()
    table = _rng("lock step balprio").randint(pr.PRIO_ONE // 100, 50 * pr.PRIO_ONE, cap + 1).astype(np.uint32)
    replay.ep_prio.view(torch.int32).copy_(torch.from_numpy(table.view(np.int32)).to(replay.device))
    H, n, B = replay.horizon, replay.n_steps, 8
    W = H - n
    seen = []
    inner = tr._update_priorities

    def spy(q, tq1, reward, weight):
        seen.append([x.detach().cpu().numpy().copy() for x in (q, tq1, reward, weight)])
        inner(q, tq1, reward, weight)
    tr._update_priorities = spy
    seed = tr.sample_seed & (2 ** 64 - 1)
    tags_all = replay.ep_class[:cap].cpu().numpy()
    for update in range(3):
        before = replay.priorities().cpu().numpy()
        draw = int(tr.native.it.item())                                          # the update count the sampler reads: Philox counter and class rotation
        tr._learn_eager()
        torch.cuda.synchronize()
        ring = _host_ring(replay, before)
        ring["ep_class"] = tags_all
        ue, us = philox_uniforms(np.arange(B), 0x5a4d, seed, draw), philox_uniforms(np.arange(B * W), 0x5a4e, seed, draw).reshape(B, W)
        ref = bp.sample_ref(B, H, n, ring, ue, us, 2, 0.4, 0, draw)
        picked = tr.picked.cpu().numpy()
        assert picked.tolist() == ref[6].tolist()
        for k in range(5):
            assert tr.batch[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
        check_weights(tr.batch[5].cpu().numpy(), ref[5], f"lock-step trainer update {update}")
        per = np.bincount(tags_all[picked], minlength=2)
        assert per.sum() == B and abs(int(per[0]) - int(per[1])) <= 1, per
        q, tq1, reward, weight = seen[update]
        tq1 = tq1.reshape(-1)[:B * W]                                            # (the target critic's [2 R] block: 1-step values first)
        _, written = pr.update_priorities_ref(B, B, W, n, q, tq1, reward, weight, policy.discount, picked, 0.6, 1e-3, 1.0)
        after = replay.priorities().cpu().numpy()
        assert sorted(written[0]) == sorted(set(picked.tolist())) and not written[1]
        for s, x in written[0].items():
            check_entry(after[s], x, f"update {update} slot {s}")
        others = np.setdiff1d(np.arange(cap + 1), list(written[0]))
        assert (after[others] == before[others]).all()
        print(f"\nBALPRIO lock step update {update}: picked {picked.tolist()}, classes {per.tolist()}, entries {[int(after[s]) for s in picked]}")
    assert len(seen) == 3 and replay.priority_max() >= pr.PRIO_ONE
    sim.close()


def test_free_running_trainer_keeps_tags_and_priorities_consistent():
    """AsyncTrainer(balanced=True, prioritized=True) on the same set-up, three launches of 13 env-steps from captured graphs: every committed slot
    holds the tag of its env's class and a priority in [1, prio_max], no episode was dropped and no pacing wait timed out, the last batch holds
    both classes in equal shares; set_per_beta reaches the captured sampler - the first two launches run with beta 0.4 (their least real weight is
    printed), the last with beta 0, where every real weight is exactly 1 whatever the table holds"""
    from kinovagrasping_amd.pipeline import AsyncTrainer
    sim, policy, replay, eng = _two_shape_setup()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=8, balanced=True, prioritized=True, per_beta=0.4)
    tr.capture()
    assert replay.priority_max() == pr.PRIO_ONE and (replay.priorities() == pr.PRIO_ONE).all()       # the warm-up updates left no trace
    low = []
    for k in range(3):
        tr.set_per_beta(0.4 if k < 2 else 0.0)
        tr.run(13)
        tr.flush()
        torch.cuda.synchronize()
        weight = tr.batch[5].cpu().numpy()
        assert ((weight >= 0) & (weight <= 1)).all()
        low.append(float(weight[weight > 0].min()) if (weight > 0).any() else None)      # (None: the ring held fewer than two episodes yet)
    c = tr.counts()
    tags = _check_tags(replay, at_least=2 * 64)
    cnt, head, cap = replay.count, replay.head, replay.capacity
    assert c["episodes_dropped"] == 0 and c["pacing_timeouts"] == 0 and c["episodes_kept"] == cnt
    slots = (head - cnt + np.arange(cnt)) % cap
    table, top = replay.priorities().cpu().numpy(), replay.priority_max()
    assert (table[slots] >= 1).all() and (table[slots] <= top).all() and pr.PRIO_ONE <= top <= pr.U32_MAX
    changed = int((table[slots] != pr.PRIO_ONE).sum())
    picked = tr.picked.cpu().numpy()
    assert ((picked >= 0) & (picked < cap)).all()
    per = np.bincount(replay.ep_class[torch.as_tensor(picked).long().to(replay.device)].cpu().numpy(), minlength=2)
    print(f"\nBALPRIO free running: {c}, ring {np.bincount(tags).tolist()}, batch slots {per.tolist()}, updates {tr.updates}, prio_max {top / pr.PRIO_ONE:.3f}, "
          f"{changed} of {cnt} entries written, least real weight per launch {low}")
    assert tr.updates == 39 and changed > 0 and np.isfinite(tr.per_delta.cpu().numpy()).all()
    assert per.sum() == 8 and abs(int(per[0]) - int(per[1])) <= 1
    assert set(np.unique(weight).tolist()) <= {0.0, 1.0} and low[2] == 1.0
    sim.close()


def test_run_stage_free_running_prioritized_on_two_shapes(tmp_path):
    """curriculum.run_stage(free_running=True, prioritized=True) on a two-shape plan: the result has priority_max (the agent ring's in units of
    1 / 65536; no expert data here), the last batch is balanced over the shapes and both shapes are in the ring"""
    from kinovagrasping_amd import curriculum
    from kinovagrasping_amd.ddpgfd import DDPGfD
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=8, hidden=(64, 64), device=torch.device("cuda", 0))
    plan = dict(curriculum.experiment_plan(3, root=tmp_path), requested_shapes=["CubeS", "CylinderS"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        out = curriculum.run_stage(plan, policy, n_envs=64, rounds=2, starts_per_env=4, free_running=True, prioritized=True, save=False,
                                   load_previous=False)
    print("run_stage free running prioritized:", {k: out[k] for k in ("env_steps", "replay_class_counts", "batch_class_slots", "priority_max", "updates")})
    assert out["env_steps"] == 2 * 30 * 64 and out["updates"] == 2 * 30 * 3
    assert set(out["priority_max"]) == {"agent", "expert"} and out["priority_max"]["expert"] is None
    assert isinstance(out["priority_max"]["agent"], int) and pr.PRIO_ONE <= out["priority_max"]["agent"] <= pr.U32_MAX
    assert list(out["replay_class_counts"]) == ["CubeS", "CylinderS"] and all(v > 0 for v in out["replay_class_counts"].values())
    slots = out["batch_class_slots"]
    assert list(slots) == ["CubeS", "CylinderS"] and sum(slots.values()) == 8 and abs(slots["CubeS"] - slots["CylinderS"]) <= 1
