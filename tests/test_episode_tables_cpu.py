"""The replay batch as episode tables without a GPU: DeviceEpisodeReplay(device="cpu").sample_tables - the torch front end, the checker of
kr_sample_tables_mixed - against the numpy restatement of tests/tables_ref.py, and the window form rebuilt from the tables against what
sample_batch_nstep, sample_mixed, sample_balanced, sample_prioritized and sample_balanced_prioritized return for the same uniforms.  Everything is compared bit for bit."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import tables_ref as tr
from kinovagrasping_amd.replay import DeviceEpisodeReplay

B = 4
FIELDS = ("table_state", "table_next", "table_action", "row_table", "slot_weight", "state0", "action0", "reward", "not_done", "weight", "next_ends")


def rings(H, n, count, head, device="cpu"):
    agent = tr.fill_ring(DeviceEpisodeReplay(2, 8, horizon=H, n_steps=n, device=device), count, head, seed=11)
    expert = tr.fill_ring(DeviceEpisodeReplay(2, 5, horizon=H, n_steps=n, device=device), 5, 0, seed=12)
    return agent, expert


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("H,n", tr.SHAPES)
@pytest.mark.parametrize("count,head", tr.RING_STATES)
def test_torch_front_end_equals_the_numpy_restatement_and_rebuilds_the_window_form(H, n, count, head):
    agent, expert = rings(H, n, count, head)
    W = H - n
    for prob in (1.0, 0.5, 0.0):                                   # batch_agent 0, 2 and B
        b_agent = int(B * (1 - prob))
        assert b_agent == {1.0: 0, 0.5: 2, 0.0: 4}[prob]
        for u in tr.uniform_cases(B, W):
            ut = torch.as_tensor(u)
            tb = agent.sample_tables(expert, B, prob, uniforms=ut, next_ends=True)
            ref = tr.tables_ref(tr.ring_arrays(agent), tr.ring_arrays(expert), B, b_agent, H, n, u)
            for k in FIELDS:
                assert same(getattr(tb, k).numpy(), ref[k]), (k, prob)
            # the window form from the tables: the reference's own, and what the window samplers return for these uniforms
            win = [t.numpy() for t in tb.windows()]
            for a, b in zip(win, tr.windows_of_tables(ref, n)):
                assert same(a, b)
            for a, b in zip(win, agent.sample_mixed(expert, B, prob, uniforms=ut)):
                assert same(a, b.numpy()), prob
            if prob == 0.0:
                single = agent.sample_tables(None, B, uniforms=ut)
                assert single.next_ends is None
                for a, b in zip(single.windows(), agent.sample_batch_nstep(B, uniforms=ut)):
                    assert same(a.numpy(), b.numpy())


@pytest.mark.parametrize("H,n", tr.SHAPES)
@pytest.mark.parametrize("count,head", tr.RING_STATES)
@pytest.mark.parametrize("pick", tr.PICKS, ids=["balanced", "prioritized", "balanced_prioritized"])
def test_tables_behind_a_pick_rebuild_what_the_window_sampler_returns(H, n, count, head, pick):
    """sample_tables(balanced / prioritized / both) for the same uniforms: the window form rebuilt from the tables and `picked` are
    sample_balanced's, sample_prioritized's and sample_balanced_prioritized's in every bit (the importance weights included: slot_weight
    is the weight of the slot's real rows); the tables are the numpy restatement's for those picks"""
    agent, expert = rings(H, n, count, head)
    tr.add_columns(agent, 31), tr.add_columns(expert, 32)
    W = H - n
    below_one = False
    for prob in (1.0, 0.5, 0.0):
        b_agent = int(B * (1 - prob))
        for i, u in enumerate(tr.uniform_cases(B, W)):
            ut = torch.as_tensor(u)
            kw = dict(uniforms=ut, draw=i)
            tb = agent.sample_tables(expert, B, prob, beta=0.6, rotation=1, **pick, **kw)
            win, picked = tr.window_sampler(agent, expert, B, prob, pick, 0.6, 1, **kw)
            assert tb.picked.dtype == torch.int32 and torch.equal(tb.picked, picked)
            for a, b in zip(tb.windows(), win):
                assert same(a.numpy(), b.numpy()), prob
            w, sw = tb.weight.view(B, W), tb.slot_weight.view(B, 1)
            assert ((w == 0) | (w == sw)).all() and (sw > 0).all() and (sw <= 1).all()
            below_one |= bool((sw < 1).any())
            ref = tr.tables_ref(tr.ring_arrays(agent), tr.ring_arrays(expert), B, b_agent, H, n, u, picked.numpy(), tb.slot_weight.numpy())
            for k in FIELDS[:-1]:
                assert same(getattr(tb, k).numpy(), ref[k]), (k, prob)
    assert below_one == bool(pick.get("prioritized"))                # (random priorities: some picked episode is not its ring's least likely one)


def test_one_episode_in_two_batch_slots_and_every_length():
    """with one uniform for every slot all four slots hold the same episode: four equal tables, window rows that point into their own slot's
    table; over the ring's five lengths (n - 1 .. H) every window stays inside its table and real rows end at the episode's length"""
    H, n = 30, 5
    agent, expert = rings(H, n, 8, 3)
    W = H - n
    for k in range(7):                                             # the k-th oldest of the 7 eligible episodes
        u = np.random.RandomState(k).rand(B * (W + 1)).astype(np.float32)
        u[:B] = (k + 0.5) / 7
        tb = agent.sample_tables(None, B, uniforms=torch.as_tensor(u))
        ts = tb.table_state.view(B, H, -1)
        assert all(torch.equal(ts[0], ts[b]) for b in range(B))
        slot = (3 - 8 + k) % 8
        assert torch.equal(ts[0], agent.ep_state[slot])
        rt = tb.row_table.view(B, W).long()
        lo = torch.arange(B).view(B, 1) * H
        assert ((rt >= lo) & (rt + n <= lo + H)).all()
        length = int(agent.ep_len[slot])
        live = tb.weight.view(B, W) > 0
        assert int(live.sum(1)[0]) == max(length - n, 1)
        if length > n:
            assert ((rt - lo)[live] + n <= length).all()


def test_refusals():
    agent, _ = rings(30, 5, 5, 5)
    other = DeviceEpisodeReplay(2, 5, horizon=31, n_steps=5, device="cpu")
    with pytest.raises(ValueError):
        agent.sample_tables(other, B)
    with pytest.raises(ValueError, match="set_env_classes"):
        agent.sample_tables(None, B, balanced=True)
    with pytest.raises(ValueError, match="enable_priorities"):
        agent.sample_tables(None, B, prioritized=True)
