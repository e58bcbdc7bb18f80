"""The replay batch as episode tables (DeviceEpisodeReplay.sample_tables, kr_sample_tables_mixed) restated in plain numpy, and the rings
the table tests draw from.  Written from the rule (utils.py:240-306 of the reference: the k-th oldest of count - 1 episodes; ceiling =
len - n windows, the last one starting at `ceiling`), one batch slot and one window at a time."""
from __future__ import annotations

import numpy as np

S, A = 82, 4
RING_STATES = ((0, 0), (1, 1), (2, 2), (5, 5), (8, 3))            # (count, head) of an 8-slot ring
SHAPES = ((7, 2), (30, 5))                                        # (horizon, n_steps)
UNIFORMS = (0.0, 0.5, float(1 - 2.0 ** -24))


def episode_lengths(capacity, H, n):
    """n - 1, n, n + 1, n + 2, H in turn over the ring's slots"""
    return np.array([(n - 1, n, n + 1, n + 2, H)[i % 5] for i in range(capacity + 1)], dtype=np.int64)


def fill_ring(rep, count, head, seed):
    """give the DeviceEpisodeReplay `rep` `count` committed episodes with the next slot at `head`: every row of every slot random (rows at
    or beyond an episode's length too: the tables copy them as the ring holds them), lengths by episode_lengths"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    for t in (rep.ep_state, rep.ep_next, rep.ep_action, rep.ep_reward, rep.ep_not_done):
        t.copy_(torch.rand(t.shape, generator=g).to(t.device))
    rep.ep_len.copy_(torch.as_tensor(episode_lengths(rep.capacity, rep.horizon, rep.n_steps)).to(rep.ep_len.device))
    rep._count.fill_(count)
    rep._head.fill_(head)
    return rep


CLASS_NAMES = ("a", "b", "c")


def add_columns(rep, seed):
    """give the ring a class column (three classes) and a priority column, both random per slot"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    rep.set_env_classes(None, list(CLASS_NAMES))
    rep.ep_class.copy_(torch.randint(0, len(CLASS_NAMES), rep.ep_class.shape, generator=g, dtype=torch.int32).to(rep.ep_class.device))
    rep.enable_priorities()
    rep.ep_prio.view(torch.int32).copy_(torch.randint(1, 1000, rep.ep_prio.shape, generator=g, dtype=torch.int32).to(rep.ep_prio.device))
    return rep


PICKS = (dict(balanced=True), dict(prioritized=True), dict(balanced=True, prioritized=True))


def window_sampler(rep, expert, B, prob, pick, beta, rotation, **kw):
    """the window sampler that goes with a pick of PICKS: its six tensors and `picked`"""
    if pick.get("balanced") and pick.get("prioritized"):
        out = rep.sample_balanced_prioritized(expert, B, prob, beta, rotation=rotation, **kw)
    elif pick.get("prioritized"):
        out = rep.sample_prioritized(expert, B, prob, beta, **kw)
    else:
        out = rep.sample_balanced(expert, B, prob, rotation=rotation, **kw)
    return out[:6], out[-1]


def ring_arrays(rep):
    """the numpy view of a ring the reference reads"""
    c = lambda t: t.detach().cpu().numpy()
    return dict(count=int(rep._count), head=int(rep._head), capacity=rep.capacity, ep_len=c(rep.ep_len), ep_state=c(rep.ep_state), ep_next=c(rep.ep_next),
                ep_action=c(rep.ep_action), ep_reward=c(rep.ep_reward), ep_not_done=c(rep.ep_not_done))


def draws_ref(agent, expert, B, b_agent, H, n, uniforms, picked=None):
    """per batch slot the ring slot it reads (picked: given, behind a balanced or prioritized pick), per window row its start and its 0 / 1
    weight; float32 products truncated, as the kernels'"""
    W = H - n
    u = np.asarray(uniforms, dtype=np.float32)
    ue, us = u[:B], u[B:].reshape(B, W)
    ep, start, weight = np.zeros(B, np.int64), np.zeros((B, W), np.int64), np.zeros((B, W), np.float32)
    for b in range(B):
        g = agent if b < b_agent else expert
        hi = max(g["count"] - 1, 1)
        k = min(int(np.float32(ue[b]) * np.float32(hi)), hi - 1)
        ep[b] = (g["head"] - g["count"] + k) % g["capacity"] if picked is None else picked[b]
        ceiling = max(int(g["ep_len"][ep[b]]) - n, 1)
        for w in range(W):
            s = min(int(np.float32(us[b, w]) * np.float32(ceiling)), H - n)
            if w == ceiling - 1:
                s = ceiling
            start[b, w] = min(s, H - n)
            weight[b, w] = 1.0 if (g["count"] >= 2 and w < ceiling) else 0.0
    return ep, start, weight


def tables_ref(agent, expert, B, b_agent, H, n, uniforms, picked=None, slot_weight=None):
    """the table form (picked [B], slot_weight [B]: the episodes and importance weights a pick chose; None: the uniform draw, weight 1): dict of table_state, table_next [B H, S], table_action [B H, A], row_table int32 [B W], slot_weight [B], state0,
    action0, reward, not_done, weight, next_ends [2 B W, S]"""
    W = H - n
    ep, start, weight = draws_ref(agent, expert, B, b_agent, H, n, uniforms, picked)
    sw = np.ones(B, np.float32) if slot_weight is None else np.asarray(slot_weight, np.float32)
    weight = weight * sw[:, None]
    out = dict(table_state=np.zeros((B * H, S), np.float32), table_next=np.zeros((B * H, S), np.float32), table_action=np.zeros((B * H, A), np.float32),
               row_table=np.zeros(B * W, np.int32), slot_weight=sw, state0=np.zeros((B * W, S), np.float32),
               action0=np.zeros((B * W, A), np.float32), reward=np.zeros((B * W, n), np.float32), not_done=np.zeros((B * W, n), np.float32),
               weight=weight.reshape(-1), next_ends=np.zeros((2 * B * W, S), np.float32))
    for b in range(B):
        g = agent if b < b_agent else expert
        out["table_state"][b * H:(b + 1) * H] = g["ep_state"][ep[b]]
        out["table_next"][b * H:(b + 1) * H] = g["ep_next"][ep[b]]
        out["table_action"][b * H:(b + 1) * H] = g["ep_action"][ep[b]]
        for w in range(W):
            r, s = b * W + w, int(start[b, w])
            out["row_table"][r] = b * H + s
            out["state0"][r] = g["ep_state"][ep[b], s]
            out["action0"][r] = g["ep_action"][ep[b], s]
            out["reward"][r] = g["ep_reward"][ep[b], s:s + n]
            out["not_done"][r] = g["ep_not_done"][ep[b], s:s + n]
            out["next_ends"][r] = g["ep_next"][ep[b], s]
            out["next_ends"][B * W + r] = g["ep_next"][ep[b], s + n - 1]
    return out


def windows_of_tables(tb, n):
    """the window form rebuilt from a table-form dict: state, action, next_state [R, n, *], reward, not_done, weight"""
    t = tb["row_table"].astype(np.int64)[:, None] + np.arange(n)[None, :]
    return tb["table_state"][t], tb["table_action"][t], tb["table_next"][t], tb["reward"], tb["not_done"], tb["weight"]


def uniform_cases(B, W, seed=0):
    """the uniform vectors [B + B W] of the table tests: each of UNIFORMS everywhere (every batch slot then picks the same episode: one
    episode in several slots), and a random mix of random values with them (slots 0 and 1 forced onto one episode)"""
    rng = np.random.RandomState(seed)
    cases = [np.full(B * (W + 1), v, np.float32) for v in UNIFORMS]
    mix = rng.rand(B * (W + 1)).astype(np.float32)
    pick = rng.randint(0, 4, size=mix.shape)
    for i, v in enumerate(UNIFORMS):
        mix[pick == i] = v
    mix[1] = mix[0]
    cases.append(mix)
    return cases
