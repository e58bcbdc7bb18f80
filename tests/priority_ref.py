"""Plain numpy restatement of prioritized episode replay (include/kinova_rollout.h: kr_commit_priorities, kr_sample_windows_prioritized,
kr_update_priorities; DeviceEpisodeReplay.sample_prioritized), written as loops over ages and rows with Python integers for the sums and
np.float32 arithmetic where the kernels are fp32 - it shares nothing with the torch path or the kernels.
tests/test_priority_sampler_cpu.py holds the torch path to it, tests/test_gpu_priority_sampler.py the kernels.

A ring is tests/balanced_ref.py's dict with ep_prio uint32 [capacity] in ep_class's place.  The two powers are evaluated in float64 on the
fp32 operands the kernels form; callers compare the kernels' fp32 results with them under the allowance stated in the GPU test."""
import numpy as np

RING_FIELDS = ("state", "next", "action", "reward", "not_done")
PRIO_ONE = 65536
U32_MAX = 2 ** 32 - 1


def commit_priorities_ref(keep, rank, head, capacity, prio_max, ep_prio):
    """ep_prio[(head + rank[i] - 1) % capacity] = max(prio_max, 1) for every kept env i, in place; nothing else is written"""
    for i in range(len(keep)):
        if keep[i] != 0:
            ep_prio[(int(head) + int(rank[i]) - 1) % capacity] = max(int(prio_max), 1)
    return ep_prio


def eligible_priorities(ring):
    """[(slot, priority)] of the count - 1 oldest episodes, oldest first; a stored 0 reads as 1"""
    count, head, cap = int(ring["count"]), int(ring["head"]), int(ring["capacity"])
    out = []
    for age in range(max(count - 1, 0)):
        slot = (head - count + age) % cap
        out.append((slot, max(int(ring["ep_prio"][slot]), 1)))
    return out


def pick_ref(ring, n_slots, u_ep, beta):
    """per batch slot of this ring's segment: (ring slot, importance weight in float64, priority of the episode, p_min, T, t)"""
    count, head, cap = int(ring["count"]), int(ring["head"]), int(ring["capacity"])
    u_ep = np.asarray(u_ep, np.float32).reshape(n_slots)
    elig = eligible_priorities(ring)
    total = sum(p for _, p in elig)
    out = []
    for i in range(n_slots):
        if not elig:
            hi = max(count - 1, 1)
            k = min(int(u_ep[i] * np.float32(hi)), hi - 1)
            out.append(((head - count + k) % cap, 1.0, 0, 0, 0, 0))
            continue
        assert total < 2 ** 53
        t = min(total - 1, int(float(u_ep[i]) * float(total)))           # one double product: both factors are exact doubles
        p_min = min(p for _, p in elig)
        run = 0
        for slot, p in elig:
            run += p
            if run > t:
                break
        ratio = np.float32(p_min) / np.float32(p)                         # two fp32 conversions and an fp32 division, as in the kernel
        out.append((slot, float(np.power(np.float64(ratio), np.float64(np.float32(beta)))), p, p_min, total, t))
    return out


def sample_prioritized_ref(batch, horizon, n_steps, agent, u_ep, u_start, beta, expert=None, batch_agent=None):
    """The whole batch: state, action, next_state, reward, not_done, weight (float64: the real rows' importance weight, 0 for padding; layout of
    kr_sample_windows), picked int32 [batch], next_ends [2 batch W, 82], and pick_ref's list, agent segment first."""
    W = horizon - n_steps
    batch_agent = batch if expert is None else int(batch_agent)
    u_ep, u_start = np.asarray(u_ep, np.float32).reshape(batch), np.asarray(u_start, np.float32).reshape(batch, W)
    picks = pick_ref(agent, batch_agent, u_ep[:batch_agent], beta)
    if batch > batch_agent:
        picks += pick_ref(expert, batch - batch_agent, u_ep[batch_agent:], beta)
    out = {f: [] for f in RING_FIELDS}
    weight = []
    for b in range(batch):
        g = agent if b < batch_agent else expert
        slot = picks[b][0]
        ceiling = max(int(g["ep_len"][slot]) - n_steps, 1)
        for w in range(W):
            start = min(int(u_start[b, w] * np.float32(ceiling)), W)
            if w == ceiling - 1:
                start = min(ceiling, W)                       # the final window of the episode
            for f in RING_FIELDS:
                out[f].append(g[f][slot, start:start + n_steps])
            weight.append(picks[b][1] if (int(g["count"]) >= 2 and w < ceiling) else 0.0)
    st = {f: np.stack(out[f]).astype(np.float32) for f in RING_FIELDS}
    ends = np.concatenate([st["next"][:, 0], st["next"][:, n_steps - 1]])
    return (st["state"], st["action"], st["next"], st["reward"], st["not_done"], np.asarray(weight, np.float64),
            np.asarray([p[0] for p in picks], np.int32), ends, picks)


def episode_deltas_ref(batch, W, n_steps, q, tq1, reward, weight, discount):
    """delta_b float32 [batch]: the largest |q - (reward[:, 0] + discount * tq1)| over the rows with weight > 0, each step rounded to fp32
    as the kernel's; NaN where such a row's error is NaN, -1 without such a row"""
    q, tq1, weight = (np.asarray(x, np.float32).reshape(batch * W) for x in (q, tq1, weight))
    reward = np.asarray(reward, np.float32).reshape(batch * W, n_steps)
    d32 = np.float32(discount)
    out = np.empty(batch, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(batch):
            m, bad = np.float32(-1.0), False
            for w in range(W):
                r = b * W + w
                if weight[r] > 0:
                    t1 = np.float32(reward[r, 0] + np.float32(d32 * tq1[r]))
                    e = np.float32(abs(np.float32(q[r] - t1)))
                    if np.isnan(e):
                        bad = True
                    elif e > m:
                        m = e
            out[b] = np.float32(np.nan) if bad else m
    return out


def quantise_ref(delta, eps, alpha):
    """(delta + eps)^alpha * 65536 before the floor, in float64 on the fp32 sum the kernel forms (the caller floors, clamps and allows for
    powf's error)"""
    base = np.float32(np.float32(delta) + np.float32(eps))
    return float(np.power(np.float64(base), np.float64(np.float32(alpha)))) * 65536.0


def clamp_priority(x):
    return int(min(max(np.floor(x), 1), U32_MAX))


def update_priorities_ref(batch, batch_agent, W, n_steps, q, tq1, reward, weight, discount, picked, alpha, eps_agent, eps_expert):
    """deltas float32 [batch], and per segment (agent, expert) {slot: (float64 value before the floor of the winning batch episode)} for the
    slots that are written - the maximum over the segment's batch episodes that read the slot and have a finite delta >= 0"""
    deltas = episode_deltas_ref(batch, W, n_steps, q, tq1, reward, weight, discount)
    written = ({}, {})
    for b in range(batch):
        seg, eps = (0, eps_agent) if b < batch_agent else (1, eps_expert)
        d, s = deltas[b], int(picked[b])
        if s < 0 or not np.isfinite(d) or d < 0:
            continue
        x = quantise_ref(d, eps, alpha)
        if s not in written[seg] or x > written[seg][s]:
            written[seg][s] = x
    return deltas, written


# ---- the case list the CPU and the GPU test share ------------------------------------------------------------------------------------
CAP, B, B_AGENT, H, N_STEPS = 8, 6, 4, 8, 3           # W = 5
COUNT_HEAD = [(0, 0), (1, 1), (2, 2), (5, 5), (8, 0), (8, 3), (8, 7), (5, 3), (2, 0), (5, 7), (1, 0), (0, 3)]   # count 0, 1, 2, 5, 8; wrapped rings among them
TOP = np.float32(1.0 - 2.0 ** -24)


def ring_lens(H, n):
    return [H, n + 2, n + 1, n, n - 1, H, n + 2, n + 1]


def make_ring(cap, H, count, head, lens, prio, rng):
    ring = dict(count=count, head=head, capacity=cap, ep_len=np.asarray(lens, np.int64), ep_prio=np.asarray(prio, np.uint32))
    S, A = 82, 4
    for f, s in dict(state=(cap, H, S), next=(cap, H, S), action=(cap, H, A), reward=(cap, H), not_done=(cap, H)).items():
        ring[f] = rng.standard_normal(s).astype(np.float32)
    return ring


def priority_patterns(cap, rng):
    """{name: uint32 [cap]}: equal priorities; the extremes 1 and 2^32 - 1 side by side (and a stored 0, which reads as 1); random over the
    whole range; random around PRIO_ONE"""
    ext = np.array([1, U32_MAX, 0, U32_MAX, 1, 1, U32_MAX, 7] * (cap // 8 + 1), np.uint64)[:cap]
    return {"equal": np.full(cap, PRIO_ONE, np.uint32), "extremes": ext.astype(np.uint32),
            "random": rng.randint(0, 2 ** 32, cap, dtype=np.uint64).astype(np.uint32),
            "near_one": rng.randint(PRIO_ONE // 50, 40 * PRIO_ONE, cap).astype(np.uint32)}


def episode_uniforms(batch, ring, shift):
    """u_ep [batch]: 0, 1 - 2^-24, 0.5, and values at and beside the prefix-sum boundaries of the ring's eligible priorities"""
    pool = [0.0, TOP, 0.5]
    elig = eligible_priorities(ring)
    total, run = sum(p for _, p in elig), 0
    for _, p in elig[:4]:
        run += p
        x = np.float32(run / max(total, 1))
        pool += [x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(1))]
    pool = np.asarray(pool, np.float32)
    pool = pool[(pool >= 0) & (pool < 1)]
    return np.roll(np.resize(pool, max(batch, len(pool))), shift)[:batch].copy()


def start_uniforms(batch, W, shift):
    pool = np.asarray([0.0, 0.5, TOP] + [j / 25.0 for j in range(1, 25)] + [1.0 / 3, 2.0 / 3], np.float32)
    return np.stack([np.roll(pool, 5 * b + shift)[:W] for b in range(batch)])
