"""Plain numpy restatement of the class-balanced prioritized window sampler (include/kinova_rollout.h: kr_sample_windows_balanced_prioritized;
DeviceEpisodeReplay.sample_balanced_prioritized), written as loops over ages and rows with Python integers for the sums - it shares nothing
with the torch path or the kernel.  tests/test_balanced_prioritized_cpu.py holds the torch path to it, tests/test_gpu_balanced_prioritized.py
the kernel.

A ring is tests/balanced_ref.py's dict with tests/priority_ref.py's ep_prio uint32 [capacity] beside ep_class.  The power is evaluated in float64
on the fp32 operands the kernel forms, as in priority_ref."""
import numpy as np

from tests import balanced_ref as br
from tests import priority_ref as pr

RING_FIELDS = pr.RING_FIELDS


def eligible(ring):
    """[(slot, priority, tag)] of the count - 1 oldest episodes, oldest first; a stored 0 reads as 1"""
    count, head, cap = int(ring["count"]), int(ring["head"]), int(ring["capacity"])
    out = []
    for age in range(max(count - 1, 0)):
        slot = (head - count + age) % cap
        out.append((slot, max(int(ring["ep_prio"][slot]), 1), int(ring["ep_class"][slot])))
    return out


def pick_ref(ring, n_slots, u_ep, n_classes, beta, rotation=0, draw=None):
    """per batch slot of this ring's segment: (ring slot, importance weight in float64, priority of the episode, pmin_c, T_c, t, class, m_c) -
    m_c == 0: the fallback, pmin, T and t over all eligible episodes"""
    count, head, cap = int(ring["count"]), int(ring["head"]), int(ring["capacity"])
    u_ep = np.asarray(u_ep, np.float32).reshape(n_slots)
    elig = eligible(ring)
    out, per_class = [], {}
    for i in range(n_slots):
        c = (i + int(rotation) + (0 if draw is None else int(draw))) % n_classes          # (Python's %: non-negative)
        if not elig:
            hi = max(count - 1, 1)
            k = min(int(u_ep[i] * np.float32(hi)), hi - 1)
            out.append(((head - count + k) % cap, 1.0, 0, 0, 0, 0, c, 0))
            continue
        if c not in per_class:                                            # (the class's masked priorities: the same for every slot that wants it)
            m_c = sum(1 for _, _, tag in elig if tag == c)
            masked = [(slot, p if (tag == c or m_c == 0) else 0) for slot, p, tag in elig]
            per_class[c] = (m_c, masked, sum(q for _, q in masked), min(q for _, q in masked if q > 0))
        m_c, masked, total, p_min = per_class[c]
        assert 0 < total < 2 ** 53
        t = min(total - 1, int(float(u_ep[i]) * float(total)))           # one double product: both factors are exact doubles
        run = 0
        for slot, q in masked:
            run += q
            if run > t:
                break
        assert q > 0
        ratio = np.float32(p_min) / np.float32(q)                         # two fp32 conversions and an fp32 division, as in the kernel
        out.append((slot, float(np.power(np.float64(ratio), np.float64(np.float32(beta)))), q, p_min, total, t, c, m_c))
    return out


def sample_ref(batch, horizon, n_steps, agent, u_ep, u_start, n_classes, beta, rotation=0, draw=None, expert=None, batch_agent=None):
    """The whole batch, priority_ref.sample_prioritized_ref's tuple: state, action, next_state, reward, not_done, weight (float64), picked int32
    [batch], next_ends [2 batch W, 82], and pick_ref's list, agent segment first."""
    W = horizon - n_steps
    batch_agent = batch if expert is None else int(batch_agent)
    u_ep, u_start = np.asarray(u_ep, np.float32).reshape(batch), np.asarray(u_start, np.float32).reshape(batch, W)
    picks = pick_ref(agent, batch_agent, u_ep[:batch_agent], n_classes, beta, rotation, draw)
    if batch > batch_agent:
        picks += pick_ref(expert, batch - batch_agent, u_ep[batch_agent:], n_classes, beta, rotation, draw)
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


# ---- the case list the CPU and the GPU test share ------------------------------------------------------------------------------------
CAP, B, B_AGENT, H, N_STEPS = pr.CAP, pr.B, pr.B_AGENT, pr.H, pr.N_STEPS           # 8 slots, 6 batch slots, 4 + 2, W = 5
COUNT_HEAD = pr.COUNT_HEAD
N_CLASSES = (1, 3, 64)
ROTATIONS = (-5, 0, 7)


def make_ring(cap, Hh, count, head, lens, tags, prio, rng):
    ring = pr.make_ring(cap, Hh, count, head, lens, prio, rng)
    ring["ep_class"] = np.asarray(tags, np.int32)
    return ring


def tag_patterns(n_classes, count, head, cap=CAP):
    """balanced_ref's patterns - cyclic; absent (a class with no episode: the fallback); newest_only (a class whose only member is the newest
    episode); unknown (age 0 tagged -1) - and `outside`: age 1 tagged n_classes + 2, a value at or above n_classes, beside a -1"""
    pats = br.tag_patterns(n_classes, count, head, cap)
    first = (head - count) % cap
    pats["outside"] = np.array([{0: -1, 1: n_classes + 2}.get((s - first) % cap, ((s - first) % cap) % n_classes) for s in range(cap)], np.int32)
    return pats


def expert_ring(rng, n_classes):
    """priority_ref's expert ring of 5 slots (count 4, head 2) with tags over the first two classes and one -1"""
    n = N_STEPS
    tags = np.array([0, 1 % n_classes, -1, 0, 1 % n_classes], np.int32)
    return make_ring(5, H, 4, 2, [n + 2, H, n + 1, H, n + 3], tags, [3 * pr.PRIO_ONE, 1, pr.PRIO_ONE // 7, pr.U32_MAX, 5], rng)


def power_of_two_ring(Hh, head, rng, cap=16):
    """a full ring of 16 slots, every priority 65536, whose 15 eligible episodes are 8, 4, 2 and 1 of classes 0 .. 3, interleaved by age (the
    newest is of class 0): the class sizes at which the balanced and the prioritized rule take the same floor on every uniform"""
    by_age = [0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 0, 0]
    first = (head - cap) % cap
    tags = np.array([by_age[(s - first) % cap] for s in range(cap)], np.int32)
    return make_ring(cap, Hh, cap, head, [Hh] * cap, tags, np.full(cap, pr.PRIO_ONE, np.uint32), rng)


def episode_uniforms(batch, ring, n_classes, rotation, shift):
    """u_ep [batch]: for slot i one of 0, 1 - 2^-24, 0.5 and the values on, just below and just above the first prefix-sum boundaries of the
    masked priorities of the class the slot wants (of all priorities where the class is empty); `shift` moves every slot through its list"""
    elig = eligible(ring)
    out = np.zeros(batch, np.float32)
    for i in range(batch):
        c = (i + rotation) % n_classes
        qs = [p for _, p, tag in elig if tag == c] or [p for _, p, _ in elig]
        pool, total, run = [0.0, pr.TOP, 0.5], sum(qs), 0
        for q in qs[:3]:
            run += q
            x = np.float32(run / max(total, 1))
            pool += [x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(1))]
        pool = [x for x in np.asarray(pool, np.float32) if 0 <= x < 1]
        out[i] = pool[(i + 4 * shift) % len(pool)]
    return out
