"""Plain numpy restatement of the class-balanced window sampler (include/kinova_rollout.h: kr_commit_classes, kr_sample_windows_balanced;
DeviceEpisodeReplay.sample_balanced), written as loops over ages and rows - it shares nothing with the torch path or the kernels.
tests/test_balanced_sampler_cpu.py holds the torch path to it, tests/test_gpu_balanced_sampler.py the kernels.

A ring is a dict(count, head, capacity, ep_len [capacity], ep_class [capacity], state / next [capacity, H, 82], action [capacity, H, 4],
reward / not_done [capacity, H]) - tests/glue_ref.py's ring with the class column."""
import numpy as np

RING_FIELDS = ("state", "next", "action", "reward", "not_done")


def commit_classes_ref(keep, rank, head, capacity, env_class, ep_class):
    """ep_class[(head + rank[i] - 1) % capacity] = env_class[i] for every kept env i, in place; nothing else is written"""
    for i in range(len(keep)):
        if keep[i] != 0:
            ep_class[(int(head) + int(rank[i]) - 1) % capacity] = env_class[i]
    return ep_class


def pick_ref(ring, n_slots, u_ep, n_classes, rotation=0, draw=None):
    """the ring slot of each of the n_slots batch slots of this ring's segment (u_ep: their episode uniforms), and the class each wanted
    with the number of eligible episodes it found there: [(slot, class, m_c), ...]"""
    count, head, cap = int(ring["count"]), int(ring["head"]), int(ring["capacity"])
    u_ep = np.asarray(u_ep, np.float32).reshape(n_slots)
    out = []
    for i in range(n_slots):
        c = (i + int(rotation) + (0 if draw is None else int(draw))) % n_classes          # (Python's %: non-negative)
        of_class = []                                                                   # the eligible episodes of class c, oldest first
        for age in range(max(count - 1, 0)):                                            # the newest episode, age count - 1, is never eligible
            slot = (head - count + age) % cap
            if int(ring["ep_class"][slot]) == c:
                of_class.append(slot)
        m = len(of_class)
        if m > 0:
            j = min(int(u_ep[i] * np.float32(m)), m - 1)
            out.append((of_class[j], c, m))
        else:
            hi = max(count - 1, 1)
            k = min(int(u_ep[i] * np.float32(hi)), hi - 1)
            out.append(((head - count + k) % cap, c, 0))
    return out


def sample_balanced_ref(batch, horizon, n_steps, agent, u_ep, u_start, n_classes, rotation=0, draw=None, expert=None, batch_agent=None):
    """The whole batch: state, action, next_state, reward, not_done, weight (kr_sample_windows' layout: batch * W rows, W = horizon - n_steps),
    picked int32 [batch], next_ends [2 batch W, 82] and the (slot, class, m_c) list of pick_ref, agent segment first."""
    W = horizon - n_steps
    batch_agent = batch if expert is None else int(batch_agent)
    u_ep, u_start = np.asarray(u_ep, np.float32).reshape(batch), np.asarray(u_start, np.float32).reshape(batch, W)
    picks = pick_ref(agent, batch_agent, u_ep[:batch_agent], n_classes, rotation, draw)
    if batch > batch_agent:
        picks += pick_ref(expert, batch - batch_agent, u_ep[batch_agent:], n_classes, rotation, draw)
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
            weight.append(1.0 if (int(g["count"]) >= 2 and w < ceiling) else 0.0)
    st = {f: np.stack(out[f]).astype(np.float32) for f in RING_FIELDS}
    ends = np.concatenate([st["next"][:, 0], st["next"][:, n_steps - 1]])
    return (st["state"], st["action"], st["next"], st["reward"], st["not_done"], np.asarray(weight, np.float32),
            np.asarray([p[0] for p in picks], np.int32), ends, picks)


# ---- the case list the CPU and the GPU test share -----------------------------------------------------------------------------------
CAP, B, N_STEPS = 8, 7, 5                        # (B = 7: no multiple of 2, 3 or 5)


def ring_lens(H, n):
    return [H, n + 2, n + 1, n, n - 1, H, n + 2, n + 1]


def make_ring(cap, H, count, head, lens, tags, rng):
    ring = dict(count=count, head=head, capacity=cap, ep_len=np.asarray(lens, np.int64), ep_class=np.asarray(tags, np.int32))
    S, A = 82, 4
    for f, s in dict(state=(cap, H, S), next=(cap, H, S), action=(cap, H, A), reward=(cap, H), not_done=(cap, H)).items():
        ring[f] = rng.standard_normal(s).astype(np.float32)
    return ring


def tag_patterns(n_classes, count, head, cap=CAP):
    """{name: tags [cap]} - cyclic: every class present; absent: class n_classes - 1 has no episode (n_classes > 1); newest_only: the
    last class's only episode is the newest one, which is never eligible, so its slots fall back; unknown: age 0 is tagged -1"""
    first = (head - count) % cap
    by_age = lambda f: np.array([f((s - first) % cap) for s in range(cap)], np.int32)
    pats = {"cyclic": by_age(lambda a: a % n_classes)}
    if n_classes > 1:
        pats["absent"] = by_age(lambda a: a % (n_classes - 1))
        pats["newest_only"] = by_age(lambda a: n_classes - 1 if a == count - 1 else a % (n_classes - 1))
    pats["unknown"] = by_age(lambda a: -1 if a == 0 else a % n_classes)
    return pats


def episode_uniforms(batch, m_values, shift):
    """u_ep [batch]: 0, the largest fp32 below 1, 0.5 and, for every class population m the case has, values whose product with m lands on
    m - 1 and on or beside an integer"""
    top = np.float32(np.nextafter(np.float32(1.0), np.float32(0.0)))
    pool = [0.0, top, 0.5]
    for m in sorted(set(int(v) for v in m_values if v > 0)):
        pool += [np.float32(m - 1) / np.float32(m), np.float32(1.0) / np.float32(m), np.nextafter(np.float32(m - 1) / np.float32(m), np.float32(1.0))]
    pool = np.asarray(pool, np.float32)
    pool = pool[pool < 1]
    return np.roll(np.resize(pool, max(batch, len(pool))), shift)[:batch].copy()


def start_uniforms(batch, W, shift):
    top = np.float32(1.0 - 2.0 ** -24)
    pool = np.asarray([0.0, 0.5, top] + [j / 25.0 for j in range(1, 25)] + [1.0 / 3, 2.0 / 3], np.float32)
    return np.stack([np.roll(pool, 5 * b + shift)[:W] for b in range(batch)])


COUNT_HEAD = [(0, 0), (1, 1), (2, 2), (5, 5), (8, 0), (8, 3), (8, 7), (5, 3), (2, 0), (5, 7), (1, 0), (0, 3)]   # count in {0,1,2,5,8} x head in {0,3,7} (wrapped)
N_CLASSES = (1, 2, 3, 5)


def small_cases():
    """(count, head, n_classes, pattern name, tags) over rings of capacity 8"""
    out = []
    for count, head in COUNT_HEAD:
        for nc in N_CLASSES:
            for name, tags in tag_patterns(nc, count, head).items():
                out.append((count, head, nc, name, tags))
    return out


def class_populations(ring, n_classes):
    count, head, cap = int(ring["count"]), int(ring["head"]), int(ring["capacity"])
    tags = [int(ring["ep_class"][(head - count + a) % cap]) for a in range(max(count - 1, 0))]
    return [tags.count(c) for c in range(n_classes)]
