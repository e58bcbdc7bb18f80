"""Plain references of the replay and learner glue rules of include/kinova_rollout.h (the kr_* entry points of csrc/ks_rollout.hip),
one function per kernel, written from the header's rules and the reference's formulas (ddpgfd.py, replay.py docstrings) - not from
the kernels.  numpy on the host: float64 arithmetic on float32 inputs widened exactly (the scalars too: pass float(np.float32(tau))),
int64 / Python ints for the bookkeeping.  Nothing here rounds to float32 except the two products of the window sampler whose
truncation IS the rule (u_ep * hi and u_start * ceiling are float32 products in the reference's device form, replay.py).

tests/test_glue_reference_cpu.py checks these functions against torch.optim.Adam, float64 autograd of DDPGfD's losses and the torch
paths of DeviceEpisodeReplay / RolloutEngine; tests/test_gpu_glue_kernels.py then holds every kernel to them.
"""
import numpy as np

S, A = 82, 4


def wide(x):
    """a float32 array (or scalar) widened exactly to float64"""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64), x.dtype
    return x.astype(np.float64)


# ---- learner glue ----------------------------------------------------------------------------------------------------
def adam_ref(p, g, m, v, step, lr, b1, b2, eps, wd):
    """torch.optim.Adam, single tensor, weight decay as L2 added to the gradient; `step` is the number of THIS update
    (already incremented), step <= 0: nothing has produced a gradient yet and nothing changes.
        g' = g + wd p;  m' = m + (g' - m)(1 - b1);  v' = b2 v + (1 - b2) g'^2
        p' = p - lr / (1 - b1^step) * m' / (sqrt(v') / sqrt(1 - b2^step) + eps)
    Returns (p', m', v') in float64."""
    p, g, m, v = wide(p), wide(g), wide(m), wide(v)
    if step <= 0:
        return p, m, v
    g = g + wd * p if wd != 0 else g
    m1 = m + (g - m) * (1.0 - b1)
    v1 = v * b2 + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return p - (lr / bc1) * (m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps)), m1, v1


def soft_update_ref(p, tp, tau, it, freq):
    """target' = tau p + (1 - tau) target when the update counter `it` is a positive multiple of `freq`, else target"""
    p, tp = wide(p), wide(tp)
    if it > 0 and it % freq == 0:
        return tau * p + (1.0 - tau) * tp
    return tp


def critic_targets(tq1, tqn, reward, discount):
    """target_Q = r_0 + discount tq1  and  target_QN = sum_i discount^i r_i + discount^n tqn  (reward [R, n])"""
    reward = wide(reward)
    n = reward.shape[1]
    t1 = reward[:, 0] + discount * wide(tq1)
    tn = (reward * discount ** np.arange(n)).sum(1) + discount ** n * wide(tqn)
    return t1, tn


def critic_grad_ref(q, tq1, tqn, reward, weight, wsum, discount):
    """L1 = sum w (q - target_Q)^2 / wsum,  LN = sum w (q - target_QN)^2 / wsum,  loss = L1 + 0.5 LN,
    dq = w / wsum (2 (q - target_Q) + (q - target_QN));  weight None = all ones;  wsum <= 0 (an all-padding batch): everything 0.
    Returns dq [R] and (loss, L1, LN)."""
    q = wide(q)
    w = np.ones_like(q) if weight is None else wide(weight)
    t1, tn = critic_targets(tq1, tqn, reward, discount)
    if wsum <= 0:
        return np.zeros_like(q), (0.0, 0.0, 0.0)
    e1, en = q - t1, q - tn
    l1, ln = float((w * e1 * e1).sum() / wsum), float((w * en * en).sum() / wsum)
    return w / wsum * (2.0 * e1 + en), (l1 + 0.5 * ln, l1, ln)


def prologue_ref(rows, n, weight, it, it_head, pipelined):
    """start of an update: wsum = max(sum w, 1) (weight None = all ones), dq_actor [rows * n] = -w[row] / (wsum n)
    (dLoss/dQ of the actor loss -mean Q), it + 1, and it_head = it + 1 when pipelined.  Returns (wsum, dq_actor, it', it_head')."""
    w = np.ones(rows) if weight is None else wide(weight)
    wsum = max(float(w.sum()), 1.0)
    it = int(it) + 1
    return wsum, np.repeat(-w / (wsum * n), n), it, (it if pipelined else int(it_head))


def relu_backward_ref(act, grad):
    """g where the ReLU OUTPUT is positive, else +0 (float32 in, float32 out: nothing is computed)"""
    act, grad = np.asarray(act, np.float32), np.asarray(grad, np.float32)
    return np.where(act > 0, grad, np.float32(0.0)).astype(np.float32)


def sigmoid_scale_backward_ref(a, max_action, grad):
    """g a (1 - a / max_action): the backward of a = max_action sigmoid(z)"""
    a = wide(a)
    return wide(grad) * (a * (1.0 - a / max_action))


# ---- ring bookkeeping ------------------------------------------------------------------------------------------------
def rank_ref(keep):
    """rank[i] = number of kept envs among 0..i (inclusive), total = rank[n - 1]; a flag is set when its byte is non-zero"""
    rank = np.cumsum(np.asarray(keep) != 0, dtype=np.int64)
    return rank, int(rank[-1])


RING_FIELDS = ("state", "next", "action", "reward", "not_done")


def commit_ref(keep, rank, head, capacity, cur, cur_len, ep, ep_len):
    """kept env i goes to slot (head + rank[i] - 1) % capacity, whole [H, ...] rows and its length, in env order.
    cur / ep: dicts of the five RING_FIELDS ([n, H, ...] / [>= capacity, H, ...]); ep and ep_len are changed in place."""
    for i in np.flatnonzero(np.asarray(keep) != 0):
        slot = (int(head) + int(rank[i]) - 1) % capacity
        for f in RING_FIELDS:
            ep[f][slot] = cur[f][i]
        ep_len[slot] = cur_len[i]


def advance_ref(total, head, count, capacity, ended, cur_len):
    """head' = (head + total) % capacity, count' = min(capacity, count + total), cur_len = 0 where ended.  Returns (head', count', cur_len')"""
    return (int(head) + int(total)) % capacity, min(capacity, int(count) + int(total)), np.where(np.asarray(ended) != 0, 0, cur_len).astype(np.int64)


def store_transition_ref(i, horizon, n_steps, auto_reset, sim, eng, rep):
    """One env-step of env i after ks_step, in place.  sim: obs, final_obs [n, 82], reward [n], done uint8 [n] (non-zero = finished);
    eng: obs, prev_obs, has_prev, t, ready, lifting, action, reward_out, done_out; rep (None: no replay): cur_state .. cur_not_done,
    cur_len, keep.

      next_state = the terminal observation when the episode ended and the sim resets itself, else the new observation
      not lifting: replay_buffer.add - the transition goes to row min(cur_len, H - 1) of the env's open episode, cur_len = that + 1
      the episode ended during the lift: replace - the last stored transition (if any) takes the reward and not_done = 0
      keep = ended and cur_len - n_steps > 1
      prev_obs = the new observation for an env that starts over, else the state acted in; has_prev = not ended; t = 0 or t + 1;
      ready is dropped at the end of the episode."""
    done, lift = bool(sim["done"][i] != 0), bool(eng["lifting"][i] != 0)
    rew, new = sim["reward"][i], sim["obs"][i].copy()
    state = eng["obs"][i].copy()
    nxt = sim["final_obs"][i].copy() if (done and auto_reset) else new
    if rep is not None:
        length = int(rep["cur_len"][i])
        if not lift:
            row = min(length, horizon - 1)
            rep["cur_state"][i, row], rep["cur_next"][i, row], rep["cur_action"][i, row] = state, nxt, eng["action"][i]
            rep["cur_reward"][i, row], rep["cur_not_done"][i, row] = rew, 0.0 if done else 1.0
            length = row + 1
        if done and lift and length > 0:
            rep["cur_reward"][i, length - 1], rep["cur_not_done"][i, length - 1] = rew, 0.0
        rep["cur_len"][i] = length
        rep["keep"][i] = 1 if (done and length - n_steps > 1) else 0
    eng["prev_obs"][i] = new if done else state
    eng["obs"][i] = new
    eng["has_prev"][i] = 0 if done else 1
    eng["t"][i] = 0 if done else int(eng["t"][i]) + 1
    eng["ready"][i] = 1 if (eng["ready"][i] != 0 and not done) else 0
    eng["reward_out"][i] = rew
    eng["done_out"][i] = 1 if done else 0


def sample_windows_ref(batch, horizon, n_steps, ring, u_ep, u_start, expert=None, batch_agent=None):
    """sample_batch_nstep as one fixed-shape batch of batch * W rows, W = horizon - n_steps; with `expert`, episodes b >= batch_agent
    come from that ring, each ring with its own count / head / capacity.  ring: dict(count, head, capacity, ep_len, state, next,
    action, reward, not_done).  Per episode b:
        k = floor(u_ep[b] * max(count - 1, 1)) capped at max(count - 1, 1) - 1: the k-th OLDEST episode, slot (head - count + k) mod capacity
        ceiling = max(ep_len - n_steps, 1)
    and per row w: start = floor(u_start[b, w] * ceiling), the final window start = ceiling for w == ceiling - 1, both capped at W;
    weight 1 for w < ceiling when the ring holds at least two episodes, else 0.  Every row is defined, weight-0 rows too.
    The two products are float32.  Returns state, action, next_state, reward, not_done, weight and the (episode slot, start) per row."""
    W = horizon - n_steps
    u_ep, u_start = np.asarray(u_ep, np.float32).reshape(batch), np.asarray(u_start, np.float32).reshape(batch, W)
    out = {f: [] for f in RING_FIELDS}
    weight, picks = [], []
    for b in range(batch):
        g = ring if (expert is None or b < batch_agent) else expert
        count, head, cap = int(g["count"]), int(g["head"]), int(g["capacity"])
        hi = max(count - 1, 1)
        k = min(int(u_ep[b] * np.float32(hi)), hi - 1)
        slot = (head - count + k) % cap
        ceiling = max(int(g["ep_len"][slot]) - n_steps, 1)
        for w in range(W):
            start = min(int(u_start[b, w] * np.float32(ceiling)), W)
            if w == ceiling - 1:
                start = min(ceiling, W)
            for f in RING_FIELDS:
                out[f].append(g[f][slot, start:start + n_steps])
            weight.append(1.0 if (count >= 2 and w < ceiling) else 0.0)
            picks.append((slot, start))
    st = {f: np.stack(out[f]).astype(np.float32) for f in RING_FIELDS}
    return st["state"], st["action"], st["next"], st["reward"], st["not_done"], np.asarray(weight, np.float32), picks


# ---- the enumerated edge rows of kr_store_transition (shared by the host and the GPU test) ----------------------------
def store_cases(horizon, n_steps, seed=0, sentinel=None):
    """One env per combination of  done in {0, 1, 3} x lifting x cur_len in {0, 1, n+1, n+2, H-2, H-1, H} x ready x t in {0, 5}
    (168 envs).  Returns (sim, eng, rep) as store_transition_ref takes them; the open-episode rows hold distinct random data (or the
    float32 `sentinel` bit pattern), the outputs reward_out / done_out / keep a value the rule never writes."""
    import itertools
    H, n = horizon, n_steps
    combos = list(itertools.product((0, 1, 3), (0, 1), (0, 1, n + 1, n + 2, H - 2, H - 1, H), (0, 1), (0, 5)))
    N = len(combos)
    rng = np.random.RandomState(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    fill = (lambda *s: f(*s)) if sentinel is None else (lambda *s: np.full(s, sentinel, np.uint32).view(np.float32))
    c = np.array(combos, np.int64)
    sim = dict(obs=f(N, S), final_obs=f(N, S), reward=f(N) * 50, done=c[:, 0].astype(np.uint8))
    eng = dict(obs=f(N, S), prev_obs=f(N, S), has_prev=rng.randint(0, 2, N).astype(np.uint8), t=c[:, 4].copy(), ready=c[:, 3].astype(np.uint8),
               lifting=c[:, 1].astype(np.uint8), action=f(N, A), reward_out=np.full(N, -7.0, np.float32), done_out=np.full(N, 9, np.uint8))
    rep = dict(cur_state=fill(N, H, S), cur_next=fill(N, H, S), cur_action=fill(N, H, A), cur_reward=fill(N, H), cur_not_done=fill(N, H),
               cur_len=c[:, 2].copy(), keep=np.full(N, 9, np.uint8))
    return sim, eng, rep
