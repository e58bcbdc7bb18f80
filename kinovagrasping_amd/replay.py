"""Episode replay for n-step DDPGfD (L4): restatement of ReplayBuffer_Queue (gym-kinova-gripper/utils.py:9-343)
as (a) a host sampler that consumes the same np.random stream as the reference (golden-vector parity)
and (b) a device-resident, fixed-shape episode ring for the batched rollout.

Reference semantics kept (utils.py:240-306): episodes drawn with np.random.randint(replay_ep_num - 1)
(the newest episode is never sampled); for an episode of length L, ceiling = L - n windows:
ceiling - 1 uniform random starts in [0, ceiling) plus the final window starting at `ceiling`.
"""
from __future__ import annotations

import ctypes
import json
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch


def sample_windows_host(ep_lens, n_steps: int, batch_size: int, rng=np.random):
    """Exactly the draws of ReplayBuffer_Queue.sample_batch_nstep: returns [(episode, start), ...]."""
    out = []
    if batch_size < 1:
        return out
    episode_idx = rng.randint(len(ep_lens) - 1, size=batch_size)
    for idx in episode_idx:
        ceiling = int(ep_lens[idx]) - n_steps
        for _ in range(ceiling - 1):
            out.append((int(idx), int(rng.randint(ceiling))))
        out.append((int(idx), ceiling))
    return out


# ---- the reference's on-disk replay bundle (utils.py:345-390): a directory of .npy files, each the pickled
# nested list the buffer holds in memory - state / action / next_state / reward / not_done: one list per episode
# (+ the empty list of the episode being filled), episodes: [first, last] timestep counters per episode,
# episodes_info: [max_episode, size, episodes_count, replay_ep_num], orientation_indexes.
_BUNDLE_FIELDS = ("state", "action", "next_state", "reward", "not_done")


def _object_rows(rows):
    out = np.empty(len(rows), dtype=object)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def save_reference_bundle(dirpath, episodes, max_episode=10000, orientation_indexes=None):
    """Write episodes (list of dicts with the five _BUNDLE_FIELDS, each [L, ...] array) in the layout
    ReplayBuffer_Queue.save_replay_buffer produces, readable by store_saved_data_into_replay (utils.py:367-400)."""
    d = Path(dirpath)
    d.mkdir(parents=True, exist_ok=True)
    for f in _BUNDLE_FIELDS:
        rows = []
        for ep in episodes:
            a = np.asarray(ep[f])
            rows.append([np.asarray(x, dtype=np.float64) if a.ndim > 1 else float(x) for x in a])
        rows.append([])                                         # the open episode
        np.save(d / f, _object_rows(rows), allow_pickle=True)
    lens = [len(np.asarray(ep["reward"])) for ep in episodes]
    np.save(d / "episodes", _object_rows([[0, n] for n in lens] + [[]]), allow_pickle=True)
    np.save(d / "episodes_info", np.array([max_episode, sum(lens), len(lens), len(lens)]))
    np.save(d / "orientation_indexes", _object_rows(list(orientation_indexes) if orientation_indexes is not None else []), allow_pickle=True)


def load_reference_bundle(dirpath):
    """Read a bundle written by the reference (or by save_reference_bundle): list of episode dicts of float32 arrays
    (empty trailing episodes dropped) + the episodes_info vector."""
    d = Path(dirpath)
    cols = {f: np.load(d / (f + ".npy"), allow_pickle=True) for f in _BUNDLE_FIELDS}
    n = len(cols["reward"])
    episodes = []
    for i in range(n):
        if len(cols["reward"][i]) == 0:
            continue
        episodes.append({f: np.asarray([np.asarray(x, dtype=np.float32) for x in cols[f][i]], dtype=np.float32) for f in _BUNDLE_FIELDS})
    info = np.load(d / "episodes_info.npy", allow_pickle=True)
    return episodes, np.asarray(info, dtype=np.int64)


class HostEpisodeReplay:
    """Flat-array host replay with the reference's sampler; used for expert data and parity tests."""

    def __init__(self, state_dim=82, action_dim=4, n_steps=5):
        self.n_steps = n_steps
        self.lens, self.offsets = [], []
        self.state, self.action, self.next_state, self.reward, self.not_done = [], [], [], [], []

    def add_episode_arrays(self, state, action, next_state, reward, not_done):
        self.offsets.append(sum(self.lens))
        self.lens.append(len(reward))
        for lst, arr in ((self.state, state), (self.action, action), (self.next_state, next_state), (self.reward, reward), (self.not_done, not_done)):
            lst.append(np.asarray(arr, dtype=np.float32))

    @property
    def replay_ep_num(self):
        return len(self.lens)

    def episodes(self):
        return [dict(state=self.state[i], action=self.action[i], next_state=self.next_state[i], reward=self.reward[i], not_done=self.not_done[i])
                for i in range(len(self.lens))]

    def save(self, dirpath, max_episode=10000):
        """the reference's replay bundle (utils.py:345-365)"""
        save_reference_bundle(dirpath, self.episodes(), max_episode)

    def load(self, dirpath):
        """append the episodes of a reference replay bundle (utils.py:367-400)"""
        eps, info = load_reference_bundle(dirpath)
        for ep in eps:
            self.add_episode_arrays(ep["state"], ep["action"], ep["next_state"], ep["reward"], ep["not_done"])
        return info

    def sample_batch_nstep(self, batch_size, num_ts_from_ep=5, rng=np.random):
        wins = sample_windows_host(self.lens, self.n_steps, batch_size, rng)
        n = self.n_steps
        pick = lambda lst: torch.from_numpy(np.stack([lst[e][s:s + n] for e, s in wins])) if wins else torch.zeros(0)
        return pick(self.state), pick(self.action), pick(self.next_state), pick(self.reward), pick(self.not_done)


CLASS_SIDECAR = "episode_classes.json"      # beside the reference bundle's files: DeviceEpisodeReplay.save / load
PRIO_ONE = 65536                            # priority 1.0 in ep_prio's unit of 1 / 65536 (include/kinova_rollout.h)
PRIO_MAX_CAPACITY = 1 << 20                 # the largest ring kr_sample_windows_prioritized takes: sums of priorities stay exact as double


def _i32_bits(value: int) -> int:
    """the int32 with the bit pattern of the uint32 `value` (torch's uint32 has few kernels: tables are written through an int32 view)"""
    value = int(value) & 0xFFFFFFFF
    return value - (1 << 32) if value >= (1 << 31) else value


class TableBatch(NamedTuple):
    """A replay batch as episode tables (DeviceEpisodeReplay.sample_tables; include/kinova_rollout.h: kr_sample_tables_mixed).  B batch
    episodes, H = horizon, W = H - n_steps, R = B * W window rows."""
    table_state: torch.Tensor      # [B * H, S] row b * H + t: row t of batch slot b's episode, as the ring holds it
    table_next: torch.Tensor       # [B * H, S]
    table_action: torch.Tensor     # [B * H, A]
    row_table: torch.Tensor        # int32 [R]: b * H + start of window row (b, w), padding rows included
    slot_weight: torch.Tensor      # [B]: the weight every real window row of slot b carries
    state0: torch.Tensor           # [R, S] the window rows' first state ...
    action0: torch.Tensor          # [R, A] ... and action
    reward: torch.Tensor           # [R, n]
    not_done: torch.Tensor         # [R, n]
    weight: torch.Tensor           # [R]
    n_steps: int
    horizon: int
    next_ends: torch.Tensor | None = None      # [2 R, S] on request: next_state[:, 0] and next_state[:, -1] stacked (a TD3fD learner's target rows)
    picked: torch.Tensor | None = None         # int32 [B] behind a balanced or prioritized pick: the ring slot of every batch episode

    def windows(self):
        """the window form of the same batch: (state [R, n, S], action [R, n, A], next_state, reward, not_done, weight), every bit what
        sample_mixed returns for the same draws"""
        t = self.row_table.long().unsqueeze(1) + torch.arange(self.n_steps, device=self.row_table.device)
        return self.table_state[t], self.table_action[t], self.table_next[t], self.reward, self.not_done, self.weight


class DeviceEpisodeReplay:
    """Fixed-shape episode ring on the GPU: [capacity, horizon, ...] plus per-episode lengths.
    Envs append to their own open episode; a finished episode is committed to the ring (FIFO).

    Every method is a fixed sequence of fixed-shape device ops - no host synchronisation, no data-dependent
    shapes - so a whole rollout step can be captured in a HIP graph.  Masked rows are handled with
    torch.where; episodes that are not committed are copied to a trash row behind the ring."""

    def __init__(self, n_envs, capacity, horizon=30, state_dim=82, action_dim=4, n_steps=5, device="cuda"):
        self.n_envs, self.capacity, self.horizon, self.n_steps = n_envs, capacity, horizon, n_steps
        self.device = torch.device(device)
        z = lambda *s: torch.zeros(*s, device=self.device)
        rows = capacity + 1                                # row `capacity` is the trash row
        self.ep_state, self.ep_next = z(rows, horizon, state_dim), z(rows, horizon, state_dim)
        self.ep_action, self.ep_reward, self.ep_not_done = z(rows, horizon, action_dim), z(rows, horizon), z(rows, horizon)
        self.ep_len = torch.zeros(rows, dtype=torch.long, device=self.device)
        self._count = torch.zeros((), dtype=torch.long, device=self.device)   # committed episodes
        self._head = torch.zeros((), dtype=torch.long, device=self.device)    # next ring slot
        self.cur_state, self.cur_next = z(n_envs, horizon, state_dim), z(n_envs, horizon, state_dim)
        self.cur_action, self.cur_reward, self.cur_not_done = z(n_envs, horizon, action_dim), z(n_envs, horizon), z(n_envs, horizon)
        self.cur_len = torch.zeros(n_envs, dtype=torch.long, device=self.device)
        self._env_ar = torch.arange(n_envs, device=self.device)
        self._all = torch.ones(n_envs, dtype=torch.bool, device=self.device)
        self._row = torch.arange(horizon - n_steps, device=self.device).unsqueeze(0)
        self._win = torch.arange(n_steps, device=self.device)
        self.env_class = self.ep_class = self.class_names = None          # per-episode class column: set_env_classes
        self.ep_prio = self.prio_max = None                                # per-episode priority column: enable_priorities
        # on a GPU the bookkeeping runs as the kr_* kernels of libkinova_sim.so (include/kinova_rollout.h), one launch
        # per method instead of a dozen torch ops; the torch code below is the same arithmetic (and their checker)
        self.native = self.device.type == "cuda"
        if self.native:
            from . import sim as _sim
            self._lib, self._ptr = _sim.load_library(), _sim._ptr
            self._rank = torch.zeros(n_envs, dtype=torch.long, device=self.device)
            self._total = torch.zeros(1, dtype=torch.long, device=self.device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc})")

    @property
    def count(self):
        """committed episodes (host read: synchronises)"""
        return int(self._count)

    @property
    def head(self):
        return int(self._head)

    def add(self, state, action, next_state, reward, done, store_mask=None):
        """Append one transition per env (where store_mask is True; utils.py:34-64)."""
        m = self._all if store_mask is None else store_mask
        ar, t = self._env_ar, self.cur_len.clamp(max=self.horizon - 1)
        mc = m.unsqueeze(1)
        self.cur_state[ar, t] = torch.where(mc, state, self.cur_state[ar, t])
        self.cur_next[ar, t] = torch.where(mc, next_state, self.cur_next[ar, t])
        self.cur_action[ar, t] = torch.where(mc, action, self.cur_action[ar, t])
        self.cur_reward[ar, t] = torch.where(m, reward, self.cur_reward[ar, t])
        self.cur_not_done[ar, t] = torch.where(m, 1.0 - done.float(), self.cur_not_done[ar, t])
        self.cur_len.copy_(torch.where(m, t + 1, self.cur_len))

    def replace_last(self, env_mask, reward):
        """utils.py:309-343: overwrite the last stored transition of the open episode with the lift outcome."""
        m = env_mask & (self.cur_len > 0)
        ar, last = self._env_ar, (self.cur_len - 1).clamp(min=0)
        self.cur_reward[ar, last] = torch.where(m, reward, self.cur_reward[ar, last])
        self.cur_not_done[ar, last] = torch.where(m, torch.zeros_like(reward), self.cur_not_done[ar, last])

    def end_episodes(self, env_mask):
        """Commit the open episodes of `env_mask` envs in env order; episodes with len - n <= 1 are dropped
        (main_DDPGfD.py:469-471).  Returns the number committed as a 0-d device tensor."""
        keep = env_mask & (self.cur_len - self.n_steps > 1)
        if self.native:
            return self.commit_native(keep, env_mask)
        rank = torch.cumsum(keep.long(), 0) - 1
        slots = torch.where(keep, (self._head + rank) % self.capacity, torch.full_like(rank, self.capacity))
        self.ep_state.index_copy_(0, slots, self.cur_state)
        self.ep_next.index_copy_(0, slots, self.cur_next)
        self.ep_action.index_copy_(0, slots, self.cur_action)
        self.ep_reward.index_copy_(0, slots, self.cur_reward)
        self.ep_not_done.index_copy_(0, slots, self.cur_not_done)
        self.ep_len.index_copy_(0, slots, self.cur_len)
        if self.ep_class is not None:
            self.ep_class.index_copy_(0, slots, self.env_class)
        if self.ep_prio is not None:                       # (kr_commit_priorities; an env that is not kept rewrites the trash row with itself)
            table, top = self.ep_prio.view(torch.int32), self.prio_max.view(torch.int32)
            enter = torch.where(top == 0, torch.ones_like(top), top).expand(self.n_envs)
            table.index_copy_(0, slots, torch.where(keep, enter, table[slots]))
        k = keep.sum()
        self._head.copy_((self._head + k) % self.capacity)
        self._count.copy_((self._count + k).clamp(max=self.capacity))
        self.cur_len.copy_(torch.where(env_mask, torch.zeros_like(self.cur_len), self.cur_len))
        return k

    def host_episodes(self):
        """committed episodes, oldest first, as numpy dicts (synchronises)"""
        cnt, head = self.count, self.head
        first = (head - cnt) % self.capacity
        out = []
        for k in range(cnt):
            s = (first + k) % self.capacity
            L = int(self.ep_len[s])
            out.append(dict(state=self.ep_state[s, :L].cpu().numpy(), action=self.ep_action[s, :L].cpu().numpy(),
                            next_state=self.ep_next[s, :L].cpu().numpy(), reward=self.ep_reward[s, :L].cpu().numpy(),
                            not_done=self.ep_not_done[s, :L].cpu().numpy()))
        return out

    def save(self, dirpath, max_episode=None):
        """the reference's replay bundle (utils.py:345-365).  With classes set (set_env_classes) the directory also gets the sidecar
        CLASS_SIDECAR - the class names and the class index of every saved episode, oldest first -, which the reference's loader, reading
        its files by name, never opens; the bundle's own files are what they are without classes."""
        save_reference_bundle(dirpath, self.host_episodes(), self.capacity if max_episode is None else max_episode)
        if self.ep_class is not None:
            cnt, head = self.count, self.head
            slots = (head - cnt + torch.arange(cnt, device=self.device)) % self.capacity
            (Path(dirpath) / CLASS_SIDECAR).write_text(json.dumps({"class_names": list(self.class_names),
                                                                   "episode_class": [int(c) for c in self.ep_class[slots].tolist()]}))

    def load(self, dirpath, class_id=None):
        """append the episodes of a reference replay bundle to the ring (episodes longer than the horizon are cut).  On a ring with classes
        every loaded episode is tagged `class_id` when one is given; else by the bundle's sidecar (save), its class NAMES mapped onto this
        ring's - a name this ring does not know, like a bundle without a sidecar, gives -1: the episode belongs to no class.  On a ring with
        priorities (enable_priorities) every loaded episode enters at the ring's current prio_max, as a committed one does."""
        eps, info = load_reference_bundle(dirpath)
        tags = None
        if self.ep_class is not None:
            tags = [-1 if class_id is None else int(class_id)] * len(eps)
            if class_id is not None and not -1 <= int(class_id) < len(self.class_names):
                raise ValueError(f"load: class_id {class_id} is not one of the ring's {len(self.class_names)} classes")
            side = Path(dirpath) / CLASS_SIDECAR
            if class_id is None and side.is_file():
                rec = json.loads(side.read_text())
                known = {name: i for i, name in enumerate(self.class_names)}
                if len(rec["episode_class"]) == len(eps):            # (a sidecar of another bundle's length says nothing about this one)
                    tags = [known.get(rec["class_names"][c], -1) if 0 <= c < len(rec["class_names"]) else -1 for c in rec["episode_class"]]
        for i, ep in enumerate(eps):
            L = min(len(ep["reward"]), self.horizon)
            s = int(self._head)
            for name, key in (("ep_state", "state"), ("ep_next", "next_state"), ("ep_action", "action"), ("ep_reward", "reward"), ("ep_not_done", "not_done")):
                getattr(self, name)[s, :L] = torch.as_tensor(ep[key][:L]).to(self.device)
            self.ep_len[s] = L
            if tags is not None:
                self.ep_class[s] = tags[i]
            if self.ep_prio is not None:
                self.ep_prio.view(torch.int32)[s] = _i32_bits(max(self.priority_max(), 1))
            self._head.copy_((self._head + 1) % self.capacity)
            self._count.copy_((self._count + 1).clamp(max=self.capacity))
        return info

    def set_env_classes(self, env_class, class_names):
        """Give the ring a per-episode class column: env_class int [n_envs] - the class of whatever env i collects (an index into
        class_names; None: -1 for every env, a ring that is only loaded into, such as an expert ring) -, class_names the classes' names
        (1 .. 64 of them).  Allocates ep_class int32 [capacity + 1] filled with -1 (the episodes the ring already holds belong to no
        class); from here on every commit - commit_native, both buffers of commit_published, the torch path of end_episodes - tags
        the slots it fills (kr_commit_classes between the rank and the advance), load / save carry the tags and sample_balanced can
        draw by them.  Without this call nothing about the ring changes."""
        names = [str(c) for c in class_names]
        if not 1 <= len(names) <= 64 or len(set(names)) != len(names):
            raise ValueError("set_env_classes: 1 .. 64 distinct class names")
        if env_class is None:
            env_class = torch.full((self.n_envs,), -1, dtype=torch.int32)
        env_class = torch.as_tensor(env_class)
        if env_class.shape != (self.n_envs,) or env_class.dtype.is_floating_point or env_class.dtype == torch.bool:
            raise ValueError("set_env_classes: env_class is an int tensor [n_envs]")
        if env_class.numel() and not (-1 <= int(env_class.min()) and int(env_class.max()) < len(names)):
            raise ValueError("set_env_classes: env_class values are indices into class_names (or -1)")
        self.env_class = env_class.to(device=self.device, dtype=torch.int32).contiguous()
        self.class_names = names
        self.ep_class = torch.full((self.capacity + 1,), -1, dtype=torch.int32, device=self.device)

    def enable_priorities(self):
        """Give the ring a per-episode priority column for prioritized replay (sample_prioritized / update_priorities): ep_prio uint32
        [capacity + 1] in units of 1 / PRIO_ONE - the episodes the ring already holds get PRIO_ONE, priority 1.0 - and prio_max uint32 [1],
        the largest priority an update has written, PRIO_ONE at first.  From here on every commit - commit_native, both buffers of
        commit_published, the torch path of end_episodes - gives the slots it fills the current prio_max (kr_commit_priorities beside
        kr_commit_classes), and load does the same: a new episode is sampled soon.  Priorities are transient: save writes the reference
        bundle (and the class sidecar) and nothing about them, a loaded ring starts over.  Without this call nothing about the ring changes."""
        if self.ep_prio is not None:
            return
        if self.capacity > PRIO_MAX_CAPACITY:
            raise ValueError(f"enable_priorities: a ring of at most {PRIO_MAX_CAPACITY} episodes (the sum of the priorities must stay exact as a double)")
        self.ep_prio = torch.full((self.capacity + 1,), PRIO_ONE, dtype=torch.uint32, device=self.device)
        self.prio_max = torch.full((1,), PRIO_ONE, dtype=torch.uint32, device=self.device)

    def priorities(self):
        """ep_prio as int64 [capacity + 1] (a copy; torch's uint32 has few kernels)"""
        return self.ep_prio.view(torch.int32).long() & 0xFFFFFFFF

    def priority_max(self) -> int:
        """prio_max (host read: synchronises)"""
        return int(self.prio_max.view(torch.int32).item()) & 0xFFFFFFFF

    def _commit_priorities(self, keep, st):
        """kr_commit_priorities behind a kr_rank_episodes on the same keep (a ring without priorities: nothing)"""
        if self.ep_prio is not None:
            P = self._ptr
            self._check(self._lib.kr_commit_priorities(self.n_envs, self.capacity, P(keep), P(self._rank), P(self._head), P(self.prio_max),
                                                       P(self.ep_prio), st), "kr_commit_priorities")

    def _commit_classes(self, keep, st):
        """kr_commit_classes behind a kr_rank_episodes on the same keep (a ring without classes: nothing)"""
        if self.ep_class is not None:
            P = self._ptr
            self._check(self._lib.kr_commit_classes(self.n_envs, self.capacity, P(keep), P(self._rank), P(self._head), P(self.env_class),
                                                    P(self.ep_class), st), "kr_commit_classes")

    def enable_async(self):
        """Open-episode buffers of the free-running rollout kernel (ks_rollout): TWO per env, so that an env can start its next
        episode while the learner's stream has not yet moved the finished one into the ring.  a_* [2, n, H, ...], a_len [2, n],
        a_sel [n] (which one is open), pub_len [2, n] (> 0: a finished episode of that length awaits commit_published)."""
        if hasattr(self, "pub_len"):
            return
        n, H, dev = self.n_envs, self.horizon, self.device
        S, A = self.ep_state.shape[2], self.ep_action.shape[2]
        z = lambda *sh, **k: torch.zeros(*sh, device=dev, **k)
        self.a_state, self.a_next, self.a_action = z(2, n, H, S), z(2, n, H, S), z(2, n, H, A)
        self.a_reward, self.a_not_done = z(2, n, H), z(2, n, H)
        self.a_len, self.pub_len = z(2, n, dtype=torch.long), z(2, n, dtype=torch.long)
        self.a_sel = z(n, dtype=torch.uint8)
        self._keep2 = torch.zeros(2, n, dtype=torch.bool, device=dev)

    def commit_published(self, into=None):
        """Move every published episode (pub_len > 0) of both buffers into the ring, buffer 0 first, env order within a buffer,
        and free the buffers (commit_episodes with the published lengths as cur_len).
        into: another ring that takes the episodes instead (AsyncTrainer's staging ring), and only as many as it has free rows - a row
        it holds is never overwritten: what does not fit stays published in its buffer (a rank, the clip, then commit_episodes' own rank).
        Fixed-shape device ops: capturable; runs on the learner's stream ahead of the window sampling."""
        for b in (0, 1):
            keep = self._keep2[b]
            torch.gt(self.pub_len[b], 0, out=keep)
            if into is not None:
                into._rank_episodes(keep, into._stream())
                torch.logical_and(keep, into._rank + into._count <= into.capacity, out=keep)
            (self if into is None else into).commit_episodes((self.a_state[b], self.a_next[b], self.a_action[b], self.a_reward[b], self.a_not_done[b]),
                                                             self.pub_len[b], keep, keep)

    def commit_native(self, keep, ended):
        """rank -> commit -> advance with the kr_* kernels; keep / ended: bool [n_envs]"""
        self.commit_episodes((self.cur_state, self.cur_next, self.cur_action, self.cur_reward, self.cur_not_done), self.cur_len, keep, ended)
        return self._total[0]

    def _rank_episodes(self, keep, st):
        self._check(self._lib.kr_rank_episodes(keep.shape[0], self._ptr(keep), self._ptr(self._rank), self._ptr(self._total), st), "kr_rank_episodes")

    def _commit_rows(self, src, src_len, keep, rank, st):
        """kr_commit_episodes: row i of src (state, next_state, action, reward, not_done) with keep[i] -> ring slot head + rank[i], the others -> the trash row"""
        P = self._ptr
        self._check(self._lib.kr_commit_episodes(keep.shape[0], self.horizon, self.capacity, P(keep), P(rank), P(self._head), *[P(x) for x in src], P(src_len),
                                                 P(self.ep_state), P(self.ep_next), P(self.ep_action), P(self.ep_reward), P(self.ep_not_done),
                                                 P(self.ep_len), st), "kr_commit_episodes")

    def _advance_ring(self, ended, src_len, st):
        """kr_advance_ring: head and count move by the ranked total, src_len[i] = 0 where ended[i]"""
        P = self._ptr
        self._check(self._lib.kr_advance_ring(ended.shape[0], self.capacity, P(self._total), P(self._head), P(self._count), P(ended), P(src_len), st),
                    "kr_advance_ring")

    def commit_episodes(self, src, src_len, keep, ended):
        """How an episode enters the ring on the GPU: rank -> commit -> classes -> priorities -> advance, one kr_* launch each (the last two only on
        a ring that has the column).  src: the open-episode buffers (state, next_state, action, reward, not_done), [n_envs, horizon, ...] each, and
        src_len int64 [n_envs] their lengths; keep bool [n_envs]: the rows that enter, in env order; ended bool [n_envs]: the rows whose src_len
        is reset to 0.  Fixed-shape device ops: capturable."""
        st = self._stream()
        self._rank_episodes(keep, st)
        self._commit_rows(src, src_len, keep, self._rank, st)
        self._commit_classes(keep, st)
        self._commit_priorities(keep, st)
        self._advance_ring(ended, src_len, st)

    def commit_ranked(self, src, src_len, keep, rank, total):
        """commit_episodes for rows the caller has ranked itself: row i of src ([n, horizon, ...] each, any n) with keep[i] enters at slot
        head + rank[i]; total int64 [1]: how many enter; the kept rows' src_len is reset.  No rank launch, and nothing is tagged: for a ring
        without classes and priorities (AsyncTrainer's launch boundary, staged rows in key order)."""
        st = self._stream()
        self._total.copy_(total)
        self._commit_rows(src, src_len, keep, rank, st)
        self._advance_ring(keep, src_len, st)

    def _ring(self):
        from .sim import KrRing
        P = lambda t: t.data_ptr()
        return KrRing(P(self._count), P(self._head), self.capacity, P(self.ep_len), P(self.ep_state), P(self.ep_next), P(self.ep_action),
                      P(self.ep_reward), P(self.ep_not_done))

    def _sample_native(self, entry, expert, batch_size, b_agent, pick_args, uniforms, draw, seed, generator, with_picked):
        """The native front end of every sampler: one call of libkinova_sim's `entry` (kr_sample_windows_mixed, or an entry point with its
        argument list plus pick_args - what only its pick needs - behind the rings and `picked` behind next_ends).  Allocates the batch, the
        7th tensor exactly when `draw` is given without `uniforms`, and `picked` on request; the uniforms are the caller's, torch.rand's
        (neither uniforms nor draw) or the kernel's own (draw).  expert=None: this ring serves as both."""
        n, W = self.n_steps, self.horizon - self.n_steps
        R, dev = batch_size * W, self.device
        S, A = self.ep_state.shape[2], self.ep_action.shape[2]
        out = (torch.empty(R, n, S, device=dev), torch.empty(R, n, A, device=dev), torch.empty(R, n, S, device=dev),
               torch.empty(R, n, device=dev), torch.empty(R, n, device=dev), torch.empty(R, device=dev))
        picked = (torch.empty(batch_size, dtype=torch.int32, device=dev),) if with_picked else ()
        P = self._ptr
        ends = (torch.empty(2 * R, S, device=dev),) if (draw is not None and uniforms is None) else ()
        if uniforms is None and draw is None:
            uniforms = torch.rand(batch_size * (W + 1), device=dev, generator=generator)
        u = None if uniforms is None else uniforms.contiguous()
        ra = self._ring()
        re = ra if expert is None else expert._ring()
        self._check(getattr(self._lib, entry)(batch_size, b_agent, self.horizon, n, ctypes.byref(ra), ctypes.byref(re), *pick_args, P(u),
                                              P(u[batch_size:]) if u is not None else None, int(seed) & (2 ** 64 - 1), P(draw),
                                              P(out[0]), P(out[1]), P(out[2]), P(out[3]), P(out[4]), P(out[5]), P(ends[0]) if ends else None,
                                              *[P(t) for t in picked], self._stream()), entry)
        return out + ends + picked

    def _sample_torch(self, expert, batch_size, b_agent, uniforms, generator, pick):
        """The torch front end of the two-ring samplers (the checker of the kernels): batch slots [0, b_agent) from this ring, the others from
        `expert`.  pick(ring, ue) -> (the ring slot of every batch slot of the ring's segment, ue [nb] its episode uniforms; the episodes'
        weights or None).  Returns the six batch tensors and the picked slots int32 [batch_size]."""
        W = self.horizon - self.n_steps
        if uniforms is None:
            uniforms = torch.rand(batch_size * (W + 1), device=self.device, generator=generator)
        ue, us = uniforms[:batch_size], uniforms[batch_size:].view(batch_size, W)
        parts, picks = [], []
        for ring, lo, hi in ((self, 0, b_agent), (expert, b_agent, batch_size)):
            if hi > lo:
                slot, w_ep = pick(ring, ue[lo:hi])
                rows = list(ring._windows_of(slot, us[lo:hi]))
                if w_ep is not None:
                    rows[5] = rows[5] * w_ep.repeat_interleave(W)               # (0 / 1 times the episode's weight)
                picks.append(slot)
                parts.append(rows)
        return tuple(torch.cat([p[k] for p in parts], 0) for k in range(6)) + (torch.cat(picks).to(torch.int32),)

    def sample_mixed(self, expert: "DeviceEpisodeReplay", batch_size, prob=0.3, uniforms=None, draw=None, seed=0, generator=None):
        """DDPGfD's batch (DDPGfD.train_batch, DDPGfD.py:232-254): agent_batch_size = int(batch_size * (1 - prob)) episodes from THIS
        ring followed by batch_size - agent_batch_size episodes from `expert`, each sampled with sample_batch_nstep's rule on its own
        ring.  Same return layout as sample_batch_nstep (incl. the 7th tensor when `draw` is given).  One kernel launch on the GPU
        (kr_sample_windows_mixed); the torch path below - the concatenation of two sample_batch_nstep calls - is its checker."""
        if expert.horizon != self.horizon or expert.n_steps != self.n_steps:
            raise ValueError("sample_mixed: the expert ring must have the agent ring's horizon and n_steps")
        b_agent = int(batch_size * (1 - prob))
        if self.native and expert.native:
            return self._sample_native("kr_sample_windows_mixed", expert, batch_size, b_agent, (), uniforms, draw if uniforms is None else None, seed,
                                       generator, False)
        return self._sample_torch(expert, batch_size, b_agent, uniforms, generator, lambda ring, ue: (ring._pick_uniform(ue), None))[:6]

    def sample_batch_nstep(self, batch_size, generator=None, uniforms=None, draw=None, seed=0):
        """Fixed-shape batch: batch_size episodes x (horizon - n) window rows, padding rows have weight 0.
        Returns state [R,n,S], action [R,n,A], next_state [R,n,S], reward [R,n], not_done [R,n], weight [R].
        `uniforms` (optional, tests): the batch_size + batch_size*W numbers in [0,1) to use instead of torch.rand.
        `draw` (native path): a device int64 counter that differs from call to call (the learner's update count) - the
        uniforms are then drawn inside the kernel (Philox keyed by `seed`; no torch generator, hence none of its state
        launches in a captured graph) and a 7th tensor is returned: next_state[:, 0] and next_state[:, -1] stacked
        [2R, S], the rows the target networks evaluate."""
        W = self.horizon - self.n_steps
        if self.native:                                    # (kr_sample_windows_mixed with this ring as both: kr_sample_windows' launch, or _draw's)
            return self._sample_native("kr_sample_windows_mixed", None, batch_size, batch_size, (), uniforms, draw if uniforms is None else None, seed,
                                       generator, False)
        ue = torch.rand(batch_size, device=self.device, generator=generator) if uniforms is None else uniforms[:batch_size]
        ep = self._pick_uniform(ue)
        u = torch.rand(batch_size, W, device=self.device, generator=generator) if uniforms is None else uniforms[batch_size:].view(batch_size, W)
        return self._windows_of(ep, u)

    def _pick_uniform(self, ue):
        """sample_batch_nstep's pick (torch path): the k-th oldest episode, k in [0, count - 1) - the newest one (ring slot head - 1) is never
        sampled (utils.py:259) -, ue [nb] the episode uniforms"""
        hi = (self._count - 1).clamp(min=1)
        k = torch.minimum((ue * hi).long(), hi - 1)
        return (self._head - self._count + k) % self.capacity

    def _windows_of(self, ep, u):
        """the window rows of the episodes in ring slots ep [B] with the start uniforms u [B, W] (torch path)"""
        n, W, batch_size = self.n_steps, self.horizon - self.n_steps, ep.shape[0]
        start, weight = self._starts_of(ep, u)
        t = start.unsqueeze(-1) + self._win                                  # [B,W,n]
        e = ep.view(-1, 1, 1).expand(-1, W, n)
        g = lambda x: x[e, t].reshape(batch_size * W, n, *x.shape[2:])
        return g(self.ep_state), g(self.ep_action), g(self.ep_next), g(self.ep_reward), g(self.ep_not_done), weight

    def _starts_of(self, ep, u):
        """where the W windows of the episodes in ring slots ep [B] start, [B, W] (start uniforms u [B, W]), and the rows' 0 / 1 weights [B * W]"""
        n, W = self.n_steps, self.horizon - self.n_steps
        ceiling = (self.ep_len[ep] - n).clamp(min=1)       # [B]
        row = self._row                                                      # [1,W]
        start = (u * ceiling.unsqueeze(1)).long().clamp(max=self.horizon - n)
        start = torch.where(row == (ceiling.unsqueeze(1) - 1), ceiling.unsqueeze(1).expand(-1, W), start)
        start = start.clamp(max=self.horizon - n)
        weight = ((row < ceiling.unsqueeze(1)) & (self._count >= 2)).float().reshape(-1)     # nothing to sample from < 2 episodes
        return start, weight

    def sample_tables(self, expert, batch_size, prob=0.3, uniforms=None, draw=None, seed=0, generator=None, next_ends=False, balanced=False,
                      prioritized=False, beta=1.0, rotation=0):
        """sample_mixed's batch (expert None: sample_batch_nstep's; balanced / prioritized: sample_balanced's, sample_prioritized's or
        sample_balanced_prioritized's, with their `rotation` and `beta`, their requirements of the rings, and `picked` in the result)
        as EPISODE TABLES, a TableBatch: the same draws, but every batch episode's
        `horizon` ring rows once (table_state / table_next [B * H, S], table_action [B * H, A]) and per window row the index of its first state (row_table), the
        weight of the slot's real rows (slot_weight [B]) and what the critic phase reads at R = B * W rows (state0, action0, reward,
        not_done, weight).  TableBatch.windows() is sample_mixed's batch bit for bit.  The learner evaluates the B * H table rows where
        the window form makes it evaluate the B * W * n window states drawn from them (NativeDDPGfDUpdate.phase_critic_tables /
        phase_actor_tables).  On the GPU one launch (kr_sample_tables_mixed), behind a pick two (kr_sample_tables_balanced, _prioritized,
        _balanced_prioritized: the window samplers' pick, the table gather); the torch path is their checker."""
        if expert is not None and (expert.horizon != self.horizon or expert.n_steps != self.n_steps):
            raise ValueError("sample_tables: the expert ring must have the agent ring's horizon and n_steps")
        both = [self] + ([expert] if expert is not None else [])
        if balanced and (any(r.ep_class is None for r in both) or any(r.class_names != self.class_names for r in both)):
            raise ValueError("sample_tables: balanced needs rings with the same classes (set_env_classes)")
        if prioritized and any(r.ep_prio is None for r in both):
            raise ValueError("sample_tables: prioritized needs rings with priorities (enable_priorities)")
        if prioritized:
            beta = self._beta_tensor(beta, "sample_tables")
        b_agent = batch_size if expert is None else int(batch_size * (1 - prob))
        n, H, W, dev = self.n_steps, self.horizon, self.horizon - self.n_steps, self.device
        S, A = self.ep_state.shape[2], self.ep_action.shape[2]
        R, T = batch_size * W, batch_size * H
        if self.native and (expert is None or expert.native):
            f = lambda *shape: torch.empty(*shape, device=dev)
            out = TableBatch(f(T, S), f(T, S), f(T, A), torch.empty(R, dtype=torch.int32, device=dev), f(batch_size), f(R, S), f(R, A), f(R, n), f(R, n), f(R), n, H,
                             f(2 * R, S) if next_ends else None, torch.empty(batch_size, dtype=torch.int32, device=dev) if (balanced or prioritized) else None)
            if uniforms is None and draw is None:
                uniforms = torch.rand(batch_size * (W + 1), device=dev, generator=generator)
            u = None if uniforms is None else uniforms.contiguous()
            P = self._ptr
            ra = self._ring()
            re = ra if expert is None else expert._ring()
            other = lambda t: None if expert is None else P(getattr(expert, t))
            pick_args = ((P(self.ep_class), other("ep_class"), len(self.class_names), int(rotation)) if balanced else ()) + \
                        ((P(self.ep_prio), other("ep_prio"), P(beta)) if prioritized else ())
            entry = "kr_sample_tables_" + ("_".join(k for k, on in (("balanced", balanced), ("prioritized", prioritized)) if on) or "mixed")
            # (a pick rotates with the draw counter whatever the uniforms are, as in the window samplers; kr_sample_tables_mixed takes one or the other)
            d = draw if (balanced or prioritized or u is None) else None
            self._check(getattr(self._lib, entry)(batch_size, b_agent, H, n, ctypes.byref(ra), ctypes.byref(re), *pick_args, P(u),
                                                  P(u[batch_size:]) if u is not None else None, int(seed) & (2 ** 64 - 1), P(d),
                                                  *[P(t) for t in out[:10]], P(out.next_ends), *([P(out.picked)] if out.picked is not None else []),
                                                  self._stream()), entry)
            return out
        if uniforms is None:
            uniforms = torch.rand(batch_size * (W + 1), device=dev, generator=generator)
        ue, us = uniforms[:batch_size], uniforms[batch_size:].view(batch_size, W)
        parts, picks = [], []
        for ring, lo, hi in ((self, 0, b_agent), (expert, b_agent, batch_size)):
            if hi > lo:
                w_ep, dd = None, (0 if draw is None else int(draw))
                if balanced and prioritized:
                    ep, w_ep = ring._pick_balanced_prioritized(ue[lo:hi], rotation, dd, beta)
                elif prioritized:
                    ep, w_ep = ring._pick_prioritized(ue[lo:hi], beta)
                else:
                    ep = ring._pick_balanced(ue[lo:hi], rotation, dd) if balanced else ring._pick_uniform(ue[lo:hi])
                start, weight = ring._starts_of(ep, us[lo:hi])
                if w_ep is not None:
                    weight = weight * w_ep.repeat_interleave(W)                  # (0 / 1 times the episode's weight)
                picks.append(ep.to(torch.int32))
                src = (ep.view(-1, 1), start)                                    # the window rows' first ring rows
                row_table = (torch.arange(lo, hi, device=dev).view(-1, 1) * H + start).reshape(-1).to(torch.int32)
                parts.append((ring.ep_state[ep].reshape(-1, S), ring.ep_next[ep].reshape(-1, S), ring.ep_action[ep].reshape(-1, A), row_table, torch.ones(hi - lo, device=dev) if w_ep is None else w_ep,
                              ring.ep_state[src].reshape(-1, S), ring.ep_action[src].reshape(-1, A),
                              ring.ep_reward[ep.view(-1, 1, 1), start.unsqueeze(-1) + ring._win].reshape(-1, n),
                              ring.ep_not_done[ep.view(-1, 1, 1), start.unsqueeze(-1) + ring._win].reshape(-1, n), weight))
        tb = TableBatch(*[torch.cat([p[k] for p in parts], 0) for k in range(10)], n, H, None, torch.cat(picks) if (balanced or prioritized) else None)
        if next_ends:
            nx = tb.windows()[2]
            tb = tb._replace(next_ends=torch.cat([nx[:, 0], nx[:, -1]], 0))
        return tb

    def _pick_balanced(self, ue, rotation, d):
        """sample_balanced's pick on this ring (torch path, the checker of k_pick_balanced): the ring slot of every batch slot of the
        ring's segment, ue [nb] its episode uniforms"""
        nb, cap, nc = ue.shape[0], self.capacity, len(self.class_names)
        cnt, head = self._count, self._head
        ages = torch.arange(cap - 1, device=self.device)                     # eligible: ages 0 .. count - 2
        slots = (head - cnt + ages) % cap
        tags = torch.where(ages < cnt - 1, self.ep_class[slots].long(), torch.full_like(ages, -1))
        want = (torch.arange(nb, device=self.device) + int(rotation) + d) % nc           # (non-negative: the divisor's sign)
        match = tags.unsqueeze(0) == want.unsqueeze(1)                       # [nb, cap - 1]
        m = match.sum(1)
        j = torch.minimum((ue * m.float()).long(), m - 1)
        at = (match & (match.cumsum(1) == (j + 1).unsqueeze(1))).long().argmax(1) if cap > 1 else torch.zeros_like(m)
        return torch.where(m > 0, (head - cnt + at) % cap, self._pick_uniform(ue))

    def sample_balanced(self, expert, batch_size, prob=0.3, uniforms=None, draw=None, seed=0, rotation=0, generator=None):
        """sample_mixed with every batch episode drawn from ONE class of its ring (set_env_classes), the classes in cyclic rotation: slot i
        of a ring's segment of the batch - agent [0, b_agent), expert [b_agent, batch_size); expert=None: one ring, the whole batch - wants
        class (i + rotation + draw) mod n_classes and takes the floor(u * m)-th oldest of that class's m eligible episodes (the newest
        episode of the ring is never eligible); a class without eligible episodes falls back to sample_batch_nstep's draw over all of
        them.  So whatever the ring holds, the classes' shares of a segment differ by one slot at most, and over n_classes consecutive
        draws each class gets exactly the segment's length.  Return layout of sample_mixed, then `picked` int32 [batch_size]: the ring
        slot every batch episode was read from.  On the GPU two launches (kr_sample_windows_balanced: the pick, the gather); the torch
        path below is the same rule and their checker."""
        if self.ep_class is None or (expert is not None and expert.ep_class is None):
            raise ValueError("sample_balanced: the ring has no classes (set_env_classes)")
        if expert is not None and (expert.horizon != self.horizon or expert.n_steps != self.n_steps or expert.class_names != self.class_names):
            raise ValueError("sample_balanced: the expert ring must have the agent ring's horizon, n_steps and class names")
        b_agent = batch_size if expert is None else int(batch_size * (1 - prob))
        if self.native and (expert is None or expert.native):
            tables = (self._ptr(self.ep_class), None if expert is None else self._ptr(expert.ep_class), len(self.class_names), int(rotation))
            return self._sample_native("kr_sample_windows_balanced", expert, batch_size, b_agent, tables, uniforms, draw, seed, generator, True)
        d = 0 if draw is None else int(draw)
        return self._sample_torch(expert, batch_size, b_agent, uniforms, generator, lambda ring, ue: (ring._pick_balanced(ue, rotation, d), None))

    def _pick_prioritized(self, ue, beta):
        """sample_prioritized's pick on this ring (torch path, the checker of k_pick_prioritized): the ring slot of every batch slot of the
        ring's segment, ue [nb] its episode uniforms, and the episodes' importance weights.  Integer arithmetic up to the two fp32
        conversions of the weight; the power itself is taken in fp64 and rounded once."""
        cap, cnt, head = self.capacity, self._count, self._head
        ages = torch.arange(max(cap - 1, 1), device=self.device)            # eligible: ages 0 .. count - 2
        slots = (head - cnt + ages) % cap
        prio = self.priorities()[slots].clamp(min=1)
        inside = ages < cnt - 1
        prio = torch.where(inside, prio, torch.zeros_like(prio))
        csum = prio.cumsum(0)                                                # int64: below 2^52
        total = csum[-1]
        t = torch.minimum((ue.double() * total.double()).long(), (total - 1).clamp(min=0))
        at = (csum.unsqueeze(0) > t.unsqueeze(1)).long().argmax(1)          # the smallest age whose inclusive prefix sum exceeds t
        least = torch.where(inside, prio, torch.full_like(prio, 1 << 32)).min()
        ratio = least.float() / prio[at].clamp(min=1).float()
        weight = torch.pow(ratio.double(), beta.to(self.device).float().double()).float()
        some = total > 0
        return torch.where(some, (head - cnt + at) % cap, self._pick_uniform(ue)), torch.where(some, weight, torch.ones_like(weight))

    def sample_prioritized(self, expert, batch_size, prob=0.3, beta=1.0, uniforms=None, draw=None, seed=0, generator=None):
        """sample_mixed with every batch episode drawn in proportion to its priority within its ring (enable_priorities): with T the sum of
        the priorities of the ring's eligible episodes - the count - 1 oldest - and u the slot's episode uniform, the episode at the
        smallest age whose inclusive prefix sum exceeds min(T - 1, floor((double)u * T)).  Its real window rows carry the importance weight
        (p_min / p)^beta in the weight column - 1 for the ring's least likely episode, smaller for the others -, padding rows 0; the
        learner's weighted means (kr_update_prologue, kr_critic_grad, phase_actor) take it from there.  expert=None: one ring, the whole
        batch.  beta: a float, or a device float tensor [1] that a captured graph reads at every replay.  Return layout of sample_balanced,
        ending in `picked` int32 [batch_size]: the ring slot every batch episode was read from, which update_priorities needs.  On the GPU
        two launches (kr_sample_windows_prioritized: the pick, the gather); the torch path below is the same rule and their checker."""
        if self.ep_prio is None or (expert is not None and expert.ep_prio is None):
            raise ValueError("sample_prioritized: the ring has no priorities (enable_priorities)")
        if expert is not None and (expert.horizon != self.horizon or expert.n_steps != self.n_steps):
            raise ValueError("sample_prioritized: the expert ring must have the agent ring's horizon and n_steps")
        b_agent = batch_size if expert is None else int(batch_size * (1 - prob))
        beta = self._beta_tensor(beta, "sample_prioritized")
        if self.native and (expert is None or expert.native):
            tables = (self._ptr(self.ep_prio), None if expert is None else self._ptr(expert.ep_prio), self._ptr(beta))
            return self._sample_native("kr_sample_windows_prioritized", expert, batch_size, b_agent, tables, uniforms, draw, seed, generator, True)
        return self._sample_torch(expert, batch_size, b_agent, uniforms, generator, lambda ring, ue: ring._pick_prioritized(ue, beta))

    def _beta_tensor(self, beta, what):
        if not torch.is_tensor(beta):
            beta = torch.full((1,), float(beta), device=self.device)
        if beta.dtype != torch.float32 or beta.numel() != 1:
            raise ValueError(f"{what}: beta is a float or a float32 tensor with one element")
        return beta

    def _pick_balanced_prioritized(self, ue, rotation, d, beta):
        """sample_balanced_prioritized's pick on this ring (torch path, the checker of k_pick_balanced_prioritized): _pick_balanced's class
        for every batch slot of the ring's segment, then _pick_prioritized's rule and weight over the eligible episodes of that class -
        over all of them where the class has none.  ue [nb] the episode uniforms."""
        nb, cap, nc = ue.shape[0], self.capacity, len(self.class_names)
        cnt, head = self._count, self._head
        ages = torch.arange(max(cap - 1, 1), device=self.device)            # eligible: ages 0 .. count - 2
        slots = (head - cnt + ages) % cap
        inside = ages < cnt - 1
        prio = self.priorities()[slots].clamp(min=1)
        prio = torch.where(inside, prio, torch.zeros_like(prio))
        tags = torch.where(inside, self.ep_class[slots].long(), torch.full_like(ages, -1))
        want = (torch.arange(nb, device=self.device) + int(rotation) + d) % nc           # (non-negative: the divisor's sign)
        match = tags.unsqueeze(0) == want.unsqueeze(1)                       # [nb, cap - 1]
        mask = (match | ~match.any(1, keepdim=True)) & inside.unsqueeze(0)   # a class without eligible episodes: everybody
        q = torch.where(mask, prio.unsqueeze(0), torch.zeros_like(prio).unsqueeze(0))
        csum = q.cumsum(1)                                                   # int64: below 2^52
        total = csum[:, -1]
        t = torch.minimum((ue.double() * total.double()).long(), (total - 1).clamp(min=0))
        at = (csum > t.unsqueeze(1)).long().argmax(1)                       # the smallest age whose inclusive prefix sum exceeds t
        least = torch.where(mask, prio.unsqueeze(0), torch.full_like(q, 1 << 32)).min(1).values
        ratio = least.float() / prio[at].clamp(min=1).float()
        weight = torch.pow(ratio.double(), beta.to(self.device).float().double()).float()
        some = total > 0
        return torch.where(some, (head - cnt + at) % cap, self._pick_uniform(ue)), torch.where(some, weight, torch.ones_like(weight))

    def sample_balanced_prioritized(self, expert, batch_size, prob=0.3, beta=1.0, uniforms=None, draw=None, seed=0, rotation=0, generator=None):
        """sample_balanced and sample_prioritized combined (the ring has both columns: set_env_classes, enable_priorities): slot i of a
        ring's segment of the batch wants class (i + rotation + draw) mod n_classes, as in sample_balanced, and draws among the eligible
        episodes of that class in proportion to their priorities, as sample_prioritized does among all of them: with T_c their sum, the
        episode at the smallest age whose inclusive prefix sum of the class's priorities exceeds min(T_c - 1, floor((double)u * T_c)).  Its
        real rows carry (pmin_c / p)^beta, pmin_c the least priority of the class: the weight that corrects the draw back to
        sample_balanced's, uniform within the class, over its maximum over the class.  A class without eligible episodes falls back to
        sample_prioritized's draw and weight over all of them.  So the classes' shares of a segment are sample_balanced's whatever the
        priorities are.  Arguments and return layout of sample_prioritized, `rotation` of sample_balanced.  On the GPU two launches
        (kr_sample_windows_balanced_prioritized: the pick, the gather); the torch path is the same rule and their checker."""
        if self.ep_class is None or (expert is not None and expert.ep_class is None):
            raise ValueError("sample_balanced_prioritized: the ring has no classes (set_env_classes)")
        if self.ep_prio is None or (expert is not None and expert.ep_prio is None):
            raise ValueError("sample_balanced_prioritized: the ring has no priorities (enable_priorities)")
        if expert is not None and (expert.horizon != self.horizon or expert.n_steps != self.n_steps or expert.class_names != self.class_names):
            raise ValueError("sample_balanced_prioritized: the expert ring must have the agent ring's horizon, n_steps and class names")
        b_agent = batch_size if expert is None else int(batch_size * (1 - prob))
        beta = self._beta_tensor(beta, "sample_balanced_prioritized")
        if self.native and (expert is None or expert.native):
            P = self._ptr
            tables = (P(self.ep_class), None if expert is None else P(expert.ep_class), len(self.class_names), int(rotation),
                      P(self.ep_prio), None if expert is None else P(expert.ep_prio), P(beta))
            return self._sample_native("kr_sample_windows_balanced_prioritized", expert, batch_size, b_agent, tables, uniforms, draw, seed, generator,
                                       True)
        d = 0 if draw is None else int(draw)
        return self._sample_torch(expert, batch_size, b_agent, uniforms, generator,
                                  lambda ring, ue: ring._pick_balanced_prioritized(ue, rotation, d, beta))

    def update_priorities(self, expert, q, tq1, reward, weight, picked, prob=0.3, discount=0.995, alpha=0.3, eps=1e-3, eps_expert=1.0, delta_out=None):
        """kr_update_priorities: after the critic's forward on a batch of sample_prioritized - q [R], tq1 [R] (the 1-step target critic's
        values), reward [R, n], weight [R], picked [batch] - every picked episode's priority becomes (delta + eps)^alpha in ep_prio's unit,
        delta its largest 1-step TD error over its real rows; expert episodes (batch slots from int(batch * (1 - prob)) on; expert=None:
        none) use eps_expert, the demonstration bonus, and the expert ring's table and prio_max.  An episode picked twice gets the larger
        value, one without a finite error stays as it is.  delta_out (optional) float [batch].  GPU only: it has no torch path."""
        if self.ep_prio is None or (expert is not None and expert.ep_prio is None):
            raise ValueError("update_priorities: the ring has no priorities (enable_priorities)")
        if not self.native or (expert is not None and not expert.native):
            raise ValueError("update_priorities needs device rings (DeviceEpisodeReplay on the GPU)")
        batch = picked.shape[0]
        b_agent = batch if expert is None else int(batch * (1 - prob))
        P = self._ptr
        self._check(self._lib.kr_update_priorities(batch, b_agent, self.horizon, self.n_steps, P(q), P(tq1), P(reward), P(weight), float(discount), P(picked),
                                                   float(alpha), float(eps), float(eps_expert), P(self.ep_prio), None if expert is None else P(expert.ep_prio),
                                                   P(self.prio_max), None if expert is None else P(expert.prio_max), P(delta_out), self._stream()),
                    "kr_update_priorities")
