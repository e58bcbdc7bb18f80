"""Experiment outputs in the reference's file formats: heatmap coordinate arrays, reward box-plot data
and the scalars its training loop sends to tensorboard.  The plots themselves (plotting_code/heatmap_plot.py,
boxplot_plot.py) and tensorboard are not reproduced; these are the data files they are drawn from.

    save_heatmap_coords   plotting_code/heatmap_coords.py:34-99 (filter_heatmap_coords -> save_coordinates)
    save_boxplot_rewards  main_DDPGfD.py:521-528
    ScalarLog             main_DDPGfD.py:310-330 (write_tensor_plot): same tags, written as JSON lines
    EpisodeLedger         eval_policy's per-episode bookkeeping (main_DDPGfD.py:130-272, add_heatmap_coords :310-330) for the episodes that
                          end inside the stepping kernels: folds the in-kernel episode log (sim.KinovaSim.episode_log)
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

ORIENTATIONS = ("normal", "rotated", "top")


def save_heatmap_coords(success_coords, fail_coords, episode_num, saving_dir):
    """Object start coordinates of an evaluation, split by outcome and hand orientation, as the reference writes them:
    <dir>/<orientation>/{success,fail,total}_{x,y}[_<episode>].npy + heatmap_info.txt.  `success_coords` / `fail_coords`:
    dicts with "x", "y", "orientation" lists (evaluate.eval_policy returns them).  As in the reference, the `total`
    arrays of an orientation are written once from the successes and then AGAIN from the failures when it has any
    (heatmap_coords.py:48-56), so they end up holding the failures wherever an orientation has both."""
    saving_dir = Path(saving_dir)
    idx = lambda c, o: [i for i, x in enumerate(c["orientation"]) if x == o]
    ep = "" if episode_num is None else "_" + str(episode_num)

    def write(coords, indexes, name):
        d = saving_dir / str(coords["orientation"][indexes[0]])
        d.mkdir(parents=True, exist_ok=True)
        np.save(d / f"{name}_x{ep}.npy", np.array([coords["x"][i] for i in indexes]))
        np.save(d / f"{name}_y{ep}.npy", np.array([coords["y"][i] for i in indexes]))

    s_idx, f_idx = [idx(success_coords, o) for o in ORIENTATIONS], [idx(fail_coords, o) for o in ORIENTATIONS]
    for il in s_idx:
        if il:
            write(success_coords, il, "success")
            write(success_coords, il, "total")
    for il in f_idx:
        if il:
            write(fail_coords, il, "fail")
            write(fail_coords, il, "total")
    saving_dir.mkdir(parents=True, exist_ok=True)
    text = (f"Heatmap Coords \nSaved at: {saving_dir}\n\nTotal # Success: {len(success_coords['x'])}\nTotal # Fail: {len(fail_coords['x'])}\n")
    for o, s, f in zip(("Normal", "Rotated", "Top"), s_idx, f_idx):
        text += f"\n{o} Orientation\n# Success: {len(s)}\n# Fail: {len(f)}\n"
    (saving_dir / "heatmap_info.txt").write_text(text)
    return text


def save_boxplot_rewards(boxplot_dir, episode_num, finger_reward, grasp_reward, lift_reward, total_reward):
    """finger/grasp/lift/total_reward_<episode>.npy (main_DDPGfD.py:525-528)"""
    d = Path(boxplot_dir)
    d.mkdir(parents=True, exist_ok=True)
    for name, v in (("finger_reward", finger_reward), ("grasp_reward", grasp_reward), ("lift_reward", lift_reward), ("total_reward", total_reward)):
        np.save(d / f"{name}_{episode_num}.npy", np.asarray(v, dtype=object) if _ragged(v) else np.asarray(v))


def _ragged(v):
    try:
        return len({len(x) for x in v}) > 1
    except TypeError:
        return False


class ScalarLog:
    """add_scalar(tag, value, step) like tensorboardX.SummaryWriter, appended to <dir>/scalars.jsonl; write_eval() uses
    the reference's tags (write_tensor_plot, main_DDPGfD.py:310-330)."""

    def __init__(self, log_dir, eval_freq: int = 200):
        self.dir = Path(log_dir)
        self.dir.mkdir(parents=True, exist_ok=True)
        self.path = self.dir / "scalars.jsonl"
        self.eval_freq = eval_freq

    def add_scalar(self, tag: str, value, step: int):
        with open(self.path, "a") as f:
            f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")

    def write_eval(self, episode_num, avg_reward, avg_rewards, actor_loss, critic_loss, critic_L1loss, critic_LNloss):
        k = f", Avg. {self.eval_freq} episodes"
        self.add_scalar("Episode total reward" + k, avg_reward, episode_num)
        self.add_scalar("Episode finger reward" + k, avg_rewards["finger_reward"], episode_num)
        self.add_scalar("Episode grasp reward" + k, avg_rewards["grasp_reward"], episode_num)
        self.add_scalar("Episode lift reward" + k, avg_rewards["lift_reward"], episode_num)
        self.add_scalar("Actor loss", actor_loss, episode_num)
        self.add_scalar("Critic loss", critic_loss, episode_num)
        self.add_scalar("Critic L1loss", critic_L1loss, episode_num)
        self.add_scalar("Critic LNloss", critic_LNloss, episode_num)

    def read(self):
        return [json.loads(l) for l in open(self.path)] if self.path.exists() else []


def param_success_table(records, mass, mu, mass_edges, mu_edges):
    """Which physical parameters succeeded: records (the in-kernel episode log's, sim.KinovaSim.episode_log(): `done` [m] is what is
    read) with the object mass [m] and object-hand friction [m] each record's episode ran with -> (attempts, successes), int64
    [len(mass_edges) - 1, len(mu_edges) - 1] per (mass bin, mu bin).  Bins are [edge_i, edge_i+1), the last one closed; a value outside
    the edges is not counted.  An episode is a success when it ended lifted (done bit 0).
    With per-episode ranges (sim.KinovaSim.set_param_ranges) set at the same boundary as the log, a record's `episode` ordinal IS the
    draw's episode number: mass, mu = scenarios.param_draw_reference(seed, records["env"], records["episode"], ranges, dtype)."""
    host = lambda v: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    done, mass, mu = host(records["done"]).astype(np.int64).ravel(), host(mass).astype(np.float64).ravel(), host(mu).astype(np.float64).ravel()
    me, ue = np.asarray(mass_edges, dtype=np.float64), np.asarray(mu_edges, dtype=np.float64)
    if not (len(done) == len(mass) == len(mu)):
        raise ValueError("param_success_table: one mass and one mu per record")
    if len(me) < 2 or len(ue) < 2 or (np.diff(me) <= 0).any() or (np.diff(ue) <= 0).any():
        raise ValueError("param_success_table: edges must be increasing, at least two")

    def bins(v, edges):
        i = np.searchsorted(edges, v, side="right") - 1
        i[v == edges[-1]] = len(edges) - 2
        return i, (i >= 0) & (i < len(edges) - 1)

    (i, oki), (j, okj) = bins(mass, me), bins(mu, ue)
    keep = oki & okj
    attempts = np.zeros((len(me) - 1, len(ue) - 1), dtype=np.int64)
    successes = np.zeros_like(attempts)
    np.add.at(attempts, (i[keep], j[keep]), 1)
    np.add.at(successes, (i[keep], j[keep]), (done[keep] & 1))
    return attempts, successes


class EpisodeLedger:
    """Which env, object and start succeeded: the fold of the in-kernel episode log's records (sim.KinovaSim.episode_log(); include/
    kinova_sim.h: ks_episode_record).  add(records) accumulates, as torch ops on the device the records live on:
        totals, success_rate()             an episode is a success when it ended lifted (done bit 0: the 50-point lift reward)
        per_object()                       attempts / successes / mean steps of every object of the context  [n_objects]
        attempts_table / successes_table   with a start pool (starts_per_env = K): [N, K] counts per (env, pool entry)
        coords(classes)                    success_coords / fail_coords dicts {x, y, orientation} as save_heatmap_coords takes them
    Records without a pool entry (start_index -1: no pool) count in the totals and per object only.  keep_coords=False drops the
    per-episode start coordinates (a long training run that only wants the tables)."""

    def __init__(self, n_envs: int, n_objects: int, starts_per_env: int | None = None, keep_coords: bool = True):
        self.n_envs, self.n_objects, self.starts_per_env = int(n_envs), int(n_objects), (int(starts_per_env) if starts_per_env else None)
        self.keep_coords = keep_coords
        self.episodes = self.successes = self.lost = 0
        self._dev = None
        self._coords = []

    def _tables(self, dev):
        import torch
        if self._dev is None:
            self._dev = dev
            z = lambda *shape: torch.zeros(*shape, dtype=torch.long, device=dev)
            self.object_attempts, self.object_successes, self.object_steps = z(self.n_objects), z(self.n_objects), z(self.n_objects)
            if self.starts_per_env:
                self.attempts_table, self.successes_table = z(self.n_envs, self.starts_per_env), z(self.n_envs, self.starts_per_env)

    def add(self, records: dict):
        """records: env, object, start_index, steps, done [m] and start_xy [m, 2] (extra keys are ignored; `lost` is summed)"""
        import torch
        env, obj, start = records["env"].long(), records["object"].long(), records["start_index"].long()
        self._tables(env.device)
        self.lost += int(records.get("lost", 0))
        if env.numel() == 0:
            return self
        ok = (records["done"] & 1) != 0
        okl = ok.long()
        self.object_attempts.index_add_(0, obj, torch.ones_like(obj))
        self.object_successes.index_add_(0, obj, okl)
        self.object_steps.index_add_(0, obj, records["steps"].long())
        if self.starts_per_env:
            pooled = start >= 0
            flat = (env * self.starts_per_env + start)[pooled]
            self.attempts_table.view(-1).index_add_(0, flat, torch.ones_like(flat))
            self.successes_table.view(-1).index_add_(0, flat, okl[pooled])
        if self.keep_coords:
            self._coords.append((env, start, records["start_xy"].float(), ok))
        self.episodes += int(env.numel())
        self.successes += int(okl.sum())
        return self

    def success_rate(self) -> float:
        return self.successes / self.episodes if self.episodes else 0.0

    def per_object(self, names=None) -> dict:
        """{object (or names[object]): {"attempts", "successes", "mean_steps"}} for every object of the context"""
        if self._dev is None:
            a = s = t = [0] * self.n_objects
        else:
            a, s, t = self.object_attempts.tolist(), self.object_successes.tolist(), self.object_steps.tolist()
        return {(names[i] if names is not None else i): {"attempts": a[i], "successes": s[i], "mean_steps": (t[i] / a[i] if a[i] else 0.0)}
                for i in range(self.n_objects)}

    def coords(self, classes, clear: bool = False):
        """(success_coords, fail_coords) of the episodes added so far (since the last clear).  classes: the orientation class of every
        pool entry as scenarios.draw_start_pool returns it ([K, N] array of "normal" / "rotated" / "top": a record's orientation is
        classes[start_index, env]); or [N] (one class per env), or one string - the only forms a record without a pool entry can use."""
        import torch
        if isinstance(classes, str):
            look = lambda e, j: np.full(len(e), classes, dtype=object)
        else:
            cl = np.asarray(classes, dtype=object)
            if cl.ndim == 1:
                look = lambda e, j: cl[e]
            else:
                def look(e, j):
                    if (j < 0).any():
                        raise ValueError("EpisodeLedger.coords: records without a pool entry need one class per env, not a [K, N] table")
                    return cl[j, e]
        if self._coords:
            env, start, xy, ok = (torch.cat([c[i] for c in self._coords]).cpu().numpy() for i in range(4))
        else:
            env, start, xy, ok = np.zeros(0, int), np.zeros(0, int), np.zeros((0, 2), np.float32), np.zeros(0, bool)
        orient = look(env, start)
        pick = lambda m: {"x": xy[m, 0].tolist(), "y": xy[m, 1].tolist(), "orientation": [str(o) for o in orient[m]]}
        if clear:
            self._coords = []
        return pick(ok), pick(~ok)
