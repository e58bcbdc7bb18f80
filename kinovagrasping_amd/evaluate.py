"""Batched policy evaluation: the counterpart of eval_policy in
gym-kinova-gripper/main_DDPGfD.py:130-272 with one evaluation episode per env.

As in the reference: the deterministic policy acts (no exploration noise) until check_grasp - after >= 6 steps -
latches the lift (main_DDPGfD.py:179-196), then the scripted lift action [0.6, 0.5, 0.5, 0.5] is repeated until the
episode ends (eval_lift_hand, main_DDPGfD.py:293-307); an episode is a success when a step reward exceeds 25
(the 50-point lift reward, main_DDPGfD.py:222-223); start coordinates of the object in the palm frame are
collected per outcome for the success / fail heatmaps (add_heatmap_coords, main_DDPGfD.py:310-330).
"""
from __future__ import annotations

import torch

from .rollout import LIFT_ACTION, SKIP_NUM_TS, check_grasp


@torch.no_grad()
def eval_policy(sim, policy, obs0: torch.Tensor, horizon: int = 30, orientation: str = "normal"):
    """One evaluation episode per env of `sim` (auto_reset off, or horizon <= the sim's).  obs0 [N, 82] from the reset.
    Returns the reference's result dict: avg_reward, avg_rewards{total,finger,grasp,lift}, all_ep_reward_values,
    num_success, success_coords / fail_coords {x, y, orientation} (object start position in the palm frame), plus
    `success` [N] bool and `steps` [N] tensors."""
    n, dev = sim.n_envs, sim.device
    obs = obs0.clone()
    start_xy = obs0[:, 21:23].clone()                       # Tfw . object position (main_DDPGfD.py:166-171) = obs[21:24]
    prev = None
    ready = torch.zeros(n, dtype=torch.bool, device=dev)
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    success = torch.zeros(n, dtype=torch.bool, device=dev)
    steps = torch.zeros(n, dtype=torch.long, device=dev)
    totals = torch.zeros(4, n, device=dev)                  # total, finger, grasp, lift reward per episode
    lift = torch.tensor(LIFT_ACTION, device=dev).expand(n, 4)
    for t in range(horizon):
        if prev is not None and t + 1 >= SKIP_NUM_TS:
            ready |= check_grasp(prev[:, 9:17], obs[:, 9:17]) & alive
        action = torch.where(ready.unsqueeze(1), lift, policy.select_action(obs))
        state = obs
        nobs, reward, done, info = sim.step(action.t().contiguous())
        live = alive.float()
        totals[0] += reward * live
        totals[1:] += info * live
        steps += alive.long()
        done_b = (done != 0) & alive
        success |= alive & (reward > 25)
        alive &= ~done_b
        prev, obs = state, nobs.clone()
    xs, ys = start_xy[:, 0].cpu().numpy(), start_xy[:, 1].cpu().numpy()
    ok = success.cpu().numpy()
    coords = lambda m: {"x": xs[m].tolist(), "y": ys[m].tolist(), "orientation": [orientation] * int(m.sum())}
    tot = totals.cpu().numpy()
    names = ("total_reward", "finger_reward", "grasp_reward", "lift_reward")
    return {"avg_reward": float(tot[0].mean()), "avg_rewards": {k: float(tot[i].mean()) for i, k in enumerate(names)},
            "all_ep_reward_values": {k: tot[i].tolist() for i, k in enumerate(names)}, "num_success": int(ok.sum()),
            "success_coords": coords(ok), "fail_coords": coords(~ok), "success": success, "steps": steps}


@torch.no_grad()
def eval_policy_free_running(sim, policy, episodes_per_env: int = 1, obs0: torch.Tensor | None = None, classes="normal", chunk: int | None = None,
                             max_launches: int | None = None, object_names=None):
    """eval_policy on the free-running path: the deterministic policy runs through ks_rollout (in-kernel actor, sigma = 0, nothing
    stored: with_replay = 0) on an AUTO-RESET context, whose stepping kernel writes one record per finished episode into the context's
    episode log (sim.set_episode_log) - until every env has logged `episodes_per_env` episodes.  An env that is done early goes on
    with further episodes meanwhile (with a start pool: from further starts); only each env's first `episodes_per_env` count.
    The envs must stand at the start of an episode: call it behind sim.reset / sim.set_start_pool, whose observation `obs0` is
    (default: sim.obs).  classes: the orientation class of the starts for the heatmap coordinates - scenarios.draw_start_pool's
    [K, N] array for a pooled context, else one class per env or one string (metrics.EpisodeLedger.coords).
    Sets an episode log of its own on `sim` and clears it afterwards: a log the caller had set is gone.
    Returns eval_policy's dict - avg_reward, avg_rewards, all_ep_reward_values, num_success, success_coords, fail_coords, `success`
    and `steps` ([N] tensors; [N, episodes_per_env] for more than one episode) - plus `per_object` (attempts / successes / mean steps
    per object of the context), `start_index` (the pool entry of every counted episode, -1 without a pool) and `env_steps`.  An
    episode's reward is exactly 50 x lifted here (the finger and grasp rewards of this environment are identically 0), and an
    episode that lifts ends with that step - so success = the record's lifted bit."""
    from .metrics import EpisodeLedger
    from .pipeline import rollout_args
    from .rollout import RolloutEngine
    from .sim import EPISODE_LOG_CAPACITY_MAX
    n, dev, E = sim.n_envs, sim.device, int(episodes_per_env)
    horizon = int(sim.cfg.horizon)
    if not (sim.cfg.auto_reset and sim.obs_env_major) or horizon <= 0 or E < 1:
        raise ValueError("eval_policy_free_running needs an auto-reset context with env-major observations and a time limit, and episodes_per_env >= 1")
    eng = RolloutEngine(sim, policy, None, expl_noise=0.0, max_action=float(getattr(policy.actor, "max_action", 0.8)))
    if eng._fused_actor_layers() is None:
        raise ValueError("eval_policy_free_running needs the in-kernel actor: a 3-layer MLP at a width ks_rollout supports (256-256, 400-300, 128-128, 64-64)")
    eng.start(sim.obs if obs0 is None else obs0)
    flat = policy.acting_flat()              # (obs_norm: the copy with the normalisation folded into the first layer)
    pub = torch.zeros(3, (flat.numel() + 3) // 4 * 4, device=dev)
    pub[0, :flat.numel()].copy_(flat)
    pub_ver = torch.zeros(1, dtype=torch.long, device=dev)
    steps_total, counters = torch.zeros(n, dtype=torch.long, device=dev), torch.zeros(8 + 4 * 512 + 8, dtype=torch.long, device=dev)
    args = rollout_args(sim, policy, eng, pub, pub_ver, steps_total, counters, replay=None, sigma=0.0)
    chunk = horizon if chunk is None else int(chunk)
    # at most one record per env and env-step: a launch's records always fit, whatever the envs do
    sim.set_episode_log(min(max(n * chunk, n), EPISODE_LOG_CAPACITY_MAX))
    n_obj = len(getattr(sim, "models", [None]))
    ledger = EpisodeLedger(n, n_obj, None)
    success = torch.zeros(n, E, dtype=torch.bool, device=dev)
    steps = torch.zeros(n, E, dtype=torch.long, device=dev)
    start = torch.full((n, E), -1, dtype=torch.long, device=dev)
    have = torch.zeros(n, dtype=torch.long, device=dev)
    launches, limit = 0, (max_launches if max_launches is not None else (E * horizon + chunk - 1) // chunk + 1)
    try:
        while int(have.min()) < E:
            if launches >= limit:
                raise RuntimeError(f"eval_policy_free_running: {launches} launches of {chunk} env-steps and an env has logged {int(have.min())} of {E} episodes")
            sim.rollout(chunk, args)
            launches += 1
            rec = sim.episode_log()
            if rec["lost"]:
                raise RuntimeError(f"eval_policy_free_running: the episode log lost {rec['lost']} records")
            m = rec["episode"] < E
            counted = {k: (v[m] if torch.is_tensor(v) else v) for k, v in rec.items()}
            e, j = counted["env"].long(), counted["episode"].long()
            success[e, j] = (counted["done"] & 1) != 0
            steps[e, j] = counted["steps"].long()
            start[e, j] = counted["start_index"].long()
            have.index_add_(0, e, torch.ones_like(e))
            ledger.add(counted)
    finally:
        sim.set_episode_log(0)
    ok_coords, fail_coords = ledger.coords(classes)
    total = success.float() * 50.0
    names = ("total_reward", "finger_reward", "grasp_reward", "lift_reward")
    per = {"total_reward": total, "finger_reward": torch.zeros_like(total), "grasp_reward": torch.zeros_like(total), "lift_reward": total}
    sq = (lambda t: t[:, 0]) if E == 1 else (lambda t: t)
    return {"avg_reward": float(total.mean()), "avg_rewards": {k: float(per[k].mean()) for k in names},
            "all_ep_reward_values": {k: per[k].reshape(-1).tolist() for k in names}, "num_success": int(success.sum()),
            "success_coords": ok_coords, "fail_coords": fail_coords, "success": sq(success), "steps": sq(steps), "start_index": sq(start),
            "per_object": ledger.per_object(object_names), "env_steps": launches * chunk * n}
