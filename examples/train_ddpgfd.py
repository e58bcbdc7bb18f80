#!/usr/bin/env python3
"""End-to-end DDPGfD training on the batched simulator (the counterpart of
`python main_DDPGfD.py --mode train ...` in the reference, gym-kinova-gripper/main_DDPGfD.py:333-537):

  1. expert data: a scripted demonstrator (expert_data.py:596-671, loop :746-804) on start positions sampled from the
     no_noise start table fills the expert replay;
  2. training: N envs roll out clip(pi(s) + N(0, 0.08), 0, 0.8) with the scripted lift after check_grasp,
     agent transitions go to the device replay, and every env-step one DDPGfD update mixes 70 % agent /
     30 % expert episodes (DDPGfD.py:232-254);
  3. periodic evaluation without exploration noise (eval_policy, main_DDPGfD.py:130-272): lift success rate on 1024 fresh start positions.
     (The lift rate of the TRAINING rollouts is depressed by the exploration noise on the wrist channel: clip(pi + N(0, 0.08), 0, 0.8) lifts the
     hand by ~5 mm per env-step on average while the fingers close - as in the reference, main_DDPGfD.py:443-446.)

    python examples/train_ddpgfd.py --envs 1024 --steps 600 --hidden 256 256 (or 400 300: the reference's widths, free-running too) [--free-running] [--expert-prob 0] [--starts-per-env 64]
                                    [--success-map DIR] [--demonstrations free-running] [--randomize-params] [--prioritized]
                                    [--q-bounds 0 50] [--huber-delta 10] [--max-grad-norm 10] [--bc-weight 1 [--q-filter]]
                                    [--obs-norm [--obs-norm-eps 1e-2] [--obs-norm-freeze-after N]]

--success-map DIR (with --free-running): the stepping kernel logs every finished training episode (ks_set_episode_log); at every report
the script folds the log (metrics.EpisodeLedger) and writes DIR/per_shape_success.jsonl and the success / fail start coordinates of the
report's episodes as DIR/train/<orientation>/*.npy (metrics.save_heatmap_coords), and the periodic noise-free evaluation runs on the
free-running path as well (evaluate.eval_policy_free_running; its coordinates: DIR/eval).

Measured curves: profiles/r04_training_curves.txt.  One update per env-step of 4096 envs (BASELINE config 3's workload) is 1e4 times fewer
updates per stored transition than the reference's 100 updates per episode of one env (main_DDPGfD.py:474-476); with the reference's target
rate (tau 0.0005 every 10th update, DDPGfD.py:64-66,360-366) the target networks move 26 % of the way in 6000 updates and nothing
propagates.  The defaults below therefore let the targets follow EVERY update at tau = 0.001 (--tau 0.0005 --target-every 10 are the
reference's values): with the 30 % expert mix the noise-free evaluation reaches 0.92 lift success after 600 updates and stays >= 0.80 for
9000 consecutive updates (the demonstrator itself: 0.64); plain DDPG needs 7000 updates to leave the 0.65 plateau of a constant closing action.
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from kinovagrasping_amd import scenarios                       # noqa: E402
from kinovagrasping_amd.ddpgfd import DDPGfD, TD3fD            # noqa: E402
from kinovagrasping_amd.demonstrators import run_controller_episodes, run_controller_free_running  # noqa: E402
from kinovagrasping_amd.evaluate import eval_policy, eval_policy_free_running  # noqa: E402
from kinovagrasping_amd.metrics import EpisodeLedger, param_success_table, save_heatmap_coords      # noqa: E402
from kinovagrasping_amd.replay import DeviceEpisodeReplay      # noqa: E402
from kinovagrasping_amd.rollout import RolloutEngine           # noqa: E402
from kinovagrasping_amd.sim import EPISODE_LOG_CAPACITY_MAX, KinovaSim      # noqa: E402


def start_states(n, shape, rng):
    tab = scenarios.start_coord_table(shape)
    q = np.zeros((16, n)); q[12] = 1.0
    q[9:12] = tab[rng.randint(0, len(tab), n)].T
    return q, np.repeat(scenarios.hand_quat_for("normal")[:, None], n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--shape", default="CubeS")
    ap.add_argument("--hidden", type=int, nargs=2, default=[256, 256])
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--expert-episodes", type=int, default=2048)
    ap.add_argument("--controller", default="combined", choices=["naive", "position-dependent", "combined"])
    ap.add_argument("--demonstrations", default="loop", choices=["loop", "free-running"], help="how the expert replay is filled: the Python loop around "
                    "ks_step, one episode per env and pass (loop), or the controller inside the persistent rollout kernel on an auto-reset context "
                    "whose envs draw their starts from a pool (free-running: ks_set_rollout_controller; --starts-per-env sets the pool's size, default 8)")
    ap.add_argument("--expert-prob", type=float, default=0.3, help="share of expert episodes in a batch (DDPGfD.py:232-254); 0: plain DDPG, no demonstrations")
    ap.add_argument("--eval-every", type=int, default=600, help="env-steps between evaluations without exploration noise (0: none)")
    ap.add_argument("--free-running", action="store_true", help="the persistent rollout kernel (ks_rollout) instead of one launch per env-step")
    ap.add_argument("--starts-per-env", type=int, default=0, help="K > 0: every training env holds a pool of K start positions and each of its episodes starts from one "
                    "drawn inside the stepping kernel (ks_set_start_pool); 0: an env replays the one start it was reset to")
    ap.add_argument("--randomize-params", action="store_true", help="every training episode draws its object mass (0.05-0.15 kg) and object-hand friction "
                    "(0.5-1.0) inside the stepping kernel (ks_set_param_ranges: BASELINE config 5's ranges, per episode); with --success-map the "
                    "success table per (mass, friction) bin is printed at every report")
    ap.add_argument("--success-map", default=None, help="with --free-running: keep the in-kernel episode log and write per-shape success and the success / fail "
                    "heatmap coordinates of the training episodes into this directory at every report; the evaluation runs through ks_rollout too")
    ap.add_argument("--batch-episodes", type=int, default=64, help="episodes per update (x 25 five-step windows each); the reference: 64")
    ap.add_argument("--updates-per-step", type=int, default=1, help="learner updates per env-step of the whole batch of envs")
    ap.add_argument("--prioritized", action="store_true", help="prioritized episode replay: episodes are drawn in proportion to (last TD error + eps)^alpha, "
                    "demonstrations with a priority bonus, importance weights (p_min / p)^beta in the losses (DeviceEpisodeReplay.sample_prioritized)")
    ap.add_argument("--per-alpha", type=float, default=0.3, help="with --prioritized: the priorities' exponent")
    ap.add_argument("--per-beta0", type=float, default=0.4, help="with --prioritized: the importance weights' exponent at the start; annealed linearly to 1 over --steps")
    ap.add_argument("--per-eps-expert", type=float, default=1.0, help="with --prioritized: the constant added to a demonstration's TD error (the agent's: 1e-3)")
    ap.add_argument("--actor-lr", type=float, default=1e-4, help="reference: 1e-4 (DDPGfD.py:57)")
    ap.add_argument("--critic-lr", type=float, default=1e-3, help="reference: Adam's default 1e-3 (DDPGfD.py:61)")
    ap.add_argument("--tau", type=float, default=0.001, help="soft target update rate (reference: 0.0005, main_DDPGfD.py:894 - for 100 updates per episode of one env)")
    ap.add_argument("--target-every", type=int, default=1, help="target networks follow every this many updates (reference: 10, DDPGfD.py:64-66,360-366)")
    ap.add_argument("--td3", action="store_true", help="TD3fD: twin critics with the minimum in the targets, noise-smoothed target actions, a delayed actor "
                    "(ddpgfd.TD3fD) - against the single critic's over-estimated Q; profiles/td3fd.txt has what it does on the reference's schedule")
    ap.add_argument("--policy-noise", type=float, default=None, help="with --td3: std of the target smoothing noise (default 0.1 x max_action = 0.08)")
    ap.add_argument("--noise-clip", type=float, default=None, help="with --td3: clip of the target smoothing noise (default 0.25 x max_action = 0.2)")
    ap.add_argument("--policy-freq", type=int, default=2, help="with --td3: the actor steps on every this many updates")
    ap.add_argument("--log-q", action="store_true", help="print the mean Q(s, pi(s)) of the last update's batch beside the critic loss (the critic's own estimate: "
                    "the best possible return is 50); with --max-grad-norm also the critic's gradient norm and clip coefficient of that update")
    ap.add_argument("--q-bounds", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="clamp the bootstrapped target-critic value to [LO, HI] before it "
                    "enters the 1-step and the n-step target (the attainable return here: 0 50); default: no clamp")
    ap.add_argument("--huber-delta", type=float, default=None, metavar="D", help="Huber-shaped TD loss: e^2 up to |e| = D, D (2 |e| - D) beyond, so a row's pull on "
                    "the critic stops growing at 2 D; default: the plain square")
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="G", help="clip each network's gradient to the global L2 norm G right before its Adam step "
                    "(torch.nn.utils.clip_grad_norm_; kr_grad_sqnorm + kr_adam_step_clipped); default: no clip")
    ap.add_argument("--bc-weight", type=float, default=0.0, metavar="X", help="weight of the behaviour-cloning term of the actor loss on the expert episodes of every "
                    "batch (Nair et al. 2018; kr_bc_actor_grad): pi(s) is pulled towards the demonstrated action; needs --expert-prob > 0; default 0: no such term. "
                    "With --log-q the term and the filter's pass share are printed too")
    ap.add_argument("--q-filter", action="store_true", help="with --bc-weight: only on the demonstration states where the critic rates the demonstrated action above "
                    "the actor's own, Q(s, a) > Q(s, pi(s))")
    ap.add_argument("--obs-norm", action="store_true", help="running observation normalisation: a running mean and standard deviation per observation component "
                    "from the batches' window-first states, every network on the normalised state, the rollout on the actor with the map folded into its first "
                    "layer (kr_obs_stats_update / kr_obs_normalize / kr_fold_obs_norm); default: raw observations. With --log-q the smallest and largest "
                    "per-column standard deviation are printed too")
    ap.add_argument("--obs-norm-eps", type=float, default=None, metavar="E", help="with --obs-norm: the floor of the standard deviation (default 1e-2)")
    ap.add_argument("--obs-norm-freeze-after", type=int, default=None, metavar="N", help="with --obs-norm: the statistics stop changing after N updates")
    ap.add_argument("--expl-noise", type=float, default=0.1, help="exploration noise, std = 0.8 x this (main_DDPGfD.py:443-446: 0.1)")
    ap.add_argument("--dump-replay", default=None, help="write the replay (last 1500 agent + first 400 expert episodes) and the four networks as one .npz "
                    "(tools/r06/reference_learner_on_replay.py runs the REFERENCE's train_batch on it)")
    ap.add_argument("--save", default=None, help="write the trained policy as the reference's 4-file checkpoint with this prefix")
    args = ap.parse_args()
    if args.success_map and not args.free_running:
        ap.error("--success-map needs --free-running")
    if args.bc_weight > 0 and not args.expert_prob > 0:
        ap.error("--bc-weight needs demonstrations in the batches: --expert-prob > 0")
    if args.q_filter and not args.bc_weight > 0:
        ap.error("--q-filter needs --bc-weight > 0")
    if (args.obs_norm_eps is not None or args.obs_norm_freeze_after is not None) and not args.obs_norm:
        ap.error("--obs-norm-eps / --obs-norm-freeze-after need --obs-norm")
    bounded = dict(q_bounds=None if args.q_bounds is None else tuple(args.q_bounds), huber_delta=args.huber_delta, max_grad_norm=args.max_grad_norm,
                   bc_weight=args.bc_weight, q_filter=args.q_filter)
    if args.obs_norm:
        bounded.update(obs_norm=True, obs_norm_freeze_after=args.obs_norm_freeze_after, **({} if args.obs_norm_eps is None else dict(obs_norm_eps=args.obs_norm_eps)))
    torch.manual_seed(args.seed)
    rng = np.random.RandomState(args.seed)
    dev = torch.device("cuda", 0)
    n = args.envs

    # 1. expert replay: the combined controller with the demonstration loop of expert_data.py:746-804
    expert = DeviceEpisodeReplay(n, capacity=args.expert_episodes, device=dev) if args.expert_prob > 0 else None
    free_demos = args.demonstrations == "free-running"
    sim = KinovaSim(n, args.shape, auto_reset=free_demos, horizon=30)
    succ = []
    if expert is not None and free_demos:
        kd = args.starts_per_env if args.starts_per_env > 0 else 8
        qd, hqd, _ = scenarios.draw_start_pool([args.shape] * n, "normal", kd, rng)
        sim.set_start_pool(torch.as_tensor(qd), torch.as_tensor(hqd), seed=args.seed)
        out = run_controller_free_running(sim, expert, episodes_per_env=-(-args.expert_episodes // n), mode=args.controller, object_names=[args.shape])
        succ.append(out["success"].float().mean().item())
        print(f"demonstrations on the free-running path: {out['env_steps']} env-steps, {out['episodes_dropped']} episodes dropped")
    while expert is not None and not free_demos and expert.count < args.expert_episodes:
        q0, hq = start_states(n, args.shape, rng)
        out = run_controller_episodes(sim, sim.reset(torch.as_tensor(q0), torch.as_tensor(hq)), expert, mode=args.controller)
        succ.append(out["success"].float().mean().item())
    if expert is not None:
        print(f"expert replay: {expert.count} episodes, {args.controller}-controller lift success {np.mean(succ):.2f}")
    print(f"targets follow every {args.target_every} update(s) at tau {args.tau} (reference: every 10th at 0.0005), batch {args.batch_episodes} episodes, "
          f"{args.updates_per_step} update(s) per env-step, actor / critic lr {args.actor_lr} / {args.critic_lr}, expert share {args.expert_prob}")
    sim.close()

    # 2. training on the product path: HIP-graph trainer, native MFMA learner, every batch 44 agent + 20 expert episodes sampled by
    #    one launch inside the captured update (pipeline.GraphedTrainer; --free-running: the persistent rollout kernel, AsyncTrainer)
    from kinovagrasping_amd.pipeline import AsyncTrainer, GraphedTrainer
    sim = KinovaSim(n, args.shape, auto_reset=True, horizon=30)
    if args.starts_per_env > 0:
        qp, hqp, pool_classes = scenarios.draw_start_pool([args.shape] * n, "normal", args.starts_per_env, rng)
        print(f"start pool: {args.starts_per_env} starts per env, {qp.shape[0] * n * 102 * 4 / 1e6:.0f} MB on the device")
    else:
        q0, hq = start_states(n, args.shape, rng)
    if args.td3:
        policy = TD3fD(82, 4, 0.8, 5, tau=args.tau, batch_size=args.batch_episodes, hidden=tuple(args.hidden), device=dev, policy_noise=args.policy_noise,
                       noise_clip=args.noise_clip, policy_freq=args.policy_freq, **bounded)
        policy.critic2_optimizer.param_groups[0]["lr"] = args.critic_lr
        print(f"TD3fD: target smoothing noise {policy.policy_noise:g} clipped at {policy.noise_clip:g}, actor steps every {policy.policy_freq} update(s)")
    else:
        policy = DDPGfD(82, 4, 0.8, 5, tau=args.tau, batch_size=args.batch_episodes, hidden=tuple(args.hidden), device=dev, **bounded)
    if policy.obs_norm is not None:
        print(f"running observation normalisation: eps {policy.obs_norm.eps:g}, freeze after {policy.obs_norm.freeze_after}")
    if policy.bc_weight > 0:
        print(f"behaviour cloning on the expert episodes of every batch: weight {policy.bc_weight:g}, Q-filter {'on' if policy.q_filter else 'off'}")
    if any(bounded[k] is not None for k in ("q_bounds", "huber_delta", "max_grad_norm")):
        print(f"bounded critic update: q_bounds {policy.q_bounds}, huber_delta {policy.huber_delta}, max_grad_norm {policy.max_grad_norm}")
    policy.network_repl_freq = args.target_every
    policy.actor_optimizer.param_groups[0]["lr"] = args.actor_lr
    policy.critic_optimizer.param_groups[0]["lr"] = args.critic_lr
    agent = DeviceEpisodeReplay(n, capacity=max(4 * n, 4096), device=dev)
    eng = RolloutEngine(sim, policy, agent, expl_noise=args.expl_noise)
    if args.starts_per_env > 0:
        eng.start(sim.set_start_pool(torch.as_tensor(qp), torch.as_tensor(hqp), seed=args.seed))
    else:
        eng.start(sim.reset(torch.as_tensor(q0), torch.as_tensor(hq)))
    param_ranges = None
    if args.randomize_params:               # (behind the pool: an episode boundary; the ranges reset nothing)
        param_ranges = sim.set_param_ranges(seed=args.seed, **scenarios.config5_param_ranges(n)).cpu().numpy()
        print("per-episode parameters: object mass 0.05-0.15 kg, object-hand friction 0.5-1.0, drawn at every auto-reset")
    Trainer = AsyncTrainer if args.free_running else GraphedTrainer
    tr = Trainer(sim, policy, agent, eng, batch_episodes=args.batch_episodes, expert_replay=expert, expert_prob=args.expert_prob if expert is not None else 0.3,
                 updates_per_step=args.updates_per_step, prioritized=args.prioritized, per_alpha=args.per_alpha, per_beta=args.per_beta0,
                 per_eps_expert=args.per_eps_expert)
    tr.native.track_actor_loss = args.log_q          # (before the capture: the evaluation is part of the captured update)
    tr.capture()
    if args.free_running:
        tr.run(36, learn=False)
        tr.flush()
    lifted = episodes = 0
    ledger = None
    if args.success_map:
        import json
        map_dir = Path(args.success_map)
        map_dir.mkdir(parents=True, exist_ok=True)
        ledger = EpisodeLedger(n, 1, args.starts_per_env or None)
        sim.set_episode_log(min(n * 60, EPISODE_LOG_CAPACITY_MAX))           # a report's 60 env-steps: at most one record per env and env-step
        if param_ranges is not None:
            # the log starts here, the draws started behind the pool: the record of ordinal k of an env ran the env's draw number first_draw + k
            first_draw = sim.env_params()[2].cpu().numpy()
            mass_edges, mu_edges = np.linspace(0.05, 0.15, 5), np.linspace(0.5, 1.0, 5)
            p_attempts, p_successes = np.zeros((4, 4), dtype=np.int64), np.zeros((4, 4), dtype=np.int64)
    sim_eval = KinovaSim(1024, args.shape, auto_reset=bool(args.success_map), horizon=30)
    qe, hqe = start_states(1024, args.shape, np.random.RandomState(args.seed + 1))
    qe, hqe = torch.as_tensor(qe), torch.as_tensor(hqe)
    t0 = time.perf_counter()
    t_eval = 0.0
    for it in range(0, args.steps, 60):
        if args.prioritized:                # beta from --per-beta0 to 1 over the run (a fill of the device scalar the captured sampler reads)
            tr.set_per_beta(args.per_beta0 + (1.0 - args.per_beta0) * min(1.0, it / max(args.steps - 60, 1)))
        if args.free_running:
            tr.run(60)                      # one persistent launch of 60 env-steps (+ 60 updates beside it): long launches keep the launch tail small
            tr.flush()
            c = tr.counts()
            d_ep, d_lift = c["episodes_finished"] - episodes, c["lifted"] - lifted
            episodes, lifted = c["episodes_finished"], c["lifted"]
            if ledger is not None:
                records = sim.episode_log()
                ledger.add(records)
                if param_ranges is not None:
                    r_env, r_ep = records["env"].cpu().numpy(), records["episode"].cpu().numpy()
                    r_mass, r_mu = scenarios.param_draw_reference(args.seed, r_env, first_draw[r_env] + r_ep, param_ranges, np.float32)
                    a_, s_ = param_success_table(records, r_mass, r_mu, mass_edges, mu_edges)
                    p_attempts += a_
                    p_successes += s_
                    print("lift success per (mass bin, mu bin), rows mass 0.05 .. 0.15 kg, columns mu 0.5 .. 1.0 (successes / attempts):")
                    for i in range(4):
                        print("   " + "  ".join(f"{p_successes[i, j]:6d}/{p_attempts[i, j]:<6d}" for j in range(4)))
                with open(map_dir / "per_shape_success.jsonl", "a") as f:
                    f.write(json.dumps({"step": it + 60, "episodes": ledger.episodes, "lost": ledger.lost, "per_shape": ledger.per_object([args.shape])}) + "\n")
                save_heatmap_coords(*ledger.coords(pool_classes if args.starts_per_env > 0 else "normal", clear=True), it + 60, map_dir / "train")
        else:
            d_ep = d_lift = 0
            for _ in range(60):
                reward, done = tr.step()
                d_lift += int(((reward > 0) & done).sum())
                d_ep += int(done.sum())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0 - t_eval
        ls = tr.native.losses.tolist()
        ev = ""
        clip = bc = ""
        mean_q = -tr.native.actor_loss.item() if args.log_q else 0.0
        if args.log_q and args.bc_weight > 0:               # (the tracked actor loss holds the term as well)
            bc_loss = tr.native.bc_loss.item()
            mean_q += bc_loss
            bc = f"  BC loss {bc_loss:8.5f} pass {tr.native.bc_pass.item():5.3f}"
        if args.log_q and args.max_grad_norm is not None:
            norm_c, coef_c = tr.native.clip[1].tolist()
            clip = f"  critic grad norm {norm_c:9.3f} coef {coef_c:6.4f}"
        if args.log_q and policy.obs_norm is not None:
            sd = policy.obs_norm.std()
            clip += f"  obs std {sd.min().item():.3g} .. {sd.max().item():.3g} ({int(policy.obs_norm.count.item())} rows)"
        if args.eval_every and (it + 60) % args.eval_every == 0:
            te = time.perf_counter()
            tr.flush(finish_update=True)                     # the actor the next rollout step would use
            torch.cuda.synchronize()
            if ledger is not None:
                res = eval_policy_free_running(sim_eval, policy, obs0=sim_eval.reset(qe, hqe), classes="normal", object_names=[args.shape])
                save_heatmap_coords(res["success_coords"], res["fail_coords"], it + 60, map_dir / "eval")
            else:
                res = eval_policy(sim_eval, policy, sim_eval.reset(qe, hqe))
            ev = f"  eval (no noise, 1024 starts): lift success {res['num_success'] / 1024:.3f}"
            t_eval += time.perf_counter() - te
        print(f"step {it + 60:5d}  episodes {d_ep:7d}  training lift rate {d_lift / max(1, d_ep):.3f}  critic loss {ls[0]:9.3f}{f' / {ls[3]:9.3f}' if args.td3 else ''}{f'  mean Q {mean_q:8.3f}' if args.log_q else ''}{bc}{clip}  {n * (it + 60) / dt:9.0f} env-steps/s{ev}")
    if args.log_q and policy.obs_norm is not None:
        print("obs std per column: " + " ".join(f"{v:.3g}" for v in policy.obs_norm.std().tolist()))
    if args.free_running:
        c = tr.counts()
        print(f"free-running rollout: {c['episodes_finished']} episodes finished, {c['episodes_dropped']} dropped, {c['pacing_timeouts']} pacing time-outs, {tr.updates} updates")
    if args.dump_replay:
        tr.flush(finish_update=True)
        torch.cuda.synchronize()
        out = {}
        for name, rep, keep in (("agent", agent, slice(-1500, None)), ("expert", expert, slice(0, 400))):
            eps = rep.host_episodes()[keep] if rep is not None else []
            out[f"{name}_lens"] = np.array([len(e["reward"]) for e in eps])
            for f in ("state", "action", "next_state", "reward"):
                out[f"{name}_{f}"] = np.concatenate([np.asarray(e[f], dtype=np.float32) for e in eps]) if eps else np.zeros(0, np.float32)
        for name, net in (("actor", policy.actor), ("critic", policy.critic), ("actor_target", policy.actor_target), ("critic_target", policy.critic_target)):
            for k, v in net.state_dict().items():
                out[f"{name}.{k}"] = v.detach().cpu().numpy()
        out["updates"] = np.array(tr.updates)
        np.savez_compressed(args.dump_replay, **out)
        print("dumped", args.dump_replay, {k: v.shape for k, v in out.items() if k.endswith("_lens")}, "after", tr.updates, "updates")
    if args.save:
        tr.flush(finish_update=True)
        policy.save(args.save)
        print("saved", args.save + ("_{actor,critic,critic2,actor_optimizer,critic_optimizer,critic2_optimizer}" if args.td3 else "_{actor,critic,actor_optimizer,critic_optimizer}"))
    sim.close()
    sim_eval.close()


if __name__ == "__main__":
    main()
