"""Staged experiments of the reference's `experiment` mode (gym-kinova-gripper/main_DDPGfD.py):
which policy a stage starts from, which objects / orientations it trains on, where its files go - and a batched
driver that runs one stage on the GPU simulator.

    stage 0  pretrain_policy                (expert policy, small cube)
    stage 1  1 sizes | 2 shapes | 3 orientations                        each starts from stage 0
    stage 2  4 sizes_shapes_orientations <- 1 | 5 shapes_sizes_orientations <- 2 | 6 orientations_sizes_shapes <- 3

`experiment_info` / `experiment_input` / `experiment_dirs` restate get_experiment_info (main_DDPGfD.py:624-671),
get_exp_input (710-738) and get_experiment_file_structure (674-707); tests/golden/curriculum.json holds the
reference's own answers (tools/gen_golden_curriculum.py).
"""
from __future__ import annotations

import datetime
from pathlib import Path

import numpy as np

from . import scenarios

STAGE0 = "pretrain_policy"
STAGE1 = {"1": ["0", "sizes"], "2": ["0", "shapes"], "3": ["0", "orientations"]}
STAGE2 = {"4": ["1", "sizes_shapes_orientations"], "5": ["2", "shapes_sizes_orientations"], "6": ["3", "orientations_sizes_shapes"]}
# shape / size lists of the experiment mode (main_DDPGfD.py:1270-1282)
TRAIN_SHAPES = ["Cube", "Cylinder", "Cube45", "Vase2", "Bottle", "Bowl", "TBottle"]
TRAIN_SIZES = ["S", "B"]
TEST_SHAPES = ["Vase1", "RBowl"]
TEST_SIZES = ["M"]


def experiment_info(exp_num):
    """(prev_exp_stage, prev_exp_num, prev_exp_name, exp_stage, exp_name) of experiment 1..6.
    The reference's table of third-stage experiments is commented out, so every other number - including the
    `kitchen_sink` experiment 16 its last branch was written for - ends in a NameError there (main_DDPGfD.py:657);
    here they raise ValueError."""
    key = str(exp_num)
    if key in STAGE1:
        return "0", "0", STAGE0, "1", STAGE1[key][1]
    if key in STAGE2:
        prev = STAGE2[key][0]
        return "1", prev, STAGE1[prev][1], "2", STAGE2[key][1]
    raise ValueError(f"invalid experiment number {exp_num!r} (1..6)")


def experiment_input(exp_name: str, shapes, sizes):
    """(requested shape keys, requested orientation) of an experiment name: the name's parts say what varies -
    `shapes` (else only Cube), `sizes` (else only S), `orientations` (else only normal); kitchen_sink = all three."""
    types = ["shapes", "sizes", "orientations"] if exp_name == "kitchen_sink" else exp_name.split("_")
    if "shapes" in types and "sizes" in types:
        req = [shape + size for size in sizes for shape in shapes]
    elif "shapes" in types:
        req = [shape + "S" for shape in shapes]
    elif "sizes" in types:
        req = ["Cube" + size for size in sizes]
    else:
        req = ["CubeS"]
    return req, ("random" if "orientations" in types else "normal")


def experiment_dirs(prev_exp_stage, prev_exp_name, exp_stage, exp_name, with_grasp: bool = False, root=".", create: bool = False):
    """Directory layout of a stage (main_DDPGfD.py:674-707): rl_experiments/<no_grasp|with_grasp>/stage<k>/<name>/
    {policy, replay_buffer, output}; the expert data under expert_replay_data/<...>/combined/<shape>/<orientation>/."""
    grasp = "with_grasp" if with_grasp else "no_grasp"
    root = Path(root)
    exp_dir = root / "rl_experiments" / grasp / f"stage{exp_stage}" / exp_name
    prev_dir = root / "rl_experiments" / grasp / f"stage{prev_exp_stage}" / prev_exp_name
    d = {"exp_dir": exp_dir, "policy_dir": exp_dir / "policy", "replay_dir": exp_dir / "replay_buffer", "output_dir": exp_dir / "output",
         "prev_exp_dir": prev_dir, "prev_policy_dir": prev_dir / "policy", "prev_replay_dir": prev_dir / "replay_buffer",
         "expert_replay_dir": root / "expert_replay_data" / grasp / "combined"}
    if create:
        for k in ("exp_dir", "policy_dir", "replay_dir", "output_dir"):
            d[k].mkdir(parents=True, exist_ok=True)
    return d


def experiment_plan(exp_num, exp_mode: str = "train", with_grasp: bool = False, root="."):
    """Everything main_DDPGfD.py's experiment mode derives from the experiment number before it starts training
    (main_DDPGfD.py:1265-1300): stage info, shape keys, orientation classes, directories."""
    shapes, sizes = (TEST_SHAPES, TEST_SIZES) if exp_mode == "test" else (TRAIN_SHAPES, TRAIN_SIZES)
    prev_stage, prev_num, prev_name, stage, name = experiment_info(exp_num)
    req, orientation = experiment_input(name, shapes, sizes)
    return {"exp_num": int(exp_num), "exp_stage": stage, "exp_name": name, "prev_exp_stage": prev_stage, "prev_exp_num": prev_num,
            "prev_exp_name": prev_name, "requested_shapes": req, "requested_orientation": orientation,
            "requested_orientation_list": ["normal", "rotated", "top"] if orientation == "random" else ["normal"],
            "dirs": experiment_dirs(prev_stage, prev_name, stage, name, with_grasp, root)}


def policy_basename(policy_dir) -> str:
    """name of the checkpoint saved in a policy directory (rl_experiment: glob '*_actor_optimizer', main_DDPGfD.py:781-785)"""
    hits = sorted(Path(policy_dir).glob("*_actor_optimizer"))
    if not hits:
        raise FileNotFoundError(f"no '*_actor_optimizer' checkpoint file in {policy_dir}")
    return hits[0].name[: -len("_actor_optimizer")]


def run_stage(plan, policy, n_envs: int = 1024, rounds: int = 10, updates_per_round: int = 100, expert_prob: float = 0.3, seed: int = 2,
              device: int = 0, load_previous: bool = True, save: bool = True, eval_envs: int | None = None, starts_per_env: int = 0,
              param_ranges=None, free_running: bool = False, balanced: bool | None = None, budget_ms: float | None = None, prioritized: bool = False,
              per_alpha: float = 0.3, per_beta: float = 1.0, per_eps: float = 1e-3, per_eps_expert: float = 1.0):
    """One stage of the curriculum on the GPU simulator (the batched counterpart of rl_experiment + train_policy,
    main_DDPGfD.py:600-621, 776-800): start from the previous stage's policy and agent replay, mix in the expert
    replay of the stage's shapes at `expert_prob` (DDPGfD.py:232-254), train, evaluate, save policy + replay + info.

    The reference runs max_episode episodes one at a time, objects in Latin-square order, and 100 updates at the end
    of each (main_DDPGfD.py:466-486).  Here a ROUND is one episode of every env (the envs are split over the stage's
    shapes, orientation classes drawn per env by the reference's rule) followed by `updates_per_round` updates.
    Every shape key of the reference's stages has a compiled asset since round 4 - the multi-geom Bottle / Bowl / TBottle / RBowl
    objects included (a stage that holds one runs on libkinova_sim_mg.so, sim.KinovaSim picks it) -; a key without one would be
    listed under `skipped_shapes`.  Where the reference has no start-coordinate file for a (shape, orientation) - Normal/BowlS - the
    start is drawn by the reference's empty-file rule (scenarios.fallback_start).
    starts_per_env = K > 0: the stage runs an AUTO-RESET simulator whose envs each hold a pool of K starts drawn by the same rules
    (scenarios.draw_start_pool) and take one of them at every episode inside the stepping kernel (ks_set_start_pool): no host reset
    between rounds - a round is then 30 env-steps of every env, whose episodes end and restart on their own -, and `distinct_starts`
    in the result counts the (env, start) pairs that were run.  The stage then also keeps the in-kernel episode log (ks_set_episode_log)
    over the rounds and returns its fold: `episodes` (episodes that ended in the rounds) and `per_shape_success` ({shape: attempts,
    successes, mean_steps}, by the object the record names; with several shapes every env is given its shape's object before the pool
    is set).  0: the host reset per round, as before (same draws from the same rng).
    param_ranges = {"mass": (lo, hi), "mu": (lo, hi)} (scenarios.config5_param_ranges; honoured only with starts_per_env > 0, ValueError
    otherwise): every episode also draws its object's mass and object-hand friction inside the stepping kernel (ks_set_param_ranges, set
    behind the pool with the episode log, seed = `seed`) - the final evaluation's episodes included.  The result gains `param_success`:
    {"mass_edges", "mu_edges", "attempts", "successes"}, the rounds' episodes per (mass bin, mu bin) in four bins each over the ranges
    (metrics.param_success_table; every record's parameters from scenarios.param_draw_reference: the log's episode ordinal is the draw's
    episode number).
    free_running=True (needs starts_per_env > 0, ValueError otherwise): the stage trains through pipeline.AsyncTrainer - capture, then one
    run per round, then flush - instead of eng.step() plus serial updates: a round is ONE persistent launch of 30 env-steps (ks_rollout)
    with the learner's captured updates beside it on a second stream.  updates_per_round maps to the trainer's updates_per_step =
    max(1, round(updates_per_round / 30)): that many updates per env-step of the launch, so 100 becomes 3 per step = 90 per round, and
    anything below 45 one per step = 30 per round.  The batch is policy.batch_size episodes.  budget_ms: every round is one TIME-budgeted
    launch (AsyncTrainer.run(30, budget_ms=...): each wave steps its envs until the budget has passed, at most 30 env-steps) - cheap
    objects then finish several times the episodes of expensive ones; only on a context whose rollout plan is "waves" (KS_PLAN_WAVES:
    asked once the envs hold their shapes' objects, since the plan follows the objects' 16-env groups), ValueError before the trainer is
    built or a rollout launched otherwise.  balanced (None: true when the stage has more than one shape): the agent ring's
    episodes carry their shape as a class (DeviceEpisodeReplay.set_env_classes(sim.shape_of_env, shapes)), every shape's expert bundle
    is loaded with its shape's class, and each batch is drawn balanced over the shapes (sample_balanced) whatever the ring holds - the
    Latin square's equal shares, kept at the sampler instead of at collection.  The episode-log fold, per_shape_success, param_success,
    the final evaluation and the saved files are the lock-step stage's; `distinct_starts` is counted from the log's records (the starts
    of the episodes that ended in the rounds) and the starts running when the rounds end.  The result gains `env_steps` (the sum of the
    envs' step counters), `replay_class_counts` ({shape: episodes in the agent ring}) and `batch_class_slots` ({shape: slots of the
    last update's agent segment}, from the sampler's `picked`; empty without balanced).
    prioritized (free_running=True only, ValueError otherwise), per_*: AsyncTrainer's prioritized replay with the demonstration bonus - the
    trainer enables priorities on the agent ring and on the expert ring; with balanced each batch is drawn by sample_balanced_prioritized, the
    shapes' shares by the balanced rule and the episode within a shape by priority.  The result gains `priority_max`: {"agent": ...,
    "expert": ... (None without an expert mix)}, the largest priority an update has written to each ring, in units of 1 / 65536.
    A policy with obs_norm (ddpgfd: running observation normalisation) keeps it through the stage on either path: the previous stage's
    statistics are loaded with its weights (<prefix>_obs_norm), keep running over this stage's batches - whose object-size and rangefinder
    columns are distributed differently - and are saved with the policy; the result gains `obs_std` (min, max over the components).
    Returns a dict (num_success, num_total, paths, ...)."""
    import torch

    from .evaluate import eval_policy
    from .multi_shape import MultiShapeSim
    from .replay import DeviceEpisodeReplay
    from .rollout import RolloutEngine

    if param_ranges is not None and starts_per_env <= 0:
        raise ValueError("run_stage: param_ranges are drawn where an episode restarts inside the stepping kernel - they need starts_per_env > 0")
    if free_running and starts_per_env <= 0:
        raise ValueError("run_stage: free_running episodes restart inside the rollout kernel - they need starts_per_env > 0")
    if not free_running and (balanced or budget_ms is not None):
        raise ValueError("run_stage: balanced / budget_ms belong to free_running=True")
    if prioritized and not free_running:
        raise ValueError("run_stage: prioritized belongs to free_running=True")
    dirs = plan["dirs"]
    known = scenarios.SHAPES + scenarios.MEDIUM_SHAPES + scenarios.EXTRA_SHAPES + scenarios.MULTI_GEOM_SHAPES
    shapes = [s for s in plan["requested_shapes"] if s in known]
    skipped = [s for s in plan["requested_shapes"] if s not in known]
    if not shapes:
        raise ValueError(f"none of the stage's shapes {plan['requested_shapes']} has a compiled asset")
    rng = np.random.RandomState(seed)
    dev = torch.device("cuda", device)
    if load_previous:
        policy.load(str(dirs["prev_policy_dir"] / policy_basename(dirs["prev_policy_dir"])))
    sim = MultiShapeSim(n_envs, shapes, device=device, auto_reset=starts_per_env > 0, horizon=30)
    replay = DeviceEpisodeReplay(n_envs, capacity=max(4 * n_envs, 1024), horizon=30, device=dev)
    if free_running:
        balanced = len(shapes) > 1 if balanced is None else bool(balanced)
        replay.set_env_classes(sim.shape_of_env, shapes)          # (before the load: a previous stage's sidecar names its episodes' shapes)
    if load_previous and dirs["prev_replay_dir"].is_dir():
        replay.load(dirs["prev_replay_dir"])
    expert = None
    for s in shapes:                      # expert_replay_data/<grasp>/combined/<shape>/<orientation>/replay_buffer (main_DDPGfD.py:1183-1187)
        p = dirs["expert_replay_dir"] / s / plan["requested_orientation"] / "replay_buffer"
        if p.is_dir():
            if expert is None:
                expert = DeviceEpisodeReplay(n_envs, capacity=max(4 * n_envs, 1024), horizon=30, device=dev)
                if free_running:
                    expert.set_env_classes(None, shapes)
            if free_running:
                expert.load(p, class_id=shapes.index(s))
            else:
                expert.load(p)

    def reset_all(the_sim, count):
        """per env: orientation class by the reference's rule, start row from that class's table of the env's shape"""
        q, hq, classes = np.zeros((16, count)), np.zeros((4, count)), []
        q[12] = 1.0
        shape_ids = the_sim.shape_of_env.cpu().numpy()
        for e in range(count):
            shape = the_sim.shapes[shape_ids[e]]
            o = scenarios.select_orientation(shape, plan["requested_orientation"], rng) if plan["requested_orientation"] == "random" else "normal"
            if scenarios.has_start_table(shape, o):
                tab = scenarios.start_coord_table(shape, o)
                q[9:12, e] = tab[rng.randint(0, len(tab))]
            else:
                q[9:12, e] = scenarios.fallback_start(shape, o, rng)
            q[9:12, e] = scenarios.reset_body_position(shape, q[9:12, e])          # the reference reset's 5 cm correction (ENV:1379-1386)
            hq[:, e] = scenarios.hand_quat_for(o)
            classes.append(o)
        return the_sim.reset(torch.as_tensor(q), torch.as_tensor(hq)), classes

    eng = RolloutEngine(sim, policy, replay, expl_noise=0.1)
    # the updates run on the product learner (learner_native: fused MFMA forward / backward launches + kr_* glue), each batch =
    # int(batch_size * (1 - expert_prob)) agent + the rest expert episodes sampled by ONE launch (kr_sample_windows_mixed,
    # DDPGfD.train_batch's mix, DDPGfD.py:232-254); without expert data every episode comes from the agent ring
    from .learner_native import NativeDDPGfDUpdate
    native = None if free_running else NativeDDPGfDUpdate(policy)
    mix = expert is not None and expert.count >= 2
    losses = []
    seen = None
    if starts_per_env > 0:
        shape_ids = sim.shape_of_env.cpu().numpy()
        qp, hqp, _ = scenarios.draw_start_pool([sim.shapes[i] for i in shape_ids], plan["requested_orientation"], starts_per_env, rng)
        if len(shapes) > 1:
            # the context starts with every env on object 0: give each env its shape's object (ks_reset_objects, which would end a pool:
            # so before the pool is set), at a start of that shape
            sim.reset(torch.as_tensor(qp[0]), torch.as_tensor(hqp[0]), object_id=sim.shape_of_env)
        eng.start(sim.set_start_pool(torch.as_tensor(qp), torch.as_tensor(hqp), seed=seed))
        seen = torch.zeros(n_envs, starts_per_env, dtype=torch.bool, device=dev)      # (env, start) pairs that were run
        all_envs = torch.arange(n_envs, device=dev)
        # which shape succeeded: one record per episode that ends in a round; the ring holds a round's 30 records per env at most and is
        # read after every round, so it never wraps
        from .metrics import EpisodeLedger
        from .sim import EPISODE_LOG_CAPACITY_MAX
        ledger = EpisodeLedger(n_envs, len(shapes), starts_per_env, keep_coords=False)
        sim.set_episode_log(min(n_envs * 30, EPISODE_LOG_CAPACITY_MAX))
        if param_ranges is not None:
            from .metrics import param_success_table
            ranges = sim.set_param_ranges(seed=seed, **param_ranges).cpu().numpy()
            npdt = np.float32 if sim.dtype == torch.float32 else np.float64
            edges = lambda lo, hi: np.linspace(float(ranges[lo].min()), float(ranges[hi].max()), 5) if ranges[hi].max() > ranges[lo].min() \
                else np.array([float(ranges[lo].min()), float(np.nextafter(ranges[lo].min(), np.inf))])
            mass_edges, mu_edges = edges(0, 1), edges(2, 3)
            p_attempts = np.zeros((len(mass_edges) - 1, len(mu_edges) - 1), dtype=np.int64)
            p_successes = np.zeros_like(p_attempts)
    trainer = None
    if budget_ms is not None and sim.rollout_plan()[0] != "waves":
        # (asked here, with every env on its shape's object: the plan follows the objects' 16-env groups - 14 shapes over 4096 envs leave partly
        # filled groups, more than there are workgroups; 4032 = 14 x 18 whole groups is the wave form)
        plan_name = sim.rollout_plan()[0]
        sim.close()
        raise ValueError(f"run_stage: budget_ms needs the wave form of the rollout kernel (KS_PLAN_WAVES); this context's plan is {plan_name!r}")
    if free_running:
        from .pipeline import AsyncTrainer
        trainer = AsyncTrainer(sim, policy, replay, eng, batch_episodes=policy.batch_size, expert_replay=expert if mix else None, expert_prob=expert_prob,
                               updates_per_step=max(1, round(updates_per_round / 30)), balanced=balanced, prioritized=prioritized, per_alpha=per_alpha,
                               per_beta=per_beta, per_eps=per_eps, per_eps_expert=per_eps_expert)
        trainer.capture()
    for r in range(rounds if free_running else 0):             # a round = one launch, the updates beside it
        trainer.run(30, budget_ms=budget_ms)
        trainer.flush()
        torch.cuda.synchronize(dev)
        records = sim.episode_log()
        ledger.add(records)
        seen[records["env"].long(), records["start_index"].long()] = True
        if param_ranges is not None:
            r_env = records["env"].cpu().numpy()
            r_mass, r_mu = scenarios.param_draw_reference(seed, r_env, records["episode"].cpu().numpy(), ranges, npdt)
            a_, s_ = param_success_table(records, r_mass, r_mu, mass_edges, mu_edges)
            p_attempts += a_
            p_successes += s_
    if trainer is not None:
        trainer.flush(finish_update=True)
        torch.cuda.synchronize(dev)
        seen[all_envs, sim.start_index()[0].long()] = True
        cnt, head = replay.count, replay.head
        tags = replay.ep_class[(head - cnt + torch.arange(cnt, device=dev)) % replay.capacity].cpu().numpy()
        free_out = {"env_steps": int(trainer.steps_total.sum()), "replay_class_counts": {s: int((tags == i).sum()) for i, s in enumerate(shapes)},
                    "batch_class_slots": {}}
        if balanced and trainer.picked is not None and trainer.updates > 0:
            b_agent = int(trainer.batch_episodes * (1 - expert_prob)) if mix else trainer.batch_episodes
            got = replay.ep_class[trainer.picked[:b_agent].long()].cpu().numpy()
            free_out["batch_class_slots"] = {s: int((got == i).sum()) for i, s in enumerate(shapes)}
        if prioritized:
            free_out["priority_max"] = {"agent": replay.priority_max(), "expert": expert.priority_max() if mix else None}
        n_updates = trainer.updates
    for r in range(0 if free_running else rounds):             # lock step: a round = 30 eng.step() calls, then the updates
        if starts_per_env <= 0:
            obs0, _ = reset_all(sim, n_envs)
            eng.start(obs0)
        for t in range(30):
            if seen is not None:
                seen[all_envs, sim.start_index()[0].long()] = True
            eng.step()
        if seen is not None:
            records = sim.episode_log()
            ledger.add(records)
            if param_ranges is not None:
                r_env = records["env"].cpu().numpy()
                r_mass, r_mu = scenarios.param_draw_reference(seed, r_env, records["episode"].cpu().numpy(), ranges, npdt)
                a_, s_ = param_success_table(records, r_mass, r_mu, mass_edges, mu_edges)
                p_attempts += a_
                p_successes += s_
        if replay.count >= 2:
            for u in range(updates_per_round):
                batch = replay.sample_mixed(expert, policy.batch_size, expert_prob) if mix else replay.sample_batch_nstep(policy.batch_size)
                st, ac, ns, rw, nd, w = batch[:6]
                losses.append(native.train_on_batch(st, ac, ns, rw, w))
    if seen is not None:
        sim.set_episode_log(0)                # (the evaluation's episodes end in the kernel too: they are not the stage's)
    # final evaluation: one deterministic episode per env (eval_policy, main_DDPGfD.py:130-272)
    obs0, classes = reset_all(sim, n_envs)
    res = eval_policy(sim, policy, obs0, horizon=30, orientation=plan["requested_orientation"])
    out = {"expert_episodes": 0 if expert is None else int(expert.count), "num_success": res["num_success"], "num_total": n_envs, "avg_reward": res["avg_reward"], "skipped_shapes": skipped, "shapes": shapes,
           "updates": len(losses) if trainer is None else n_updates,
           "distinct_starts": n_envs * rounds if seen is None else int(seen.sum()), "orientation_counts": {c: classes.count(c) for c in sorted(set(classes))}}
    if seen is not None:
        out.update(episodes=ledger.episodes, per_shape_success=ledger.per_object(shapes))
    if trainer is not None:
        out.update(free_out)
    if getattr(policy, "obs_norm", None) is not None:
        sd = policy.obs_norm.std()
        out["obs_std"] = (float(sd.min()), float(sd.max()))
    if param_ranges is not None:
        out["param_success"] = {"mass_edges": mass_edges.tolist(), "mu_edges": mu_edges.tolist(), "attempts": p_attempts.tolist(),
                                "successes": p_successes.tolist()}
    if save:
        for k in ("policy_dir", "replay_dir", "output_dir"):
            Path(dirs[k]).mkdir(parents=True, exist_ok=True)
        stamp = datetime.datetime.now().strftime("%m_%d_%y_%H%M")
        name = f"DDPGfD_kinovaGrip_{stamp}"
        policy.save(str(dirs["policy_dir"] / name))
        replay.save(dirs["replay_dir"])
        text = (f"{'WITH' if 'with_grasp' in str(dirs['exp_dir']) else 'NO'} grasp Experiment {plan['exp_num']}: {plan['exp_name']}, Stage {plan['exp_stage']}\n"
                f"Date: {stamp}\nPrevious experiment: {plan['prev_exp_name']}\nExperiment shapes: {plan['requested_shapes']}\n"
                f"Experiment orientation: {plan['requested_orientation']}\nFinal Policy Evaluation:\n# Success: {out['num_success']}\n"
                f"# Failures: {n_envs - out['num_success']}\n# Total: {n_envs}\nOutput directory: {dirs['exp_dir']}")
        (dirs["output_dir"] / "experiment_info.txt").write_text(text)          # rl_experiment's info file (main_DDPGfD.py:802-822)
        out["policy_path"], out["replay_path"] = str(dirs["policy_dir"] / name), str(dirs["replay_dir"])
    sim.close()
    return out
