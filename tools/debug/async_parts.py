#!/usr/bin/env python3
"""Free-running rollout: how fast is the rollout launch alone, the learner alone (one-wave kernels, KS_MLP_SPLIT=0), and both?
With a -DKS_ROLLOUT_STAMP build (KS_LIB=...) it also prints the kernel's phase stamps: per workgroup in the workgroup forms, per wave in the
free-running wave form (policy | 15 substeps | rays: snapshot + cull, walks | observation + replay write; walk-loop iterations; with
-DKS_ROLLOUT_STAMP=2 the serial triangle round trips per iteration as well - that build's reductions cost time, read times from a plain one).
usage (GPU box): python tools/debug/async_parts.py [chunk]"""
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from kinovagrasping_amd import scenarios  # noqa: E402
from kinovagrasping_amd.ddpgfd import DDPGfD  # noqa: E402
from kinovagrasping_amd.pipeline import AsyncTrainer  # noqa: E402
from kinovagrasping_amd.replay import DeviceEpisodeReplay  # noqa: E402
from kinovagrasping_amd.rollout import RolloutEngine  # noqa: E402
from kinovagrasping_amd.sim import KinovaSim  # noqa: E402

chunk = int(sys.argv[1]) if len(sys.argv) > 1 else 10
n = 4096
q0, hq = scenarios.config2_states(n)
sim = KinovaSim(n, "CubeS", horizon=30, auto_reset=True)
obs0 = sim.reset(torch.as_tensor(q0), torch.as_tensor(hq))
torch.manual_seed(2)
policy = DDPGfD(82, 4, 0.8, 5, batch_size=64, hidden=(256, 256), device=sim.device)
replay = DeviceEpisodeReplay(n, capacity=4 * n, horizon=30, device=sim.device)
eng = RolloutEngine(sim, policy, replay, expl_noise=0.1)
eng.start(obs0)
tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=64)
tr.capture()
tr.run(36, learn=False); tr.flush()
for _ in range(60):                      # train a while: contact-rich regime
    tr.run(chunk)
tr.flush(); torch.cuda.synchronize()


def timed(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    tr.flush(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * chunk) * 1e3


both = timed(lambda: tr.run(chunk), 30)
roll = timed(lambda: tr.run(chunk, learn=False), 30)


def learner_only():
    with torch.cuda.stream(tr.side):
        for _ in range(chunk):
            tr.g_commit.replay(); tr.g_head.replay(); tr.publish(); tr._body()


learn = timed(learner_only, 30)
ph = tr.counters[4:8].tolist()
waves = tr.rollout_plan == "waves"       # the free-running waves stamp per WAVE (4 envs), the workgroup forms per workgroup (16 envs)
unit, nunit, lanes, tasks = ("wave", n // 4, 64, 4 * 136) if waves else ("workgroup", n // 16, 256, 16 * 136)
if sum(ph):
    import numpy as np
    for label, fn in (("rollout alone", lambda: tr.run(chunk, learn=False)), ("rollout + learner", lambda: tr.run(chunk))):
        tr.flush(); torch.cuda.synchronize()
        ph0, st0, rp0 = tr.counters[4:8].clone(), tr.env_steps, tr.counters[8 + 4 * 512:].clone()
        for _ in range(3):
            fn()
        tr.flush(); torch.cuda.synchronize()
        dph = ((tr.counters[4:8] - ph0).double() / ((tr.env_steps - st0) * nunit) / 100.0).tolist()
        print(f"{label}: phases, mean per {unit} and env-step [us]: policy %.1f  15 substeps %.1f  rays %.1f  observation + replay write %.1f" % tuple(dph))
        rp = ((tr.counters[8 + 4 * 512:] - rp0).double() / ((tr.env_steps - st0) * nunit)).tolist()
        print(f"{label}: rays per {unit} and env-step: snapshot + culling %.1f us, walks %.1f us; surviving (ray, geom) tasks %.0f of {tasks}, node visits %.0f "
              f"(= %.1f per lane), the busiest lane's visits %.0f, subtrees handed to waiting lanes %.0f" % (rp[0] / 100.0, rp[1] / 100.0, rp[2], rp[3], rp[3] / lanes, rp[4], rp[5]))
        # (iterations are counted per wave of 64 lanes in every form; the round trips only by a -DKS_ROLLOUT_STAMP=2 build, whose times are not to be read)
        per_wave = 1.0 if waves else 4.0
        if rp[6]:
            print(f"{label}: walk loop per wave and env-step: %.1f iterations with a node visit = %.2f us each; serial triangle round trips %.1f = %.2f per iteration%s"
                  % (rp[6] / per_wave, rp[1] / 100.0 / (rp[6] / per_wave), rp[7] / per_wave, rp[7] / rp[6], "" if rp[7] else " (not counted by this build)"))
        if waves:
            continue                     # (the per-workgroup launch stamps below are written by the workgroup forms only)
        nwg = nunit
        raw = tr.counters[8:8 + 4 * 512].cpu().numpy().reshape(4, 512)[:, :nwg].astype(np.float64)
        mhz = raw[3] / (raw[2] / 100.0)
        print(f"{label}: shader clock during the loop (cycles / wall time) mean {mhz.mean():.0f} MHz  min {mhz.min():.0f}  max {mhz.max():.0f}")
        c = raw[:3] / 100.0          # us
        entry, stage, loop = c[0] - c[0].min(), c[1], c[2]
        end = entry + stage + loop
        print(f"{label}, last launch of {chunk} env-steps, per workgroup [us]: entry spread max {entry.max():.0f}; tables -> LDS mean {stage.mean():.0f} max {stage.max():.0f}; "
              f"loop mean {loop.mean():.0f}  p50 {np.median(loop):.0f}  p90 {np.percentile(loop, 90):.0f}  max {loop.max():.0f}; first entry -> last exit {end.max():.0f} "
              f"= {end.max() / chunk:.0f} per env-step (mean loop / step {loop.mean() / chunk:.0f})")
if sum(ph):
    tot = tr.env_steps * nunit
    print(f"k_rollout phases, mean per {unit} and env-step [us]: policy %.1f  15 substeps %.1f  rays %.1f  observation + replay write %.1f" % tuple(p / tot / 100.0 for p in ph))
print(f"chunk {chunk}: per env-step  rollout + learner {both:.4f} ms   rollout alone {roll:.4f} ms   learner alone {learn:.4f} ms", flush=True)
sim.close()
