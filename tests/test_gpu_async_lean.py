"""pipeline.AsyncTrainer at the reference's 400-300: the persistent rollout kernel (k_rollout<25,19>) with the whole DDPGfD update
beside it on the lean LDS-free kernels (kr_mlp3_forward_lean / kr_mlp3_backward_lean, NativeDDPGfDUpdate(lean=True))."""
import pytest
import torch

from tests.test_gpu_async import _setup

pytestmark = pytest.mark.gpu

HIDDEN = (400, 300)


def _trainer(n, horizon, **kw):
    from kinovagrasping_amd.pipeline import AsyncTrainer
    sim, policy, replay, eng = _setup(n, horizon, hidden=HIDDEN)
    tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=16, **kw)          # (the parent commit: ValueError)
    assert tr.native.lean and tr.native.lds_free
    return sim, policy, tr


def _launch_synchronous_weights(n, horizon, launch):
    sim, policy, tr = _trainer(n, horizon, launch_synchronous=True, max_launch_steps=horizon + 6)
    tr.capture()
    tr.run(horizon + 6, learn=False)
    for _ in range(2):
        tr.run(launch)
    tr.flush(finish_update=True)
    torch.cuda.synchronize()
    out = (tr.counts(), {k: v.cpu().clone() for k, v in policy._flat_params.items()})
    sim.close()
    return out


def test_async_trainer_runs_400_300_and_is_reproducible_launch_synchronously():
    """272 envs (17 groups), horizon 12.  The default form: two launches through run(), as many updates as asked for, finite parameters,
    a newer published actor.  The launch-synchronous form twice from the same seeds: bit-identical final parameters (the determinism check
    of tests/test_gpu_async.py at 256-256)."""
    n, horizon, launch = 272, 12, 12
    sim, policy, tr = _trainer(n, horizon)
    tr.capture()
    w0 = {k: v.clone() for k, v in policy._flat_params.items()}
    tr.run(horizon + 6, learn=False)
    tr.flush()
    pub0 = tr.n_pub
    for _ in range(2):
        tr.run(launch)
    tr.flush(finish_update=True)
    torch.cuda.synchronize()
    c = tr.counts()
    print("400-300 async trainer:", c, "updates", tr.updates, "published versions", tr.n_pub)
    assert tr.updates == 2 * launch and int(tr.native.it.item()) == 2 * launch
    assert tr.n_pub >= pub0 + 2 * launch and int(tr.pub_ver) == tr.n_pub
    assert torch.equal(tr.pub[tr.n_pub % 3, :tr.actor_flat.numel()], tr.actor_flat)
    for k, w in policy._flat_params.items():
        assert torch.isfinite(w).all(), k
    for k in ("actor", "critic"):
        assert (policy._flat_params[k] - w0[k]).abs().max().item() > 0, k
    assert torch.isfinite(tr.native.losses).all()
    assert torch.equal(tr.steps_total, torch.full_like(tr.steps_total, horizon + 6 + 2 * launch))
    sim.close()
    a = _launch_synchronous_weights(n, horizon, launch)
    b = _launch_synchronous_weights(n, horizon, launch)
    assert a[0]["episodes_dropped"] == 0 and a[0] == b[0], (a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_lean_learner_waves_are_resident_beside_the_400_300_rollout_kernel():
    """4096 envs: 256 groups, a persistent workgroup on every CU, holding 416 of the 512 registers of every SIMD lane and all of the LDS for the
    whole launch of 60 env-steps.  Three replays of the captured update, unpaced, on the trainer's own learner stream, issued right after the
    launch: the learner's last event must precede the launch's end.  Learner waves that cannot be resident beside k_rollout<25,19> start
    only as its workgroups retire, and the learner would end after the launch."""
    sim, policy, tr = _trainer(4096, 30)
    tr.capture()
    torch.cuda.synchronize()
    main, side = tr.main, tr.side
    assert torch.cuda.current_stream(sim.device) == main
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    side.wait_stream(main)
    ev[0].record(main)
    sim.rollout(60, tr.args)
    ev[1].record(main)
    with torch.cuda.stream(side):
        ev[2].record(side)
        for _ in range(3):
            tr.g_head.replay()
            tr._body()
        ev[3].record(side)
    torch.cuda.synchronize()
    rollout_ms, learner_start, learner_end = ev[0].elapsed_time(ev[1]), ev[0].elapsed_time(ev[2]), ev[0].elapsed_time(ev[3])
    print(f"400-300: launch of 60 env-steps {rollout_ms:.1f} ms; three updates beside it from {learner_start:.2f} to {learner_end:.1f} ms "
          f"({(learner_end - learner_start) / 3:.2f} ms each)")
    assert tr.updates == 3 and learner_end < rollout_ms, (learner_end, rollout_ms)
    sim.close()
