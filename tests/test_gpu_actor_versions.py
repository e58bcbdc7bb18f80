"""The weight hand-off of the free-running rollout kernel (include/kinova_sim.h, ks_rollout_args.actor_pub / actor_ver): the learner publishes a
new actor into one of three buffers while k_rollout keeps acting.  Every action the kernel stores must come from ONE whole published version -
never a mix of two buffers, never a version older than one the same env already acted with, never one published after the launch's bounds.

Method: with expl_noise = 0 a stored action is 0.8 * sigmoid(...) of exactly one forward, and kr_actor_select's actor_out is bit-equal to the
in-kernel tile for the same weights (test_gpu_async.py).  So for every stored (state, action) row, the versions whose lock-step forward
reproduces the action bit for bit are the versions the kernel can have read; the fp64 torch forward of the matched version anchors the
identification (<= 2e-5, the tolerance of test_fused_mlp_forward_matches_torch).

Also here: the in-kernel exploration noise (krsel::normal4, csrc/ks_select.h) against the fp64 Philox4x32-10 / Box-Muller reference
(tests/philox_ref.py, whose Philox reproduces Random123's known answers: test_noise_reference_cpu.py)."""
import collections

import numpy as np
import pytest
import torch

from kinovagrasping_amd import scenarios
from tests import philox_ref

pytestmark = pytest.mark.gpu

LIFT = (0.6, 0.5, 0.5, 0.5)                  # the scripted lift action (krsel::lift_action): such rows come from no forward


def _setup(n, horizon, hidden=(256, 256), cohort=1, ring=8):
    """test_gpu_async._setup without exploration noise (sigma = 0: every stored action is the actor's output)"""
    from kinovagrasping_amd.ddpgfd import DDPGfD
    from kinovagrasping_amd.replay import DeviceEpisodeReplay
    from kinovagrasping_amd.rollout import RolloutEngine
    from kinovagrasping_amd.sim import KinovaSim
    if cohort > 1:
        oid, _, q0, hq, mf = scenarios.config5_states(n, seed=5, cohort=cohort)
        sim = KinovaSim(n, scenarios.SHAPES, horizon=horizon, auto_reset=True)
        obs0 = sim.reset(torch.as_tensor(q0), torch.as_tensor(hq), object_id=oid, mass_friction=mf)
    else:
        q0, hq = scenarios.config2_states(n)
        sim = KinovaSim(n, "CubeS", horizon=horizon, auto_reset=True)
        obs0 = sim.reset(torch.as_tensor(q0), torch.as_tensor(hq))
    torch.manual_seed(2)
    policy = DDPGfD(82, 4, 0.8, 5, batch_size=64, hidden=hidden, device=sim.device)
    replay = DeviceEpisodeReplay(n, capacity=ring * n, horizon=horizon, device=sim.device)
    eng = RolloutEngine(sim, policy, replay, expl_noise=0.0)
    eng.start(obs0)
    return sim, policy, replay, eng


# ---- reading what the kernel stored

def _episode_rows(parts):
    """parts: (state [E, H, 82], action [E, H, 4], len [E]) -> rows of every episode in time order: state [R, 82], action [R, 4], episode id [R]
    (scripted-lift rows left out)"""
    S, A, E = [], [], []
    base = 0
    for st, ac, ln in parts:
        if st.shape[0] == 0:
            continue
        m = torch.arange(st.shape[1], device=st.device)[None, :] < ln[:, None]
        eid = (torch.arange(st.shape[0], device=st.device) + base)[:, None].expand(-1, st.shape[1])
        S.append(st[m]); A.append(ac[m]); E.append(eid[m])
        base += st.shape[0]
    S, A, E = torch.cat(S), torch.cat(A), torch.cat(E)
    keep = ~(A == torch.tensor(LIFT, device=A.device)).all(1)
    return S[keep].contiguous(), A[keep].contiguous(), E[keep]


def _snapshot(replay, stage=None):
    """every stored row that is visible now: the ring's episodes, the staging ring's (launch-synchronous form), and both open-episode buffers
    of every env - a published buffer with its published length, the open one with its current length (ks_rollout.hip / k_rollout's store:
    rows [0, len) of a buffer are the episode's transitions in order; lift steps are not stored)"""
    parts = []
    for r in (replay, stage):
        if r is not None:
            c = r.count
            parts.append((r.ep_state[:c], r.ep_action[:c], r.ep_len[:c]))
    for b in (0, 1):
        ln = torch.where(replay.pub_len[b] > 0, replay.pub_len[b], torch.where(replay.a_sel.long() == b, replay.a_len[b], torch.zeros_like(replay.a_len[b])))
        parts.append((replay.a_state[b], replay.a_action[b], ln))
    return _episode_rows(parts)


_MULT = None


def _row_hash(S, A):
    global _MULT
    x = torch.cat([S, A], 1).view(torch.int32).long() & 0xFFFFFFFF
    if _MULT is None or _MULT.device != x.device:
        g = torch.Generator().manual_seed(7)
        _MULT = (torch.randint(1, 2**62, (x.shape[1],), generator=g) * 2 + 1).to(x.device)
    return (x * _MULT).sum(1).cpu().numpy()            # (int64 arithmetic wraps: a 64-bit hash of the row's bits)


def _new_rows(h_now, h_prev):
    """rows of this snapshot beyond what the previous one already held (by content: an episode moves from an open buffer into the ring
    between two snapshots; rows with identical bits identify identically, so which copy counts as new does not matter)"""
    prev = collections.Counter(h_prev.tolist()) if h_prev is not None else collections.Counter()
    out = np.zeros(len(h_now), dtype=bool)
    for i, x in enumerate(h_now.tolist()):
        if prev[x] > 0:
            prev[x] -= 1
        else:
            out[i] = True
    return out


# ---- identification

def _lock_step_outputs(L, S, flat, args):
    """kr_actor_select's actor_out (the lock-step fused actor) for rows S with the weights `flat` (sigma = 0, no check_grasp state)"""
    from kinovagrasping_amd.rollout import SKIP_NUM_TS
    R, dev = S.shape[0], S.device
    z8 = torch.zeros(R, dtype=torch.uint8, device=dev)
    t = torch.zeros(R, dtype=torch.long, device=dev)
    noise = torch.zeros(R, 4, device=dev)
    out, act, act_t = torch.empty(R, 4, device=dev), torch.empty(R, 4, device=dev), torch.empty(4, R, device=dev)
    lifting = torch.empty(R, dtype=torch.uint8, device=dev)
    w = lambda off: flat.data_ptr() + 4 * off
    rc = L.kr_actor_select(R, args.h1, args.h2, S.data_ptr(), S.data_ptr(), z8.data_ptr(), t.data_ptr(), z8.clone().data_ptr(), w(args.off_w1),
                           w(args.off_b1), w(args.off_w2), w(args.off_b2), w(args.off_w3), w(args.off_b3), noise.data_ptr(), 0, None, 0.0, args.max_action,
                           SKIP_NUM_TS, out.data_ptr(), act.data_ptr(), act_t.data_ptr(), lifting.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return out


def _fp64_outputs(S, flat, args, chunk=1 << 17):
    h1, h2 = args.h1, args.h2
    f = flat.double()
    W1, b1 = f[args.off_w1:args.off_w1 + h1 * 82].view(h1, 82), f[args.off_b1:args.off_b1 + h1]
    W2, b2 = f[args.off_w2:args.off_w2 + h2 * h1].view(h2, h1), f[args.off_b2:args.off_b2 + h2]
    W3, b3 = f[args.off_w3:args.off_w3 + 4 * h2].view(4, h2), f[args.off_b3:args.off_b3 + 4]
    out = []
    for i in range(0, S.shape[0], chunk):
        x = S[i:i + chunk].double()
        x = torch.relu(x @ W1.T + b1)
        x = torch.relu(x @ W2.T + b2)
        out.append(args.max_action * torch.sigmoid(x @ W3.T + b3))
    return torch.cat(out)


def _identify(L, S, A, versions, args):
    """-> match [R, K] bool (version v's lock-step forward gives the stored action bit for bit), the fp64 anchor error of the lowest matched
    version [R], the distance of the nearest NOT matched version's fp64 output from the action [R] (max over the 4 components)"""
    R, K = S.shape[0], len(versions)
    match = torch.zeros(R, K, dtype=torch.bool, device=S.device)
    Ai = A.view(torch.int32)
    for v, flat in enumerate(versions):
        match[:, v] = (_lock_step_outputs(L, S, flat, args).view(torch.int32) == Ai).all(1)
    first = torch.where(match.any(1), match.int().argmax(1), torch.full((R,), -1, device=S.device))
    anchor = torch.full((R,), float("inf"), dtype=torch.float64, device=S.device)
    other = torch.full((R,), float("inf"), dtype=torch.float64, device=S.device)
    for v, flat in enumerate(versions):
        d = (_fp64_outputs(S, flat, args) - A.double()).abs().amax(1)
        anchor = torch.where(first == v, d, anchor)
        other = torch.where(match[:, v], other, torch.minimum(other, d))
    return match, first, anchor, other


def _monotone_violations(match, eid):
    """episodes along which no non-decreasing choice of versions exists (each row may match a set of versions: the greedy choice of the
    smallest admissible version decides)"""
    M, e = match.cpu().numpy(), eid.cpu().numpy()
    K = M.shape[1]
    uniq, inv = np.unique(e, return_inverse=True)
    pos = np.zeros(len(e), dtype=np.int64)
    start = np.r_[0, np.flatnonzero(np.diff(inv)) + 1]            # rows of an episode are contiguous and in time order
    for s, t in zip(start, np.r_[start[1:], len(e)]):
        pos[s:t] = np.arange(t - s)
    cur = np.full(len(uniq), -1)
    bad = np.zeros(len(uniq), dtype=bool)
    ar = np.arange(K)
    for p in range(pos.max() + 1 if len(pos) else 0):
        rows = np.flatnonzero(pos == p)
        ep = inv[rows]
        ok = M[rows] & (ar[None, :] >= cur[ep][:, None])
        has = ok.any(1)
        bad[ep[~has]] = True
        cur[ep[has]] = ok[has].argmax(1)
    return int(bad.sum())


def _check_launch(name, L, snap, prev_hash, versions, args, lo, hi, exact=False, distinct=False):
    """identification of every visible row + the checks of the rows stored during this launch (versions in [lo, hi]; exact: the launch acted
    with version hi only).  Returns the row hashes and a report."""
    S, A, E = snap
    match, first, anchor, other = _identify(L, S, A, versions, args)
    h = _row_hash(S, A)
    new = torch.as_tensor(_new_rows(h, prev_hash), device=S.device)
    unmatched = int((first < 0).sum())
    assert unmatched == 0, f"{name}: {unmatched} of {len(first)} stored actions match no published version bit for bit (a torn or foreign read)"
    assert anchor.max().item() <= 2e-5, f"{name}: fp64 forward of the matched version {anchor.max().item():.2e} from the stored action"
    if distinct:
        share = (other >= 1e-3).double().mean().item()
        assert share >= 0.999, f"{name}: only {share:.4f} of rows have every other version >= 1e-3 away"
    nv = _monotone_violations(match, E)
    assert nv == 0, f"{name}: {nv} episodes act with an OLDER version after a newer one"
    Mn = match[new]
    assert Mn.shape[0] > 0, f"{name}: no rows stored during the launch"
    inside = Mn[:, lo:hi + 1].any(1)
    assert inside.all(), f"{name}: {int((~inside).sum())} rows match no version in [{lo}, {hi}] - the versions published before / during this launch"
    if exact:
        assert Mn[:, hi].all() and not Mn[:, hi + 1:].any(), f"{name}: a launch-synchronous launch acted with another version than {hi}"
    # episodes (with rows of this launch) whose rows of this launch used >= 2 versions
    fn, en = first[new], E[new]
    ue, inv = torch.unique(en, return_inverse=True)
    vmin = torch.full((len(ue),), 1 << 30, device=S.device, dtype=torch.long).scatter_reduce(0, inv, fn.long(), "amin")
    vmax = torch.full((len(ue),), -1, device=S.device, dtype=torch.long).scatter_reduce(0, inv, fn.long(), "amax")
    span = (vmax > vmin).double().mean().item()
    seen = sorted(set(torch.unique(fn).tolist()))
    rep = dict(rows=int(new.sum()), versions_seen=len(seen), version_range=(seen[0], seen[-1]), episodes=len(ue), spanning=round(span, 3))
    return h, rep


# ---- 2. a synthetic publisher beside the running kernel, every scheduling form

def _random_versions(policy, k, seed):
    """k very different actors (fresh weights; l3.bias spread so that outputs cover about 0.1 - 0.7 of the 0.8 bound), as flat copies"""
    actor, flat = policy.actor, policy._flat_params["actor"]
    g = torch.Generator(device=flat.device).manual_seed(seed)
    out = []
    with torch.no_grad():
        for _ in range(k):
            for lin in (actor.l1, actor.l2, actor.l3):
                bound = lin.weight.shape[1] ** -0.5
                lin.weight.copy_((torch.rand(lin.weight.shape, generator=g, device=flat.device) * 2 - 1) * bound)
                lin.bias.copy_((torch.rand(lin.bias.shape, generator=g, device=flat.device) * 2 - 1) * bound)
            p = 0.125 + 0.75 * torch.rand(4, generator=g, device=flat.device)
            actor.l3.bias.copy_(torch.log(p / (1 - p)))
            out.append(flat.clone())
    return out


def _schedule(base):
    """(target env-step, publications): every 3rd env-step of a 44-step launch, bursts of 3 back to back at two of every three"""
    return [(base + 1 + 3 * j, 1 if j % 3 == 2 else 3) for j in range(15)]


@pytest.mark.parametrize("hidden,n,env,cohort,plan", [((256, 256), 4096, {}, 1, "waves"), ((64, 64), 272, {}, 1, "waves"),
                                                      ((128, 128), 272, {}, 1, "waves"), ((256, 256), 272, {"KS_ROLLOUT_WAVES": "0"}, 1, "workgroups"),
                                                      ((256, 256), 8192, {}, 16, "queue")])
def test_every_stored_action_comes_from_one_whole_published_version(monkeypatch, hidden, n, env, cohort, plan):
    """Two launches of 44 env-steps at horizon 30 (no episode ends on a launch's last step, where its env would drop it: the rows of the
    second launch's later versions stay visible); beside each, on another stream, the product's own writer (AsyncTrainer.publish) publishes 35
    very different actors paced on the envs' progress (kr_wait_min_counted on steps_total): singles and bursts of three (a forward that overlaps
    a burst sees the counter move by two and must repeat).  Episodes are collected only between the launches (some may be dropped).
    Every width the product trainer takes (AsyncTrainer needs the LDS-free learner: 256-256, 128-128, 64-64 - not 400-300).
    Measured on an MI355X: the whole file runs in about 10 s; repeated forwards per burst: 4.2 % of the waves at 4096 envs,
    5 - 9 % at 272 envs (128-128), 8 % of the workgroups in the barrier-joined form.  At 64-64 the forward is so short that, with the publisher
    on its high-priority stream, none repeated in three runs (28 and 36 on a normal-priority stream): that case does not require a repeat."""
    from kinovagrasping_amd.pipeline import AsyncTrainer
    from kinovagrasping_amd.sim import load_library
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    per, launches = 44, 2
    sim, policy, replay, eng = _setup(n, 30, hidden=hidden, cohort=cohort)
    K = 1 + sum(b for _, b in _schedule(0)) * launches
    versions = _random_versions(policy, K, seed=11)
    policy._flat_params["actor"].copy_(versions[0])
    tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=16)
    form = sim.rollout_plan()[0]
    assert form == plan == tr.rollout_plan, (form, plan)
    L = load_library()
    dev = sim.device
    # the publisher on a high-priority stream: HIP takes its hardware queue from another pool than the launch's, so that the publications
    # cannot end up queued behind the persistent launch (with a normal-priority stream that sharing was seen: no version changed under it)
    main, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev, priority=-1)
    timeouts = torch.zeros(1, dtype=torch.long, device=dev)
    torch.cuda.synchronize()
    prev_hash, reports = None, []
    for launch in range(launches):
        lo = tr.n_pub
        side.wait_stream(main)
        sim.rollout(per, tr.args)
        with torch.cuda.stream(side):
            for target, burst in _schedule(launch * per):
                assert L.kr_wait_min_counted(tr.steps_total.data_ptr(), n, target, 10.0, timeouts.data_ptr(), side.cuda_stream) == 0
                for _ in range(burst):
                    tr.actor_flat = versions[tr.n_pub + 1]
                    tr.publish()
        main.wait_stream(side)
        torch.cuda.synchronize()
        replay.commit_published()
        torch.cuda.synchronize()
        prev_hash, rep = _check_launch(f"{form} {hidden} launch {launch}", L, _snapshot(replay), prev_hash, versions, tr.args, lo, tr.n_pub, distinct=True)
        reports.append(rep)
    tr.actor_flat = policy._flat_params["actor"]
    c, reps = tr.counts(), tr.repeated_forwards()
    print(f"\n{form} {hidden} n={n}: {tr.n_pub} versions published, repeated forwards {reps}, pacing waits timed out {int(timeouts)}, counts {c}")
    for i, r in enumerate(reports):
        print(f"  launch {i}: {r['rows']} rows checked, {r['versions_seen']} versions seen ({r['version_range'][0]}..{r['version_range'][1]}), "
              f"{r['spanning']:.1%} of {r['episodes']} episodes span >= 2 versions")
    assert tr.n_pub == K - 1 and int(timeouts) == 0
    assert all(r["spanning"] >= 0.25 for r in reports), "the versions did not change under the running kernel: nothing was tested"
    assert reps > 0 or hidden == (64, 64), "no forward overlapped a burst: the repeat path was not exercised"
    assert (sim.get_state()["status"] & 2).sum().item() == 0
    sim.close()


# ---- 3. the product trainer with its real learner

@pytest.mark.parametrize("launch_synchronous", [False, True])
def test_async_trainer_acts_with_whole_published_versions(launch_synchronous):
    """4096 envs, the learner beside the launches publishing after every Adam step (launch-synchronous: once, before every launch).  Every
    publication is recorded (publish() is eager Python on the learner's stream: a clone behind its copy holds what was published).  Consecutive
    learner versions are close, so a row may match several; what must hold is a non-decreasing choice along every episode, and the launch's
    bounds (launch-synchronous: exactly the version published at the launch's boundary)."""
    from kinovagrasping_amd.pipeline import AsyncTrainer
    from kinovagrasping_amd.sim import load_library
    n = 4096
    sim, policy, replay, eng = _setup(n, 30)
    tr = AsyncTrainer(sim, policy, replay, eng, batch_episodes=64, launch_synchronous=launch_synchronous)
    history = [tr.pub[0, :tr.actor_flat.numel()].clone()]
    publish = tr.publish

    def recorded_publish():
        publish()
        history.append(tr.actor_flat.clone())            # (same stream, behind the copy and before the next update)
    tr.publish = recorded_publish
    tr.capture()
    L = load_library()
    prev_hash, reports = None, []
    for i, (steps, learn) in enumerate([(36, False), (30, True), (30, True), (30, True)]):
        lo = tr.n_pub
        tr.run(steps, learn=learn)
        torch.cuda.synchronize()
        hi = tr.n_pub
        assert len(history) == hi + 1
        prev_hash, rep = _check_launch(f"trainer launch {i}", L, _snapshot(replay, tr.stage if launch_synchronous else None), prev_hash, history,
                                       tr.args, hi if launch_synchronous else lo, hi, exact=launch_synchronous)
        reports.append(rep)
    c = tr.counts()
    print(f"\ntrainer launch_synchronous={launch_synchronous} ({tr.rollout_plan}): {tr.n_pub} versions published, repeated forwards "
          f"{tr.repeated_forwards()}, counts {c}")
    for i, r in enumerate(reports):
        print(f"  launch {i}: {r['rows']} rows checked, {r['versions_seen']} versions seen ({r['version_range'][0]}..{r['version_range'][1]}), "
              f"{r['spanning']:.1%} of {r['episodes']} episodes span >= 2 versions")
    assert tr.updates == 90 and c["pacing_timeouts"] == 0
    if not launch_synchronous:
        assert tr.n_pub == 90 and all(r["versions_seen"] >= 2 for r in reports[1:])
    assert (sim.get_state()["status"] & 2).sum().item() == 0
    sim.close()


# ---- 5. the exploration noise against its fp64 reference

NOISE_TOL = 6e-6          # 3 x the measured maximum (1.94e-6 on an MI355X over the 1.1 M draws below): __logf / __sincosf, the fp32 products


def test_in_kernel_noise_equals_the_fp64_philox_box_muller_reference():
    """kr_actor_select with its in-kernel generator on a zero actor: pi = max_action / 2 = 8 for every row, sigma = 1, so the stored action is
    8 + z (|z| < 6: never clipped; 8 + z is rounded to fp32, < 1e-6).  Seeds with high bits set, step counters around and above 2^32, env ids up
    to 8191.  A wrong counter word, key word or Box-Muller pairing is an O(1) error; the kernel's fast __logf / __sincosf stay far below."""
    from kinovagrasping_amd.rollout import SKIP_NUM_TS
    from kinovagrasping_amd.sim import load_library
    L = load_library()
    dev = torch.device("cuda", 0)
    n, h = 8192, 64
    obs = torch.randn(n, 82, device=dev)
    z8 = torch.zeros(n, dtype=torch.uint8, device=dev)
    t = torch.zeros(n, dtype=torch.long, device=dev)
    W1, b1, W2, b2 = torch.zeros(h, 82, device=dev), torch.zeros(h, device=dev), torch.zeros(h, h, device=dev), torch.zeros(h, device=dev)
    W3, b3 = torch.zeros(4, h, device=dev), torch.zeros(4, device=dev)
    rng = torch.zeros(2, dtype=torch.long, device=dev)
    act, act_t, out = torch.empty(n, 4, device=dev), torch.empty(4, n, device=dev), torch.empty(n, 4, device=dev)
    lifting, ready = torch.empty(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    worst = 0.0
    for seed in (0, 1, 0x9E3779B97F4A7C15, 0xFFFFFFFF00000000, 2**64 - 1):
        for step in (0, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 0x0123456789AB, 2**62 + 5):
            rng[0], rng[1] = step, 0
            ready.zero_()
            rc = L.kr_actor_select(n, h, h, obs.data_ptr(), obs.data_ptr(), z8.data_ptr(), t.data_ptr(), ready.data_ptr(), W1.data_ptr(), b1.data_ptr(),
                                   W2.data_ptr(), b2.data_ptr(), W3.data_ptr(), b3.data_ptr(), None, seed, rng.data_ptr(), 1.0, 16.0, SKIP_NUM_TS,
                                   out.data_ptr(), act.data_ptr(), act_t.data_ptr(), lifting.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            torch.cuda.synchronize()
            assert torch.equal(out, torch.full_like(out, 8.0)) and int(rng[0]) == step + 1
            z = act.double().cpu().numpy() - 8.0
            ref = philox_ref.normal4(np.uint64(seed), np.uint64(step), np.arange(n, dtype=np.uint64))
            err = np.abs(z - ref).max()
            worst = max(worst, err)
            assert err <= NOISE_TOL, (hex(seed), hex(step), err, np.unravel_index(np.abs(z - ref).argmax(), z.shape))
    print(f"\nin-kernel noise vs fp64 reference: max |z - z_ref| = {worst:.3e} over {5 * 7 * n * 4} draws (tolerance {NOISE_TOL:.0e})")
