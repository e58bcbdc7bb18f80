"""csrc/ks_controller.h on the host, without a GPU: the scripted demonstrators' per-env rule (krsel::controller_one - what
kr_controller_select and the rollout kernels' controller callee compile) against demonstrators.controller_action on fp32 CPU tensors, bit for
bit, against the reference's own fp64 answers (tests/golden/controllers.npz), and the two lift rules and the start-value latch against
known answers written out here.  The header is built stand-alone (tests/native/ks_controller_host.cpp) with g++ -O2 -ffp-contract=off."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from kinovagrasping_amd.demonstrators import controller_action

HERE = Path(__file__).resolve().parent
CSRC = HERE.parent / "kinovagrasping_amd" / "csrc"
MODES = {"naive": 1, "position-dependent": 2, "combined": 3}
TRAIN, EXPERT = 0, 1
SKIP = 6
fp_, u8p_, i64p_ = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
# |fp32 controller - fp64 golden|: the outputs are constants (exact in both up to the rounding of 0.6 and 0.8, <= 3e-8) or
# (obs[81] - obs[78|79]) * (1 + 1/15) clamped to [0.5, 0.8] - two input roundings, a difference, the constant's rounding and a
# product, about five roundings of values <= 0.8 (half an ulp each: 3e-8) - so 5e-7 with margin; no case may flip a branch
GOLDEN_TOL = 5e-7


def F(a):
    return a.ctypes.data_as(fp_)


def U8(a):
    return a.ctypes.data_as(u8p_)


@pytest.fixture(scope="module")
def lib():
    so, src = HERE / "native" / "libks_controller_host.so", HERE / "native" / "ks_controller_host.cpp"
    deps = [src, CSRC / "ks_controller.h"]
    if not so.exists() or any(d.stat().st_mtime > so.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    L = C.CDLL(str(so))
    L.kc_action.argtypes = [C.c_int, C.c_int, fp_, fp_, fp_, u8p_, fp_]
    L.kc_action.restype = None
    L.kc_lift.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, u8p_]
    L.kc_check_grasp.argtypes = [fp_, fp_]
    L.kc_args_ok.argtypes = [C.c_int, C.c_int]
    L.kc_select.argtypes = [C.c_int, C.c_int, C.c_int, fp_, fp_, u8p_, i64p_, u8p_, fp_, C.c_int, fp_, fp_, u8p_]
    L.kc_select.restype = None
    return L


def host_action(lib, mode, obs, init_x, init_dot, lift):
    n = len(obs)
    obs, init_x, init_dot = (np.ascontiguousarray(a, dtype=np.float32) for a in (obs, init_x, init_dot))
    lift8 = np.ascontiguousarray(lift, dtype=np.uint8)
    out = np.full((n, 4), np.nan, dtype=np.float32)
    lib.kc_action(n, MODES[mode], F(obs), F(init_x), F(init_dot), U8(lift8), F(out))
    return out


def torch_action(mode, obs, init_x, init_dot, lift):
    a = controller_action(mode, torch.from_numpy(obs), torch.from_numpy(init_x), torch.from_numpy(init_dot), torch.from_numpy(lift))
    assert a.dtype == torch.float32
    return a.numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.int32), np.ascontiguousarray(b, dtype=np.float32).view(np.int32))


def golden_cases():
    g = np.load(HERE / "golden" / "controllers.npz")
    n = len(g["obs21"])
    obs = np.zeros((n, 82), dtype=np.float32)
    for col, key in ((21, "obs21"), (78, "obs78"), (79, "obs79"), (81, "obs81")):
        obs[:, col] = g[key].astype(np.float32)
    return g, obs, g["init21"].astype(np.float32), g["init81"].astype(np.float32), g["lift"].astype(bool)


def test_the_600_golden_cases_equal_torch_bit_for_bit_and_the_reference_within_five_roundings(lib):
    g, obs, ix, idot, lift = golden_cases()
    assert len(obs) == 600
    for mode, key in (("naive", "action_naive"), ("position-dependent", "action_position_dependent"), ("combined", "action_combined")):
        a = host_action(lib, mode, obs, ix, idot, lift)
        ref = torch_action(mode, obs, ix, idot, lift)
        assert same_bits(a, ref), (mode, int((a != ref).any(1).sum()))
        err = np.abs(a.astype(np.float64) - g[key]).max(1)
        print(f"{mode}: max |fp32 - fp64 golden| over 600 cases {err.max():.3e} (torch fp32: {np.abs(ref.astype(np.float64) - g[key]).max():.3e})")
        assert (err < GOLDEN_TOL).all(), (mode, int((err >= GOLDEN_TOL).sum()), float(err.max()), int(err.argmax()))


def random_cases(n, seed):
    """obs[21] in +-0.08; obs[78], obs[79], obs[81] and the start values likewise in [0, 1.2] / +-0.08; then values ON the thresholds: the
    fp32 roundings of 0.01, 0.02, 0.03, 0.04 (and their negatives) as obs[21] and as the start x, and obs[81] exactly 0.01 (fp32) from the
    start value and from 1, with their fp32 neighbours on either side"""
    rng = np.random.RandomState(seed)
    obs = np.zeros((n, 82), dtype=np.float32)
    obs[:, 21] = rng.uniform(-0.08, 0.08, n)
    for c in (78, 79, 81):
        obs[:, c] = rng.uniform(0.0, 1.2, n)
    ix = rng.uniform(-0.08, 0.08, n).astype(np.float32)
    idot = rng.uniform(0.0, 1.2, n).astype(np.float32)
    lift = rng.rand(n) < 0.4
    edges = np.float32([0.01, 0.02, 0.03, 0.04])
    edges = np.concatenate([edges, np.nextafter(edges, np.float32(1)), np.nextafter(edges, np.float32(0))])
    edges = np.concatenate([edges, -edges]).astype(np.float32)
    k = n // 4
    obs[:k, 21] = edges[rng.randint(len(edges), size=k)]
    ix[k:2 * k] = edges[rng.randint(len(edges), size=k)]
    # |dot - init_dot| on / beside 0.01: dot = init_dot +- e, e in {0.01, its neighbours}
    e = np.float32([0.01, np.nextafter(np.float32(0.01), np.float32(1)), np.nextafter(np.float32(0.01), np.float32(0))])
    sgn = np.where(rng.rand(k) < 0.5, -1.0, 1.0).astype(np.float32)
    obs[2 * k:3 * k, 81] = idot[2 * k:3 * k] + sgn * e[rng.randint(3, size=k)]
    # |1 - dot| on / beside 0.01, and dot close to its start value so that the post-contact forms are reached elsewhere
    obs[3 * k:, 81] = np.float32(1.0) + np.where(rng.rand(n - 3 * k) < 0.5, -1.0, 1.0).astype(np.float32) * e[rng.randint(3, size=n - 3 * k)]
    return obs, ix, idot, lift


def test_a_few_thousand_random_cases_with_values_on_every_threshold_equal_torch_bit_for_bit(lib):
    obs, ix, idot, lift = random_cases(8000, seed=7)
    # the cases reach every branch: centre / right / left, pre- and post-contact, far and near 1, the three bands of the combined mode
    moved = np.abs(obs[:, 81] - idot)
    assert (np.abs(ix) <= np.float32(0.03)).sum() > 500 and (ix > np.float32(0.03)).sum() > 500 and (ix < -np.float32(0.03)).sum() > 500
    assert (moved < np.float32(0.01)).sum() > 200 and (moved > np.float32(0.01)).sum() > 2000 and (moved == np.float32(0.01)).sum() > 10
    assert (np.abs(np.float32(1) - obs[:, 81]) <= np.float32(0.01)).sum() > 500
    x = np.abs(obs[:, 21])
    assert (x > np.float32(0.04)).sum() > 500 and ((x >= np.float32(0.02)) & (x <= np.float32(0.04))).sum() > 500 and (x < np.float32(0.02)).sum() > 500
    for v in np.float32([0.02, 0.03, 0.04]):
        assert (x == v).sum() > 10 and (np.abs(ix) == v).sum() > 10
    for mode in MODES:
        a = host_action(lib, mode, obs, ix, idot, lift)
        ref = torch_action(mode, obs, ix, idot, lift)
        assert same_bits(a, ref), (mode, int((a != ref).any(1).sum()), np.flatnonzero((a != ref).any(1))[:5])
    # values in between the clamp's ends come out (the touch velocities of the side branches: a minority of the cases): the comparison is
    # not one of constants only
    pd = host_action(lib, "position-dependent", obs, ix, idot, lift)
    assert len(np.unique(pd[:, 1:])) > 100


# (t, has_prev, ready_in, still) -> (ready, lifting); still: the fingertips moved less than 0.0002 per substep (check_grasp)
LIFT_TABLE = {
    EXPERT: [  # expert_data.py:746-804: check_grasp from step 2 on and only with a previous observation, every hit counts, the lift flag needs t > 10
        ((0, 0, 0, 1), (0, 0)), ((0, 1, 0, 1), (0, 0)), ((1, 1, 0, 1), (0, 0)), ((2, 1, 0, 1), (1, 0)), ((2, 0, 0, 1), (0, 0)), ((2, 1, 0, 0), (0, 0)),
        ((5, 1, 0, 1), (1, 0)), ((10, 1, 0, 1), (1, 0)), ((10, 1, 1, 0), (1, 0)), ((11, 1, 0, 1), (1, 1)), ((11, 1, 1, 0), (1, 1)), ((11, 0, 1, 0), (1, 1)),
        ((11, 1, 0, 0), (0, 0)), ((11, 0, 0, 1), (0, 0)), ((29, 1, 0, 1), (1, 1)), ((29, 1, 0, 0), (0, 0)), ((1, 0, 1, 0), (1, 0)), ((0, 0, 1, 0), (1, 0)),
    ],
    TRAIN: [   # main_DDPGfD.py:418-439: check_grasp from the 6th step on (t + 1 >= 6), latched, lifting at once
        ((0, 0, 0, 1), (0, 0)), ((4, 1, 0, 1), (0, 0)), ((5, 1, 0, 1), (1, 1)), ((5, 0, 0, 1), (0, 0)), ((5, 1, 0, 0), (0, 0)), ((6, 1, 0, 1), (1, 1)),
        ((2, 1, 1, 0), (1, 1)), ((0, 0, 1, 0), (1, 1)), ((29, 1, 0, 0), (0, 0)), ((29, 1, 0, 1), (1, 1)), ((11, 1, 0, 0), (0, 0)),
    ],
}


def test_both_lift_rules_give_the_known_answers(lib):
    # check_grasp itself: sum |dx| / 15 over columns 9, 12, 15 against 0.0002, as select_one has it
    o, p = np.zeros(82, dtype=np.float32), np.zeros(82, dtype=np.float32)
    assert lib.kc_check_grasp(F(o), F(p)) == 1
    p[9], p[12], p[15] = 0.0009, -0.0009, 0.0009          # 0.0027 / 15 = 0.00018
    assert lib.kc_check_grasp(F(o), F(p)) == 1
    p[15] = 0.0013                                         # 0.0031 / 15 = 0.000207
    assert lib.kc_check_grasp(F(o), F(p)) == 0
    p[:] = 0
    p[10] = p[16] = 1.0                                    # other columns do not count
    assert lib.kc_check_grasp(F(o), F(p)) == 1
    for rule, rows in LIFT_TABLE.items():
        for (t, has_prev, ready_in, still), (ready, lifting) in rows:
            r = np.array([ready_in], dtype=np.uint8)
            got = lib.kc_lift(rule, still, has_prev, t, SKIP, U8(r))
            assert (int(r[0]), got) == (ready, lifting), (rule, t, has_prev, ready_in, still, int(r[0]), got)
    assert all(lib.kc_args_ok(m, r) for m in (1, 2, 3) for r in (0, 1))
    assert not any(lib.kc_args_ok(m, r) for m, r in ((0, 0), (4, 1), (-1, 0), (1, 2), (3, -1)))


@pytest.mark.parametrize("rule", [EXPERT, TRAIN])
def test_the_start_values_are_latched_at_t_0_only_and_the_batch_rule_is_the_pieces_put_together(lib, rule):
    n = 37
    obs, ix, idot, _ = random_cases(n, seed=3)
    rng = np.random.RandomState(5)
    prev = obs.copy()
    moving = rng.rand(n) < 0.5
    prev[moving, 9] += 0.01                                 # 0.01 / 15 > 0.0002: these envs' fingers still move
    t = rng.randint(0, 30, n).astype(np.int64)
    t[:8] = 0
    has_prev = (rng.rand(n) < 0.8).astype(np.uint8)
    ready = (rng.rand(n) < 0.2).astype(np.uint8)
    init = np.stack([ix, idot]).astype(np.float32).copy()
    init0, ready0 = init.copy(), ready.copy()
    action, action_t = np.full((n, 4), np.nan, dtype=np.float32), np.full((4, n), np.nan, dtype=np.float32)
    lifting = np.full(n, 7, dtype=np.uint8)
    lib.kc_select(n, MODES["combined"], rule, F(obs), F(prev), U8(has_prev), t.ctypes.data_as(i64p_), U8(ready), F(init), SKIP, F(action), F(action_t),
                  U8(lifting))
    first = t == 0
    assert first.sum() >= 8 and (~first).sum() > 8
    assert same_bits(init[:, first], np.stack([obs[first, 21], obs[first, 81]])) and same_bits(init[:, ~first], init0[:, ~first])
    still = ~moving
    if rule == EXPERT:
        want_ready = (ready0 != 0) | (still & (has_prev != 0) & (t >= 2))
        want_lift = want_ready & (t > 10)
    else:
        want_ready = (ready0 != 0) | (still & (has_prev != 0) & (t + 1 >= SKIP))
        want_lift = want_ready
    assert np.array_equal(ready != 0, want_ready) and np.array_equal(lifting != 0, want_lift)
    assert want_lift.any() and (~want_lift).any() and (want_ready & ~want_lift).any() == (rule == EXPERT)
    ref = torch_action("combined", obs, init[0].copy(), init[1].copy(), want_lift)
    assert same_bits(action, ref) and same_bits(action_t, ref.T)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rule", ["train", "expert"])
def test_the_engines_torch_path_is_the_header_put_together(lib, mode, rule):
    """RolloutEngine(controller=...).pre() on CPU tensors - the torch statement of the rule, the checker of kr_controller_select on the GPU -
    against controller_one for every env: the same actions, ready, lifting and start values"""
    from types import SimpleNamespace
    from kinovagrasping_amd.rollout import RolloutEngine
    n = 500
    eng = RolloutEngine(SimpleNamespace(n_envs=n, device=torch.device("cpu"), dtype=torch.float32), None, None, controller=mode, lift_rule=rule)
    assert not eng.native
    obs, ix, idot, _ = random_cases(n, seed=11)
    rng = np.random.RandomState(4)
    prev = obs.copy()
    prev[rng.rand(n) < 0.5, 9] += 0.01
    t = rng.randint(0, 30, n).astype(np.int64)
    t[:50] = 0
    has_prev, ready = (rng.rand(n) < 0.8).astype(np.uint8), (rng.rand(n) < 0.2).astype(np.uint8)
    init = np.stack([ix, idot]).astype(np.float32)
    for dst, src in ((eng.obs, obs), (eng.prev_obs, prev), (eng.t, t), (eng.has_prev, has_prev != 0), (eng.ready, ready != 0), (eng.init, init)):
        dst.copy_(torch.from_numpy(src))
    eng.pre()
    action, action_t, lifting = np.zeros((n, 4), np.float32), np.zeros((4, n), np.float32), np.zeros(n, np.uint8)
    lib.kc_select(n, MODES[mode], {"train": TRAIN, "expert": EXPERT}[rule], F(obs), F(prev), U8(has_prev), t.ctypes.data_as(i64p_), U8(ready), F(init), SKIP,
                  F(action), F(action_t), U8(lifting))
    assert same_bits(action, eng.action.numpy()) and same_bits(action_t, eng.action_t.numpy()) and same_bits(init, eng.init.numpy())
    assert np.array_equal(lifting != 0, eng.lifting.numpy()) and np.array_equal(ready != 0, eng.ready.numpy())
    assert lifting.any() and not lifting.all()
