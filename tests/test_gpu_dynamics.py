"""The smooth dynamics and the contact-free solve of every stepping path of the compiled gfx950 kernels - dynamics_rows, make_constraints,
constrained_step and the Euler step as the 16-lane team of every stepping kernel runs them (roles by lane, the DPP Cholesky, the scalar rows dealt
to lanes 0 - 9 of the line search; the one-lane form is the host lane's) - against the oracle on the aimed contact-free states of tests/dynamics_states.py, held to the bounds of
tests/dynamics_ref.py.  tests/test_dynamics_cpu.py checks the states, the reference and the host lane without a GPU.

Each case is one context (frame_skip 1, horizon 0), one reset to the states' poses, set_env_params (the object mass), set_state (qpos, qvel,
qacc_warmstart), ONE step and get_state.

  fp64 ks_substep, fp32 ks_substep (k_substep)          the state's own controls
  fp64 ks_step (k_env_step), fp32 ks_step (k_env_step_f32) the controls the kernel forms from the state's action (reference: ko.env_ctrl at the
                                                        oracle's palm pose); the class `actuator` is left out
  fp32 ks_step                                          275 envs (a partly filled last workgroup) holding the state list over and over, four times:
                                                        as it is and rotated by 1, 2 and 3 envs, so that every state meets every team slot of a
                                                        wave; the four placements return the same bits per state
  all                                                   ncon == 0 and status == 0 on every env, every element finite, the bounds on qpos, qvel and
                                                        qacc_warmstart; a failure names class, state, output, component and the ratio to the bound
Run with -s for the table (recorded in profiles/dynamics_parity.txt)."""
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import dynamics_ref as dr, dynamics_states as ds

pytestmark = pytest.mark.gpu

N_TEAM = 275
Path = namedtuple("Path", "name precision kind placements")
SUB64, SUB32 = Path("fp64 ks_substep", 64, "substep", 0), Path("fp32 ks_substep", 32, "substep", 0)
STEP64, STEP32 = Path("fp64 ks_step", 64, "step", 0), Path("fp32 ks_step", 32, "step", 4)
PATHS = (SUB64, SUB32, STEP64, STEP32)
CASES = [(c, s, p) for c, s in ds.cases() for p in PATHS if not (c == "actuator" and p.kind == "step")]
case_id = lambda v: v.name.replace(" ", "_") if isinstance(v, Path) else str(v)
_results = {}


def run_context(s: ds.States, path: Path, idx):
    """env e holds state idx[e]: {output: [k, n] float64}, ncon, status"""
    from kinovagrasping_amd.sim import KinovaSim
    n = len(idx)
    sim = KinovaSim(n, s.shape, precision=path.precision, frame_skip=1, horizon=0)
    assert sim.multi_geom == (s.shape == ds.MG_SHAPE)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a[:, idx]))
    sim.reset(t(s.qpos), t(s.hq))
    sim.set_env_params(obj_mass=torch.as_tensor(s.mass[idx]))
    sim.set_state(t(s.qpos), t(s.qvel), t(s.warm))
    if path.kind == "substep":
        sim.substep(t(s.ctrl))
    else:
        sim.step(t(s.action))
    st = sim.get_state()
    torch.cuda.synchronize()
    dt = np.float64 if path.precision == 64 else np.float32
    out = {k: st[name].cpu().numpy().astype(dt) for k, name in (("qpos", "qpos"), ("qvel", "qvel"), ("warm", "qacc_warmstart"))}
    ncon, status = st["ncon"].cpu().numpy(), st["status"].cpu().numpy()
    sim.close()
    return out, ncon, status


def run_path(cls, shape, path):
    """[(idx, outputs, ncon, status)] of every placement of the path"""
    key = (cls, shape, path)
    if key not in _results:
        s = ds.states(cls, shape)
        n = len(s.tag)
        if path.placements:
            assert n <= N_TEAM
            _results[key] = [(idx,) + run_context(s, path, idx) for idx in ((np.arange(N_TEAM) - r) % n for r in range(path.placements))]
        else:
            idx = np.arange(n)
            _results[key] = [(idx,) + run_context(s, path, idx)]
    return _results[key]


@pytest.mark.parametrize("cls,shape,path", CASES, ids=case_id)
def test_one_step_of_every_gpu_path_meets_the_bounds(cls, shape, path):
    s = ds.states(cls, shape)
    idx, out, ncon, status = run_path(cls, shape, path)[0]
    T = dr.Tally(s, path.kind, path.precision, path.name)
    seen = set()
    for e, i in enumerate(idx):
        if int(i) in seen:
            continue
        seen.add(int(i))
        T.add(int(i), {k: v[:, e].astype(np.float64) for k, v in out.items()}, int(ncon[e]), int(status[e]))
    print(T.line())
    assert T.n == len(s.tag)
    assert (ncon == 0).all() and (status == 0).all(), (path.name, "ncon / status", int(np.abs(ncon).max()), int(status.max()))
    T.check()


@pytest.mark.parametrize("cls,shape", [(c, s) for c, s in ds.cases() if c != "actuator"], ids=str)
def test_every_team_slot_returns_the_same_bits(cls, shape):
    """the 16-lane kernel: a state gives the same bits in whichever team slot of a wave (env % 4) and whichever workgroup it stands, the partly
    filled last one included"""
    runs = run_path(cls, shape, STEP32)
    n = len(ds.states(cls, shape).tag)
    first = {}
    slots = {i: set() for i in range(n)}
    for idx, out, ncon, status in runs:
        for e, i in enumerate(idx):
            i = int(i)
            bits = np.concatenate([out[k][:, e] for k in ("qpos", "qvel", "warm")]).view(np.uint32)
            slots[i].add(e % 4)
            if i not in first:
                first[i] = bits
            assert np.array_equal(bits, first[i]) and ncon[e] == 0 and status[e] == 0, (cls, "state", i, "env", e, "placement differs")
    assert all(len(v) == 4 for v in slots.values()), "every state in every team slot"
