"""The contact solve of every stepping path of the compiled gfx950 kernels - the contact rows of make_constraints (the pyramid edges, R and aref with
impedance on dist - margin, the per-env object mass in wobj), constrained_step on contacts as the 16-lane team runs it (contacts owned by lane
ci % 16, one to three per lane; the basis Jacobian from the LDS cache or rebuilt beyond it; the warm-start choice on contact costs; the line search
over contact rows) and the forces the parity tap publishes - against the oracle on the floor-contact states of tests/contact_solve_states.py, held to the
bounds of tests/contact_solve_ref.py.  tests/test_contact_solve_cpu.py checks the states, the reference and the host lane without a GPU.

Each case is one context (frame_skip 1, horizon 0, contact_tap), one reset to the states' poses, set_env_params (the object mass), set_state (qpos,
qvel, qacc_warmstart), ONE step and get_state with the contact records.

  fp64 ks_substep, fp32 ks_substep     the state's own controls
  fp32 ks_step                         the controls the kernel forms from the state's action; 275 envs (a partly filled last workgroup) holding the state
                                       list over and over, four times: as it is and rotated by 1, 2 and 3 envs; the four placements return the same
                                       bits per state
  fp64 ks_step                         one class per library (count_edges)
  all                                  ncon equal to the oracle's, status 0 (bit 1 only where the oracle dropped: nowhere), every tapped record on the
                                       oracle's pair with the normal (0, 0, 1) and dist / pos within the plane tests' bounds, then qpos, qvel,
                                       qacc_warmstart and the tap's forces within the bounds; no state is set aside - an undecidable one must meet
                                       the bound or lie between the references of its moved states
Run with -s for the table (recorded in profiles/contact_solve_parity.txt)."""
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import contact_solve_ref as cr, contact_solve_states as cs

pytestmark = pytest.mark.gpu

N_TEAM = 275
Path = namedtuple("Path", "name precision kind placements")
SUB64, SUB32 = Path("fp64 ks_substep", 64, "substep", 0), Path("fp32 ks_substep", 32, "substep", 0)
STEP64, STEP32 = Path("fp64 ks_step", 64, "step", 0), Path("fp32 ks_step", 32, "step", 4)
CASES = [(c, s, p) for c, s in cs.cases() for p in (SUB64, SUB32, STEP32)] + [("count_edges", s, STEP64) for s in cs.HAND_SHAPES]
case_id = lambda v: v.name.replace(" ", "_") if isinstance(v, Path) else str(v)
_results = {}


def run_context(s, path: Path, idx):
    """env e holds state idx[e]: {output: [k, n] float64}, ncon, status, contact records [ncon_max, 20, n]"""
    from kinovagrasping_amd.sim import KinovaSim
    n = len(idx)
    sim = KinovaSim(n, s.shape, precision=path.precision, frame_skip=1, horizon=0, contact_tap=True)
    assert sim.multi_geom == cs.on_mg(s.shape)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a[:, idx]))
    sim.reset(t(s.qpos), t(s.hq))
    sim.set_env_params(obj_mass=torch.as_tensor(s.mass[idx]))
    sim.set_state(t(s.qpos), t(s.qvel), t(s.warm))
    if path.kind == "substep":
        sim.substep(t(s.ctrl))
    else:
        sim.step(t(s.action))
    st = sim.get_state(contacts=True)
    torch.cuda.synchronize()
    dt = np.float64 if path.precision == 64 else np.float32
    out = {k: st[name].cpu().numpy().astype(dt) for k, name in (("qpos", "qpos"), ("qvel", "qvel"), ("warm", "qacc_warmstart"))}
    ncon, status, con = st["ncon"].cpu().numpy(), st["status"].cpu().numpy(), st["contact"].cpu().numpy().astype(dt)
    sim.close()
    return out, ncon, status, con


def run_path(cls, shape, path):
    """[(idx, outputs, ncon, status, records)] of every placement of the path"""
    key = (cls, shape, path)
    if key not in _results:
        s = cs.states(cls, shape)
        n = len(s.tag)
        if path.placements:
            assert n <= N_TEAM
            _results[key] = [(idx,) + run_context(s, path, idx) for idx in ((np.arange(N_TEAM) - r) % n for r in range(path.placements))]
        else:
            idx = np.arange(n)
            _results[key] = [(idx,) + run_context(s, path, idx)]
    return _results[key]


@pytest.mark.parametrize("cls,shape,path", CASES, ids=case_id)
def test_one_step_on_floor_contacts_meets_the_bounds(cls, shape, path):
    s = cs.states(cls, shape)
    idx, out, ncon, status, con = run_path(cls, shape, path)[0]
    T = cr.Tally(s, path.kind, path.precision, path.name)
    seen = set()
    for e, i in enumerate(idx):
        if int(i) in seen:
            continue
        seen.add(int(i))
        T.add(int(i), {k: v[:, e].astype(np.float64) for k, v in out.items()}, int(ncon[e]), int(status[e]), con[:, :, e].astype(np.float64))
    print(T.line())
    assert T.n == len(s.tag)
    assert (status == 0).all(), (path.name, "status", int(status.max()))
    T.check()


@pytest.mark.parametrize("cls,shape", cs.cases(), ids=str)
def test_every_team_slot_returns_the_same_bits(cls, shape):
    """the 16-lane kernel: a state gives the same bits - the tapped records and forces included - in whichever team slot of a wave (env % 4) and
    whichever workgroup it stands, the partly filled last one included"""
    runs = run_path(cls, shape, STEP32)
    n = len(cs.states(cls, shape).tag)
    first = {}
    slots = {i: set() for i in range(n)}
    for idx, out, ncon, status, con in runs:
        for e, i in enumerate(idx):
            i = int(i)
            nc = int(ncon[e])
            bits = np.concatenate([out[k][:, e] for k in ("qpos", "qvel", "warm")] + [con[:nc, :7, e].ravel(), con[:nc, 14:17, e].ravel()]).view(np.uint32)
            slots[i].add(e % 4)
            if i not in first:
                first[i] = (bits, nc)
            assert nc == first[i][1] and np.array_equal(bits, first[i][0]) and status[e] == 0, (cls, "state", i, "env", e, "placement differs")
    assert all(len(v) == 4 for v in slots.values()), "every state in every team slot"
