"""Reference and bounds for the states of tests/dynamics_states.py.  The reference is the oracle itself: one ko_step from the state gives qpos,
qvel and qacc_warmstart, and its forward pass gives what the bounds are made of (M, efc_J, efc_R, efc_aref, efc_force, qfrc_bias, qfrc_passive,
qfrc_actuator).  Nothing here looks at a kernel's output.

fp64 paths   the project's one-step figures: qpos 1e-9, qvel 1e-7; qacc_warmstart 1e-9 (1 + |qacc|_max of the state) - the oracle's own Newton
             tolerance sets that floor, not rounding.
fp32 paths   a componentwise forward bound, u = 2^-24, h the time step, `act` the oracle's active rows (equalities, and rows with efc_force != 0):
               H = M + J_act^T D J_act
               F           = |qfrc_bias| + |qfrc_passive| + |qfrc_actuator| + W + V    (W, V: majorants of the weight and of the velocity-product
                                                                                        forces on each joint whatever the pose, see `weight`)
               bound_a     = |H^-1| (|H| |qacc| + F + |J_act|^T |D aref|)
               bound_euler = |Md^-1| (|Md| |qacc'| + F + |J_act|^T D (|J_act| (|qacc| + bound_a) + |aref|)),  Md = M + h diag(damping)
                             (a row's force is f = D (aref - J qacc): |f| alone misses what cancels in that difference - a tendon 0.05 rad off
                             its rest holds |aref| = 131 against |J qacc| of the same size - and qacc is the solver's, whose own error c u bound_a
                             the Euler solve takes in through J^T D J: a finger whose servo and limit row hold 0.33 N m against each other
                             leaves qacc = 0.25 where the forces alone would give 33)
               each with its second-order term C u |bound|_max added (a first-order bound of a component that is exactly zero in the reference
               would forbid the 1e-19 that the kernel's COM offset of 1e-20 m leaves there)
               |d warm| <= C u bound_a
               |d qvel| <= 2 u |qvel| + h C u bound_euler
               |d qpos| <= 2 u |qpos| + h (bound of d qvel)        (the quaternion: the largest angular bound of d qvel, and 8 u added)
             C_FP32 is DERIVED, by counting the roundings along the longest chain of dynamics_rows, make_constraints and the Cholesky solves as
             written (docs/kernels.md, "How the smooth dynamics and the contact-free solve are checked"); no kernel output sets or adjusts it.

A state is decidable when the oracle's active set (efc_type, the row's joint and sign, efc_force != 0) is the same with every limited joint of
the state moved by +-1e-6.  On an undecidable state an output passes if it meets the bound against the reference, or lies between the references
of the moved states widened by their bounds (whichever active set the oracle has there)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import ko_py as ko
from tests import dynamics_states as ds

U = 2.0 ** -24
# roundings made on each term of the bound along the longest chain of the code as written (docs/kernels.md has the count): on |H| |qacc| 26 into an
# entry of M (R7 -> Rb -> Rp -> Rb -> Rd -> rDD -> rDP -> jDp -> m dot(jDp, jDp) -> the sum of five) + 3 forming H + 28 of the Cholesky solve of
# the 9 x 9 hand block (3 n + 1) + 9 + 1 of the gradient's row product and its - qs + 2 of a += alpha p = 69; on the forces 30 + 6; on the rows'
# |D aref| 24.  The largest.
C_FP32 = 69
FP64 = dict(qpos=1e-9, qvel=1e-7, warm=1e-9)

Ref = namedtuple("Ref", "qpos qvel qacc qacc_smooth ncon nefc efc_type efc_J efc_R efc_aref efc_force M bias passive actuator converged iters ctrl h damping weight con_geom con_dist con_pos con_mu con_margin con_force", defaults=(None,) * 6)   # con_*: per contact of the step's forward pass (geom pair, dist, pos, mu of the two tangents, margin, force in its frame)


def step_ctrl(shape, hq, qpos, action):
    """the controls ks_step forms from an action: ko_env_ctrl at the oracle's palm pose"""
    o = ds.oracle_sim(shape, hq)
    o.set_state(qpos, np.zeros(15), np.zeros(15))
    o.forward()
    return ko.env_ctrl(o.view("geom_xpos").reshape(-1, 3)[1], o.view("geom_xmat").reshape(-1, 9)[1], action)[2]


def oracle_step(shape, hq, mass, qpos, qvel, warm, ctrl) -> Ref:
    o = ds.oracle_sim(shape, hq)
    M = ds.model(shape)
    o.s.obj_mass = mass
    o.set_state(qpos, qvel, warm)
    o.view("ctrl")[:] = ctrl
    try:
        o.step()
    finally:
        o.s.obj_mass = 0.0
    n = o.s.nefc
    v = lambda k: o.view(k).copy()
    cs = [o.s.contact[i] for i in range(o.s.ncon)]
    con = (np.array([(c.geom1, c.geom2) for c in cs], dtype=int).reshape(-1, 2), np.array([c.dist for c in cs]), np.array([c.pos[:] for c in cs]).reshape(-1, 3),
           np.array([c.mu[:2] for c in cs]).reshape(-1, 2), np.array([c.margin for c in cs]), o.contact_forces())
    return Ref(v("qpos"), v("qvel"), v("qacc"), v("qacc_smooth"), int(o.s.ncon), n, v("efc_type")[:n], v("efc_J").reshape(-1, 15)[:n], v("efc_R")[:n],
               v("efc_aref")[:n], v("efc_force")[:n], v("M").reshape(15, 15), v("qfrc_bias"), v("qfrc_passive"), v("qfrc_actuator"),
               int(o.s.newton_converged), int(o.s.newton_iters_used), np.array(ctrl, dtype=np.float64), float(M["opt"][0]), np.asarray(M["dof_damping"], dtype=np.float64),
               weight(M, mass, o.view("M").reshape(15, 15), np.asarray(qvel, dtype=np.float64)), *con)


def weight(M, obj_mass, Mm, qvel):
    """W + V: majorants of the generalized force of the bodies' weight and of their velocity-product (centripetal, gyroscopic) forces on every
    joint, WHATEVER the pose.  |qfrc_bias| alone misses them where these forces cancel in the projection onto the joint: the `normal` hand's
    horizontal slides stand 8e-4 off the horizontal and carry 6e-3 N of the hand's 7.8 N, but the entry of the rotation matrix that the 6e-3 N
    are formed with has an ABSOLUTE error of u, i.e. u times the whole weight; a link's centripetal force passes through its own axis.
    With I_i = M_ii - armature_i (the bodies' part of the diagonal), m_i the mass that joint i carries and Cauchy-Schwarz,
      W_i = g sum_b m_b |J_b,i| <= g sqrt(m_i I_i)
      V_i = sum_b m_b |a_b| |J_b,i| <= w_f^2 sqrt(I_pp I_i)     finger f: |a_b| <= w_f^2 (|t| + |r_b|), w_f = |qvel_p| + |qvel_d|, I_pp of its proximal joint
      slides: V_i <= sum_f w_f^2 sqrt(I_pp m_f);  object (spin w, I_s the sum of its three angular I_i >= 2 m |c|^2):  linear w^2 sqrt(m I_s / 2), angular w^2 I_s"""
    bm = np.asarray(M["body_mass"], dtype=np.float64)
    I = np.diag(Mm) - np.asarray(M["dof_armature"], dtype=np.float64)
    m, V = np.zeros(15), np.zeros(15)
    m[0:3] = bm[2:9].sum()
    for f in range(3):
        p, d = 3 + 2 * f, 4 + 2 * f
        m[p], m[d] = bm[p] + bm[d], bm[d]
        w2 = (abs(qvel[p]) + abs(qvel[d])) ** 2
        V[p], V[d] = w2 * I[p], w2 * np.sqrt(I[p] * I[d])
        V[0:3] += w2 * np.sqrt(I[p] * m[p])
    m[9:15] = obj_mass
    w2, Is = float(qvel[12:15] @ qvel[12:15]), I[12:15].sum()
    V[9:12], V[12:15] = w2 * np.sqrt(obj_mass * Is / 2), w2 * Is
    return abs(float(M["opt"][2])) * np.sqrt(m * I) + V


def controls(s: ds.States, mode, i):
    """mode "substep": the state's own controls; "step": those the env layer forms from the state's action (fp64: the kernel forms its own in fp32)"""
    return s.ctrl[:, i] if mode == "substep" else step_ctrl(s.shape, s.hq[:, i], s.qpos[:, i], s.action[:, i])


_refs = {}


def reference(s: ds.States, mode="substep"):
    key = (s.cls, s.shape, mode)
    if key not in _refs:
        _refs[key] = [oracle_step(s.shape, s.hq[:, i], s.mass[i], s.qpos[:, i], s.qvel[:, i], s.warm[:, i], controls(s, mode, i)) for i in range(len(s.tag))]
    return _refs[key]


# ---- the active set ----------------------------------------------------------------------------------------------------------------------
def active(ref: Ref):
    return (ref.efc_type == 0) | (ref.efc_force != 0)


def signature(ref: Ref):
    """the active set: per row its type, joint, sign and whether it carries force"""
    return tuple((int(t), int(np.argmax(np.abs(J))), float(np.sign(J[np.argmax(np.abs(J))])), bool(f != 0)) for t, J, f in zip(ref.efc_type, ref.efc_J, ref.efc_force))


def limited_joints(tag):
    if "limit" not in tag:
        return ()
    return tuple(ds.LIMIT_DOF[j] for j, _, _, _ in tag[tag.index("limit") + 1])


_moved = {}


def moved_references(s: ds.States, mode, i):
    """the oracle at the state with each of its limited joints moved by +-MOVE (the inputs stay fp32 numbers)"""
    key = (s.cls, s.shape, mode, i)
    if key not in _moved:
        out = []
        for dof in limited_joints(s.tag[i]):
            for sgn in (-1, 1):
                q = s.qpos[:, i].copy()
                q[dof] = float(ds.f32(q[dof] + sgn * ds.MOVE))
                out.append(oracle_step(s.shape, s.hq[:, i], s.mass[i], q, s.qvel[:, i], s.warm[:, i], controls(s, mode, i)))
        _moved[key] = out
    return _moved[key]


def decidable(s: ds.States, mode, i):
    ref = reference(s, mode)[i]
    return all(signature(m) == signature(ref) for m in moved_references(s, mode, i))


# ---- the bounds --------------------------------------------------------------------------------------------------------------------------
def hessian(ref: Ref):
    a = active(ref)
    J, D = ref.efc_J[a], 1.0 / ref.efc_R[a]
    return ref.M + (J.T * D) @ J, J, D, ref.efc_aref[a]


def newton_residual(ref: Ref):
    """(|H a - rhs|_max, scale) of the oracle's own solution on the active set it reports"""
    H, J, D, aref = hessian(ref)
    smooth = ref.passive - ref.bias + ref.actuator
    rhs = smooth + J.T @ (D * aref)
    scale = np.abs(H) @ np.abs(ref.qacc) + np.abs(smooth) + np.abs(J).T @ np.abs(D * aref)
    return float(np.abs(H @ ref.qacc - rhs).max()), float(scale.max())


def raw_bounds(ref: Ref):
    """(bound_a, bound_euler): the factors that C u multiplies"""
    H, J, D, aref = hessian(ref)
    forces = np.abs(ref.bias) + np.abs(ref.passive) + np.abs(ref.actuator) + ref.weight
    ba = np.abs(np.linalg.inv(H)) @ (np.abs(H) @ np.abs(ref.qacc) + forces + np.abs(J).T @ np.abs(D * aref))
    Md = ref.M + ref.h * np.diag(ref.damping)
    f = ref.passive - ref.bias + ref.actuator + ref.efc_J.T @ ref.efc_force
    qa = np.linalg.solve(Md, f)
    # the rows' forces are formed from the solver's qacc: its error, c u bound_a, enters the Euler solve through |J_act|^T D |J_act|
    be = np.abs(np.linalg.inv(Md)) @ (np.abs(Md) @ np.abs(qa) + forces + np.abs(J).T @ (D * (np.abs(J) @ (np.abs(ref.qacc) + ba) + np.abs(aref))))
    return ba, be


def bounds(ref: Ref, precision, c=C_FP32):
    """{output: componentwise bound}"""
    if precision == 64:
        return dict(qpos=np.full(16, FP64["qpos"]), qvel=np.full(15, FP64["qvel"]), warm=np.full(15, FP64["warm"] * (1 + np.abs(ref.qacc).max())))
    ba, be = raw_bounds(ref)
    ba, be = ba + c * U * ba.max(), be + c * U * be.max()          # second order: what a first-order bound drops couples the components normwise
    bv = 2 * U * np.abs(ref.qvel) + ref.h * c * U * be
    bq = 2 * U * np.abs(ref.qpos)
    bq[:12] += ref.h * bv[:12]
    bq[12:] += ref.h * bv[12:].max() + 8 * U
    return dict(qpos=bq, qvel=bv, warm=c * U * ba)


def first_form_bounds(ref: Ref, c=C_FP32):
    """the fp32 bound in its first form - F without W and V, the rows' force as |efc_force|, no second-order term - RECORDED beside the bound
    that is asserted, to show what the added terms cost; components whose first-form bound is 0 (exact zeros of the reference) are counted apart"""
    H, J, D, aref = hessian(ref)
    forces = np.abs(ref.bias) + np.abs(ref.passive) + np.abs(ref.actuator)
    ba = np.abs(np.linalg.inv(H)) @ (np.abs(H) @ np.abs(ref.qacc) + forces + np.abs(J).T @ np.abs(D * aref))
    Md = ref.M + ref.h * np.diag(ref.damping)
    qa = np.linalg.solve(Md, ref.passive - ref.bias + ref.actuator + ref.efc_J.T @ ref.efc_force)
    be = np.abs(np.linalg.inv(Md)) @ (np.abs(Md) @ np.abs(qa) + forces + np.abs(ref.efc_J).T @ np.abs(ref.efc_force))
    bv = 2 * U * np.abs(ref.qvel) + ref.h * c * U * be
    bq = 2 * U * np.abs(ref.qpos)
    bq[:12] += ref.h * bv[:12]
    bq[12:] += ref.h * bv[12:].max() + 8 * U
    return dict(qpos=bq, qvel=bv, warm=c * U * ba)


def ratios(ref: Ref, got, precision, first_form=False):
    """{output: (worst |got - ref| / bound, its component)}; got: dict(qpos, qvel, warm)"""
    b = first_form_bounds(ref) if first_form else bounds(ref, precision)
    want = dict(qpos=ref.qpos, qvel=ref.qvel, warm=ref.qacc)
    out = {}
    for k in ("qpos", "qvel", "warm"):
        err = np.abs(np.asarray(got[k], dtype=np.float64) - want[k])
        r = np.where(err > 0, err / np.where(b[k] > 0, b[k], 1e-300), 0.0)
        j = int(np.argmax(r))
        out[k] = (float(r[j]), j)
    return out


def between(refs, got, precision, bounds_of=None):
    """an undecidable state: every output lies between the references of the moved states, widened by their bounds (bounds_of(ref, precision):
    another bound than `bounds`, tests/contact_solve_ref.py)"""
    want = lambda r: dict(qpos=r.qpos, qvel=r.qvel, warm=r.qacc)
    bs = [(bounds_of or bounds)(r, precision) for r in refs]
    for k in ("qpos", "qvel", "warm"):
        lo = np.min([want(r)[k] - b[k] for r, b in zip(refs, bs)], 0)
        hi = np.max([want(r)[k] + b[k] for r, b in zip(refs, bs)], 0)
        g = np.asarray(got[k], dtype=np.float64)
        if not ((g >= lo) & (g <= hi)).all():
            return False
    return True


class Tally:
    """one (class, shape, path) against the reference: worst ratios, failures named by class, state, output, component and ratio"""

    def __init__(self, s: ds.States, mode, precision, path):
        self.s, self.mode, self.precision, self.path = s, mode, precision, path
        self.worst = dict(qpos=0.0, qvel=0.0, warm=0.0)
        self.first = dict(qvel=[], warm=[])                  # per state (ratio to the bound's first form, error on a component it bounds by 0): recorded, not asserted
        self.failures, self.n, self.undecided = [], 0, 0

    def add(self, i, got, ncon=0, status=0):
        s, ref = self.s, reference(self.s, self.mode)[i]
        self.n += 1
        if ncon != 0 or status != 0:
            self.failures.append((s.cls, i, "ncon / status", int(ncon), int(status)))
        if not all(np.isfinite(np.asarray(got[k], dtype=np.float64)).all() for k in ("qpos", "qvel", "warm")):
            return self.failures.append((s.cls, i, "not finite"))
        r = ratios(ref, got, self.precision)
        scale = 1.0 if self.precision == 64 else C_FP32
        bad = {k: v for k, v in r.items() if v[0] > 1.0}
        if bad and limited_joints(s.tag[i]) and not decidable(s, self.mode, i):
            self.undecided += 1
            if between([ref] + moved_references(s, self.mode, i), got, self.precision):
                return
        for k, (x, j) in r.items():
            self.worst[k] = max(self.worst[k], x * scale)
        if self.precision == 32:
            b1, want = first_form_bounds(ref), dict(qpos=ref.qpos, qvel=ref.qvel, warm=ref.qacc)
            for k in ("qvel", "warm"):
                err = np.abs(np.asarray(got[k], dtype=np.float64) - want[k])
                pos = b1[k] > 0
                self.first[k].append((float((err[pos] / b1[k][pos]).max()) * scale, bool((err[~pos] > 0).any())))
        for k, (x, j) in bad.items():
            self.failures.append((s.cls, i, k, j, f"{x:.3g} x the bound", s.tag[i]))

    def check(self):
        assert not self.failures, (self.path, self.s.shape, len(self.failures), self.failures[:6])

    def line(self):
        unit = "of the fp64 figure" if self.precision == 64 else "c (derived %d)" % C_FP32
        line = (f"{self.s.cls:13s} {self.s.shape:8s} {self.path:24s} states {self.n:4d} worst qpos {self.worst['qpos']:8.3g} qvel {self.worst['qvel']:8.3g} "
                f"warm {self.worst['warm']:8.3g} {unit}; set aside as undecidable {self.undecided}; failures {len(self.failures)}")
        if self.precision == 32 and self.first["qvel"]:
            w = lambda k: max(x for x, _ in self.first[k])
            over = lambda k: sum(x > C_FP32 for x, _ in self.first[k])
            zero = lambda k: sum(z for _, z in self.first[k])
            line += (f"\n{'':13s} {'':8s} {'against the first form':24s} worst qvel {w('qvel'):8.3g} warm {w('warm'):8.3g} c on the components it bounds; states above {C_FP32}: "
                     f"qvel {over('qvel')} warm {over('warm')}; states with an error on a component it bounds by 0: qvel {zero('qvel')} warm {zero('warm')}")
        return line


# ---- the conditions on the inputs --------------------------------------------------------------------------------------------------------
def share_over_bound(s: ds.States, i, mode="substep"):
    """(the aimed term's share of the one-substep change of qvel over the fp32 bound of qvel, on the component where that is largest; whether the
    state aims at the term at all).  free_flight, finger_swing: h M^-1 (qfrc_bias(v) - qfrc_bias(0)); tendon: h M^-1 J^T f of the finger's
    row; limits: of the limit rows (aimed where the oracle has one active); actuator: h M^-1 of what the clamp takes off (aimed beyond the clamp);
    warm_start aims at no term."""
    ref = reference(s, mode)[i]
    bv = bounds(ref, 32)["qvel"]
    Minv = np.linalg.inv(ref.M)
    tag = s.tag[i]
    if s.cls in ("free_flight", "finger_swing"):
        rest = oracle_step(s.shape, s.hq[:, i], s.mass[i], s.qpos[:, i], np.zeros(15), np.zeros(15), ref.ctrl)
        share = ref.h * Minv @ (ref.bias - rest.bias)
    elif s.cls == "tendon":
        f = tag[tag.index("finger") + 1]
        share = ref.h * Minv @ (ref.efc_J[f] * ref.efc_force[f])
    elif s.cls in ds.LIMIT_CLASSES:
        rows = (ref.efc_type == 1) & (ref.efc_force != 0)
        if not rows.any():
            return 0.0, False
        share = ref.h * Minv @ (ref.efc_J[rows].T @ ref.efc_force[rows])
    elif s.cls == "actuator":
        k, x = tag[tag.index("ctrl") + 1], tag[tag.index("x") + 1]
        if abs(x) < 1.5 or (k < 6 and k % 2 == 1):
            return 0.0, False
        A = ds.model(s.shape)["actuator"]
        frc = np.zeros(15)
        if k < 6:
            frc[k // 2] = A[0] * (ref.ctrl[k] - np.clip(ref.ctrl[k], -A[2], A[2]))
        else:
            frc[3 + 2 * (k - 6)] = A[3] * (ref.ctrl[k] - np.clip(ref.ctrl[k], -A[4], A[4]))
        share = ref.h * Minv @ frc
    else:
        return 0.0, False
    return float((np.abs(share) / bv).max()), True


def conditions(s: ds.States, mode="substep"):
    """dict(drop share, undecidable share, aimed states, share of the aimed states that carry the term at 100 x the fp32 bound, its median)"""
    n = len(s.tag)
    und = [i for i in range(n) if limited_joints(s.tag[i]) and not decidable(s, mode, i)]
    sh = [share_over_bound(s, i, mode) for i in range(n)]
    aimed = np.array([x for x, a in sh if a])
    return dict(n=n, dropped=ds.drop_share(s.cls, s.shape), redrawn=ds.redraws(s.cls, s.shape), undecidable=len(und) / n, aimed=len(aimed),
                carried=float((aimed >= 100).mean()) if len(aimed) else float("nan"), median=float(np.median(aimed)) if len(aimed) else float("nan"))
