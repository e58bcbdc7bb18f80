"""Reference and bounds for the floor-contact states of tests/contact_solve_states.py, built on tests/dynamics_ref.py.  The reference is the oracle
itself (dynamics_ref.oracle_step: one ko_step from the state, its forward pass, its contact list and OracleSim.contact_forces()); nothing here
looks at a kernel's solve.

fp64 paths   dynamics_ref.FP64 as it is (qpos 1e-9, qvel 1e-7, qacc_warmstart 1e-9 (1 + |qacc|_max)); the tap's contact forces 1e-6 of the
             state's largest force (the figure of tests/test_gpu_obs_contacts.py; floor 1e-3 N).
fp32 paths   u = 2^-24, `act` = equalities and rows with force, f = D (J a - aref) on them, G = H^-1 J^T D, G2 = Md^-1 J^T D kept as SIGNED
             matrices (cond(H) is 1e4 on a contact: |H^-1| |H| |qacc| would swallow the contact forces):
               bound_a     = |H^-1| (69 |M| |a| + 36 F + c_f |J|^T |f|) + 47 |G| row                     row = |J| |a| + |aref|, c_f = 100 + ncon
               bound_euler = |Md^-1| (69 |Md| |qa| + 36 F + (34 + ncon) |J|^T |f|) + 12 (|G2| + |G2 J| |G|) row
                             + |Md^-1 M| (35 |G| row + 65 |H^-1| |J|^T |f|) + |G2 J| |H^-1| (69 |M| |a| + 36 F + c_f |J|^T |f|)
                             (the issue's form |Md^-1| (..) + |G2| row + |G2 J| bound_a with each term's own count of roundings, and with what
                             solver and final forces share - basis, aref, D - sent through Md^-1 M G = G2 (I - J G): see raw_bounds)
               |d warm|  <= u bound_a + 1e-5 (1 + |a|_max + |p|_max) + 28 u |H^-1| |H| |p|,  p = a - a_start      (`solver_term`)
               |d qvel|  <= 2 u |qvel| + h u bound_euler
               |d qpos|  <= 2 u |qpos| + h (bound of d qvel)           (the quaternion as in dynamics_ref)
               |d f_e|   <= D_e (|J_e| u bound_a + 47 u (|J_e| |a| + |aref_e|)) + 43 u |f_e|   per pyramid edge with force, composed as contact_forces
                            composes the edges: normal = the sum of the four, tangent k = mu_k x (the sum of its two)
             each with the second-order term c u max(bound) of dynamics_ref.  F as there (with W and V).
             c = 100 + ncon, DERIVED by counting roundings (contact_c; docs/kernels.md, "How the contact solve is checked").
geometry     an fp32 path's contact records differ from the oracle's in dist and pos by what tests/test_gpu_plane_contacts.py allows (2e-6, 1e-4;
             measured 1.2e-7, 1.1e-7).  Each tapped record is held to those bounds, to the oracle's pair and to the normal (0, 0, 1) exactly;
             the measured differences are then carried to first order through the REFERENCE's H, J, D (`geometry_term`) and added to the bounds.
             The term uses the kernel's geometry, which is pinned elsewhere, never its solve.

A state is decidable when the set of force-carrying rows (and ncon) of the oracle is the same with whatever stands on the floor moved by +-MOVE_Z
along z (the object's z; the hand's most vertical slide) and with qvel scaled by 1 +- SCALE_V.  An undecidable state is not skipped: every output
must meet the bound against the reference or lie between the references of the moved states widened by their bounds (dynamics_ref.between)."""
from __future__ import annotations

import numpy as np

from oracle import ko_py as ko
from tests import contact_solve_states as cs, dynamics_ref as dr, dynamics_states as ds

U = dr.U
LS_RTOL = 1e-5            # ks_core.h: LS_RTOL<float>()
FORCE_FP64 = 1e-6
FORCE_FLOOR = 1e-3
GEOM = dict(dist=2e-6, pos=1e-4)          # the plane tests' fp32 bounds (fp64: contact_poses.BOUNDS[64])
GEOM64 = dict(dist=1e-9, pos=1e-9)
SHARE_FACTOR, SHARE_CAP, AIMED_MIN = 100.0, 0.90, 30


C_M, C_F, C_D, C_COMMON, C_FRESH, C_SOLVE = dr.C_FP32, 36, 43, 35, 12, 28
C_ROW = C_COMMON + C_FRESH


def contact_c(ref: dr.Ref):
    """c_f, the roundings on |J|^T |f| along the longest chain of the contact code as written (one per + - * /, an n-term sum n, a cross-product
    component 2): C_D = 43 into D xx (impedance on dist - margin leaves an absolute 1.3 u in imp, which 1 - imp >= 0.05 turns into 26; / imp 2;
    diag = (w + mu mu w) 2 mu mu / impratio with w = invw + wobj 11; x diag 1; 1 / R 1; D xx 1) + 3 (the sum of the four edges) + 21 into an entry
    of the basis (the body chain R7 -> .. -> rDD 15, pos - p 1, cross 2, the frame's 3-term product 3) + 3 (b0 gn + b1 gt1 + b2 gt2) + ncon (the
    gradient adds one term per contact) + 28 (the Cholesky solve of the 9 x 9 hand block) + 2 (a += alpha p) = 100 + ncon.
    The other terms of the bound carry their own counts: |M| |a| C_M = 69 and F C_F = 36 as in the contact-free solve (dynamics_ref); the row
    residual |J| |a| + |aref| C_ROW = C_COMMON + C_FRESH = 47: computed once per substep and shared by every evaluation are the basis (22 on the
    object: 16 into an entry of R from the normalised quaternion, pos - p 1, cross 2, the frame 3; 21 on a distal link) and aref (22 + 9 into vb -
    a floor contact touches 6 or 9 columns, the zeros add exactly -, mu x, +, x b, + base: C_COMMON = 35), fresh at every evaluation the row
    product and xb0 +- mu xb1 - aref (C_FRESH = 9 + 2 + 1).  The way of the residual on through D, J^T and the solve is counted in c_f."""
    return 100 + ref.ncon


# ---- references --------------------------------------------------------------------------------------------------------------------------
def reference(s: ds.States, mode="substep"):
    return dr.reference(s, mode)


def rows(ref: dr.Ref):
    """(first efc row of every contact or -1, contact rows mask): a contact within its margin has four pyramid rows, in contact order"""
    first = np.full(ref.ncon, -1)
    r = int((ref.efc_type != 2).sum())
    for k in range(ref.ncon):
        if ref.con_dist[k] < ref.con_margin[k]:
            first[k] = r
            r += 4
    assert r == ref.nefc
    return first, ref.efc_type == 2


def signature(ref: dr.Ref):
    """the scalar rows' signature of dynamics_ref, ncon, and per contact row whether it carries force"""
    c = ref.efc_type == 2
    sub = ref._replace(efc_type=ref.efc_type[~c], efc_J=ref.efc_J[~c], efc_force=ref.efc_force[~c])
    return dr.signature(sub), ref.ncon, tuple(bool(f != 0) for f in ref.efc_force[c])


def aimed(ref: dr.Ref):
    return bool((ref.efc_force[ref.efc_type == 2] != 0).any())


_moved = {}


def moved_references(s: ds.States, mode, i):
    """the oracle at the state with what stands on the floor moved by +-MOVE_Z along z and with qvel scaled by 1 +- SCALE_V (inputs stay fp32)"""
    key = (s.cls, s.shape, mode, i)
    if key not in _moved:
        ref = reference(s, mode)[i]
        out, step = [], lambda q, v: dr.oracle_step(s.shape, s.hq[:, i], s.mass[i], q, v, s.warm[:, i], dr.controls(s, mode, i))
        moves = []
        if (ref.con_geom[:, 1] >= 8).any():
            moves.append((11, 1.0))
        if (ref.con_geom[:, 1] < 8).any():
            D = ds.slide_dirs(s.tag[i][0])[0]
            j = int(np.argmax(np.abs(D[:, 2])))
            moves.append((j, 1.0 / D[j, 2]))
        for dof, scale in moves:
            for sgn in (-1, 1):
                q = s.qpos[:, i].copy()
                q[dof] = q[dof] + sgn * cs.MOVE_Z * scale
                out.append(step(q, s.qvel[:, i]))
        for f in (1 - cs.SCALE_V, 1 + cs.SCALE_V):
            out.append(step(s.qpos[:, i], s.qvel[:, i] * f))
        _moved[key] = out
    return _moved[key]


def decidable(s: ds.States, mode, i):
    sig = signature(reference(s, mode)[i])
    return all(signature(m) == sig for m in moved_references(s, mode, i))


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------
def ingredients(ref: dr.Ref):
    H, J, D, aref = dr.hessian(ref)
    Hi = np.linalg.inv(H)
    Md = ref.M + ref.h * np.diag(ref.damping)
    Mi = np.linalg.inv(Md)
    a = ref.qacc
    f = D * (J @ a - aref)
    forces = np.abs(ref.bias) + np.abs(ref.passive) + np.abs(ref.actuator) + ref.weight
    qa = Mi @ (ref.passive - ref.bias + ref.actuator + ref.efc_J.T @ ref.efc_force)
    return dict(H=H, J=J, D=D, aref=aref, Hi=Hi, Md=Md, Mi=Mi, a=a, f=f, F=forces, qa=qa, G=Hi @ (J.T * D), G2=Mi @ (J.T * D), act=dr.active(ref))


def inputs(s: ds.States, i):
    """what the bounds take from the state itself: its qvel (a contact row's aref by its two parts), its qacc_warmstart (`solver_term`), and the
    row constant b of aref = -b J v - k imp r"""
    return dict(qvel=s.qvel[:, i], warm=s.warm[:, i], b=ds.constants(ds.model(s.shape))["b"])


def raw_bounds(ref: dr.Ref, g=None, inp=None):
    """(bound_a, bound_euler), each term with its own count of roundings inside (u multiplies the result).  A contact row's aref = -b J v - k imp r is
    a difference - an object leaving the floor at 1 m/s holds b v = 526 against k imp r = 8 - and |aref| alone misses what cancels in it: with
    the state's qvel given, the row takes |b J v| + |aref + b J v|."""
    g = g or ingredients(ref)
    J, a, f = g["J"], g["a"], g["f"]
    aref = np.abs(g["aref"])
    if inp is not None:
        bv = inp["b"] * (J @ np.asarray(inp["qvel"], dtype=np.float64))
        con = ref.efc_type[g["act"]] == 2
        aref = np.where(con, np.abs(bv) + np.abs(g["aref"] + bv), aref)
    cf = contact_c(ref)
    row = np.abs(J) @ np.abs(a) + aref
    Jf = np.abs(J).T @ np.abs(f)
    rest = np.abs(g["Hi"]) @ (C_M * (np.abs(ref.M) @ np.abs(a)) + C_F * g["F"] + cf * Jf)
    ba = rest + np.abs(g["G"]) @ (C_ROW * row)
    # qvel: what is computed ONCE and used by the solver and by the final forces alike (the basis, aref, D: C_COMMON on the residual, C_D + 22 on
    # the force) reaches qvel through Md^-1 M H^-1 J^T D, not through Md^-1 J^T D: the solver's a absorbs it,
    #   G2 (I - J G) = Md^-1 (I - J^T D J H^-1) J^T D = Md^-1 M G
    # Fresh at every evaluation are only the row products (C_FRESH = 9 + 2 + 1) and the last J^T f with the Euler solve (3 + 3 + ncon + 28).
    MiM = np.abs(g["Mi"] @ ref.M)
    be = (np.abs(g["Mi"]) @ (C_M * (np.abs(g["Md"]) @ np.abs(g["qa"])) + C_F * g["F"] + (6 + ref.ncon + C_SOLVE) * Jf)
          + (np.abs(g["G2"]) + np.abs(g["G2"] @ J) @ np.abs(g["G"])) @ (C_FRESH * row)
          + MiM @ (np.abs(g["G"]) @ (C_COMMON * row) + np.abs(g["Hi"]) @ ((C_D + 22) * Jf))
          + np.abs(g["G2"] @ J) @ rest)
    return ba, be


NEWTON_TOL = 1e-5         # ks_core.h: the Newton loop ends on a step below 1e-5 (1 + |a|_max)


def solver_term(ref: dr.Ref, warm_in, g):
    """What the solver's stopping rules leave in qacc_warmstart:
        1e-5 (1 + |a|_max + |p|_max)  on every component   +   C_SOLVE u |H^-1| |H| |p|,       p = a - a_start
    The Newton loop ends on a step below NEWTON_TOL (1 + |a|_max), or - without a confirming iteration - after a step on which no row changed
    sides.  That step is taken with a step length the line search knows to LS_RTOL = 1e-5 of itself (168 u), and along a direction H^-1 g whose
    Cholesky solve keeps its own error, C_SOLVE u |H^-1| |H| |p| with the WHOLE |H| = |M| + |J|^T D |J|: cond(H) is 1e4 on a contact, and the soft
    directions (an object turning about its contact point) take 1e-3 rad/s^2 of it.  Its size |p| is bounded by the way from the start, a_start =
    the cheaper of the state's qacc_warmstart and qacc_smooth (`starts`).  Measured on the host lane: a tilted cube 3 mm in the floor
    ends 1.3e-3 off in its angular acceleration from qacc_smooth, 1.6e-4 from zero and 5e-7 when started from the solution (rounding term 1e-4).
    The first part is normwise: a component that ends where it started (the acceleration across a sliding contact whose active edges do not
    touch it) has moved on the way, while other edges were active, and keeps 1e-5 of that swing - 6e-5 on a component whose rounding bound is
    2e-5.  The error lies where the cost is flat: the rows' forces and qvel do not take the term (measured: below 0.3 of their bounds without it)."""
    a = ref.qacc
    p = np.max([np.abs(a - x) for x in starts(ref, warm_in)], 0)
    return max(LS_RTOL, NEWTON_TOL) * (1 + np.abs(a).max() + p.max()) + C_SOLVE * U * (np.abs(g["Hi"]) @ (np.abs(g["H"]) @ p))


def start_cost(ref: dr.Ref, x):
    """the cost the warm-start choice compares: the Gauss term about qacc_smooth and every row's 1/2 D r^2 (an equality always, another row where
    r = J x - aref < 0)"""
    d = x - ref.qacc_smooth
    r = ref.efc_J @ x - ref.efc_aref
    on = (ref.efc_type == 0) | (r < 0)
    return 0.5 * d @ ref.M @ d + 0.5 * float(((r * r / ref.efc_R)[on]).sum())


def starts(ref: dr.Ref, warm_in):
    """where the solver starts: the cheaper of the state's qacc_warmstart and qacc_smooth (the kernel's rule, `cw < cs`); both where the two costs
    agree to 1e-6 (rounding may decide).  The bound follows the RIGHT choice: a solver that starts from the dearer one is held to the cheaper one's."""
    w = np.asarray(warm_in, dtype=np.float64)
    cw, c0 = start_cost(ref, w), start_cost(ref, ref.qacc_smooth)
    if abs(cw - c0) <= 1e-6 * max(cw, c0):
        return [w, ref.qacc_smooth]
    return [w] if cw < c0 else [ref.qacc_smooth]


def edge_bounds(ref: dr.Ref, bw, g, inp=None):
    """per contact [ncon, 3]: the bound of (normal, tangent 1, tangent 2) of the tap, from the edges with force"""
    first, _ = rows(ref)
    idx = np.flatnonzero(g["act"])
    pos = {int(r): k for k, r in enumerate(idx)}                 # efc row -> row of the active system
    J, D, a, aref, f = g["J"], g["D"], g["a"], np.abs(g["aref"]), g["f"]
    if inp is not None:
        bv = inp["b"] * (J @ np.asarray(inp["qvel"], dtype=np.float64))
        aref = np.abs(bv) + np.abs(g["aref"] + bv)
    out = np.zeros((ref.ncon, 3))
    for k in range(ref.ncon):
        if first[k] < 0:
            continue
        e = np.zeros(4)
        for kk in range(4):
            r = pos.get(int(first[k]) + kk)
            if r is not None:
                e[kk] = D[r] * (np.abs(J[r]) @ bw + C_ROW * U * (np.abs(J[r]) @ np.abs(a) + aref[r])) + C_D * U * abs(f[r])
        out[k] = [e.sum(), ref.con_mu[k, 0] * (e[0] + e[1]), ref.con_mu[k, 1] * (e[2] + e[3])]
    return out


def bounds(ref: dr.Ref, precision, inp=None, geometry=None):
    """{qpos, qvel, warm, force: componentwise bound}; inp: `inputs` of the state; geometry: the first-order term of `geometry_term` (fp32 paths)"""
    if precision == 64:
        b = dr.bounds(ref, 64)
        scale = max(FORCE_FLOOR, float(np.abs(ref.con_force).max()) if ref.ncon else 0.0)
        b["force"] = np.full((ref.ncon, 3), FORCE_FP64 * scale)
        return b
    c, g = contact_c(ref), ingredients(ref)
    ba, be = raw_bounds(ref, g, inp)
    ba, be = U * (ba + c * U * ba.max()), U * (be + c * U * be.max())
    bw = ba + solver_term(ref, np.zeros(15) if inp is None else inp["warm"], g)      # (qvel and the forces do not take it: see solver_term)
    bv = 2 * U * np.abs(ref.qvel) + ref.h * be
    bf = edge_bounds(ref, ba, g, inp)
    bf = bf + c * U * (bf.max() if bf.size else 0.0)
    if geometry is not None:
        bw, bv, bf = bw + geometry["warm"], bv + geometry["qvel"], bf + geometry["force"]
    bq = 2 * U * np.abs(ref.qpos)
    bq[:12] += ref.h * bv[:12]
    bq[12:] += ref.h * bv[12:].max() + 8 * U
    return dict(qpos=bq, qvel=bv, warm=bw, force=bf)


def check_records(ref: dr.Ref, con, ncon, precision):
    """the tapped records against the plane tests' bounds: None, or what is wrong.  con [ncon_max, 20]: pos 0:3, normal 3:6, dist 6, bodies 8"""
    if ncon != ref.ncon:
        return f"ncon {ncon} for {ref.ncon}"
    if ncon == 0:
        return None
    c = np.asarray(con, dtype=np.float64)[:ncon]
    B = GEOM if precision == 32 else GEOM64
    bodies = np.array([ko.GEOM_BODY[a] + 16 * ko.GEOM_BODY[b] for a, b in ref.con_geom])
    if not np.array_equal(c[:, 8].astype(int) & 255, bodies):
        return "pair list"
    if not np.array_equal(c[:, 3:6], np.tile([0.0, 0.0, 1.0], (ncon, 1))):
        return "normal is not (0, 0, 1)"
    dd, dp = np.abs(c[:, 6] - ref.con_dist).max(), np.abs(c[:, 0:3] - ref.con_pos).max()
    if dd > B["dist"] or dp > B["pos"]:
        return f"dist {dd:.2e} pos {dp:.2e}"
    return None


def first_order(ref: dr.Ref, g, dJ, daref, dDrel):
    """perturbations of the active rows (|dJ| [n, 15], |d aref| [n], |dD / D| [n]) carried to first order through the reference's H, J, D:
        H da = -(dJ^T f + J^T dD r + J^T D (dJ a - d aref)),   r = J a - aref
    -> dict(warm, qvel, force [ncon, 3])"""
    first, _ = rows(ref)
    pos = {int(r): n for n, r in enumerate(np.flatnonzero(g["act"]))}
    J, D, a, aref, f = g["J"], g["D"], g["a"], g["aref"], g["f"]
    da = np.abs(g["Hi"]) @ (dJ.T @ np.abs(f)) + np.abs(g["G"]) @ (dDrel * np.abs(J @ a - aref) + dJ @ np.abs(a) + daref)
    df_row = D * (np.abs(J) @ da + dJ @ np.abs(a) + daref) + dDrel * np.abs(f)
    dv = ref.h * (np.abs(g["Mi"]) @ (dJ.T @ np.abs(f)) + np.abs(g["G2"]) @ (dDrel * np.abs(J @ a - aref) + dJ @ np.abs(a) + daref) + np.abs(g["G2"] @ J) @ da)
    force = np.zeros((ref.ncon, 3))
    for kc in range(ref.ncon):
        if first[kc] < 0:
            continue
        e = np.array([df_row[pos[int(first[kc]) + kk]] if int(first[kc]) + kk in pos else 0.0 for kk in range(4)])
        force[kc] = [e.sum(), ref.con_mu[kc, 0] * (e[0] + e[1]), ref.con_mu[kc, 1] * (e[2] + e[3])]
    return dict(warm=da, qvel=dv, force=force)


ROT = np.array([0.0] * 3 + [1.0] * 6 + [0.0] * 3 + [1.0] * 3)      # the rotational dofs: a contact's lever arm enters their columns


def contact_rows(ref: dr.Ref, g):
    """[(contact, row of the active system)] of the pyramid edges with force"""
    first, _ = rows(ref)
    pos = {int(r): n for n, r in enumerate(np.flatnonzero(g["act"]))}
    return [(kc, pos[int(first[kc]) + kk]) for kc in range(ref.ncon) if first[kc] >= 0 for kk in range(4) if int(first[kc]) + kk in pos]


def geometry_term(ref: dr.Ref, con, M):
    """The difference between the tapped and the oracle's dist and pos, carried through `first_order`:
      |d aref_e| <= k (dmax + s |dist - margin|) |d dist|          s = 2 (dmax - dmin) / width: the steepest slope of impedance()
      |dD / D|   <= s |d dist| / (imp (1 - imp)) <= s |d dist| / (dmin (1 - dmax))
      |dJ_e,j|   <= (1 + mu) sqrt(3) |d pos|_inf on the rotational dofs (hinges, the object's angular rows), 0 on the translational ones"""
    g = ingredients(ref)
    k = ds.constants(M)
    s = 2 * (k["dmax"] - k["dmin"]) / k["width"]
    c = np.asarray(con, dtype=np.float64)[:ref.ncon]
    ddist, dpos = np.abs(c[:, 6] - ref.con_dist), np.abs(c[:, 0:3] - ref.con_pos).max(1) if ref.ncon else np.zeros(0)
    n = len(g["D"])
    daref, dDrel, dJ = np.zeros(n), np.zeros(n), np.zeros((n, 15))
    for kc, r in contact_rows(ref, g):
        rr = abs(ref.con_dist[kc] - ref.con_margin[kc])
        daref[r] = k["k"] * (k["dmax"] + s * rr) * ddist[kc]
        dDrel[r] = s * ddist[kc] / (k["dmin"] * (1 - k["dmax"]))
        dJ[r] = (1 + ref.con_mu[kc].max()) * np.sqrt(3.0) * dpos[kc] * ROT * (np.abs(g["J"][r]) > 0)
    return first_order(ref, g, dJ, daref, dDrel)


def between(refs, got, precision, inp):
    if not dr.between(refs, got, precision, bounds_of=lambda r, p: bounds(r, p, inp)):
        return False
    same = [r for r in refs if r.ncon == refs[0].ncon]             # (the kernel's ncon is the reference's: check_records)
    bs = [bounds(r, precision, inp)["force"] for r in same]
    lo = np.min([r.con_force - b for r, b in zip(same, bs)], 0)
    hi = np.max([r.con_force + b for r, b in zip(same, bs)], 0)
    return bool(((got["force"] >= lo) & (got["force"] <= hi)).all())


OUTPUTS = ("qpos", "qvel", "warm", "force")


class Tally(dr.Tally):
    """one (class, shape, path) against the reference.  Ratios are to the whole bound (rounding + geometry); `geom` records, per output, the largest
    share of the geometry term in a bound."""

    def __init__(self, s, mode, precision, path):
        super().__init__(s, mode, precision, path)
        self.worst = {k: 0.0 for k in OUTPUTS}
        self.geom = {k: 0.0 for k in ("qvel", "warm", "force")}
        self.whole = []                                          # per aimed state: the contact forces' share of qvel over the WHOLE bound asserted
        self.M = ds.model(s.shape)

    def add(self, i, got, ncon, status, con):
        """got: dict(qpos, qvel, warm); con [ncon_max, 20]: the tapped records with the forces in 14:17"""
        s, ref = self.s, reference(self.s, self.mode)[i]
        self.n += 1
        if status != 0:
            self.failures.append((s.cls, i, "status", int(status)))
        wrong = check_records(ref, con, ncon, self.precision)
        if wrong:
            return self.failures.append((s.cls, i, "records", wrong, s.tag[i]))
        got = dict(got, force=np.asarray(con, dtype=np.float64)[:ref.ncon, 14:17])
        if not all(np.isfinite(np.asarray(got[k], dtype=np.float64)).all() for k in OUTPUTS):
            return self.failures.append((s.cls, i, "not finite"))
        geo = geometry_term(ref, con, self.M) if self.precision == 32 and ref.ncon else None
        b = bounds(ref, self.precision, inputs(s, i), geo)
        want = dict(qpos=ref.qpos, qvel=ref.qvel, warm=ref.qacc, force=ref.con_force)
        if self.precision == 32 and aimed(ref):
            self.whole.append(share_over_bound(ref, bound=b["qvel"]))
        r = {}
        for k in OUTPUTS:
            err = np.abs(np.asarray(got[k], dtype=np.float64) - want[k]).ravel()
            bk = b[k].ravel()
            x = np.where(err > 0, err / np.where(bk > 0, bk, 1e-300), 0.0)
            j = int(np.argmax(x)) if x.size else 0
            r[k] = (float(x[j]) if x.size else 0.0, j)
            if geo is not None and k in geo and x.size:
                self.geom[k] = max(self.geom[k], float((geo[k].ravel() / np.where(bk > 0, bk, 1e-300)).max()))
        bad = {k: v for k, v in r.items() if v[0] > 1.0}
        if bad and not decidable(s, self.mode, i):
            self.undecided += 1
            if between([ref] + moved_references(s, self.mode, i), got, self.precision, inputs(s, i)):
                return
        for k, (x, j) in r.items():
            self.worst[k] = max(self.worst[k], x)
        for k, (x, j) in bad.items():
            self.failures.append((s.cls, i, k, j, f"{x:.3g} x the bound", f"ncon {ref.ncon}", s.tag[i]))

    def check(self):
        """as dynamics_ref.Tally.check; the message also names the contact counts of the failing states (a fault of the cache edge or of the lane deal
        shows as failures from one count on)"""
        counts = sorted({int(f[5][5:]) for f in self.failures if len(f) > 5 and isinstance(f[5], str) and f[5].startswith("ncon ")})
        assert not self.failures, (self.path, self.s.shape, len(self.failures), "contact counts of the failing states", counts, self.failures[:6])

    def line(self):
        unit = "of the fp64 figure" if self.precision == 64 else "of the bound"
        w = self.worst
        line = (f"{self.s.cls[8:]:15s} {self.s.shape:9s} {self.path:20s} states {self.n:4d} worst qpos {w['qpos']:7.3g} qvel {w['qvel']:7.3g} warm {w['warm']:7.3g} "
                f"force {w['force']:7.3g} {unit}; undecidable and between {self.undecided}; failures {len(self.failures)}")
        if self.precision == 32:
            w = np.array(self.whole) if self.whole else np.zeros(1)
            line += (f"; geometry term's largest share of a bound: qvel {self.geom['qvel']:.2f} warm {self.geom['warm']:.2f} force {self.geom['force']:.2f}; the contact forces over the WHOLE "
                     f"qvel bound, geometry included: {SHARE_FACTOR:.0f} x in {(w >= SHARE_FACTOR).mean():.3f}, 10 x in {(w >= 10).mean():.3f} of the aimed states (median {np.median(w):.3g} x, lowest {w.min():.3g} x)")
        return line


# ---- the conditions on the inputs --------------------------------------------------------------------------------------------------------
def basis(ref: dr.Ref, k):
    """(Jn, Jt1, Jt2) of contact k from its four pyramid rows J_n +- mu J_t"""
    r = rows(ref)[0][k]
    e, mu = ref.efc_J[r:r + 4], ref.con_mu[k]
    return 0.5 * (e[0] + e[1]), (e[0] - e[1]) / (2 * mu[0]), (e[2] - e[3]) / (2 * mu[1])


def share_over_bound(ref: dr.Ref, inp=None, tangential=False, bound=None):
    """what the contact forces (or their tangential part alone) do to qvel in one substep, over the fp32 bound of qvel, on the component where that
    is largest.  bound None: the rounding terms alone, which the reference knows; Tally passes the WHOLE bound of a path, geometry term included"""
    first, crow = rows(ref)
    if tangential:
        q = np.zeros(15)
        for k in range(ref.ncon):
            if first[k] >= 0:
                _, t1, t2 = basis(ref, k)
                q += t1 * ref.con_force[k, 1] + t2 * ref.con_force[k, 2]
    else:
        q = ref.efc_J[crow].T @ ref.efc_force[crow]
    Md = ref.M + ref.h * np.diag(ref.damping)
    return float((np.abs(ref.h * np.linalg.solve(Md, q)) / (bounds(ref, 32, inp)["qvel"] if bound is None else bound)).max())


def conditions(s: ds.States, mode="substep"):
    refs = reference(s, mode)
    n = len(refs)
    und = [i for i in range(n) if not decidable(s, mode, i)]
    sh = np.array([share_over_bound(r, inputs(s, i)) for i, r in enumerate(refs) if aimed(r)])
    return dict(n=n, dropped=cs.drop_share(s.cls[8:], s.shape), undecidable=len(und) / n, undecidable_states=und, aimed=len(sh),
                carried=float((sh >= SHARE_FACTOR).mean()) if len(sh) else float("nan"), carried10=float((sh >= 10).mean()) if len(sh) else float("nan"),
                median=float(np.median(sh)) if len(sh) else float("nan"), lowest=float(sh.min()) if len(sh) else float("nan"))
