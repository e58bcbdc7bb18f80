"""Reference, bound and decidability for the observation stage (build_obs of csrc/ks_obs.h; obs_write / obs_finish / wg_obs / k_obs of
csrc/ks_api.hip) on the snapshots of tests/obs_states.py.  Nothing here looks at a kernel's output.

reference   the oracle's env layer (oracle/ko_env.c through ko.env_obs_from_inputs / ko.env_reward) on the inputs that inputs_from_snapshot
            forms in float64 from the 105-value snapshot and the blob, with ONE restatement: slots 48-49 are atan2(|s|, y), not
            acos(y / sqrt(y^2 + s^2)) - the acos form loses 1e-16 / angle near zero (tests/test_obs_cpu.py holds the two to 1e-9 above 1e-6).
evaluate    the same arithmetic in vectorised numpy float64 on a packed input vector (snapshot, rays and the model constants that reach a
            slot), with every decision (palm-ray membership, a miss, the gravity axis `am`, the larger fan, the lift test) either taken
            from the inputs or forced.  It serves the partial derivatives of the bound and the "decision taken either way" references;
            tests/test_obs_cpu.py holds it to the oracle's C at 1e-12.
bound       fp32:  bound_j = c_j u (|y_j| + sum_k |dy_j/dx_k| |x_k|) + (c_j u)^2 max_j(...),  u = 2^-24, x = the packed inputs (the constants
            count: Model<float> rounds them), partials by central differences at two step sizes with the decisions held; where the two
            sums differ by more than 1 % the slot of that state is not smooth.  c_j is the number of roundings along the longest chain
            into the slot of build_obs as written (C_GROUP below; docs/kernels.md has the count).  Two terms that the partials cannot
            see are added (the host lane missed the first form of the bound on exactly these slots; docs/kernels.md):
              slots 70-72  a palm site and the wrist are both formed from the hand's origin p7, which cancels in their difference - the
                           partial with respect to p7 is zero, but the two sums are rounded at the size of p7:
                           u |T3| (4 A + 7 B), A and B the majorants of the site's and the wrist's sums
              slots 75-81  d of dot_product20 is a cosine: at d = 1 it is stationary in every input, but the C_D = 10 roundings of the two
                           normalisations, the two quotients each, the product and the sum scale d itself: 20 C_D u |y|
            fp64:  1e-9 (1 + |ref|) on every slot.  Exact slots (EXACT) carry no bound; reward, done and info are exact.
in-step     a stepping kernel forms the snapshot itself, in fp32: its kinematic error e_k reaches slot j as sum_k |dy_j/dx_k| e_k over the
            snapshot's entries (Bound.kin, added to the fp32 bound by the in-step tests).  e_k = C_KIN u for an entry of a rotation matrix
            (absolute: the entries are at most 1) and C_KIN u max|p| for a body origin's coordinates; C_KIN = 16 is the chain into a distal
            link's rotation - the hand's matrix from its quaternion 4, then R7 -> Rb -> Rp -> Rb -> Rd, 3 each, the chain that the dynamics
            section of docs/kernels.md counts - and covers the origin's (slides 6, two links 4 each, the parent rotation's error on a 5 cm
            offset).  The jointpos sensors are copies of qpos.
decidable   lift: |z - 0.195| beyond 8 u (|po_z| + |Ro_z.| . |geom_pos[8]|); palm ray: not equal to 0.06f; am: the two largest |g| more than
            8 u apart; fan: |total1 - total2| beyond the sum of the two totals' bounds."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import ko_py as ko

U = 2.0 ** -24
NOBS, NRAY, NSNAP = 82, 17, 105
T1, T2 = 82, 83                              # evaluate()'s two extra rows: the fans' totals
F06 = float(np.float32(0.06))                # the fp32 kernel's threshold: 0.05999999865889549
FP64_TOL = 1e-9
REL_STEPS = (1e-8, 4e-8)                     # central differences: relative steps of the inputs
SMOOTH = 0.01
DECIDE = 8 * U
# roundings along the longest chain into a slot of build_obs as written (one per multiply, add, divide, square root; negation, |x| and the
# halving are exact; atan2 counted 3): Rpalm 3, ppalm 4, wrist 7, a geom / site centre 4, its difference to the wrist 8, in the wrist frame 11
C_GROUP = (((0, 18), 11), ((21, 24), 11), ((36, 48), 9), ((48, 50), 14), ((67, 70), 3), ((70, 73), 17), ((73, 75), 20), ((75, 82), 16), ((82, 84), 19))
C_D = 10                                     # roundings that scale d of dot_product20: (3 + 1) + (3 + 1) of a product's two factors, the product, the sum
C_SITE, C_WRIST = 4, 7                       # roundings into a palm site's centre and into the wrist
C_KIN = 16                                   # roundings into a distal link's rotation in the stepping kernel's kinematics
C_SLOT = np.zeros(84)
for (_a, _b), _c in C_GROUP:
    C_SLOT[_a:_b] = _c
EXACT = np.r_[18:21, 24:36, 50:67]           # +0.0 | the sensor values, two negated | obj_size_obs rounded | the given ray or exactly 6
BOUNDED = np.setdiff1d(np.arange(NOBS), EXACT)
PALM_SLOTS, FAN_SLOTS = np.r_[70:73], np.r_[73:75]
FINGER_GEOMS = (2, 4, 6, 3, 5, 7)            # f1_prox f2_prox f3_prox f1_dist f2_dist f3_dist (ko_env_inputs_from_sim)
SITE_ORDER = (5, 6, 9, 10, 13, 14, 7, 8, 11, 12, 15, 16)
# packed inputs
X_SNAP, X_RAYS, X_GPOS, X_GR1, X_SITE, X_SIZE, X_OFF, NX = 0, 105, 122, 146, 155, 206, 209, 211


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def quat_to_mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def constants(M):
    """the model constants that reach a slot, in the packed order (float64, as the blob holds them)"""
    q = np.asarray(M["geom_quat"][1], dtype=np.float64)
    return np.concatenate([np.asarray(M["geom_pos"][1:9], dtype=np.float64).ravel(), quat_to_mat(q / np.linalg.norm(q)).ravel(),
                           np.asarray(M["site_pos"], dtype=np.float64).ravel(), np.asarray(M["obj_size_obs"], dtype=np.float64).ravel(), [-0.009, 0.048]])


def pack(M, snap, rays):
    """X [211, n] of snapshots [105, n] and rays [17, n]; M: one blob dict, or one per state"""
    snap, rays = np.asarray(snap, dtype=np.float64).reshape(NSNAP, -1), np.asarray(rays, dtype=np.float64).reshape(NRAY, -1)
    n = snap.shape[1]
    Ms = M if isinstance(M, (list, tuple)) else [M] * n
    cache = {}
    cons = np.stack([cache.setdefault(id(m), constants(m)) for m in Ms], 1)
    return np.concatenate([snap, rays, cons], 0)


def _body(X, b):
    o = X_SNAP + (b - 2) * 12
    return X[o:o + 9].reshape(3, 3, -1), X[o + 9:o + 12]


def _rv(R, v):
    return np.einsum("ijn,jn->in", R, v)


def _area(a, b):
    return np.sqrt((np.cross(a, b, axis=0) ** 2).sum(0)) / 2


def _dot20(obj, hand):
    ox, oy = np.abs(obj[0] - hand[0]), np.abs(obj[1] - hand[1])
    cx, cy = np.abs(hand[0]), np.abs(hand[1])
    on, cn = np.sqrt(ox * ox + oy * oy), np.sqrt(cx * cx + cy * cy)
    return ((ox / on) * (cx / cn) + (oy / on) * (cy / cn)) ** 20


Decisions = namedtuple("Decisions", "member miss am fan lifted")     # member [5, n] bool, miss [17, n] bool, am [n] int, fan [n] bool (total1 > total2), lifted [n] bool


def evaluate(X, site_body, force: Decisions | None = None):
    """(y [84, n], z [n], Decisions taken, g [3, n]): the 82 slots and the two fan totals of the packed inputs X [211, n]"""
    with np.errstate(all="ignore"):
        X = np.asarray(X, dtype=np.float64)
        n = X.shape[1]
        y = np.zeros((84, n))
        R7, p7 = _body(X, 2)
        gpos = X[X_GPOS:X_GR1].reshape(8, 3, n)                  # geoms 1 .. 8
        Rpalm = np.einsum("ijn,jkn->ikn", R7, X[X_GR1:X_SITE].reshape(3, 3, n))
        ppalm = p7 + _rv(R7, gpos[0])
        T3 = np.stack([-Rpalm[:, 1], -Rpalm[:, 2], Rpalm[:, 0]])                  # rows of (R_palm C)^T
        wrist = ppalm + T3[0] * X[X_OFF] + T3[1] * X[X_OFF + 1]
        fw = []
        for k, g in enumerate(FINGER_GEOMS):
            R, p = _body(X, ko.GEOM_BODY[g])
            fw.append(p + _rv(R, gpos[g - 1]))
            y[3 * k:3 * k + 3] = _rv(T3, fw[k] - wrist)
        fl = y[0:18].reshape(6, 3, n)
        Ro, po = _body(X, 9)
        ow = po + _rv(Ro, gpos[7])
        ol = _rv(T3, ow - wrist)
        y[21:24] = ol
        jp = X[X_SNAP + 96:X_SNAP + 105]
        y[24:26], y[26:33] = -jp[:2], jp[2:]
        y[33:36] = X[X_SIZE:X_OFF]
        site = X[X_SITE:X_SIZE].reshape(17, 3, n)
        for k, si in enumerate(SITE_ORDER):
            R, p = _body(X, int(site_body[si]))
            y[36 + k] = np.sqrt((((p + _rv(R, site[si])) - ow) ** 2).sum(0))
        y[48], y[49] = np.arctan2(np.abs(ol[2]), ol[1]), np.arctan2(np.abs(ol[0]), ol[1])
        rays = X[X_RAYS:X_GPOS]
        miss = (rays == -1) if force is None else force.miss
        rng = np.where(miss, 6.0, rays)
        y[50:67] = rng
        g = -T3[:, 2]
        y[67:70] = g
        member = (rng[:5] < 0.06) if force is None else force.member
        s, nh = np.zeros((3, n)), member.sum(0)
        for i in range(5):
            l = _rv(T3, (p7 + _rv(R7, site[i])) - wrist)
            l[1] = l[1] + rng[i]
            s = s + np.where(member[i], l, 0.0)
        y[70:73] = np.where(nh == 0, 0.2, s / np.maximum(nh, 1))
        front = _area(fl[0] - fl[2], fl[0] - fl[1])
        top1, top2, top3 = _area(fl[0], fl[3]), _area(fl[3], fl[4]), _area(fl[1], fl[4])
        top4, top5 = _area(fl[2], fl[5]), _area(fl[3], fl[5])
        total1, total2 = top1 + top2 + top3, top1 + top4 + top5
        fan = (total1 > total2) if force is None else force.fan
        top = np.where(fan, total1, total2)
        z0, z1, z2 = X[X_SIZE], X[X_SIZE + 1], X[X_SIZE + 2] * 0.5
        if force is None:
            am = np.zeros(n, dtype=int)
            ag = np.abs(g)
            am = np.where(ag[1] > ag[0], 1, am)
            am = np.where(ag[2] > ag[am, np.arange(n)], 2, am)
        else:
            am = force.am
        y[73] = np.where(am == 0, np.abs(z0 * z1), np.abs(z0 * z2)) / front
        y[74] = np.where(am == 2, np.abs(z0 * z1), np.where(am == 1, np.abs(z1 * z2), np.abs(z0 * z2))) / top
        for k in range(6):
            y[75 + k] = _dot20(fw[k], p7)
        y[81] = _dot20(ow, p7)
        y[T1], y[T2] = total1, total2
        z = ow[2]
        lifted = ((np.abs(z - 0.2) < 0.005) | (z >= 0.2)) if force is None else force.lifted
        return y, z, Decisions(member, miss, am, fan, lifted), g


# ---- the oracle's env layer on a snapshot ---------------------------------------------------------------------------------------------
def inputs_from_snapshot(M, snap, rays):
    """the oracle's ko_env_inputs of ONE snapshot [105] and its rays [17], formed in float64 from the blob's constants"""
    X = pack(M, snap, rays)
    gpos, site = X[X_GPOS:X_GR1, 0].reshape(8, 3), X[X_SITE:X_SIZE, 0].reshape(17, 3)
    body = lambda b: (X[(b - 2) * 12:(b - 2) * 12 + 9, 0].reshape(3, 3), X[(b - 2) * 12 + 9:(b - 2) * 12 + 12, 0])
    centre = lambda g: body(ko.GEOM_BODY[g])[1] + body(ko.GEOM_BODY[g])[0] @ gpos[g - 1]
    R7, p7 = body(2)
    size = X[X_SIZE:X_OFF, 0]
    return dict(palm_xpos=centre(1), palm_xmat=R7 @ X[X_GR1:X_SITE, 0].reshape(3, 3), finger_xpos=np.stack([centre(g) for g in FINGER_GEOMS]),
                obj_xpos=centre(8), link7_xpos=p7, site_xpos=np.stack([body(int(M["site_body"][s]))[1] + body(int(M["site_body"][s]))[0] @ site[s] for s in range(17)]),
                sensordata=np.concatenate([X[96:105, 0], X[X_RAYS:X_GPOS, 0]]), obj_size=np.array([size[0], size[1], size[2] / 2]))


def bearing(inp):
    """slots 48-49 restated: atan2(|s|, y) of the object in the wrist frame, in float64 (x angle, z angle)"""
    Tfw, _, _ = ko.env_ctrl(inp["palm_xpos"], inp["palm_xmat"], np.zeros(4))
    ol = Tfw[:3, :3] @ np.asarray(inp["obj_xpos"]) + Tfw[:3, 3]
    return np.arctan2(abs(ol[2]), ol[1]), np.arctan2(abs(ol[0]), ol[1])


def reference(M, snap, rays):
    """(obs [82], reward, done, info [3], the oracle's own acos slots 48-49) of one snapshot"""
    inp = inputs_from_snapshot(M, snap, rays)
    obs = ko.env_obs_from_inputs(inp)[0]
    acos = obs[48:50].copy()
    obs[48:50] = bearing(inp)
    rew, done, info = ko.env_reward(inp["obj_xpos"][2])
    return obs, rew, done, info, acos


# ---- bound and decidability -----------------------------------------------------------------------------------------------------------
Bound = namedtuple("Bound", "ref z dec bound smooth lift_ok ray_ok am_ok fan_ok finite sens kin")
# ref [n, 84] evaluate()'s slots; bound [n, 84] fp32; smooth [n, 84]; *_ok [n] the decisions decidable; finite [n]; sens [n, 84] the sum |dy/dx_k| |x_k|


def kinematic_error(X):
    """e [105, n]: what fp32 kinematics may leave in every entry of the snapshot"""
    e = np.zeros((NSNAP, X.shape[1]))
    for b in range(2, 10):
        o = (b - 2) * 12
        e[o:o + 9] = C_KIN * U
        e[o + 9:o + 12] = C_KIN * U * np.abs(X[o + 9:o + 12]).max(0)
    return e


def sensitivity(X, site_body, dec, rel, weights=None):
    """(sum_k |dy_j/dx_k| |x_k|, sum over the snapshot's entries of |dy_j/dx_k| weights_k) [84, n] each, by central differences with
    relative step `rel`, the decisions held"""
    n = X.shape[1]
    out, kin = np.zeros((84, n)), np.zeros((84, n))
    rep = lambda a: np.repeat(a, 2, axis=-1)
    dec2 = Decisions(rep(dec.member), rep(dec.miss), rep(dec.am), rep(dec.fan), rep(dec.lifted))
    for k in range(NX):
        x = X[k]
        weighted = weights is not None and k < NSNAP and weights[k].any()
        if not x.any() and not weighted:
            continue
        h = np.where(x != 0, np.abs(x) * rel, rel)
        Xp = np.repeat(X, 2, axis=1)
        Xp[k, 0::2] += h
        Xp[k, 1::2] -= h
        y = evaluate(Xp, site_body, dec2)[0]
        d = np.abs((y[:, 0::2] - y[:, 1::2]) / (2 * h))
        out += d * np.abs(x)
        if weighted:
            kin += d * weights[k]
    return out, kin


def palm_cancellation(X):
    """[3, n]: what the roundings of a palm site's centre and of the wrist - two sums that both start from p7 - leave in their difference in
    the wrist frame; the largest over the five palm sites"""
    n = X.shape[1]
    R7, p7 = _body(X, 2)
    Rpalm = np.einsum("ijn,jkn->ikn", R7, X[X_GR1:X_SITE].reshape(3, 3, n))
    T3 = np.abs(np.stack([-Rpalm[:, 1], -Rpalm[:, 2], Rpalm[:, 0]]))
    B = np.abs(p7) + _rv(np.abs(R7), np.abs(X[X_GPOS:X_GPOS + 3])) + T3[0] * abs(-0.009) + T3[1] * 0.048
    site = np.abs(X[X_SITE:X_SITE + 15].reshape(5, 3, n))
    A = np.max([np.abs(p7) + _rv(np.abs(R7), site[i]) for i in range(5)], 0)
    return U * _rv(T3, C_SITE * A + C_WRIST * B)


def bound(M, snap, rays, chunk=128, kinematics=False) -> Bound:
    X = pack(M, snap, rays)
    n = X.shape[1]
    sb = (M[0] if isinstance(M, (list, tuple)) else M)["site_body"]
    y, z, dec, g = evaluate(X, sb)
    sens, kin = [np.zeros((84, n)), np.zeros((84, n))], np.zeros((84, n))
    ke = kinematic_error(X) if kinematics else None
    for a in range(0, n, chunk):
        sl = slice(a, min(n, a + chunk))
        d = Decisions(dec.member[:, sl], dec.miss[:, sl], dec.am[sl], dec.fan[sl], dec.lifted[sl])
        for i, rel in enumerate(REL_STEPS):
            sens[i][:, sl], k = sensitivity(X[:, sl], sb, d, rel, None if ke is None or i else ke[:, sl])
            if ke is not None and i == 0:
                kin[:, sl] = k
    with np.errstate(all="ignore"):
        S = np.maximum(sens[0], sens[1])
        smooth = np.abs(sens[0] - sens[1]) <= SMOOTH * S
        first = np.abs(y) + S
        b = C_SLOT[:, None] * U * first
        b[75:82] += 20 * C_D * U * np.abs(y[75:82])
        b[70:73] += palm_cancellation(X)
        b = b + (C_SLOT[:, None] * U) ** 2 * np.nanmax(np.where(np.isfinite(first), first, 0.0)[BOUNDED], 0)
        finite = np.isfinite(y[:NOBS]).all(0) & np.isfinite(b[BOUNDED]).all(0)
        Ro, po = _body(X, 9)
        gp8 = X[X_GPOS + 21:X_GPOS + 24]
        lift_ok = np.abs(z - 0.195) > DECIDE * (np.abs(po[2]) + (np.abs(Ro[2]) * np.abs(gp8)).sum(0))
        ray_ok = ~((X[X_RAYS:X_RAYS + 5] == F06).any(0))
        ag = np.sort(np.abs(g), 0)
        am_ok = ag[2] - ag[1] > DECIDE
        fan_ok = np.abs(y[T1] - y[T2]) > b[T1] + b[T2]
    return Bound(y.T, z, dec, b.T, smooth.T, lift_ok, ray_ok, am_ok, fan_ok, finite, S.T, kin.T)


def alternatives(M, snap, rays, bd: Bound, i, left_out_only=False):
    """the references [82] of state i with each undecidable decision taken either way (the state's own reference included)"""
    X = pack(M[i] if isinstance(M, (list, tuple)) else M, np.asarray(snap)[:, i], np.asarray(rays)[:, i])
    sb = (M[0] if isinstance(M, (list, tuple)) else M)["site_body"]
    d = bd.dec
    member, am, fan = d.member[:, i:i + 1], d.am[i:i + 1], d.fan[i:i + 1]
    members = [member]
    if not bd.ray_ok[i]:
        on = np.flatnonzero(X[X_RAYS:X_RAYS + 5, 0] == F06)
        out_ = member.copy()
        out_[on] = False
        members = [out_] if left_out_only else [member, out_]
    ams = [am] if bd.am_ok[i] else [np.array([k]) for k in np.argsort(-np.abs(evaluate(X, sb)[3][:, 0]))[:2]]       # the two largest |g|
    fans = [fan] if bd.fan_ok[i] else [np.array([True]), np.array([False])]
    return [evaluate(X, sb, Decisions(m, d.miss[:, i:i + 1], a, f, d.lifted[i:i + 1]))[0][:NOBS, 0] for m in members for a in ams for f in fans]


def exact_failures(s, obs, precision):
    """slots that carry no bound: +0.0 in every bit | the sensor values, the first two negated | obj_size_obs rounded | the ray, or exactly 6"""
    want = np.zeros((s.snap.shape[1], 82))
    want[:, 24:26], want[:, 26:33] = -s.snap[96:98].T, s.snap[98:105].T
    size = np.asarray(s.M["obj_size_obs"], dtype=np.float64)
    want[:, 33:36] = f32(size) if precision == 32 else size
    want[:, 50:67] = np.where(s.rays == -1, 6.0, s.rays).T
    bad = [(s.cls, int(i), int(EXACT[j]), "exact slot") for i, j in np.argwhere(obs[:, EXACT] != want[:, EXACT])[:5]]
    if np.signbit(obs[:, 18:21]).any():
        bad.append((s.cls, "slots 18-20 hold -0.0"))
    return bad


class Tally:
    """one (class, shape, path) against the reference: worst error over bound per slot group in units of c, failures named by state and slot.
    got: obs [n, 82], reward [n], done [n] (bit 0), info [n, 3] or None.  on_threshold: an fp32 path must leave the ray that equals 0.06f out."""

    def __init__(self, cls, shape, path, precision, M, snap, rays, bd: Bound, extra=None):
        self.cls, self.shape, self.path, self.precision, self.M, self.snap, self.rays, self.bd = cls, shape, path, precision, M, snap, rays, bd
        self.extra = extra                         # [n, 82] added to the fp32 bound (the kinematic error of an in-step snapshot)
        self.failures, self.worst, self.n, self.set_aside = [], np.zeros(NOBS), 0, 0

    def add_all(self, obs, reward, done, info=None, skip=None):
        """skip [n, 82] bool: slots of a state that are not asserted here"""
        bd, obs = self.bd, np.asarray(obs, dtype=np.float64)
        for i in np.flatnonzero(bd.finite):
            self.n += 1
            ref = bd.ref[i, :NOBS]
            b = FP64_TOL * (1 + np.abs(ref)) if self.precision == 64 else bd.bound[i, :NOBS] + (0 if self.extra is None else self.extra[i])
            b = np.where(np.isin(np.arange(NOBS), EXACT), 0.0, b)
            if self.precision == 32:
                ref = ref.copy()
                ref[33:36] = f32(ref[33:36])                  # Model<float> holds the rounded size
            err = np.abs(obs[i] - ref)
            ok = err <= b
            if skip is not None:
                ok[skip[i]] = True
            hang = np.zeros(NOBS, dtype=bool)
            if not bd.ray_ok[i]:
                hang[PALM_SLOTS] = True
            if not (bd.am_ok[i] and bd.fan_ok[i]):
                hang[FAN_SLOTS] = True
            if hang.any():
                # fp64 paths take the reference's decision on a ray that equals 0.06f (the state's own reference); fp32 paths leave that ray out
                alts = alternatives(self.M, self.snap, self.rays, bd, i, left_out_only=self.precision == 32)
                if self.precision == 64 and not bd.ray_ok[i]:
                    alts = [a for a in alts if np.array_equal(a[PALM_SLOTS], ref[PALM_SLOTS])] or alts
                self.set_aside += 1
                # (an alternative's own size stands in the bound: "none" is the constant 0.2, whatever the sums of the other branch are)
                ok[hang] = np.array([np.abs(obs[i] - a)[hang] <= (b + (0 if self.precision == 64 else C_SLOT[:NOBS] * U * np.abs(a)))[hang] for a in alts]).any(0)
            else:
                r = np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0) * (1.0 if self.precision == 64 else C_SLOT[:NOBS])
                if skip is not None:
                    r[skip[i]] = 0
                self.worst = np.maximum(self.worst, np.where(bd.smooth[i, :NOBS], r, 0.0))
            for j in np.flatnonzero(~ok):
                self.failures.append((self.cls, int(i), int(j), f"{obs[i, j]!r} against {ref[j]!r}: {err[j] / b[j] if b[j] else np.inf:.3g} x the bound"))
            want = 50.0 if bd.dec.lifted[i] else 0.0
            got = (float(reward[i]), int(done[i]) & 1) + (() if info is None else tuple(float(v) for v in info[i]))
            exp = [(w, int(w > 0)) + (() if info is None else (0.0, 0.0, w)) for w in ((want,) if bd.lift_ok[i] else (0.0, 50.0))]
            if got not in exp:
                self.failures.append((self.cls, int(i), "reward / done / info", got, exp))

    def check(self):
        assert not self.failures, (self.path, self.shape, len(self.failures), self.failures[:6])

    def line(self):
        unit = "of 1e-9 (1 + |ref|)" if self.precision == 64 else "c"
        w = " ".join(f"{a}-{b - 1}:{self.worst[a:b].max():.3g}" + ("" if self.precision == 64 else f"/{c}") for (a, b), c in C_GROUP if a < NOBS)
        return f"{self.cls:15s} {self.shape:8s} {self.path:28s} states {self.n:4d} worst error over bound in {unit} per slot group {w}; set aside {self.set_aside}; failures {len(self.failures)}"
