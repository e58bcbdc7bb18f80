"""Plain float64 references of the behaviour-cloning term of the actor loss (include/kinova_rollout.h: kr_bc_actor_grad; ddpgfd.DDPGfD with
bc_weight, q_filter).  numpy only; tests/test_bc_reference_cpu.py holds them to float64 autograd of the loss and to the torch policy."""
import numpy as np


def wide(x):
    return np.asarray(x, np.float64)


def bc_filter_ref(rows, demo_from, q_demo=None, q_pi=None):
    """f [rows]: 0 below demo_from; from there 1 without the filter, else 1 where q_demo > q_pi on the floats as given (strict; a NaN on
    either side compares false)"""
    f = np.zeros(rows, np.float64)
    if q_demo is None:
        f[demo_from:] = 1.0
    else:
        with np.errstate(invalid="ignore"):
            f[demo_from:] = (np.asarray(q_demo).reshape(-1)[demo_from:] > np.asarray(q_pi).reshape(-1)[demo_from:]).astype(np.float64)
    return f


def bc_actor_grad_ref(demo_from, pi, demo, q_demo, q_pi, dq, bc_weight, max_action, dz3):
    """the header's expression in float64 on the given floats.  Returns (dz3', sq, f, written): written [rows] marks the rows whose dz3
    the kernel stores - f = 1, dq != 0 (a NaN is not 0), bc_weight != 0; every other row of dz3' is dz3's own"""
    pi, demo, dq, dz3 = wide(pi), wide(demo), wide(dq).reshape(-1), wide(dz3)
    rows = pi.shape[0]
    f = bc_filter_ref(rows, demo_from, q_demo, q_pi)
    on = f == 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        d = pi - demo
        sq = np.where(on, (d * d).sum(1), 0.0)
        written = on & (dq != 0.0) & (bc_weight != 0.0)
        add = (2.0 * bc_weight * -dq)[:, None] * d * (pi * (1.0 - pi / max_action))
    out = dz3.copy()
    out[written] = dz3[written] + add[written]
    return out, sq, f, written


def bc_loss_ref(sq, f, weight, n, demo_from_rows, bc_weight):
    """the term itself and the weighted pass share from per-state sq and f [R * n] and the window rows' weight [R]:
    bc_weight sum_r w_r sum_k sq_rk / (max(sum(w), 1) n);  sum_r w_r sum_k f_rk / (sum_{r >= demo_from} w_r n)"""
    w = wide(weight)
    loss = bc_weight * float((wide(sq).reshape(-1, n).sum(1) * w).sum()) / (max(float(w.sum()), 1.0) * n)
    den = float(w[demo_from_rows:].sum()) * n
    share = float((wide(f).reshape(-1, n).sum(1) * w).sum()) / den if den > 0 else 0.0
    return loss, share
