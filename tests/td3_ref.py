"""Plain references of the TD3fD rules of include/kinova_rollout.h (kr_target_smooth, kr_twin_critic_grad, kr_adam_step_every), written
from the header's rules - not from the kernels.  numpy on the host, in the style of tests/glue_ref.py: float64 arithmetic on float32
inputs widened exactly, except where the rule itself is a float32 expression (the smoothing: two roundings and two clamps).

tests/test_td3_reference_cpu.py checks these functions against float64 autograd of ddpgfd.TD3fD's phases;
tests/test_gpu_td3_kernels.py then holds the kernels to them.
"""
import numpy as np

from tests import glue_ref as gr
from tests.philox_ref import MASK, philox4x32_10

TAG_TARGET_SMOOTH = 0x5433          # the stream of kr_target_smooth (the exploration noise: 0x4b52, the samplers: 0x5a4d / 0x5a4e)


def normal4_tagged(seed, step, row, tag):
    """fp64 reference of krsel::normal4_tagged: counter (row, step low word, step high word, tag), key (seed low word, seed high word); the
    top 24 bits of each word -> uniforms (r + 0.5) / 2^24 as philox_ref.normal4 forms them; Box-Muller on (u0, u1) and (u2, u3).
    Returns [..., 4] float64."""
    seed, step, row = (np.asarray(x, dtype=np.uint64) for x in (seed, step, row))
    seed, step, row = np.broadcast_arrays(seed, step, row)
    r = philox4x32_10((row & MASK, step & MASK, step >> np.uint64(32), np.full_like(row, tag)), (seed & MASK, seed >> np.uint64(32)))
    u = [((x >> np.uint32(8)).astype(np.float32) + np.float32(0.5)).astype(np.float64) / 16777216.0 for x in r]
    ra, rb = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a, b = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    return np.stack([ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)], -1)


def clamp(x, lo, hi):
    """x < lo ? lo : (x > hi ? hi : x) - a NaN fails both comparisons and stays"""
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def target_smooth_f32(action, z, sigma, clip, max_action):
    """the header's rule in float32, every operation rounded once: e = sigma z; e clamped to [-clip, clip]; s = action + e; s clamped
    to [0, max_action].  float32 in, float32 out - the kernel must give these bits."""
    f = np.float32
    action, z = np.asarray(action, f), np.asarray(z, f)
    with np.errstate(invalid="ignore"):
        e = clamp((f(sigma) * z).astype(f), f(-f(clip)), f(clip)).astype(f)
        return clamp((action + e).astype(f), f(0.0), f(max_action)).astype(f)


def target_smooth_ref(action, z, sigma, clip, max_action):
    """the same rule in float64 on widened inputs (what TD3fD.phase_critic computes in float64)"""
    with np.errstate(invalid="ignore"):
        return clamp(gr.wide(action) + clamp(sigma * gr.wide(z), -clip, clip), 0.0, max_action)


def nan_min(a, b):
    """the smaller of the two; NaN if either is NaN (np.minimum's rule)"""
    return np.minimum(a, b)


def twin_critic_grad_ref(q1, q2, tq1_a, tq1_b, tqn_a, tqn_b, reward, weight, wsum, discount):
    """m1 = min(tq1_a, tq1_b), mn = min(tqn_a, tqn_b); targets from them as glue_ref.critic_targets; per critic k
    dq_k = w / wsum (2 (q_k - target_Q) + (q_k - target_QN)) and (loss, L1, LN) as glue_ref.critic_grad_ref.
    Returns dq1, dq2, tmin [2R] (in the inputs' type: the minimum is exact), losses (six floats)."""
    m1, mn = nan_min(np.asarray(tq1_a), np.asarray(tq1_b)), nan_min(np.asarray(tqn_a), np.asarray(tqn_b))
    dq1, l1 = gr.critic_grad_ref(q1, m1, mn, reward, weight, wsum, discount)
    dq2, l2 = gr.critic_grad_ref(q2, m1, mn, reward, weight, wsum, discount)
    return dq1, dq2, np.concatenate([m1, mn]), tuple(l1) + tuple(l2)


def adam_every_ref(p, g, m, v, step, every, lr, b1, b2, eps, wd):
    """glue_ref.adam_ref as step number step / every when step is a positive multiple of `every`; otherwise nothing changes"""
    if step > 0 and step % every == 0:
        return gr.adam_ref(p, g, m, v, step // every, lr, b1, b2, eps, wd)
    return gr.wide(p), gr.wide(m), gr.wide(v)
