"""Plain float64 numpy references of running observation normalisation (ddpgfd.DDPGfD with obs_norm; include/kinova_rollout.h:
kr_obs_stats_update, kr_obs_normalize, kr_fold_obs_norm), written from the rules and not from the kernels, and the error bounds the tests
hold the implementations to.  tests/test_obsnorm_reference_cpu.py checks this file against numpy's one-shot mean and variance and holds
ddpgfd.ObsNorm to it.

Bounds.  u = 2^-53 is the relative error of one fp64 operation.  For a column whose entries and prior mean are at most X in magnitude,
`rows` counted rows merged in `merges` batches:
  * a batch mean is a sum of nb terms and a division, (nb + 1) u X; a merge mean + delta (nb / n) adds at most 8 u X (|delta| <= 2 X); the
    previous merges' error enters with the factor na / n <= 1.  Two implementations differ by twice that: mean_bound = 4 (rows + 16 merges) u X;
  * a batch's squared deviations: each d = x - mb carries the batch mean's error, |d| <= 2 X, so sum d^2 is off by at most
    2 (nb + 1) u X * 2 X nb + (nb + 3) u * 4 X^2 nb <= 8 nb (nb + 2) u X^2; the merge's term delta^2 na nb / n (weight <= nb) carries the
    running mean's error, 2 |delta| nb * 4 (rows + 16 merges) u X, and the additions a few u of the sum, which is at most m2_prior + 4 rows X^2.
    Summed over the merges and doubled: m2_bound = 64 rows (rows + 16 merges + 16) u X^2 + 16 u m2_prior.
Both are "a few rows x 2^-53 of the column's magnitude" (X for the mean, rows X^2 for m2).
"""
import math

import numpy as np

U53 = 2.0 ** -53
U24 = 2.0 ** -24


def counted(weight, rows):
    """the rows that count: weight != 0 (None: all; a NaN weight is not 0)"""
    return np.ones(rows, bool) if weight is None else ~(np.asarray(weight) == 0)


def derived_ref(count, mean, m2, eps):
    """mean32 = fp32(mean), inv32 = fp32(1 / max(sqrt(m2 / count), eps))"""
    sd = np.sqrt(np.asarray(m2, np.float64) / np.float64(count))
    return np.asarray(mean, np.float64).astype(np.float32), (1.0 / np.where(sd > eps, sd, np.float64(eps))).astype(np.float32)


def stats_update_ref(x, weight, count, mean, m2, it=None, freeze_after=None):
    """x [rows, >= S] (the first S = len(mean) columns are the observation), weight [rows] or None -> (count, mean, m2) after the update, or
    None where the update leaves everything untouched: no counted row, or it >= freeze_after.  Two passes in fp64 within the batch, then
    Chan's parallel formula."""
    S = len(mean)
    on = counted(weight, x.shape[0])
    if not on.any() or (freeze_after is not None and it is not None and it >= freeze_after):
        return None
    xb = np.asarray(x, np.float64)[on][:, :S]
    nb = float(xb.shape[0])
    mb = xb.sum(0) / nb
    q = ((xb - mb) ** 2).sum(0)
    na = float(count)
    n = na + nb
    delta = mb - mean
    return n, mean + delta * (nb / n), (m2 + q) + (delta * delta) * (na * (nb / n))


def mean_bound(rows, merges, X):
    return 4.0 * (rows + 16 * merges) * U53 * np.asarray(X, np.float64)


def m2_bound(rows, merges, X, m2_prior=0.0):
    X = np.asarray(X, np.float64)
    return 64.0 * rows * (rows + 16 * merges + 16) * U53 * X * X + 16.0 * U53 * np.asarray(m2_prior, np.float64)


def normalize_ref(x, mean32, inv32):
    """the first S = len(mean32) columns of x [rows, >= S] -> fl(fl(x - mean32) * inv32) in float32, the others as they are"""
    S = len(mean32)
    out = np.array(x, np.float32, copy=True)
    out[:, :S] = (out[:, :S] - np.asarray(mean32, np.float32)) * np.asarray(inv32, np.float32)
    return out


def fold_ref(W1, b1, mean32, inv32):
    """W1 [h1, in_dim], b1 [h1] float32, the first S = len(mean32) columns normalised ->
    (W1_out float32: fl(W1 * inv32) on those columns, the others copied;  b1_out as an exactly rounded float64 of
    b1 - sum_k W1_out_jk mean32_k - the products of two float32 are exact in float64, math.fsum adds without error -;  sum of the |terms|)"""
    S = len(mean32)
    W1, b1 = np.asarray(W1, np.float32), np.asarray(b1, np.float32)
    out = W1.copy()
    out[:, :S] = W1[:, :S] * np.asarray(inv32, np.float32)
    prod = out[:, :S].astype(np.float64) * np.asarray(mean32, np.float64)
    bias = np.array([math.fsum([float(b1[j])] + (-prod[j]).tolist()) for j in range(W1.shape[0])])
    return out, bias, np.abs(b1.astype(np.float64)) + np.abs(prod).sum(1)


def fold_bias_bound(bias, terms, norm_dim):
    """half an fp32 ulp of the result + the fp64 sum's (norm_dim + 1) u sum |terms|"""
    a = np.maximum(np.abs(bias), 2.0 ** -126).astype(np.float32)
    ulp = np.maximum(np.nextafter(a, np.float32(np.inf)) - a, a - np.nextafter(a, np.float32(0))).astype(np.float64)
    return 0.5 * ulp + (norm_dim + 1) * U53 * terms


def preactivation_bound(W1_out, x, mean32):
    """the first layer through folded fp32 weights against explicit normalisation in fp64, per (row, unit): (S + 2) 2^-24 sum_k |W1'_jk| (|x_k| +
    |mean32_k|), S = len(mean32) - the fold's one rounding per weight, the bias's, and an fp32 dot product of S terms"""
    S = len(mean32)
    mag = np.abs(np.asarray(x, np.float64)[:, :S]) + np.abs(np.asarray(mean32, np.float64))
    return (S + 2) * U24 * (mag @ np.abs(np.asarray(W1_out, np.float64)[:, :S]).T)
