"""The explicit Q of the panel-pivoted QR, accumulated first factor to last (CPU, numpy).

dqmc_amd/csrc/qr_panel.hip no longer forms Q = H_0 ... H_{p-1} I from the last factor to the first after the factorisation: the
update launch of panel k applies H_k^T to a buffer that starts as the identity, Q^T = H_{p-1}^T ... H_0^T I, and retires rows
16 k .. 16 k + 15 of it into columns 16 k .. 16 k + 15 of Q at once, because the reflectors of every later factor start below
them.  This file restates exactly that scheme on the compact-WY factors I - V_k T_k V_k^T of the factorisation
oracle/panel_qr.py::qr_sketch(b = 16, p = 16, sign = True, local_pivot = False) performs, and compares with the Q it returns.

The factors are LAPACK's own (dgeqrf on each selected panel, as in panel_qr._apply_panel, whose steps are repeated here call for
call so that both sides see the same reflectors), T is dlarft's recurrence.

Bound: both sides are products of the same n Householder reflectors applied to a matrix of orthonormal columns; every reflector
application perturbs an entry by at most a small multiple of eps times the column's norm (= 1), and a row takes part in at most n
of them, in either order: |dQ| <= 4 n eps, entry by entry, covers both evaluations with the constant 2 each that the usual
analysis of a reflector application gives (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 19.2 / 19.3)."""
import numpy as np
import pytest
import scipy.linalg as sla

from oracle import panel_qr as pq

B = 16
EPS = np.finfo(np.float64).eps


def dqmc_like(n, seed):
    """columns graded over ~10 orders of magnitude, the shape (M L) diag(d) has in a sweep"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, n)) * np.exp(rng.uniform(-12, 12, n))[None, :]


def compact_wy_factors(M, P):
    """(V_k, T_k) of every 16-column panel of the unpivoted blocked Householder QR of M[:, P], with the trailing update done as
    panel_qr._apply_panel does it (explicit Qp^T), so the reflectors are those of the oracle's factorisation."""
    A = np.array(M[:, P], dtype=np.float64, copy=True)
    n = A.shape[0]
    factors = []
    for k in range(0, n, B):
        (h, tau), _ = sla.qr(A[k:, k:k + B], mode="raw")
        Qp, Rp = sla.qr(A[k:, k:k + B])
        V = np.tril(h, -1)[:, :B] + np.eye(n - k, B)
        T = np.zeros((B, B))
        for j in range(B):                                    # dlarft, forward / columnwise
            T[j, j] = tau[j]
            T[:j, j] = -tau[j] * (T[:j, :j] @ (V[:, :j].T @ V[:, j]))
        A[k:, k:k + B] = Rp
        A[k:, k + B:] = Qp.T @ A[k:, k + B:]
        factors.append((k, V, T))
    return factors, np.triu(A)


def q_first_to_last(n, factors):
    """Q^T = H_{p-1}^T ... H_0^T I on rows >= k only; the 16 rows factor k completes go into Q as columns and are never touched again."""
    Qacc = np.eye(n)
    Q = np.full((n, n), np.nan)
    for (k, V, T) in factors:
        W = V.T @ Qacc[k:, :]                                 # the kernel's three products: W = V^T A, W' = T^T W, A - V W'
        Qacc[k:, :] -= V @ (T.T @ W)
        Q[:, k:k + B] = Qacc[k:k + B, :].T
        Qacc[k:k + B, :] = np.nan                             # retired: a later read of these rows would poison the result
    return Q


@pytest.mark.parametrize("n", [64, 256, 576])
def test_factors_applied_first_to_last_reproduce_the_oracles_q(n):
    M = dqmc_like(n, 40 + n)
    Q, R0, P = pq.qr_sketch(M, 16, 16, local_pivot=False, sign=True)
    factors, R0_mine = compact_wy_factors(M, P)
    assert np.abs(R0_mine - R0).max() <= 4 * n * EPS * np.abs(R0).max()          # the same factorisation, panel by panel
    Qf = q_first_to_last(n, factors)
    assert np.isfinite(Qf).all()                                                 # every column was retired exactly once
    err = float(np.abs(Qf - Q).max())
    print(f"n = {n}: max|Q(first to last) - Q(oracle)| = {err:.3e}, bound {4 * n * EPS:.3e}")
    assert err <= 4 * n * EPS
    assert np.abs(Qf.T @ Qf - np.eye(n)).max() <= 4 * n * EPS


def test_rows_above_a_factor_are_left_alone():
    """The retiring-rows argument itself: H_k = I - V_k T_k V_k^T with V_k zero above row 16 k is the identity on those rows."""
    n = 64
    M = dqmc_like(n, 5)
    _, _, P = pq.qr_sketch(M, 16, 16, local_pivot=False, sign=True)
    factors, _ = compact_wy_factors(M, P)
    for (k, V, T) in factors:
        H = np.eye(n)
        H[k:, k:] -= V @ T @ V.T
        assert np.array_equal(H[:k, :], np.eye(n)[:k, :]) and np.array_equal(H[:, :k], np.eye(n)[:, :k])
        assert np.abs(H.T @ H - np.eye(n)).max() <= 4 * n * EPS
