"""Per-trajectory cost weights without a GPU: the size query of the packed buffer, the weight-sweep workload, the host-side
checks of the weights and the mirror's length check."""
import ctypes

import numpy as np
import pytest

from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, _capi, workloads


def test_weights_bytes_query():
    lib = _capi.load()
    p = _capi.Problem()
    p.kind, p.m, p.N, p.dt = _capi.DYN_SE3, 6, 200, 0.05
    for B in (1, 4, 13, 4096):
        Bp = (B + 3) // 4 * 4
        assert lib.tolg_weights_bytes(ctypes.byref(p), B) == (24 + 6) * Bp * 8
    assert lib.tolg_weights_bytes(ctypes.byref(p), 0) == 0
    p.kind, p.m = _capi.DYN_DRONE, 4
    assert lib.tolg_weights_bytes(ctypes.byref(p), 13) == (24 + 4) * 16 * 8
    p.kind, p.m = _capi.DYN_SE3, 4  # SE3 dynamics has 6 inputs: an invalid problem
    assert lib.tolg_weights_bytes(ctypes.byref(p), 16) == 0
    p.kind, p.m, p.dt = _capi.DYN_DRONE, 4, -1.0
    assert lib.tolg_weights_bytes(ctypes.byref(p), 16) == 0


def test_set_weights_without_handle_is_an_argument_error():
    lib = _capi.load()
    assert lib.tolg_set_weights(None, 4, None, None, None, None, 0, None) == -1


def test_weight_sweep_workload_is_seeded():
    a = workloads.se3_weight_sweep(13, 3, N=40)
    b = workloads.se3_weight_sweep(13, 3, N=40)
    for x, y in zip(a[1:8], b[1:8]):
        np.testing.assert_array_equal(x, y)
    c = workloads.se3_weight_sweep(13, 3, N=40, seed=workloads.SEED + 7)
    assert not np.array_equal(a[4], c[4])


def test_weight_sweep_sets():
    B, K, spread = 10, 4, 10.0
    prob, q, xi, us, Q, P, R, idx, (Qk, Pk, Rk) = workloads.se3_weight_sweep(B, K, N=40, spread=spread)
    assert Q.shape == (B, 12, 12) and P.shape == (B, 12, 12) and R.shape == (B, 6, 6)
    np.testing.assert_array_equal(idx, np.arange(B) % K)
    for b in range(B):
        np.testing.assert_array_equal(Q[b], Qk[idx[b]])
        np.testing.assert_array_equal(R[b], Rk[idx[b]])
    for A, base in ((Qk, prob.Q), (Pk, prob.P), (Rk, prob.R)):
        d = np.diagonal(A, axis1=1, axis2=2)
        np.testing.assert_array_equal(A, d[:, :, None] * np.eye(A.shape[1]))  # diagonal
        ratio = d / np.diag(base)
        assert np.all(ratio >= 1 / spread) and np.all(ratio <= spread)
    assert len({tuple(np.diag(x)) for x in Qk}) == K


def _fake_solver(B=4, m=6):
    """the host-side check alone: no handle, no device"""
    s = object.__new__(BatchedTrackingILQR)
    s.m = m
    return s, np.tile(np.eye(12), (B, 1, 1)), np.tile(np.eye(12), (B, 1, 1)), np.tile(np.eye(m), (B, 1, 1))


def test_check_weights_accepts_diagonals():
    s, Q, P, R = _fake_solver()
    assert s._check_weights(4, None, None, None) is None
    R[1] = 0.0  # a zero weight is legal
    q, p, r = s._check_weights(4, Q, P, R)
    assert q.shape == (4, 12) and p.shape == (4, 12) and r.shape == (4, 6)
    np.testing.assert_array_equal(r[1], 0.0)


def test_check_weights_errors():
    s, Q, P, R = _fake_solver()
    with pytest.raises(ValueError):
        s._check_weights(4, Q, P, None)                      # all three or none
    with pytest.raises(ValueError):
        s._check_weights(4, Q[:3], P, R)                     # wrong B
    with pytest.raises(ValueError):
        s._check_weights(4, Q, P, np.tile(np.eye(4), (4, 1, 1)))  # R of another m
    with pytest.raises(ValueError):
        s._check_weights(4, Q[:, :6, :6], P, R)              # a 6 x 6 Q
    for name, k in (("Q", 0), ("P", 1), ("R", 2)):
        for bad in ("offdiag_in_block", "offdiag_cross", "negative", "nan", "inf"):
            w = [Q.copy(), P.copy(), R.copy()]
            a = w[k]
            if bad == "offdiag_in_block":
                a[2, 0, 1] = 0.5                             # inside the pose block the kernels read
            elif bad == "offdiag_cross":
                a[2, 1, a.shape[1] - 1] = 0.5                # between the blocks (R: an off-diagonal entry too)
            elif bad == "negative":
                a[3, 2, 2] = -1.0
            elif bad == "nan":
                a[0, 0, 0] = np.nan
            else:
                a[0, 1, 1] = np.inf
            with pytest.raises(ValueError):
                s._check_weights(4, *w)


def test_mirror_weights_length_check():
    from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_controller import _stack_weights
    assert _stack_weights(None, 3) == (None, None, None)
    w = [(np.eye(12) * (b + 1), np.eye(6), np.eye(12) * 2) for b in range(3)]
    Q, P, R = _stack_weights(w, 3)
    assert Q.shape == (3, 12, 12) and P.shape == (3, 12, 12) and R.shape == (3, 6, 6)
    assert Q[2, 0, 0] == 3 and P[0, 0, 0] == 2 and R[1, 0, 0] == 1
    with pytest.raises(ValueError):
        _stack_weights(w[:2], 3)
