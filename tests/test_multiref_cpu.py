"""Per-trajectory references without a GPU: the size query of the packed buffer, the multi-reference workload, the
host-side shape checks."""
import ctypes
import types

import numpy as np
import pytest

from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, _capi, workloads


def test_refs_bytes_query():
    lib = _capi.load()
    p = _capi.Problem()
    p.kind, p.m, p.N, p.dt = _capi.DYN_SE3, 6, 200, 0.05
    for B in (1, 4, 13, 4096):
        Bp = (B + 3) // 4 * 4
        assert lib.tolg_refs_bytes(ctypes.byref(p), B) >= (200 + 1) * 13 * Bp * 8
    assert lib.tolg_refs_bytes(ctypes.byref(p), 0) == 0
    p.m = 4  # SE3 dynamics has 6 inputs: an invalid problem
    assert lib.tolg_refs_bytes(ctypes.byref(p), 16) == 0
    p.kind, p.m, p.dt = _capi.DYN_DRONE, 4, -1.0
    assert lib.tolg_refs_bytes(ctypes.byref(p), 16) == 0


def test_set_refs_without_handle_is_an_argument_error():
    lib = _capi.load()
    assert lib.tolg_set_refs(None, 4, None, None, None, 0, None) == -1


def test_multiref_workload_is_seeded():
    a = workloads.se3_multiref(13, 3, N=40)
    b = workloads.se3_multiref(13, 3, N=40)
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)
    c = workloads.se3_multiref(13, 3, N=40, seed=workloads.SEED + 7)
    assert not np.array_equal(a[4], c[4])


def test_multiref_references_are_rigid_motions_of_the_base():
    B, R, N = 10, 4, 200
    prob, x0_q, x0_xi, us0, q_ref, xi_ref, idx, G = workloads.se3_multiref(B, R, N=N)
    assert q_ref.shape == (B, N + 1, 4, 4) and xi_ref.shape == (B, N + 1, 6) and G.shape == (R, 4, 4)
    np.testing.assert_array_equal(idx, np.arange(B) % R)
    assert len({tuple(np.round(g.ravel(), 12)) for g in G}) == R  # distinct
    for r in range(R):
        Rg = G[r, :3, :3]
        np.testing.assert_allclose(Rg @ Rg.T, np.eye(3), atol=1e-12)
        assert np.linalg.det(Rg) == pytest.approx(1.0, abs=1e-12)
        np.testing.assert_array_equal(G[r, 3], [0, 0, 0, 1])
    for b in range(B):
        g = G[idx[b]]
        for i in range(N + 1):
            np.testing.assert_allclose(q_ref[b, i], g @ prob.q_ref[i], rtol=0, atol=1e-12)
        # same body twists, and the same relative motion between knots: a kinematically consistent path
        np.testing.assert_array_equal(xi_ref[b], prob.xi_ref)
        rel = np.linalg.inv(q_ref[b, :-1]) @ q_ref[b, 1:]
        np.testing.assert_allclose(rel, np.linalg.inv(prob.q_ref[:-1]) @ prob.q_ref[1:], rtol=0, atol=1e-10)
        # the initial state sits where se3_tracking puts it relative to the first pose of the unmoved path
        base = workloads.se3_tracking(B, N=N)[1]
        np.testing.assert_allclose(np.linalg.inv(q_ref[b, 0]) @ x0_q[b], np.linalg.inv(prob.q_ref[0]) @ base[b], atol=1e-10)


def test_multiref_index_argument():
    prob, *_, idx, G = workloads.se3_multiref(12, 3, N=20, index=np.arange(12) // 4)
    np.testing.assert_array_equal(idx, np.repeat([0, 1, 2], 4))
    with pytest.raises(ValueError):
        workloads.se3_multiref(12, 3, N=20, index=np.arange(12))
    with pytest.raises(ValueError):
        workloads.se3_multiref(12, 3, N=20, index=np.zeros(5, dtype=int))


def test_reference_shapes_are_checked_on_the_host():
    fake = types.SimpleNamespace(N=20)
    check = BatchedTrackingILQR._check_refs
    q = np.zeros((5, 21, 4, 4)); xi = np.zeros((5, 21, 6))
    assert check(fake, 5, None, None) is None
    assert check(fake, 5, q, xi) is not None
    for bad in ((q[:, :-1], xi[:, :-1]), (q[:-1], xi[:-1]), (q, None), (None, xi), (q[..., :3], xi), (q, xi[..., :4])):
        with pytest.raises(ValueError):
            check(fake, 5, *bad)


def test_mirror_refs_must_match_the_initial_states():
    from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_controller import _stack_refs
    q = np.zeros((21, 4, 4)); xi = np.zeros((21, 6))
    assert _stack_refs(None, 3) == (None, None)
    qs, xs = _stack_refs([(q, xi)] * 3, 3)
    assert qs.shape == (3, 21, 4, 4) and xs.shape == (3, 21, 6)
    with pytest.raises(ValueError):
        _stack_refs([(q, xi)] * 2, 3)
