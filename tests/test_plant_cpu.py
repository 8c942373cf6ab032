"""Plants (tolg_set_plant): the parts that need no GPU -- the C ABI surface, the host-side checks of plant_J / plant_pend,
the mismatch workload, and the CPU restatement of a closed-loop rollout on a plant that tests/test_gpu_plant.py checks the
kernels against."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from oracle import bridge as ob
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, _capi, workloads
from tests.restate import plant_problem, restate_plant_policy, restate_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tolg_plant_bytes", "tolg_set_plant")


def test_new_symbols_in_header_capi_and_library():
    hdr = open(os.path.join(ROOT, "include", "tolg.h")).read()
    lib = _capi.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name)
    assert re.search(r"TOLG_PLANT_DIAG = 0, TOLG_PLANT_DENSE = 1", hdr)
    assert (_capi.PLANT_DIAG, _capi.PLANT_DENSE) == (0, 1)


def test_plant_bytes_is_consistent():
    lib = _capi.load()
    p = _capi.Problem()
    p.kind, p.m, p.N, p.dt = _capi.DYN_SE3, 6, 40, 0.05
    n = lambda B, S: lib.tolg_plant_bytes(C.byref(p), B, S)  # noqa: E731
    assert n(1, 1) > 0 and n(1, 1) % 8 == 0
    assert n(7, 3) == 21 * n(1, 1) and n(4096, 16) == 4096 * 16 * n(1, 1)
    # every form fits: the dense form's 36 inertia constants and more per row
    assert n(1, 1) >= 36 * 8
    assert n(0, 1) == 0 and n(1, 0) == 0 and n(-3, 2) == 0
    p.m = 4  # SE3 has 6 inputs: an invalid problem
    assert lib.tolg_plant_bytes(C.byref(p), 2, 2) == 0


def test_null_handle_is_an_argument_error():
    lib = _capi.load()
    assert lib.tolg_set_plant(None, 1, 1, 0, None, None, None, 0, None) == -1


@pytest.mark.parametrize("model", ["se3", "pendulum"])
def test_restatement_with_the_model_as_plant_is_restate_policy(model):
    if model == "pendulum":
        prob, q0, xi0, us = workloads.pendulum_swingup(1)
    else:
        prob, q0, xi0, us = workloads.se3_tracking(1, N=20)
    op = ob.OracleProblem(prob.kind, prob.J, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref,
                          pend_mass=prob.pend_mass, pend_length=prob.pend_length)
    N, m = prob.N, prob.m
    rng = np.random.default_rng(4)
    u = rng.normal(size=(N, m)) * 0.1
    q_nom = np.zeros((N + 1, 4, 4)); xi_nom = np.zeros((N + 1, 6))
    q_nom[0], xi_nom[0] = np.asarray(prob.q_ref[0], float), np.asarray(prob.xi_ref[0], float)
    for i in range(N):
        q_nom[i + 1], xi_nom[i + 1] = ob.f(op, q_nom[i], xi_nom[i], u[i])
    K = rng.normal(size=(N, m, 12)) * 0.01
    dx0 = rng.normal(size=(3, 12)) * 0.01
    w = rng.normal(size=(3, N, 6)) * 1e-3
    a = restate_policy(op, q_nom, xi_nom, u, K, dx0, w, S=3)
    b = restate_plant_policy(op, plant_problem(prob, prob.J), q_nom, xi_nom, u, K, dx0, w, S=3)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # and a plant that is not the model steps elsewhere
    J2 = np.array(prob.J, float); J2[0, 0] *= 1.2
    c = restate_plant_policy(op, plant_problem(prob, J2), q_nom, xi_nom, u, K, dx0, w, S=3)
    assert not np.array_equal(a[1], c[1])


def test_plant_mismatch_workload_is_seeded_and_shaped():
    for kind in ("se3", "drone"):
        a = workloads.plant_mismatch(3, 4, kind=kind, N=20, seed=7)
        b = workloads.plant_mismatch(3, 4, kind=kind, N=20, seed=7)
        c = workloads.plant_mismatch(3, 4, kind=kind, N=20, seed=8)
        prob, q, xi, us, dx0, noise, PJ = a
        assert prob.kind == kind and prob.N == 20 and q.shape[0] == 3 and us.shape == (3, 20, prob.m)
        assert dx0.shape == (3, 4, 12) and noise.shape == (3, 4, 20, 6) and PJ.shape == (3, 4, 6, 6)
        assert np.array_equal(PJ, b[6]) and np.array_equal(dx0, b[4]) and not np.array_equal(PJ, c[6])
        assert not PJ[..., :3, 3:].any() and not PJ[..., 3:, :3].any()
        off = PJ - np.diagonal(PJ, axis1=-2, axis2=-1)[..., None] * np.eye(6)
        assert not off.any()  # diagonal unless rotate=True
        assert np.all(np.linalg.eigvalsh(PJ) > 0)
        assert np.array_equal(PJ[..., 3, 3], PJ[..., 4, 4]) and np.array_equal(PJ[..., 4, 4], PJ[..., 5, 5])
        ratio = np.diagonal(PJ, axis1=-2, axis2=-1) / np.diag(prob.J)
        assert 0.5 < ratio.min() and ratio.max() < 2.0 and ratio.std() > 0.01
    _, _, _, _, _, _, PR = workloads.plant_mismatch(2, 3, N=10, rotate=True, seed=7)
    Ib = PR[..., :3, :3]
    assert (Ib - np.diagonal(Ib, axis1=-2, axis2=-1)[..., None] * np.eye(3)).any()  # dense blocks
    assert np.array_equal(Ib, np.swapaxes(Ib, -1, -2)) and np.all(np.linalg.eigvalsh(Ib) > 0)
    z = workloads.plant_mismatch(2, 2, N=10, sigma_inertia=0.0, sigma_mass=0.0)
    assert np.array_equal(z[6], np.broadcast_to(z[0].J, (2, 2, 6, 6)))
    with pytest.raises(ValueError):
        workloads.plant_mismatch(1, 1, kind="so3")


# the host-side checks of BatchedTrackingILQR._check_plant, on a stand-in for the solver (they read self.problem only)
def _checker(kind):
    if kind == "pendulum3d":
        prob = workloads.pendulum_swingup(1)[0]
    elif kind == "so3":
        prob = workloads.so3_tracking(1, N=10)[0]
    else:
        prob = workloads.se3_tracking(1, N=10)[0]
    return types.SimpleNamespace(problem=prob), prob


def test_plant_checks_pick_the_form_and_embed_the_so3_family():
    me, prob = _checker("se3")
    J, pend, form, Sp = BatchedTrackingILQR._check_plant(me, 2, np.broadcast_to(prob.J, (2, 6, 6)), None, per_sample=True)
    assert form == _capi.PLANT_DIAG and Sp == 1 and pend is None and J.shape == (2, 1, 36)
    Jd = np.array(np.broadcast_to(prob.J, (2, 3, 6, 6)))
    Jd[1, 2, 0, 1] = Jd[1, 2, 1, 0] = 0.01
    J, pend, form, Sp = BatchedTrackingILQR._check_plant(me, 2, Jd, None, per_sample=True)
    assert form == _capi.PLANT_DENSE and Sp == 3 and np.array_equal(J.reshape(2, 3, 6, 6), Jd)
    assert BatchedTrackingILQR._check_plant(me, 2, None, None, per_sample=True) is None
    me, prob = _checker("pendulum3d")
    J3 = np.broadcast_to(prob.J[:3, :3], (2, 3, 3))
    J, pend, form, Sp = BatchedTrackingILQR._check_plant(me, 2, J3, [[1.0, 0.5]] * 2, per_sample=False)
    assert np.array_equal(J.reshape(2, 6, 6), np.broadcast_to(prob.J, (2, 6, 6))) and pend.shape == (2, 1, 2)


@pytest.mark.parametrize("case", ["shape", "batch", "nan", "offblock", "asym", "notpd", "pend_missing", "pend_extra",
                                  "pend_nonpos", "pend_shape", "pend_alone"])
def test_plant_checks_refuse(case):
    kind = "pendulum3d" if case.startswith("pend_") and case != "pend_extra" else "se3"
    me, prob = _checker(kind)
    n = 3 if kind == "pendulum3d" else 6
    J = np.array(np.broadcast_to(prob.J[:n, :n], (2, n, n)))
    pend = np.array([[prob.pend_mass, prob.pend_length]] * 2) if kind == "pendulum3d" else None
    if case == "shape":
        J = J[:, :5, :5]
    elif case == "batch":
        J = J[:1]
    elif case == "nan":
        J[0, 0, 0] = np.nan
    elif case == "offblock":
        J[1, 0, 4] = 0.1
    elif case == "asym":
        J[1, 0, 1] = 0.1
    elif case == "notpd":
        J[0, 2, 2] = -0.5
    elif case == "pend_missing":
        pend = None
    elif case == "pend_extra":
        pend = np.ones((2, 2))
    elif case == "pend_nonpos":
        pend[1, 1] = 0.0
    elif case == "pend_shape":
        pend = pend[:, :1]
    elif case == "pend_alone":
        J = None
    with pytest.raises(ValueError):
        BatchedTrackingILQR._check_plant(me, 2, J, pend, per_sample=False)
