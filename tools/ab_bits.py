"""Do two builds of the library compute the same bits?  One sha256 per case over what a solve (xs_q, xs_xi, us, J_hist,
alpha_hist, iters, status), a closed-loop rollout (J, status, xs_q, xs_xi, us; under a box with clearance also n_sat, u_excess,
clearance, clearance_knot) or a receding-horizon step (every tensor of mpc_advance's dict) returns, on small cases that between
them run every rollout kernel: the fused launch, K3 alone, the one- and two-wave line-search stages of both searches, the
statement-form LINEAR steps, the pendulum, a dense inertia, the closed loop and the receding-horizon step with and without a
plant, free and under an actuator box (a case whose box moves no input fails: it would not have run the clamp).

usage: python tools/ab_bits.py                    the cases on the library TOLG_HIP_LIB selects (default: the in-tree one)
       python tools/ab_bits.py LIB [LIB ...]      each LIB (a path, or `intree`) in a fresh child process under its own time
                                                  limit, a child started only if the one before it exited 0; then the cases
                                                  whose digests differ between the first LIB and each later one (exit 1 if any)
Give a library twice to see which cases repeat at all."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_SECONDS = 240


def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        a = t.detach().cpu().contiguous().numpy()
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def _fit_fields(r):
    return [r.xs_q, r.xs_xi, r.us, r.J_hist, r.alpha_hist, r.iters, r.status]


def cases():
    """[(name, thunk -> list of tensors)]"""
    import numpy as np
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, TrackingProblem, workloads

    def fit(prob, q, xi, us, modes, env=None, K=6, **kw):
        out = []
        for k, v in (env or {}).items():
            os.environ[k] = v
        try:
            for mode in modes:
                r = BatchedTrackingILQR(prob, q.shape[0]).fit_batch(q, xi, us, mode=mode, n_iterations=K, tol_grad_norm=0.0,
                                                                    tol_d_norm=0.0, **kw)
                torch.cuda.synchronize()
                out += _fit_fields(r)
        finally:
            for k in env or {}:
                os.environ.pop(k, None)
        return out

    def tracking(make, B, N, modes, env=None, **kw):
        return lambda: fit(*make(B, N=N), modes, env, **kw)

    def dense_inertia():
        prob, q, xi, us = workloads.se3_tracking(20, N=30)
        A = np.array([[0.10, -0.05, 0.02], [0.03, 0.12, -0.04], [-0.02, 0.06, 0.09]])
        Jd = np.array(prob.J, dtype=float).copy()
        Jd[:3, :3] += A @ A.T
        Jd[3:, 3:] += 0.5 * (A @ A.T)
        pd = TrackingProblem("se3", Jd, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref)
        return fit(pd, q, xi, us, ["ms"], line_search=True)

    def solved(kind):
        """The closed-loop cases' workload and solve: B = 9, S = 3 is 27 quads, so the last wavefront is partial and replays
        the last sample"""
        prob, q, xi, us, dx0, noise, plant_J = workloads.plant_mismatch(9, 3, kind=kind, N=20, rotate=True)
        s = BatchedTrackingILQR(prob, 9)
        r = s.fit_batch(q, xi, us, mode="ms", n_iterations=6, tol_grad_norm=0.0, tol_d_norm=0.0)
        torch.cuda.synchronize()
        return prob, s, r.xs_q.cpu().numpy(), r.us.cpu().numpy(), dx0, noise, plant_J

    def policy(kind):
        def run():
            prob, s, xs_q, us, dx0, noise, plant_J = solved(kind)
            out = []
            for plant in (None, plant_J):
                r = s.policy_rollout(dx0=dx0, noise=noise, trajectories=True, plant_J=plant)
                torch.cuda.synchronize()
                out += [r.J, r.status, r.xs_q, r.xs_xi, r.us]
            return out
        return run

    def policy_limited(kind):
        def run():
            prob, s, xs_q, us, dx0, noise, plant_J = solved(kind)
            lb, ub = us.min(axis=1), us.max(axis=1)  # the nominal input range: perturbed samples leave it somewhere
            # K = 3 static spheres about the nominal position at the middle knot: one touches it from above, two stand off
            off, rad = np.array([[-0.4, 2.0, 0.6], [1.5, 0.3, 0.0], [0.0, 0.0, 0.4]]), np.array([0.7, 0.5, 0.4])
            sp = np.concatenate([xs_q[:, xs_q.shape[1] // 2, None, :3, 3] + off[None], np.broadcast_to(rad, (9, 3))[..., None]], axis=2)
            s.set_al_obstacles(sp)
            out = []
            for plant in (None, plant_J):
                r = s.policy_rollout(dx0=dx0, noise=noise, trajectories=True, plant_J=plant, u_lb=lb, u_ub=ub, clearance=True)
                torch.cuda.synchronize()
                if int(r.n_sat.sum()) == 0:
                    raise RuntimeError("the box moved no input: the clamp did not run")
                out += [r.J, r.status, r.xs_q, r.xs_xi, r.us, r.n_sat, r.u_excess, r.clearance, r.clearance_knot]
            return out
        return run

    def advance(kind):
        def run():
            prob, s, xs_q, us, dx0, noise, plant_J = solved(kind)
            # the middle half of the nominal input range: u*_0 of some trajectory is outside it
            lo, hi = us.min(axis=1), us.max(axis=1)
            lb, ub = lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo)
            diag = np.array(np.broadcast_to(np.asarray(prob.J, float), (9, 6, 6)))
            diag[:, range(3), range(3)] *= np.random.default_rng(2).uniform(0.8, 1.2, (9, 3))  # a diagonal plant per trajectory
            out, moved = [], 0
            for plant in (None, diag, plant_J[:, 0]):
                for box in ({}, dict(u_lb=lb, u_ub=ub)):
                    J_cl = torch.zeros(9, dtype=torch.float64, device=s.device)
                    a = s.mpc_advance(noise[:, 0, 0], J_cl=J_cl, plant_J=plant, **box)
                    torch.cuda.synchronize()
                    moved += int(a["n_sat"].sum()) if box else 0
                    out += [a[k] for k in sorted(a)]
            if moved == 0:
                raise RuntimeError("the box moved no input: the clamp did not run")
            return out
        return run

    se3, drone = workloads.se3_tracking, workloads.drone_tracking
    return [
        ("se3 B37 N45 ms line-search", tracking(se3, 37, 45, ["ms"], line_search=True)),
        ("se3 B21 N30 ss", tracking(se3, 21, 30, ["ss"], line_search=True)),
        ("se3 B21 N30 ss one-wave", tracking(se3, 21, 30, ["ss"], {"TOLG_LS_ONEWAVE": "1"}, line_search=True)),
        ("drone B10 N60 ms line-search", tracking(drone, 10, 60, ["ms"], line_search=True)),
        ("drone B18 N40 ss", tracking(drone, 18, 40, ["ss"], line_search=True)),
        ("pendulum B11 xi0_scale 1 ms, ss line-search", lambda: fit(*workloads.pendulum_swingup(11, xi0_scale=1.0), ["ms", "ss"],
                                                                line_search=True)),
        ("se3 dense inertia B20 N30 ms line-search", dense_inertia),
        ("se3 B18 N7 ms accept-always split", tracking(se3, 18, 7, ["ms"], schedule="split")),
        ("se3 B18 N7 ms accept-always auto", tracking(se3, 18, 7, ["ms"], schedule="auto")),
        ("se3 B13 N25 linear split line-search ms, ss", tracking(se3, 13, 25, ["ms", "ss"], rollout="linear", schedule="split",
                                                                line_search=True)),
        ("se3 B9 N20 policy_rollout S3, model and dense plant", policy("se3")),
        ("drone B9 N20 policy_rollout S3, model and dense plant", policy("drone")),
        ("se3 B9 N20 policy_rollout S3 under a box with clearance, model and dense plant", policy_limited("se3")),
        ("drone B9 N20 policy_rollout S3 under a box with clearance, model and dense plant", policy_limited("drone")),
        ("se3 B9 N20 mpc_advance free and under a box: model, diagonal and dense plant", advance("se3")),
        ("drone B9 N20 mpc_advance free and under a box: model, diagonal and dense plant", advance("drone")),
    ]


def run_cases():
    from trajectory_optimization_matrix_lie_groups_amd import _build
    print("library %s" % _build.lib_path(), flush=True)
    for name, thunk in cases():
        print("%s  %s" % (_digest(thunk()), name), flush=True)


def run_libraries(libs):
    runs = []
    for lib in libs:
        env = dict(os.environ)
        env.pop("TOLG_HIP_LIB", None)
        if lib != "intree":
            env["TOLG_HIP_LIB"] = os.path.abspath(lib)
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__)], env=env,
                           stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print("%s: exit %d -- nothing further is started" % (lib, p.returncode))
            return 2
        runs.append({ln[66:]: ln[:64] for ln in p.stdout.splitlines() if len(ln) > 66 and ln[64:66] == "  "})
    bad = 0
    for lib, run in zip(libs[1:], runs[1:]):
        diff = [n for n in runs[0] if run.get(n) != runs[0][n]]
        bad += len(diff)
        print("%s against %s: %d of %d cases differ%s" % (lib, libs[0], len(diff), len(runs[0]), "".join("\n  " + n for n in diff)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(run_libraries(sys.argv[1:]) if len(sys.argv) > 1 else run_cases())
