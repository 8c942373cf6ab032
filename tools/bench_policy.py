"""What the closed-loop rollouts of the held policy cost (tolg_policy_rollout): S perturbed rollouts per trajectory of a
solved 4096 x 200 SE3 tracking batch, J and status only.

usage: python tools/bench_policy.py [--B 4096] [--N 200] [--S 1,16,64] [--rounds 7] [--iters 20] [--layouts samples,traj]
                                    [--limits | --margins | --actuator] [--out FILE.json]

One process.  The batch is solved once, untimed (multiple shooting, accept-always, 20 iterations), once per sample order of
k_policy_rollout: `samples` (the default order, the samples of one trajectory side by side in a wavefront) and `traj`
(TOLG_POLICY_TRAJ_FAST=1 when the handle is created: trajectory fastest, K3's order).  Then, round after round, every
(S, layout) pair and tolg_rollout(ms = 0, alpha = 0) -- K3 on the same batch, the nearest existing kernel -- are timed in
alternation: `iters` back-to-back calls between two events, through the C ABI (no host-side input checks).  Reported per
pair: the median ms per call over the rounds, min and max, closed-loop knot steps per second (B S N per call), and the HBM
bytes the call has to move at least (inputs, outputs, and the nominal data -- gains, controls, states: 97 doubles per knot
and trajectory -- read once per wavefront that needs it: ceil(S / 16) times in `samples` order, S times in `traj` order).

--limits: instead, per S and in the first layout, tolg_policy_rollout and tolg_policy_rollout_limited back to back in the same
alternating rounds: `unlimited` (tolg_policy_rollout), `box` (the box alone: the input range of every trajectory's unperturbed
sample, which the perturbed ones leave; n_sat and u_excess written) and `box+clearance` (the box and the clearance from K = 8 static keep-out
spheres per trajectory, placed about its nominal path; clearance and its knot written too).  J and status in all three.

--margins: instead, per S and in the first layout, the reports of tolg_policy_rollout_margins added in turn to `box+clearance`
(the limited call above, the base of every ratio): `+pose K=2` and `+pose K=8` (pose_margin and its knot from K pose slots per
trajectory, tilt and view cones alternating, built on its nominal path), `+counts few` (both violation counts too, cones the
nominal clears by 0.2 in the cosine: few pairs (sample, knot) outside) and `+counts most` (cones at the median of the nominal's own cosines
and spheres the nominal grazes: most samples outside at most knots, the worst case for the atomics).  Last, at the middle S,
the alternative the report replaces: policy_rollout(trajectories=True) and the host rollout_margins on the device tensors,
wall clock with a synchronisation, and the bytes of the trajectories it writes.

--actuator: instead, per S and in the first layout, tolg_policy_rollout_margins under the box of --limits (`margins`: J, status,
n_sat, u_excess) and tolg_policy_rollout_actuated with the same box and the same outputs behind a lag of 1.5 knots and a rate
limit of a twentieth of the box's width per knot, at delays of 0, 1 and 4 knots (`actuated D=...`), in the same alternating
rounds; the ratio of each to `margins`.  The batch is solved with the input weight at 10 (ACT_R_SCALE), not the headline's
1e-5: at the headline's gains no sample stays finite behind a knot of delay, and a call that carries NaNs down the horizon
does not cost what a finite one costs."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajectory_optimization_matrix_lie_groups_amd import workloads  # noqa: E402
from _benchlib import add_common_args, emit, event_rounds, print_row, stats_row  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_common_args(ap, "B", "N", "S", "rounds", "iters")
    ap.add_argument("--layouts", default="samples,traj")
    ap.add_argument("--limits", action="store_true", help="time tolg_policy_rollout_limited beside tolg_policy_rollout")
    ap.add_argument("--margins", action="store_true", help="time the reports of tolg_policy_rollout_margins, each added in turn")
    ap.add_argument("--actuator", action="store_true", help="time tolg_policy_rollout_actuated beside tolg_policy_rollout_margins")
    add_common_args(ap, "out")
    a = ap.parse_args(argv)
    a.S = [int(s) for s in a.S.split(",")]
    a.layouts = [x for x in ("samples", "traj") if x in a.layouts.split(",")]
    if a.B < 1 or a.N < 1 or min(a.S) < 1 or a.rounds < 1 or a.iters < 1 or not a.layouts:
        ap.error("B, N, S, rounds, iters >= 1; layouts from samples, traj")
    return a


def nominal_bytes(B, N, m, S, layout):
    per = (13 * m + m + 13) * 8  # gains [K | k], nominal control and state of one knot of one trajectory
    reads = -(-S // 16) if layout == "samples" else S
    return B * N * per * reads


def main(argv=None):
    a = parse_args(argv)
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR

    B, N = a.B, a.N
    # (--actuator: a loop soft enough to stay finite behind four knots of delay, so that both calls time finite samples)
    prob, q, xi, us = workloads.se3_tracking(B, N=N, **(dict(R_scale=ACT_R_SCALE) if a.actuator else {}))
    m = prob.m
    solvers = {}
    for layout in a.layouts:
        os.environ["TOLG_POLICY_TRAJ_FAST"] = "1" if layout == "traj" else "0"
        s = BatchedTrackingILQR(prob, B)
        s.fit_batch(q, xi, us, mode="ms", n_iterations=20, tol_grad_norm=0.0, tol_d_norm=0.0)
        solvers[layout] = s
    os.environ.pop("TOLG_POLICY_TRAJ_FAST", None)
    torch.cuda.synchronize()
    dev = solvers[a.layouts[0]].device
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    f64 = dict(dtype=torch.float64, device=dev)
    inputs = {}
    for S in a.S:
        dx0 = torch.randn(B, S, 12, generator=g, **f64) * 0.05
        w = torch.randn(B, S, N, 6, generator=g, **f64) * 0.01
        inputs[S] = (dx0, w, torch.empty(B, S, **f64), torch.empty(B, S, dtype=torch.int32, device=dev))
    ro = tuple(torch.empty(*shape, **f64) for shape in ((B, N + 1, 4, 4), (B, N + 1, 6), (B, N, m)))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(name):
        if name == "rollout":
            s = solvers[a.layouts[0]]
            return s.lib.tolg_rollout(s._h, 0, 0, 0.0, B, p(ro[0]), p(ro[1]), p(ro[2]), s._stream())
        layout, S = name
        s = solvers[layout]
        dx0, w, J, st = inputs[S]
        return s.lib.tolg_policy_rollout(s._h, B, S, p(dx0), p(w), p(J), p(st), None, None, None, s._stream())

    if a.limits:
        return limits(a, solvers[a.layouts[0]], a.layouts[0], inputs, p)
    if a.actuator:
        return actuator(a, solvers[a.layouts[0]], a.layouts[0], inputs, p)
    if a.margins:
        return margins(a, prob, (q, xi, us), solvers[a.layouts[0]], a.layouts[0], inputs, p)
    names = [(layout, S) for S in a.S for layout in a.layouts] + ["rollout"]
    times = event_rounds(names, call, a.rounds, a.iters)
    rows = []
    for n in names:
        row = dict(kernel="tolg_rollout(ms=0, alpha=0)" if n == "rollout" else "tolg_policy_rollout", **stats_row(times[n]))
        med = row["ms_median"]
        if n == "rollout":
            row.update(S=1, steps_per_s=B * N / (med * 1e-3))
        else:
            layout, S = n
            st = inputs[S][3]
            nb = nominal_bytes(B, N, m, S, layout) + B * S * (12 + N * 6) * 8 + B * S * 12
            row.update(layout=layout, S=S, steps_per_s=B * S * N / (med * 1e-3), hbm_bytes_est=nb,
                       hbm_GBps_est=nb / (med * 1e-3) / 1e9, status_ok=int((st == 0).sum().item()),
                       J_finite=int(torch.isfinite(inputs[S][2]).sum().item()))
        rows.append(row)
        print_row(row)
    res = dict(B=B, N=N, rounds=a.rounds, iters=a.iters, device=torch.cuda.get_device_name(dev), rows=rows)
    emit(res, a.out)
    return res


LIMIT_FORMS = ("unlimited", "box", "box+clearance")
LIMIT_K = 8


def limit_spheres(t, K=LIMIT_K):
    """K static spheres per trajectory about its nominal positions t [B, N+1, 3]: centred 0.5 beside K knots spread over the
    path, radius 0.45 -- the nominal passes 0.05 clear of each, a perturbed sample may not.  [B, K, 4]."""
    import torch
    B, N1 = t.shape[:2]
    knots = torch.linspace(0, N1 - 1, K + 2, device=t.device).long()[1:-1]
    sp = torch.empty(B, K, 4, dtype=t.dtype, device=t.device)
    sp[:, :, :3] = t[:, knots]
    sp[:, :, 2] += 0.5
    sp[:, :, 3] = 0.45
    return sp


def limits(a, s, layout, inputs, p):
    import torch
    B, N = a.B, a.N
    f64 = dict(dtype=torch.float64, device=s.device)
    nom = s.policy_rollout(S=1, trajectories=True)  # the held nominal: the unperturbed sample
    lb, ub = nom.us[:, 0].amin(dim=1).contiguous(), nom.us[:, 0].amax(dim=1).contiguous()
    s.set_al_obstacles(limit_spheres(nom.xs_q[:, 0, :, :3, 3]))
    outs = {S: (torch.empty(B, S, dtype=torch.int32, device=s.device), torch.empty(B, S, **f64), torch.empty(B, S, **f64),
                torch.empty(B, S, dtype=torch.int32, device=s.device)) for S in a.S}

    def call(name):
        S, form = name
        dx0, w, J, st = inputs[S]
        if form == "unlimited":
            return s.lib.tolg_policy_rollout(s._h, B, S, p(dx0), p(w), p(J), p(st), None, None, None, s._stream())
        ns, ex, cl, ck = outs[S]
        clear = (p(cl), p(ck)) if form == "box+clearance" else (None, None)
        return s.lib.tolg_policy_rollout_limited(s._h, B, S, p(dx0), p(w), p(lb), p(ub), p(J), p(st), None, None, None, p(ns),
                                                 p(ex), *clear, s._stream())

    names = [(S, form) for S in a.S for form in LIMIT_FORMS]
    times = event_rounds(names, call, a.rounds, a.iters)
    rows = []
    for S in a.S:
        base = stats_row(times[(S, "unlimited")])
        for form in LIMIT_FORMS:
            row = dict(kernel="tolg_policy_rollout" if form == "unlimited" else "tolg_policy_rollout_limited", form=form,
                       layout=layout, S=S, **stats_row(times[(S, form)]))
            row.update(steps_per_s=B * S * N / (row["ms_median"] * 1e-3), vs_unlimited=row["ms_median"] / base["ms_median"] - 1,
                       unlimited_spread=(base["ms_max"] - base["ms_min"]) / base["ms_median"])
            if form != "unlimited":
                call((S, form))
                torch.cuda.synchronize()
                ns, ex, cl, ck = outs[S]
                row.update(saturated_samples=int((ns > 0).sum().item()), status_ok=int((inputs[S][3] == 0).sum().item()))
                if form == "box+clearance":
                    row.update(K=LIMIT_K, penetrating_samples=int((cl < 0).sum().item()))
            rows.append(row)
            print_row(row)
    s.set_al_obstacles(None)
    res = dict(B=B, N=N, rounds=a.rounds, iters=a.iters, device=torch.cuda.get_device_name(s.device), rows=rows)
    emit(res, a.out)
    return res


ACT_FORMS = ("margins", "actuated D=0", "actuated D=1", "actuated D=4")
ACT_R_SCALE = 10.0  # the input weight of --actuator's batch: at the headline's 1e-5 no sample survives a knot of delay


def actuator(a, s, layout, inputs, p):
    """tolg_policy_rollout_margins under the box of --limits (J, status, n_sat, u_excess) and tolg_policy_rollout_actuated with
    the same box and the same outputs behind a lag of 1.5 knots and a rate limit of a twentieth of the box's width per knot, at
    delays of 0, 1 and 4 knots, in alternating rounds."""
    import math
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import _capi
    B, N = a.B, a.N
    f64 = dict(dtype=torch.float64, device=s.device)
    nom = s.policy_rollout(S=1, trajectories=True)
    lb, ub = nom.us[:, 0].amin(dim=1).contiguous(), nom.us[:, 0].amax(dim=1).contiguous()
    beta = torch.full_like(lb, math.exp(-1.0 / 1.5))
    du = (0.05 * (ub - lb)).clamp(min=1e-6).contiguous()
    acts = {}
    for D in (0, 1, 4):
        st = _capi.Actuator()
        st.d_lb, st.d_ub, st.d_beta, st.d_du_max, st.d_u_init, st.delay = (lb.data_ptr(), ub.data_ptr(), beta.data_ptr(),
                                                                            du.data_ptr(), None, D)
        acts["actuated D=%d" % D] = st
    outs = {S: (torch.empty(B, S, dtype=torch.int32, device=s.device), torch.empty(B, S, **f64),
                torch.empty(B, S, dtype=torch.int32, device=s.device), torch.empty(B, S, **f64)) for S in a.S}
    none6, none3 = (None,) * 6, (None,) * 3

    def call(name, reports=False):
        S, form = name
        dx0, w, J, st = inputs[S]
        ns, ex, nr, gap = outs[S]
        if form == "margins":
            return s.lib.tolg_policy_rollout_margins(s._h, B, S, p(dx0), p(w), p(lb), p(ub), p(J), p(st), None, None, None, p(ns),
                                                     p(ex), *none6, s._stream())
        more = (None, p(nr), p(gap)) if reports else none3
        return s.lib.tolg_policy_rollout_actuated(s._h, B, S, p(dx0), p(w), C.byref(acts[form]), p(J), p(st), None, None, None,
                                                  p(ns), p(ex), *none6, *more, s._stream())

    names = [(S, form) for S in a.S for form in ACT_FORMS]
    times = event_rounds(names, call, a.rounds, a.iters)
    rows = []
    for S in a.S:
        base = stats_row(times[(S, "margins")])
        for form in ACT_FORMS:
            row = dict(kernel="tolg_policy_rollout_margins" if form == "margins" else "tolg_policy_rollout_actuated", form=form,
                       layout=layout, S=S, **stats_row(times[(S, form)]))
            row.update(steps_per_s=B * S * N / (row["ms_median"] * 1e-3), vs_margins=row["ms_median"] / base["ms_median"] - 1,
                       margins_spread=(base["ms_max"] - base["ms_min"]) / base["ms_median"])
            assert call((S, form), reports=True) == 0
            torch.cuda.synchronize()
            ns, ex, nr, gap = outs[S]
            row.update(saturated_samples=int((ns > 0).sum().item()), status_ok=int((inputs[S][3] == 0).sum().item()))
            if form != "margins":
                row.update(rate_limited_samples=int((nr > 0).sum().item()), u_gap_median=float(gap.nanmedian().item()))
            rows.append(row)
            print_row(row)
    res = dict(B=B, N=N, rounds=a.rounds, iters=a.iters, device=torch.cuda.get_device_name(s.device), rows=rows)
    emit(res, a.out)
    return res


MARGIN_FORMS = ("box+clearance", "+pose K=2", "+pose K=8", "+counts few", "+counts most")


def margin_cones(xs_q, K, tight):
    """K pose slots per trajectory on its nominal poses xs_q [B, N+1, 4, 4], tilt cones (even k: the nominal thrust axis at an
    anchor knot) and view cones (odd k: a target 2 ahead of the nominal pose there) alternating; the cosine is the slot's
    smallest nominal cosine less 0.2, or with `tight` the median of its nominal cosines.  Returns ([B, K, 4], kinds)."""
    import torch
    B, N1 = xs_q.shape[:2]
    R, t = xs_q[..., :3, :3], xs_q[..., :3, 3]
    knots = torch.linspace(0, N1 - 1, K + 2, device=xs_q.device).long()[1:-1]
    sl = torch.empty(B, K, 4, dtype=xs_q.dtype, device=xs_q.device)
    kinds = []
    for k, a_ in enumerate(knots.tolist()):
        if k % 2 == 0:
            n = R[:, a_, :, 2]
            cos = (R[:, :, :, 2] * n[:, None]).sum(-1)
            sl[:, k, :3] = n
        else:
            tg = t[:, a_] + 2.0 * R[:, a_, :, 0]
            d = (R * (tg[:, None] - t)[..., :, None]).sum(-2)
            cos = d[..., 0] / d.norm(dim=-1)
            sl[:, k, :3] = tg
        sl[:, k, 3] = (cos.median(dim=1).values if tight else cos.amin(dim=1) - 0.2).clamp(-0.99, 0.99)
        kinds.append(k % 2)
    return sl, kinds


def margins(a, prob, start, s2, layout, inputs, p):
    import time
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, rollout_margins
    B, N = a.B, a.N
    dev = s2.device
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    os.environ["TOLG_POLICY_TRAJ_FAST"] = "1" if layout == "traj" else "0"
    handles = {"K2": s2}
    for name in ("K8", "K8 tight"):  # a handle per slot set: attaching between timed calls would time the packing
        h = BatchedTrackingILQR(prob, B)
        h.fit_batch(*start, mode="ms", n_iterations=20, tol_grad_norm=0.0, tol_d_norm=0.0)
        handles[name] = h
    os.environ.pop("TOLG_POLICY_TRAJ_FAST", None)
    nom = s2.policy_rollout(S=1, trajectories=True)
    lb, ub = nom.us[:, 0].amin(dim=1).contiguous(), nom.us[:, 0].amax(dim=1).contiguous()
    xq = nom.xs_q[:, 0]
    slots = {}
    for name, h in handles.items():
        sp = limit_spheres(xq[:, :, :3, 3])
        if name == "K8 tight":
            sp[:, :, 3] = 0.5  # the nominal grazes every sphere
        h.set_al_obstacles(sp)
        sl, kinds = margin_cones(xq, 2 if name == "K2" else 8, name == "K8 tight")
        h.set_al_pose_constraints(sl, kinds=kinds)
        slots[name] = (sp, sl, kinds)
    outs = {S: (torch.empty(B, S, **i32), torch.empty(B, S, **f64), torch.empty(B, S, **f64), torch.empty(B, S, **i32),
                torch.empty(B, S, **f64), torch.empty(B, S, **i32), torch.empty(B, N + 1, **i32), torch.empty(B, N + 1, **i32))
            for S in a.S}
    which = {"box+clearance": ("K2", 4), "+pose K=2": ("K2", 6), "+pose K=8": ("K8", 6), "+counts few": ("K8", 8),
             "+counts most": ("K8 tight", 8)}

    def call(name):
        S, form = name
        dx0, w, J, st = inputs[S]
        hname, n_out = which[form]
        h = handles[hname]
        o = [p(t) for t in outs[S][:n_out]]
        if form == "box+clearance":
            return h.lib.tolg_policy_rollout_limited(h._h, B, S, p(dx0), p(w), p(lb), p(ub), p(J), p(st), None, None, None, *o,
                                                     h._stream())
        o += [None] * (8 - n_out)
        return h.lib.tolg_policy_rollout_margins(h._h, B, S, p(dx0), p(w), p(lb), p(ub), p(J), p(st), None, None, None, *o,
                                                 h._stream())

    names = [(S, form) for S in a.S for form in MARGIN_FORMS]
    times = event_rounds(names, call, a.rounds, a.iters)
    rows = []
    for S in a.S:
        base = stats_row(times[(S, MARGIN_FORMS[0])])
        for form in MARGIN_FORMS:
            row = dict(kernel="tolg_policy_rollout_limited" if form == MARGIN_FORMS[0] else "tolg_policy_rollout_margins",
                       form=form, layout=layout, S=S, **stats_row(times[(S, form)]))
            row.update(vs_base=row["ms_median"] / base["ms_median"] - 1, base_spread=(base["ms_max"] - base["ms_min"]) / base["ms_median"])
            assert call((S, form)) == 0
            torch.cuda.synchronize()
            o = outs[S]
            if which[form][1] >= 6:
                row.update(outside_a_cone=int((o[4] < 0).sum().item()))
            if which[form][1] == 8:
                row.update(viol_pos_share=float(o[6].sum().item()) / (B * S * (N + 1)),
                           viol_pose_share=float(o[7].sum().item()) / (B * S * (N + 1)))
            rows.append(row)
            print_row(row)
    # the alternative: trajectories to HBM, then the host function on the device tensors
    S = a.S[len(a.S) // 2]
    dx0, w, _, _ = inputs[S]
    h = handles["K8"]
    sp, sl, kinds = slots["K8"]
    wall = []
    J, st = inputs[S][2:]
    tr = (torch.empty(B, S, N + 1, 4, 4, **f64), torch.empty(B, S, N + 1, 6, **f64), torch.empty(B, S, N, prob.m, **f64))
    for _ in range(3):  # (through the C ABI as the timed calls above: no host-side input checks)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert h.lib.tolg_policy_rollout_limited(h._h, B, S, p(dx0), p(w), p(lb), p(ub), p(J), p(st), p(tr[0]), p(tr[1]), p(tr[2]),
                                                 None, None, None, None, h._stream()) == 0
        rep = rollout_margins(tr[0], obstacles=sp, pose_slots=sl, pose_kinds=kinds)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    row = dict(kernel="policy_rollout(trajectories=True) + rollout_margins", S=S, ms_wall_min=min(wall), ms_wall_max=max(wall),
               trajectory_bytes=B * S * ((N + 1) * 22 + N * prob.m) * 8, outside_a_cone=int((rep["pose_margin"] < 0).sum().item()))
    rows.append(row)
    print_row(row)
    for h in handles.values():
        h.set_al_obstacles(None)
        h.set_al_pose_constraints(None)
    res = dict(B=B, N=N, rounds=a.rounds, iters=a.iters, device=torch.cuda.get_device_name(dev), rows=rows)
    emit(res, a.out)
    return res


if __name__ == "__main__":
    main()
