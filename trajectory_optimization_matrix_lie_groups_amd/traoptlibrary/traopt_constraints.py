"""Constraints with the reference's interface (traoptlibrary/traopt_constraints.py:5-169)."""
import abc

import numpy as np


class BaseConstraint():
    """traopt_constraints.py:5-63"""

    @abc.abstractmethod
    def g(self, x, u, i, terminal=False, *args, **kwargs):
        raise NotImplementedError

    @abc.abstractmethod
    def g_x(self, x, u, i, terminal=False, *args, **kwargs):
        raise NotImplementedError

    @abc.abstractmethod
    def g_u(self, x, u, i, terminal=False, *args, **kwargs):
        raise NotImplementedError


class InputConstraint(BaseConstraint):
    """Box input constraint g = [lb - u; u - ub] <= 0 (traopt_constraints.py:66-169).  The values are
    trivial affine maps of u (host code in the reference as well); the augmented-Lagrangian terms
    built from them run on the device (tolg_set_al / tolg_al_update).  input_lb, input_ub [m], or [N, m]: a box per knot,
    g(x, u, i) then uses row i (on the device tolg_set_al_box's per-knot form / tolg_al_update_state)."""

    def __init__(self, input_lb, input_ub, state_size=(6, 6), action_size=6):
        self._state_size = state_size[0] + state_size[1]
        self._error_state_size = state_size[0]
        self._vel_state_size = state_size[1]
        self._action_size = action_size
        self._lb = input_lb
        self._ub = input_ub
        self._constr_size = 2 * action_size

    lb = property(lambda self: self._lb)
    ub = property(lambda self: self._ub)
    constr_size = property(lambda self: self._constr_size)
    state_size = property(lambda self: self._state_size)
    error_state_size = property(lambda self: self._error_state_size)
    vel_state_size = property(lambda self: self._vel_state_size)
    action_size = property(lambda self: self._action_size)

    def g(self, x, u, i, terminal=False, *args, **kwargs):
        if terminal:
            return np.zeros((self._constr_size,))
        lb, ub = np.asarray(self.lb), np.asarray(self.ub)
        if lb.ndim == 2:  # [N, m]: the box of knot i
            lb, ub = lb[i], ub[i]
        return np.concatenate([lb - u, u - ub])

    def g_x(self, x, u, i, terminal=False, *args, **kwargs):
        return np.zeros([self.constr_size, self.state_size])

    def g_u(self, x, u, i, terminal=False, *args, **kwargs):
        if terminal:
            return np.zeros([self.constr_size, self.action_size])
        return np.vstack([-1 * np.identity(self.action_size), np.identity(self.action_size)])


class SphereObstacleConstraint(BaseConstraint):
    """Keep-out spheres g_k(x) = r_k^2 - |t - c_k|^2 <= 0 on the translation t of the pose X = (R, t) of x = [X, xi], at every
    knot, terminal included; the reference's BaseConstraint interface (traopt_constraints.py:5-63).  In the error coordinates
    of the SE(3) costs (right perturbation X Exp(delta), twist order [omega, v]) g_x = [0, -2 (t - c)^T R, 0], g_u = 0.
    The augmented-Lagrangian terms of these spheres run on the device (tolg_set_al_obstacles / tolg_al_update_state)."""

    def __init__(self, centers, radii, state_size=(6, 6), action_size=6):
        self._centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
        self._radii = np.asarray(radii, dtype=np.float64).reshape(-1)
        if self._radii.shape[0] != self._centers.shape[0]:
            raise ValueError("one radius per center")
        self._state_size = state_size[0] + state_size[1]
        self._error_state_size = state_size[0]
        self._vel_state_size = state_size[1]
        self._action_size = action_size
        self._constr_size = self._radii.shape[0]

    centers = property(lambda self: self._centers)
    radii = property(lambda self: self._radii)
    constr_size = property(lambda self: self._constr_size)
    state_size = property(lambda self: self._state_size)
    error_state_size = property(lambda self: self._error_state_size)
    vel_state_size = property(lambda self: self._vel_state_size)
    action_size = property(lambda self: self._action_size)

    def obstacles(self):
        """The spheres as rows (cx, cy, cz, r) [K, 4]: the layout of tolg_set_al_obstacles."""
        return np.concatenate([self._centers, self._radii[:, None]], axis=1)

    def _at(self, i):
        """(centers [K, 3], radii [K]) at knot i"""
        return self._centers, self._radii

    def g(self, x, u, i, terminal=False, *args, **kwargs):
        c, r = self._at(i)
        d = np.asarray(x[0])[:3, 3][None] - c
        return r ** 2 - np.sum(d * d, axis=1)

    def g_x(self, x, u, i, terminal=False, *args, **kwargs):
        X = np.asarray(x[0])
        d = X[:3, 3][None] - self._at(i)[0]
        gx = np.zeros((self._constr_size, self._state_size))
        gx[:, 3:6] = -2.0 * d @ X[:3, :3]
        return gx

    def g_u(self, x, u, i, terminal=False, *args, **kwargs):
        return np.zeros((self._constr_size, self._action_size))


class MovingSphereObstacleConstraint(SphereObstacleConstraint):
    """Keep-out spheres whose geometry depends on the knot: g_k(x, i) = r_ik^2 - |t - c_ik|^2 <= 0 with centers [N+1, K, 3] and
    radii [N+1, K] (or [K]: the same at every knot), terminal knot included.  g and g_x are SphereObstacleConstraint's on the
    geometry of knot i (_at); on the device these are the terms of tolg_set_al_obstacles_moving."""

    def __init__(self, centers, radii, state_size=(6, 6), action_size=6):
        c = np.asarray(centers, dtype=np.float64)
        if c.ndim != 3 or c.shape[2] != 3:
            raise ValueError("centers has shape %s, expected (N+1, K, 3)" % (c.shape,))
        r = np.asarray(radii, dtype=np.float64)
        if r.shape not in (c.shape[:2], c.shape[1:2]):
            raise ValueError("radii has shape %s, expected (N+1, K) or (K,)" % (r.shape,))
        super().__init__(c[0], np.broadcast_to(r, c.shape[:2])[0], state_size, action_size)  # (sizes; knot 0's geometry)
        self._centers = c.copy()                             # [N+1, K, 3]
        self._radii = np.broadcast_to(r, c.shape[:2]).copy()  # [N+1, K]

    def obstacles(self):
        """The spheres as rows (cx, cy, cz, r) per knot [N+1, K, 4]: a trajectory's slice of tolg_set_al_obstacles_moving."""
        return np.concatenate([self._centers, self._radii[..., None]], axis=2)

    def _at(self, i):
        return self._centers[i], self._radii[i]


class PositionObstacleConstraint(BaseConstraint):
    """Position constraints of a kind per slot (tolg_set_al_obstacle_kinds), beside SphereObstacleConstraint and with its
    interface: obstacles [K, 4], or [N+1, K, 4] with the geometry of every knot, rows (f0, f1, f2, f3) read per kind, kinds a
    length-K sequence of 0..3.  With d = t - (f0, f1, f2):
      0 keep-out sphere  g = r^2 - |d|^2          grad_t g = -2 d
      1 keep-in sphere   g = |d|^2 - r^2          grad_t g = 2 d
      2 half-space       g = n.t - o, |n| = 1     grad_t g = n
      3 vertical column  g = r^2 - (dx^2 + dy^2)  grad_t g = -2 (dx, dy, 0)
    In the error coordinates (X Exp(delta), twist order [omega, v]) g_x = [0, (grad_t g)^T R, 0], g_u = 0."""

    def __init__(self, obstacles, kinds, state_size=(6, 6), action_size=6):
        o = np.asarray(obstacles, dtype=np.float64)
        if o.ndim not in (2, 3) or o.shape[-1] != 4:
            raise ValueError("obstacles has shape %s, expected (K, 4) or (N+1, K, 4)" % (o.shape,))
        k = np.asarray(kinds)
        if k.shape != (o.shape[-2],) or not np.issubdtype(k.dtype, np.integer) or np.any(k < 0) or np.any(k > 3):
            raise ValueError("kinds: one of 0..3 per slot")
        self._obs = o.copy()
        self._kinds = k.astype(np.int64)
        self._state_size = state_size[0] + state_size[1]
        self._error_state_size = state_size[0]
        self._vel_state_size = state_size[1]
        self._action_size = action_size
        self._constr_size = o.shape[-2]

    kinds = property(lambda self: self._kinds)
    constr_size = property(lambda self: self._constr_size)
    state_size = property(lambda self: self._state_size)
    error_state_size = property(lambda self: self._error_state_size)
    vel_state_size = property(lambda self: self._vel_state_size)
    action_size = property(lambda self: self._action_size)

    def obstacles(self):
        """The slots as given, [K, 4] or [N+1, K, 4]: a trajectory's slice of tolg_set_al_obstacles(_moving)."""
        return self._obs

    def _rows(self, x, i):
        """(g [K], grad_t g [K, 3]) at knot i"""
        o = self._obs if self._obs.ndim == 2 else self._obs[i]
        t = np.asarray(x[0])[:3, 3]
        kd = self._kinds
        d = t[None] - o[:, :3]
        d[kd == 3, 2] = 0.0
        g = o[:, 3] ** 2 - np.sum(d * d, axis=1)
        grad = -2.0 * d
        g[kd == 1], grad[kd == 1] = -g[kd == 1], -grad[kd == 1]
        hs = kd == 2
        g[hs], grad[hs] = o[hs, :3] @ t - o[hs, 3], o[hs, :3]
        return g, grad

    def g(self, x, u, i, terminal=False, *args, **kwargs):
        return self._rows(x, i)[0]

    def g_x(self, x, u, i, terminal=False, *args, **kwargs):
        gx = np.zeros((self._constr_size, self._state_size))
        gx[:, 3:6] = self._rows(x, i)[1] @ np.asarray(x[0])[:3, :3]
        return gx

    def g_u(self, x, u, i, terminal=False, *args, **kwargs):
        return np.zeros((self._constr_size, self._action_size))


class PoseConstraint(BaseConstraint):
    """Pose constraints of a kind per slot (tolg_set_al_pose_constraints), with the interface of the classes above: slots
    [K, 4], or [N+1, K, 4] with the geometry of every knot, kinds a length-K sequence of 0..1.  Body axes e3 = (0, 0, 1), the
    thrust axis, and e1 = (1, 0, 0), forward; X = (R, t) the pose of x = [X, xi]:
      0 tilt cone  fields (nx, ny, nz, c), |n| = 1   g = c - n^T R e3                    g_omega = (R^T n) x e3   g_v = 0
      1 view cone  fields (px, py, pz, c)            g = c |b| - e1^T b, b = R^T (p - t)   g_omega = b x e1         g_v = e1 - c b / |b|
    In the error coordinates (X Exp(delta), twist order [omega, v]) g_x = [g_omega, g_v, 0], g_u = 0.  The tilt gradient
    vanishes at the antipode of the axis; the view row is not differentiable at t = p."""

    def __init__(self, slots, kinds, state_size=(6, 6), action_size=6):
        o = np.asarray(slots, dtype=np.float64)
        if o.ndim not in (2, 3) or o.shape[-1] != 4:
            raise ValueError("slots has shape %s, expected (K, 4) or (N+1, K, 4)" % (o.shape,))
        k = np.asarray(kinds)
        if k.shape != (o.shape[-2],) or not np.issubdtype(k.dtype, np.integer) or np.any(k < 0) or np.any(k > 1):
            raise ValueError("kinds: one of 0..1 per slot")
        self._slots = o.copy()
        self._kinds = k.astype(np.int64)
        self._state_size = state_size[0] + state_size[1]
        self._error_state_size = state_size[0]
        self._vel_state_size = state_size[1]
        self._action_size = action_size
        self._constr_size = o.shape[-2]

    kinds = property(lambda self: self._kinds)
    constr_size = property(lambda self: self._constr_size)
    state_size = property(lambda self: self._state_size)
    error_state_size = property(lambda self: self._error_state_size)
    vel_state_size = property(lambda self: self._vel_state_size)
    action_size = property(lambda self: self._action_size)

    def slots(self):
        """The slots as given, [K, 4] or [N+1, K, 4]: a trajectory's slice of tolg_set_al_pose_constraints."""
        return self._slots

    def _rows(self, x, i):
        """(g [K], g_omega [K, 3], g_v [K, 3]) at knot i"""
        o = self._slots if self._slots.ndim == 2 else self._slots[i]
        X = np.asarray(x[0])
        R, t = X[:3, :3], X[:3, 3]
        e1, e3 = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
        g, gw, gv = np.empty(len(o)), np.zeros((len(o), 3)), np.zeros((len(o), 3))
        for k, (f, kd) in enumerate(zip(o, self._kinds)):
            if kd == 0:
                a = R.T @ f[:3]
                g[k], gw[k] = f[3] - a[2], np.cross(a, e3)
            else:
                b = R.T @ (f[:3] - t)
                nb = np.sqrt(b @ b)
                g[k], gw[k], gv[k] = f[3] * nb - b[0], np.cross(b, e1), e1 - f[3] * b / nb
        return g, gw, gv

    def g(self, x, u, i, terminal=False, *args, **kwargs):
        return self._rows(x, i)[0]

    def g_x(self, x, u, i, terminal=False, *args, **kwargs):
        _, gw, gv = self._rows(x, i)
        gx = np.zeros((self._constr_size, self._state_size))
        gx[:, 0:3], gx[:, 3:6] = gw, gv
        return gx

    def g_u(self, x, u, i, terminal=False, *args, **kwargs):
        return np.zeros((self._constr_size, self._action_size))


class ConstraintStack(BaseConstraint):
    """Several constraints as one: g, g_x, g_u concatenated in the order given."""

    def __init__(self, *constraints):
        if not constraints:
            raise ValueError("ConstraintStack needs at least one constraint")
        self.constraints = tuple(constraints)
        self._constr_size = sum(c.constr_size for c in constraints)
        self._state_size = constraints[0].state_size
        self._action_size = constraints[0].action_size

    constr_size = property(lambda self: self._constr_size)
    state_size = property(lambda self: self._state_size)
    action_size = property(lambda self: self._action_size)

    def g(self, x, u, i, terminal=False, *args, **kwargs):
        return np.concatenate([c.g(x, u, i, terminal) for c in self.constraints])

    def g_x(self, x, u, i, terminal=False, *args, **kwargs):
        return np.vstack([c.g_x(x, u, i, terminal) for c in self.constraints])

    def g_u(self, x, u, i, terminal=False, *args, **kwargs):
        return np.vstack([c.g_u(x, u, i, terminal) for c in self.constraints])
