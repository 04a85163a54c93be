"""Quadcopter trim for tests/test_trim_hard.py and tests/test_trim_hard_gpu.py: the operating points, a NumPy restatement of the
iteration of quad_trim_kernel (zopt_amd/csrc/linearize.hip: Levenberg-Marquardt on the 8 residuals of rigidBodyDynamics in the 9
unknowns (p, q, r, phi, theta, thrust, mx, my, mz), from z0 = (0,0,0,0,0, g,0,0,0), damping 1e-3 divided by 10 on an accepted
step and multiplied by 10 on a rejected one, at most 200 outer and 12 inner iterations), and the residual in long double.

The restatement tells which operating points are trimmable at all: with fa_i = -0.2 v_i - 0.05 v_i^2 the horizontal drag must be
carried by tilting the thrust, and |(fa_0, fa_1)| >= m g cannot be (theta -> -pi/2: (21, 0, 0) and (25, 0, 0))."""
import numpy as np

from oracle import zopt_oracle as zo
from tests import model_hp_ref as hp

MG = hp.MASS * hp.G
WINDS = [(0.0, 0.0, 0.0), (1.0, 0.5, -0.5), (-2.0, 3.0, 0.3), (5.0, -3.0, 1.0)]     # body winds; the first: still air
FAILING = np.array([[25.0, 0.0, 0.0], [21.0, 0.0, 0.0]])


def drag(v):
    return -0.2 * v - 0.05 * v * v


def family(count=300, seed=11):
    """hover, the axis points and `count` seeded uvw with |(fa_0, fa_1)| <= 0.9 m g, |w| <= 19"""
    rng = np.random.default_rng(seed)
    pts = [np.zeros(3)] + [s * a * e + 0.0 for e in np.eye(3) for a in (3.0, 15.0) for s in (1.0, -1.0)]
    out = []
    while len(out) < count:
        v = rng.uniform(-19.0, 19.0, 3)
        if np.hypot(drag(v[0]), drag(v[1])) <= 0.9 * MG:
            out.append(v)
    pts = [p for p in pts if np.hypot(drag(p[0]), drag(p[1])) <= 0.9 * MG]
    return np.array(pts + out)


def residual_ld(xTrim, uTrim, wind):
    """|rigidBodyDynamics(x, u)| in long double at the returned point: (b,)"""
    r = hp.values_ld("rigid", np.atleast_2d(xTrim), np.atleast_2d(uTrim), wind)
    return np.sqrt(np.sum(r * r, axis=1))


def lm_trim(uvw, wind=(0.0, 0.0, 0.0), tol=1e-9):
    """the kernel's iteration for one operating point in fp64 NumPy -> (z (9,), residual norm, accepted outer iterations)"""
    wind = np.asarray(wind, dtype=np.float64)

    def res(z):
        return zo.quad_rigidBodyDynamics(np.concatenate([uvw, z[:5]]), z[5:], wind_body=wind)

    z = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 9.807, 0.0, 0.0, 0.0])
    with np.errstate(all="ignore"):
        r = res(z)
        cost, lam, its = float(r @ r), 1e-3, 0
        for _ in range(200):
            if not cost > tol * tol * 1e-6:
                break
            _, fx, fu = zo.jacobians(lambda x, u: zo.quad_rigidBodyDynamics(x, u, wind_body=wind), np.concatenate([uvw, z[:5]]), z[5:])
            J = np.hstack([fx[:, 3:8], fu])
            A, b = J.T @ J, J.T @ r
            accepted = False
            for _ in range(12):
                M = A + lam * np.diag(np.diag(A) + 1e-9)
                try:
                    Lc = np.linalg.cholesky(M)
                    d = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
                    pd = True
                except np.linalg.LinAlgError:
                    pd, d = False, np.zeros(9)
                zn = z + d
                rn = res(zn)
                cn = float(rn @ rn)
                if pd and cn < cost:
                    z, r, cost = zn, rn, cn
                    lam = lam * 0.1 if lam > 1e-10 else lam
                    accepted = True
                    break
                lam *= 10.0
            if not accepted:
                break
            its += 1
    return z, float(np.sqrt(cost)), its
