"""The yardstick and the comparison of tests/test_mpc_closed_loop_gpu.py (and of its child process); a helper module, not collected as a test.

The yardstick of `lqrMpc.simulate` is the receding-horizon loop written out in Python over `lqrMpc.solve` (`loop` below), run on a SECOND
lqrMpc object built from the same data -- the behaviour `solve` has without `simulate`, which tests/test_mpc_iterates_gpu.py ties to the NumPy
ADMM.  `hold` asks of every instance and every step: the same status string, the same iteration count, and states, inputs and
predictions within TOL * max(1, max |loop's value|) (TOL = 1e-9, the suite's iterate tolerance); it prints the largest absolute difference."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from tests.mpc_iterates_cases import TOL, _random


def problem(mpcUtils, data, N):
    A, B, Q, R, Qf, xl, xu, ul, uu = data
    return mpcUtils.lqrMpc(A, B, Q, R, N, xl, xu, ul, uu, Qf=Qf)


def random_pair(mpcUtils, n, m, N, nb, seed=None):
    """two lqrMpc objects of the random stable problem of tests/mpc_iterates_cases.py (state box 4, input box 0.15) and its `nb` starts"""
    data, x0 = _random(n, m, N, 1000 * n + 10 * m + N if seed is None else seed, nb)
    return problem(mpcUtils, data, N), problem(mpcUtils, data, N), x0, data


def loop(prob, x0, steps, disturbance=None, clip_tol=1e-6, xRef=None, uRef=None, warm_start="shift", **opts):
    """the loop `simulate` documents, over prob.solve, on host arrays"""
    N, n = prob.N, prob._n_user
    x0 = np.asarray(x0, dtype=np.float64)
    leads = [x0.shape[:-1]] + [np.shape(X)[:-2] for X in (disturbance, xRef, uRef) if X is not None]
    lead = np.broadcast_shapes(*leads, *(() if prob.P is None else (prob.P,)))
    lb, ub = prob.x_lb[..., :n], prob.x_ub[..., :n]
    clip = (lambda v: v) if clip_tol is None else (lambda v: np.clip(v, lb + clip_tol, ub - clip_tol))
    x = np.array(np.broadcast_to(x0, lead + (n,)))
    xs, us, st, its, px, pu = [], [], [], [], [], []
    for s in range(steps):
        x = clip(x)
        xs.append(x)
        window = {}
        if xRef is not None:
            window["xRef"] = np.asarray(xRef)[..., s:s + N + 1, :]
        if uRef is not None:
            window["uRef"] = np.asarray(uRef)[..., s:s + N, :]
        u, traj, status = prob.solve(x, warm_start=(False if s == 0 else warm_start), **window, **opts)
        us.append(np.asarray(u))
        st.append(np.asarray(status, dtype=object))
        its.append(np.asarray(prob.last_iterations).copy())
        px.append(np.asarray(traj.xTraj))
        pu.append(np.asarray(traj.uTraj))
        x = px[-1][..., 1, :]
        if disturbance is not None:
            x = x + np.asarray(disturbance)[..., s, :]
    xs.append(clip(x))
    return SimpleNamespace(xTraj=np.stack(xs, axis=-2), uTraj=np.stack(us, axis=-2), status=np.stack(st, axis=-1),
                           iterations=np.stack(its, axis=-1), px=np.stack(px, axis=-3), pu=np.stack(pu, axis=-3))


def as_arrays(run):
    """a MpcClosedLoop as host arrays, in the fields of `loop`'s result (px, pu None without predictions)"""
    host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    pred = run.predictions
    return SimpleNamespace(xTraj=host(run.xTraj), uTraj=host(run.uTraj), status=np.asarray(run.status, dtype=object),
                           iterations=host(run.iterations), px=None if pred is None else host(pred.xTraj),
                           pu=None if pred is None else host(pred.uTraj))


def hold(got, ref, what, steps=None):
    """`got` (as_arrays of a simulate) against the first `steps` steps of `ref` (a loop of at least as many steps: its first steps are the
    shorter loop's).  Returns the largest absolute difference."""
    S = got.uTraj.shape[-2] if steps is None else steps
    assert got.xTraj.shape == ref.xTraj[..., :S + 1, :].shape and got.uTraj.shape == ref.uTraj[..., :S, :].shape, what
    assert got.status.shape == ref.status[..., :S].shape and got.iterations.shape == got.status.shape, what
    rs, gs = ref.status[..., :S].astype(str), got.status.astype(str)
    assert np.array_equal(gs, rs), (what, gs.tolist(), rs.tolist())
    assert got.iterations.dtype == np.int32
    assert np.array_equal(got.iterations, ref.iterations[..., :S]), (what, got.iterations.tolist(), ref.iterations[..., :S].tolist())
    worst = 0.0
    pairs = [("xTraj", got.xTraj, ref.xTraj[..., :S + 1, :]), ("uTraj", got.uTraj, ref.uTraj[..., :S, :])]
    if got.px is not None:
        pairs += [("predictions.xTraj", got.px, ref.px[..., :S, :, :]), ("predictions.uTraj", got.pu, ref.pu[..., :S, :, :])]
    for name, a, b in pairs:
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        diff = float(np.max(np.abs(a - b))) if a.size else 0.0
        bound = TOL * max(1.0, float(np.max(np.abs(b))) if b.size else 0.0)
        worst = max(worst, diff)
        assert diff <= bound, (what, name, diff, bound)
    print(f"{what}: largest absolute difference {worst:.3e}; iterations up to {int(ref.iterations[..., :S].max())}; "
          f"statuses {sorted(set(rs.ravel().tolist()))}")
    return worst
