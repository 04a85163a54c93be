"""GPU tests: the lqrMpc solve kernels against the NumPy restatement of the whole solve (oracle/mpc_oracle.py: admm_levels), iterate by
iterate, in the configuration every user runs: adaptive penalty levels, over-relaxation 1.6, warm and shifted starts; the tracking
kernels with their cycle guard; the lane-per-instance kernel.

Every instance of every batch is compared (tests/mpc_iterates_cases.py: compare): status and iteration count equal, trajectories within
1e-9 max(1, max |reference|), the reported residuals within twice that (the dual one times the final penalty), and the state a warm start
reads -- y, lam, the ok flag and the final level, read back from the solve's workspace -- against the reference's.  The inputs and their
references are those of tests/mpc_iterates_cases.py; tests/test_mpc_levels_oracle.py pins the restatement and shows, without a GPU, that no
reference sits within 1e-4 of a level decision's rounding point or within 1e-6 of a stopping threshold (kernel and NumPy differ by ~1e-12
per iteration).  A chain of solves feeds the reference its own previous state and both sides the reference's x_1.

An instance whose x0 lies outside its box returns, from kernel and restatement alike, the feedback rollout u_k = -K_k x_k of the zero
iterate at 0 iterations."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mpc_iterates_cases as ic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mpc():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import mpcUtils
    return mpcUtils


def _hold(mpc, name):
    worst = ic.compare(name, ic.run_kernel(mpc, name))
    ref = ic.reference(name)
    print(f"{name}: largest deviation {worst * ic.TOL:.1e} x scale (bound {ic.TOL:.0e}); iterations "
          f"{[[r.iters for r in row] for row in ref]}")


@pytest.mark.parametrize("name", ic.GROUPS["shapes"][0])
def test_every_compiled_shape_and_loop_remainder(mpc, name):
    """(1,1) ... (12,4) at N in {1, 2, 3, 4, 5, 7}: the remainders of the three-stage unrolled sweeps; batch 7 = two waves, the second with an
    idle group; instance 3 starts outside its box ("infeasible", 0 iterations) next to wave-mates that must not notice"""
    _hold(mpc, name)


def test_quadcopter_at_its_own_horizon(mpc):
    _hold(mpc, "quad")


@pytest.mark.parametrize("name", ic.GROUPS["embedded"][0])
def test_embedded_shapes_on_the_users_data(mpc, name):
    """(3,2), (5,3), (9,4) restated un-embedded: the padding is inert and rho comes from the user's weights"""
    _hold(mpc, name)


@pytest.mark.parametrize("name", ic.GROUPS["per_problem"][0])
def test_per_problem_data(mpc, name):
    """five different problems in one call, each against the restatement on its own problem with its own prob.rho[p]"""
    _hold(mpc, name)


def test_dynamic_infeasibility_next_to_feasible_instances(mpc):
    _hold(mpc, "infeasible")


@pytest.mark.parametrize("name", ic.GROUPS["cap"][0])
def test_iteration_cap(mpc, name):
    """"optimal_inaccurate" / "user_limit" as the reference names them, at the cap's iterate.  16 is a check iteration at which the level
    rule wants a move: the returned trajectory must still be the last iterate, not its kf under the next level's gains (seen before the
    rule learnt to skip the cap's iteration; the quadcopter hides it, its weights are all I and its K_k the same at every level, hence
    the random (8, 4, 7) problem)"""
    _hold(mpc, name)


@pytest.mark.parametrize("name", ic.GROUPS["warm"][0])
def test_warm_start_chain(mpc, name):
    """cold at 1e-3 under a cap that holds one instance back -> default warm start at 1e-5 (that slot cold, the others from their stored
    y, lam and level) -> warm_start="shift" from x_1"""
    _hold(mpc, name)


@pytest.mark.parametrize("name", ic.GROUPS["tracking"][0])
def test_tracking_adaptive(mpc, name):
    """the (4, 1, 8) batch whose instance 0 locks its level (mpc_wave.hip: ZM_TRK_LEVEL) beside instances that do not, the quadcopter
    reference, a per-problem family"""
    _hold(mpc, name)


@pytest.mark.parametrize("name", ic.GROUPS["lane"][0])
def test_lane_kernel(mpc, name):
    """n > 12, m > 4 and N beyond the LDS horizon cap: the lane-per-instance kernel, which holds the level-`level0` penalty whatever
    adaptive_rho says (mpc.hip: mpc_solve) -- the reference runs n_levels = 1 -- and keeps a warm state: cold, warm, shifted"""
    _hold(mpc, name)


@pytest.mark.parametrize("name", ic.GROUPS["unstable"][0])
def test_unstable_plant_with_active_input_bounds(mpc, name):
    """an open-loop-unstable plant (spectral radius 1.3) at N = 40 with active input bounds: the restatement's rule, and the KKT
    certificate of tests/test_mpc_gpu.py: test_constrained_small_problems_against_independent_solve on the kernel's own result.  (With
    tables from an unsymmetrised value matrix both sides share the tables' error; the certificate does not.)"""
    from oracle import mpc_oracle as mo
    got = ic.run_kernel(mpc, name)
    print(f"{name}: largest deviation {ic.compare(name, got) * ic.TOL:.1e} x scale (bound {ic.TOL:.0e})")
    c = ic.build(name)
    A, B, Q, R, N = c.ctor[:5]
    n_active = 0
    for b in range(len(c.x0)):
        x, u = got[0]["x"][b], got[0]["u"][b]
        kkt = mo.kkt_residuals(A, B, Q, R, c.Qf, N, *c.ctor[5:], c.x0[b], x, u, act_tol=1e-4)
        print(f"{name} instance {b}: {kkt}")
        assert kkt["dyn"] <= 1e-12 and kkt["bound"] <= 1e-4 and kkt["stat"] <= 1e-3
        n_active += int(np.max(np.abs(u)) >= c.ctor[8][0] - 1e-5)
    assert n_active >= 1 and np.all(got[0]["status"] == "optimal")


def test_forced_lane_path_in_a_child_process(tmp_path):
    out_file = str(tmp_path / "lane.npz")
    env = dict(os.environ, ZOPT_AMD_MPC_PATH="lane")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mpc_iterates_lane_child.py"), out_file], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MPC-ITERATES-LANE-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    z = np.load(out_file)
    for name in ic.GROUPS["lane_child"][0]:
        got = [{k: z[f"{name}|{s}|{k}"] for k in ("x", "u", "status", "iters", "resid", "y", "lam", "ok", "level")}
               for s in range(len(ic.build(name).steps))]
        print(f"{name}: largest deviation {ic.compare(name, got) * ic.TOL:.1e} x scale")
