"""The NumPy restatement of quad_trim_kernel's iteration (tests/trim_ref.py) on the operating points of tests/test_trim_hard_gpu.py:
which points are trimmable, and how fast -- the facts the GPU test's requirements rest on."""
import numpy as np

from tests import trim_ref as tr


def test_restatement_converges_on_the_required_family_within_six_iterations():
    F = tr.family()
    assert len(F) == 313 and np.all(np.hypot(tr.drag(F[:, 0]), tr.drag(F[:, 1])) <= 0.9 * tr.MG) and np.all(np.abs(F[:, 2]) <= 19.0)
    for v in F:
        z, r, its = tr.lm_trim(v)
        assert r <= 1e-12 and its <= 6, (v, r, its)
        assert tr.residual_ld(np.concatenate([v, z[:5]]), z[5:], (0, 0, 0))[0] <= 1e-12


def test_restatement_on_the_failing_points_and_with_wind():
    """(25, 0, 0) and (21, 0, 0): the drag exceeds m g; the iterate of the second walks to theta = -pi/2.  A body wind of (5, -3, 1)
    on a sample of the family: converged, in at most 10 iterations."""
    z, r, its = tr.lm_trim(tr.FAILING[0])
    assert 4.6 < r < 4.8 and its == 200
    z, r, _ = tr.lm_trim(tr.FAILING[1])
    assert 0.69 < r < 0.70 and abs(z[4] + np.pi / 2) < 1e-6
    for v in tr.family()[::13]:
        _, r, its = tr.lm_trim(v, tr.WINDS[3])
        assert r <= 1e-12 and its <= 10
