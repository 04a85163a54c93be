"""CPU check of the NumPy restatement of the ADMM solve (oracle/mpc_oracle.py: admm_levels_stage and its adapters) against the pins of
tests/golden/mpc_reference_pins.json, written by tests/golden/make_mpc_reference_pins.py when every family still had a restatement of
its own: every reference the MPC GPU tests hold the kernels to, of every family at once.  Status, iterations, level, moves and lock are
equal; rho_final, rp, rd and u[0] are within the suite's iterate tolerance, 1e-9 max(1, |pinned|) -- the rule between kernel and
restatement, which allows for another BLAS; the cases are clear of rounding-sensitive decisions (test_gpu_cases_are_decisive).  No GPU."""
import json

import pytest

from tests import mpc_iterates_cases as mc
from tests.golden import make_mpc_reference_pins as pins

with open(pins.PATH) as f:
    PINNED = json.load(f)


def test_every_case_is_pinned():
    assert list(PINNED) == pins.MODULES
    for module in pins.MODULES:
        assert list(PINNED[module]) == pins.names(module), module


@pytest.mark.parametrize("module,name", [(module, name) for module in pins.MODULES for name in PINNED[module]])
def test_reference_is_the_pinned_one(module, name):
    want, got = PINNED[module][name], pins.collect(module, name)
    assert [len(row) for row in got] == [len(row) for row in want]
    worst = 0.0
    for s, (wrow, grow) in enumerate(zip(want, got)):
        for b, (w, g) in enumerate(zip(wrow, grow)):
            at = (module, name, s, b)
            assert set(g) == set(w)
            for k in w:
                if k not in pins.FLOATS and k != "u0":
                    assert g[k] == w[k], (at, k, g[k], w[k])
                    continue
                gv, wv = (r[k] if k == "u0" else [r[k]] for r in (g, w))
                assert len(gv) == len(wv), (at, k)
                for a, p in zip(map(float, gv), map(float, wv)):
                    dev = abs(a - p) / (mc.TOL * max(1.0, abs(p)))
                    assert dev <= 1.0, (at, k, a, p)
                    worst = max(worst, dev)
    print(f"{module} {name}: largest deviation {worst:.3f} of its bound")
