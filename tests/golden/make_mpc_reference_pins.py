"""Regenerates tests/golden/mpc_reference_pins.json (run from the repo root: python tests/golden/make_mpc_reference_pins.py).

The pins are what the NumPy restatement of the ADMM solve (oracle/mpc_oracle.py: admm_levels_stage, through its adapters) returns on every
named case the MPC GPU tests are held to: per (module, case, step, instance) the status, the iteration count, the final level, the level
moves, the lock, and -- written as `repr`, so that they read back to the bit -- rho_final, rp, rd and u[0].  They were written before the
four restatements of the solve became one, and tests/test_mpc_reference_pins.py holds the tree to them: an edit of the one body that
changes any family's reference shows there, without a GPU.  Regenerate them only with a change that is meant to move a reference.
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mpc_reference_pins.json")
MODULES = ["mpc_iterates_cases", "mpc_ltv_ref", "mpc_ltv_stage_ref", "mpc_ltv_soft_ref", "mpc_rti_ref"]
FLOATS = ("rho_final", "rp", "rd")     # and every entry of "u0"


def names(module):
    mod = importlib.import_module("tests." + module)
    return list(mod.CASES) if module == "mpc_rti_ref" else list(mod.ALL)


def steps(module, name):
    """[step][instance] -> the namespace a solve returned"""
    ref = importlib.import_module("tests." + module).reference(name)
    if module == "mpc_rti_ref":        # [instance] -> run, whose `results` are its solves in order
        return [list(row) for row in zip(*(r.results for r in ref))]
    return ref


def record(r):
    return dict(status=str(r.status), iters=int(r.iters), level=int(r.level), moves=[[int(v) for v in mv] for mv in r.moves],
                locked=bool(r.locked), rho_final=repr(float(r.rho_final)), rp=repr(float(r.rp)), rd=repr(float(r.rd)),
                u0=[repr(float(v)) for v in r.u[0]])


def collect(module, name):
    return [[record(r) for r in row] for row in steps(module, name)]


def main():
    pins = {module: {name: collect(module, name) for name in names(module)} for module in MODULES}
    with open(PATH, "w") as f:       # one line per case
        f.write("{\n" + ",\n".join(
            json.dumps(module) + ": {\n" + ",\n".join(json.dumps(name) + ": " + json.dumps(rows) for name, rows in cases.items()) + "\n}"
            for module, cases in pins.items()) + "\n}\n")
    n = sum(len(row) for cases in pins.values() for rows in cases.values() for row in rows)
    print(f"wrote {os.path.basename(PATH)}: {sum(len(c) for c in pins.values())} cases, {n} instance-solves")


if __name__ == "__main__":
    main()
