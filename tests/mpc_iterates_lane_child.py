"""Child process of tests/test_mpc_iterates_gpu.py: with ZOPT_AMD_MPC_PATH=lane in the environment (read once per process) the shapes of
the 16-lane kernels run the lane-per-instance kernel.  Runs the "lanechild" cases of tests/mpc_iterates_cases.py and writes what the
kernel returned to the .npz file named on the command line; the parent compares.  Prints "MPC-ITERATES-LANE-OK" when it is through."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(out_file):
    from tests import mpc_iterates_cases as ic
    from zopt_amd import mpcUtils
    out = {}
    for name in ic.GROUPS["lane_child"][0]:
        for s, got in enumerate(ic.run_kernel(mpcUtils, name)):
            for k, v in got.items():
                out[f"{name}|{s}|{k}"] = v
    np.savez(out_file, **out)
    print("MPC-ITERATES-LANE-OK")


if __name__ == "__main__":
    main(sys.argv[1])
