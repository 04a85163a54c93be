"""Child process of tests/test_lqr_hard_gpu.py: the product library reads ZOPT_AMD_LQR_PATH once per process, so the kernels behind it
(the LDS coverage kernel, the register kernel at the aligned K1 shapes) need a process of their own.  Runs the parent's checks of the
mode given on the command line with the environment the parent set; prints "LQR-HARD-CHILD-OK" and exits 0 when they pass."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from tests import test_lqr_hard_gpu as t
    t.child(sys.argv[1])


if __name__ == "__main__":
    main()
