"""Child process of tests/test_linesearch_hard_gpu.py: the switches ZOPT_AMD_ROLLOUT_PATH (product library) and ZOPT_AMD_ROLLOUT_QUAD
(lab library, through ZOPT_AMD_LIB) are read once per process, so the forms of the line search behind them need a process of their
own.  Runs the parent's checks of the mode given on the command line with whatever the parent put into the environment; prints
"LINESEARCH-CHILD-OK" and exits 0 when they pass."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from tests import test_linesearch_hard_gpu as t
    t.child(sys.argv[1])


if __name__ == "__main__":
    main()
