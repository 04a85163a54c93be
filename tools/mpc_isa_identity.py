#!/usr/bin/env python3
"""CPU check: the gfx950 ISA of every selected kernel that exists at a base revision is unchanged in the working tree.

Compiles the given sources (default mpc.hip and mpc_wave.hip) of both trees to assembly (`hipcc --cuda-device-only -S`, the flags of
tests/test_dpp_hazards.py; no GPU needed), cuts out every kernel of the base whose symbol matches the regex (default: the
mpc_setup_kernel, mpc_solve_kernel, mpc_solve_wave_kernel instantiations) and compares its instruction text with the same symbol's
in the working tree.  Basic-block labels carry the function's ordinal in the file (.LBB<f>_<b>), which moves when kernels are added
before it, so the ordinal is dropped before comparing.

    python tools/mpc_isa_identity.py [--base HEAD]
    # every lqr_backward_tiled instantiation with DARE = false (the last template flag: ...Lb0EE):
    python tools/mpc_isa_identity.py --src lqr_backward_tiled_f32.hip lqr_backward_tiled_f64.hip \
        --kernels 'lqr_backward_tiled.*Lb[01]ELb[01]ELb0EE'
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-pragma-unroll-threshold=1000000", "--cuda-device-only", "-S"]
SOURCES = ("mpc.hip", "mpc_wave.hip")
KERNELS = re.compile(r"mpc_setup_kernel|mpc_solve_kernel|mpc_solve_wave_kernel")


def functions(asm):
    """{symbol: normalised instruction text} of every function in an assembly file"""
    out, name, body = {}, None, []
    for ln in asm.splitlines():
        m = re.match(r"^([A-Za-z_][\w.$]*):", ln)
        if m and name is None and not ln.startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is not None:
            if ln.startswith(".Lfunc_end"):
                out[name] = "\n".join(body)
                name = None
                continue
            t = ln.split(";")[0].rstrip()
            t = re.sub(r"\.LBB\d+_", ".LBB_", t)
            t = re.sub(r"\.Ltmp\d+", ".Ltmp", t)
            if t.strip():
                body.append(t)
    return out


def compile_tree(csrc, out_dir, sources):
    res = {}
    for src in sources:
        out = os.path.join(out_dir, src + ".s")
        p = subprocess.run([HIPCC] + FLAGS + [os.path.join(csrc, src), "-o", out], capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit(f"{csrc}/{src}: {p.stderr[-2000:]}")
        res.update(functions(open(out).read()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="HEAD", help="git revision whose kernels must be reproduced")
    ap.add_argument("--src", nargs="+", default=list(SOURCES), help="sources under zopt_amd/csrc to compile")
    ap.add_argument("--kernels", default=KERNELS.pattern, help="regex on the (mangled) symbol: the kernels to compare")
    args = ap.parse_args()
    kernels = re.compile(args.kernels)
    with tempfile.TemporaryDirectory() as tmp:
        base_tree = os.path.join(tmp, "base")
        os.makedirs(base_tree)
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.base, "zopt_amd/csrc", "include"], capture_output=True, check=True)
        subprocess.run(["tar", "-x", "-C", base_tree], input=tar.stdout, check=True)
        os.makedirs(os.path.join(tmp, "b"))
        os.makedirs(os.path.join(tmp, "w"))
        base = compile_tree(os.path.join(base_tree, "zopt_amd", "csrc"), os.path.join(tmp, "b"), args.src)
        work = compile_tree(os.path.join(ROOT, "zopt_amd", "csrc"), os.path.join(tmp, "w"), args.src)
    names = sorted(k for k in base if kernels.search(k))
    bad = 0
    for k in names:
        same = work.get(k) == base[k]
        bad += not same
        print(f"{'same' if same else 'DIFFERENT':9s} {len(base[k].splitlines()):6d} lines  {k}")
    new = sorted(k for k in work if k not in base)
    print(f"{len(names)} kernels of {args.base} compared, {bad} differ; {len(new)} new functions in the working tree")
    for k in new:
        print(f"new       {len(work[k].splitlines()):6d} lines  {k}")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    sys.exit(main())
