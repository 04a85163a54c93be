#!/usr/bin/env python3
"""CPU check: the gfx950 device code of every selected function that exists at a base revision is unchanged in the working tree.

Compiles the given sources (default mpc.hip and mpc_wave.hip) of both trees to assembly (`hipcc --cuda-device-only -S`, the flags of
tests/test_dpp_hazards.py; no GPU needed), cuts out every function of the base whose symbol matches the regex (default: the
mpc_setup_kernel, mpc_solve_kernel, mpc_solve_wave_kernel instantiations) and compares with the same symbol in the working tree
  * its instruction text.  Basic-block labels carry the function's ordinal in the file (.LBB<f>_<b>), which moves when kernels are
    added before it, so the ordinal is dropped before comparing; so is the per-file counter in the labels of long branches
    (.Lpost_getpc<c>), which moves when the order of the functions in the file does;
  * for a kernel, the lines of its descriptor that decide occupancy (RESOURCES below: LDS, scratch, registers).
A function of the base that the working tree no longer has counts as DIFFERENT.

    python tools/isa_identity.py [--base HEAD]
    # every lqr_backward_tiled instantiation with DARE = false (the last template flag: ...Lb0EE):
    python tools/isa_identity.py --src lqr_backward_tiled_f32.hip lqr_backward_tiled_f64.hip \
        --kernels 'lqr_backward_tiled.*Lb[01]ELb[01]ELb0EE'
    # the whole library as the lab target builds it:
    python tools/isa_identity.py --src $(sed -n 's/^SRCS := //p' zopt_amd/csrc/Makefile) --kernels . --extra-flags=-DZM_LAB
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-pragma-unroll-threshold=1000000", "--cuda-device-only", "-S"]
SOURCES = ("mpc.hip", "mpc_wave.hip")
KERNELS = re.compile(r"mpc_setup_kernel|mpc_solve_kernel|mpc_solve_wave_kernel")
RESOURCES = ("group_segment_fixed_size", "private_segment_fixed_size", "next_free_vgpr", "next_free_sgpr", "accum_offset")


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
            t = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", t)
            if t.strip():
                body.append(t)
    return out


def resources(asm):
    """{kernel symbol: "lds=… scratch=… vgpr=… sgpr=… accum=…"} from the .amdhsa_kernel blocks of an assembly file"""
    out = {}
    for name, block in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
        vals = dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", block))
        out[name] = " ".join(f"{short}={vals[key]}" for short, key in zip(("lds", "scratch", "vgpr", "sgpr", "accum"), RESOURCES))
    return out


def compile_tree(csrc, out_dir, sources, extra, jobs):
    def one(src):
        out = os.path.join(out_dir, src + ".s")
        p = subprocess.run([HIPCC] + FLAGS + extra + [os.path.join(csrc, src), "-o", out], capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit(f"{csrc}/{src}: {p.stderr[-2000:]}")
        return open(out).read()

    text, res = {}, {}
    with ThreadPoolExecutor(jobs) as pool:
        for asm in pool.map(one, sources):
            text.update(functions(asm))
            res.update(resources(asm))
    return text, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="HEAD", help="git revision whose kernels must be reproduced")
    ap.add_argument("--src", nargs="+", default=list(SOURCES), help="sources under zopt_amd/csrc to compile")
    ap.add_argument("--kernels", default=KERNELS.pattern, help="regex on the (mangled) symbol: the functions to compare")
    ap.add_argument("--extra-flags", default="", help="further compiler flags for both trees, e.g. --extra-flags=-DZM_LAB")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1), help="sources compiled at the same time")
    args = ap.parse_args()
    kernels = re.compile(args.kernels)
    extra = args.extra_flags.split()
    base_sha = subprocess.run(["git", "-C", ROOT, "rev-parse", args.base], capture_output=True, text=True, check=True).stdout.strip()
    print(f"# base {base_sha}: python tools/isa_identity.py --base {args.base} --src {' '.join(args.src)} --kernels '{args.kernels}'"
          + (f" --extra-flags='{args.extra_flags}'" if extra else ""))
    with tempfile.TemporaryDirectory() as tmp:
        base_tree = os.path.join(tmp, "base")
        os.makedirs(base_tree)
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.base, "zopt_amd/csrc", "include"], capture_output=True, check=True)
        subprocess.run(["tar", "-x", "-C", base_tree], input=tar.stdout, check=True)
        os.makedirs(os.path.join(tmp, "b"))
        os.makedirs(os.path.join(tmp, "w"))
        base, base_res = compile_tree(os.path.join(base_tree, "zopt_amd", "csrc"), os.path.join(tmp, "b"), args.src, extra, args.jobs)
        work, work_res = compile_tree(os.path.join(ROOT, "zopt_amd", "csrc"), os.path.join(tmp, "w"), args.src, extra, args.jobs)
    names = sorted(k for k in base if kernels.search(k))
    bad = bad_res = 0
    for k in names:
        same = work.get(k) == base[k]
        same_res = work_res.get(k) == base_res.get(k)
        bad += not same
        bad_res += not same_res
        print(f"{'same' if same else 'DIFFERENT':9s} {len(base[k].splitlines()):6d} lines  {k}  {base_res.get(k, '(no kernel descriptor)')}"
              + ("" if same_res else f"  RESOURCES NOW {work_res.get(k, '(none)')}"))
    new = sorted(k for k in work if k not in base)
    print(f"{len(names)} functions of {args.base} compared, {bad} differ, {bad_res} with other resources; "
          f"{len(new)} new functions in the working tree")
    for k in new:
        print(f"new       {len(work[k].splitlines()):6d} lines  {k}")
    return 1 if bad or bad_res or not names else 0


if __name__ == "__main__":
    sys.exit(main())
