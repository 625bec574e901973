"""Developer script: compare the machine code of the kernels of two device-assembly files, kernel by kernel.

Make the two files from two trees, device side only, each unit with the flags the Makefile compiles it with
(make -s -C offline_raytracer_amd/csrc print-kernel-flags UNIT=ort_kernels_w5), e.g. for the four-waves unit:
  hipcc -std=c++17 -O3 -fPIC -ffp-contract=off -fno-math-errno --offload-arch=gfx950 -Wall -Wno-unused-function \
        -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize \
        --cuda-device-only -S -x hip offline_raytracer_amd/csrc/ort_kernels.hip -o before.s
(the five-waves unit ort_kernels_w5.hip with -mllvm -disable-machine-licm as well).  Then
  python3 tools/isa_diff.py before.s after.s [name filter regex]
prints, per kernel present in both, whether its instructions are identical.  Kernels are paired by their mangled name up
to the end of the template arguments: the argument types that follow name the namespace the argument structs are
defined in, which is no part of what a kernel is.  Local labels are renumbered by their order inside the function (a
kernel added before another shifts the function numbers in .LBB<f>_<n>); comments and assembler directives are ignored.
Exit status 1 if any common kernel differs."""
import re
import sys

DEFAULT = r"pt_persistent|pt_adaptive|pt_groups|pt_sample_map|pt_accumulate|pt_depths|wf_|combine_chunks|unit_eval|raycast_rays|occluded_rays|ao_points|feature_pixels|follow_pixels|matte_pixels|radiance_|irradiance_|probe_sh_"  # every kernel family


def kernel_key(sym):
    """_ZN<namespace><name>[I<bools>E]E<argument types> -> the name without the argument types (sym itself where it is no such name)"""
    if not sym.startswith("_ZN"):
        return sym
    i = 3
    while i < len(sym) and sym[i].isdigit():
        m = re.match(r"\d+", sym[i:])
        i += len(m.group(0)) + int(m.group(0))
    m = re.match(r"(I(Lb[01]E)+E)?E", sym[i:])
    return sym[:i + len(m.group(0))] if m and i <= len(sym) else sym


def functions(path):
    out, cur, body = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_.$][\w.$]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L"):
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            assert kernel_key(cur) not in out, "two functions of %s share the name %s" % (path, kernel_key(cur))
            out[kernel_key(cur)] = body
            cur = None
            continue
        s = line.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB") and ":" not in s):
            continue  # directives (.p2align, .loc, ...) and comments
        body.append(s)
    return out


def normalised(body):
    names = {}

    def ren(m):
        return names.setdefault(m.group(0), ".L%d" % len(names))
    return [re.sub(r"\.LBB\d+_\d+|\.Ltmp\d+", ren, s) for s in body]


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else DEFAULT)
    common = sorted(k for k in a if k in b and pat.search(k))
    differ = 0
    for k in common:
        same = normalised(a[k]) == normalised(b[k])
        differ += not same
        print("%-9s %6d instr  %s" % ("identical" if same else "DIFFERS", len(a[k]), k))
    only = sorted(k for k in set(a) ^ set(b) if pat.search(k))
    for k in only:
        print("only in %s: %s" % ("before" if k in a else "after", k))
    print("%d kernels compared, %d differ" % (len(common), differ))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
