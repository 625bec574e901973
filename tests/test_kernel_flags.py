"""One source of compile flags for the kernel units: csrc/Makefile.  The developer scripts that compile a unit by hand
(tools/kernel_resources.sh for the register / spill table, tools/build_variant.sh for A/B builds) must describe and build the
binary that ships, so their compile lines -- printed by --dry-run, nothing is compiled here -- carry exactly the flags of the
Makefile's own rule for that unit; and every kernel rule keeps the two flags the bit-exact results rest on."""
import os
import shlex
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "offline_raytracer_amd", "csrc")
UNITS = ["ort_kernels", "ort_kernels_w5", "ort_kernels_adaptive", "ort_kernels_render_adaptive", "ort_kernels_irradiance"]
ENV = {k: v for k, v in os.environ.items() if k not in ("MAKEFLAGS", "MFLAGS", "HIPCC", "ARCH", "FLAGS", "KERNEL_FLAGS", "W5FLAGS", "UNIT")
       and not k.startswith(("KERNEL_FLAGS_", "UNITFLAGS_"))}


def run(cmd, **env):
    return subprocess.run(cmd, cwd=ROOT, env=dict(ENV, **env), capture_output=True, text=True, timeout=120, check=True).stdout


def compile_lines(text):
    """unit -> the flags of its compile command: the words between the compiler and `-x hip -c <unit>.hip`"""
    out = {}
    for line in text.splitlines():
        w = shlex.split(line)
        if "-c" not in w or not w[w.index("-c") + 1].endswith(".hip"):
            continue
        unit = os.path.basename(w[w.index("-c") + 1])[:-len(".hip")]
        at = w.index("-c")
        assert w[at - 2:at] == ["-x", "hip"], line
        assert unit not in out, "two compile lines for " + unit
        out[unit] = w[1:at - 2]
    return out


@pytest.fixture(scope="module")
def make_rules():
    """what `make` would run for every kernel object (-n: nothing runs; -B: whatever is built already)"""
    rules = compile_lines(run(["make", "-n", "-B", "-C", CSRC]))
    assert sorted(rules) == sorted(UNITS)
    return rules


def test_makefile_names_its_units_and_flags(make_rules):
    assert run(["make", "-s", "-C", CSRC, "print-kernel-units"]).split() == UNITS
    for u in UNITS:
        for name in (u, u + ".hip"):
            assert shlex.split(run(["make", "-s", "-C", CSRC, "print-kernel-flags", "UNIT=" + name])) == make_rules[u], name


@pytest.mark.parametrize("unit", UNITS)
def test_every_kernel_rule_keeps_the_bit_exactness_flags(make_rules, unit):
    flags = make_rules[unit]
    assert "-ffp-contract=off" in flags and "-fhip-fp32-correctly-rounded-divide-sqrt" in flags
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    assert not any(f.startswith("-ffast-math") or f == "-Ofast" or f.startswith("-ffp-contract=fast") for f in flags)


@pytest.mark.parametrize("unit", UNITS)
def test_kernel_resources_compiles_the_unit_as_the_makefile_does(make_rules, unit):
    got = compile_lines(run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "--dry-run"], UNIT=unit + ".hip"))
    assert list(got) == [unit]
    assert [f for f in got[unit] if f != "-Rpass-analysis=kernel-resource-usage"] == make_rules[unit]
    # extra flags are added after the Makefile's, never in their place
    got = compile_lines(run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "--dry-run", "-DORT_X=1"], UNIT=unit + ".hip"))
    assert got[unit] == make_rules[unit] + ["-Rpass-analysis=kernel-resource-usage", "-DORT_X=1"]


def test_build_variant_compiles_every_unit_as_the_makefile_does(make_rules):
    text = run(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), "--dry-run", "tag"])
    got = compile_lines(text)
    assert got == make_rules
    link = [shlex.split(ln) for ln in text.splitlines() if "-shared" in ln]
    assert len(link) == 1
    host = shlex.split(run(["make", "-s", "-C", CSRC, "print-flags"]))
    assert link[0][1:1 + len(host)] == host and "-fno-slp-vectorize" not in host
    for u in UNITS:
        assert any(w.endswith("/%s_tag.o" % u) for w in link[0]), u
    # what the caller adds goes to the units it names, after the Makefile's flags
    got = compile_lines(run(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), "--dry-run", "tag", "-DORT_X=1"],
                            W5FLAGS="-DORT_Y=2", UNITFLAGS_ort_kernels_irradiance="-DORT_Z=3"))
    want = {u: list(f) for u, f in make_rules.items()}
    want["ort_kernels"].append("-DORT_X=1")
    want["ort_kernels_w5"].append("-DORT_Y=2")
    want["ort_kernels_irradiance"].append("-DORT_Z=3")
    assert got == want
