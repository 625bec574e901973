#!/bin/bash
# Developer script: registers / spills / scratch of every path-trace and ray-query kernel variant (hipcc -Rpass-analysis=kernel-resource-usage).
# The unit is compiled with the flags csrc/Makefile compiles it with (make print-kernel-flags): the table describes the binary that ships.
# usage: [UNIT=ort_kernels_irradiance.hip] tools/kernel_resources.sh [--dry-run] [extra hipcc flags]      (UNIT: the kernel unit, ort_kernels.hip by default)
# --dry-run prints the compile command and stops.
set -o pipefail
cd "$(dirname "$0")/../offline_raytracer_amd/csrc" || exit 1
UNIT="${UNIT:-ort_kernels.hip}"
dry=0
if [ "$1" = "--dry-run" ]; then dry=1; shift; fi
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
KFLAGS=$(make -s print-kernel-flags UNIT="$UNIT") || exit 1
OBJ="${TMPDIR:-/tmp}/ort_k.$$.o"
if [ $dry = 1 ]; then
  echo "$HIPCC" $KFLAGS -Rpass-analysis=kernel-resource-usage "$@" -x hip -c "$UNIT" -o "$OBJ"
  exit 0
fi
"$HIPCC" $KFLAGS -Rpass-analysis=kernel-resource-usage "$@" -x hip -c "$UNIT" -o "$OBJ" 2>&1 | python3 -c '
import re, sys
cur = None
rows = {}
for line in sys.stdin:
    m = re.search(r"Function Name: (\S+)", line)
    if m: cur = m.group(1); rows[cur] = {}; continue
    m = re.search(r"remark: +(\w[^:]*): (\S+)", line)
    if m and cur: rows[cur][m.group(1).strip()] = m.group(2)
def pretty(k):
    # _ZN <len>namespace <len>name [I Lb0E Lb1E ... E] E <argument types> -> name<0,1,...>, with the namespace in front where a sibling unit named one
    if not k.startswith("_ZN"): return k
    parts, i = [], 3
    while k[i].isdigit():
        n = re.match(r"\d+", k[i:]).group(0)
        parts.append(k[i + len(n):i + len(n) + int(n)])
        i += len(n) + int(n)
    bools = re.match(r"I((?:Lb[01]E)+)E", k[i:])
    return "::".join(p for p in parts if p != "ort") + ("<" + ",".join(re.findall(r"Lb([01])E", bools.group(1))) + ">" if bools else "")
for k, v in rows.items():
    if "pt_persistent" not in k and "wf_" not in k and "raycast_rays" not in k and "occluded_rays" not in k and "ao_points" not in k and "feature_pixels" not in k and "follow_pixels" not in k and "matte_pixels" not in k and "radiance_rays" not in k and "radiance_adaptive_rays" not in k and "irradiance" not in k and "probe_sh" not in k and "pt_adaptive" not in k and "pt_groups" not in k and "pt_sample_map" not in k and "pt_accumulate" not in k and "pt_depths" not in k: continue
    print(pretty(k), " ".join("%s=%s" % (a, b) for a, b in v.items()))
'
rc=$?
rm -f "$OBJ"
exit $rc
