#!/bin/bash
# Developer script: registers / spills / scratch of every path-trace and ray-query kernel variant (hipcc -Rpass-analysis=kernel-resource-usage).
# usage: [UNIT=ort_kernels_irradiance.hip] tools/kernel_resources.sh [extra hipcc flags]      (UNIT: the kernel unit, ort_kernels.hip by default)
cd "$(dirname "$0")/../offline_raytracer_amd/csrc"
/opt/rocm/bin/hipcc -std=c++17 -O3 -fPIC -ffp-contract=off -fno-math-errno --offload-arch=gfx950 -fhip-fp32-correctly-rounded-divide-sqrt \
  -Rpass-analysis=kernel-resource-usage "$@" -x hip -c "${UNIT:-ort_kernels.hip}" -o /tmp/ort_k.o 2>&1 | python3 -c '
import re, sys
cur = None
rows = {}
for line in sys.stdin:
    m = re.search(r"Function Name: (\S+)", line)
    if m: cur = m.group(1); rows[cur] = {}; continue
    m = re.search(r"remark: +(\w[^:]*): (\S+)", line)
    if m and cur: rows[cur][m.group(1).strip()] = m.group(2)
for k, v in rows.items():
    if "pt_persistent" not in k and "wf_" not in k and "raycast_rays" not in k and "occluded_rays" not in k and "ao_points" not in k and "radiance_rays" not in k and "radiance_adaptive_rays" not in k and "irradiance" not in k and "pt_adaptive" not in k: continue
    name = k.replace("_ZN3ort", "").replace("EvNS_9SceneViewENS_9RenderHotE", "").replace("NS_9RaycastIOE", "").replace("NS_10OccludedIOE", "").replace("NS_4AoIOE", "")
    print(name, " ".join("%s=%s" % (a, b) for a, b in v.items()))
'
