#!/usr/bin/env python3
"""Developer tool: registers / spills / occupancy / LDS of every kernel of one translation unit, from hipcc's
-Rpass-analysis=kernel-resource-usage (build container; no GPU needed), compiled with the flags the Makefile builds the unit with
(`make print-flags`; --dev: the developer build's, implied for units that exist only there).
    tools/kernel_resources.py [--dev] kernels_tdnn_chain [filter]"""
import re, subprocess, sys, os
csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "asv-subtools_amd", "csrc")
args = [a for a in sys.argv[1:] if a != "--dev"]
unit = args[0]
flt = args[1] if len(args) > 1 else ""
in_tools = not os.path.exists(os.path.join(csrc, unit + ".hip"))
dev = "--dev" in sys.argv or in_tools
flags = subprocess.run(["make", "-s", "-C", csrc, "print-flags", "UNIT=" + unit] + (["DEV=1"] if dev else []), capture_output=True, text=True, check=True).stdout.split()
cmd = ["/opt/rocm/bin/hipcc"] + flags + ["-c", os.path.join("tools", unit + ".hip") if in_tools else unit + ".hip", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
if r.returncode != 0:
    sys.exit(r.stderr[-4000:])
out = r.stderr
cur = None
rows = {}
for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        cur = re.sub(r"asv::\(anonymous namespace\)::", "", cur).split("(")[0]
        rows[cur] = {}
        continue
    m = re.search(r"remark:\s+([A-Za-z][\w \[\]/]*?): (\d+)", line)
    if m and cur:
        rows[cur][m.group(1).strip()] = int(m.group(2))
for k, v in rows.items():
    if flt in k:
        print("%-70s VGPR %3d AGPR %3d spill %3d SGPR %3d occ %d LDS %6d scratch %d" % (k[:70], v.get("VGPRs", -1), v.get("AGPRs", -1), v.get("VGPRs Spill", -1),
              v.get("TotalSGPRs", -1), v.get("Occupancy [waves/SIMD]", -1), v.get("LDS Size [bytes/block]", -1), v.get("ScratchSize [bytes/lane]", -1)))
