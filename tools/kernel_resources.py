#!/usr/bin/env python3
"""Per-kernel resource table from hipcc's -Rpass-analysis=kernel-resource-usage remarks.

usage: kernel_resources.py [--mangled] REMARKS...   (files of compiler stderr; `make resources`)

One line per kernel, sorted by demangled name: VGPRs, SGPRs, AGPRs, scratch bytes/lane, occupancy in
waves per SIMD, LDS bytes/block, spilled SGPRs / VGPRs.  --mangled keys the lines by the mangled
name instead (what two trees are compared by: the same kernel under the same name).
"""
import re
import subprocess
import sys

FIELDS = ["VGPRs", "TotalSGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]",
          "SGPRs Spill", "VGPRs Spill"]
HEAD = ["VGPRs", "SGPRs", "AGPRs", "scrtch", "occup", "LDS", "Sspill", "Vspill"]


def parse(paths):
    kernels, cur = {}, None
    for path in paths:
        for line in open(path, errors="replace"):
            m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis=kernel-resource-usage\]", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                cur = kernels.setdefault(m.group(2), {})
            elif cur is not None:
                cur[m.group(1)] = m.group(2)
    return kernels


def main():
    args = sys.argv[1:]
    mangled = "--mangled" in args
    kernels = parse([a for a in args if a != "--mangled"])
    names = sorted(kernels)
    shown = names
    if not mangled:
        out = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True,
                             check=True).stdout.split("\n")
        shown = [s.replace("vox::", "") for s in out[:len(names)]]
    rows = sorted(zip(shown, names))
    w = max([len(s) for s in shown] + [6])
    print(f"{'kernel':<{w}} | " + " ".join(f"{h:>6}" for h in HEAD))
    for s, n in rows:
        print(f"{s:<{w}} | " + " ".join(f"{kernels[n].get(f, '?'):>6}" for f in FIELDS))


if __name__ == "__main__":
    main()
