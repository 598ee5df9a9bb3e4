#!/usr/bin/env python3
"""Table of the compiler's per-kernel resource figures, and a before/after comparison.

Input: the remarks hipcc prints with -Rpass-analysis=kernel-resource-usage (they need no GPU), e.g.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -x hip --cuda-device-only \
        -Rpass-analysis=kernel-resource-usage -c openair4g_amd/csrc/oai4g_ofdm.hip -o /dev/null 2> ofdm.rpt

  kernel_resources.py ofdm.rpt                      one line per kernel
  kernel_resources.py --compare old.rpt new.rpt     kernels of old.rpt whose figures differ in new.rpt,
                                                    and the kernels only new.rpt has; exit 1 on a difference
  --filter SUBSTR                                   only kernels whose demangled name contains SUBSTR
"""
import re
import subprocess
import sys

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(.*?): (\d+) \[", line)
        if m and name and m.group(1).strip() in FIELDS:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(d):
    d = re.sub(r"^void ", "", d)
    return re.sub(r"\(.*$", "", d)


def row(name, f):
    return "%-46s vgpr %3d agpr %3d sgpr %3d scratch %4d occ %2d lds %6d" % (
        (name,) + tuple(f.get(k, -1) for k in FIELDS))


def main(argv):
    flt = ""
    if "--filter" in argv:
        i = argv.index("--filter")
        flt = argv[i + 1]
        del argv[i:i + 2]
    if argv and argv[0] == "--compare":
        old, new = parse(argv[1]), parse(argv[2])
        dm = demangle(sorted(set(old) | set(new)))
        diff = 0
        same = 0
        for n in sorted(old, key=lambda k: dm[k]):
            if flt and flt not in dm[n]:
                continue
            if n not in new:
                print("GONE    " + short(dm[n]))
                diff += 1
            elif old[n] != new[n]:
                print("CHANGED " + row(short(dm[n]), old[n]))
                print("     -> " + row(short(dm[n]), new[n]))
                diff += 1
            else:
                same += 1
        print("%d kernels of the old report identical in the new one, %d differ" % (same, diff))
        for n in sorted(set(new) - set(old), key=lambda k: dm[k]):
            if not flt or flt in dm[n]:
                print("NEW     " + row(short(dm[n]), new[n]))
        return 1 if diff else 0
    rep = parse(argv[0])
    dm = demangle(sorted(rep))
    for n in sorted(rep, key=lambda k: dm[k]):
        if not flt or flt in dm[n]:
            print(row(short(dm[n]), rep[n]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
