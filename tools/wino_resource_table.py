"""Kernel resource usage of two builds of the Winograd translation units, side by side, from hipcc's
``-Rpass-analysis=kernel-resource-usage`` remarks (needs no device).

  for f in conv_wino conv_wino4 conv_wino_wgrad conv_wino4_wgrad; do
    hipcc <the Makefile's flags of that file> --cuda-device-only -Rpass-analysis=kernel-resource-usage \
        -c csrc/$f.hip -o /dev/null 2> DIR/$f.txt
  done                                   # once per build, into its own DIR
  python tools/wino_resource_table.py PARENT_DIR NEW_DIR [kernel dropped on purpose ...]

Prints one line per kernel symbol (parent -> new where they differ) and a verdict; exit status 1 when a kernel has
more spilled registers or scratch than in the parent, another occupancy or static LDS size, or when the sets of symbols
differ by more than the kernels named on the command line."""
import glob
import os
import re
import subprocess
import sys

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
          "LDS Size [bytes/block]"]
HEAD = ["VGPR", "AGPR", "SGPR", "Sspill", "Vspill", "scratch", "occ", "LDS"]
NO_MORE = ["SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]"]
EQUAL = ["Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]


def short_names(symbols):
    """Mangled symbol -> kernel name with its template arguments, without namespace and parameter list (a kernel that gains a
    parameter is the same kernel)."""
    pretty = subprocess.run(["c++filt"] + symbols, capture_output=True, text=True).stdout.splitlines()
    return {s: re.sub(r"^void |dvg::|\(.*$", "", p) for s, p in zip(symbols, pretty)}


def read(directory):
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.txt"))):
        name = None
        for line in open(path):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                out[name] = {"file": os.path.basename(path)[:-4]}
                continue
            m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[-Rpass", line)
            if m and name:
                out[name][m.group(1)] = int(m.group(2))
    short = short_names(sorted(out))
    return {short[k]: v for k, v in out.items()}


def main():
    parent, new, dropped = read(sys.argv[1]), read(sys.argv[2]), set(sys.argv[3:])
    names = sorted(set(parent) | set(new))
    bad = []
    print("%-12s %-62s " % ("file", "kernel") + " ".join("%11s" % h for h in HEAD))
    for n in names:
        p, q = parent.get(n), new.get(n)
        short = n
        if p is None or q is None:
            gone = short in dropped
            print("%-12s %-62s %s" % ((p or q)["file"], short, ("only in the parent" if q is None else "only in the new build") +
                                      (" (dropped on purpose)" if gone and q is None else "")))
            if not (gone and q is None):
                bad.append("%s: %s" % (short, "missing" if q is None else "new symbol"))
            continue
        cells = ["%11s" % (str(p[f]) if p[f] == q[f] else "%d->%d" % (p[f], q[f])) for f in FIELDS]
        print("%-12s %-62s " % (p["file"], short) + " ".join(cells))
        bad += ["%s: %s %d -> %d" % (short, f, p[f], q[f]) for f in NO_MORE if q[f] > p[f]]
        bad += ["%s: %s %d -> %d" % (short, f, p[f], q[f]) for f in EQUAL if q[f] != p[f]]
    lower = sum(1 for n in names if n in parent and n in new and any(new[n][f] < parent[n][f] for f in NO_MORE))
    print("kernels: %d in the parent, %d in the new build; %d with fewer spills or less scratch" % (len(parent), len(new), lower))
    print("verdict: " + ("PASS (no kernel has more spilled registers or scratch; occupancy and LDS equal; same symbols)" if not bad
                         else "FAIL\n  " + "\n  ".join(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
