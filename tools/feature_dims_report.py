#!/usr/bin/env python3
"""The tables of profiles/feature_dims.md from the PARITY-OP lines that `pytest tests/test_gpu_dsn.py tests/test_gpu_rrn.py -m gpu -s` prints:
per network, feature_dim and plan, the worst fraction of its bound that any launch of an op kind reached.  Reads the log, runs nothing.
usage: tools/feature_dims_report.py LOG"""
import re
import sys

DSN = re.compile(r"PARITY-OP \| (\d+x\d+) fd (\d+) fused (\d) \| [^|]+ \| [^|]+ \| (\w+) \| HIP [^|]+ \| (.*)$")
RRN = re.compile(r"PARITY-OP \| S (\d+) fd (\d+) head (\d) \| [^|]+ \| [^|]+ \| (\w+) \| HIP [^|]+ \| (.*)$")


def fraction(note):
    """'exact' -> 0 (the test asserted equality), 'rel 1.4e-07 of 2e-6' -> 0.07, '0.54 of the bound' -> 0.54"""
    if "FAILED" in note:
        return float("inf")
    if note.startswith("exact"):
        return 0.0
    m = re.match(r"rel ([0-9.e+-]+) of 2e-6", note)
    return float(m.group(1)) / 2e-6 if m else float(note.split()[0])


def table(rows, kinds, key_names):
    print("| " + " | ".join(key_names + kinds) + " |")
    print("|" + "---|" * (len(key_names) + len(kinds)))
    for key in sorted(rows):
        cells = []
        for k in kinds:
            v = rows[key].get(k)
            cells.append("-" if v is None else "exact" if v[0] == 0.0 else "%.2f" % v[0])
        print("| " + " | ".join([str(x) for x in key] + cells) + " |")
    print()


def main():
    dsn, rrn = {}, {}
    for line in open(sys.argv[1]):
        line = line.strip().lstrip(".")
        for rx, dst in ((DSN, dsn), (RRN, rrn)):
            m = rx.search(line)
            if m:
                size, fd, arm, kind, note = m.groups()
                if kind in ("pack8", "classes", "fg", "votes"):
                    kind = "pack"                                    # the exact kinds of the network's two ends
                slot = dst.setdefault((int(fd), int(arm), size), {})
                f = fraction(note)
                old = slot.get(kind, (0.0, 0))
                slot[kind] = (max(old[0], f), old[1] + 1)
    print("DSN: worst fraction of the bound per op kind (fused = option key 53)\n")
    table(dsn, ["pack", "pool", "conv", "gn", "bilinear", "esp", "merge", "head"], ["fd", "fused", "frame"])
    print("RRN: worst fraction of the bound per op kind (head = option key 54)\n")
    table(rrn, ["pack", "pool", "conv", "gn", "bilinear", "head", "head3"], ["fd", "head", "S"])


if __name__ == "__main__":
    main()
