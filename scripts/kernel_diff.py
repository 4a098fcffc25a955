"""Compare the step kernels of two `make asm` output directories.

    python scripts/kernel_diff.py OLD_DIR NEW_DIR

Per kernel symbol: whether the instruction stream is identical, otherwise the
per-opcode instruction counts that differ, and VGPRs, SGPRs, scratch, LDS and
waves/SIMD of both builds.  The B3/S23 torus instances (LIFE = 1, CLIPPED = 0)
must be identical; the others may differ in operand order and register
numbers only (equal opcode counts, scratch 0 where it was 0, equal LDS and
waves/SIMD).  Exit status 1 if a kernel breaks its bar."""
import collections
import glob
import os
import re
import sys

from resource_usage import short

KEYS = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def load(d):
    """{symbol: (instruction lines, {resource: value})} of a directory."""
    code, res, cur = {}, collections.defaultdict(dict), None
    for path in glob.glob(os.path.join(d, "*.s")):
        for line in open(path):
            m = re.match(r"(_Z\w+):", line)
            if m:
                cur = code.setdefault(m.group(1), [])
            elif line.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None:
                text = line.split(";")[0].strip()
                if text and not text.startswith(".") or text.endswith(":"):
                    cur.append(" ".join(text.split()))
    for path in glob.glob(os.path.join(d, "resource-usage-*.txt")):
        for line in open(path):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = res[m.group(1)]
            m = re.search(r"remark:\s+(.*?): (\d+) \[", line)
            if m and m.group(1) in KEYS:
                cur[m.group(1)] = int(m.group(2))
    return {k: (v, res[k]) for k, v in code.items()}


def life_torus(sym):
    flags = re.findall(r"Lb([01])E", sym)  # LIFE, HASH, CLIPPED[, WR]
    return flags[0] == "1" and flags[2] == "0"


def main():
    old, new = load(sys.argv[1]), load(sys.argv[2])
    bad = len(set(old) ^ set(new))
    for sym in sorted(set(old) ^ set(new)):
        print(f"{short(sym):52s} only in {'OLD' if sym in old else 'NEW'}")
    tally = collections.Counter()
    for sym in sorted(set(old) & set(new), key=short):
        (ca, ra), (cb, rb) = old[sym], new[sym]
        same = ca == cb and ra == rb
        ops = collections.Counter(x.split()[0] for x in ca if not x.endswith(":"))
        ops.subtract(collections.Counter(x.split()[0] for x in cb if not x.endswith(":")))
        ops = {k: v for k, v in ops.items() if v}
        loose = not ops and all(ra[k] == rb[k] for k in KEYS[3:]) and (ra[KEYS[2]] != 0 or rb[KEYS[2]] == 0)
        ok = same or (loose and not life_torus(sym))
        kind = "life" if life_torus(sym) else "generic/clipped"
        tally[(kind, "identical" if same else "same opcode counts" if loose else "DIFFERENT")] += 1
        bad += not ok
        if not same:
            print(f"{short(sym):52s} {'ok  ' if ok else 'FAIL'} {len(ca)} -> {len(cb)} instructions, old - new {ops}")
            print("    " + "  ".join(f"{k.split(' ')[0]} {ra[k]} -> {rb[k]}" for k in KEYS))
    for (kind, what), n in sorted(tally.items()):
        print(f"{kind:16s} {what:20s} {n}")
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW: {'FAIL' if bad else 'pass'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
