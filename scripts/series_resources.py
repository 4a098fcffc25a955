"""The population-series instances next to their hashed siblings, from
`make asm`'s resource remarks.

    python scripts/series_resources.py akka-game-of-life_amd/build/asm

Reads DIR/resource-usage-g*.txt (the plain instances) and
DIR/series/resource-usage-g*.txt (the series instances, whose last template
argument carries kKindSeries = 4 on top of the interleave).  Per series
instance: VGPRs and waves/SIMD of the instance and of the hashed instance of
the same shape, scratch, and a mark where it sits below that sibling.  Exit
status 1 if a series instance uses scratch."""
import glob
import os
import re
import sys

from resource_usage import KEYS, short


def load(pattern):
    rows, cur = {}, None
    for p in sorted(glob.glob(pattern)):
        for line in open(p):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = rows.setdefault(short(m.group(1)), {})
                continue
            for k in KEYS:
                m = re.search(r"remark:\s+%s: (\d+)" % re.escape(k), line)
                if m and cur is not None:
                    cur[k] = int(m.group(1))
    return rows


def main():
    d = sys.argv[1]
    plain = load(os.path.join(d, "resource-usage-g*.txt"))
    series = load(os.path.join(d, "series", "resource-usage-g*.txt"))
    bad = below = 0
    print(f"{'series instance':44s} {'VGPR':>4s} {'waves':>5s} scratch | hashed sibling VGPR waves")
    for name in sorted(series):
        m = re.match(r"(\w+)<(.*)>", name)
        if not m:
            continue
        args = m.group(2).split(",")
        wr = m.group(1) == "multistep_hg_kernel" and len(args) == 7
        kind = -2 if wr else -1
        hash_at = kind - 2  # ..., HASH, CLIPPED, KIND[, WR]
        if int(args[kind]) < 4:
            continue
        sib = list(args)
        sib[kind] = str(int(args[kind]) & 3)
        sib[hash_at] = "1"
        s = plain.get(f"{m.group(1)}<{','.join(sib)}>", {})
        r = series[name]
        what = "hash+pop" if args[hash_at] == "1" else "pop"
        lower = s and r.get(KEYS[3], 0) < s.get(KEYS[3], 0)
        below += bool(lower)
        bad += r.get(KEYS[2], 0) != 0
        print(f"{name:34s} {what:9s} {r.get('VGPRs', 0):4d} {r.get(KEYS[3], 0):5d} {r.get(KEYS[2], 0):7d} | "
              f"{s.get('VGPRs', 0):19d} {s.get(KEYS[3], 0):5d}{'   BELOW' if lower else ''}")
    print(f"{len(series)} series kernels, {bad} with scratch, {below} a wave or more below the hashed sibling")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
