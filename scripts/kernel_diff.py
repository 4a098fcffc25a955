"""Compare the step kernels of two `make asm` output directories.

    python scripts/kernel_diff.py OLD_DIR NEW_DIR

Per kernel symbol one verdict, from strict to loose:

  identical           the same instruction stream and resource figures
  instruction-equal   the same number of instructions, the same count of every
                      opcode once the VOP encoding suffix (_e32 / _e64: which
                      operand went where) is removed, and VGPRs, SGPRs,
                      scratch, LDS and waves/SIMD all equal
  same opcode counts  the same count of every opcode (encoding suffix
                      removed), equal LDS and waves/SIMD, no more scratch
  different           anything else

For every kernel that is not identical: the number of differing lines, the
per-opcode counts that differ, and the five resource figures of both builds.

The bar (exit status 1 if a kernel breaks it, or the symbol sets differ): a
B3/S23 torus instance (LIFE = 1, CLIPPED = 0) is identical or
instruction-equal; every other kernel keeps its LDS and waves/SIMD and gains
no scratch.  Other kernels that are `different` inside that bar pass and are
listed by name at the end."""
import collections
import difflib
import glob
import os
import re
import sys

from resource_usage import short

KEYS = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
SCRATCH, LDS, WAVES = KEYS[2], KEYS[3], KEYS[4]


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


def instructions(lines):
    return [x for x in lines if not x.endswith(":")]


def opcodes(lines):
    """Opcode -> count, the VOP encoding suffix removed."""
    return collections.Counter(re.sub(r"_e(32|64)$", "", x.split()[0]) for x in instructions(lines))


def differing_lines(a, b):
    """Lines of the longer side that an alignment of the two streams leaves unmatched."""
    if len(a) == len(b):
        return sum(x != y for x, y in zip(a, b))
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")


def verdict(ca, ra, cb, rb):
    if ca == cb and ra == rb:
        return "identical"
    ops = opcodes(ca) == opcodes(cb)
    if ops and len(instructions(ca)) == len(instructions(cb)) and all(ra[k] == rb[k] for k in KEYS):
        return "instruction-equal"
    if ops and ra[LDS] == rb[LDS] and ra[WAVES] == rb[WAVES] and rb[SCRATCH] <= ra[SCRATCH]:
        return "same opcode counts"
    return "different"


def main():
    old, new = load(sys.argv[1]), load(sys.argv[2])
    bad = len(set(old) ^ set(new))
    for sym in sorted(set(old) ^ set(new)):
        print(f"{short(sym):52s} only in {'OLD' if sym in old else 'NEW'}")
    tally, moved = collections.Counter(), []
    for sym in sorted(set(old) & set(new), key=short):
        (ca, ra), (cb, rb) = old[sym], new[sym]
        what = verdict(ca, ra, cb, rb)
        if life_torus(sym):
            kind, ok = "life", what in ("identical", "instruction-equal")
        else:
            kind = "generic/clipped"
            ok = ra[LDS] == rb[LDS] and ra[WAVES] == rb[WAVES] and rb[SCRATCH] <= ra[SCRATCH]
        tally[(kind, what if ok else "FAIL")] += 1
        bad += not ok
        if what == "identical":
            continue
        na, nb = len(instructions(ca)), len(instructions(cb))
        ops = opcodes(ca)
        ops.subtract(opcodes(cb))
        ops = {k: v for k, v in ops.items() if v}
        print(f"{short(sym):52s} {'ok  ' if ok else 'FAIL'} {what}: {na} -> {nb} instructions, "
              f"{differing_lines(ca, cb)} lines differ, old - new {ops}")
        print("    " + "  ".join(f"{k.split(' ')[0]} {ra[k]} -> {rb[k]}" for k in KEYS))
        if what == "different":
            moved.append(f"{short(sym):52s} VGPRs {ra[KEYS[0]]} -> {rb[KEYS[0]]}, instructions {na} -> {nb}")
    for (kind, what), n in sorted(tally.items()):
        print(f"{kind:16s} {what:20s} {n}")
    if moved:
        print("not at least 'same opcode counts':")
        for line in moved:
            print("    " + line)
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW: {'FAIL' if bad else 'pass'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
