"""Compares the device assembly of two builds kernel by kernel: did a change to the source move
any kernel's code?  Takes two directories of .s files (`make asm`, or `make build/asm/<unit>.s`
for any HIP unit, at the two commits) and matches the files by name and the kernels by symbol.

Per kernel it compares
  - the instruction lines and labels, comments stripped and local labels (.L...) renumbered in
    order of appearance, so that a kernel's place in its file does not matter;
  - the .amdhsa_kernel ... .end_amdhsa_kernel block (registers, LDS, scratch, kernarg size).
Every kernel that differs is printed with its instruction count, next_free_vgpr and next_free_sgpr
on both sides; a kernel or file on one side only is unmatched.  `--rename old=new` rewrites `old`
to `new` in the first directory's text before matching (a renamed kernel or helper).  Text only:
no instruction is known by name.  Exit status 1 on any difference or unmatched kernel.

  python scripts/kernel_asm_diff.py parent/build/asm of-spmm_amd/build/asm edge_softmax.s
"""
from __future__ import annotations

import argparse
import os
import re
import sys

LOCAL_LABEL = re.compile(r"\.L[A-Za-z0-9_$.]+")
FUNCTION_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
NEXT_FREE = re.compile(r"\.amdhsa_next_free_([vs]gpr)\s+(\d+)")


class Kernel:
    def __init__(self):
        self.code = []        # instructions and labels, normalised
        self.descriptor = []  # the .amdhsa_kernel block
        self.instructions = 0
        self.next_free = {"vgpr": None, "sgpr": None}

    def finish(self):
        names = {}

        def renumber(m):
            return names.setdefault(m.group(0), f".L{len(names)}")

        self.code = [LOCAL_LABEL.sub(renumber, line) for line in self.code]


def kernels_of(path, renames):
    """{symbol: Kernel} of the functions of `path` that have a kernel descriptor."""
    found, name, body, in_descriptor = {}, None, None, False
    with open(path, errors="replace") as f:
        for raw in f:
            for old, new in renames:
                raw = raw.replace(old, new)
            line = raw.split(";", 1)[0].strip()
            if not line:
                continue
            m = FUNCTION_LABEL.match(line)  # a global symbol: labels inside a function are local
            if m:
                name, body, in_descriptor = m.group(1), Kernel(), False
            elif name is None:
                continue
            elif line.startswith(".size") and line.split()[1].rstrip(",") == name:
                if body.descriptor:
                    body.finish()
                    found[name] = body
                name = None
            elif line.startswith(".amdhsa_kernel"):
                in_descriptor = True
                body.descriptor.append(line)
            elif in_descriptor:
                body.descriptor.append(" ".join(line.split()))
                in_descriptor = not line.startswith(".end_amdhsa_kernel")
                m = NEXT_FREE.match(line)
                if m:
                    body.next_free[m.group(1)] = int(m.group(2))
            elif line.endswith(":"):
                body.code.append(line)
            elif not line.startswith("."):  # a directive is no code
                body.code.append(" ".join(line.split()))
                body.instructions += 1
    return found


def compare_unit(unit, old_path, new_path, renames):
    old, new = kernels_of(old_path, renames), kernels_of(new_path, [])
    differ = unmatched = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in old or sym not in new:
            unmatched += 1
            print(f"  only in the {'first' if sym in old else 'second'}: {sym}")
            continue
        a, b = old[sym], new[sym]
        what = [w for w, same in (("code", a.code == b.code),
                                  ("descriptor", a.descriptor == b.descriptor)) if not same]
        if what:
            differ += 1
            print(f"  differs ({', '.join(what)}): {sym}\n"
                  f"    instructions {a.instructions} -> {b.instructions}, "
                  f"next_free_vgpr {a.next_free['vgpr']} -> {b.next_free['vgpr']}, "
                  f"next_free_sgpr {a.next_free['sgpr']} -> {b.next_free['sgpr']}")
    matched = len(set(old) & set(new))
    print(f"{unit}: {matched} kernels matched, {differ} differ, {unmatched} unmatched")
    return matched, differ, unmatched


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_dir")
    ap.add_argument("new_dir")
    ap.add_argument("units", nargs="*",
                    help=".s files to compare (default: all of both directories)")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="rewrite OLD to NEW in the first directory's text (repeatable)")
    args = ap.parse_args()
    renames = []
    for r in args.rename:
        if "=" not in r:
            ap.error(f"--rename takes OLD=NEW, not {r!r}")
        renames.append(tuple(r.split("=", 1)))
    listing = lambda d: {f for f in os.listdir(d) if f.endswith(".s")}  # noqa: E731
    units = args.units or sorted(listing(args.old_dir) | listing(args.new_dir))
    if not units:
        ap.error("no .s files to compare")
    total = [0, 0, 0]
    for unit in units:
        paths = [os.path.join(d, unit) for d in (args.old_dir, args.new_dir)]
        missing = [p for p in paths if not os.path.isfile(p)]
        if missing:
            print(f"{unit}: missing {', '.join(missing)}")
            total[2] += 1
            continue
        for i, n in enumerate(compare_unit(unit, *paths, renames)):
            total[i] += n
    print(f"total: {total[0]} kernels matched, {total[1]} differ, {total[2]} unmatched")
    return 1 if total[1] or total[2] else 0


if __name__ == "__main__":
    sys.exit(main())
