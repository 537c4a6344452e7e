#!/usr/bin/env python3
"""Writes tests/fixtures/forward_config_grid.json: the configuration (ofx_spmm_csr_describe) of
every case of tests/test_forward_config_grid.py, as the library in use chooses it (the in-tree one,
or OFX_SPMM_LIB=<path>).  The file holds the distinct strings without their workspace size, then
one [string index, workspace bytes] pair per case in the order of the test's cases().  Run it on
the library whose choices are to be kept, before a change to the launch rules; on an unchanged
rule set it reproduces the file byte for byte.  No GPU is needed.

  python scripts/make_forward_config_grid.py [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_forward_config_grid as grid  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=grid.FIXTURE)
    args = ap.parse_args()
    strings, index, rows = [], {}, []
    for case in grid.cases():
        head, ws = grid.split_ws(grid.describe(case))
        if head not in index:
            index[head] = len(strings)
            strings.append(head)
        rows.append([index[head], ws])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write('{"strings": [\n')
        f.write(",\n".join(json.dumps(s) for s in strings))
        f.write('\n],\n"cases": [\n')
        # 16 pairs per line keep the file diffable without one line per case
        lines = [", ".join(json.dumps(r, separators=(",", ":")) for r in rows[i:i + 16])
                 for i in range(0, len(rows), 16)]
        f.write(",\n".join(lines))
        f.write("\n]}\n")
    errors = sum(1 for s in strings if s.startswith("error: "))
    print(f"{len(rows)} cases, {len(strings)} distinct strings ({errors} of them errors) -> {args.out}")


if __name__ == "__main__":
    main()
