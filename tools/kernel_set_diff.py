#!/usr/bin/env python3
"""Did a host-side change alter the set of compiled kernels?  Compares two builds' register reports, unit by unit:

    python tools/kernel_set_diff.py <other checkout>/build/obj [build/obj]

Rows (name, vgpr, agpr, sgpr, scratch, vgpr_spill, lds, occupancy) must agree one for one; exits non-zero otherwise.
--counts prints {unit: {kernel family: instantiations}} of the first directory (tests/golden/kernel_counts.json)."""
import collections
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

KEYS = ("name", "vgpr", "agpr", "sgpr", "scratch", "vgpr_spill", "lds", "occupancy")


def rows(objdir):
    return {os.path.basename(f).split(".")[0]: sorted(tuple(r[k] for k in KEYS) for r in ge.parse_resource_usage(open(f).read()))
            for f in sorted(glob.glob(os.path.join(objdir, "*.resource_usage.txt")))}


args = [a for a in sys.argv[1:] if a != "--counts"]
a = rows(args[0])
if "--counts" in sys.argv:
    print(json.dumps({u: dict(sorted(collections.Counter(r[0].split("<")[0] for r in rs).items())) for u, rs in a.items()}, indent=1))
    sys.exit(0)
b = rows(args[1] if len(args) > 1 else os.path.join(ROOT, "build", "obj"))
bad = 0
for unit in sorted(set(a) | set(b)):
    only_a, only_b = sorted(set(a.get(unit, [])) - set(b.get(unit, []))), sorted(set(b.get(unit, [])) - set(a.get(unit, [])))
    same = a.get(unit) == b.get(unit)
    print(f"{unit}: {len(a.get(unit, []))} vs {len(b.get(unit, []))} kernels, {'identical' if same else 'DIFFERENT'}")
    for tag, rs in (("-", only_a), ("+", only_b)):
        for r in rs[:20]:
            print("  ", tag, *r)
    bad += not same
print(f"total {sum(map(len, a.values()))} vs {sum(map(len, b.values()))}")
sys.exit(1 if bad else 0)
