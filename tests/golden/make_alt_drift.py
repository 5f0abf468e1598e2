"""Writes tests/golden/alt_drift_emulation.json: for every case of tests/_alt_drift.py the error of the NumPy emulation of the
alternating iteration (tests/_segmented.alternating_loop, 2 QPs) against the C oracle at the GPU tier's checkpoints, 8 ... 400
iterations.  The 400-iteration emulation takes ~10 s per case, too long for the GPU test file that needs these figures as the
yardstick of its bound D; tests/test_alt_drift_host.py re-derives the part up to 120 iterations on every run.

    python tests/golden/make_alt_drift.py          (CPU only; a few minutes)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)

import __graft_entry__ as ge   # noqa: E402

ge.build()
import _alt_drift as ad        # noqa: E402

cases = {}
for c in ad.CASES:
    e = ad.emulate(c, ad.CHECKPOINTS)
    assert e["alt_ok"], c.id
    cases[c.id] = {k: [float(f"{v:.3e}") for v in e[k]] for k in ("early", "late", "total", "plain_total")}
    cases[c.id]["K"] = list(ad.CHECKPOINTS)
    print(c.id, " ".join(f"{v:.1e}" for v in e["total"]), "| plain", f"{max(e['plain_total']):.1e}", "| late", f"{max(e['late']):.1e}",
          flush=True)
with open(ad.FIXTURE, "w") as f:
    json.dump(dict(qps=ad.EMU_QPS, early_below=ad.EARLY, late_from=ad.LATE, cases=cases), f, indent=1)
    f.write("\n")
