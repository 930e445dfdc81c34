#!/usr/bin/env python3
"""bench.py with the int8 shadow forced at every size: how GpuIndex.SHADOW_MIN_ROWS is measured.

  python tools/bench_shadow_rows.py --gpus 1 --rows 250000        # every argument goes to bench.py

bench.py builds its index with GpuIndex(dim, rows, device), i.e. shadow="auto".  This wrapper lowers
the class attribute GpuIndex.SHADOW_MIN_ROWS to 1 for the process and then runs bench.py unchanged, so
a corpus below the shipped cut takes the shadow-first chain.  Alternate it with
`python bench.py --gpus 1 --rows N` of the parent commit, three runs each, and take the smallest N at
which the shadow wins outside the parent's spread (profiles/flat_shadow_min_rows.json)."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rag_fin_amd.index import GpuIndex   # noqa: E402

GpuIndex.SHADOW_MIN_ROWS = 1
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
