#!/usr/bin/env python3
"""Record the workspace sizes an earlier build of libttamm.so reports for the descriptor matrix of
tests/test_tower_workspace_cpu.py, as tests/golden/tower_workspace_parent.json.

The fixture holds the sizes of the library at the commit before the tower entries shared one
workspace planner.  To regenerate it, build that commit in a scratch checkout and pass its
library (nothing of that build is committed; the file holds recorded results only):

    git worktree add /tmp/ttamm_parent <commit>
    make -C /tmp/ttamm_parent/two-tower-augmented-with-adaptive-mimic-mechanism_amd/csrc
    python tests/golden/make_tower_workspace_fixture.py <commit> \\
        /tmp/ttamm_parent/two-tower-augmented-with-adaptive-mimic-mechanism_amd/ttamm/_native/libttamm.so
"""

from __future__ import annotations

import ctypes
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "two-tower-augmented-with-adaptive-mimic-mechanism_amd"), str(ROOT / "tests")]

import test_tower_workspace_cpu as tw  # noqa: E402
from ttamm import _lib  # noqa: E402


def main(commit: str, library: str) -> None:
    lib = ctypes.CDLL(library)
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        if name.endswith("_workspace_size"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    sizes = {tw.case_id(c): {str(n): tw.query_sizes(lib, c, n) for n in tw.ROWS} for c in tw.CASES}
    head = {"commit": commit, "queries": list(tw.QUERIES), "rows": list(tw.ROWS)}
    lines = [f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in sizes.items()]  # a case per line
    tw.GOLDEN.write_text(json.dumps(head)[:-1] + ', "sizes": {\n' + ",\n".join(lines) + "\n}}\n")
    print(f"{tw.GOLDEN}: {len(sizes)} cases, {tw.GOLDEN.stat().st_size} bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
