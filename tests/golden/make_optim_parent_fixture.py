#!/usr/bin/env python3
"""Record what an earlier build of libttamm.so computes for the cases of
tests/test_optim_parent_bits_gpu.py, as tests/golden/optim_parent.json.

The fixture holds, per case, a sha256 digest of every parameter and optimizer state tensor and the
losses as float hex strings, from the library at the commit before csrc/optim.hip was split into
group.hip / replay.hip / optim.hip.  Run it once on an MI355X with that commit's library (nothing
of that build is committed; the file holds recorded results only):

    git worktree add /tmp/ttamm_parent <commit>
    make -C /tmp/ttamm_parent/two-tower-augmented-with-adaptive-mimic-mechanism_amd/csrc
    TTAMM_LIBRARY=/tmp/ttamm_parent/two-tower-augmented-with-adaptive-mimic-mechanism_amd/ttamm/_native/libttamm.so \\
        python tests/golden/make_optim_parent_fixture.py <commit>

An optional second argument names another output file.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "two-tower-augmented-with-adaptive-mimic-mechanism_amd"), str(ROOT / "tests")]

import test_optim_parent_bits_gpu as ob  # noqa: E402


def main(commit: str, out: Path) -> None:
    cases = {}
    for name in ob.CASES:
        cases[name] = ob.run_case(name)
        print(name, cases[name], flush=True)
    # the parent already computes the same bits with the prologue on one stream or two
    assert cases["no-overlap"]["overlap_state"] == cases["no-overlap"]["state"], cases["no-overlap"]
    lines = [f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in cases.items()]  # a case per line
    out.write_text(json.dumps({"commit": commit})[:-1] + ', "cases": {\n' + ",\n".join(lines) + "\n}}\n")
    print(f"{out}: {len(cases)} cases, {out.stat().st_size} bytes")


if __name__ == "__main__":
    main(sys.argv[1], Path(sys.argv[2]) if len(sys.argv) > 2 else ob.GOLDEN)
