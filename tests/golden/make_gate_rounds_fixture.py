#!/usr/bin/env python3
"""Record what an earlier build of libttamm.so computes for the cases of
tests/test_gate_rounds_gpu.py, as tests/golden/gate_rounds_parent.json.

The fixture holds the losses (and, where the case has one, the compute_loss pass's loss) and a
sha256 of every parameter and optimizer-state tensor after three one-process steps with the
library at the commit before the fused gate's block counts changed.  Run it once on the GPU with that commit's library (nothing of that build is committed;
the file holds recorded results only):

    git worktree add /tmp/ttamm_parent <commit>
    make -C /tmp/ttamm_parent/two-tower-augmented-with-adaptive-mimic-mechanism_amd/csrc
    TTAMM_LIBRARY=/tmp/ttamm_parent/two-tower-augmented-with-adaptive-mimic-mechanism_amd/ttamm/_native/libttamm.so \\
        python tests/golden/make_gate_rounds_fixture.py <commit>

It also runs every case on a zeroed workspace and records ("poison_equal") whether the 0xFF
bytes the test fills the workspace with changed anything on that build: they must not, or the
test would compare garbage with garbage.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "two-tower-augmented-with-adaptive-mimic-mechanism_amd"), str(ROOT / "tests")]

import test_gate_rounds_gpu as gr  # noqa: E402


def main(commit: str) -> None:
    cases = {}
    poison_equal = True
    for c in gr.CASES:
        got = gr.run_case(c)
        if any(v != v for l in got["losses"] for v in l.values()):
            raise SystemExit(f"{c.name}: NaN loss on the poisoned workspace: {got['losses']}")
        if gr.run_case(c, poison=False) != got:
            poison_equal = False
            print(f"{c.name}: differs on a zeroed workspace", flush=True)
        cases[c.name] = got
        print(c.name, got["losses"][-1], got.get("eval_loss"), flush=True)
    head = {"commit": commit, "steps": gr.STEPS, "poison_equal": poison_equal}
    lines = [f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in cases.items()]  # a case per line
    gr.GOLDEN.write_text(json.dumps(head)[:-1] + ', "cases": {\n' + ",\n".join(lines) + "\n}}\n")
    print(f"{gr.GOLDEN}: {len(cases)} cases, {gr.GOLDEN.stat().st_size} bytes, poison_equal {poison_equal}")


if __name__ == "__main__":
    main(sys.argv[1])
