#!/usr/bin/env python3
"""Record what an earlier build of libttamm.so computes for the cases of
tests/test_backward_tail_gpu.py, as tests/golden/backward_tail_parent.json.

The fixture holds the losses and a sha256 of every parameter and optimizer-state tensor after
three one-process steps with the library at the commit before the backward's tail changed
(prefetched dgrad mask rows, slab reduce fused with AdamW).  Run it once on the GPU with that
commit's library (nothing of that build is committed; the file holds recorded results only):

    git worktree add /tmp/ttamm_parent <commit>
    make -C /tmp/ttamm_parent/two-tower-augmented-with-adaptive-mimic-mechanism_amd/csrc
    TTAMM_LIBRARY=/tmp/ttamm_parent/two-tower-augmented-with-adaptive-mimic-mechanism_amd/ttamm/_native/libttamm.so \\
        python tests/golden/make_backward_tail_fixture.py <commit>

It also runs that library's one-stream step (overlap=False) and its clipped step with a
coefficient of 1.0 and records ("twins_equal") whether both are bit-equal to the default step in
every case: where they are, the test uses them as twins that need no fixture.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "two-tower-augmented-with-adaptive-mimic-mechanism_amd"), str(ROOT / "tests")]

import test_backward_tail_gpu as bt  # noqa: E402


def main(commit: str) -> None:
    cases = {}
    twins_equal = {"one-stream": True, "clip-coef-1": True}

    def twin(name, c, got, want):
        if got != want:
            twins_equal[name] = False
            print(f"{bt.case_id(c)}: the {name} twin differs", flush=True)

    for c in bt.CASES:
        base = bt.run_case(c)
        cases[bt.case_id(c)] = base
        twin("one-stream", c, bt.run_case(c, overlap=False), base)
        if c in bt.TWIN_CASES:
            dense = bt.run_case(c, **bt.DENSE_ID)
            cases[bt.dense_id_key(c)] = dense
            twin("clip-coef-1", c, bt.run_case(c, **bt.DENSE_ID, gradient_clip_norm=1e30), dense)
        print(bt.case_id(c), base["losses"][-1], flush=True)
    head = {"commit": commit, "steps": bt.STEPS, "twins_equal": twins_equal}
    lines = [f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in cases.items()]  # a case per line
    bt.GOLDEN.write_text(json.dumps(head)[:-1] + ', "cases": {\n' + ",\n".join(lines) + "\n}}\n")
    print(f"{bt.GOLDEN}: {len(cases)} cases, {bt.GOLDEN.stat().st_size} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
