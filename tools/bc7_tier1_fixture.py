#!/usr/bin/env python3
"""Takes the first-tier bound fixture of tests/test_bc7_tier1_mfma_gpu.py from a bound-dump build (developer tool, GPU box):
   python tools/bc7_tier1_fixture.py path/to/libcvtt_mi355x_bounddump.so COMMIT [out.npz]
The library is the dump build of the commit the bounds are to be held to (the parent of a change to the first-tier sums, built in
a worktree of its own); COMMIT is recorded in the file.  Default output: tests/golden/bc7_tier1_parent_bounds.npz."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import bc7_tier1_inputs as T1
    from oracle import pyref
    lib, commit = os.path.abspath(sys.argv[1]), sys.argv[2]
    out = sys.argv[3] if len(sys.argv) > 3 else T1.PARENT_FIXTURE
    with tempfile.TemporaryDirectory() as tmp:
        rec = T1.run_dump(tmp, pyref.OracleLib().probe_rcp(), lib=lib)
    keys, vals = T1.tier1_records(rec)
    sets, counts = np.unique(keys[:, 1], return_counts=True)
    print("%d records, %d of the first tier; per bound set %s; dropped %d" % (len(rec), len(keys), dict(zip(sets.tolist(), counts.tolist())), int(vals[:, 2].sum())))
    np.savez_compressed(out, keys=keys.astype(np.uint8), vals=vals, blocks=T1.fixture_blocks(), commit=np.array(commit))
    print("%s: %d bytes" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
