"""Generator of tests/golden/warm_start/robust.npz: the robust set of the warm-start tests, measured on the oracle alone.

    python tests/golden/warm_start/make_robust.py            # from the repository root; needs no GPU

For every workload of tests/test_gpu_settings.py (WORKLOADS), each warm-start mode (1, 2) and each warm tick (2, 3) of the three-tick
scenario of tests/_warm_ref.py, the file holds one uint8 mask per instance under the key <workload>_m<mode>_t<tick>: 1 where the
oracle's (status, iteration count, polish flag) of that tick is the same under its stage-wise and its RCM elimination order and
under two warm starts perturbed by 1e-6 relative, the oracle has an answer and the previous tick did not end at the iteration cap
(tests/_warm_ref.py robust_mask).  tests/test_warm_start_host.py regenerates the masks and compares; tests/test_gpu_warm_start.py
holds the device to the oracle's warm tick on the instances of the mask and counts the others.  The key set is recorded in
MANIFEST.json next to the fixture.  The controller workloads are measured a second time with termination checked on every iteration
and the polish off (tests/_warm_ref.py FINE_SETTINGS, keys <workload>_fine_m<mode>_t<tick>): their iteration counts then resolve
single iterations.

Measured shares (robust instances / batch; this script prints the table), the bar being 3/4 of every (workload, mode, tick):

    workload         B   mode 1: tick 2   tick 3       mode 2: tick 2   tick 3
    ctrl8           71   71 (1.000)   71 (1.000)   71 (1.000)   71 (1.000)
    ctrl10          71   71 (1.000)   71 (1.000)   71 (1.000)   71 (1.000)
    ctrl13          71   71 (1.000)   71 (1.000)   71 (1.000)   71 (1.000)
    ctrl20          71   71 (1.000)   71 (1.000)   71 (1.000)   71 (1.000)
    ctrl20d3        71   71 (1.000)   71 (1.000)   71 (1.000)   71 (1.000)
    plan20          67   66 (0.985)   66 (0.985)   66 (0.985)   65 (0.970)
    plan25          67   60 (0.896)   59 (0.881)   61 (0.910)   59 (0.881)
    plan30          67   60 (0.896)   60 (0.896)   61 (0.910)   61 (0.910)
    plan40          67   62 (0.925)   62 (0.925)   61 (0.910)   64 (0.955)
    ctrl8 fine      71   71 (1.000)   71 (1.000)   71 (1.000)   71 (1.000)
    ctrl10 fine     71   71 (1.000)   71 (1.000)   71 (1.000)   71 (1.000)
    ctrl13 fine     71   71 (1.000)   71 (1.000)   71 (1.000)   71 (1.000)
    ctrl20 fine     71   71 (1.000)   71 (1.000)   71 (1.000)   71 (1.000)
    ctrl20d3 fine   71   71 (1.000)   71 (1.000)   71 (1.000)   71 (1.000)

Of the planner instances outside the set, those whose previous tick ended at the iteration cap are 1 (N = 20), 6 to 8 (N = 25), 6
(N = 30) and 3 to 5 (N = 40) per tick; the others flip between the two elimination orders or under the perturbation.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    from tests import _warm_ref as WR
    from tests import test_gpu_settings as G
    masks = {k: v.astype(np.uint8) for k, v in WR.compute_robust().items()}
    np.savez_compressed(os.path.join(HERE, "robust.npz"), **masks)
    man = {"robust.npz": {k: {"dtype": str(v.dtype), "shape": list(v.shape)} for k, v in sorted(masks.items())}}
    with open(os.path.join(HERE, "MANIFEST.json"), "w") as fh:
        json.dump(man, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for n, c in [(n, None) for n in G.WORKLOADS] + [(n, WR.FINE_CASE) for n in WR.FINE_NAMES]:
        row = [masks[WR.fixture_key(n, m, t, c)] for m in WR.MODES for t in WR.WARM_TICKS]
        print("    %-14s %3d   %s" % (n + (" " + c if c else ""), row[0].size, "   ".join("%2d (%.3f)" % (int(r.sum()), r.mean()) for r in row)))


if __name__ == "__main__":
    main()
