"""GPU: the solve kernels' round-off, pinned word for word.

A fixed seeded sample -- 64 controller instances at N = 20, 32 planner instances at N = 30 and 32 at N = 40, default options --
is solved and `xPred, uPred, status, iters, polish, resid` are compared bit for bit with
tests/golden/solve_bits/solve_bits_parent.npz (a directory of its own with its key list beside it, like the other fixtures that
tests/golden/make_golden.py does not write: tests/golden/MANIFEST.json lists that generator's files only).
-0.0 against +0.0 counts as equal and a NaN equals a NaN, as in tools/ab_equal.py; nothing else does.

How the fixture was made: on an MI355X, from the build of the commit BEFORE the solve's factorisation pivots were rewritten
(commit 2a590af, "Give every vehicle of a device fleet or race its own plant parameters"), by
    python3 tests/test_gpu_bitwise_golden.py --record <library file name inside the package directory> tests/golden/solve_bits/solve_bits_parent.npz
(the command also writes the file's keys, shapes and dtypes to MANIFEST.json beside it; a second recording of the same build gave the
same words).
The fixture is a pin of that build's round-off, not a statement about accuracy (the oracle tests hold that): a change that is
meant to alter the arithmetic of a solve kernel regenerates it with the command above and says so; a change that is meant to
leave the arithmetic alone (re-ordered loads, fewer moves, other cross-lane traffic) must pass it unchanged."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


FIXTURE = os.path.join(ROOT, "tests", "golden", "solve_bits", "solve_bits_parent.npz")
CASES = [("controller", 20, 64, 7001), ("planner", 30, 32, 7002), ("planner", 40, 32, 7003)]
KEYS = ("xPred", "uPred", "status", "iters", "polish", "resid")


def solve_sample():
    from lpvmpc import workloads
    res = {}
    for kind, N, B, seed in CASES:
        ctrl = kind == "controller"
        w = (workloads.controller_batch if ctrl else workloads.planner_batch)(B, N=N, seed=seed)
        eng = workloads.make_solver(w)
        o = eng.solve(w["x0"], w["u_prev"], w["vel_ref"] if ctrl else None, w["curv_s"], w["u_old"],
                      None if ctrl else w["max_ey"], *((w["cf_new"], w["lap"]) if ctrl else ()))
        for k in KEYS:
            res["%s_n%d_%s" % (kind, N, k)] = np.array(o[k])
        eng.close()
    return res


def same_words(x, y):
    """Equal word for word, but for the sign of a zero and the payload of a NaN."""
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    if x.tobytes() == y.tobytes():
        return True
    return bool(np.array_equal(x, y, equal_nan=x.dtype.kind == "f"))


@pytest.mark.gpu
def test_seeded_sample_matches_the_recorded_bits():
    gold = np.load(FIXTURE)
    got = solve_sample()
    assert sorted(gold.files) == sorted(got), (sorted(gold.files), sorted(got))
    bad = []
    for name in sorted(got):
        x, y = gold[name], got[name]
        if not same_words(x, y):
            if x.shape == y.shape:
                ne = ~((x == y) | (np.isnan(x.astype(float)) & np.isnan(y.astype(float))))
                bad.append("%s: %d of %d words differ, max |d| %.3g" % (name, int(ne.sum()), x.size,
                                                                        float(np.nanmax(np.abs(x.astype(float) - y.astype(float))))))
            else:
                bad.append("%s: %s %s against %s %s" % (name, y.dtype, y.shape, x.dtype, x.shape))
    assert not bad, "the solve's output words differ from tests/golden/solve_bits/solve_bits_parent.npz:\n  " + "\n  ".join(bad)


def test_fixture_matches_its_key_list():
    """No GPU: the committed fixture holds the keys, shapes and dtypes that the recording wrote beside it, for every case and output."""
    import json
    gold = np.load(FIXTURE)
    man = json.load(open(os.path.join(os.path.dirname(FIXTURE), "MANIFEST.json")))[os.path.basename(FIXTURE)]
    assert sorted(gold.files) == sorted(man) == sorted("%s_n%d_%s" % (kind, N, k) for kind, N, _, _ in CASES for k in KEYS)
    for k in gold.files:
        assert [list(gold[k].shape), str(gold[k].dtype)] == man[k] and gold[k].dtype.kind in "fiu", k
        assert gold[k].shape[0] == {c[1]: c[2] for c in CASES}[int(k.split("_")[1][1:])], k


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] != "--record":
        sys.exit("usage: test_gpu_bitwise_golden.py --record <library file name> <out.npz>")
    from lpvmpc import _ffi
    _ffi.LIB_PATH = os.path.join(os.path.dirname(_ffi.LIB_PATH), sys.argv[2])
    res = solve_sample()
    np.savez_compressed(sys.argv[3], **res)
    # the key set beside the fixture, as the other fixture directories keep it
    import json
    man = {os.path.basename(sys.argv[3]): {k: [list(v.shape), str(v.dtype)] for k, v in sorted(res.items())}}
    with open(os.path.join(os.path.dirname(os.path.abspath(sys.argv[3])), "MANIFEST.json"), "w") as fh:
        json.dump(man, fh, indent=0, sort_keys=True)
    print("recorded %s from %s" % (sys.argv[3], _ffi.LIB_PATH))
