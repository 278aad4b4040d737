#!/usr/bin/env python3
"""Generate tests/golden/track_edges/track_edges.npz from the REFERENCE's own Map (Utilities/trackInitialization.py) and Curvature
(Utilities/utilities.py), read from the reference tree at generation time only and imported with the stub machinery of
../make_golden.py.  Nothing of the reference's text is stored: only the grid's inputs and the numbers its functions return.

The points are the edge grid of tests/_track_edges.py (seams, lap ends, closing rows, the width limit, headings turns away from the
tangent) for the reference's four shapes, whose tables must equal the package's word for word (asserted).  Per shape:
  table [rows, 6], hw, slack
  g_sey [n, 2], g_out [n, 3], g_raised [n]         Map.getGlobalPosition(s, ey); NaN and 1 where the call raised
  c_s [k], c_out [k], c_raised [k]                 Curvature(s, PointAndTangent)
  l_x, l_y, l_psi [m], l_s, l_ey, l_epsi [m], l_inside [m], l_raised [m]      Map.getLocalPosition(x, y, psi)
float64 and int32 only.  s = +inf is left out: the reference subtracts the lap length from it for ever.  The archive is written with
fixed time stamps, so a second run reproduces the file byte for byte.  The key set is recorded in MANIFEST.json next to it.

Usage:  python tests/golden/track_edges/make_track_edges_golden.py [--out DIR]   (needs the reference tree; not run on the GPU machine)
"""
import io
import json
import os
import shutil
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)


def write_npz(path, arrays):
    """numpy's .npz layout with every member stamped 1980-01-01, members in sorted order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def scalar(v):
    a = np.asarray(v, float).reshape(-1)
    if a.size != 1:
        raise ValueError("not one value")
    return float(a[0])


def main():
    out_dir = HERE
    if "--out" in sys.argv:
        out_dir = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(out_dir, exist_ok=True)
    warnings.simplefilter("ignore")
    import make_golden as MG
    from tests import _track_edges as E
    CTRL, PLAN, TRACK, UTIL, tmp = MG.import_reference()
    out = {}
    try:
        maps = E.tracks()
        for t, shape in enumerate(E.REFERENCE_SHAPES):
            mp = MG.make_map(TRACK, shape)
            m = maps[t]
            tab = np.array(mp.PointAndTangent, float)
            assert m.shape == shape and np.array_equal(tab, m.PointAndTangent) and mp.halfWidth == m.halfWidth and mp.slack == m.slack, shape
            sey = E.global_points(m)[0]
            sey = sey[~np.isposinf(sey[:, 0])]
            g_out, g_raised = np.full((sey.shape[0], 3), np.nan), np.zeros(sey.shape[0], np.int32)
            for n, (s, ey) in enumerate(sey):
                try:
                    g_out[n] = [scalar(v) for v in mp.getGlobalPosition(float(s), float(ey))]
                except Exception:
                    g_raised[n] = 1
            c_s = E.s_grid(tab)[0]
            c_s = c_s[~np.isposinf(c_s)]
            c_out, c_raised = np.full(c_s.size, np.nan), np.zeros(c_s.size, np.int32)
            for n, s in enumerate(c_s):
                try:
                    c_out[n] = scalar(UTIL.Curvature(float(s), mp.PointAndTangent))
                except Exception:
                    c_raised[n] = 1
            pts = E.local_points(m)["pts"]
            l_out, l_raised = np.full((pts.shape[0], 4), np.nan), np.zeros(pts.shape[0], np.int32)
            for n, p in enumerate(pts):
                try:
                    l_out[n] = [scalar(v) for v in mp.getLocalPosition(float(p[0]), float(p[1]), float(p[2]))]
                except Exception:
                    l_raised[n] = 1
            assert not l_raised.any(), shape
            arrays = dict(table=tab, hw=np.array(float(mp.halfWidth)), slack=np.array(float(mp.slack)), g_sey=sey, g_out=g_out, g_raised=g_raised,
                          c_s=c_s, c_out=c_out, c_raised=c_raised, l_x=pts[:, 0], l_y=pts[:, 1], l_psi=pts[:, 2], l_s=l_out[:, 0],
                          l_ey=l_out[:, 1], l_epsi=l_out[:, 2], l_inside=l_out[:, 3].astype(np.int32), l_raised=l_raised)
            out.update({shape + "_" + k: v for k, v in arrays.items()})
            print("%s: %d global (%d raised), %d curvature (%d raised), %d local (%d inside)"
                  % (shape, sey.shape[0], g_raised.sum(), c_s.size, c_raised.sum(), pts.shape[0], int(l_out[:, 3].sum())))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    write_npz(os.path.join(out_dir, "track_edges.npz"), out)
    manifest = {"track_edges.npz": {k: {"shape": list(np.shape(v)), "dtype": str(np.asarray(v).dtype)} for k, v in sorted(out.items())}}
    with open(os.path.join(out_dir, "MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote track_edges.npz (%d bytes)" % os.path.getsize(os.path.join(out_dir, "track_edges.npz")))


if __name__ == "__main__":
    main()
