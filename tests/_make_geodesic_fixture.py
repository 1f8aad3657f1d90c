"""Writes tests/golden/geodesic_4ddress.npz from the reference's 4D-Dress SMPL body of frame 00122_Inner_Take2_00011 and the default markerset
(not collected by pytest, imported by no test).

    python tests/_make_geodesic_fixture.py <reference root>

Contents: the body (vertices as int32 multiples of 1e-8 m, the OBJ's 8 decimals, and faces), the oracle's (tests/_geodesic_oracle.py) flip
count and flipped edges of the subdivided body, the min distance (fp64), label and second-best margin (fp32) per subdivided vertex, the full
distance column of marker 0 under both Laplacians, and the oracle's max error against the analytic distance on the icosphere and the grid
of the known-answer tests."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _geodesic_oracle as O  # noqa: E402
from etch_amd import constants as K  # noqa: E402
from etch_amd.inference_demo import load_obj  # noqa: E402

ID = "00122_Inner_Take2_00011"


def known_answers():
    """(icosphere max |d - great-circle| over the oracle's column of vertex 0, grid max |d - euclid| within 0.3 of the centre)."""
    v, f = O.icosphere(4)
    s = O.HeatSolver(v, f)
    d = s.distance(0)
    gc = np.arccos(np.clip(v @ v[0], -1, 1))
    g, gf = O.planar_grid(33)
    c = 16 * 33 + 16
    sg = O.HeatSolver(g, gf)
    dg = sg.distance(c)
    eu = np.linalg.norm(g - g[c], axis=1)
    near = eu < 0.3
    return float(np.abs(d - gc).max()), float(np.abs(dg - eu)[near].max())


def main(ref):
    body = load_obj(os.path.join(ref, "datafolder/4D-DRESS/data_processed/smplh", ID, f"mesh_smpl_{ID}.obj"))
    q = np.rint(body.vertices * 1e8).astype(np.int64)
    assert np.all(np.abs(q) < 2 ** 31) and np.array_equal(q / 1e8, body.vertices)
    v = q / 1e8
    mv = list(K.default_markerset().values())
    dmin, lab, margin, cols, s = O.marker_fields(v, body.faces, mv, keep=(0,))
    sv, sf = O.subdivide(v, body.faces)
    ref_mesh = O.EdgeMesh(sv, sf)
    changed = np.flatnonzero(np.any(ref_mesh.ev != s.mesh.ev, axis=1))
    cot = O.HeatSolver(sv, sf, laplacian="cotan")
    ico_err, grid_err = known_answers()
    out = os.path.join(ROOT, "tests", "golden", "geodesic_4ddress.npz")
    np.savez_compressed(out, vertices_q=q.astype(np.int32), faces=np.asarray(body.faces, np.int16), markers=np.asarray(mv, np.int32),
                        flips=np.int64(s.flips), flipped_edges=changed.astype(np.int32), flipped_ev=s.mesh.ev[changed].astype(np.int32),
                        min_dist=dmin, label=lab.astype(np.uint8), margin=margin.astype(np.float32), dist0=cols[0],
                        dist0_cotan=cot.distance(mv[0]), ico_err=np.float64(ico_err), grid_err=np.float64(grid_err))
    print(out, os.path.getsize(out), "flips", s.flips, "ico", ico_err, "grid", grid_err, "margin<1e-6:", int((margin < 1e-6).sum()))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
