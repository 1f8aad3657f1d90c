"""Writes tests/golden/infopoints_4ddress.npz from the reference's 4D-Dress frame 00122_Inner_Take2_00011 (not collected by pytest, imported by no
test).

    python tests/_make_infopoints_fixture.py <reference root>

The whole frame (80 000 scan faces and the reference's 11 876 info points at full precision) does not fit a small fixture, so this keeps a
horizontal band of it, chosen so that every ray the info-point tests cast from the band sees exactly the geometry it sees in the whole frame:

* inner band: y (the up axis) in [Y0, Y1].  `body_inner_faces` lists the body faces with all three vertices in it: the faces samples are drawn
  from, and the reference records whose body point s = p - v lies in it.
* kept geometry: every scan and body face whose y extent meets [Y0 - MARGIN, Y1 + MARGIN].  Every ray of tests 1-4 for a sample s in the inner
  band stays within 0.16 m of s (test 1 is cut at 0.16; test 4 starts at the scan hit p, |p - s| < 0.16, and an accepted hit lies at s), so
  any face it can hit meets that range: first hits, and so acceptance, are those of the whole frame.  The vertex normals of the inner faces'
  vertices are too (every face around such a vertex is kept).
* faces keep their relative order (ties still go to the same face), vertices are renumbered in their original order.

Vertices are stored as int32 multiples of 1e-8 m: the OBJ files carry exactly 8 decimals, and q / 1e8 (one correctly rounded division) is
the double that etch_amd.inference_demo.load_obj parses.  The reference's .ply is represented by its header and the two lines of every kept
record (the record's scan hit and its body point), as bytes.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from etch_amd.inference_demo import load_obj  # noqa: E402

ID = "00122_Inner_Take2_00011"
Y0, Y1, MARGIN = -1.22, -1.14, 0.17


def _crop(v, f, lo, hi):
    fy = v[f][:, :, 1]
    keep = np.flatnonzero((fy.max(1) >= lo) & (fy.min(1) <= hi))
    used = np.unique(f[keep])
    remap = np.full(len(v), -1, np.int64)
    remap[used] = np.arange(len(used))
    return v[used], remap[f[keep]].astype(np.int32)


def _q(v):
    q = np.round(v * 1e8).astype(np.int64)
    assert np.array_equal(q / 1e8, v) and np.abs(q).max() < 2 ** 31
    return q.astype(np.int32)


def main(ref):
    data = os.path.join(ref, "datafolder")
    scan = load_obj(os.path.join(data, "4D-DRESS", "data_processed", "model", ID, f"{ID}.obj"))
    body = load_obj(os.path.join(data, "4D-DRESS", "data_processed", "smplh", ID, f"mesh_smpl_{ID}.obj"))
    gt = np.load(os.path.join(data, "gt_4D-Dress_data", "npz", f"{ID}.npz"))
    with open(os.path.join(data, "gt_4D-Dress_data", "ply", f"{ID}.ply"), "rb") as fh:
        ply = fh.read().split(b"\n")
    P, V = np.asarray(gt["info_points"], np.float64), np.asarray(gt["info_vectors"], np.float64)
    K = len(P)
    s = P - V
    rec = np.flatnonzero((s[:, 1] >= Y0) & (s[:, 1] <= Y1))
    lo, hi = Y0 - MARGIN, Y1 + MARGIN
    sv, sf = _crop(scan.vertices, scan.faces, lo, hi)
    bv, bf = _crop(body.vertices, body.faces, lo, hi)
    inner = np.flatnonzero((bv[bf][:, :, 1].min(1) >= Y0) & (bv[bf][:, :, 1].max(1) <= Y1)).astype(np.int32)
    assert ply[12] == b"end_header"
    header = b"\n".join(ply[:13]) + b"\n"
    lines = np.array([ply[13 + i] + b"\n" + ply[13 + K + i] + b"\n" for i in rec], dtype=object)
    out = os.path.join(ROOT, "tests", "golden", "infopoints_4ddress.npz")
    np.savez_compressed(out, id=np.array(ID), band=np.array([Y0, Y1, MARGIN]), scan_vertices_e8=_q(sv), scan_faces=sf, body_vertices_e8=_q(bv),
                        body_faces=bf, body_inner_faces=inner, records=rec.astype(np.int32), info_points=P[rec], info_vectors=V[rec],
                        ply_header=np.frombuffer(header, np.uint8), ply_lines=np.frombuffer(b"".join(lines), np.uint8),
                        ply_line_offsets=np.cumsum([0] + [len(x) for x in lines]).astype(np.int64))
    print(out, os.path.getsize(out), "bytes:", len(sf), "scan faces,", len(bf), "body faces,", len(inner), "inner,", len(rec), "records")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "reference")
