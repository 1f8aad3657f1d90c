"""Writes tests/golden/point_mesh_unit_soup.npz: the unit-scale triangle soup of the closest-point tests and the reference's own
`my_point_mesh_face_distance` (src/utils/customized_losses.py:29) on it, in fp32 and in fp64 (not collected by pytest, imported by no test).

    python tests/_make_surface_fixture.py <reference root>

The reference function is IMPORTED from the reference at generation time, with the two pytorch3d imports of its module stubbed (it uses
five accessor methods of Meshes / Pointclouds, stood in for below); none of its text is copied.

The soup: B = 3 meshes of V = 40 vertices (scan 0 seeded, scans 1 and 2 perturbed copies) sharing F = 70 faces -- 67 random faces over
shared vertices, two zero-area faces built on an edge and on a vertex of face 0 (the exact distance to them is never below the distance to
face 0, and the reference drops zero-area faces, so both sides still state the same distance), and face 69 = face 3 duplicated (an exact
tie: the lower face must win).  Faces 0 = (a, b, c) and 1 = (b, a, d) are a roof over their shared edge, on four dyadic vertices that no
other random face uses: a = (-1/2, 0, 2), b = (1/2, 0, 2), c = (0, -1/2, 3/2), d = (0, 1/2, 3/2), above the box the other
vertices lie in, so no other face comes near.  N = 257 points per scan: 240 seeded
ones, then per region of face 0 (A, B, AB, C, AC, BC, interior) two points just off that region, then three points over the ridge: rows 254
and 255 at (1/8, 0, 2 + 1/16) and (-1/4, 0, 2 + 1/8), on the bisector of the dihedral, and row 256 at (1/4, 1/16, 2 + 1/16), off it.  All
three lie in the edge region of BOTH faces and every operation of both region tests is exact on them, so the two fp32 d2 are bitwise equal
(2^-8, 2^-6, 2^-7) although face 1 walks the edge the other way (v = 3/8 against 5/8 in row 254): face 0 must win."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def soup():
    rng = np.random.default_rng(17)
    V, F, N = 40, 70, 257
    v0 = rng.uniform(-1.0, 1.0, (V, 3))
    verts = np.stack([v0, v0 + 0.05 * rng.standard_normal((V, 3)), 0.9 * v0 + 0.03 * rng.standard_normal((V, 3))]).astype(np.float32)
    faces = np.empty((F, 3), np.int32)
    ridge = [int(v) for v in rng.choice(V, 4, replace=False)]                                # a, b, c, d
    free = np.array([v for v in range(V) if v not in ridge])
    for f in range(67):
        faces[f] = rng.choice(free, 3, replace=False)
    faces[0] = ridge[:3]
    faces[1] = (ridge[1], ridge[0], ridge[3])                                                # shares the edge (a, b) of face 0, walked backwards
    verts[:, ridge] = np.array([[-0.5, 0, 2], [0.5, 0, 2], [0, -0.5, 1.5], [0, 0.5, 1.5]], np.float32)
    faces[67] = (faces[0][0], faces[0][0], faces[0][1])                                      # zero area: an edge of face 0
    faces[68] = (faces[0][2],) * 3                                                           # zero area: a vertex of face 0
    faces[69] = faces[3]                                                                     # a duplicate
    pts = np.empty((3, N, 3), np.float64)
    pts[:, :240] = rng.uniform(-1.2, 1.2, (3, 240, 3))
    for b in range(3):
        a, bb, c = (verts[b, faces[0][k]].astype(np.float64) for k in range(3))
        n = np.cross(bb - a, c - a)
        n /= np.linalg.norm(n)
        m = (a + bb + c) / 3
        anchors = [a + 0.05 * (a - m), bb + 0.05 * (bb - m), (a + bb) / 2 + 0.05 * ((a + bb) / 2 - c), c + 0.05 * (c - m),
                   (a + c) / 2 + 0.05 * ((a + c) / 2 - bb), (bb + c) / 2 + 0.05 * ((bb + c) / 2 - a), m]
        k = 240
        for q in anchors:
            for s in (0.01, -0.02):
                pts[b, k] = q + s * n
                k += 1
        pts[b, k:k + 3] = [[0.125, 0, 2.0625], [-0.25, 0, 2.125], [0.25, 0.0625, 2.0625]]
        k += 3
        assert k == N
    return verts, faces, pts.astype(np.float32), np.array([257, 64, 0], np.int32)


def import_reference(root):
    """src/utils/customized_losses.py with `pytorch3d` and `pytorch3d.structures` stubbed."""
    import importlib.util
    p3d, st = types.ModuleType("pytorch3d"), types.ModuleType("pytorch3d.structures")
    p3d._C, p3d.structures = None, st
    st.Meshes = st.Pointclouds = object
    sys.modules.setdefault("pytorch3d", p3d)
    sys.modules.setdefault("pytorch3d.structures", st)
    spec = importlib.util.spec_from_file_location("ref_customized_losses", os.path.join(root, "src", "utils", "customized_losses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.my_point_mesh_face_distance


class _Meshes:
    """The five accessors the reference function calls."""

    def __init__(self, verts, faces):
        self.v, self.f = verts, faces

    def __len__(self):
        return self.v.shape[0]

    def num_faces_per_mesh(self):
        return torch.full((len(self),), self.f.shape[1])

    def verts_padded(self):
        return self.v

    def faces_padded(self):
        return self.f


class _Pointclouds:
    def __init__(self, pts):
        self.p = pts

    def num_points_per_cloud(self):
        return torch.full((self.p.shape[0],), self.p.shape[1])

    def points_padded(self):
        return self.p


def main(root):
    fn = import_reference(root)
    verts, faces, pts, lengths = soup()
    out = {}
    for name, dt in (("ref32", torch.float32), ("ref64", torch.float64)):
        torch.set_default_dtype(dt)                        # the function builds its +inf tensors in the default dtype
        f = torch.from_numpy(faces.astype(np.int64))[None].expand(3, -1, -1).contiguous()
        p2f, _ = fn(_Meshes(torch.from_numpy(verts).to(dt), f), _Pointclouds(torch.from_numpy(pts).to(dt)))
        assert p2f.dtype == dt
        out[name] = p2f.numpy()
    torch.set_default_dtype(torch.float32)
    path = os.path.join(HERE, "golden", "point_mesh_unit_soup.npz")
    np.savez(path, verts=verts, faces=faces, points=pts, lengths=lengths, **out)
    print(path, os.path.getsize(path), "bytes; reference fp32 vs fp64: max", float(np.abs(out["ref32"] - out["ref64"]).max()))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
