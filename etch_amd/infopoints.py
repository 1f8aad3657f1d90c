"""MI355X counterpart of scripts/generate_infopoints.py (step 1 of the reference's data preparation) and of the tightness half of
GTDataset.__getitem__ (src/data_utils/GT_dataloader.py:95-122): the supervision the training step consumes.

The reference casts four trimesh / embree ray queries per sample in a Python loop.  Here every query is a batch of rays on the GPU
(csrc/raycast.hip: exact fp64 Moller-Trumbore, Ericson's closest point, angle-weighted vertex normals, the even sampler's thinning); the
host only draws the seeded candidates and compacts between the tests.

One deliberate divergence, `self_face`: the reference's test 3 casts from the body sample s along -n against the body itself, and in about
half of the samples the ray "hits" the triangle s lies on at t ~ 0 (embree's float32 tnear = 0 decides), so the sample is dropped as an
"intersection between smpl parts".  The default, "exclude", skips the sample's own face in that test; "reference" keeps it and so
reproduces the reference's yield.
"""
import os
import warnings

import numpy as np
import torch

from . import ops

SELF_FACE_MODES = ("exclude", "reference")


def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def mesh_to_device(mesh, device=None):
    """(vertices (V,3) fp64, faces (F,3) int32) on the device from anything with .vertices / .faces."""
    dev = _device(device)
    v = torch.as_tensor(np.ascontiguousarray(mesh.vertices, np.float64), device=dev)
    f = torch.as_tensor(np.ascontiguousarray(mesh.faces, np.int32), device=dev)
    return v, f


def _face_areas(vertices, faces):
    tri = np.asarray(vertices, np.float64)[np.asarray(faces)]
    return 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)


def sample_surface(mesh, count, seed=0):
    """Area-weighted faces and uniform barycentrics (host numpy, the recipe of inference_demo.sample_points_from_mesh) ->
    points (count,3), face (count) int64, bary (count,3): points = v0 + r1 (v1 - v0) + r2 (v2 - v0), bary = (1 - r1 - r2, r1, r2)."""
    rng = np.random.default_rng(seed)
    tri = np.asarray(mesh.vertices, np.float64)[np.asarray(mesh.faces)]
    area = _face_areas(mesh.vertices, mesh.faces)
    face = rng.choice(len(area), size=count, p=area / area.sum())
    r = rng.random((count, 2))
    flip = r.sum(1) > 1
    r[flip] = 1 - r[flip]
    t = tri[face]
    points = t[:, 0] + r[:, :1] * (t[:, 1] - t[:, 0]) + r[:, 1:] * (t[:, 2] - t[:, 0])
    bary = np.stack([1.0 - r[:, 0] - r[:, 1], r[:, 0], r[:, 1]], axis=1)
    return points, face.astype(np.int64), bary


def sample_surface_even(mesh, count, seed=0, radius=None, device=None):
    """trimesh.sample.sample_surface_even: 3 count seeded candidates, thinned on the GPU by remove_close with radius sqrt(area / (3 count)),
    -> the first `count` survivors (points, face, bary as sample_surface), or all of them with a warning if fewer remain."""
    if radius is None:
        radius = float(np.sqrt(_face_areas(mesh.vertices, mesh.faces).sum() / (3 * count)))
    points, face, bary = sample_surface(mesh, 3 * count, seed)
    _, removed = ops.remove_close(torch.as_tensor(points, device=_device(device)), radius)
    keep = ~removed.cpu().numpy()
    points, face, bary = points[keep], face[keep], bary[keep]
    if len(points) < count:
        warnings.warn(f"only got {len(points)}/{count} samples!")
    return points[:count], face[:count], bary[:count]


def interpolate_normals(vertex_normals, faces, face, bary):
    """Per-sample normal: (b0 n[v0] + b1 n[v1]) + b2 n[v2], normalised (generate_infopoints.py:94-96).  Device tensors, fp64."""
    fv = faces[face.long()].long()
    n = (bary[:, 0:1] * vertex_normals[fv[:, 0]] + bary[:, 1:2] * vertex_normals[fv[:, 1]]) + bary[:, 2:3] * vertex_normals[fv[:, 2]]
    return n / torch.sqrt((n * n).sum(1, keepdim=True))


def trace_samples(scan_dev, body_dev, points, face, bary, ray_length=0.16, ray_length_ops=0.025, self_face="exclude", body_normals=None):
    """The four tests of generate_infopoints.py:120-185 for body samples (points (S,3), their face (S) and barycentrics (S,3) on the body),
    every test one batch of rays.  scan_dev / body_dev = mesh_to_device(...).  Returns (keep (K) int64 sample indices in ascending order,
    info_points (K,3), info_vectors (K,3), counts) on the device; counts = samples and the rejections of each test."""
    if self_face not in SELF_FACE_MODES:
        raise ValueError(f"self_face must be one of {SELF_FACE_MODES}, got {self_face!r}")
    sv, sf = scan_dev
    bv, bf = body_dev
    dev = bv.device
    s = torch.as_tensor(points, dtype=torch.float64, device=dev).contiguous()
    fc = torch.as_tensor(face, device=dev).to(torch.int32).contiguous()
    b = torch.as_tensor(bary, dtype=torch.float64, device=dev)
    S = s.shape[0]
    if body_normals is None:
        body_normals = ops.vertex_normals(bv, bf)
    n = interpolate_normals(body_normals, bf, fc, b).contiguous()
    neg = (-n).contiguous()
    full = lambda v: torch.full((S,), float(v), dtype=torch.float64, device=dev)  # noqa: E731
    # 1. the scan along +n, closer than ray_length: p
    f1, _, _, p = ops.ray_first_hit(s, n, sv, sf, t_max=full(ray_length))
    ok1 = f1 >= 0
    # 2. rejected if the scan lies along -n closer than ray_length_ops
    f2, _, _, _ = ops.ray_first_hit(s, neg, sv, sf, t_max=full(ray_length_ops))
    ok2 = ok1 & (f2 < 0)
    # 3. rejected if the body itself lies along -n closer than 0.03 ("intersection between smpl parts"); "exclude" skips the sample's own face
    f3, _, _, _ = ops.ray_first_hit(s, neg, bv, bf, excl_face=fc if self_face == "exclude" else None, t_max=full(0.03))
    ok3 = ok2 & (f3 < 0)
    # 4. from p along -n the body must be hit within 1e-4 of s (survivors of 1-3 only)
    idx = torch.nonzero(ok3).flatten()
    f4, _, _, loc = ops.ray_first_hit(p[idx].contiguous(), neg[idx].contiguous(), bv, bf)
    e = loc - s[idx]
    ok4 = (f4 >= 0) & (torch.sqrt((e * e).sum(1)) < 1e-4)
    keep = idx[ok4]
    info_points = p[keep]
    info_vectors = info_points - s[keep]
    n1, n2, n3, n4 = (int(v) for v in torch.stack([ok1.sum(), ok2.sum(), ok3.sum(), ok4.sum()]).cpu())
    counts = {"samples": S, "rejected_test1": S - n1, "rejected_test2": n1 - n2, "rejected_test3": n2 - n3, "rejected_test4": n3 - n4,
              "accepted": n4}
    return keep, info_points, info_vectors, counts


def generate_infopoints(scan, body, num_samples=30000, ray_length=0.16, ray_length_ops=0.025, seed=0, self_face="exclude", device=None):
    """scripts/generate_infopoints.py:get_data for one (scan, fitted body) pair (meshes with .vertices / .faces) -> (info_points (K,3) fp64,
    info_vectors (K,3) fp64 = info point - body sample, in sample order, counts: the samples and each test's rejections)."""
    scan_dev, body_dev = mesh_to_device(scan, device), mesh_to_device(body, device)
    points, face, bary = sample_surface_even(body, num_samples, seed=seed, device=body_dev[0].device)
    _, ip, iv, counts = trace_samples(scan_dev, body_dev, points, face, bary, ray_length, ray_length_ops, self_face)
    return ip.cpu().numpy(), iv.cpu().numpy(), counts


def tightness_vectors(sample_points, info_points, info_vectors, body, threshold=0.01, device=None):
    """GT_dataloader.py:105-122: a scan point takes the vector of its nearest info point when that point lies closer than `threshold`, else
    (point - its closest point on the body).  The nearest info point comes from ops.nn_bidir (exact fp32 distances, ties -> lowest index);
    the threshold is tested on the fp64 distance to it.  -> (vectors (N,3) fp64, use_info (N) bool), numpy."""
    dev = _device(device)
    x = torch.as_tensor(np.asarray(sample_points, np.float64), device=dev)
    bv, bf = mesh_to_device(body, dev)
    _, _, closest, _ = ops.closest_point_on_mesh(x, bv, bf)
    vectors = x - closest
    use = torch.zeros((x.shape[0],), dtype=torch.bool, device=dev)
    if len(info_points):
        ip = torch.as_tensor(np.asarray(info_points, np.float64), device=dev)
        iv = torch.as_tensor(np.asarray(info_vectors, np.float64), device=dev)
        idx, _, _, _ = ops.nn_bidir(x.float()[None].contiguous(), ip.float()[None].contiguous())
        j = idx[0].long()
        e = x - ip[j]
        use = torch.sqrt((e * e).sum(1)) < threshold
        vectors = torch.where(use[:, None], iv[j], vectors)
    return vectors.cpu().numpy(), use.cpu().numpy()


# ---------------------------------------------------------------------------------------------- output files (generate_infopoints.py:21-65)
def save_data(info_points, info_vectors, file_path):
    """<id>.npz with keys info_points / info_vectors."""
    np.savez(file_path, info_points=np.asarray(info_points, np.float64).reshape(-1, 3), info_vectors=np.asarray(info_vectors, np.float64).reshape(-1, 3))


def save_points_with_vector(args, hit_points, vectors, file_path):
    """The reference's ASCII .ply, byte for byte: the info points (red), their body points (blue) and an edge between each pair.
    `args` is unused, as in the reference."""
    num_points = len(hit_points)
    assert num_points == len(vectors)
    hit_points = np.asarray(hit_points, np.float64).reshape(-1, 3)
    vectors = np.asarray(vectors, np.float64).reshape(-1, 3)
    vector_end_points = hit_points - vectors
    with open(file_path, "w") as f:
        f.write("ply\n")
        f.write("format ascii 1.0\n")
        f.write(f"element vertex {num_points * 2}\n")
        f.write("property float x\n")
        f.write("property float y\n")
        f.write("property float z\n")
        f.write("property uchar red\n")
        f.write("property uchar green\n")
        f.write("property uchar blue\n")
        f.write(f"element edge {num_points}\n")
        f.write("property int vertex1\n")
        f.write("property int vertex2\n")
        f.write("end_header\n")
        for p in hit_points:
            f.write(f"{p[0]} {p[1]} {p[2]} 255 0 0\n")
        for v in vector_end_points:
            f.write(f"{v[0]} {v[1]} {v[2]} 0 0 255\n")
        for i in range(num_points):
            f.write(f"{i} {num_points + i}\n")


def write_outputs(info_points, info_vectors, ply_path, npz_path):
    for pth in (ply_path, npz_path):
        d = os.path.dirname(pth)
        if d:
            os.makedirs(d, exist_ok=True)
    save_points_with_vector(None, info_points, info_vectors, ply_path)
    save_data(info_points, info_vectors, npz_path)
