"""Raw point clouds as input: cleaning and evening out a cloud a scanner, photogrammetry or a depth sensor delivered, and
handing it to the pipeline.

    pack(list_of_arrays) -> Cloud                              a ragged batch of (n,3) arrays as depth.Cloud (index = the original row)
    knn_mean_distance(cloud, k, cell=None, brute=False)        mean distance of every point to its k nearest neighbours (exact grid kNN)
    remove_statistical_outliers(cloud, k=16, ratio=2.0)        keep m_i <= mean + ratio * std over the cloud
    remove_radius_outliers(cloud, radius, min_neighbours)      keep the points with enough neighbours within radius
    voxel_downsample(cloud, voxel)                             one centroid per occupied cell, in spatial (ix, iy, iz) order
    prepare(cloud, N, keys, voxel=, stat=, radius=, floor=, cluster=)   filters, floor, largest cluster, voxel grid, centre, pick: the network's input

    fit_plane(cloud, threshold, keys, ...), remove_plane(...)  the dominant plane by RANSAC + one refit; drop it and what lies under it (section 22)
    cluster(cloud, radius), keep_clusters(cloud, radius, ...)  Euclidean clusters = components of the radius graph; keep the largest

    python -m etch_amd.cloud --cloud_path scan.ply [--voxel V] [--outlier_k K --outlier_ratio R] [--outlier_radius r --outlier_min_neighbours m]
                             [--floor_threshold T --floor_up X Y Z --floor_max_tilt DEG] [--cluster_radius R]
                             [--more_views B.ply C.ply .. --align_gate G --align_gate_min g --align_decay D --align_iters K --align_metric {point,plane} --align_normal_k K
                              --view_init F.npz --fuse_voxel V
                              --align_global --align_global_voxel V --align_feature_k K --align_hypotheses H --view_origin X Y Z]

    nearest(source, target, gate), align(source, target, ...)  gated nearest rows across two clouds; rigid registration by ICP on the cell grid (section 23)
    transform(cloud, R, t), register_views(views), fuse(views, transforms, voxel=)   several views into one frame, one cloud per subject

    normals(cloud, k=16, viewpoint=None)                       unit normal, surface variation and flag per row from the k nearest rows (section 24)

    features(cloud, k=32, viewpoint=), global_align(source, target, keys, viewpoint=(vs, vt), ...)   FPFH descriptors; a rough pose from nothing by
                                                               feature matches and RANSAC, the start of align(init="global") (section 25)

    reconstruct(surface, voxel) -> Reconstruction   the watertight mesh of an OrientedCloud (section 27): the level set |w| = 0.5 of its winding
                                  number by marching tetrahedra on blocks that follow the surface
    areas(cloud, k=8), orient_normals(cloud, normals, sensors), surface(cloud, sensors=, normals=) -> OrientedCloud   a cloud with an inside (section 26):
                                                               what etch_amd.containment and fit_surface(scan=) take in place of a mesh
    fuse(views, transforms, voxel=, return_view=True)          also the view every fused row came from

    python -m etch_amd.cloud ... --surface_refine [--surface_iters I ..] [--surface_contain --contain_w W --contain_every K --contain_normal_k K --contain_area_k K]
                             the dense surface refinement (section 17) on the cleaned cloud's fit, with --surface_contain kept inside the cleaned cloud:
                             several views (their sensors: --view_origin through the registration) or one file that carries normals

Neighbours are rows of the same cloud only.  The kernels (csrc/cloud_filter.hip, csrc/cloud_isolate.hip, csrc/cloud_align.hip, csrc/cloud_normals.hip, csrc/cloud_global.hip) are exact and defined in fp64, the sweep of csrc/cloud_winding.hip in fp32 to the bit; there is no CPU path."""
import argparse
import math
import os

import numpy as np

from . import _lib
from .depth import Cloud

STATUS_NONFINITE, STATUS_RANGE, STATUS_EMPTY = 1, 2, 4
MAX_K = 32


def pack(arrays, device="cuda"):
    """A list of (n,3) arrays -> Cloud(points (M,3) fp64, index (M) int32 = the row inside its own array, offsets (B+1) int32, count (B)
    int32, depth None) on the device.  An array may be empty; non-finite coordinates are reported by the call that meets them."""
    import torch
    arrays = [np.asarray(a) for a in ([arrays] if isinstance(arrays, np.ndarray) and arrays.ndim == 2 else arrays)]
    if not arrays:
        raise ValueError("no cloud to pack")
    for k, a in enumerate(arrays):
        if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "fiu":
            raise ValueError(f"cloud {k}: needs an (n,3) array of numbers, got {a.dtype} {a.shape}")
    n = np.array([len(a) for a in arrays], np.int64)
    if n.sum() >= 2 ** 31 // 3:
        raise ValueError("the batch is too large for 32-bit offsets: filter it in parts")
    dev = torch.device(device)
    pts = np.ascontiguousarray(np.concatenate([a.astype(np.float64) for a in arrays]))
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    idx = np.concatenate([np.arange(m, dtype=np.int32) for m in n])
    return Cloud(torch.from_numpy(pts).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(n.astype(np.int32)).to(dev), None)


def _offsets(cloud):
    """The host's copy of a cloud's offsets, checked: bad offsets raise before any launch."""
    o = cloud.offsets.cpu().numpy().astype(np.int64)
    M = cloud.points.shape[0]
    if cloud.points.dim() != 2 or cloud.points.shape[1] != 3 or o.ndim != 1 or len(o) < 2:
        raise ValueError(f"a cloud is points (M,3) and offsets (B+1) with B >= 1, got {tuple(cloud.points.shape)} and {tuple(cloud.offsets.shape)}")
    if o[0] != 0 or (np.diff(o) < 0).any() or o[-1] > M:
        raise ValueError(f"offsets must start at 0, not decrease and end within the {M} rows, got {o.tolist() if len(o) <= 9 else o[:9].tolist()}")
    if cloud.index.shape != (M,):
        raise ValueError(f"index must be ({M},), got {tuple(cloud.index.shape)}")
    return o


def _check_k(k):
    if int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in 1 .. {MAX_K}, got {k}")
    return int(k)


def _check_positive(x, name):
    if not (float(x) > 0.0 and math.isfinite(float(x))):
        raise ValueError(f"{name} must be positive and finite, got {x}")
    return float(x)


def _raise_status(what, status):
    status = np.asarray(status)
    if status.any():
        b = int(np.flatnonzero(status)[0])
        s = int(status[b])
        why = ("a coordinate is not finite" if s & STATUS_NONFINITE else "an axis has more than 2^21 voxels: the voxel size is too small for the cloud's extent"
               if s & STATUS_RANGE else "the cloud has no point")
        raise _lib.EtchHipError(f"{what}: cloud {b}: {why}")


def _ops(cloud):
    import torch

    from . import ops
    return torch, ops, torch.cuda.device(cloud.points.device)


def knn_mean_distance(cloud, k, cell=None, brute=False):
    """m_i = the mean distance from row i to its min(k, n - 1) nearest other rows of its cloud (0 where the cloud has one row), (M) fp64 on the
    device.  The cell size is internal (ops.cloud_cell_grid states the rule); cell= overrides it and brute=True scans every cloud whole for every
    query -- the bits are the same in every form.  ValueError for k outside 1 .. 32 or bad offsets, before any launch; EtchHipError naming the
    cloud that holds a non-finite coordinate, after the one status readback."""
    k = _check_k(k)
    if cell is not None:
        _check_positive(cell, "cell")
    o = _offsets(cloud)
    torch, ops, ctx = _ops(cloud)
    with ctx:
        mean, status = ops.cloud_knn_mean(cloud.points, cloud.offsets, k, cell=cell, brute=brute)
    _raise_status("knn_mean_distance", status.cpu().numpy())
    return mean[:int(o[-1])]


NORMAL_FLAG_FEW, NORMAL_FLAG_AMBIGUOUS = 1, 2
NORMAL_MIN_K = 3


def _check_normal_k(k):
    if int(k) != k or not NORMAL_MIN_K <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in {NORMAL_MIN_K} .. {MAX_K}, got {k}")
    return int(k)


def _viewpoint(viewpoint, B, dev):
    """None, one position (3,) for every cloud or (B,3) -> None or a (B,3) fp64 tensor on the device; ValueError for any other shape."""
    import torch
    if viewpoint is None:
        return None
    v = viewpoint.detach().cpu().numpy() if isinstance(viewpoint, torch.Tensor) else np.asarray(viewpoint)
    if v.dtype.kind not in "fiu" or v.shape not in ((3,), (B, 3)):
        raise ValueError(f"viewpoint must be (3,) or ({B},3) numbers, got {v.dtype} {v.shape}")
    v = np.array(np.broadcast_to(v.astype(np.float64), (B, 3)), order="C")
    if not np.isfinite(v).all():
        raise ValueError("viewpoint must be finite")
    return torch.from_numpy(v).to(dev)


def normals(cloud, k=16, viewpoint=None, cell=None, brute=False, return_cov=False):
    """Surface normals from the k nearest rows: -> normal (M,3) fp64, variation (M) fp64, flag (M) int32 on the device (and the
    covariance (M,6) with return_cov).  The normal is the unit eigenvector of the smallest eigenvalue of the neighbourhood's covariance, variation
    that eigenvalue over the trace; a row with flag != 0 (NORMAL_FLAG_FEW: a cloud of 1 or 2 rows, NORMAL_FLAG_AMBIGUOUS: collinear, coincident or
    isotropic neighbours) gets (0, 0, 0).  Sign: the largest component positive, or towards `viewpoint` ((3,) or one position per cloud) --
    nothing is propagated from row to row, so the field is not globally consistent on a closed surface without a viewpoint.  cell= and brute=True
    change no bit.  ValueError for k outside 3 .. 32, a bad viewpoint or bad offsets, before any launch; EtchHipError naming the cloud that holds a
    non-finite coordinate."""
    k = _check_normal_k(k)
    if cell is not None:
        _check_positive(cell, "cell")
    o = _offsets(cloud)
    view = _viewpoint(viewpoint, len(o) - 1, cloud.points.device)
    torch, ops, ctx = _ops(cloud)
    with ctx:
        out = ops.cloud_normals(cloud.points, cloud.offsets, k, viewpoint=view, cell=cell, brute=brute, return_cov=return_cov)
    _raise_status("normals", out[3].cpu().numpy())
    total = int(o[-1])
    res = (out[0][:total], out[1][:total], out[2][:total])
    return res + (out[4][:total],) if return_cov else res


def radius_neighbour_count(cloud, radius, brute=False):
    """c_i = the number of other rows of its cloud within `radius` of row i (d2 <= radius * radius), (M) int32 on the device."""
    radius = _check_positive(radius, "radius")
    o = _offsets(cloud)
    torch, ops, ctx = _ops(cloud)
    with ctx:
        count, status = ops.cloud_radius_count(cloud.points, cloud.offsets, radius, brute=brute)
    _raise_status("radius_neighbour_count", status.cpu().numpy())
    return count[:int(o[-1])]


def _compact(ops, cloud, keep):
    kept, offsets, index, points = ops.cloud_compact(cloud.points, cloud.index, cloud.offsets, keep)
    return Cloud(points, index, offsets, kept, None)


def _trim(cloud, total):
    cloud.points, cloud.index = cloud.points[:total], cloud.index[:total]
    return cloud


def _stat(ops, cloud, k, ratio):
    mean, status = ops.cloud_knn_mean(cloud.points, cloud.offsets, k)
    keep, stats = ops.cloud_stat_keep(mean, cloud.offsets, ratio, status)
    return keep, stats, status


def _check_stat(k, ratio):
    if not math.isfinite(float(ratio)):
        raise ValueError(f"ratio must be finite, got {ratio}")
    return _check_k(k), float(ratio)


def _check_radius(radius, min_neighbours):
    if int(min_neighbours) != min_neighbours or int(min_neighbours) < 0:
        raise ValueError(f"min_neighbours must be a non-negative integer, got {min_neighbours}")
    return _check_positive(radius, "radius"), int(min_neighbours)


def remove_statistical_outliers(cloud, k=16, ratio=2.0, return_stats=False):
    """Statistical outlier removal per cloud: keep_i = m_i <= mu + ratio s with mu, s the mean and the (n - 1) standard deviation of the m_i of
    knn_mean_distance.  -> (Cloud of the kept rows in row order, keep (M) bool on the device) [, stats (B,2) fp64 = mu, s]."""
    k, ratio = _check_stat(k, ratio)
    o = _offsets(cloud)
    torch, ops, ctx = _ops(cloud)
    with ctx:
        keep, stats, status = _stat(ops, cloud, k, ratio)
        out = _compact(ops, cloud, keep)
        host = torch.cat([status, out.offsets]).cpu().numpy()              # the one readback
    B = len(o) - 1
    _raise_status("remove_statistical_outliers", host[:B])
    out = _trim(out, int(host[-1]))
    keep = keep[:int(o[-1])].bool()
    return (out, keep, stats) if return_stats else (out, keep)


def remove_radius_outliers(cloud, radius, min_neighbours):
    """Radius outlier removal: keep the rows with at least min_neighbours other rows of their cloud within radius.  -> (Cloud, keep (M) bool)."""
    radius, min_neighbours = _check_radius(radius, min_neighbours)
    o = _offsets(cloud)
    torch, ops, ctx = _ops(cloud)
    with ctx:
        count, status = ops.cloud_radius_count(cloud.points, cloud.offsets, radius)
        keep = (count >= min_neighbours).to(torch.int32)
        out = _compact(ops, cloud, keep)
        host = torch.cat([status, out.offsets]).cpu().numpy()
    B = len(o) - 1
    _raise_status("remove_radius_outliers", host[:B])
    return _trim(out, int(host[-1])), keep[:int(o[-1])].bool()


def _voxel(ops, cloud, voxel):
    offsets, centroid, count, lowest, cell, status = ops.cloud_voxel_grid(cloud.points, cloud.offsets, voxel)
    out = Cloud(centroid, lowest, offsets, offsets[1:] - offsets[:-1], None)
    out.cell = cell
    return out, count, status


def voxel_downsample(cloud, voxel):
    """Voxel-grid down-sampling: cell = floor((p - o) / voxel) with o the cloud's bounding-box minimum; one output row per occupied cell in
    ascending (ix, iy, iz) order = the centroid of its rows.  -> (Cloud whose index is the cell's lowest row and whose .cell (., 3) int32 are
    the cell coordinates, count (.) int32 = the rows of each cell).  EtchHipError naming the cloud where an axis has more than 2^21 cells."""
    voxel = _check_positive(voxel, "voxel")
    o = _offsets(cloud)
    torch, ops, ctx = _ops(cloud)
    with ctx:
        out, count, status = _voxel(ops, cloud, voxel)
        host = torch.cat([status, out.offsets]).cpu().numpy()
    B = len(o) - 1
    _raise_status("voxel_downsample", host[:B])
    total = int(host[-1])
    out.cell = out.cell[:total]
    return _trim(out, total), count[:total]


# ---------------------------------------------------------------------------------------------------------------- isolating the subject
MAX_HYPOTHESES = 65536


def _check_plane(B, threshold, keys, hypotheses=1024, up=None, max_tilt=None, min_inliers=3, refit=True):
    """fit_plane's arguments, checked before any launch.  -> a dict: tau, keys (B) int64 numpy, H, up (a unit 3-tuple or None), cos_tilt,
    min_inliers, refit."""
    from . import mesh_io
    tau = _check_positive(threshold, "threshold")
    if int(hypotheses) != hypotheses or not 1 <= int(hypotheses) <= MAX_HYPOTHESES:
        raise ValueError(f"hypotheses must be an integer in 1 .. {MAX_HYPOTHESES}, got {hypotheses}")
    if int(min_inliers) != min_inliers or int(min_inliers) < 0:
        raise ValueError(f"min_inliers must be a non-negative integer, got {min_inliers}")
    cos_tilt = 0.0
    if max_tilt is not None:
        if not 0.0 <= float(max_tilt) <= 90.0:
            raise ValueError(f"max_tilt must lie in [0, 90] degrees, got {max_tilt}")
        if up is None:
            raise ValueError("max_tilt needs up")
        cos_tilt = 0.0 if float(max_tilt) == 90.0 else min(1.0, math.cos(math.radians(float(max_tilt))))
    if up is not None:
        u = np.asarray(up, np.float64).reshape(-1)
        if u.shape != (3,) or not np.isfinite(u).all() or not float(np.sqrt((u * u).sum())) > 0.0:
            raise ValueError(f"up must be three finite numbers, not all zero, got {up}")
        u = u / np.sqrt((u * u).sum())
        up = (float(u[0]), float(u[1]), float(u[2]))
    return dict(tau=tau, keys=mesh_io._keys(keys, B), H=int(hypotheses), up=up, cos_tilt=cos_tilt, min_inliers=int(min_inliers), refit=bool(refit))


def _plane(torch, ops, cloud, a):
    """The launches of fit_plane on a checked argument dict.  -> plane (B,4), counts (B,3), found (B) int32, status (B) int32, on the device."""
    pts, off = cloud.points, cloud.offsets
    # the status words (NONFINITE) come from the bounding-box pass of the cell grid; it also writes M keys nobody reads here, which costs one pass
    # over the rows, and with sort=False the cell size only scales those keys: any positive value does, 1.0 is one
    _, status, _, _, _ = ops.cloud_cell_grid(pts, off, 1, 1, 1.0, sort=False)
    key = torch.from_numpy(a["keys"]).to(pts.device)
    planes, valid = ops.cloud_plane_hypotheses(pts, off, key, a["H"], up=a["up"], cos_tilt=a["cos_tilt"])
    counts = ops.cloud_plane_score(pts, off, planes, a["tau"], valid=valid)
    plane, best, found = ops.cloud_plane_select(planes, valid, counts, min_inliers=a["min_inliers"], has_up=a["up"] is not None)
    if a["refit"]:
        plane, best = ops.cloud_plane_refit(pts, off, plane, best, found, a["tau"])
    return plane, best, found, status


def fit_plane(cloud, threshold, keys, hypotheses=1024, up=None, max_tilt=None, min_inliers=3, refit=True):
    """The dominant plane of every cloud by RANSAC: `hypotheses` planes through three rows drawn under the cloud's key (one integer per cloud, or
    one for all), each scored by its rows within `threshold`; the one with the most inliers wins (a tie: the lowest hypothesis) and is refitted
    once to its inliers by least squares.  up (with max_tilt in degrees) admits only planes whose normal lies within max_tilt of +-up and
    orients them along up; without up the normal points to the side with more rows.  -> plane (B,4) fp64 = unit normal and d (s = n . x + d),
    counts (B,3) int32 = inliers, above, below, found (B) bool -- False where the cloud has no plane with min_inliers inliers, which is a
    result, not an error.  ValueError for bad arguments before any launch."""
    o = _offsets(cloud)
    a = _check_plane(len(o) - 1, threshold, keys, hypotheses, up, max_tilt, min_inliers, refit)
    torch, ops, ctx = _ops(cloud)
    with ctx:
        plane, counts, found, status = _plane(torch, ops, cloud, a)
    _raise_status("fit_plane", status.cpu().numpy())
    return plane, counts, found.bool()


def _raise_emptied(what, before, after):
    gone = np.flatnonzero((np.asarray(after) == 0) & (np.asarray(before) > 0))
    if len(gone):
        raise _lib.EtchHipError(f"{what}: cloud {int(gone[0])}: no row is left")


def remove_plane(cloud, threshold, keys, hypotheses=1024, up=None, max_tilt=None, min_inliers=3, refit=True):
    """fit_plane, then keep_i = s_i > threshold where a plane was found: the floor and everything under it goes (and what stands closer than the
    threshold to it).  -> (Cloud of the kept rows, keep (M) bool, plane (B,4), found (B) bool).  EtchHipError naming a cloud that loses every row."""
    o = _offsets(cloud)
    B = len(o) - 1
    a = _check_plane(B, threshold, keys, hypotheses, up, max_tilt, min_inliers, refit)
    torch, ops, ctx = _ops(cloud)
    with ctx:
        plane, _, found, status = _plane(torch, ops, cloud, a)
        keep = ops.cloud_plane_keep(cloud.points, cloud.offsets, plane, found, a["tau"])
        out = _compact(ops, cloud, keep)
        host = torch.cat([status, out.offsets]).cpu().numpy()            # the one readback
    _raise_status("remove_plane", host[:B])
    _raise_emptied("remove_plane", np.diff(o), np.diff(host[B:].astype(np.int64)))
    return _trim(out, int(host[-1])), keep[:int(o[-1])].bool(), plane, found.bool()


def cluster(cloud, radius, brute=False):
    """Euclidean clusters: the connected components of the graph that links two rows of a cloud at d2 <= radius * radius.  -> labels (M) int32 =
    the lowest row of the row's component (local to its cloud), sizes (M) int32 = the rows of that component.  brute=True links by a scan of the
    whole cloud: the same bits."""
    radius = _check_positive(radius, "radius")
    o = _offsets(cloud)
    torch, ops, ctx = _ops(cloud)
    with ctx:
        label, size, status = ops.cloud_components(cloud.points, cloud.offsets, radius, brute=brute)
    _raise_status("cluster", status.cpu().numpy())
    return label[:int(o[-1])], size[:int(o[-1])]


def _check_cluster(radius, min_points=1):
    if int(min_points) != min_points or int(min_points) < 1:
        raise ValueError(f"min_points must be a positive integer, got {min_points}")
    return _check_positive(radius, "radius"), int(min_points)


def keep_clusters(cloud, radius, largest=True, min_points=1):
    """Keep the largest cluster of every cloud (a tie: the one with the lowest row), or with largest=False every cluster of at least min_points
    rows.  -> (Cloud, keep (M) bool).  EtchHipError naming a cloud that loses every row."""
    radius, min_points = _check_cluster(radius, min_points)
    o = _offsets(cloud)
    B = len(o) - 1
    torch, ops, ctx = _ops(cloud)
    with ctx:
        label, size, status = ops.cloud_components(cloud.points, cloud.offsets, radius)
        keep, _ = ops.cloud_component_keep(label, size, cloud.offsets, largest=largest, min_points=min_points)
        out = _compact(ops, cloud, keep)
        host = torch.cat([status, out.offsets]).cpu().numpy()
    _raise_status("keep_clusters", host[:B])
    _raise_emptied("keep_clusters", np.diff(o), np.diff(host[B:].astype(np.int64)))
    return _trim(out, int(host[-1])), keep[:int(o[-1])].bool()


def prepare(cloud, N, keys, voxel=None, stat=None, radius=None, center=True, floor=None, cluster=None):
    """A raw cloud -> the network's input: the statistical filter (stat = (k, ratio)), the radius filter (radius = (r, min_neighbours)), the floor
    (floor = a dict of fit_plane's arguments: threshold, keys, ...; keys defaults to `keys`), the largest cluster (cluster = (radius,
    min_points)), the voxel grid (voxel = the cell size), ops.bbox_center of what is left, and depth.pick's stratified pick of N points per cloud
    under `keys` -- with a voxel grid the pick walks the cells in spatial order.  -> points (B,N,3) fp32, centres (B,3) fp64 (None without
    center), the cleaned Cloud, which also carries .keep ((M) bool over the given rows: what the stages kept), .stages (rows per cloud after each
    stage, a dict of numpy arrays) and, with floor, .plane (B,4) fp64 and .plane_found (B) bool (both None without).  One readback for all
    stages; errors as in the single calls."""
    from . import depth, mesh_io
    o = _offsets(cloud)
    B = len(o) - 1
    if stat is not None:
        stat = _check_stat(*stat)
    if radius is not None:
        radius = _check_radius(*radius)
    if floor is not None:
        floor = dict(floor)
        floor.setdefault("keys", keys)
        floor = _check_plane(B, **floor)
    if cluster is not None:
        cluster = _check_cluster(*cluster)
    if voxel is not None:
        voxel = _check_positive(voxel, "voxel")
    mesh_io._keys(keys, B)
    if int(N) < 0:
        raise ValueError("N must not be negative")
    torch, ops, ctx = _ops(cloud)
    dev = cloud.points.device
    words, names, cur = [], [], cloud
    keep = torch.ones((cloud.points.shape[0],), dtype=torch.bool, device=dev)
    plane = found = None

    def compose(keep, k):                                            # a kept row's rank among the kept rows is its row in the compacted cloud
        if not names:
            return k.bool()
        rank = (torch.cumsum(keep.to(torch.int64), 0) - 1).clamp_(min=0)
        return keep & k.bool()[rank]

    with ctx:
        if stat is not None:
            k1, _, status = _stat(ops, cur, *stat)
            keep = k1.bool()
            cur = _compact(ops, cur, k1)
            words += [status, cur.offsets]
            names.append("statistical")
        if radius is not None:
            count, status = ops.cloud_radius_count(cur.points, cur.offsets, radius[0])
            k2 = (count >= radius[1]).to(torch.int32)
            keep = compose(keep, k2)
            cur = _compact(ops, cur, k2)
            words += [status, cur.offsets]
            names.append("radius")
        if floor is not None:                                        # strays are gone: they vote for no plane
            plane, _, found, status = _plane(torch, ops, cur, floor)
            k3 = ops.cloud_plane_keep(cur.points, cur.offsets, plane, found, floor["tau"])
            keep = compose(keep, k3)
            cur = _compact(ops, cur, k3)
            words += [status, cur.offsets]
            names.append("floor")
        if cluster is not None:                                      # the floor is gone: it no longer links the subject to what stands beside it
            label, size, status = ops.cloud_components(cur.points, cur.offsets, cluster[0])
            k4, _ = ops.cloud_component_keep(label, size, cur.offsets, largest=True, min_points=cluster[1])
            keep = compose(keep, k4)
            cur = _compact(ops, cur, k4)
            words += [status, cur.offsets]
            names.append("cluster")
        if voxel is not None:
            cur, _, status = _voxel(ops, cur, voxel)
            words += [status, cur.offsets]
            names.append("voxel")
        c = ops.bbox_center(cur.points, cur.offsets) if center else None
        p64, p32, pixel, pstatus = depth._pick(cur, N, keys, c, dev)
        host = torch.cat(words + [pstatus]).cpu().numpy()            # the one readback
    stages = {"input": np.diff(o)}
    for i, name in enumerate(names):
        part = host[i * (2 * B + 1):(i + 1) * (2 * B + 1)]
        _raise_status(f"prepare ({name})", part[:B])
        stages[name] = np.diff(part[B:].astype(np.int64))
        if name in ("floor", "cluster"):
            _raise_emptied(f"prepare ({name})", list(stages.values())[-2], stages[name])
    if host[-B:].any():
        raise _lib.EtchHipError(f"prepare: cloud {int(np.flatnonzero(host[-B:])[0])}: no point is left to pick from")
    total = int(host[-B - 1]) if names else int(o[-1])
    if names:
        if hasattr(cur, "cell"):
            cur.cell = cur.cell[:total]
        cur = _trim(cur, total)
    else:
        cur = Cloud(cloud.points[:total], cloud.index[:total], cloud.offsets, cloud.count, None)
    cur.keep, cur.stages, cur.picked = keep[:int(o[-1])], stages, pixel             # picked (B,N) int32: the index of every picked row
    cur.plane, cur.plane_found = plane, (found.bool() if found is not None else None)
    return p32, c, cur


# ---------------------------------------------------------------------------------------------------------------- registering several views
STATUS_DEGENERATE = 8
ALIGN_TOL_ANGLE, ALIGN_TOL_SHIFT = 1e-9, 1e-9                       # radians, metres: far below a scanner's noise, far above fp64 rounding


class Alignment:
    """What align() returns, per pair of clouds: R (B,3,3), t (B,3) fp64 and pair (Ms) int32 (the last matching, -1 = unmatched) on the device;
    matched (B), rms (B), steps (B), status (B) numpy -- status holds STATUS_DEGENERATE where a step had fewer than 3 pairs or pairs of rank < 2
    (the transform then stayed as it was from that step on)."""

    def __init__(self, R, t, matched, rms, steps, status, pair):
        self.R, self.t, self.matched, self.rms, self.steps, self.status, self.pair = R, t, matched, rms, steps, status, pair


def _check_pairs(source, target):
    so, to = _offsets(source), _offsets(target)
    if len(so) != len(to):
        raise ValueError(f"source and target must hold the same number of clouds, got {len(so) - 1} and {len(to) - 1}")
    return so, to


def _check_align(gate=0.2, gate_min=0.02, decay=0.9, iters=40, tol_angle=ALIGN_TOL_ANGLE, tol_shift=ALIGN_TOL_SHIFT, cell=None):
    """align's loop arguments, checked before any launch.  -> a dict: gates (the gate of every step, fp64 on the host), tol_angle, tol_shift, cell."""
    gate = _check_positive(gate, "gate")
    gate_min = _check_positive(gate_min, "gate_min")
    if gate_min > gate:
        raise ValueError(f"gate_min must not exceed gate, got {gate_min} > {gate}")
    if not 0.0 < float(decay) <= 1.0:
        raise ValueError(f"decay must lie in (0, 1], got {decay}")
    if int(iters) != iters or int(iters) < 1:
        raise ValueError(f"iters must be a positive integer, got {iters}")
    if not (float(tol_angle) >= 0.0 and float(tol_shift) >= 0.0):
        raise ValueError(f"tol_angle and tol_shift must not be negative, got {tol_angle} and {tol_shift}")
    if cell is not None:
        _check_positive(cell, "cell")
    return dict(gates=[max(gate_min, gate * float(decay) ** k) for k in range(int(iters))], tol_angle=float(tol_angle), tol_shift=float(tol_shift), cell=cell)


def _init_pose(init, B, dev):
    """init: None, (R (B,3,3), t (B,3)) or (B,4,4) poses, arrays or tensors -> R, t fp64 on the device (None, None for None)."""
    import torch
    if init is None:
        return None, None
    if isinstance(init, (tuple, list)) and len(init) == 2 and (init[0] is None) != (init[1] is None):
        raise ValueError("a transform is R and t together: one of them is missing")
    if isinstance(init, (tuple, list)) and len(init) == 2 and all(isinstance(x, torch.Tensor) and x.is_cuda for x in init):
        R, t = (x.to(device=dev, dtype=torch.float64) for x in init)         # device tensors (an Alignment's) stay there: no copy to the host, and
        if R.numel() != 9 * B or t.numel() != 3 * B:                         # so no look at their values
            raise ValueError(f"init must give a rotation and a shift for each of the {B} clouds")
        return R.reshape(B, 3, 3).contiguous(), t.reshape(B, 3).contiguous()
    if isinstance(init, (tuple, list)) and len(init) == 2:
        R, t = (np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, np.float64) for x in init)
    else:
        T = np.asarray(init.cpu() if isinstance(init, torch.Tensor) else init, np.float64).reshape(-1, 4, 4)
        R, t = T[:, :3, :3], T[:, :3, 3]
    R, t = R.reshape(-1, 3, 3), t.reshape(-1, 3)
    if R.shape != (B, 3, 3) or t.shape != (B, 3) or not (np.isfinite(R).all() and np.isfinite(t).all()):
        raise ValueError(f"init must give a finite rotation and shift for each of the {B} clouds")
    return torch.from_numpy(np.ascontiguousarray(R)).to(dev), torch.from_numpy(np.ascontiguousarray(t)).to(dev)


def nearest(source, target, gate, R=None, t=None, cell=None, brute=False):
    """For every row of source cloud b, moved by x = R_b p + t_b: the nearest row of target cloud b with d2 <= gate * gate, a tie to the lowest
    row.  -> pair (Ms) int32 = that row, local to its cloud (-1 without one), d2 (Ms) fp64 (+inf without one), on the device.  The same bits for
    any cell size and from brute=True.  EtchHipError naming the cloud where a coordinate of either side is not finite."""
    gate = _check_positive(gate, "gate")
    if cell is not None:
        _check_positive(cell, "cell")
    so, _ = _check_pairs(source, target)
    R, t = _init_pose(None if R is None and t is None else (R, t), len(so) - 1, source.points.device)
    torch, ops, ctx = _ops(source)
    with ctx:
        pair, d2, status = ops.cloud_nearest(source.points, source.offsets, target.points, target.offsets, gate, R=R, t=t, cell=cell, brute=brute)
    _raise_status("nearest", status.cpu().numpy() & STATUS_NONFINITE)
    return pair[:int(so[-1])], d2[:int(so[-1])]


def _align(torch, ops, source, target, a, R, t, brute, normals=None):
    return ops.cloud_align(source.points, source.offsets, target.points, target.offsets, a["gates"], a["tol_angle"], a["tol_shift"], R=R, t=t,
                           cell=a["cell"], brute=brute, tgt_normals=normals)


METRICS = ("point", "plane")


def _check_metric(metric, normals=None, normal_k=16):
    """The metric arguments of align and register_views, checked before any launch."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if metric == "point" and normals is not None:
        raise ValueError("normals= are the target's normals for metric='plane'; metric='point' takes none")
    return _check_normal_k(normal_k) if metric == "plane" else None


def _given_normals(normals, Mt, dev):
    """normals= of align: (Mt,3) numbers, an array or a tensor -> fp64 on the device; ValueError for any other shape."""
    import torch
    if isinstance(normals, torch.Tensor):
        if tuple(normals.shape) != (Mt, 3) or not (normals.dtype.is_floating_point or normals.dtype in (torch.int32, torch.int64)):
            raise ValueError(f"normals must be ({Mt},3) numbers, got {normals.dtype} {tuple(normals.shape)}")
        return normals.to(device=dev, dtype=torch.float64).contiguous()
    n = np.asarray(normals)
    if n.shape != (Mt, 3) or n.dtype.kind not in "fiu":
        raise ValueError(f"normals must be ({Mt},3) numbers, got {n.dtype} {n.shape}")
    return torch.from_numpy(np.array(n, np.float64, order="C")).to(dev)


def _alignment(torch, out, B, what):
    """The one readback of an align call."""
    host = torch.cat([out["matched"].double(), out["steps"].double(), out["status"].double(), out["rms"]]).cpu().numpy().reshape(4, B)
    status = host[2].astype(np.int32)
    _raise_status(what, status & STATUS_NONFINITE)
    return Alignment(out["R"], out["t"], host[0].astype(np.int32), host[3], host[1].astype(np.int32), status, out["pair"])


def align(source, target, gate=0.2, gate_min=0.02, decay=0.9, iters=40, tol_angle=ALIGN_TOL_ANGLE, tol_shift=ALIGN_TOL_SHIFT, init=None, cell=None,
          brute=False, metric="point", normals=None, normal_k=16, keys=None, viewpoint=None, global_kw=None):
    """Point-to-point ICP with a shrinking gate, every pair of clouds on its own: step k matches every moved source row to its nearest target row
    within max(gate_min, gate * decay^k), then takes the rigid step that fits the matched rows best (least squares, closed form).  A pair
    stops early once a step turns by less than tol_angle radians and moves its matched rows' centroid by less than tol_shift; the defaults end
    a pair whose matching has frozen (copies of the same rows) and are inert between two samplings of a surface, where the steps shrink by
    only ~0.86 a step and `iters` ends the loop: set tol_shift to a fraction of the expected rms there.  init: start poses
    (R, t) or (B,4,4); the method converges from about 20 degrees and 10 cm on a body, not from anywhere.  -> Alignment.  The loop runs on the
    device without a host synchronisation; brute=True gives the same bits without the grid.  ValueError for bad arguments before any launch.
    metric="plane"  takes point-to-plane steps instead: the matching is the same, the step minimises the squared distances to the
    tangent planes of the matched target rows, which lets a surface slide along itself and converges in a few steps where the point metric needs
    tens.  The target's normals are computed once per call from normal_k neighbours (normals()), or handed in as normals= (Mt,3), a file's own for
    example; their sign does not matter, a target row with the normal (0, 0, 0) matches nothing.  A step with fewer than 6 matched rows or an exactly
    singular system (an exact plane, collinear rows) is STATUS_DEGENERATE; a merely near-symmetric target is not detected and slides.
    init="global"  starts from global_align(source, target, keys, viewpoint=viewpoint, **global_kw) instead of a given pose: keys
    and viewpoint = (the source's, the target's) sensor position are then needed.  Where it finds no pose the loop starts from the identity and the
    status holds STATUS_GLOBAL_NOT_FOUND; the GlobalAlignment is the result's .start."""
    a = _check_align(gate, gate_min, decay, iters, tol_angle, tol_shift, cell)
    normal_k = _check_metric(metric, normals, normal_k)
    so, to = _check_pairs(source, target)
    B = len(so) - 1
    if normals is not None:
        normals = _given_normals(normals, target.points.shape[0], target.points.device)
    start = None
    if isinstance(init, str):
        if init != "global":
            raise ValueError(f"init must be None, poses or 'global', got {init!r}")
        if keys is None:
            raise ValueError("init='global' needs keys")
        start = global_align(source, target, keys, viewpoint=viewpoint, **(global_kw or {}))
        init = (start.R, start.t)
    elif keys is not None or viewpoint is not None or global_kw is not None:
        raise ValueError("keys, viewpoint and global_kw belong to init='global'")
    torch, ops, ctx = _ops(source)
    R, t = _init_pose(init, B, source.points.device)
    with ctx:
        if metric == "plane" and normals is None:
            normals = ops.cloud_normals(target.points, target.offsets, normal_k)[0]     # a non-finite row: the loop's own status raises below
        out = _align(torch, ops, source, target, a, R, t, brute, normals)
        res = _alignment(torch, out, B, "align")
    res.pair = res.pair[:int(so[-1])]
    if start is not None:
        res.status = res.status | np.where(start.found, 0, STATUS_GLOBAL_NOT_FOUND).astype(np.int32)
        res.start = start
    return res


def transform(cloud, R, t):
    """The cloud moved: x = R_b p + t_b for every row of cloud b (R, t: arrays, or device tensors such as an Alignment's, which are used where
    they are).  -> a Cloud with the same index, offsets and count."""
    o = _offsets(cloud)
    R, t = _init_pose((R, t), len(o) - 1, cloud.points.device)
    torch, ops, ctx = _ops(cloud)
    with ctx:
        pts = ops.cloud_transform(cloud.points, cloud.offsets, R, t)
    return Cloud(pts, cloud.index, cloud.offsets, cloud.count, None)


def _union(torch, clouds, offsets):
    """Clouds of B subjects each (host offsets given) -> one Cloud whose cloud b holds the rows of every part's cloud b, part after part; index is
    the row inside the part.  Packed on the device."""
    B = len(offsets[0]) - 1
    dev = clouds[0].points.device
    parts, index = [], []
    for b in range(B):
        for c, o in zip(clouds, offsets):
            parts.append(c.points[int(o[b]):int(o[b + 1])])
            index.append(c.index[int(o[b]):int(o[b + 1])])
    n = np.array([sum(int(o[b + 1] - o[b]) for o in offsets) for b in range(B)], np.int64)
    if n.sum() >= 2 ** 31 // 3:
        raise ValueError("the views together are too large for 32-bit offsets")
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(n)]).astype(np.int32)).to(dev)
    return Cloud(torch.cat(parts).contiguous(), torch.cat(index).contiguous(), off, torch.from_numpy(n.astype(np.int32)).to(dev), None)


def _check_views(views):
    views = list(views)
    if not views:
        raise ValueError("no view to register")
    offsets = [_offsets(v) for v in views]
    if len({len(o) for o in offsets}) != 1:
        raise ValueError(f"every view must hold the same number of clouds, got {[len(o) - 1 for o in offsets]}")
    return views, offsets


def _union_rows(torch, rows, offsets):
    """Per-row tensors of several parts (host offsets given) in the row order of _union."""
    B = len(offsets[0]) - 1
    return torch.cat([r[int(o[b]):int(o[b + 1])] for b in range(B) for r, o in zip(rows, offsets)]).contiguous()


def _global_views_prepare(torch, ops, views, a, viewpoints):
    """The descriptors of every view in its own frame, once: -> a list of (Cloud trimmed to its rows, feature, has_feature, host offsets)."""
    B = views[0].offsets.numel() - 1
    dev = views[0].points.device
    if viewpoints is None or len(viewpoints) != len(views):
        raise ValueError(f"viewpoints must hold one sensor position per view, got {0 if viewpoints is None else len(viewpoints)} for {len(views)} views")
    vp = [_viewpoint(v, B, dev) for v in viewpoints]
    if any(v is None for v in vp):
        raise ValueError("viewpoints must give a sensor position for every view")
    words, sides = [], []
    for v, w in zip(views, vp):
        n = len(words)
        sides.append(_global_side(ops, v, a, w, words) + (len(words) - n,))
    host = torch.cat(words + [s[0].offsets for s in sides]).cpu().numpy()      # one readback for all views
    at, out = 0, []
    for k, (c, f, h, n) in enumerate(sides):
        for _ in range(n):
            _raise_status(f"register_views (view {k})", host[at:at + B])
            at += B
    for c, f, h, n in sides:
        o = host[at:at + B + 1].astype(np.int64)
        at += B + 1
        total = int(o[-1])
        out.append((Cloud(c.points[:total], c.index[:total], c.offsets, c.count, None), f[:total], h[:total], o))
    return out


def register_views(views, init=None, metric="point", normal_k=16, keys=None, viewpoints=None, global_kw=None, **align_kw):
    """Views (Clouds of B subjects each) into the frame of view 0: view k is aligned to the union of the views 0 .. k - 1 as already placed.
    init: one start pose per view (None, (R, t) or (B,4,4)), or None.  metric="plane": align's point-to-plane steps, the normals computed on the
    union anew for every view.  -> a list of Alignment, one per view (view 0: the identity).
    init="global"  needs no start pose: the descriptors of every view are computed once in its own frame (global_align's
    arguments in global_kw, its keys in keys, one sensor position per view in viewpoints, each in its view's frame), view k is matched against the
    voxelised rows of the views 0 .. k - 1 as placed, with their own descriptors, and then refined against the union exactly as with a given pose.
    A view without a found pose starts from the identity, its status holds STATUS_GLOBAL_NOT_FOUND; every Alignment but the first carries .start."""
    a = _check_align(**align_kw)
    normal_k = _check_metric(metric, None, normal_k)
    views, offsets = _check_views(views)
    B = len(offsets[0]) - 1
    g = None
    if isinstance(init, str):
        if init != "global":
            raise ValueError(f"init must be None, poses or 'global', got {init!r}")
        if keys is None:
            raise ValueError("init='global' needs keys")
        g, init = _check_global(B, keys, **(global_kw or {})), None
    elif keys is not None or viewpoints is not None or global_kw is not None:
        raise ValueError("keys, viewpoints and global_kw belong to init='global'")
    if init is not None and len(init) != len(views):
        raise ValueError(f"init must hold one entry per view, got {len(init)} for {len(views)} views")
    torch, ops, ctx = _ops(views[0])
    dev = views[0].points.device
    with ctx:
        sides = _global_views_prepare(torch, ops, views, g, viewpoints) if g is not None else None
        coarse = [sides[0][0]] if g is not None else None
        eye = torch.eye(3, dtype=torch.float64, device=dev).repeat(B, 1, 1)
        out = [Alignment(eye, torch.zeros((B, 3), dtype=torch.float64, device=dev), np.diff(offsets[0]).astype(np.int32), np.zeros(B),
                         np.zeros(B, np.int32), np.zeros(B, np.int32), None)]
        placed = [views[0]]
        for k in range(1, len(views)):
            R, t = _init_pose(None if init is None else init[k], B, dev)
            start = None
            if g is not None:
                so = [s[3] for s in sides[:k]]
                seen = _union(torch, coarse, so)
                src, fs, hs, _ = sides[k]
                match = _global_match(torch, ops, src, fs, hs, seen, _union_rows(torch, [s[1] for s in sides[:k]], so),
                                      _union_rows(torch, [s[2] for s in sides[:k]], so), g["mutual"])
                start = _global_result(torch, [], B, *_global_pose(torch, ops, src, seen, match, g), f"register_views (view {k})")
                R, t = start.R, start.t
            union = _union(torch, placed, offsets[:k])
            normals = ops.cloud_normals(union.points, union.offsets, normal_k)[0] if metric == "plane" else None
            res = _alignment(torch, _align(torch, ops, views[k], union, a, R, t, False, normals), B, f"register_views (view {k})")
            res.pair = res.pair[:int(offsets[k][-1])]
            if start is not None:
                res.status = res.status | np.where(start.found, 0, STATUS_GLOBAL_NOT_FOUND).astype(np.int32)
                res.start = start
                c = sides[k][0]
                coarse.append(Cloud(ops.cloud_transform(c.points, c.offsets, res.R, res.t), c.index, c.offsets, c.count, None))
            out.append(res)
            placed.append(Cloud(ops.cloud_transform(views[k].points, views[k].offsets, res.R, res.t), views[k].index, views[k].offsets, views[k].count, None))
    return out


def fuse(views, transforms, voxel=None, return_view=False):
    """The views, each moved by its transform (an Alignment or (R, t)), concatenated into one cloud per subject; with voxel, voxel_downsample of
    that, so that a surface several views saw is present once.  -> Cloud; with return_view also view (M) int32 on the device = the view every
    output row came from -- under voxel the view of the cell's lowest row, the row Cloud.index names."""
    views, offsets = _check_views(views)
    transforms = list(transforms)
    if len(transforms) != len(views):
        raise ValueError(f"fuse needs one transform per view, got {len(transforms)} for {len(views)} views")
    if voxel is not None:
        voxel = _check_positive(voxel, "voxel")
    torch, ops, ctx = _ops(views[0])
    moved = [transform(v, *((T.R, T.t) if isinstance(T, Alignment) else T)) for v, T in zip(views, transforms)]
    with ctx:
        union = _union(torch, moved, offsets)
        ids = _view_ids(torch, offsets, union.points.device) if return_view else None
    if voxel is None:
        return (union, ids) if return_view else union
    out = voxel_downsample(union, voxel)[0]
    if not return_view:
        return out
    with ctx:
        return out, _lowest_view(torch, ids, union.offsets, out.index, out.offsets)


def _view_ids(torch, offsets, dev):
    """The view of every row of _union(views, offsets) (host offsets, one array per view): (M) int32 on dev."""
    return _union_rows(torch, [torch.full((int(o[-1]),), k, dtype=torch.int32, device=dev) for k, o in enumerate(offsets)], offsets)


def _lowest_view(torch, ids, union_offsets, index, out_offsets):
    """Under a voxel grid: ids at the cell's lowest row.  index (rows) = that row, local to its cloud of the union; both offsets on the device."""
    rows = torch.arange(index.shape[0], device=index.device)
    b = (torch.searchsorted(out_offsets.long(), rows, right=True) - 1).clamp_(0, out_offsets.numel() - 2)
    return ids[index.long() + union_offsets.long()[b]]


# ---------------------------------------------------------------------------------------------------------------- oriented clouds: inside and outside
AREA_MIN_K = 3


class OrientedCloud:
    """A cloud that knows its inside: per row pos (M,3) = the position, moment (M,3) = area x oriented unit normal and cap (M)
    = area / pi, all fp32 on the device, with offsets (B+1) int32 and max_rows = the largest cloud's rows on the host.  What surface() returns and
    etch_amd.containment takes in place of a mesh."""

    def __init__(self, pos, moment, cap, offsets, max_rows):
        self.pos, self.moment, self.cap, self.offsets, self.max_rows = pos, moment, cap, offsets, int(max_rows)


def _check_area_k(k):
    if int(k) != k or not AREA_MIN_K <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in {AREA_MIN_K} .. {MAX_K}, got {k}")
    return int(k)


def _ke(torch, o, k, dev):
    """min(k, n - 1) of every row's cloud as (M) fp64 on the device, from the host offsets."""
    n = np.diff(o)
    ke = np.repeat(np.minimum(k, n - 1), n).astype(np.float64)
    return torch.from_numpy(ke).to(dev)


def areas(cloud, k=8, cell=None, brute=False):
    """The area every row stands for: a_i = (pi d2k_i) / ke with d2k_i the squared distance to the ke-th nearest other row of its
    cloud, ke = min(k, n - 1), 3 <= k <= 32 -- the disc to the k-th neighbour holds k rows, so a row of a surface sampled at density rho gets 1 / rho,
    and half of it where two views overlap.  -> (M) fp64 on the device; 0 for a cloud of one row.  cell= and brute=True change no bit.  ValueError
    for bad arguments before any launch; EtchHipError naming the cloud that holds a non-finite coordinate."""
    k = _check_area_k(k)
    if cell is not None:
        _check_positive(cell, "cell")
    o = _offsets(cloud)
    torch, ops, ctx = _ops(cloud)
    total = int(o[-1])
    with ctx:
        d2k, status = ops.cloud_knn_kth(cloud.points, cloud.offsets, k, cell=cell, brute=brute)
        ke = _ke(torch, o, k, cloud.points.device)
        a = torch.where(ke > 0, (math.pi * d2k[:total]) / ke.clamp(min=1.0), torch.zeros_like(ke))
    _raise_status("areas", status.cpu().numpy())
    return a


def _sensors(sensors, o, dev):
    """sensors: one position (3,), one per cloud (B,3) or one per row (M,3) -> (M,3) fp64 on the device; ValueError for any other shape."""
    import torch
    B, M = len(o) - 1, int(o[-1])
    if isinstance(sensors, torch.Tensor) and sensors.is_cuda and tuple(sensors.shape) == (M, 3) and sensors.dtype.is_floating_point:
        return sensors.to(device=dev, dtype=torch.float64).contiguous()       # per-row device tensors stay there: no look at their values
    s = sensors.detach().cpu().numpy() if isinstance(sensors, torch.Tensor) else np.asarray(sensors)
    if s.dtype.kind not in "fiu" or s.shape not in ((3,), (B, 3), (M, 3)):
        raise ValueError(f"sensors must be (3,), ({B},3) or ({M},3) numbers, got {s.dtype} {s.shape}")
    s = s.astype(np.float64)
    if not np.isfinite(s).all():
        raise ValueError("sensors must be finite")
    if s.shape == (3,):
        s = np.broadcast_to(s, (B, 3))
    if s.shape != (M, 3):
        s = np.repeat(s, np.diff(o), axis=0)
    return torch.from_numpy(np.ascontiguousarray(s)).to(dev)


def orient_normals(cloud, normals, sensors):
    """Normals turned towards the sensor that saw their row: n is flipped where ((n_x w_x + n_y w_y) + n_z w_z) < 0 with w = sensor - p, section
    24's rule.  sensors: (3,), one position per cloud (B,3), or one per row (M,3) -- a fused cloud, whose rows several sensors saw.  A row without
    a normal, (0, 0, 0), stays so.  Nothing is propagated from row to row.  -> (M,3) fp64 on the device."""
    o = _offsets(cloud)
    M = int(o[-1])
    dev = cloud.points.device
    n = _given_normals(normals, M, dev)
    s = _sensors(sensors, o, dev)
    import torch
    w = s - cloud.points[:M]                                         # plain torch: runs wherever the cloud is
    dot = (n[:, 0] * w[:, 0] + n[:, 1] * w[:, 1]) + n[:, 2] * w[:, 2]
    return torch.where((dot < 0.0)[:, None], -n, n)                  # a flagged row's (0, 0, 0) has dot 0 and stays


def surface(cloud, sensors=None, normals=None, normal_k=16, area_k=8, center=None):
    """A cloud with an inside -> OrientedCloud, what etch_amd.containment and fit_surface(scan=) take in place of a mesh.
    The normals are normals(cloud, normal_k) turned towards `sensors` (orient_normals: one position, one per cloud, or one per row for a fused
    cloud), or are given, already oriented, as normals= (M,3) -- a file's own (mesh_io.read_cloud(path, return_normals=True)) for example; a row
    whose normal is (0, 0, 0) or not finite counts as flagged.  Exactly one of the two is needed, ValueError otherwise: there is NO orientation
    propagation, so a cloud with neither sensor positions nor normals is out of scope.  Each row stands for the area areas(cloud, area_k); a
    flagged row gets none and adds nothing to a winding number.  center (B,3) is subtracted from the positions in fp64 before the rounding to
    fp32: give the centre of the frame the queries are in.  ValueError for every argument out of range, before any launch; EtchHipError naming the
    cloud that holds a non-finite coordinate."""
    if (sensors is None) == (normals is None):
        raise ValueError("surface needs sensors= (the sensor positions, to orient computed normals) or normals= (already oriented), and not both")
    area_k = _check_area_k(area_k)
    if sensors is not None:
        normal_k = _check_normal_k(normal_k)
    o = _offsets(cloud)
    B, M = len(o) - 1, int(o[-1])
    dev = cloud.points.device
    import torch
    if sensors is not None:
        sensors = _sensors(sensors, o, dev)
    else:
        normals = _given_normals(normals, M, dev)
    c = None
    if center is not None:
        cc = center.detach().cpu().numpy() if isinstance(center, torch.Tensor) else np.asarray(center)
        if cc.dtype.kind not in "fiu" or cc.shape not in ((3,), (B, 3)) or not np.isfinite(cc.astype(np.float64)).all():
            raise ValueError(f"center must be (3,) or ({B},3) finite numbers, got {cc.dtype} {cc.shape}")
        c = torch.from_numpy(np.array(np.broadcast_to(cc.astype(np.float64), (B, 3)), order="C")).to(dev)
    torch, ops, ctx = _ops(cloud)
    pts = cloud.points[:M].contiguous()
    with ctx:
        if normals is None:
            n, _, flag, status = ops.cloud_normals(pts, cloud.offsets, normal_k)
            w = sensors - pts
            dot = (n[:, 0] * w[:, 0] + n[:, 1] * w[:, 1]) + n[:, 2] * w[:, 2]
            n = torch.where((dot < 0.0)[:, None], -n, n)
        else:
            n = normals
            flag = ((n == 0.0).all(1) | ~torch.isfinite(n).all(1)).to(torch.int32) * NORMAL_FLAG_AMBIGUOUS
            n = torch.where((flag != 0)[:, None], torch.zeros_like(n), n)
        d2k, status = ops.cloud_knn_kth(pts, cloud.offsets, area_k)
        pos, moment, cap = ops.cloud_surface_pack(pts, cloud.offsets, n.contiguous(), flag.contiguous(), d2k, area_k, center=c)
    _raise_status("surface", status.cpu().numpy())
    return OrientedCloud(pos, moment, cap, cloud.offsets, int(np.diff(o).max()))


# ---------------------------------------------------------------------------------------------------------------- a mesh from the winding field
MESH_KEEP = ("largest", "all")
MESH_MAX_PAD, MESH_MAX_DILATE, MESH_MAX_ROUNDS = 64, 2, 1 << 20


class Reconstruction:
    """What reconstruct() returns: meshes = one Mesh per cloud (float64 vertices, int32 faces; empty for an empty cloud), and per cloud closed (B)
    bool, clipped (B) = mixed faces that pointed out of the lattice, blocks (B) = blocks evaluated, rounds (B) = growth rounds that added blocks,
    components (B) = connected components before keep= chose, status (B) = STATUS_EMPTY or 0, all numpy."""

    def __init__(self, meshes, closed, clipped, blocks, rounds, components, status):
        self.meshes, self.closed, self.clipped, self.blocks, self.rounds, self.components, self.status = meshes, closed, clipped, blocks, rounds, components, status


def _check_int(x, lo, hi, name):
    if isinstance(x, bool) or int(x) != x or not lo <= int(x) <= hi:
        raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {x}")
    return int(x)


def reconstruct(surface, voxel, level=0.5, keep="largest", seed_dilate=0, pad_blocks=2, max_rounds=32, center=None):
    """The watertight surface of an oriented cloud: the level set |w| = level of section 26's winding number, by marching
    tetrahedra on a lattice of `voxel`-sized cells in blocks of 8 x 8 x 8.  Only the blocks the surface runs through are evaluated: the blocks
    that hold a row (dilated by seed_dilate blocks), then, round by round, the neighbours behind every block face the level set crosses, at most
    max_rounds rounds.  closed[b] says that the followed surface left neither the evaluated blocks nor the lattice (pad_blocks blocks around the
    rows): then the mesh has no boundary edge.  closed = False is a result, not an error.  keep="largest" keeps the connected component with the
    most faces (a tie: the one with the lowest vertex), keep="all" everything.  Vertices are welded by the integer key of the lattice edge they
    lie on, in ascending key order; center (B,3) or (3,) is added to them in fp64.  Bitwise reproducible; cloud b in a batch is bitwise cloud b
    alone.  ValueError for every argument out of range before any launch; EtchHipError naming the cloud whose lattice is out of range (an axis
    with more than 2^20 - 1 nodes or more than 2^24 blocks: the voxel is too small for the cloud's extent).  -> Reconstruction."""
    if not isinstance(surface, OrientedCloud):
        raise ValueError(f"surface must be an OrientedCloud (cloud.surface), got {type(surface).__name__}")
    if isinstance(voxel, bool) or not isinstance(voxel, (int, float, np.floating, np.integer)) or not (float(voxel) > 0.0 and math.isfinite(float(voxel))):
        raise ValueError(f"voxel must be positive and finite, got {voxel}")
    if isinstance(level, bool) or not isinstance(level, (int, float, np.floating, np.integer)) or not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must lie in (0, 1), got {level}")
    if keep not in MESH_KEEP:
        raise ValueError(f"keep must be one of {MESH_KEEP}, got {keep!r}")
    seed_dilate = _check_int(seed_dilate, 0, MESH_MAX_DILATE, "seed_dilate")
    pad_blocks = _check_int(pad_blocks, 0, MESH_MAX_PAD, "pad_blocks")
    max_rounds = _check_int(max_rounds, 0, MESH_MAX_ROUNDS, "max_rounds")
    import torch

    from . import ops
    from .models.fit_SMPL import Mesh
    B = int(surface.offsets.numel()) - 1
    c = np.zeros((B, 3))
    if center is not None:
        cc = center.detach().cpu().numpy() if isinstance(center, torch.Tensor) else np.asarray(center)
        if cc.dtype.kind not in "fiu" or cc.shape not in ((3,), (B, 3)) or not np.isfinite(cc.astype(np.float64)).all():
            raise ValueError(f"center must be (3,) or ({B},3) finite numbers, got {cc.dtype} {cc.shape}")
        c = np.array(np.broadcast_to(cc.astype(np.float64), (B, 3)))
    voxel, level = float(voxel), float(level)
    dev = surface.pos.device
    with torch.cuda.device(dev):
        lattice, status = ops.cloud_mesh_lattice(surface, voxel, pad_blocks)
        lat, st = lattice.cpu().numpy().astype(np.int64), status.cpu().numpy()
        if (st & STATUS_RANGE).any():
            b = int(np.flatnonzero(st & STATUS_RANGE)[0])
            raise _lib.EtchHipError(f"reconstruct: cloud {b}: the lattice has an axis with more than 2^20 - 1 nodes or more than 2^24 blocks: "
                                    "the voxel is too small for the cloud's extent")
        toff_host = np.concatenate([[0], np.cumsum((lat[:, 3:] - lat[:, :3]).prod(1))]).astype(np.int64)
        toff = torch.from_numpy(toff_host).to(dev)
        table = torch.full((int(toff_host[-1]),), ops.MESH_TABLE_INACTIVE, dtype=torch.int32, device=dev)
        ops.cloud_mesh_seed(surface, voxel, seed_dilate, lattice, status, toff, table)
        slots, fields = [], []
        clipped = torch.zeros((B,), dtype=torch.int64, device=dev)
        rounds = torch.zeros((B,), dtype=torch.int64, device=dev)
        left_open = torch.zeros((B,), dtype=torch.bool, device=dev)
        n_slots, r = 0, 0
        while True:
            new = torch.nonzero(table == ops.MESH_TABLE_MARK, as_tuple=False)[:, 0]      # ascending = (cloud, block key); the round's one readback
            if new.numel() == 0:
                break
            of = torch.bucketize(new, toff[1:], right=True)
            if r > max_rounds:                                                            # the surface goes on, the rounds are used up
                table[new] = ops.MESH_TABLE_INACTIVE
                left_open[of] = True
                break
            if r > 0:
                rounds[torch.unique(of)] += 1
            sl = torch.stack([of, new - toff[of]], 1).to(torch.int32).contiguous()
            table[new] = torch.arange(n_slots, n_slots + new.numel(), dtype=torch.int32, device=dev)
            n_slots += int(new.numel())
            fld = ops.cloud_mesh_field(surface, voxel, level, lattice, sl)
            flags = ops.cloud_mesh_grow(lattice, toff, sl, fld, table)
            clipped.index_add_(0, of, (flags == 2).sum(1))
            slots.append(sl), fields.append(fld)
            r += 1
        meshes = [Mesh(np.zeros((0, 3)) + c[b], np.zeros((0, 3), np.int32)) for b in range(B)]
        components = np.zeros(B, np.int64)
        blocks = np.zeros(B, np.int64)
        if slots:
            sl, fld = torch.cat(slots), torch.cat(fields)
            order = torch.argsort(sl[:, 0].long() * (1 << 32) + sl[:, 1].long())
            sl, fld = sl[order].contiguous(), fld[order].contiguous()
            counts, keys, fpos = ops.cloud_mesh_extract(lattice, voxel, sl, fld)
            per_cloud = torch.zeros((B,), dtype=torch.int64, device=dev).index_add_(0, sl[:, 0].long(), counts.sum(1, dtype=torch.int64))
            f_end = np.cumsum(per_cloud.cpu().numpy())
            blocks = torch.bincount(sl[:, 0].long(), minlength=B).cpu().numpy()
            for b in range(B):
                f0, f1 = int(f_end[b - 1]) if b else 0, int(f_end[b])
                if f1 == f0:
                    continue
                _, verts, faces = ops.cloud_mesh_weld(keys[f0:f1], fpos[f0:f1])
                labels = ops.mesh_components(verts.shape[0], faces)
                components[b] = int((labels == torch.arange(verts.shape[0], dtype=torch.int32, device=dev)).sum())
                if keep == "largest" and components[b] > 1:
                    per_label = torch.bincount(labels[faces[:, 0].long()].long(), minlength=verts.shape[0])
                    winner = int(torch.nonzero(per_label == per_label.max(), as_tuple=False)[0, 0])      # a tie: the lowest label
                    verts, faces = ops.mesh_keep_component(verts, faces, labels, winner)
                meshes[b] = Mesh(verts.cpu().numpy().astype(np.float64) + c[b], faces.cpu().numpy())
        clipped = clipped.cpu().numpy()
        closed = (st == 0) & ~left_open.cpu().numpy() & (clipped == 0)
    return Reconstruction(meshes, closed, clipped, blocks, rounds.cpu().numpy(), components, st)


# ---------------------------------------------------------------------------------------------------------------- global registration
MAX_GLOBAL_HYPOTHESES = 262144
STATUS_GLOBAL_NOT_FOUND = 16                                       # align(init="global"): no pose was found, the loop started from the identity


class GlobalAlignment:
    """What global_align() returns, per pair of clouds: R (B,3,3), t (B,3) fp64 on the device; found (B) bool, inliers (B) int32 and
    correspondences (B) int32 numpy.  found False (R = I, t = 0) is a result, not an error."""

    def __init__(self, R, t, found, inliers, correspondences):
        self.R, self.t, self.found, self.inliers, self.correspondences = R, t, found, inliers, correspondences


def _feature_normals(ops, cloud, k, view, normals, grid, brute):
    """The oriented normals and their flags for the descriptors, on a cell grid built before.  -> normal (M,3) fp64, flag (M) int32 on the device."""
    import torch
    if normals is not None:
        n = _given_normals(normals, cloud.points.shape[0], cloud.points.device)
        return n, ((n == 0.0).all(1) | ~torch.isfinite(n).all(1)).to(torch.int32) * NORMAL_FLAG_AMBIGUOUS      # a row without a normal has no descriptor
    out = ops.cloud_normals(cloud.points, cloud.offsets, k, viewpoint=view, brute=brute, grid=grid)
    return out[0], out[2]


def _features(ops, cloud, k, view, normals, cell=None, brute=False):
    """Normals and descriptors on ONE cell grid: the keys and the two sorts are the same for both."""
    grid = ops.cloud_cell_grid(cloud.points, cloud.offsets, 0, k, 0.0 if cell is None else float(cell), sort=not brute)
    normal, flag = _feature_normals(ops, cloud, k, view, normals, grid, brute)
    return ops.cloud_fpfh(cloud.points, cloud.offsets, normal, flag, k, brute=brute, grid=grid)


def _check_feature_source(viewpoint, normals):
    if viewpoint is None and normals is None:
        raise ValueError("features need oriented normals: give viewpoint= (the sensor position) or normals=; sign-free normals make no descriptor")
    if viewpoint is not None and normals is not None:
        raise ValueError("give viewpoint= or normals=, not both")


def features(cloud, k=32, viewpoint=None, normals=None, cell=None, brute=False, return_spfh=False):
    """FPFH descriptors: 33-bin histograms of the angles between a row's normal and those of its k nearest rows, weighted over
    the neighbourhood.  The normals come from `viewpoint` ((3,) or one sensor position per cloud) through normals(), or are given as oriented
    `normals` (M,3); neither raises ValueError.  -> feature (M,33) fp64, has_feature (M) bool on the device (and with return_spfh the pass-1
    counts spfh (M,33) int32, their number c (M) int32 and the neighbour lists (M,k) int32).  A row has no feature where its normal is flagged, it
    counted no pair or a block of its histogram is empty.  cell= and brute=True change no bit."""
    k = _check_normal_k(k)
    _check_feature_source(viewpoint, normals)
    if cell is not None:
        _check_positive(cell, "cell")
    o = _offsets(cloud)
    view = _viewpoint(viewpoint, len(o) - 1, cloud.points.device)
    torch, ops, ctx = _ops(cloud)
    with ctx:
        feature, has, spfh, count, nbr, status = _features(ops, cloud, k, view, normals, cell, brute)
    _raise_status("features", status.cpu().numpy())
    total = int(o[-1])
    res = (feature[:total], has[:total].bool())
    return res + (spfh[:total], count[:total], nbr[:total]) if return_spfh else res


def _check_global(B, keys, voxel=0.02, feature_k=32, hypotheses=65536, tau=None, edge_similarity=0.9, min_edge=0.05, min_inliers=6, mutual=False,
                  refit_steps=2):
    """global_align's arguments, checked before any launch.  -> a dict."""
    from . import mesh_io
    if voxel is not None:
        voxel = _check_positive(voxel, "voxel")
    if tau is None:
        if voxel is None:
            raise ValueError("tau=None means 1.5 * voxel: with voxel=None give tau")
        tau = 1.5 * voxel
    tau = _check_positive(tau, "tau")
    if int(hypotheses) != hypotheses or not 1 <= int(hypotheses) <= MAX_GLOBAL_HYPOTHESES:
        raise ValueError(f"hypotheses must be an integer in 1 .. {MAX_GLOBAL_HYPOTHESES}, got {hypotheses}")
    if not 0.0 < float(edge_similarity) <= 1.0:
        raise ValueError(f"edge_similarity must lie in (0, 1], got {edge_similarity}")
    if not (float(min_edge) >= 0.0 and math.isfinite(float(min_edge))):
        raise ValueError(f"min_edge must be finite and not negative, got {min_edge}")
    if int(min_inliers) != min_inliers or int(min_inliers) < 0:
        raise ValueError(f"min_inliers must be a non-negative integer, got {min_inliers}")
    if int(refit_steps) != refit_steps or int(refit_steps) < 0:
        raise ValueError(f"refit_steps must be a non-negative integer, got {refit_steps}")
    return dict(keys=mesh_io._keys(keys, B), voxel=voxel, k=_check_normal_k(feature_k), H=int(hypotheses), tau=tau, e=float(edge_similarity),
                min_edge=float(min_edge), min_inliers=int(min_inliers), mutual=bool(mutual), refit_steps=int(refit_steps))


def _global_views(viewpoint, B, dev):
    if viewpoint is None or len(viewpoint) != 2:
        raise ValueError("viewpoint must be (source's, target's) sensor positions: the descriptors need oriented normals")
    vs, vt = _viewpoint(viewpoint[0], B, dev), _viewpoint(viewpoint[1], B, dev)
    if vs is None or vt is None:
        raise ValueError("viewpoint must give a sensor position for the source and for the target")
    return vs, vt


def _global_match(torch, ops, src, fs, hs, tgt, ft, ht, mutual):
    match, _ = ops.cloud_feature_match(fs, hs, src.offsets, ft, ht, tgt.offsets)
    if mutual and match.numel() and ft.shape[0]:
        back, _ = ops.cloud_feature_match(ft, ht, tgt.offsets, fs, hs, src.offsets)
        rows = torch.arange(match.numel(), device=match.device)
        B = src.offsets.numel() - 1
        cloud = torch.bucketize(rows, src.offsets[1:].long().contiguous(), right=True).clamp_(max=B - 1)
        j = (tgt.offsets.long()[cloud] + match.long()).clamp_(0, ft.shape[0] - 1)
        agree = (match >= 0) & (back[j].long() == rows - src.offsets.long()[cloud])
        match = torch.where(agree, match, torch.full_like(match, -1))
    return match


def _global_pose(torch, ops, src, tgt, match, a):
    """Hypotheses, scores, selection and the refit for given matches.  -> R (B,3,3), t (B,3), found (B) int32, inliers (B) int32,
    correspondences (B) int32, on the device."""
    dev = src.points.device
    cs, ct, crow, coff, _ = ops.cloud_correspondences(src.points, src.offsets, tgt.points, tgt.offsets, match)
    key = torch.from_numpy(a["keys"]).to(dev)
    transforms, valid, _ = ops.cloud_global_hypotheses(cs, ct, crow, coff, key, a["H"], a["e"], a["min_edge"])
    counts = ops.cloud_global_score(cs, ct, coff, transforms, a["tau"], valid=valid)
    R, t, best, _, found = ops.cloud_global_select(transforms, valid, counts, a["min_inliers"])
    for _ in range(a["refit_steps"]):
        pair = ops.cloud_global_inliers(src.points, src.offsets, tgt.points, tgt.offsets, match, R, t, a["tau"])
        Rn, tn = ops.cloud_align_step(src.points, src.offsets, tgt.points, tgt.offsets, pair, R=R, t=t)[5:7]
        again = ops.cloud_global_score(cs, ct, coff, torch.cat([Rn.reshape(-1, 1, 9), tn.reshape(-1, 1, 3)], 2).contiguous(), a["tau"])[:, 0]
        keep = (found != 0) & (again >= best)                                   # the last pose whose count did not fall
        R, t, best = torch.where(keep[:, None, None], Rn, R), torch.where(keep[:, None], tn, t), torch.where(keep, again, best)
    return R, t, found, best, coff[1:] - coff[:-1]


def _global_side(ops, cloud, a, view, words):
    """One side of global_align: the voxel grid (where asked for) and the descriptors.  Status words go to `words` for the one readback."""
    if a["voxel"] is not None:
        cloud, _, status = _voxel(ops, cloud, a["voxel"])
        words.append(status)
    feature, has, _, _, _, status = _features(ops, cloud, a["k"], view, None)
    words.append(status)
    return cloud, feature, has


def _global_result(torch, words, B, R, t, found, best, ncorr, what):
    host = torch.cat(words + [found, best, ncorr]).cpu().numpy()                 # the one readback
    n = len(words)
    for i in range(n):
        _raise_status(what, host[i * B:(i + 1) * B])
    return GlobalAlignment(R, t, host[n * B:(n + 1) * B].astype(bool), host[(n + 1) * B:(n + 2) * B].astype(np.int32), host[(n + 2) * B:].astype(np.int32))


def global_align(source, target, keys, voxel=0.02, feature_k=32, viewpoint=None, hypotheses=65536, tau=None, edge_similarity=0.9, min_edge=0.05,
                 min_inliers=6, mutual=False, refit_steps=2):
    """A rough pose of every source cloud on its target from nothing: FPFH descriptors (features()) on voxel_downsample of both
    sides (voxel=None: the clouds as given), the nearest target descriptor of every source row (mutual=True: kept only where the reverse search
    agrees), `hypotheses` rigid poses from three correspondences drawn under the pair's key (one integer per pair, or one for all) -- a triple is
    dropped where its edges differ in length by more than edge_similarity or are shorter than min_edge --, each scored by the correspondences it
    brings within tau (None: 1.5 voxel); the best (a tie: the lowest hypothesis) is refitted refit_steps times to its inliers.  viewpoint = (the
    source's, the target's) sensor position, each (3,) or (B,3), each in its own cloud's frame: the descriptors need oriented normals.
    -> GlobalAlignment; found False where fewer than min_inliers correspondences agree.  The result is a start for align(), which converges from
    about 20 degrees and 10 cm.  ValueError for bad arguments before any launch; one readback."""
    so, _ = _check_pairs(source, target)
    B = len(so) - 1
    a = _check_global(B, keys, voxel, feature_k, hypotheses, tau, edge_similarity, min_edge, min_inliers, mutual, refit_steps)
    vs, vt = _global_views(viewpoint, B, source.points.device)
    torch, ops, ctx = _ops(source)
    with ctx:
        words = []
        src, fs, hs = _global_side(ops, source, a, vs, words)
        tgt, ft, ht = _global_side(ops, target, a, vt, words)
        match = _global_match(torch, ops, src, fs, hs, tgt, ft, ht, a["mutual"])
        R, t, found, best, ncorr = _global_pose(torch, ops, src, tgt, match, a)
        return _global_result(torch, words, B, R, t, found, best, ncorr, "global_align")


# ---------------------------------------------------------------------------------------------------------------- the command
def add_align_flags(p):
    """The flags that register further views onto --cloud_path's frame; without --more_views nothing changes."""
    p.add_argument("--more_views", type=str, nargs="+", default=None, help="further views of the same subject, registered onto the first cloud's frame "
                   "and fused with it before the cleaning stages")
    p.add_argument("--align_gate", type=float, default=0.2, help="registration: the first gate in metres")
    p.add_argument("--align_gate_min", type=float, default=0.02, help="registration: the smallest gate")
    p.add_argument("--align_decay", type=float, default=0.9, help="registration: the gate shrinks by this factor a step")
    p.add_argument("--align_iters", type=int, default=40, help="registration: steps at most")
    p.add_argument("--align_metric", type=str, default="point", choices=METRICS, help="registration: point-to-point steps, or point-to-plane steps "
                   "on normals computed from the views (a few steps instead of tens)")
    p.add_argument("--align_normal_k", type=int, default=16, help="registration with --align_metric plane: neighbours per normal (3 .. 32)")
    p.add_argument("--view_init", type=str, default=None, help="an .npz whose array `poses` (V,4,4) holds a start pose for every view of --more_views")
    p.add_argument("--fuse_voxel", type=float, default=0.0, help="fuse the registered views on a voxel grid of V metres; 0 = concatenate")
    p.add_argument("--align_global", action="store_true", help="registration without start poses: FPFH descriptors, feature matches and RANSAC find a rough "
                   "pose for every view, which the registration then refines (instead of --view_init)")
    p.add_argument("--align_global_voxel", type=float, default=0.02, help="--align_global: the voxel size the descriptors are computed on, in metres")
    p.add_argument("--align_feature_k", type=int, default=32, help="--align_global: neighbours per descriptor (3 .. 32)")
    p.add_argument("--align_hypotheses", type=int, default=65536, help=f"--align_global: RANSAC hypotheses (1 .. {MAX_GLOBAL_HYPOTHESES})")
    p.add_argument("--view_origin", type=float, nargs=3, metavar=("X", "Y", "Z"), default=(0.0, 0.0, 0.0), help="--align_global: the camera position in each "
                   "view's own frame")


def check_align_flags(p, a):
    try:
        _check_align(a.align_gate, a.align_gate_min, a.align_decay, a.align_iters)
        _check_metric(a.align_metric, None, a.align_normal_k)
    except ValueError as e:
        p.error(f"registration: {e}")
    if a.fuse_voxel < 0.0 or not math.isfinite(a.fuse_voxel):
        p.error("--fuse_voxel must be positive and finite")
    if a.more_views is None and a.view_init is not None:
        p.error("--view_init needs --more_views")
    if a.align_global:
        if a.more_views is None:
            p.error("--align_global needs --more_views")
        if a.view_init is not None:
            p.error("--view_init and --align_global exclude each other")
        try:
            _check_global(1, [0], voxel=a.align_global_voxel, feature_k=a.align_feature_k, hypotheses=a.align_hypotheses)
        except ValueError as e:
            p.error(f"--align_global: {e}")
        if not all(math.isfinite(x) for x in a.view_origin):
            p.error("--view_origin must be three finite numbers")


def register_files(first, args, return_view=False):
    """The command's registration stage: --more_views read, registered onto `first` ((n,3) numpy) and fused.  -> the fused (n,3) numpy, the report,
    and with return_view the view (n) int32 numpy of every fused row (fuse(return_view=True))."""
    from . import mesh_io
    more = [mesh_io.read_cloud(f) for f in args.more_views]
    init = None
    if args.view_init is not None:
        poses = np.asarray(np.load(args.view_init)["poses"], np.float64)
        if poses.shape != (len(more), 4, 4):
            raise ValueError(f"--view_init: poses must be ({len(more)},4,4), got {poses.shape}")
        init = [None] + [poses[k:k + 1] for k in range(len(more))]
    views = [pack([v], args.device) for v in [first] + more]
    extra = {}
    if getattr(args, "align_global", False):
        init = "global"
        extra = dict(keys=[args.seed], viewpoints=[tuple(args.view_origin)] * len(views),
                     global_kw=dict(voxel=args.align_global_voxel, feature_k=args.align_feature_k, hypotheses=args.align_hypotheses))
    res = register_views(views, init=init, gate=args.align_gate, gate_min=args.align_gate_min, decay=args.align_decay, iters=args.align_iters,
                         metric=args.align_metric, normal_k=args.align_normal_k, **extra)
    fused, view = fuse(views, res, voxel=args.fuse_voxel if args.fuse_voxel > 0.0 else None, return_view=True) if return_view else \
        (fuse(views, res, voxel=args.fuse_voxel if args.fuse_voxel > 0.0 else None), None)
    pose = np.tile(np.eye(4), (len(views), 1, 1))
    for k, r in enumerate(res):
        pose[k, :3, :3], pose[k, :3, 3] = r.R[0].cpu().numpy(), r.t[0].cpu().numpy()
    report = {"view_pose": pose, "view_matched": np.array([int(r.matched[0]) for r in res]), "view_rms": np.array([float(r.rms[0]) for r in res]),
              "view_steps": np.array([int(r.steps[0]) for r in res]), "view_status": np.array([int(r.status[0]) for r in res]), "view_metric": np.array(args.align_metric)}
    if extra:                                                        # view 0 fixes the frame: found, no inliers, the identity
        start = np.tile(np.eye(4), (len(views), 1, 1))
        for k, r in enumerate(res[1:], 1):
            start[k, :3, :3], start[k, :3, 3] = r.start.R[0].cpu().numpy(), r.start.t[0].cpu().numpy()
        report.update(view_global_found=np.array([True] + [bool(r.start.found[0]) for r in res[1:]]),
                      view_global_inliers=np.array([0] + [int(r.start.inliers[0]) for r in res[1:]]), view_global_pose=start)
    if return_view:
        return fused.points.cpu().numpy(), report, view.cpu().numpy()
    return fused.points.cpu().numpy(), report


def source_rows(clean, voxel):
    """The row of prepare()'s INPUT behind every row of its cleaned cloud, (rows) int64 on the device: the kept rows in order, and under a voxel grid
    the kept row that is its cell's lowest (Cloud.index).  One cloud."""
    import torch
    kept = torch.nonzero(clean.keep, as_tuple=False)[:, 0]
    return kept[clean.index.long()] if voxel else kept


def contain_cloud(args, clean, center, raw_normals, view, poses):
    """--surface_contain: the cleaned cloud as an OrientedCloud in the centred frame.  Several views: the normals are computed and turned towards the
    sensor of the view each row came from, R_k o + t_k with o = --view_origin.  One view: the file's own normals, row by row."""
    import torch
    src = source_rows(clean, args.voxel > 0.0)
    if view is not None:
        o = np.asarray(args.view_origin, np.float64)
        sensor = np.einsum("kij,j->ki", poses[:, :3, :3], o) + poses[:, :3, 3]
        per_row = torch.from_numpy(sensor).to(clean.points.device)[torch.from_numpy(view).to(clean.points.device).long()[src]]
        return surface(clean, sensors=per_row, normal_k=args.contain_normal_k, area_k=args.contain_area_k, center=center)
    normals = torch.from_numpy(np.ascontiguousarray(raw_normals, np.float64)).to(clean.points.device)[src]
    return surface(clean, normals=normals, area_k=args.contain_area_k, center=center)


def add_filter_flags(p):
    """The cleaning flags python -m etch_amd.cloud and python -m etch_amd.depth share; all default to off."""
    p.add_argument("--outlier_k", type=int, default=0, help="statistical outlier removal: neighbours per point (1 .. 32); 0 = off")
    p.add_argument("--outlier_ratio", type=float, default=2.0, help="statistical outlier removal: keep m_i <= mean + RATIO * std")
    p.add_argument("--outlier_radius", type=float, default=0.0, help="radius outlier removal: the radius in metres; 0 = off")
    p.add_argument("--outlier_min_neighbours", type=int, default=2, help="radius outlier removal: neighbours a point needs within the radius")


def check_filter_flags(p, a):
    if a.outlier_k and not 1 <= a.outlier_k <= MAX_K:
        p.error(f"--outlier_k must lie in 1 .. {MAX_K}")
    if not math.isfinite(a.outlier_ratio):
        p.error("--outlier_ratio must be finite")
    if a.outlier_radius < 0.0 or not math.isfinite(a.outlier_radius) or a.outlier_min_neighbours < 0:
        p.error("--outlier_radius must be positive and finite, --outlier_min_neighbours not negative")


def filter_args(a):
    """The flags as prepare()'s stat= and radius=."""
    return ((a.outlier_k, a.outlier_ratio) if a.outlier_k else None, (a.outlier_radius, a.outlier_min_neighbours) if a.outlier_radius > 0.0 else None)


def add_isolate_flags(p):
    """The flags that isolate the subject, shared like the cleaning flags; all default to off."""
    p.add_argument("--floor_threshold", type=float, default=0.0, help="remove the floor: fit a plane by RANSAC and drop what lies closer than T metres "
                   "to it or under it; 0 = off")
    p.add_argument("--floor_hypotheses", type=int, default=1024, help=f"floor: RANSAC hypotheses (1 .. {MAX_HYPOTHESES})")
    p.add_argument("--floor_up", type=float, nargs=3, metavar=("X", "Y", "Z"), default=None, help="floor: the up direction; the floor's normal points along it")
    p.add_argument("--floor_max_tilt", type=float, default=None, help="floor: with --floor_up, admit only planes within DEG degrees of horizontal")
    p.add_argument("--floor_min_inliers", type=int, default=3, help="floor: a plane with fewer inliers is no floor, and nothing is removed")
    p.add_argument("--cluster_radius", type=float, default=0.0, help="keep the largest Euclidean cluster: points closer than R metres are linked; 0 = off")
    p.add_argument("--cluster_min_points", type=int, default=1, help="cluster: the rows the largest cluster must have")


def check_isolate_flags(p, a):
    if a.floor_threshold < 0.0 or not math.isfinite(a.floor_threshold):
        p.error("--floor_threshold must be positive and finite")
    if not 1 <= a.floor_hypotheses <= MAX_HYPOTHESES:
        p.error(f"--floor_hypotheses must lie in 1 .. {MAX_HYPOTHESES}")
    if a.floor_up is not None and (not all(math.isfinite(x) for x in a.floor_up) or not any(a.floor_up)):
        p.error("--floor_up must be three finite numbers, not all zero")
    if a.floor_max_tilt is not None and (a.floor_up is None or not 0.0 <= a.floor_max_tilt <= 90.0):
        p.error("--floor_max_tilt needs --floor_up and must lie in [0, 90]")
    if a.floor_min_inliers < 0:
        p.error("--floor_min_inliers must not be negative")
    if a.cluster_radius < 0.0 or not math.isfinite(a.cluster_radius) or a.cluster_min_points < 1:
        p.error("--cluster_radius must be positive and finite, --cluster_min_points at least 1")


def isolate_args(a):
    """The flags as prepare()'s floor= and cluster=."""
    floor = dict(threshold=a.floor_threshold, hypotheses=a.floor_hypotheses, up=a.floor_up, max_tilt=a.floor_max_tilt,
                 min_inliers=a.floor_min_inliers) if a.floor_threshold > 0.0 else None
    return floor, (a.cluster_radius, a.cluster_min_points) if a.cluster_radius > 0.0 else None


def isolate_report(clean):
    """What the floor stage adds to a command's report: {} without it."""
    if clean.plane is None:
        return {}
    return {"plane": clean.plane.cpu().numpy(), "plane_found": clean.plane_found.cpu().numpy()}


def build_parser():
    from .inference_demo import add_flags, add_surface_refine_flags
    p = argparse.ArgumentParser(prog="python -m etch_amd.cloud", description="Fit SMPL to a raw point cloud", conflict_handler="resolve")
    p.add_argument("--cloud_path", type=str, required=True, help="the cloud: .ply, .obj (vertices), .npy / .npz ((M,3)), .xyz / .txt (three columns)")
    p.add_argument("--voxel", type=float, default=0.0, help="voxel-grid down-sampling before the pick: the cell size in metres; 0 = off")
    add_filter_flags(p)
    add_isolate_flags(p)
    add_align_flags(p)
    add_flags(p)
    p.add_argument("--chamfer_refine", type=str, nargs="?", const="partial", default="none", choices=["none", "both", "partial", "clutter"],
                   help="refine the body against the whole cleaned cloud after the marker fit; without a value: partial")
    add_surface_refine_flags(p)
    p.add_argument("--contain_normal_k", type=int, default=16, help="--surface_contain: neighbours per normal of the cleaned cloud (3 .. 32)")
    p.add_argument("--contain_area_k", type=int, default=8, help="--surface_contain: neighbours per area of the cleaned cloud (3 .. 32)")
    p.add_argument("--mesh_out", action="store_true", help="write the subject's surface, the level set of the cleaned cloud's winding number, as "
                   "<name>_surface.obj in the input frame; needs --more_views or a file that carries normals; uses --contain_normal_k and --contain_area_k")
    p.add_argument("--mesh_voxel", type=float, default=0.01, help="--mesh_out: the lattice's cell size in metres")
    p.add_argument("--mesh_level", type=float, default=0.5, help="--mesh_out: the level of |w| the surface is, in (0, 1)")
    p.add_argument("--mesh_keep", type=str, default="largest", choices=list(MESH_KEEP), help="--mesh_out: the largest connected component, or all")
    return p


def parse_args(argv=None):
    p = build_parser()
    a = p.parse_args(argv)
    check_filter_flags(p, a)
    check_isolate_flags(p, a)
    check_align_flags(p, a)
    if a.voxel < 0.0 or not math.isfinite(a.voxel):
        p.error("--voxel must be positive and finite")
    if a.num_point < 1:
        p.error("--num_point must be at least 1")
    from .inference_demo import surface_contain_settings, surface_refine_settings
    surface_refine_settings(a, p)
    if a.mesh_voxel <= 0.0 or not math.isfinite(a.mesh_voxel):
        p.error("--mesh_voxel must be positive and finite")
    if not 0.0 < a.mesh_level < 1.0:
        p.error("--mesh_level must lie in (0, 1)")
    if surface_contain_settings(a, p) is not None or a.mesh_out:
        for k in (a.contain_normal_k, a.contain_area_k):
            if not AREA_MIN_K <= k <= MAX_K:
                p.error(f"--contain_normal_k and --contain_area_k must lie in {AREA_MIN_K} .. {MAX_K}")
    return a


def main(argv=None):
    from . import inference_demo as demo
    from . import mesh_io
    from .models.fit_SMPL import Mesh
    args = parse_args(argv)
    raw, raw_normals = mesh_io.read_cloud(args.cloud_path, return_normals=True)     # a malformed file raises before the model is loaded
    contain = getattr(args, "surface_contain", False)
    for flag, on in (("--surface_contain", contain), ("--mesh_out", args.mesh_out)):
        if on and not args.more_views and raw_normals is None:
            build_parser().error(f"{flag}: a single view is half a shell and has no inside; give --more_views, or a file that carries normals")
    model = demo.prepare_common(args)
    export = Mesh.export
    if getattr(args, "ingest", "host") == "device":
        export = mesh_io.write_obj
    stat, radius = filter_args(args)
    floor, cluster = isolate_args(args)
    views, view = {}, None
    if args.more_views:                                               # the views enter as one cloud, ahead of every cleaning stage
        if contain or args.mesh_out:
            raw, views, view = register_files(raw, args, return_view=True)
        else:
            raw, views = register_files(raw, args)
    p32, c, clean = prepare(pack([raw], args.device), args.num_point, [args.seed], voxel=args.voxel if args.voxel > 0.0 else None, stat=stat, radius=radius,
                            floor=floor, cluster=cluster)
    points, center, cleaned = p32[0].cpu().numpy(), c[0].cpu().numpy(), clean.points.cpu().numpy()
    name = os.path.splitext(os.path.basename(args.cloud_path))[0]
    stages = {f"rows_{k}": v for k, v in clean.stages.items()}
    report = dict(keep=clean.keep.cpu().numpy(), center=center, points=points, removed=np.int64(len(raw) - int(clean.keep.sum())),
                  rows_output=np.array([len(cleaned)]), **stages, **isolate_report(clean), **views)
    if args.mesh_out:                                                 # the subject's own surface, next to the body's
        rec = reconstruct(contain_cloud(args, clean, center, raw_normals, view, views.get("view_pose")), args.mesh_voxel, level=args.mesh_level,
                          keep=args.mesh_keep, center=center)
        export(rec.meshes[0], os.path.join(args.output_folder, f"{name}_surface.obj"))
        report.update(mesh_closed=rec.closed[0], mesh_blocks=rec.blocks[0], mesh_rounds=rec.rounds[0], mesh_components=rec.components[0],
                      mesh_vertices=np.int64(len(rec.meshes[0].vertices)), mesh_faces=np.int64(len(rec.meshes[0].faces)))
    if getattr(args, "surface_refine", False):                        # the fit comes first: the report holds the containment figures
        scan = contain_cloud(args, clean, center, raw_normals, view, views.get("view_pose")) if contain else Mesh(cleaned - center, np.zeros((0, 3), np.int64))
        found = {}
        demo._refine_and_save(args, model, points, scan, center, name, export, report=found)
        for when in ("before", "after"):
            report.update({f"contain_{when}_{k}": np.float64(v) for k, v in found.get("contain_" + when, {}).items()})
        np.savez(os.path.join(args.output_folder, f"{name}_cloud.npz"), **report)
        print(f"Predicted SMPL mesh, smpl info and the cleaning report saved under {args.output_folder}")
        return
    np.savez(os.path.join(args.output_folder, f"{name}_cloud.npz"), **report)
    if args.chamfer_refine != "none":
        demo._refine_and_save(args, model, points, Mesh(cleaned - center, np.zeros((0, 3), np.int64)), center, name, export)
    else:
        pred, info = demo.predict_smpl(args, model, points, args.gender)
        final = pred.copy()
        final.vertices = pred.vertices + center
        export(final, os.path.join(args.output_folder, f"{name}_pred_smpl.obj"))
        np.savez(os.path.join(args.output_folder, f"{name}_output_smpl_info.npz"), body_pose=info[0][0, :21, :], hand_pose=info[0][0, 21:23, :],
                 betas=info[1][0], global_orient=info[2][0], transl=info[3][0], joints=info[4][0])
    print(f"Predicted SMPL mesh, smpl info and the cleaning report saved under {args.output_folder}")


if __name__ == "__main__":
    main()
