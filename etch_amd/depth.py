"""Single-view scans: what one depth camera sees of a scan, as points the pipeline takes.

    Camera(fx, fy, cx, cy, width, height, R, t)      a pinhole camera, world to camera p_c = R x + t, x right, y down, z forward (OpenCV)
    Camera.look_at / Camera.orbit                    cameras aimed at a target / circling a centre (y-up data)
    render(meshes, cameras)                          depth, face and barycentric maps of a ragged batch (csrc/depth_render.hip)
    unproject(depth, cameras)                        the valid pixels of depth maps (rendered or a caller's) as a packed world-space cloud
    pick(cloud, N, keys)                             N points per view, stratified over the view's pixels in row-major order
    partial_view_points(meshes, cameras, N, keys)    render, unproject, centre on the visible cloud's bounding box, pick
    ViewSpec                                         the random training views of datasets.GTDataset(view=...)

    python -m etch_amd.depth --depth_path D.npy --intrinsics FX FY CX CY [...]      fit a real depth frame
    python -m etch_amd.depth --scan_path S.obj --view_azimuth DEG [...]             fit a virtual view of a mesh
    ... --outlier_k K --outlier_ratio R / --outlier_radius r --outlier_min_neighbours m   drop flying pixels first (etch_amd.cloud, section 19)
    ... --floor_threshold T [--floor_up X Y Z --floor_max_tilt DEG] / --cluster_radius R  drop the floor, keep the largest cluster (section 22)

The kernels are bit-defined; there is no CPU path."""
import argparse
import collections
import dataclasses
import math
import os

import numpy as np

from . import _lib

RenderResult = collections.namedtuple("RenderResult", "depth face bary dropped large")
PartialViews = collections.namedtuple("PartialViews", "points centers cloud dropped points64 pixel")


class Camera:
    """A pinhole camera of a width x height image.  World to camera: p_c = R x + t; pixel (r, c) has its centre at (c + 0.5, r + 0.5) and a point
    projects to u = fx x_c / z_c + cx, v = fy y_c / z_c + cy."""

    def __init__(self, fx, fy, cx, cy, width, height, R=None, t=None):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.width, self.height = int(width), int(height)
        self.R = np.eye(3) if R is None else np.array(R, np.float64).reshape(3, 3)
        self.t = np.zeros(3) if t is None else np.array(t, np.float64).reshape(3)
        if self.width < 1 or self.height < 1:
            raise ValueError(f"a camera needs an image of at least 1 x 1, got {self.height} x {self.width}")
        if not (np.isfinite([self.fx, self.fy, self.cx, self.cy]).all() and self.fx != 0.0 and self.fy != 0.0):
            raise ValueError("fx, fy, cx, cy must be finite and the focal lengths non-zero")
        if not (np.isfinite(self.R).all() and np.isfinite(self.t).all()):
            raise ValueError("R and t must be finite")

    @classmethod
    def look_at(cls, eye, target, up=(0.0, 1.0, 0.0), fx=1.0, fy=None, cx=0.0, cy=0.0, width=1, height=1):
        eye, target, up = (np.asarray(x, np.float64).reshape(3) for x in (eye, target, up))
        forward = target - eye
        n = np.linalg.norm(forward)
        if not n > 0.0:
            raise ValueError("look_at: eye and target coincide")
        forward = forward / n
        right = np.cross(forward, up)
        n = np.linalg.norm(right)
        if not n > 1e-12:
            raise ValueError("look_at: up is parallel to the viewing direction")
        right = right / n
        down = np.cross(forward, right)
        R = np.stack([right, down, forward])
        return cls(fx, fx if fy is None else fy, cx, cy, width, height, R, -R @ eye)

    @classmethod
    def orbit(cls, center, distance, azimuth, elevation=0.0, fov_deg=45.0, height=256, width=256):
        """A camera `distance` from `center` at `azimuth` / `elevation` (radians; y is up, azimuth 0 looks from +z), vertical field of view fov_deg."""
        center = np.asarray(center, np.float64).reshape(3)
        eye = center + float(distance) * np.array([math.sin(azimuth) * math.cos(elevation), math.sin(elevation), math.cos(azimuth) * math.cos(elevation)])
        f = (height / 2.0) / math.tan(math.radians(fov_deg) / 2.0)
        return cls.look_at(eye, center, fx=f, fy=f, cx=width / 2.0, cy=height / 2.0, width=width, height=height)

    @property
    def eye(self):
        return -self.R.T @ self.t

    def row(self):
        """The 16 doubles the kernels read: fx, fy, cx, cy, R row-major, t."""
        return np.concatenate([[self.fx, self.fy, self.cx, self.cy], self.R.reshape(9), self.t])

    def project(self, points):
        pc = np.asarray(points, np.float64) @ self.R.T + self.t
        return np.stack([self.fx * pc[:, 0] / pc[:, 2] + self.cx, self.fy * pc[:, 1] / pc[:, 2] + self.cy], 1), pc[:, 2]


def _camera_rows(cameras):
    cameras = [cameras] if isinstance(cameras, Camera) else list(cameras)
    if not cameras:
        raise ValueError("no camera")
    H, W = cameras[0].height, cameras[0].width
    for k, c in enumerate(cameras):
        if (c.height, c.width) != (H, W):
            raise ValueError(f"camera {k}: all views of one call share H and W, got {c.height} x {c.width} against {H} x {W}")
    return cameras, np.stack([c.row() for c in cameras]), H, W


def _view_mesh(view_mesh, NV, B):
    if view_mesh is None:
        if B == NV:
            return np.arange(NV, dtype=np.int32)
        if B == 1:
            return np.zeros(NV, np.int32)
        raise ValueError(f"{NV} cameras for {B} meshes: say which mesh each view looks at (view_mesh)")
    vm = np.asarray(view_mesh)
    if vm.shape != (NV,) or vm.dtype.kind not in "iu" or (NV and (vm.min() < 0 or vm.max() >= B)):
        raise ValueError(f"view_mesh must be {NV} integers in [0, {B})")
    return vm.astype(np.int32)


def _raise_status(what, status):
    if status.any():
        k = int(np.flatnonzero(status)[0])
        s = int(status[k])
        why = ("a vertex (or its projection) is not finite" if s & 1 else "it names no mesh with vertices" if s & 2 else "no pixel of the view is valid")
        raise _lib.EtchHipError(f"{what}: view {k}: {why}")


def _render(meshes, cameras, view_mesh, bary, near, device):
    import torch

    from . import mesh_io, ops
    meshes = list(meshes)
    cameras, rows, H, W = _camera_rows(cameras)
    v, f, voff, foff = mesh_io.pack_meshes(meshes)
    vm = _view_mesh(view_mesh, len(cameras), len(meshes))
    if not (float(near) > 0.0 and math.isfinite(float(near))):
        raise ValueError(f"near must be positive and finite, got {near}")
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(a).to(dev)
    B = len(meshes)
    ints = up(np.concatenate([voff, foff, vm]))                  # one copy per array
    with torch.cuda.device(dev):
        out = ops.render_depth(up(v), up(f), ints[:B + 1], ints[B + 1:2 * B + 2], ints[2 * B + 2:], up(rows), H, W, int(np.diff(foff).max()), near=near,
                               want_bary=bary)
    return out, rows, dev


def render(meshes, cameras, view_mesh=None, bary=False, near=0.05, device="cuda"):
    """Depth maps of a ragged batch of meshes.  cameras: Camera objects that share H and W; view_mesh: the mesh each looks at (default: mesh k for
    camera k, or the one mesh for all).  -> RenderResult(depth (NV,H,W) fp64 with +inf where nothing is hit, face (NV,H,W) int32 local to the
    mesh with -1, bary (NV,H,W,3) perspective-corrected or None, dropped (NV) int32 = faces dropped whole at the near plane, large (NV) int32 =
    faces the large-face launch rasterised), device tensors.  ValueError on bad input before any launch, EtchHipError naming the view where a
    vertex is not finite."""
    (depth, face, b, dropped, status, large), _, _ = _render(meshes, cameras, view_mesh, bary, near, device)
    _raise_status("render", status.cpu().numpy())
    return RenderResult(depth, face, b, dropped, large)


class Cloud:
    """The valid pixels of NV depth maps, view after view in row-major order: points (M,3) fp64 in world space, index (M) int32 = r W + c, offsets
    (NV+1) int32, count (NV) int32, depth (NV,H,W) fp64 = the maps they came from -- device tensors; view k owns rows offsets[k] .. offsets[k+1]."""

    def __init__(self, points, index, offsets, count, depth):
        self.points, self.index, self.offsets, self.count, self.depth = points, index, offsets, count, depth

    def view(self, k):
        o = self.offsets.cpu().numpy()
        return self.points[o[k]:o[k + 1]], self.index[o[k]:o[k + 1]]


def _unproject(depth, rows, near, far, dev):
    import torch

    from . import ops
    with torch.cuda.device(dev):
        count, offsets, index, points = ops.depth_compact(depth, torch.from_numpy(rows).to(dev), near=near, far=far)
    return Cloud(points, index, offsets, count, depth)


def unproject(depth, cameras, near=0.05, far=math.inf, device="cuda"):
    """The packed cloud of depth maps (NV,H,W) -- rendered, or a caller's frames as a tensor or an array (any real dtype; zero, negative,
    non-finite and out-of-range pixels are background: a pixel is valid where near < z < far).  -> Cloud, trimmed to its valid rows."""
    import torch
    cameras, rows, H, W = _camera_rows(cameras)
    if not (float(near) >= 0.0 and float(far) > float(near)):
        raise ValueError(f"needs 0 <= near < far, got {near} and {far}")
    if not isinstance(depth, torch.Tensor):
        depth = torch.from_numpy(np.ascontiguousarray(np.asarray(depth), dtype=np.float64))
    if depth.dim() == 2:
        depth = depth[None]
    if tuple(depth.shape) != (len(cameras), H, W):
        raise ValueError(f"depth must be ({len(cameras)},{H},{W}), got {tuple(depth.shape)}")
    dev = depth.device if depth.is_cuda else torch.device(device)
    depth = depth.to(dev, torch.float64).contiguous()
    cloud = _unproject(depth, rows, near, far, dev)
    total = int(cloud.offsets[-1])
    cloud.points, cloud.index = cloud.points[:total], cloud.index[:total]
    return cloud


def _pick(cloud, N, keys, center, dev):
    import torch

    from . import mesh_io, ops
    NV = cloud.offsets.numel() - 1
    if int(N) < 0:
        raise ValueError("N must not be negative")
    key = torch.from_numpy(mesh_io._keys(keys, NV)).to(dev)
    with torch.cuda.device(dev):
        return ops.depth_pick(cloud.offsets, cloud.index, cloud.points, key, int(N), center=center)


def pick(cloud, N, keys, center=None):
    """N points of each view of a Cloud, stratified in row-major order: sample j owns the view's rows [a_j, a_j + w), a_j = floor(j n / N),
    w = floor((j + 1) n / N) - a_j, and takes row a_j + floor(u_j w) (row a_j where n < N leaves the stratum empty), u_j the Philox uniform of
    sample j under the view's key (one integer per view, or one for all).  With n >= N no pixel is picked twice.  center (NV,3) fp64 device
    tensor: subtracted.  -> points (NV,N,3) fp32, the same in fp64, pixel (NV,N) int32.  EtchHipError naming the view where a view has no
    valid pixel."""
    p64, p32, pixel, status = _pick(cloud, N, keys, center, cloud.points.device)
    _raise_status("pick", status.cpu().numpy())
    return p32, p64, pixel


def partial_view_points(meshes, cameras, N, keys, view_mesh=None, center=True, near=0.05, device="cuda"):
    """What each camera sees of its mesh, as N points: render, unproject, pick.  center=True subtracts the bounding-box mid-point of each view's
    VISIBLE cloud (what inference on a real frame does).  -> PartialViews(points (NV,N,3) fp32, centers (NV,3) fp64 or None, cloud (the packed
    visible points, uncentred), dropped (NV) int32, points64, pixel (NV,N) int32), device tensors.  ValueError on bad input before any launch;
    EtchHipError naming the view for an empty view or a non-finite vertex, after the one status readback."""
    import torch

    from . import ops
    (depth, _, _, dropped, rstatus, _), rows, dev = _render(meshes, cameras, view_mesh, False, near, device)
    NV = len(rows)
    from . import mesh_io
    mesh_io._keys(keys, NV)                                      # bad keys raise before the remaining launches
    cloud = _unproject(depth, rows, near, math.inf, dev)
    with torch.cuda.device(dev):
        c = ops.bbox_center(cloud.points, cloud.offsets) if center else None
    p64, p32, pixel, pstatus = _pick(cloud, N, keys, c, dev)
    host = torch.cat([rstatus, pstatus, cloud.offsets]).cpu().numpy()        # the one readback: it also orders the caller behind the kernels
    _raise_status("partial_view_points", host[:NV])
    _raise_status("partial_view_points", host[NV:2 * NV])
    total = int(host[-1])
    cloud.points, cloud.index = cloud.points[:total], cloud.index[:total]
    return PartialViews(p32, c, cloud, dropped, p64, pixel)


# ---------------------------------------------------------------------------------------------------------------- random training views
@dataclasses.dataclass(frozen=True)
class ViewSpec:
    """The single-view augmentation of datasets.GTDataset: with `probability` an item's points are what one camera sees of the scan, the
    camera orbiting the scan's bounding-box centre at `distance` metres, a uniform azimuth and an elevation uniform in elevation_range (degrees),
    with a vertical field of view fov_deg and an image of size = (H, W)."""
    probability: float = 1.0
    elevation_range: tuple = (-10.0, 30.0)
    distance: float = 2.5
    fov_deg: float = 45.0
    size: tuple = (256, 256)

    def __post_init__(self):
        if not 0.0 <= float(self.probability) <= 1.0:
            raise ValueError(f"probability must lie in [0, 1], got {self.probability}")
        lo, hi = (float(x) for x in self.elevation_range)
        if not -90.0 < lo <= hi < 90.0:
            raise ValueError(f"elevation_range must satisfy -90 < lo <= hi < 90 degrees, got {self.elevation_range}")
        if not float(self.distance) > 0.0 or not 0.0 < float(self.fov_deg) < 180.0:
            raise ValueError("distance must be positive and fov_deg inside (0, 180)")
        if len(self.size) != 2 or min(int(s) for s in self.size) < 1:
            raise ValueError(f"size must be (H, W), got {self.size}")

    def draw(self, seed, epoch, index):
        """-> (taken, azimuth, elevation in radians, the 64-bit key of the pick): a pure function of (seed, epoch, index), so an item's view does
        not depend on how the items are batched, on the number of GPUs or on a resume."""
        rng = np.random.default_rng([int(seed), 200, int(epoch), int(index)])
        taken = bool(rng.random() < float(self.probability))
        azimuth = float(rng.uniform(0.0, 2.0 * math.pi))
        lo, hi = (math.radians(float(x)) for x in self.elevation_range)
        elevation = float(rng.uniform(lo, hi)) if hi > lo else lo
        key = int(rng.integers(0, 2 ** 63))
        return taken, azimuth, elevation, key

    def camera(self, seed, epoch, index, center):
        """The camera of item `index` in `epoch` around `center`, or None where the item keeps its full scan."""
        taken, az, el, _ = self.draw(seed, epoch, index)
        if not taken:
            return None
        return Camera.orbit(center, self.distance, az, el, self.fov_deg, int(self.size[0]), int(self.size[1]))


def bbox_mid(vertices):
    v = np.asarray(vertices, np.float64)
    return (v.min(0) + v.max(0)) / 2.0


# ---------------------------------------------------------------------------------------------------------------- the command
def load_depth(path, scale=1.0):
    """An H x W depth frame from a .npy, or a .npz with one array (or one named `depth`) -> float64 metres = stored value * scale.  Integer
    frames (uint16 millimetres with scale 0.001) are converted exactly before the multiplication."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path)
    elif ext == ".npz":
        with np.load(path) as z:
            names = list(z.keys())
            if "depth" in names:
                a = z["depth"]
            elif len(names) == 1:
                a = z[names[0]]
            else:
                raise ValueError(f"{path}: holds {names}; name the frame `depth`")
    else:
        raise ValueError(f"{path}: a depth frame is a .npy or .npz file")
    if a.ndim != 2 or a.dtype.kind not in "fiu" or not a.size:
        raise ValueError(f"{path}: a depth frame is a non-empty H x W array of numbers, got {a.dtype} {a.shape}")
    if not (math.isfinite(float(scale)) and float(scale) > 0.0):
        raise ValueError(f"--depth_scale must be positive and finite, got {scale}")
    return a.astype(np.float64) * float(scale)


def load_extrinsics(path):
    """World to camera [R | t] from a .npy of shape (3,4) or (4,4) -> R (3,3), t (3)."""
    E = np.asarray(np.load(path), np.float64)
    if E.shape not in ((3, 4), (4, 4)) or not np.isfinite(E).all():
        raise ValueError(f"{path}: extrinsics are a finite (3,4) or (4,4) world-to-camera matrix, got {E.shape}")
    return E[:3, :3].copy(), E[:3, 3].copy()


def build_parser():
    from .inference_demo import add_flags
    p = argparse.ArgumentParser(prog="python -m etch_amd.depth", description="Fit SMPL to one depth view: a real frame or a virtual view of a mesh",
                                conflict_handler="resolve")
    p.add_argument("--depth_path", type=str, default=None, help="a real frame: H x W depth in a .npy / .npz; zero, non-finite and out-of-range pixels are background")
    p.add_argument("--intrinsics", type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"), default=None)
    p.add_argument("--depth_scale", type=float, default=1.0, help="metres per stored unit (0.001 for uint16 millimetres)")
    p.add_argument("--extrinsics", type=str, default=None, help=".npy with the world-to-camera [R | t], (3,4) or (4,4); default: the camera frame")
    p.add_argument("--depth_range", type=float, nargs=2, metavar=("NEAR", "FAR"), default=None, help="metres; default 0 .. inf")
    p.add_argument("--scan_path", type=str, default=None, help="a virtual view: the mesh to look at")
    p.add_argument("--view_azimuth", type=float, default=None, help="degrees around the y axis, 0 looks from +z")
    p.add_argument("--view_elevation", type=float, default=0.0, help="degrees")
    p.add_argument("--view_distance", type=float, default=2.5, help="metres from the scan's bounding-box centre")
    p.add_argument("--view_fov", type=float, default=45.0, help="vertical field of view in degrees")
    p.add_argument("--view_size", type=int, nargs=2, metavar=("H", "W"), default=(512, 512))
    add_flags(p)
    from .cloud import add_filter_flags
    add_filter_flags(p)                                          # flying pixels: clean the back-projected cloud before the pick (section 19)
    from .cloud import add_isolate_flags
    add_isolate_flags(p)                                         # the floor and what stands beside the subject (section 22)
    # the same flag with a default mode: a single view is a partial scan, so a bare --chamfer_refine is the one-sided scan -> body refinement
    p.add_argument("--chamfer_refine", type=str, nargs="?", const="partial", default="none", choices=["none", "both", "partial", "clutter"],
                   help="refine the body against the whole visible cloud after the marker fit; without a value: partial")
    return p


def parse_args(argv=None):
    p = build_parser()
    a = p.parse_args(argv)
    if (a.depth_path is None) == (a.scan_path is None):
        p.error("give exactly one of --depth_path (a real frame) and --scan_path (a virtual view)")
    if a.depth_path is not None:
        if a.intrinsics is None:
            p.error("--depth_path needs --intrinsics FX FY CX CY")
        if a.view_azimuth is not None:
            p.error("--view_azimuth belongs to --scan_path")
        if not (a.intrinsics[0] > 0 and a.intrinsics[1] > 0 and all(math.isfinite(x) for x in a.intrinsics)):
            p.error("--intrinsics: FX and FY must be positive, all four finite")
        if not (a.depth_scale > 0 and math.isfinite(a.depth_scale)):
            p.error("--depth_scale must be positive and finite")
        if a.depth_range is not None and not 0.0 <= a.depth_range[0] < a.depth_range[1]:
            p.error("--depth_range needs 0 <= NEAR < FAR")
    else:
        if a.view_azimuth is None:
            p.error("--scan_path needs --view_azimuth DEG")
        if a.intrinsics is not None or a.extrinsics is not None or a.depth_range is not None or a.depth_scale != 1.0:
            p.error("--intrinsics, --extrinsics, --depth_scale and --depth_range belong to --depth_path")
        if not -90.0 < a.view_elevation < 90.0 or not a.view_distance > 0.0 or not 0.0 < a.view_fov < 180.0 or min(a.view_size) < 1:
            p.error("--view_elevation must lie inside (-90, 90), --view_distance be positive, --view_fov inside (0, 180), --view_size at least 1 1")
    if a.num_point < 1:
        p.error("--num_point must be at least 1")
    from .cloud import check_filter_flags
    check_filter_flags(p, a)
    from .cloud import check_isolate_flags
    check_isolate_flags(p, a)
    return a


def view_points(args, device, with_report=False):
    """The frame or the virtual view of `args` -> points (N,3) float32 numpy centred on the visible cloud, the centre, the visible cloud (M,3)
    float64 numpy (uncentred), the depth map (H,W) float64 numpy, the Camera, picked pixels (N), name; with_report=True
    appends what the floor and cluster stages report ({} without them)."""
    import torch

    from . import cloud as C
    from . import mesh_io, ops
    stat, radius = C.filter_args(args) if hasattr(args, "outlier_k") else (None, None)
    floor, cluster = C.isolate_args(args) if hasattr(args, "floor_threshold") else (None, None)
    filtered = stat is not None or radius is not None or floor is not None or cluster is not None
    report = {}
    if args.depth_path is not None:
        frame = load_depth(args.depth_path, args.depth_scale)
        R, t = load_extrinsics(args.extrinsics) if args.extrinsics else (None, None)
        cam = Camera(*args.intrinsics, frame.shape[1], frame.shape[0], R, t)
        near, far = args.depth_range if args.depth_range is not None else (0.0, math.inf)
        depth = torch.from_numpy(frame[None]).to(device)
        cloud = _unproject(depth, cam.row()[None], near, far, device)
        if filtered:
            # the outlier filters run on the back-projected cloud; its index (the pixel) travels through the compaction
            pts, c, clean = C.prepare(cloud, args.num_point, [args.seed], stat=stat, radius=radius, floor=floor, cluster=cluster)
            vis, pixel, report = clean.points, clean.picked, _isolate_report(C, clean)
        else:
            with torch.cuda.device(device):
                c = ops.bbox_center(cloud.points, cloud.offsets)
            p64, p32, pixel, status = _pick(cloud, args.num_point, [args.seed], c, device)
            host = torch.cat([status, cloud.offsets]).cpu().numpy()
            if host[0]:
                raise _lib.EtchHipError(f"{args.depth_path}: no pixel of the frame is valid (check --depth_scale and --depth_range)")
            pts, vis = p32, cloud.points[:int(host[-1])]
        name = os.path.splitext(os.path.basename(args.depth_path))[0]
    else:
        mesh = mesh_io.read_obj(args.scan_path)
        cam = Camera.orbit(bbox_mid(mesh.vertices), args.view_distance, math.radians(args.view_azimuth), math.radians(args.view_elevation), args.view_fov,
                           int(args.view_size[0]), int(args.view_size[1]))
        if filtered:
            (depth, _, _, _, rstatus, _), rows, dev = _render([mesh], [cam], None, False, 0.05, device)
            _raise_status("render", rstatus.cpu().numpy())
            pts, c, clean = C.prepare(_unproject(depth, rows, 0.05, math.inf, dev), args.num_point, [args.seed], stat=stat, radius=radius, floor=floor,
                                      cluster=cluster)
            vis, pixel, report = clean.points, clean.picked, _isolate_report(C, clean)
        else:
            pv = partial_view_points([mesh], [cam], args.num_point, [args.seed], center=True, device=device)
            pts, c, vis, depth, pixel = pv.points, pv.centers, pv.cloud.points, pv.cloud.depth, pv.pixel
        name = os.path.splitext(os.path.basename(args.scan_path))[0]
    out = (pts[0].cpu().numpy(), c[0].cpu().numpy(), vis.cpu().numpy(), depth[0].cpu().numpy(), cam, pixel[0].cpu().numpy(), name)
    return out + (report,) if with_report else out


def _isolate_report(C, clean):
    """What the floor and cluster stages add to <name>_view.npz: the plane and the rows after each of the two stages; {} without them."""
    rows = {f"rows_{k}": v for k, v in clean.stages.items() if k in ("floor", "cluster")}
    return {**C.isolate_report(clean), **rows}


def main(argv=None):
    import torch

    from . import inference_demo as demo
    from .models.fit_SMPL import Mesh
    args = parse_args(argv)
    model = demo.prepare_common(args)
    export = Mesh.export
    if getattr(args, "ingest", "host") == "device":
        from .mesh_io import write_obj as export
    points, center, visible, depth, cam, pixel, name, report = view_points(args, args.device, with_report=True)
    np.savez(os.path.join(args.output_folder, f"{name}_view.npz"), depth=depth, points=points, pixel=pixel, center=center, camera=cam.row(),
             size=np.array([cam.height, cam.width]), **report)
    if args.chamfer_refine != "none":
        # the refinement's target is the whole visible cloud, centred like the points
        demo._refine_and_save(args, model, points, Mesh(visible - center, np.zeros((0, 3), np.int64)), center, name, export)
    else:
        pred, info = demo.predict_smpl(args, model, points, args.gender)
        final = pred.copy()
        final.vertices = pred.vertices + center
        export(final, os.path.join(args.output_folder, f"{name}_pred_smpl.obj"))
        np.savez(os.path.join(args.output_folder, f"{name}_output_smpl_info.npz"), body_pose=info[0][0, :21, :], hand_pose=info[0][0, 21:23, :],
                 betas=info[1][0], global_orient=info[2][0], transl=info[3][0], joints=info[4][0])
    print(f"Predicted SMPL mesh, smpl info and the view saved under {args.output_folder}")


if __name__ == "__main__":
    main()
