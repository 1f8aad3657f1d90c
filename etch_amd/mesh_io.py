"""Native scan ingestion: the OBJ reader and writer of libetch_hip.so (csrc/obj_io.h, host C++) and the device surface
sampler (csrc/mesh_sample.hip).  Opt-in counterparts of inference_demo.load_obj, Mesh.export, preprocess_scan and sample_points_from_mesh:

    read_obj(path) -> Mesh           the arrays load_obj returns, bit for bit, with every face index checked
    read_objs(paths) -> [Mesh]       the same on a thread pool (ctypes releases the GIL during the parse)
    write_obj(mesh, path)            the bytes Mesh.export writes
    sample_surface(meshes, N, keys)  N area-weighted points on each mesh of a ragged batch, one call, on the device

The reader and the writer are host code and need no GPU; the sampler has no CPU path."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .models.fit_SMPL import Mesh

MAX_WORKERS = 16                  # never sized from os.cpu_count(): a shared host reports far more CPUs than a job may use

_OBJ_ERRORS = {-3: "a 'v' line needs three numbers", -4: "a face token is no integer that fits int64", -5: "a face index is outside [1, number of vertices]",
               -6: "the text changed between the count and the parse"}


def parse_obj(data, name="<buffer>"):
    """OBJ text (bytes) -> Mesh(vertices (V,3) float64, faces (F,3) int64); ValueError naming `name` and the line on a malformed text."""
    data = bytes(data)
    nv, nf, line = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_longlong(0)
    _lib.call("etch_obj_count", data, len(data), ctypes.byref(nv), ctypes.byref(nf))
    v = np.empty((nv.value, 3), np.float64)
    f = np.empty((nf.value, 3), np.int64)
    try:
        _lib.call("etch_obj_parse", data, len(data), nv, nf, v.ctypes.data, f.ctypes.data, ctypes.byref(line))
    except _lib.EtchHipError as e:
        if e.status in _OBJ_ERRORS:
            raise ValueError(f"{name}, line {line.value}: {_OBJ_ERRORS[e.status]}") from None
        raise
    return Mesh(v, f)


def read_obj(path):
    with open(path, "rb") as fh:
        return parse_obj(fh.read(), name=str(path))


def read_objs(paths, workers=None):
    """[read_obj(p) for p in paths], in order, on at most min(16, len(paths)) threads."""
    paths = list(paths)
    n = min(MAX_WORKERS, len(paths), workers if workers else MAX_WORKERS)
    if n <= 1:
        return [read_obj(p) for p in paths]
    with ThreadPoolExecutor(max_workers=n) as ex:
        return list(ex.map(read_obj, paths))


def format_obj(mesh):
    """The bytes Mesh.export writes for `mesh`."""
    v = np.ascontiguousarray(mesh.vertices, np.float64)
    f = np.ascontiguousarray(mesh.faces, np.int64)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"a mesh is vertices (V,3) and faces (F,3), got {v.shape} and {f.shape}")
    cap = 16 + 3 * 24 * len(v) + 3 * 21 * len(f)        # enough below 1e13; the call reports the size it needs otherwise
    for attempt in range(2):
        out = ctypes.create_string_buffer(cap)
        written = ctypes.c_longlong(0)
        try:
            _lib.call("etch_obj_format", v.ctypes.data, len(v), f.ctypes.data, len(f), out, cap, ctypes.byref(written))
            break
        except _lib.EtchHipError as e:
            if e.status != -7 or attempt:
                raise
            cap = written.value
    return out.raw[:written.value]


def write_obj(mesh, path):
    data = format_obj(mesh)
    with open(path, "wb") as fh:
        fh.write(data)


def pack_meshes(meshes):
    """The ragged batch as the sampler takes it -> verts (sum V,3) float64, faces (sum F,3) int32 local to their scan, vert_offsets,
    face_offsets (B+1) int32.  Raises ValueError on an empty mesh or a face index outside its scan: the kernels read vertices through them."""
    vs, fs = [], []
    if not len(meshes):
        raise ValueError("no mesh to sample")
    for k, m in enumerate(meshes):
        v, f = np.asarray(m.vertices, np.float64), np.asarray(m.faces)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or not len(v) or not len(f):
            raise ValueError(f"mesh {k}: needs vertices (V,3) and faces (F,3), both non-empty; got {v.shape} and {f.shape}")
        if f.dtype.kind not in "iu":
            raise ValueError(f"mesh {k}: faces must be integers, got {f.dtype}")
        lo, hi = int(f.min()), int(f.max())
        if lo < 0 or hi >= len(v):
            raise ValueError(f"mesh {k}: face indices must lie in [0, {len(v)}), got [{lo}, {hi}]")
        vs.append(v)
        fs.append(f.astype(np.int32))
    voff = np.concatenate([[0], np.cumsum([len(v) for v in vs])])
    foff = np.concatenate([[0], np.cumsum([len(f) for f in fs])])
    if voff[-1] >= 2 ** 31 // 3 or foff[-1] >= 2 ** 31 // 3:
        raise ValueError("the batch is too large for 32-bit offsets: sample it in parts")
    return np.concatenate(vs), np.concatenate(fs), voff.astype(np.int32), foff.astype(np.int32)


def _keys(keys, B):
    k = np.asarray(keys, dtype=object).reshape(-1)
    if len(k) == 1 and B != 1:
        k = np.repeat(k, B)
    if len(k) != B or any(int(x) < 0 or int(x) >= 2 ** 64 for x in k):
        raise ValueError(f"keys must be {B} integers in [0, 2^64) (or one for all)")
    return np.array([int(x) for x in k], np.uint64).view(np.int64)


def sample_surface(meshes, num_points, keys, center=True, device="cuda", return_fp64=False):
    """num_points area-weighted surface samples on each mesh, on the device in one call.  keys: one integer per mesh (or one for all), the
    Philox key of its samples; a mesh's points depend on its key, num_points and the mesh only.  center=True subtracts each mesh's bounding-box
    mid-point first (preprocess_scan).  -> points (B,N,3) float32, faces (B,N) int32, centres (B,3) float64 (None without center) [, points in
    float64] as device tensors.  Raises ValueError on a bad mesh (before any launch), EtchHipError where a mesh has no area or a non-finite vertex."""
    import torch

    from . import ops
    meshes = list(meshes)
    v, f, voff, foff = pack_meshes(meshes)
    B = len(meshes)
    key = _keys(keys, B)
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(a).to(dev)
    offs = up(np.concatenate([voff, foff]))                    # one copy per array
    dv, df, dk = up(v), up(f), up(key)
    voff_d, foff_d = offs[:B + 1], offs[B + 1:]
    with torch.cuda.device(dev):
        c = ops.bbox_center(dv, voff_d) if center else None
        p32, p64, face, status = ops.sample_surface(dv, df, voff_d, foff_d, dk, num_points, int(foff[-1]), int(np.diff(foff).max()) if B else 0,
                                                    center=c, want_fp64=return_fp64)
        st = status.cpu().numpy()                              # the one readback: it also orders the caller behind the kernels
    if st.any():
        k = int(np.flatnonzero(st)[0])
        what = "a vertex is not finite" if st[k] & 2 else "the total area is zero or not finite"
        raise _lib.EtchHipError(f"sample_surface: mesh {k}: {what}")
    return (p32, face, c, p64) if return_fp64 else (p32, face, c)
