"""Native scan ingestion: the OBJ reader and writer of libetch_hip.so (csrc/obj_io.h, host C++) and the device surface
sampler (csrc/mesh_sample.hip).  Opt-in counterparts of inference_demo.load_obj, Mesh.export, preprocess_scan and sample_points_from_mesh:

    read_obj(path) -> Mesh           the arrays load_obj returns, bit for bit, with every face index checked
    read_objs(paths) -> [Mesh]       the same on a thread pool (ctypes releases the GIL during the parse)
    write_obj(mesh, path)            the bytes Mesh.export writes
    sample_surface(meshes, N, keys)  N area-weighted points on each mesh of a ragged batch, one call, on the device
    read_ply(path) -> PlyData        PLY 1.0 (ascii, binary little / big endian): vertices, fanned faces, normals and colours when present
    write_ply(points_or_mesh, path)  binary (default) or ascii; a float64 round trip is exact
    read_cloud(path) -> (M,3)        the points of a .ply, .obj, .npy, .npz, .xyz or .txt file

The readers and the writers are host code and need no GPU; the sampler has no CPU path."""
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


# ---------------------------------------------------------------------------------------------------------------- PLY and raw clouds (host code)
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4",
              "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
_PLY_MAX_COUNT = 2 ** 31 - 1


class PlyData:
    """What read_ply returns: vertices (V,3) float64, faces (F,3) int64 (fanned polygons; (0,3) where the file has none), normals (V,3) float64
    or None, colors (V,3 or 4) in the file's type or None."""

    def __init__(self, vertices, faces, normals=None, colors=None):
        self.vertices, self.faces, self.normals, self.colors = vertices, faces, normals, colors


def _ply_type(name, path):
    if name not in _PLY_TYPES:
        raise ValueError(f"{path}: unknown type `{name}` in the header")
    return _PLY_TYPES[name]


def _ply_header(data, path):
    """-> format, [(element name, count, [(property name, type) or (property name, count type, item type)])], offset of the body."""
    if not data.startswith(b"ply"):
        raise ValueError(f"{path}: not a PLY file (no `ply` magic)")
    end = data.find(b"end_header")
    nl = data.find(b"\n", end) if end >= 0 else -1
    if end < 0 or nl < 0:
        raise ValueError(f"{path}: the header has no end_header line")
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            if len(tok) != 3 or tok[1] not in ("ascii", "binary_little_endian", "binary_big_endian") or tok[2] != "1.0":
                raise ValueError(f"{path}: unsupported format line `{line.strip()}`")
            fmt = tok[1]
        elif tok[0] == "element":
            try:
                count = int(tok[2])
            except (IndexError, ValueError):
                raise ValueError(f"{path}: element line `{line.strip()}`: the count does not fit") from None
            if not 0 <= count <= _PLY_MAX_COUNT:
                raise ValueError(f"{path}: element {tok[1]}: the count {count} does not fit")
            elements.append((tok[1], count, []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: a property line in front of the first element")
            if len(tok) == 5 and tok[1] == "list":
                ct, it = _ply_type(tok[2], path), _ply_type(tok[3], path)
                if ct[0] == "f":
                    raise ValueError(f"{path}: list property {tok[4]}: the count type must be an integer type")
                elements[-1][2].append((tok[4], ct, it))
            elif len(tok) == 3:
                elements[-1][2].append((tok[2], _ply_type(tok[1], path)))
            else:
                raise ValueError(f"{path}: malformed property line `{line.strip()}`")
        else:
            raise ValueError(f"{path}: unknown header line `{line.strip()}`")
    if fmt is None:
        raise ValueError(f"{path}: the header has no format line")
    return fmt, elements, nl + 1


class _PlyBinary:
    """Reads elements off a binary body, in file order."""

    def __init__(self, data, pos, endian, path):
        self.data, self.pos, self.e, self.path = data, pos, endian, path

    def _need(self, nbytes, name):
        if self.pos + nbytes > len(self.data):
            raise ValueError(f"{self.path}: truncated body: element {name} needs {nbytes} more bytes, {len(self.data) - self.pos} are left")

    def scalars(self, name, count, props):
        dt = np.dtype([(f"f{i}", self.e + t) for i, (_, t) in enumerate(props)])
        self._need(count * dt.itemsize, name)
        rows = np.frombuffer(self.data, dt, count, self.pos)
        self.pos += count * dt.itemsize
        return {p[0]: rows[f"f{i}"] for i, p in enumerate(props)}

    def lists(self, name, count, props):
        """The general walk: -> {list property name: [array per row]}; scalar properties between the lists are skipped."""
        out = {p[0]: [] for p in props if len(p) == 3}
        if count and len(props) == 1:                # the usual face element: try rows of one length first
            pname, ct, it = props[0]
            self._need(np.dtype(ct).itemsize, name)
            c = int(np.frombuffer(self.data, self.e + ct, 1, self.pos)[0])
            dt = np.dtype([("n", self.e + ct), ("i", self.e + it, (max(c, 0),))])
            if c > 0 and self.pos + count * dt.itemsize <= len(self.data):
                rows = np.frombuffer(self.data, dt, count, self.pos)
                if (rows["n"] == c).all():
                    self.pos += count * dt.itemsize
                    out[pname] = rows["i"]
                    return out
        for _ in range(count):
            for p in props:
                if len(p) == 2:
                    self._need(np.dtype(p[1]).itemsize, name)
                    self.pos += np.dtype(p[1]).itemsize
                    continue
                pname, ct, it = p
                self._need(np.dtype(ct).itemsize, name)
                c = int(np.frombuffer(self.data, self.e + ct, 1, self.pos)[0])
                self.pos += np.dtype(ct).itemsize
                if c < 0:
                    raise ValueError(f"{self.path}: element {name}: a list count of {c} does not fit")
                self._need(c * np.dtype(it).itemsize, name)
                out[pname].append(np.frombuffer(self.data, self.e + it, c, self.pos))
                self.pos += c * np.dtype(it).itemsize
        return out


class _PlyAscii:
    def __init__(self, data, pos, path):
        self.tok, self.pos, self.path = data[pos:].split(), 0, path

    def _take(self, n, name):
        if self.pos + n > len(self.tok):
            raise ValueError(f"{self.path}: truncated body: element {name} needs {n} more values, {len(self.tok) - self.pos} are left")
        out = self.tok[self.pos:self.pos + n]
        self.pos += n
        return out

    def _convert(self, tokens, t, name):
        try:
            a = np.array(tokens, dtype="S").astype("U")
            return a.astype("f8").astype(t) if t[0] == "f" else np.array([int(x) for x in a], dtype="i8" if t != "u8" else "u8").astype(t)
        except (ValueError, OverflowError):
            raise ValueError(f"{self.path}: element {name}: a value is no number of its type") from None

    def scalars(self, name, count, props):
        flat = np.array(self._take(count * len(props), name), dtype=object).reshape(count, len(props))
        return {p[0]: self._convert(list(flat[:, i]), p[1], name) for i, p in enumerate(props)}

    def lists(self, name, count, props):
        out = {p[0]: [] for p in props if len(p) == 3}
        for _ in range(count):
            for p in props:
                if len(p) == 2:
                    self._take(1, name)
                    continue
                c = int(self._convert(self._take(1, name), "i8", name)[0])
                if c < 0:
                    raise ValueError(f"{self.path}: element {name}: a list count of {c} does not fit")
                out[p[0]].append(self._convert(self._take(c, name), p[2], name))
        return out


def _fan(rows, nv, path):
    """Index lists -> (F,3) int64 triangles, polygons fanned (i0, ik, ik+1) and shorter rows dropped as read_obj does; every index checked."""
    if isinstance(rows, np.ndarray):
        polys = rows.astype(np.int64)
        tris = np.stack([np.repeat(polys[:, :1], polys.shape[1] - 2, 1), polys[:, 1:-1], polys[:, 2:]], 2).reshape(-1, 3) if polys.shape[1] >= 3 \
            else np.zeros((0, 3), np.int64)
    else:
        out = []
        for r in rows:
            r = r.astype(np.int64)
            if len(r) >= 3:
                out.append(np.stack([np.full(len(r) - 2, r[0]), r[1:-1], r[2:]], 1))
        tris = np.concatenate(out) if out else np.zeros((0, 3), np.int64)
    if tris.size and (tris.min() < 0 or tris.max() >= nv):
        bad = tris[(tris < 0) | (tris >= nv)][0]
        raise ValueError(f"{path}: a face index {int(bad)} is out of range [0, {nv})")
    return np.ascontiguousarray(tris)


def parse_ply(data, path="<buffer>"):
    data = bytes(data)
    fmt, elements, pos = _ply_header(data, path)
    rd = _PlyAscii(data, pos, path) if fmt == "ascii" else _PlyBinary(data, pos, "<" if fmt == "binary_little_endian" else ">", path)
    vert, face_rows = None, None
    for name, count, props in elements:
        if any(len(p) == 3 for p in props):
            got = rd.lists(name, count, props)
            if name == "face":
                key = next((k for k in ("vertex_indices", "vertex_index") if k in got), None)
                if key is None:
                    raise ValueError(f"{path}: element face has no vertex_indices list")
                it = next(p[2] for p in props if p[0] == key)
                if it[0] == "f":
                    raise ValueError(f"{path}: element face: vertex indices must be of an integer type")
                face_rows = got[key]
        else:
            got = rd.scalars(name, count, props) if props else {}
        if name == "vertex":
            vert = got
    if vert is None:
        raise ValueError(f"{path}: no element vertex")
    for a in "xyz":
        if a not in vert:
            raise ValueError(f"{path}: element vertex has no property {a} (missing {a})")
    pick = lambda names: np.stack([np.asarray(vert[n]) for n in names], 1) if all(n in vert for n in names) else None
    v = np.ascontiguousarray(pick("xyz").astype(np.float64))
    normals = pick(("nx", "ny", "nz"))
    colors = pick(("red", "green", "blue", "alpha")) if "alpha" in vert else pick(("red", "green", "blue"))
    faces = _fan(face_rows, len(v), path) if face_rows is not None else np.zeros((0, 3), np.int64)
    return PlyData(v, faces, None if normals is None else normals.astype(np.float64), colors)


def read_ply(path):
    """A PLY 1.0 file (ascii, binary_little_endian, binary_big_endian) -> PlyData.  Element vertex: scalar properties in any order and of any
    PLY type; x y z are required and widen to float64 exactly, nx ny nz and red green blue [alpha] are returned when present, everything else
    is skipped.  Element face (optional): a list property vertex_indices or vertex_index of any integer types, polygons fanned as read_obj
    fans them.  Other elements are skipped, lists included.  ValueError naming the file and the defect on a malformed file."""
    with open(path, "rb") as fh:
        return parse_ply(fh.read(), str(path))


def format_ply(points_or_mesh, binary=True, normals=None):
    v = getattr(points_or_mesh, "vertices", points_or_mesh)
    f = getattr(points_or_mesh, "faces", None)
    v = np.asarray(v)
    if v.ndim != 2 or v.shape[1] != 3 or v.dtype.kind not in "fiu":
        raise ValueError(f"write_ply: points must be (M,3) numbers, got {v.dtype} {v.shape}")
    t = "float" if v.dtype == np.float32 else "double"
    v = np.ascontiguousarray(v, np.float32 if t == "float" else np.float64)
    f = np.zeros((0, 3), np.int64) if f is None else np.asarray(f)
    if f.ndim != 2 or f.shape[1] != 3 or (len(f) and (f.min() < 0 or f.max() >= len(v))):
        raise ValueError("write_ply: faces must be (F,3) indices into the vertices")
    if normals is not None:                              # one row per vertex, in the type of the points: x y z nx ny nz
        nrm = np.asarray(normals)
        if nrm.shape != v.shape or nrm.dtype.kind not in "fiu":
            raise ValueError(f"write_ply: normals must be {v.shape} numbers, got {nrm.dtype} {nrm.shape}")
        v = np.ascontiguousarray(np.concatenate([v, nrm.astype(v.dtype)], 1))
    head = [b"ply", b"format binary_little_endian 1.0" if binary else b"format ascii 1.0", b"element vertex %d" % len(v)]
    head += [b"property %s %s" % (t.encode(), a) for a in (b"x", b"y", b"z", b"nx", b"ny", b"nz")[:v.shape[1]]]
    if len(f):
        head += [b"element face %d" % len(f), b"property list uchar int vertex_indices"]
    head = b"\n".join(head + [b"end_header"]) + b"\n"
    if binary:
        body = v.astype("<" + v.dtype.str[1:]).tobytes()
        if len(f):
            rows = np.empty(len(f), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
            rows["n"], rows["i"] = 3, f
            body += rows.tobytes()
    else:
        body = "".join(" ".join(repr(float(a)) for a in row) + "\n" for row in v.astype(np.float64)).encode()
        body += "".join(f"3 {int(a)} {int(b)} {int(c)}\n" for a, b, c in f).encode()
    return head + body


def write_ply(points_or_mesh, path, binary=True, normals=None):
    """Points (M,3) or a mesh (vertices, faces) as PLY: float32 points stay `float`, everything else is written as `double`, so a float64
    round trip is exact in both forms (the ascii form writes the shortest text that reads back to the same double).  normals (M,3), one per
    point or per vertex of the mesh, are written as nx ny nz in the type of the points; without them the file is what it always was."""
    data = format_ply(points_or_mesh, binary, normals)
    with open(path, "wb") as fh:
        fh.write(data)


def read_cloud(path, return_normals=False):
    """The points of a file as (M,3) float64: .ply, .obj (its vertices), .npy / .npz (an (M,3) array; a .npz holds one array, or one named
    `points`) and .xyz / .txt (three columns, further columns ignored).  return_normals: -> points, normals, the nx ny nz of a .ply as (M,3)
    float64, None for a file that has none (every other kind)."""
    points, normals = _read_cloud(path)
    return (points, normals) if return_normals else points


def _read_cloud(path):
    ext = os.path.splitext(str(path))[1].lower()
    normals = None
    if ext == ".ply":
        ply = read_ply(path)
        p, normals = ply.vertices, ply.normals
    elif ext == ".obj":
        p = read_obj(path).vertices
    elif ext == ".npy":
        p = np.load(path)
    elif ext == ".npz":
        with np.load(path) as z:
            names = list(z.keys())
            if "points" not in names and len(names) != 1:
                raise ValueError(f"{path}: holds {names}; name the cloud `points`")
            p = z["points" if "points" in names else names[0]]
    elif ext in (".xyz", ".txt"):
        try:
            p = np.loadtxt(path, dtype=np.float64, ndmin=2, comments="#")
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None
        if p.ndim == 2 and p.shape[1] >= 3:
            p = p[:, :3]
    else:
        raise ValueError(f"{path}: a cloud is a .ply, .obj, .npy, .npz, .xyz or .txt file")
    p = np.asarray(p)
    if p.ndim != 2 or p.shape[1] != 3 or p.dtype.kind not in "fiu":
        raise ValueError(f"{path}: a cloud is an (M,3) array of numbers, got {p.dtype} {p.shape}")
    return np.ascontiguousarray(p, np.float64), None if normals is None else np.ascontiguousarray(normals, np.float64)


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
