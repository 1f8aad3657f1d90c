"""Build libetch_hip.so (HIP kernels + C ABI) for gfx950 with hipcc.  Cross-compiles without a GPU.

    python -m etch_amd.build [--force]

Per-file flags: the index kernels are built with -ffp-contract=off ("bit-defined fp32" distances).
The library is written in-tree (etch_amd/lib/) so it travels to the GPU box with the snapshot.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
OBJDIR = os.path.join(LIBDIR, "obj")
LIB = os.path.join(LIBDIR, "libetch_hip.so")
ARCH = "gfx950"
BASE = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-I", CSRC,
        "-I", os.path.join(os.path.dirname(HERE), "include")]
EXTRA = {"index_ops.hip": ["-ffp-contract=off"], "chamfer_fit.hip": ["-ffp-contract=off"], "raycast.hip": ["-ffp-contract=off"],
         "geodesic.hip": ["-ffp-contract=off"], "mesh_sample.hip": ["-ffp-contract=off"], "register.hip": ["-ffp-contract=off"],
         "depth_render.hip": ["-ffp-contract=off"], "surface_fit.hip": ["-ffp-contract=off"], "containment.hip": ["-ffp-contract=off"],
         "cloud_filter.hip": ["-ffp-contract=off"], "cloud_isolate.hip": ["-ffp-contract=off"],
         "cloud_align.hip": ["-ffp-contract=off"], "cloud_normals.hip": ["-ffp-contract=off"],
         "cloud_global.hip": ["-ffp-contract=off"], "cloud_winding.hip": ["-ffp-contract=off"],
         "cloud_mesh.hip": ["-ffp-contract=off"]}


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    """libetch_hip.so: every source of csrc/ compiled into lib/obj (only what is stale, unless `force`) and linked."""
    os.makedirs(OBJDIR, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "etch_hip.h"))
    cc = hipcc()
    jobs, objs = [], []
    for src in sources():
        obj = os.path.join(OBJDIR, src.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [os.path.join(CSRC, src)] + headers + [os.path.abspath(__file__)]):
            jobs.append([cc] + BASE + EXTRA.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        if verbose and r.stderr.strip():
            print(r.stderr)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([cc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
