"""Emit tests/golden/selfcheck_dump.npz: a dump in the format etch_amd.selfcheck reads for its four index sections,
with the answers of the oracle's C restatement of the reference's CUDA index kernels (oracle/discrete_ops.c) in place of a CUDA box's.  It
pins the selfcheck path end to end without a CUDA box; a real dump (ETCH_SELFCHECK_DUMP) replaces it.

    python -m oracle.gen_selfcheck_fixture
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ops as O  # noqa: E402


def scan(seed, n):
    return (np.random.default_rng(seed).standard_normal((n, 3)) * np.array([0.14, 0.31, 0.085])).astype(np.float32)


def main():
    fps_xyz = np.ascontiguousarray(np.stack([scan(7000 + b, 3000).T for b in range(2)]))
    fps_m = 750
    bq_xyz = np.ascontiguousarray(np.stack([scan(7100 + b, 2000).T for b in range(2)]))
    bq_new_xyz = np.ascontiguousarray(bq_xyz[:, :, :500])
    bq_radius, bq_nsample = 0.08, 32
    segs = [2500, 1200]
    pfps_xyz = np.concatenate([scan(7200 + i, n) for i, n in enumerate(segs)])
    pfps_offset = np.cumsum(segs).astype(np.int32)
    pfps_new_offset = np.cumsum([n // 4 for n in segs]).astype(np.int32)
    knn_xyz, knn_offset = pfps_xyz, pfps_offset
    qsegs = [600, 300]
    knn_new_xyz = np.concatenate([scan(7300 + i, n) for i, n in enumerate(qsegs)])
    knn_new_offset = np.cumsum(qsegs).astype(np.int32)
    knn_nsample = 16
    knn_idx, knn_d2 = O.knnquery(knn_nsample, knn_xyz, knn_new_xyz, knn_offset, knn_new_offset)
    out = dict(fps_xyz=fps_xyz, fps_m=np.int32(fps_m), fps_idx=O.furthest_point_sampling(fps_xyz, fps_m),
               bq_new_xyz=bq_new_xyz, bq_xyz=bq_xyz, bq_radius=np.float32(bq_radius), bq_nsample=np.int32(bq_nsample),
               bq_idx=O.ball_query(bq_new_xyz, bq_xyz, bq_radius, bq_nsample),
               pfps_xyz=pfps_xyz, pfps_offset=pfps_offset, pfps_new_offset=pfps_new_offset, pfps_idx=O.furthestsampling(pfps_xyz, pfps_offset, pfps_new_offset),
               knn_xyz=knn_xyz, knn_new_xyz=knn_new_xyz, knn_offset=knn_offset, knn_new_offset=knn_new_offset, knn_nsample=np.int32(knn_nsample),
               knn_idx=knn_idx, knn_dist=np.sqrt(knn_d2).astype(np.float32))
    path = os.path.join(ROOT, "tests", "golden", "selfcheck_dump.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
