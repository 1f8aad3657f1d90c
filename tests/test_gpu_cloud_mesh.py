"""A mesh from the winding field on the GPU.  csrc/cloud_mesh.hip against tests/_cloud_mesh_oracle.py: the field by bits against
the oracle and against ops.cloud_winding_number at every row count where the sweep takes another path; the lattice, the seeds and the growth by
integers on hand-made cases; the extraction by integers and bits on random fields; cloud.reconstruct end to end by integers and bits; the
components on a hand-made mesh and on the fixture body; the command.  Clouds of at most 6 721 rows."""
import os
import types

import numpy as np
import pytest
import torch

import _cloud_mesh_oracle as MO
import _cloud_winding_oracle as WO
import _global_oracle as GO
import _train_data

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 0.5
MO_KEEP = ("all", "largest")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _same_or_nan(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return bool(((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def _oriented(clouds):
    """[(pos, moment, cap) f32] -> cloud.OrientedCloud on the device."""
    from etch_amd import cloud
    off = np.concatenate([[0], np.cumsum([len(c[0]) for c in clouds])]).astype(np.int32)
    cat = lambda i, shape: np.concatenate([c[i].reshape(shape) for c in clouds]).astype(np.float32)      # noqa: E731
    return cloud.OrientedCloud(_dev(cat(0, (-1, 3))), _dev(cat(1, (-1, 3))), _dev(cat(2, (-1,))), _dev(off), int(np.diff(off).max()))


def _i32(a):
    return _dev(np.asarray(a, np.int32))


def _toff(n):
    return _dev(np.concatenate([[0], np.cumsum(np.asarray(n, np.int64).reshape(-1, 3).prod(1))]).astype(np.int64))


# ---- the field ------------------------------------------------------------------------------------------------------------------------------------
FIELD_H, FIELD_LO, FIELD_N = 0.02, -4, 8
FIELD_ROWS = (0, 1, 1023, 1024, 1025, 2049)


@pytest.fixture(scope="module")
def field_case():
    """Clouds of 0, 1, 1 023, 1 024, 1 025 and 2 049 rows in one ragged batch: prefixes of one 2 049-row sphere (every row keeps its area), the
    one-row cloud's row moved exactly onto a node of the block it is evaluated in.  One lattice [-4, 4)^3 of 16 cm blocks for every cloud."""
    full = MO.sphere(2049, R, 8)
    clouds = [tuple(a[:n].copy() for a in full) for n in FIELD_ROWS]
    on_node = MO.node_position(8 * (FIELD_LO + np.array([2, 2, 2])) + np.array([3, 4, 5]), FIELD_H)
    clouds[1][0][0] = on_node
    flat = lambda b: (b[0] * FIELD_N + b[1]) * FIELD_N + b[2]      # noqa: E731
    blocks = [(5, (0, 0, 0)), (5, (3, 3, 6)), (5, (4, 3, 6)), (1, (2, 2, 2)), (0, (1, 1, 1)), (2, (6, 3, 3)), (3, (3, 6, 3)), (4, (3, 3, 1))]
    lo = np.full(3, FIELD_LO, np.int64)
    want = [MO.block_field(clouds[b], FIELD_H, lo, blk, 0.5).reshape(-1) for b, blk in blocks]
    lattice = _i32(np.tile([FIELD_LO] * 3 + [FIELD_LO + FIELD_N] * 3, (len(clouds), 1)))
    slots = np.array([[b, flat(blk)] for b, blk in blocks], np.int32)
    return clouds, _oriented(clouds), lattice, blocks, slots, want


@pytest.mark.parametrize("pick", [[0], [1, 2], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5, 6, 7]], ids=["1", "2", "5", "8"])
def test_the_field_is_the_oracles_by_bits(field_case, pick):
    from etch_amd import ops
    clouds, oc, lattice, blocks, slots, want = field_case
    got = _np(ops.cloud_mesh_field(oc, FIELD_H, 0.5, lattice, _i32(slots[pick])))
    assert got.shape == (len(pick), 729)
    for row, i in zip(got, pick):
        assert _same(row, want[i]), (blocks[i], np.abs(row - want[i]).max())


def test_the_field_is_the_winding_number_at_the_nodes_and_shared_nodes_agree(field_case):
    from etch_amd import ops
    clouds, oc, lattice, blocks, slots, want = field_case
    got = _np(ops.cloud_mesh_field(oc, FIELD_H, 0.5, lattice, _i32(slots)))
    lo = np.full(3, FIELD_LO, np.int64)
    for i, (b, blk) in enumerate(blocks):
        q = MO.node_position(MO.block_nodes(lo, blk).reshape(-1, 3), FIELD_H)
        w = _np(ops.cloud_winding_number(oc, _dev(np.tile(q[None], (len(clouds), 1, 1))), want_nearest=False)[0])[b]
        assert _same(got[i], np.abs(w) - np.float32(0.5)), blocks[i]
    a, b = got[1].reshape(9, 9, 9), got[2].reshape(9, 9, 9)                     # (3,3,6) and (4,3,6) share a face
    assert _same(a[8], b[0]) and not _same(a[0], b[0])
    assert (got[4] == np.float32(-0.5)).all()                                     # the empty cloud: w = 0 everywhere
    q = got[3].reshape(9, 9, 9)[3, 4, 5]                                          # the row that lies on this node: d2 = 0, the term is 0 / (cap sqrt cap)
    assert q == want[3].reshape(9, 9, 9)[3, 4, 5] and np.isfinite(q)


def test_a_cloud_of_the_batch_is_bitwise_the_cloud_alone(field_case):
    from etch_amd import ops
    clouds, oc, lattice, blocks, slots, want = field_case
    for i, (b, _) in enumerate(blocks):
        alone = ops.cloud_mesh_field(_oriented([clouds[b]]), FIELD_H, 0.5, lattice[:1].contiguous(), _i32([[0, slots[i, 1]]]))
        assert _same(_np(alone)[0], want[i]), blocks[i]
    other = _np(ops.cloud_mesh_field(oc, FIELD_H, 0.4, lattice, _i32(slots[:1])))[0]      # another level
    assert _same(other, MO.block_field(clouds[5], FIELD_H, np.full(3, FIELD_LO, np.int64), blocks[0][1], 0.4).reshape(-1))
    bad = _np(ops.cloud_mesh_field(oc, FIELD_H, 0.5, lattice, _i32([[9, 0], [0, 512], [-1, 0], [0, -1]])))       # no such block: not written
    assert (bad == 0).all()


# ---- lattice and seeds ------------------------------------------------------------------------------------------------------------------------------
LAT_H = 0.125                                                                      # 8 h = 1: block boundaries at the integers


def _hand_clouds():
    f32 = np.float32
    nan, inf = f32(np.nan), f32(np.inf)
    a = np.array([[1.0, 0.5, 0.5], [-1.0, 0.25, 0.5], [-0.5, 2.0, 0.5], [2.999, 0.0, -0.001], [50.0, 50.0, 50.0], [nan, 0.0, 0.0], [0.0, inf, 0.0],
                  [-30.0, 0.0, 0.0]], f32)
    cap_a = np.array([1, 1, 1, 1, 0, 1, 1, 0], f32) * f32(1e-3)                    # the far rows carry no area; the non-finite ones do
    none = np.zeros((0, 3), f32)
    c = np.array([[0.5, 0.5, 0.5], [3.5, 0.5, 0.5]], f32)
    d = np.array([[0.1, 0.1, 0.1]], f32)
    return [(a, np.zeros_like(a), cap_a), (none, none, np.zeros(0, f32)), (c, np.zeros_like(c), np.zeros(2, f32)), (d, np.zeros_like(d), np.ones(1, f32))]


@pytest.mark.parametrize("pad", [0, 1, 2])
def test_the_lattice_by_integers(pad):
    from etch_amd import ops
    clouds = _hand_clouds()
    lattice, status = ops.cloud_mesh_lattice(_oriented(clouds), LAT_H, pad)
    ref = [MO.lattice(c[0], c[2], LAT_H, pad) for c in clouds]
    assert _np(status).tolist() == [r[2] for r in ref] == [0, MO.STATUS_EMPTY, MO.STATUS_EMPTY, 0]
    assert np.array_equal(_np(lattice), np.array([np.concatenate([r[0], r[1]]) for r in ref]))
    assert _np(lattice)[0].tolist() == [-1 - pad, 0 - pad, -1 - pad, 3 + pad, 3 + pad, 1 + pad]       # 1.0 lies in block 1, -1.0 in block -1, -0.001 in -1


def test_a_lattice_out_of_range_is_flagged_and_reconstruct_names_the_cloud():
    from etch_amd import _lib, cloud, ops
    f32 = np.float32
    far = np.array([[0.0, 0.0, 0.0], [2.0e5, 0.0, 0.0]], f32)
    wide = np.array([[0.0, 0.0, 0.0], [300.0, 300.0, 300.0]], f32)
    huge = np.array([[0.0, 0.0, 0.0], [3.0e38, 0.0, 0.0]], f32)
    ok = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], f32)
    clouds = [(p, np.zeros_like(p), np.ones(2, f32)) for p in (ok, far, wide, huge)]
    lattice, status = ops.cloud_mesh_lattice(_oriented(clouds), LAT_H, 2)
    assert _np(status).tolist() == [0, MO.STATUS_RANGE, MO.STATUS_RANGE, MO.STATUS_RANGE]         # nodes per axis, blocks, the coordinate itself
    assert [MO.lattice(c[0], c[2], LAT_H, 2)[2] for c in clouds] == _np(status).tolist()
    assert (_np(lattice)[1:] == 0).all()
    with pytest.raises(_lib.EtchHipError, match="cloud 1"):
        cloud.reconstruct(_oriented(clouds), LAT_H)


@pytest.mark.parametrize("dilate", [0, 1, 2])
@pytest.mark.parametrize("pad", [0, 1])
def test_the_seeds_by_integers(dilate, pad):
    from etch_amd import ops
    clouds = _hand_clouds()
    oc = _oriented(clouds)
    lattice, status = ops.cloud_mesh_lattice(oc, LAT_H, pad)
    lat = _np(lattice).astype(np.int64)
    n = lat[:, 3:] - lat[:, :3]
    toff = _toff(n)
    table = torch.full((int(_np(toff)[-1]),), -1, dtype=torch.int32, device=DEV)
    ops.cloud_mesh_seed(oc, LAT_H, dilate, lattice, status, toff, table)
    t, o = _np(table), _np(toff)
    for b, c in enumerate(clouds):
        got = t[o[b]:o[b + 1]].reshape(tuple(n[b]))
        if _np(status)[b]:
            assert got.size == 0
            continue
        want = MO.seeds(c[0], c[2], LAT_H, lat[b, :3], lat[b, 3:], dilate)
        assert np.array_equal(got == -2, want) and np.array_equal(got == -1, ~want)
    if dilate == 0:
        assert (t[o[0]:o[1]] == -2).sum() == 4 and (t[o[3]:o[4]] == -2).sum() == 1


# ---- growth -------------------------------------------------------------------------------------------------------------------------------------------
def test_growth_on_hand_made_fields():
    """One lattice of 3 x 2 x 1 blocks.  A = (1,0,0) is tested: -x mixed towards an inactive block (marked), +x mixed towards an active block (left
    alone), -y mixed and out of the lattice (clipped), +y uniform (its neighbour stays inactive), -z uniform, +z mixed through a NaN (inside) and out
    of the lattice.  B = (2,0,0), all NaN, has uniform faces."""
    from etch_amd import ops
    n = np.array([3, 2, 1])
    lattice = _i32([[0, 0, 0, 3, 2, 1]])
    toff = _toff(n)
    flat = lambda x, y, z: (x * 2 + y) * 1 + z      # noqa: E731
    table = np.full(6, -1, np.int32)
    table[flat(1, 0, 0)], table[flat(2, 0, 0)] = 0, 1
    a = -np.ones((9, 9, 9), np.float32)
    a[0, 4, 4] = 0.0                                                              # -x: one node inside (0 counts as inside)
    a[8, 4, 4] = 1.0                                                              # +x
    a[4, 0, 4] = -0.0                                                             # -y (-0 counts as inside)
    a[4, 4, 8] = np.nan                                                           # +z
    b = np.full((9, 9, 9), np.nan, np.float32)
    fields = {(1, 0, 0): a, (2, 0, 0): b}
    want_new, want_clipped = MO.grow(table.reshape(3, 2, 1) >= 0, fields, [(1, 0, 0), (2, 0, 0)], n)
    assert want_new == [(0, 0, 0)] and want_clipped == 2
    for pick in ([0], [0, 1]):
        tb = _dev(table.copy())
        slots = _i32([[0, flat(1, 0, 0)], [0, flat(2, 0, 0)]])[pick].contiguous()
        fld = _dev(np.stack([a.reshape(-1), b.reshape(-1)]))[pick].contiguous()
        flags = _np(ops.cloud_mesh_grow(lattice, toff, slots, fld, tb))
        assert flags[0].tolist() == [1, 0, 2, 0, 0, 2] and (flags[1:] == 0).all()
        after = table.copy()
        after[flat(0, 0, 0)] = -2
        assert np.array_equal(_np(tb), after)


# ---- extraction -----------------------------------------------------------------------------------------------------------------------------------------
EX_LO, EX_N, EX_H = np.array([-2, -1, 0]), np.array([5, 5, 1]), 0.0125
L_BLOCKS = [(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0), (0, 4, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0)]      # an L, in key order


@pytest.fixture(scope="module")
def random_lattice():
    rng = np.random.default_rng(27)
    s = rng.uniform(-1, 1, tuple(8 * EX_N + 1)).astype(np.float32)
    for val in (0.0, -0.0, np.nan):
        for _ in range(12):
            s[tuple(rng.integers(0, 8 * EX_N + 1))] = val
    s[3, 3, 3], s[8, 5, 2], s[8, 16, 8] = 0.0, np.nan, -0.0                        # and on a face two blocks share
    return s


def _fields(s, blocks):
    return np.stack([s[8 * b[0]:8 * b[0] + 9, 8 * b[1]:8 * b[1] + 9, 8 * b[2]:8 * b[2] + 9] for b in blocks])


def _on_boundary(keys, blocks):
    """Whether the lattice edge of each crossing key lies on the boundary of the union of the blocks: not every cell around it is active."""
    cells = np.zeros(tuple(8 * EX_N), bool)
    for b in blocks:
        cells[8 * b[0]:8 * b[0] + 8, 8 * b[1]:8 * b[1] + 8, 8 * b[2]:8 * b[2] + 8] = True
    pad = np.pad(cells, 1)
    kind = keys & 7
    i = np.stack([(keys >> 43) & 0xfffff, (keys >> 23) & 0xfffff, (keys >> 3) & 0xfffff], -1)
    d = np.stack([(kind >> 2) & 1, (kind >> 1) & 1, kind & 1], -1)
    inner = np.ones(len(keys), bool)
    for off in np.ndindex(2, 2, 2):
        c = i - np.array(off) * (1 - d)                                           # an axis the edge runs along has one cell coordinate, the others two
        inner &= pad[c[:, 0] + 1, c[:, 1] + 1, c[:, 2] + 1]
    return ~inner


@pytest.mark.parametrize("count", [1, 2, 9])
def test_the_extraction_on_random_fields(random_lattice, count):
    from etch_amd import ops
    blocks = L_BLOCKS[:count] if count != 2 else [L_BLOCKS[0], L_BLOCKS[5]]        # two face-adjacent blocks
    fld = _fields(random_lattice, blocks)
    slots = _i32([[0, (b[0] * EX_N[1] + b[1]) * EX_N[2] + b[2]] for b in blocks])
    lattice = _i32([np.concatenate([EX_LO, EX_LO + EX_N])])
    counts, keys, pos = ops.cloud_mesh_extract(lattice, EX_H, slots, _dev(fld.reshape(count, -1)))
    wc, wk, wp = MO.extract_faces(np.array(blocks), fld, EX_LO, EX_H)
    assert np.array_equal(_np(counts), wc) and np.array_equal(_np(keys), wk) and len(wk) > 3000 * count
    assert _same_or_nan(_np(pos), wp) and np.isnan(wp).any()
    vk, verts, faces = ops.cloud_mesh_weld(keys, pos)
    ok, ov, of = MO.weld(wk, wp)                                                    # asserts that a key has one position, by bits
    assert np.array_equal(_np(vk), ok) and np.array_equal(_np(faces), of) and _same_or_nan(_np(verts), ov) and faces.dtype == torch.int32
    assert _same_or_nan(_np(verts)[_np(faces).reshape(-1)], _np(pos).reshape(-1, 3))       # the GPU's own copies of a key agree too
    f = of.astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    e = e[e[:, 0] != e[:, 1]]                                                       # an exact zero at a node makes index-degenerate triangles: kept, not counted
    ue, n = np.unique(e[:, 0] * (1 << 32) + e[:, 1], return_counts=True)
    edge_on = _on_boundary(ok, blocks)[ue >> 32] & _on_boundary(ok, blocks)[ue & 0xffffffff]
    assert (~edge_on).sum() > 1000 * count and edge_on.sum() > 100
    assert (n[~edge_on] == 2).all() and (n <= 2).all() and (n[edge_on] == 1).any()      # interior to the blocks: two faces; one only at their boundary


# ---- components -------------------------------------------------------------------------------------------------------------------------------------------
def _tet(v):
    a, b, c, d = v
    return [[a, b, c], [a, c, d], [a, d, b], [b, d, c]]


def test_components_and_the_tie_rule_on_a_hand_made_mesh():
    from etch_amd import ops
    faces = np.array(_tet([1, 2, 3, 5]) + [[8, 9, 10]] + _tet([0, 4, 6, 7]), np.int32)       # two tetrahedra of four faces each, one triangle
    verts = np.arange(33, dtype=np.float32).reshape(11, 3)
    labels = ops.mesh_components(11, _dev(faces))
    assert _np(labels).tolist() == [0, 1, 1, 1, 0, 1, 0, 0, 8, 8, 8] == MO.labels(11, faces).tolist()
    per = np.bincount(_np(labels)[faces[:, 0]], minlength=11)
    assert per[0] == per[1] == 4                                                    # the tie: label 0 wins
    v, f = ops.mesh_keep_component(_dev(verts), _dev(faces), labels, 0)
    wv, wf, comps = MO.keep_largest(verts, faces, MO.labels(11, faces))
    assert comps == 3 and np.array_equal(_np(v), wv) and np.array_equal(_np(f), wf) and _np(f).tolist() == _tet([0, 1, 2, 3])
    v, f = ops.mesh_keep_component(_dev(verts), _dev(faces), labels, 8)
    assert np.array_equal(_np(v), verts[8:]) and _np(f).tolist() == [[0, 1, 2]]


def test_components_of_long_strips_with_shuffled_vertices():
    """Two strips of 3 000 and 2 000 triangles whose vertices are numbered at random: the labels need many rounds, and more than one call."""
    from etch_amd import ops
    rng = np.random.default_rng(5)
    strips = []
    base = 0
    for n in (3000, 2000):
        i = np.arange(n)
        strips.append(np.stack([i, i + 1, i + 2], 1) + base)
        base += n + 2
    faces = rng.permutation(base)[np.concatenate(strips)].astype(np.int32)
    faces = faces[rng.permutation(len(faces))]
    want = MO.labels(base, faces)
    assert len(np.unique(want)) == 2
    for passes in (1, 4):
        assert np.array_equal(_np(ops.mesh_components(base, _dev(faces), passes=passes)), want)


# ---- reconstruct end to end ---------------------------------------------------------------------------------------------------------------------------------
def _check(mesh, rec, b, want, center=None):
    v = want["verts"].astype(np.float64) + (0.0 if center is None else center)
    assert mesh.vertices.dtype == np.float64 and mesh.faces.dtype == np.int32
    assert np.array_equal(mesh.faces, want["faces"]) and np.array_equal(mesh.vertices, v)
    assert (bool(rec.closed[b]), int(rec.clipped[b]), int(rec.blocks[b]), int(rec.rounds[b]), int(rec.components[b]), int(rec.status[b])) == \
        (want["closed"], want["clipped"], want["nblocks"], want["rounds"], want["components"], want["status"])


@pytest.fixture(scope="module")
def two_clouds():
    return MO.sphere(2000, R, 8), MO.hemisphere()


@pytest.mark.parametrize("level", [0.5, 0.4])
def test_reconstruct_a_ragged_batch_at_five_centimetres(two_clouds, level):
    """The 2 000-row sphere and the 300-row hemisphere in one batch at voxel 0.05 (a call has ONE voxel), each against the oracle by integers and
    bits; each alone is bitwise the batch's; the centre is added in fp64."""
    from etch_amd import cloud
    want = [MO.reconstruct(c, 0.05, level=level) for c in two_clouds]
    center = np.array([[0.25, -1.0, 3.0], [10.0, 0.0, -0.125]])
    rec = cloud.reconstruct(_oriented(list(two_clouds)), 0.05, level=level, center=center)
    for b in range(2):
        _check(rec.meshes[b], rec, b, want[b], center[b])
        alone = cloud.reconstruct(_oriented([two_clouds[b]]), 0.05, level=level, center=center[b])
        _check(alone.meshes[0], alone, 0, want[b], center[b])
    assert rec.closed[0] and MO.euler(len(rec.meshes[0].vertices), rec.meshes[0].faces) == 2
    if level == 0.5:
        assert (len(rec.meshes[0].vertices), len(rec.meshes[0].faces)) == (5666, 11328)


def test_reconstruct_the_hemisphere_grows_closed_next_to_an_empty_cloud(two_clouds):
    """The open hemisphere at voxel 0.0125 behind an empty cloud in one batch: five rounds of growth, by integers and bits; the empty cloud yields an
    empty mesh that is not closed; with the rounds capped the result is flagged open; seed_dilate and keep= change what the oracle says they do."""
    from etch_amd import cloud
    f32 = np.float32
    empty = (np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, f32))
    hemi = two_clouds[1]
    want = MO.reconstruct(hemi, 0.0125)
    assert want["rounds"] == 5 and want["closed"]
    rec = cloud.reconstruct(_oriented([empty, hemi]), 0.0125)
    _check(rec.meshes[1], rec, 1, want)
    assert len(rec.meshes[0].vertices) == 0 and len(rec.meshes[0].faces) == 0 and not rec.closed[0] and rec.status[0] == MO.STATUS_EMPTY
    alone = cloud.reconstruct(_oriented([hemi]), 0.0125, keep="all")
    _check(alone.meshes[0], alone, 0, MO.reconstruct(hemi, 0.0125, keep="all"))
    capped = cloud.reconstruct(_oriented([hemi]), 0.0125, max_rounds=2)
    _check(capped.meshes[0], capped, 0, MO.reconstruct(hemi, 0.0125, max_rounds=2))
    assert not capped.closed[0]
    dil = cloud.reconstruct(_oriented([hemi]), 0.05, seed_dilate=1, pad_blocks=0)
    _check(dil.meshes[0], dil, 0, MO.reconstruct(hemi, 0.05, seed_dilate=1, pad_blocks=0))


# ---- the fixture body ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_body_at_two_centimetres():
    """Properties only (the oracle's field is too slow for this file at 6 721 rows): closed, the oracle's component count
    (tests/test_cloud_mesh_host.py), the largest component's share; the field of 8 of its blocks by bits."""
    from etch_amd import cloud, ops
    BODY_COMPONENTS = MO.BODY_COMPONENTS_2CM
    p, n, flag, _, _ = WO.body_views()
    surf = WO.surface(p, n, 8, flag)
    oc = _oriented([surf])
    both = {keep: cloud.reconstruct(oc, 0.02, keep=keep) for keep in MO_KEEP}
    every, largest = both["all"].meshes[0], both["largest"].meshes[0]
    assert both["all"].closed[0] and both["largest"].closed[0] and all(MO.edge_counts(every.faces)) and all(MO.edge_counts(largest.faces))
    assert both["all"].components[0] == both["largest"].components[0] == BODY_COMPONENTS
    assert len(largest.faces) >= 0.98 * len(every.faces) and len(np.unique(MO.labels(len(largest.vertices), largest.faces))) == 1
    assert MO.volume(largest.vertices, largest.faces) > 0
    lattice, status = ops.cloud_mesh_lattice(oc, 0.02, 2)
    lat = _np(lattice)[0].astype(np.int64)
    seeds = np.argwhere(MO.seeds(surf[0], surf[2], 0.02, lat[:3], lat[3:], 0))
    pick = seeds[np.linspace(0, len(seeds) - 1, 8).astype(int)]
    nn = lat[3:] - lat[:3]
    slots = _i32([[0, (b[0] * nn[1] + b[1]) * nn[2] + b[2]] for b in pick])
    got = _np(ops.cloud_mesh_field(oc, 0.02, 0.5, lattice, slots))
    for row, b in zip(got, pick):
        assert _same(row, MO.block_field(surf, 0.02, lat[:3], b, 0.5).reshape(-1)), b


# ---- the command ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def common(tmp_path_factory):
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import load_seeded
    data = _train_data.build(tmp_path_factory.mktemp("mesh_data"), DEV)
    opt = types.SimpleNamespace(output_folder=os.path.join(data.root, "model"), EPN_input_radius=0.4, EPN_layer_num=2, markerset=K.default_markerset(),
                                device=torch.device(DEV))
    path = os.path.join(data.root, "model.pth")
    torch.save(load_seeded(GT_network_equiv(option=opt), 1).state_dict(), path)
    return ["--model_path", path, "--markerset_path", os.path.join(data.root, "markers.json"), "--num_point", "1024", "--synthetic_body", "--seed", "4"]


def _write_ply(path, p):
    cols = "".join(f"property double {c}\n" for c in ("x", "y", "z"))
    path.write_bytes(f"ply\nformat binary_little_endian 1.0\nelement vertex {len(p)}\n{cols}end_header\n".encode() + p.astype("<f8").tobytes())


def test_the_command_writes_the_subjects_surface(common, tmp_path):
    """python -m etch_amd.cloud on three views of the fixture body with --align_global --mesh_out: the OBJ reads back closed, in the input frame, and
    the report carries the mesh fields; without the flag the outputs are what they were."""
    from etch_amd import cloud as C, mesh_io
    parts = [GO.view(az) for az in WO.BODY_AZIMUTHS]
    moved = [GO.moved(p, cam, turn, cam)[0] for (p, cam), turn in zip(parts, (0.0, 25.0, -20.0))]
    for n, m in zip("abc", moved):
        _write_ply(tmp_path / f"{n}.ply", m)
    base = ["--cloud_path", str(tmp_path / "a.ply"), "--more_views", str(tmp_path / "b.ply"), str(tmp_path / "c.ply"), "--align_global", "--align_gate_min",
            "0.01", "--align_decay", "0.85", "--align_iters", "60", "--fuse_voxel", "0.005"] + common
    C.main(base + ["--mesh_out", "--mesh_voxel", "0.02", "--output_folder", str(tmp_path / "with")])
    C.main(base + ["--output_folder", str(tmp_path / "without")])
    names = sorted(os.listdir(tmp_path / "with"))
    assert sorted(os.listdir(tmp_path / "without")) == [n for n in names if n != "a_surface.obj"] and "a_surface.obj" in names
    rep, plain = np.load(tmp_path / "with" / "a_cloud.npz"), np.load(tmp_path / "without" / "a_cloud.npz")
    fields = ["mesh_closed", "mesh_blocks", "mesh_rounds", "mesh_components", "mesh_vertices", "mesh_faces"]
    assert sorted(set(rep.files) - set(plain.files)) == sorted(fields) and set(plain.files) <= set(rep.files)
    mesh = mesh_io.read_obj(str(tmp_path / "with" / "a_surface.obj"))
    v, f = np.asarray(mesh.vertices), np.asarray(mesh.faces)
    assert bool(rep["mesh_closed"]) and all(MO.edge_counts(f)) and (len(v), len(f)) == (int(rep["mesh_vertices"]), int(rep["mesh_faces"]))
    assert int(rep["mesh_components"]) >= 1 and int(rep["mesh_blocks"]) > 0
    # the input frame is the first view's: its rows lie on the surface.  A vertex is at most half a 2 cm cell's diagonal (1.7 cm) from any surface
    # point of its cell, and the level set lies within a few millimetres of the rows, so the median row is within 3 cm of a vertex.
    d = np.concatenate([np.sqrt(((moved[0][i:i + 256, None, :] - v[None]) ** 2).sum(-1).min(1)) for i in range(0, len(moved[0]), 256)])
    print(f"PIN command mesh: {len(v)} vertices, {len(f)} faces, {int(rep['mesh_components'])} components, {int(rep['mesh_blocks'])} blocks, "
          f"{int(rep['mesh_rounds'])} rounds; first view's rows to the nearest vertex: median {np.median(d) * 1e3:.1f} mm, p95 {np.percentile(d, 95) * 1e3:.1f} mm")
    assert np.median(d) < 0.03 and MO.volume(v, f) > 0.05
