"""The yardsticks of tests/test_gpu_handover.py have teeth on the inputs they are used on -- shown on the CPU, no GPU needed.  The numpy references
of tests/_handover_ref.py agree with torch on the CPU wherever torch defines the answer, the inputs contain the edges they are built for, and seven
wrong answers of the kind a kernel could give each fail the checker that the GPU output goes through."""
import numpy as np
import pytest
import torch

from tests import _handover_ref as H

F32 = np.float32


# ------------------------------------------------------------------------------------------------ references against torch
def test_argmax_reference_is_torch_argmax_on_every_input():
    """torch.argmax on the CPU: first maximum, -0 == +0, a NaN of either sign above +inf and the first NaN taken."""
    for name, x in list(H.am_inputs()) + [("chain", H.chain_inputs()["logits"])]:
        assert np.array_equal(H.argmax_ref(x), torch.argmax(torch.from_numpy(x), -1).numpy()), name
    assert list(H.argmax_ref(H.am_edge_rows())) == [0, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0]


def test_marker_reference_is_topk_pow_weighted_mean_where_nothing_ties():
    """A fresh torch restatement (topk, ** 20, weighted mean) on untied confidences.  torch.topk's order among equal values is unspecified (on the
    CPU it gave [1, 4, 3] for four equal values), so "ties to the lower index" is this project's definition and has no torch counterpart."""
    rng = np.random.default_rng(3)
    for M, K in ((3, 200), (86, 1000)):
        i = dict(H.mk_random(M, K))
        i["conf"] = (0.9 + 0.1 * rng.permutation(2 * K).reshape(2, K, 1) / (2 * K)).astype(F32)          # all different
        sel, centres, valid = H.markers_ref(i)
        pts, lab, conf = torch.from_numpy(i["pts"]).double(), torch.from_numpy(i["labels"]), torch.from_numpy(i["conf"][..., 0])
        for b in range(2):
            for m in range(M):
                at = torch.nonzero(lab[b] == m)[:, 0]
                assert bool(valid[b, m]) == (len(at) > 0)
                if len(at):
                    c, k = torch.topk(conf[b, at], min(3, len(at)))
                    assert np.array_equal(at[k].numpy(), sel[b][m])
                    w = (c ** 20).double()
                    want = (pts[b, at[k]] * w[:, None]).sum(0) / w.sum()
                    assert np.abs(centres[b, m] - want.numpy()).max() <= 2.0 ** -50
    assert H.check_markers(H.markers_from(i, H.select_top3), i) < 0.1          # fp32 rounding of the centre alone


def test_interp_and_inner_references_are_torch_fp32():
    i = H.pi_inputs(64, 7, 9)
    f, idx, w = torch.from_numpy(i["feats"]), torch.from_numpy(i["idx"][:18].reshape(2, 9, 3)).long(), torch.from_numpy(i["weight"][:18].reshape(2, 9, 3))
    g = torch.stack([f[b][idx[b]] for b in range(2)]) * w[..., None, None]
    assert H.same_bits(H.pi_ref(i), ((g[:, :, 0] + g[:, :, 1]) + g[:, :, 2]).reshape(18, 7, 64).numpy())
    for shape in H.IP_SHAPES:
        i = H.ip_inputs(*shape)
        t = {k: torch.from_numpy(i[k]) for k in ("pts", "dir", "mag")}
        assert H.same_bits(H.inner_ref(i), (t["pts"] - t["dir"] * t["mag"] / i["scale"]).numpy())
        H.check_inner(H.inner_ref(i), i)


def test_status_reference_and_its_three_outcomes():
    for M in H.MS_MS:
        for bad in ("inf", "-inf", "nan"):
            i = H.ms_inputs(M, bad)
            assert list(H.status_ref(i)) == [0, 1, 2]
            assert M <= 64 or not np.isfinite(i["markers"][1, 64:]).all()
            with pytest.raises(AssertionError, match="marker status"):
                H.check_status(np.array([1 if M > 1 else 0, 0, 2], np.int32), i)        # the unvalid bad marker counted, the valid one missed


# ------------------------------------------------------------------------------------------------ the inputs are sharp
def test_lattice_distances_are_exact_in_fp32_and_hold_the_edges():
    for S, N in H.P3_SHAPES:
        i = H.p3_lattice(S, N)
        x, y = i["xyz1"], i["xyz2"].transpose(0, 2, 1)
        assert (x * 8 == np.round(x * 8)).all() and (y * 8 == np.round(y * 8)).all() and np.abs(x).max() <= 2 and np.abs(y).max() <= 2
        dot = (x[:, :, None, 0] * y[:, None, :, 0] + x[:, :, None, 1] * y[:, None, :, 1]) + x[:, :, None, 2] * y[:, None, :, 2]
        d32 = (F32(-2) * dot + (x * x).sum(-1, dtype=F32)[:, :, None]) + (y * y).sum(-1, dtype=F32)[:, None, :]
        d = H.p3_sqdist(i)
        assert d32.dtype == F32 and np.array_equal(d32.astype(np.float64), d)                # every step of the fp32 evaluation is exact
        idx, _ = H.p3_lattice_ref(i, d)
        d3 = np.take_along_axis(d, idx.astype(np.int64), -1)
        for b in range(2):
            assert list(idx[b, 0, :1]) == [S - 1] and d3[b, 0, 0] == 0 and d3[b, 0, 1] > 0         # a unique nearest neighbour, the last coarse point
            assert S < 4 or (y[b, S // 3] == y[b, 0]).all()
            if S - 1 > 1024 and N > 1:
                assert list(idx[b, 1, :2]) == [5, 1024] and (d3[b, 1, :2] == 0).all()           # tile 0 against tile 1, the earlier first
        if S > 1000 and N > 1:
            assert (d3[..., 2] == np.sort(d, -1)[..., 3]).any()                                  # ties across the rank-3 boundary


def test_off_lattice_reference_passes_its_own_check():
    for S, N in ((3, 255), (1025, 257)):
        i = H.p3_gauss(S, N)
        d = H.p3_sqdist(i)
        idx = np.argsort(d, -1, kind="stable")[..., :3]
        excess, dev = H.check_p3_gauss((idx.astype(np.int32), H.p3_weights(np.take_along_axis(d, idx, -1)).astype(F32)), i)
        assert excess < 1e-6 and dev <= 1.5


def test_marker_inputs_pin_the_selected_set_not_only_the_centre():
    """No exchange of one selected point for a left-out one of its label moves a centre by less than 100 bounds; the scenes are what they say."""
    for name, i in H.mk_inputs():
        assert H.swap_margin(i) > 100, name
    i = H.mk_scenes()
    sel, centres, valid = H.markers_ref(i)
    scene = {n: j for j, n in enumerate(H.MK_SCENES)}
    for b in range(2):
        at = lambda n: scene[n] if b == 0 else 85 - scene[n]
        count = lambda n: int((i["labels"][b] == at(n)).sum())
        assert [count(n) for n in ("no point", "one point", "two points", "three points", "four points")] == [0, 1, 2, 3, 4]
        assert not valid[b, at("no point")] and valid[b].sum() == 69       # 15 scenes and the 54 background labels
        for n in ("one lane ascending", "one lane descending", "one lane mixed"):
            assert count(n) == 5 and (np.flatnonzero(i["labels"][b] == at(n)) % 64 == 7).all()
        assert len(set(np.flatnonzero(i["labels"][b] == at("five lanes")) % 64)) == 5
        assert np.isnan(centres[b, at("-0 before +0")]).tolist() == [True, False, False] and np.isfinite(centres[b, at("+0 before -0")]).all()
        for n in ("positive NaN", "negative NaN", "underflow"):
            assert np.isnan(centres[b, at(n)]).all() and valid[b, at(n)] and count(n) > 3
        assert set(np.unique(i["labels"][b])) >= {-1, 86, 300}
    # every rank of the per-lane list is inserted into: ascending -> always rank 0, descending -> ranks 0, 1, 2, mixed -> rank 1 too
    assert np.signbit(i["conf"][i["labels"] == scene["negative NaN"]]).any() and not np.signbit(i["conf"][i["labels"] == scene["positive NaN"]]).any()


# ------------------------------------------------------------------------------------------------ the seven wrong answers
def test_3nn_ties_to_the_later_index_fail():
    i = H.p3_lattice(2049, 257)
    d = H.p3_sqdist(i)
    S = d.shape[-1]
    idx = (S - 1 - np.argsort(d[..., ::-1], -1, kind="stable")[..., :3]).astype(np.int32)
    w = H.p3_weights(np.take_along_axis(d, idx.astype(np.int64), -1)).astype(F32)
    with pytest.raises(AssertionError, match="3-NN indices differ"):
        H.check_p3_lattice((idx, w), i)


@pytest.mark.parametrize("S", [1025, 2049])
def test_3nn_that_skips_coarse_index_1024_fails(S):
    """The first point of the second LDS tile never becomes a candidate: seen on the lattice (indices) and off it (a farther neighbour)."""
    for make, check, why in ((H.p3_lattice, H.check_p3_lattice, "3-NN indices differ"), (H.p3_gauss, H.check_p3_gauss, "farther than the rank's nearest")):
        i = make(S, 257)
        d = H.p3_sqdist(i)
        assert (np.argsort(d, -1, kind="stable")[..., :3] == 1024).any()
        d[..., 1024] = np.inf
        idx = np.argsort(d, -1, kind="stable")[..., :3]
        w = H.p3_weights(np.take_along_axis(d, idx, -1)).astype(F32)
        with pytest.raises(AssertionError, match=why):
            check((idx.astype(np.int32), w), i)


def sortable(c):
    """Floats ordered by bit pattern: -0 below +0, a NaN with the sign bit set below -inf."""
    u = np.ascontiguousarray(c, F32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def key_plus_zero_wins(c):
    k = sortable(np.where(np.isnan(c), np.inf, c))
    return np.where(np.isnan(c), 1 << 33, k)


def key_negative_nan_lowest(c):
    k = sortable(np.where(c == 0, 0.0, c).astype(F32))              # +-0 equal
    return np.where(np.isnan(c) & ~np.signbit(c), 1 << 33, k)


def select_by(key, keep=3):
    def select(labels, conf, m):
        cand = np.flatnonzero(labels == m)
        return cand[np.lexsort((cand, -key(conf[cand])))][:keep]
    return select


@pytest.mark.parametrize("key, scene", [(key_plus_zero_wins, "-0 before +0"), (key_negative_nan_lowest, "negative NaN")])
def test_an_order_by_bit_pattern_fails_argmax_and_markers(key, scene):
    """+0 beats -0; a NaN with the sign bit set ranks lowest."""
    for name, x in H.am_inputs():
        got = np.argmax(key(x), -1)                       # integer keys: the first of equal ones
        if name in ("edges", "R=1031 G=86", "R=%d G=%d" % H.AM_BIG):
            with pytest.raises(AssertionError, match="argmax differs"):
                H.check_argmax(got.astype(np.int64), x)
    i = H.mk_scenes()
    with pytest.raises(AssertionError, match="NaN components differ") as e:
        H.check_markers(H.markers_from(i, select_by(key)), i)
    j = H.MK_SCENES.index(scene)
    assert f"(0, {j}, 0)" in str(e.value) and f"(1, {85 - j}, 0)" in str(e.value)
    for M, K in H.MK_SHAPES:                                                  # the random inputs have neither: the two orders agree there
        H.check_markers(H.markers_from(H.mk_random(M, K), select_by(key)), H.mk_random(M, K))


def test_top_two_instead_of_top_three_fails():
    for name, i in H.mk_inputs():
        if "K=1 " not in name + " ":
            with pytest.raises(AssertionError, match="marker centre off|NaN components differ"):
                H.check_markers(H.markers_from(i, lambda l, c, m: H.select_top3(l, c, m)[:2]), i)


def test_a_lane_list_that_keeps_its_best_two_fails():
    """Each of the 64 lanes (index mod 64) keeps two candidates instead of three: wrong only where a label's best three share a lane."""
    def select(labels, conf, m):
        cand = np.flatnonzero(labels == m)
        kept = np.concatenate([H.rank_order(cand[cand % 64 == l], conf[cand[cand % 64 == l]])[:2] for l in range(64)] + [cand[:0]])
        return H.rank_order(kept, conf[kept])[:3]

    i = H.mk_scenes()
    with pytest.raises(AssertionError, match=r"marker centre off .* \(0, 5, ") as e:
        H.check_markers(H.markers_from(i, select), i)
    sel_ref, sel_bad = H.markers_ref(i)[0], H.markers_ref(i, select)[0]
    differ = sorted(m for m in range(86) if not np.array_equal(sel_ref[0][m], sel_bad[0][m]))
    assert differ == [5, 6, 7], (differ, str(e.value))


@pytest.mark.parametrize("N", H.PI_NS)
def test_a_written_order_slot_past_n_fails(N):
    """The ordered grid has 8 ceil(N / 8) slots; one past N that is not skipped reads the guard slot and writes the guard row."""
    i = H.pi_inputs(32, 7, N)
    out = np.full((2 * N + 1, 7, 32), np.nan, F32)
    inv = np.full((2 * N + 1, 32), np.nan, F32)
    out[:2 * N] = H.pi_ref(i)
    inv[:2 * N] = out[:2 * N].astype(np.float64).mean(1)
    H.check_interp((out, inv), i)
    assert (i["orders"]["permutation"][2 * N:] == N).all()
    out[2 * N], inv[2 * N] = out[0], inv[0]
    with pytest.raises(AssertionError, match="wrote past the last fine point"):
        H.check_interp((out, inv), i)
    out[2 * N], inv[2 * N], inv[N] = np.nan, np.nan, np.nan                   # and a row nobody wrote
    with pytest.raises(AssertionError, match="left a row unwritten"):
        H.check_interp((out, inv), i)


def test_chain_reference_runs_on_its_inputs():
    i = H.chain_inputs()
    labels = H.argmax_ref(i["logits"])
    assert labels[0, 2] == 40 and labels[1, 4] == 10 and labels[1, 6] == 12
    assert (np.bincount(labels[0], minlength=86)[[3, 50]] > 3).all()
    st = H.chain_stage_inputs(i, labels, H.inner_ref(i))
    H.check_markers(H.markers_from(st, H.select_top3), st)
    assert H.swap_margin(st) > 100
    _, centres, valid = H.markers_ref(st)
    assert list(H.status_ref({"markers": centres.astype(F32), "valid_f": valid.astype(F32)})) == [0, 1]
