"""The kernels that hand data from one stage to the next -- etch_prop3nn, etch_prop_interp[_ordered], etch_argmax_rows, etch_inner_points,
etch_get_markers, etch_marker_status -- against the plain references of tests/_handover_ref.py, at the sizes where their code takes another path:
the 1024-point LDS tile of the 3-NN search, the four widths and the XCD-striped order grid of the interpolation, the 64-lane strides of the arg-max,
the marker selection and the status word.  tests/test_handover_host.py shows on the CPU that the same checkers fail seven wrong answers on the same
inputs.  Every case prints `PIN` lines with the observed maximum in the unit of its bound; profiles/handover_pins.txt is the record of a run."""
import numpy as np
import pytest
import torch

from tests import _handover_ref as H

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 3-NN
@pytest.mark.parametrize("S, N", H.P3_SHAPES)
def test_prop3nn_on_the_lattice_is_the_stable_order(S, N):
    from etch_amd import ops
    i = H.p3_lattice(S, N)
    idx, w = ops.prop3nn(dev(i["xyz1"]), dev(i["xyz2"]))
    worst = H.check_p3_lattice((host(idx), host(w)), i)
    print(f"PIN prop3nn lattice S={S} N={N}: idx equal; weight rel err {worst:.2f} U of 6 U")


@pytest.mark.parametrize("S, N", H.P3_SHAPES)
def test_prop3nn_off_the_lattice_finds_the_nearest_within_fp32(S, N):
    from etch_amd import ops
    i = H.p3_gauss(S, N)
    idx, w = ops.prop3nn(dev(i["xyz1"]), dev(i["xyz2"]))
    excess, dev1 = H.check_p3_gauss((host(idx), host(w)), i)
    print(f"PIN prop3nn gauss S={S} N={N}: max excess {excess:.3f} tol; |sum w - 1| {dev1:.2f} U of 3 U")


@pytest.mark.parametrize("S", [1, 2])
def test_prop3nn_needs_three_coarse_points(S):
    from etch_amd import ops
    from etch_amd._lib import EtchHipError
    with pytest.raises(EtchHipError, match="invalid argument") as e:
        ops.prop3nn(torch.zeros((2, 4, 3), device="cuda"), torch.zeros((2, 3, S), device="cuda"))
    assert e.value.status == -1


# ------------------------------------------------------------------------------------------------ interpolation
def _interp(i, order):
    """etch_prop_interp_ordered on NaN-prefilled out and inv with one guard row each."""
    from etch_amd import _lib
    B, N, S, A, C = (i[k] for k in "BNSAC")
    out = torch.full((B * N + 1, A, C), float("nan"), device="cuda")
    inv = torch.full((B * N + 1, C), float("nan"), device="cuda")
    o = i["orders"][order]
    _lib.call("etch_prop_interp_ordered", B, N, S, A, C, dev(i["feats"]), dev(i["idx"]), dev(i["weight"]), out, inv, None if o is None else dev(o))
    return host(out), host(inv)


@pytest.mark.parametrize("A", H.PI_AS)
@pytest.mark.parametrize("C", H.PI_CS)
def test_prop_interp_is_the_fp32_blend_in_every_order(C, A):
    from etch_amd import ops
    worst = 0.0
    for N in H.PI_NS:
        i = H.pi_inputs(C, A, N)
        got = {order: _interp(i, order) for order in H.PI_ORDERS}
        for order in H.PI_ORDERS:
            worst = max(worst, H.check_interp(got[order], i))
            assert H.same_bits(got[order][0], got["none"][0]) and H.same_bits(got[order][1], got["none"][1]), f"order={order} changes the result"
        out, inv = ops.prop_interp(dev(i["feats"]), dev(i["idx"][:2 * N].reshape(2, N, 3)), dev(i["weight"][:2 * N].reshape(2, N, 3)))
        assert H.same_bits(host(out).reshape(2 * N, A, C), got["none"][0][:2 * N]) and H.same_bits(host(inv).reshape(2 * N, C), got["none"][1][:2 * N])
    print(f"PIN prop_interp C={C} A={A} N={H.PI_NS} x {H.PI_ORDERS}: out bit-equal; inv err {worst:.3f} of (A + 1) U mean|out|")


def test_prop_interp_rejects_an_unsupported_width():
    from etch_amd import ops
    from etch_amd._lib import EtchHipError
    with pytest.raises(EtchHipError, match="unsupported"):
        ops.prop_interp(torch.zeros((1, 5, 2, 16), device="cuda"), torch.zeros((1, 4, 3), dtype=torch.int32, device="cuda"), torch.ones((1, 4, 3), device="cuda"))


# ------------------------------------------------------------------------------------------------ arg-max
@pytest.mark.parametrize("G", H.AM_GS)
def test_argmax_rows_first_maximum(G):
    from etch_amd import ops
    for R in H.AM_RS:
        x = H.am_input(R, G)
        H.check_argmax(host(ops.argmax_rows(dev(x))), x)
    print(f"PIN argmax_rows G={G} R={H.AM_RS}: equal")


def test_argmax_rows_signed_zeros_and_nans():
    """torch.argmax: -0 == +0 (the first wins) and a NaN of either sign is the greatest value (the first NaN wins)."""
    from etch_amd import ops
    x = H.am_edge_rows()
    got = host(ops.argmax_rows(dev(x)))
    print(f"PIN argmax_rows edges: got {got.tolist()} want {H.argmax_ref(x).tolist()}")
    H.check_argmax(got, x)


def test_argmax_rows_row_stride_loop():
    """R = 2 097 200 rows of G = 2: more than 65535 * 8 workgroups of 4 rows, so workgroups take a second row."""
    from etch_amd import ops
    x = H.am_input(*H.AM_BIG)
    H.check_argmax(host(ops.argmax_rows(dev(x))), x)
    print(f"PIN argmax_rows R={H.AM_BIG[0]} G={H.AM_BIG[1]}: equal")


# ------------------------------------------------------------------------------------------------ inner points
@pytest.mark.parametrize("B, N", H.IP_SHAPES)
def test_inner_points_bit_equal(B, N):
    """The grid cap (65535 * 8 workgroups) needs more than 400 MB per array to reach and is left untested."""
    from etch_amd import ops
    i = H.ip_inputs(B, N)
    H.check_inner(host(ops.inner_points(dev(i["pts"]), dev(i["dir"]), dev(i["mag"]), i["scale"])), i)
    print(f"PIN inner_points n={B * N}: bit-equal")


# ------------------------------------------------------------------------------------------------ markers
def _markers(i):
    from etch_amd import ops
    return tuple(host(t) for t in ops.get_markers(dev(i["pts"]), dev(i["labels"]), dev(i["conf"]), i["M"]))


def test_get_markers_scenes():
    """Labels with 0 .. 4 points, five points in one lane in three orders and over five lanes, four equal confidences across rank 3, ignored labels,
    negative, signed-zero, NaN and underflowing confidences (tests/_handover_ref.py: mk_scenes)."""
    i = H.mk_scenes()
    got = _markers(i)
    for j, name in enumerate(H.MK_SCENES):
        print(f"PIN get_markers scene '{name}': scan 0 {np.round(got[0][0, j].astype(float), 4).tolist()} scan 1 {np.round(got[0][1, 85 - j].astype(float), 4).tolist()}")
    worst = H.check_markers(got, i)
    print(f"PIN get_markers scenes M=86 K=1000: centre err {worst:.3f} of 32 U max|p|")


@pytest.mark.parametrize("M, K", H.MK_SHAPES)
def test_get_markers_tied_confidences(M, K):
    i = H.mk_random(M, K)
    worst = H.check_markers(_markers(i), i)
    print(f"PIN get_markers random M={M} K={K}: centre err {worst:.3f} of 32 U max|p|")


# ------------------------------------------------------------------------------------------------ marker status
@pytest.mark.parametrize("bad", ["inf", "-inf", "nan"])
@pytest.mark.parametrize("M", H.MS_MS)
def test_marker_status_per_scan(M, bad):
    from etch_amd import ops
    i = H.ms_inputs(M, bad)
    got = host(ops.marker_status(dev(i["markers"]), dev(i["valid_f"])))
    print(f"PIN marker_status M={M} bad={bad}: {got.tolist()} want {H.status_ref(i).tolist()}")
    H.check_status(got, i)


# ------------------------------------------------------------------------------------------------ the chain
def test_the_chain_from_logits_to_status():
    """argmax_rows -> inner_points -> get_markers -> marker_status on logits (2,130,86): every stage against the reference's, fed the stage before."""
    from etch_amd import ops
    i = H.chain_inputs()
    labels = ops.argmax_rows(dev(i["logits"]))
    H.check_argmax(host(labels), i["logits"])
    inner = ops.inner_points(dev(i["pts"]), dev(i["dir"]), dev(i["mag"]), i["scale"])
    assert H.same_bits(host(inner), H.inner_ref(i))
    markers, valid_f, valid_b = ops.get_markers(inner, labels, dev(i["conf"]), 86)
    st = H.chain_stage_inputs(i, H.argmax_ref(i["logits"]), H.inner_ref(i))
    worst = H.check_markers((host(markers), host(valid_f), host(valid_b)), st)
    _, centres, valid = H.markers_ref(st)
    H.check_status(host(ops.marker_status(markers, valid_f)), {"markers": centres.astype(F32), "valid_f": valid.astype(F32)})
    print(f"PIN chain (2,130,86): labels equal, inner bit-equal, centre err {worst:.3f} of 32 U max|p|, status {host(ops.marker_status(markers, valid_f)).tolist()}")
