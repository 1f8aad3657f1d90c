"""The yardstick of tests/test_gpu_backward_fp64.py has teeth at the shapes it is used at -- shown on the CPU, no GPU needed.  At the
256 -> 256 inter conv and the E = 256 attention layer the oracle's own fp32 gradients stand in for a kernel's: they pass the per-channel
entitled-error rule (tests/_bwd_fp64.py), and four seeded defects of the size and kind a backward kernel could have each fail it.  The first
of them passes the statistic the backward kernels were held to before (one global maximum, rel_err < 1e-4): the reason for this file."""
import numpy as np
import pytest
import torch

from oracle import stage1 as S1
from tests import _bwd_fp64 as B
from tests._parity import rel_err


@pytest.fixture(scope="module")
def inter():
    pr = B.inter_problem(256, 256, 32, 1, True)
    r64, r32, G = B.inter_oracle(pr)
    return pr, r64, r32, G


@pytest.fixture(scope="module")
def attention():
    inputs = B.mhsa_inputs(37, 256, 5)
    r64, r32, G = B.mhsa_oracle(*inputs, residual=True)
    return inputs, r64, r32, G


def slot_weights(pr, b, p, dtype):
    """w[a, k, n] of target point p of scan b (functional.py:286-324), in `dtype`."""
    t = lambda a: torch.as_tensor(a).to(dtype)
    return S1.inter_weights(t(pr["g"])[b:b + 1, :, p:p + 1], t(pr["anchors"]), t(pr["kernels"]), pr["sigma"])[0, 0].numpy()


def test_oracle_fp32_gradients_pass_the_rule(inter, attention):
    pr, r64, r32, _ = inter
    B.check("inter 256->256 y", B.channels_last(r32.y), B.channels_last(r64.y), B.channels_last(r32.y))
    B.check("inter 256->256 dfeats", B.channels_last(r32.grads["feats"]), B.channels_last(r64.grads["feats"]), B.channels_last(r32.grads["feats"]))
    B.check_weight("inter 256->256 dW", r32.grads["W"], r64.grads["W"], r32.grads["W"])
    B.check_bias("inter 256->256 dbias", r32.grads["bias"], r64.grads["bias"], r32.grads["bias"])
    _, a64, a32, _ = attention
    B.check("mhsa E=256 dx", a32.grads["x"], a64.grads["x"], a32.grads["x"])
    for k in ("wq", "wk", "wv", "wc"):
        B.check_weight(f"mhsa E=256 d{k}", a32.grads[k], a64.grads[k], a32.grads[k])
    B.check_bias("mhsa E=256 dbc", a32.grads["bc"], a64.grads["bc"], a32.grads["bc"])


def test_a_channel_window_of_dfeats_scaled_by_2e_5_fails_the_rule_and_passed_the_old_one(inter):
    """The second 64-channel window (cbase = 64 of etch_inter_dfeat / etch_inter_dfeat_slots) times 1 + 2e-5."""
    _, r64, r32, _ = inter
    ref64, ref32 = B.channels_last(r64.grads["feats"]), B.channels_last(r32.grads["feats"])
    bad = ref32.copy()
    bad[..., 64:128] *= np.float32(1 + 2e-5)
    assert rel_err(bad, ref64) < 1e-4                      # the statistic of tests/test_gpu_backward.py does not see it
    with pytest.raises(AssertionError, match="per-channel rel"):
        B.check("dfeats, window 1 scaled", bad, ref64, ref32)


def test_a_dropped_padded_slot_fails_the_rule(inter):
    """One padded slot (a repeat of an earlier neighbour in the same ball) of one target point contributes nothing to its source point."""
    pr, r64, r32, G = inter
    ball = pr["ball"].numpy()
    W = pr["W"].reshape(256, 256, 24)
    for p in range(ball.shape[1]):
        row = ball[0, p]
        pads = [n for n in range(len(row)) if row[n] in row[:n]]
        w = slot_weights(pr, 0, p, torch.float32)
        pads = [n for n in pads if w[:, :, n].max() > 0.1]
        if pads:
            break
    n = pads[-1]
    contrib = np.einsum("ak,ock,oa->ac", w[:, :, n], W, G[0, :, p, :])            # (anchor, input channel): sum_k w[a,k,n] dX1[(p,a), c 24 + k]
    assert np.abs(contrib).max() > 0
    ref64, ref32 = B.channels_last(r64.grads["feats"]), B.channels_last(r32.grads["feats"])
    bad = ref32.copy()
    bad[0, row[n]] -= contrib.astype(np.float32)
    with pytest.raises(AssertionError, match="per-channel rel"):
        B.check("dfeats, one padded slot dropped", bad, ref64, ref32)


def test_a_row_left_out_of_dW_fails_the_rule(inter):
    """dW = dY^T X1 over the rows (scan, target point, anchor): the last row of the first fifth of them (the end of a workgroup's row range
    in etch_gemm_tn_fused) is left out."""
    pr, r64, r32, G = inter
    p2 = pr["ball"].shape[1]
    r = pr["b"] * p2 * 60 // 5 - 1
    b, p, a = r // (p2 * 60), (r // 60) % p2, r % 60
    w = slot_weights(pr, b, p, torch.float32)
    x1 = np.einsum("cn,kn->ck", pr["feats"][b][:, pr["ball"].numpy()[b, p], a], w[a]).reshape(-1)        # X1[(b,p,a), c 24 + k]
    bad = r32.grads["W"] - np.outer(G[b, :, p, a], x1).astype(np.float32)
    with pytest.raises(AssertionError, match="per-channel rel"):
        B.check_weight("dW, one row left out", bad, r64.grads["W"], r32.grads["W"])


def test_one_heads_dK_scaled_by_2e_5_fails_the_rule(attention):
    """dK of head 3 times 1 + 2e-5: the head's 32 rows of dwk = dK^T x carry the factor."""
    _, r64, r32, _ = attention
    bad = r32.grads["wk"].copy()
    bad[96:128] *= np.float32(1 + 2e-5)
    assert rel_err(bad, r64.grads["wk"]) < 1e-4
    with pytest.raises(AssertionError, match="per-channel rel"):
        B.check_weight("dwk, head 3 scaled", bad, r64.grads["wk"], r32.grads["wk"])
