"""etch_train_losses (csrc/train_step.hip, etch_amd.losses) against torch fp64 autograd of the literal train.py:81-101 expression on the same inputs:
every loss and every gradient within rel_err <= 1e-4, the bar of the other training kernels."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _parity import RTOL, rel_err

pytestmark = pytest.mark.gpu

W = (2.5, 30.0, 1.0, 50.0)          # direction_w, magnitude_w, confidence_w, part_label_w
SCALE = 10
HEADS = {"direction": ("direction",), "magnitude": ("magnitude",), "confidence": ("confidences", "part_labels")}
KEYS = ("direction_loss", "magnitude_loss", "confidence_loss", "part_label_loss")


def make(B, K, N, M, seed):
    """Head outputs and targets with the inputs that break a careless kernel: a gathered target vector that is exactly zero, logits of +-80 in one
    row, labels 0 and M - 1, a gather index with repeats."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, (B, K))
    if K > 1:
        idx[:, 1] = idx[:, 0]                                        # a repeat for certain
    tv = (rng.standard_normal((B, N, 3)) * 0.05).astype(np.float32)
    tv[0, idx[0, 0]] = 0.0                                           # cosine term 1, zero gradient
    tc = rng.uniform(0, 1, (B, N, 1)).astype(np.float32)
    tl = rng.integers(0, M, (B, N))
    tl[0, idx[0, 0]] = 0
    tl[B - 1, idx[B - 1, K - 1]] = M - 1 if (B, K) != (1, 1) else 0
    heads = {"direction": rng.standard_normal((B, K, 3)).astype(np.float32), "magnitude": rng.uniform(0, 1, (B, K, 1)).astype(np.float32),
             "confidences": rng.uniform(0, 1, (B, K, 1)).astype(np.float32), "part_labels": (rng.standard_normal((B, K, M)) * 3).astype(np.float32)}
    row = np.where(np.arange(M) % 2 == 0, 80.0, -80.0).astype(np.float32)       # an unshifted log-sum-exp overflows fp32
    heads["part_labels"][0, K // 2] = row
    t = {k: torch.from_numpy(v) for k, v in heads.items()}
    return t, torch.from_numpy(idx), torch.from_numpy(tv), torch.from_numpy(tc), torch.from_numpy(tl)


def reference(heads, idx, tv, tc, tl, drop_rows=None):
    """train.py:81-101 in fp64 on the CPU (weights W, scale_magnitude SCALE); returns ({key: loss}, {head: gradient of the sum})."""
    h = {k: v.double().requires_grad_() for k, v in heads.items()}
    sel = idx.unsqueeze(-1).expand(-1, -1, 3)
    vectors, confidences, labels = tv.double(), tc.double(), tl
    losses = {}
    if "direction" in h:
        vectors_k = torch.gather(vectors, 1, sel)
        losses["direction_loss"] = (1 - F.cosine_similarity(vectors_k, h["direction"], dim=-1)).mean() * W[0]
    if "magnitude" in h:
        vectors_k = torch.gather(vectors, 1, sel)
        losses["magnitude_loss"] = F.mse_loss(torch.norm(vectors_k, dim=-1, keepdim=True) * SCALE, h["magnitude"]) * W[1]
    if "part_labels" in h:
        labels_k = torch.gather(labels, 1, sel[:, :, 0])
        confidences_k = torch.gather(confidences, 1, sel[:, :, 0].unsqueeze(-1))
        losses["confidence_loss"] = F.mse_loss(h["confidences"], confidences_k) * W[2]
        if drop_rows is None:
            losses["part_label_loss"] = F.cross_entropy(h["part_labels"].permute(0, 2, 1).contiguous(), labels_k) * W[3]
        else:       # rows with a label out of range contribute nothing; the mean stays over all B K rows
            ce = F.cross_entropy(h["part_labels"].permute(0, 2, 1).contiguous(), labels_k.clamp(0, h["part_labels"].shape[2] - 1), reduction="none")
            losses["part_label_loss"] = (ce * (~drop_rows)).sum() / ce.numel() * W[3]
    sum(losses.values()).backward()
    return {k: float(v.detach()) for k, v in losses.items()}, {k: v.grad for k, v in h.items()}


def gpu(heads, idx, tv, tc, tl, upstream=None, index3=False):
    from etch_amd import losses as L
    h = {k: v.cuda().requires_grad_() for k, v in heads.items()}
    status = torch.zeros((1,), dtype=torch.int32, device="cuda")
    index = idx.cuda()
    if index3:
        index = index.unsqueeze(-1).expand(-1, -1, 3)
    total, parts = L.train_losses(h, index, tv.cuda(), tc.cuda(), tl.cuda(), W, SCALE, status=status)
    assert not parts.requires_grad and total.requires_grad
    (total if upstream is None else total * upstream).backward()
    return parts.cpu(), {k: v.grad.cpu() for k, v in h.items()}, int(status.item())


def check(heads, idx, tv, tc, tl, **kw):
    ref_l, ref_g = reference(heads, idx, tv, tc, tl)
    parts, grads, status = gpu(heads, idx, tv, tc, tl, **kw)
    assert status == 0
    for i, k in enumerate(KEYS):
        if k in ref_l:
            e = abs(float(parts[i]) - ref_l[k]) / abs(ref_l[k])
            print(k, float(parts[i]), ref_l[k], e)
            assert e <= RTOL, (k, e)
        else:
            assert float(parts[i]) == 0.0
    e = abs(float(parts[4]) - sum(ref_l.values())) / sum(ref_l.values())
    assert e <= RTOL, ("total", e)
    for k in heads:
        e = rel_err(grads[k].numpy(), ref_g[k].numpy())
        print("d", k, e)
        assert e <= RTOL, (k, e)
    return parts, grads


# M below a wave, the real one, above two per lane; B K = 1; and more rows than the grid has waves (a wave then loops over rows)
@pytest.mark.parametrize("B,K,N,M", [(2, 257, 300, 5), (2, 257, 300, 86), (2, 257, 300, 130), (1, 1, 4, 86), (2, 1031, 1100, 86)])
def test_losses_and_gradients_match_fp64_autograd(B, K, N, M):
    heads, idx, tv, tc, tl = make(B, K, N, M, seed=M + K)
    parts, grads = check(heads, idx, tv, tc, tl, index3=True)
    # the zero target vector: cosine term exactly 1 (checked through the mean above), gradient exactly zero
    assert torch.all(grads["direction"][0, 0] == 0)
    assert torch.isfinite(grads["part_labels"]).all()


@pytest.mark.parametrize("items", [c for n in (1, 2, 3) for c in itertools.combinations(sorted(HEADS), n)])
def test_every_subset_of_pred_items(items):
    heads, idx, tv, tc, tl = make(2, 67, 80, 86, seed=3)
    sub = {k: heads[k] for it in items for k in HEADS[it]}
    check(sub, idx, tv, tc, tl)


def test_upstream_gradient_scales_and_two_calls_are_bitwise_equal():
    heads, idx, tv, tc, tl = make(2, 257, 300, 86, seed=9)
    p1, g1, _ = gpu(heads, idx, tv, tc, tl)
    p2, g2, _ = gpu(heads, idx, tv, tc, tl)
    p3, g3, _ = gpu(heads, idx, tv, tc, tl, upstream=3.0)
    assert torch.equal(p1, p2) and torch.equal(p1, p3)
    for k in heads:
        assert torch.equal(g1[k], g2[k]), k
        assert torch.equal(g3[k], g1[k] * 3.0), k
    from etch_amd import autograd as A
    assert int(A.reduce_counters(torch.device("cuda", torch.cuda.current_device())).abs().sum()) == 0


def test_out_of_range_label_sets_the_flag_and_leaves_the_other_rows_alone():
    from etch_amd import ops
    B, K, N, M = 2, 257, 300, 86
    heads, idx, tv, tc, tl = make(B, K, N, M, seed=21)
    p0, g0, s0 = gpu(heads, idx, tv, tc, tl)
    assert s0 == 0
    bad = tl.clone()
    targets = [(0, int(idx[0, 5])), (1, int(idx[1, 100]))]
    bad[targets[0]] = M
    bad[targets[1]] = -1
    drop = torch.zeros((B, K), dtype=torch.bool)
    for b, n in targets:
        drop[b] |= idx[b] == n                                        # every row that gathers the bad label (the index has repeats)
    p1, g1, s1 = gpu(heads, idx, tv, tc, bad)
    assert s1 == ops.TRAIN_STATUS_BAD_LABEL
    assert torch.equal(p1[:3], p0[:3])
    for k in ("direction", "magnitude", "confidences"):
        assert torch.equal(g1[k], g0[k]), k
    assert torch.equal(g1["part_labels"][~drop], g0["part_labels"][~drop])
    assert torch.all(g1["part_labels"][drop] == 0)
    ref_l, _ = reference(heads, idx, tv, tc, bad, drop_rows=drop)
    assert abs(float(p1[3]) - ref_l["part_label_loss"]) <= RTOL * abs(ref_l["part_label_loss"])


def test_nan_total_sets_the_status_word():
    from etch_amd import ops
    heads, idx, tv, tc, tl = make(1, 9, 12, 5, seed=1)
    tv[0, int(idx[0, 3]), 1] = float("nan")
    parts, _, status = gpu(heads, idx, tv, tc, tl)
    assert status == ops.TRAIN_STATUS_NAN and np.isnan(float(parts[4]))
