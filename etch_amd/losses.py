"""The four training losses of train.py:81-101 and their gradients in one launch (csrc/train_step.hip: etch_train_losses).

    total, parts = train_losses(results, selected_indexs, vectors, confidences, labels, weights=(direction_w, magnitude_w, confidence_w,
                                part_label_w), scale_magnitude=10, status=optimizer.status)
    total.backward()

`results` is the model's dict: whichever of "direction", "magnitude", "confidences" + "part_labels" it holds are the losses computed (train.py's
PRED_ITEMS).  `parts` is a (5,) device tensor -- direction, magnitude, confidence, part-label loss (weighted; 0 for an absent head) and the total --
with no autograd history; KEYS names its first four entries as train.py keys its `losses` dict.  Targets receive no gradient.
"""
import torch

from . import autograd as A
from . import ops

KEYS = ("direction_loss", "magnitude_loss", "confidence_loss", "part_label_loss")


class TrainLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, index, t_vectors, t_confidences, t_labels, weights, scale_magnitude, status, direction, magnitude, confidences, part_labels):
        heads = [None if h is None else h.detach().contiguous() for h in (direction, magnitude, confidences, part_labels)]
        first = next(h for h in heads if h is not None)
        losses, status, grads = ops.train_losses(*heads, t_vectors, t_confidences, t_labels, index, weights, scale_magnitude,
                                                 A.reduce_counters(first.device), status)
        ctx.grads = grads
        total = losses[4].clone()
        ctx.mark_non_differentiable(losses)
        return total, losses

    @staticmethod
    def backward(ctx, g_total, _g_parts):
        grads, ctx.grads = ctx.grads, None
        if grads is None:
            raise RuntimeError("TrainLossFunction: backward runs once (the stashed gradients are released by it)")
        return (None,) * 7 + tuple(None if g is None else g * g_total for g in grads)


def train_losses(results, selected_indexs, vectors, confidences, labels, weights=(1.0, 1.0, 1.0, 1.0), scale_magnitude=10, status=None):
    """See the module docstring.  selected_indexs: the model's (B,K,3) index (its [:, :, 0] is applied to every target, train.py:83-98) or a (B,K)
    index; status: an int32 device tensor whose [0] receives the ETCH_TRAIN_STATUS_* bits (GuardedAdam.status), or None."""
    index = selected_indexs[:, :, 0] if selected_indexs.dim() == 3 else selected_indexs
    index = index.contiguous()
    conf_head = "confidences" in results or "part_labels" in results
    if conf_head and not ("confidences" in results and "part_labels" in results):
        raise ValueError("the confidence head gives both `confidences` and `part_labels`")
    return TrainLossFunction.apply(index, vectors.contiguous() if vectors is not None else None,
                                   confidences.contiguous() if confidences is not None else None,
                                   labels.contiguous() if labels is not None else None, tuple(float(w) for w in weights), float(scale_magnitude),
                                   status, results.get("direction"), results.get("magnitude"), results.get("confidences"), results.get("part_labels"))


def reference_losses(results, selected_indexs, vectors, confidences, labels, weights=(1.0, 1.0, 1.0, 1.0), scale_magnitude=10):
    """train.py:81-101 written out with torch ops (`--reference_step`, and what the tests compare the kernel with).  Returns the dict train.py builds."""
    F = torch.nn.functional
    direction_w, magnitude_w, confidence_w, part_label_w = weights
    losses = {}
    if "direction" in results:
        vectors_k = torch.gather(vectors, 1, selected_indexs)
        losses["direction_loss"] = (1 - F.cosine_similarity(vectors_k, results["direction"], dim=-1)).mean() * direction_w
    if "magnitude" in results:
        vectors_k = torch.gather(vectors, 1, selected_indexs)
        vector_norms = torch.norm(vectors_k, dim=-1, keepdim=True)
        losses["magnitude_loss"] = F.mse_loss(vector_norms * scale_magnitude, results["magnitude"]) * magnitude_w
    if "part_labels" in results:
        labels_k = torch.gather(labels, 1, selected_indexs[:, :, 0])
        confidences_k = torch.gather(confidences, 1, selected_indexs[:, :, 0].unsqueeze(-1))
        losses["confidence_loss"] = F.mse_loss(results["confidences"], confidences_k) * confidence_w
        losses["part_label_loss"] = F.cross_entropy(results["part_labels"].permute(0, 2, 1).contiguous(), labels_k) * part_label_w
    return losses
