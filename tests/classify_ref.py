"""Float64 statement of the classify kernels (csrc/classify.hip).  TEST INFRASTRUCTURE.

  * pool:     mean over the pixels of an NHWC map; its adjoint spreads dy / HW over them
  * loss:     v8ClassificationLoss = cross_entropy(logits, cls, reduction='sum') / 64 (reference ultralytics/utils/loss.py:380-385),
              written out: sum over the rows with a label in [0, nc) of (logsumexp(z) - z[t]) / 64; gradient (softmax(z) - onehot(t)) / 64
              on those rows, 0 on the others
  * top-k:    the first k entries of a STABLE descending sort (equal values keep ascending index order); NaN ranks below every number,
              -0 equals +0.  torch.argsort (classify/val.py:42) is not stable and leaves ties open; this is the project's rule
  * metrics:  ClassifyMetrics.process / ConfusionMatrix.process_cls_preds (ultralytics/utils/metrics.py:1041-1051, 197-207): top-1 = rank
              0 equals the target, top-5 = any rank does, fitness = their mean, matrix[pred top-1][target] += 1
"""
import numpy as np
import torch

XENT_DIV = 64.0


def gap_fwd(x):
    """x [N, HW, C] -> [N, C] float64"""
    return x.double().mean(1)


def gap_bwd(dy, hw):
    """dy [N, C] -> [N, HW, C] float64"""
    return (dy.double() / hw)[:, None, :].expand(-1, hw, -1).contiguous()


def xent(logits, cls):
    """(loss, d loss / d logits) in float64; logits [B, nc] (any float dtype, used as stored), cls int64 [B]"""
    z = logits.double()
    B, nc = z.shape
    valid = (cls >= 0) & (cls < nc)
    lse = torch.logsumexp(z, 1)
    t = cls.clamp(0, nc - 1)
    per_row = torch.where(valid, lse - z.gather(1, t.view(-1, 1)).view(-1), torch.zeros_like(lse))
    onehot = torch.zeros_like(z).scatter_(1, t.view(-1, 1), 1.0)
    grad = torch.where(valid.view(-1, 1), torch.exp(z - lse.view(-1, 1)) - onehot, torch.zeros_like(z)) / XENT_DIV
    return per_row.sum() / XENT_DIV, grad


def softmax(logits):
    return torch.softmax(logits.double(), 1)


def topk(scores, k):
    """int64 [B, k]: stable descending order, NaN last"""
    s = scores.double().cpu().clone()
    s[s == 0] = 0.0                                       # -0 -> +0
    key = torch.where(torch.isnan(s), torch.full_like(s, -float("inf")), s)
    nan_rank = torch.isnan(s).to(torch.int64)             # numbers (0) before NaN (1), also before a real -inf
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    nr = nan_rank.gather(1, order)
    order = order.gather(1, torch.sort(nr, dim=1, stable=True).indices)
    return order[:, :k]


def metrics(pred, targets, nc):
    """pred int [n, k] (top-k indices), targets int [n] -> dict(top1, top5, fitness, counts [3], confusion [nc, nc])"""
    pred, targets = np.asarray(pred).astype(np.int64), np.asarray(targets).astype(np.int64)
    hit = pred == targets[:, None]
    n, h1, h5 = len(targets), int(hit[:, 0].sum()), int(hit.any(1).sum())
    cm = np.zeros((nc, nc), dtype=np.int64)
    for p, t in zip(pred[:, 0], targets):
        cm[p, t] += 1
    top1, top5 = h1 / n, h5 / n
    return dict(top1=top1, top5=top5, fitness=(top1 + top5) / 2, counts=np.array([n, h1, h5]), confusion=cm)
