"""Detection criterion on HIP kernels.

Same classes / call signatures as the reference ultralytics/utils/loss.py (v8DetectionLoss :103-193,
RcoveryDetectionLoss :388-416) and ultralytics/utils/tal.py (TaskAlignedAssigner :59-243).  The whole criterion --
target grouping, DFL decode, task-aligned assignment, BCE / CIoU / DFL sums and the gradient wrt the three Detect maps --
runs in libdedark_yolo.so; there are no host syncs on the way (n_max is taken from the CPU-side batch_idx when available).
"""
import ctypes as C
import weakref

import torch

from .. import _C, ops
from .._C import call
from ..nn.modules import Detect
from ..ops import ld_of, ptr, stream

REG_MAX = 16


_n_max_cache = {}          # id(tensor object) -> (weakref to it, _version, bsz, n_max)


def n_max_of(batch_idx, bsz):
    """Largest number of boxes in one image (host value), the reference's `counts.max()` (loss.py:130-132).  batch_idx normally
    lives on the CPU (dataloader), where this is a host-side bincount; DevicePrefetcher / preprocess_batch compute it BEFORE the
    upload and hand it over as batch['n_max'].  A batch_idx that only exists on the device costs one synchronisation per tensor
    OBJECT: the value is remembered for that object alone (weak reference + in-place version counter), so a resident batch that is
    reused stays sync-free while a fresh upload -- which the caching allocator usually puts at the previous batch's address -- can
    never inherit another batch's value (too small an n_max would drop ground-truth boxes in dy_loss_prepare_targets)."""
    if batch_idx.numel() == 0:
        return 0
    if not batch_idx.is_cuda:
        return int(torch.bincount(batch_idx.detach().view(-1).long(), minlength=bsz).max())
    hit = _n_max_cache.get(id(batch_idx))
    if hit is not None and hit[0]() is batch_idx and hit[1] == batch_idx._version and hit[2] == bsz:
        return hit[3]
    n = int(torch.bincount(batch_idx.detach().view(-1).long(), minlength=bsz).max().item())
    if len(_n_max_cache) > 64:
        for k in [k for k, v in _n_max_cache.items() if v[0]() is None]:
            del _n_max_cache[k]
        if len(_n_max_cache) > 64:
            _n_max_cache.clear()
    _n_max_cache[id(batch_idx)] = (weakref.ref(batch_idx), batch_idx._version, bsz, n)
    return n


_n_max_of = n_max_of


class _Assignment:
    __slots__ = ("pred_boxes", "gt", "counts", "target_gt_idx", "fg_mask", "norm", "target_label", "target_box", "n_max")


def assign(maps, strides, nc, batch_idx, cls, bboxes, n_max=None, frozen=None):
    """prepare targets + decode + task-aligned assignment; returns an _Assignment of device tensors.
    `frozen` (test hook, v8DetectionLoss.frozen_assignment): an _Assignment of an earlier call on the same batch whose discrete
    outcome (tal.py:84-132: target_gt_idx, fg_mask, target labels / boxes and the normalised target score) is reused instead of
    running the assigner; the predicted boxes are still decoded from THESE maps."""
    B = maps[0].shape[0]
    dev = maps[0].device
    A = sum(m.shape[2] * m.shape[3] for m in maps)
    st = stream()
    img_h, img_w = maps[0].shape[2] * strides[0], maps[0].shape[3] * strides[0]
    if n_max is None:
        n_max = _n_max_of(batch_idx, B)
    n_t = int(batch_idx.numel())
    f32 = torch.float32
    bi = batch_idx.to(dev, f32).contiguous().view(-1)
    cl = cls.to(dev, f32).contiguous().view(-1)
    bb = bboxes.to(dev, f32).contiguous().view(-1, 4)
    a = _Assignment()
    a.n_max = n_max
    a.gt = torch.empty((B, max(n_max, 1), 5), dtype=f32, device=dev)
    a.counts = torch.empty(B, dtype=torch.int32, device=dev)
    call("dy_loss_prepare_targets", ptr(bi) if n_t else None, ptr(cl) if n_t else None, ptr(bb) if n_t else None, n_t, B,
         max(n_max, 1), float(img_w), float(img_h), ptr(a.gt), ptr(a.counts), st)
    dm = ops.det_maps(maps, strides, nc)
    a.pred_boxes = torch.empty((B, A, 4), dtype=f32, device=dev)
    call("dy_loss_decode", C.byref(dm), ptr(a.pred_boxes), st)
    if frozen is not None:
        if frozen.fg_mask.shape != (B, A) or frozen.n_max != n_max:
            raise ValueError("frozen assignment belongs to another batch / anchor grid")
        a.target_gt_idx, a.fg_mask, a.norm = frozen.target_gt_idx, frozen.fg_mask, frozen.norm
        a.target_label, a.target_box = frozen.target_label, frozen.target_box
        return a
    a.target_gt_idx = torch.empty((B, A), dtype=torch.int32, device=dev)
    a.fg_mask = torch.empty((B, A), dtype=torch.uint8, device=dev)
    a.norm = torch.empty((B, A), dtype=f32, device=dev)
    a.target_label = torch.empty((B, A), dtype=torch.int32, device=dev)
    a.target_box = torch.empty((B, A, 4), dtype=f32, device=dev)
    R = B * max(n_max, 1) * A
    work_f = torch.empty(2 * R + 2 * B * max(n_max, 1), dtype=f32, device=dev)
    work_i = torch.empty(R, dtype=torch.int32, device=dev)
    work_b = torch.empty(R, dtype=torch.uint8, device=dev)
    call("dy_tal_assign", C.byref(dm), ptr(a.pred_boxes), ptr(a.gt), ptr(a.counts), n_max, ptr(work_f), ptr(work_i),
         ptr(work_b), ptr(a.target_gt_idx), ptr(a.fg_mask), ptr(a.norm), ptr(a.target_label), ptr(a.target_box), st)
    return a


def _det_forward(crit, batch, maps, rec=None, lrl=0.0):
    """The detection terms every criterion shares: assignment, dy_loss_fwd, dy_loss_finish (`rec`, `lrl`: the recovery term of the
    detect criterion).  Returns (det, out): det = (maps, strides, assignment, acc) is what _det_backward needs, out the 4 floats
    [loss, box, cls, dfl]."""
    B, dev, st = maps[0].shape[0], maps[0].device, stream()
    strides = Detect.strides_as_floats(crit.head)[:len(maps)]
    a = assign(maps, strides, crit.nc, batch["batch_idx"], batch["cls"], batch["bboxes"], batch.get("n_max"),
               frozen=crit.frozen_assignment)
    dm = ops.det_maps(maps, strides, crit.nc)
    acc = torch.zeros(4, dtype=torch.float64, device=dev)
    call("dy_loss_fwd", C.byref(dm), ptr(a.pred_boxes), ptr(a.fg_mask), ptr(a.norm), ptr(a.target_label), ptr(a.target_box),
         ptr(acc), st)
    if rec is not None:
        rec = rec.detach().to(dev, torch.float32).reshape(-1)
        rec = rec.mean().reshape(1) if rec.numel() > 1 else rec
    out = torch.empty(4, dtype=torch.float32, device=dev)
    call("dy_loss_finish", ptr(acc), ptr(rec), float(crit.hyp.box), float(crit.hyp.cls), float(crit.hyp.dfl), float(lrl), B,
         ptr(out[0:1]), ptr(out[1:4]), st)
    crit.last_assignment = a
    if crit.keep_maps:
        crit.last_maps = maps
    return (maps, strides, a, acc), out


def _det_backward(crit, det, gloss):
    """d(detection terms)/d(maps) with one dy_loss_bwd.  Returns (the per-level gradient views [B, no, h, w], g): g is the
    incoming gradient as one f32 on the device, which the task kernels take as well."""
    maps, strides, a, acc = det
    dev, dt = maps[0].device, maps[0].dtype
    dm = ops.det_maps(maps, strides, crit.nc)
    width = 4 * REG_MAX + ops.round_up(crit.nc, ops.vec_elems(dt))
    dbufs = [ops.empty_nhwc(m.shape[0], width, m.shape[2], m.shape[3], dt, dev) for m in maps]
    arr_p = (C.c_void_p * len(dbufs))(*[d.data_ptr() for d in dbufs])
    arr_l = (C.c_int64 * len(dbufs))(*[ld_of(d) for d in dbufs])
    g = gloss.detach().to(torch.float32).reshape(1).contiguous()
    call("dy_loss_bwd", C.byref(dm), arr_p, arr_l, ptr(a.pred_boxes), ptr(a.fg_mask), ptr(a.norm), ptr(a.target_label),
         ptr(a.target_box), ptr(acc), ptr(g), float(crit.hyp.box), float(crit.hyp.cls), float(crit.hyp.dfl), stream())
    ops.emu_round(*dbufs)
    no = 4 * REG_MAX + crit.nc
    return [d[:, :no] for d in dbufs], g


def _positives(a, batch_idx, with_rows):
    """What the mask and keypoint kernels walk: the gt-row table rows [B, n_max] (where image b's j-th box sits in the batch's
    label arrays; None unless `with_rows`) and the positive anchors pos [B, A] / npos [B] of assignment `a`."""
    (B, A), dev, st = a.fg_mask.shape, a.fg_mask.device, stream()
    rows = None
    if with_rows:
        n_t, n_max = int(batch_idx.numel()), max(a.n_max, 1)
        bif = batch_idx.to(dev, torch.float32).contiguous().view(-1)
        rows = torch.empty((B, n_max), dtype=torch.int32, device=dev)
        call("dy_seg_gt_rows", ptr(bif) if n_t else None, n_t, B, n_max, ptr(rows), st)
    pos = torch.empty((B, A), dtype=torch.int32, device=dev)
    npos = torch.empty(B, dtype=torch.int32, device=dev)
    call("dy_seg_positives", ptr(a.fg_mask), B, A, ptr(pos), ptr(npos), st)
    return rows, pos, npos


class _DetLossFn(torch.autograd.Function):
    """loss, loss_items = f(map0, map1, map2); backward writes d(loss)/d(maps) with one kernel."""

    @staticmethod
    def forward(ctx, crit, batch, n_maps, *maps):
        rec = batch.get("recovery_loss_batch") if crit.use_recovery else None
        ctx.crit = crit
        ctx.det, out = _det_forward(crit, batch, [ops.as_nhwc(m) for m in maps], rec, getattr(crit.hyp, "lrl", 0.0))
        loss, items = out[0], out[1:4]
        ctx.mark_non_differentiable(items)
        return loss, items

    @staticmethod
    def backward(ctx, gloss, _gitems):
        return (None, None, None, *_det_backward(ctx.crit, ctx.det, gloss)[0])


class _DFL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_dist, target):
        n = target.shape[0]
        out = torch.empty((n, 1), dtype=torch.float32, device=pred_dist.device)
        grad = torch.empty_like(pred_dist) if pred_dist.requires_grad else None
        call("dy_dfl_loss", ptr(pred_dist), ptr(target), n, ptr(out), ptr(grad), stream())
        ctx.grad = grad
        return out

    @staticmethod
    def backward(ctx, g):
        return ctx.grad * g.repeat_interleave(4, 0), None


class BboxLoss:
    """The stand-alone pieces of the reference's BboxLoss (ultralytics/utils/loss.py:54-84); the training step itself computes both
    terms inside the fused dy_loss_fwd / dy_loss_bwd kernels with the same device functions (csrc/dy_lossmath.h)."""

    def __init__(self, reg_max, use_dfl=False):
        self.reg_max, self.use_dfl = reg_max, use_dfl

    @staticmethod
    def _df_loss(pred_dist, target):
        """pred_dist [n*4, 16] logits, target [n, 4] in [0, 15) -> [n, 1] (mean over the sides of the two-bin cross entropy)."""
        if pred_dist.device.type != "cuda":
            raise RuntimeError("_df_loss needs device tensors (there is no CPU path)")
        if pred_dist.shape[-1] != REG_MAX or pred_dist.shape[0] != target.numel():
            raise ValueError(f"_df_loss: expected pred_dist [n*4, {REG_MAX}] and target [n, 4]")
        return _DFL.apply(pred_dist.float().contiguous(), target.float().contiguous().detach())


class v8DetectionLoss:
    """reference loss.py:103-193. `model.args` must carry .box/.cls/.dfl (and .lrl for the recovery variant)."""
    use_recovery = False

    def __init__(self, model):
        m = model.model[-1]
        self.hyp = model.args
        self.head = m                        # asked for its host strides every call (Detect.strides_as_floats)
        self.stride = m.stride
        self.nc = m.nc
        self.no = m.no
        self.reg_max = m.reg_max
        self.device = next(model.parameters()).device
        self.use_dfl = m.reg_max > 1
        self.assigner = TaskAlignedAssigner(topk=10, num_classes=self.nc, alpha=0.5, beta=6.0)
        self.last_assignment = None
        self.frozen_assignment = None        # test hooks: reuse an earlier assignment / keep the Detect maps of the last call
        self.keep_maps, self.last_maps = False, None

    def __call__(self, preds, batch):
        feats = preds[1] if isinstance(preds, tuple) else preds
        loss, items = _DetLossFn.apply(self, batch, len(feats), *feats)
        return loss, items


class RcoveryDetectionLoss(v8DetectionLoss):
    """reference loss.py:388-416: adds lrl * recovery_loss_batch to the total and to the cls item."""
    use_recovery = True

    def __init__(self, model):
        super().__init__(model)
        self.recovery_weight = self.hyp.lrl


def _gt_masks(batch, B, dev):
    """batch['masks'] on the device as uint8 or int32 ([B, h, w] index maps or [N, h, w] planes, the reference's collate)."""
    m = batch.get("masks")
    if m is None:
        raise ValueError("segment loss: the batch has no 'masks' (not a segment dataset?)")
    if m.dtype not in (torch.uint8, torch.int32):
        m = m.to(torch.int32) if (m.dtype != torch.bool and m.numel() and float(m.max()) > 255) else m.to(torch.uint8)
    return m.to(dev, non_blocking=True).contiguous()


class _SegLossFn(torch.autograd.Function):
    """(loss, items[box, seg, cls, dfl]) = f(maps..., mc [B, nm, A], proto [B, nm, mh, mw]); backward: one dy_loss_bwd for the maps,
    dy_seg_loss_bwd for mc and proto."""

    @staticmethod
    def forward(ctx, crit, batch, n_maps, *ts):
        dt = ops.get_compute_dtype()
        maps = [ops.as_nhwc(m) for m in ts[:n_maps]]
        mc, proto = ts[n_maps], ops.as_nhwc(ts[n_maps + 1])
        B, dev, st = maps[0].shape[0], maps[0].device, stream()
        A = mc.shape[2]
        mcr = mc.transpose(1, 2)                                         # [B, A, nm] rows
        if (mcr.dtype != dt or mcr.stride(2) != 1 or mcr.stride(1) != mcr.shape[2] or mcr.stride(0) != A * mcr.shape[2]
                or mcr.data_ptr() % 16):
            mcr = mcr.to(dt).contiguous()
        ctx.det, det = _det_forward(crit, batch, maps)
        _, strides, a, _ = ctx.det
        masks = _gt_masks(batch, B, dev)
        n_t, n_max = int(batch["batch_idx"].numel()), max(a.n_max, 1)
        want = f"B={B}" if crit.overlap else f"N={n_t}"          # one index map per image, or one plane per label
        if masks.dim() != 3 or masks.shape[0] != (B if crit.overlap else n_t):
            raise ValueError(f"segment loss: overlap_mask={crit.overlap} needs masks [{want}, h, w], got {tuple(masks.shape)}")
        rows, pos, npos = _positives(a, batch["batch_idx"], with_rows=not crit.overlap)
        d = _C.SegDesc()
        d.mc, d.mc_ld, d.proto, d.proto_ld = mcr.data_ptr(), mcr.stride(1), proto.data_ptr(), ld_of(proto)
        d.B, d.A, d.nm, d.mh, d.mw = B, A, mc.shape[1], proto.shape[2], proto.shape[3]
        d.target_gt_idx, d.fg_mask, d.target_box = ptr(a.target_gt_idx), ptr(a.fg_mask), ptr(a.target_box)
        if masks.numel() == 0:          # no labels at all ([0, h, w] per-instance stack): no positive reads a mask, the kernels need a pointer
            masks = torch.zeros((1, max(masks.shape[1], 1), max(masks.shape[2], 1)), dtype=masks.dtype, device=dev)
        d.masks, d.mask_dtype, d.mask_h, d.mask_w = masks.data_ptr(), int(masks.dtype == torch.int32), masks.shape[1], masks.shape[2]
        d.overlap, d.gt_rows, d.n_max = int(bool(crit.overlap)), ptr(rows), n_max
        d.img_h, d.img_w = maps[0].shape[2] * strides[0], maps[0].shape[3] * strides[0]
        d.pos, d.npos, d.dtype = pos.data_ptr(), npos.data_ptr(), ops.dt_id(mcr.dtype)
        lossp = torch.empty(B * A + B, dtype=torch.float32, device=dev)
        out = torch.empty(5, dtype=torch.float32, device=dev)
        call("dy_seg_loss_fwd", C.byref(d), float(crit.hyp.box), ptr(lossp), ptr(det), ptr(out), st)
        ctx.crit, ctx.desc, ctx.keep = crit, d, (mcr, proto, masks, rows, pos, npos)
        ctx.mc_meta = (mc.shape, mc.dtype)
        loss, items = out[0], out[1:5]
        ctx.mark_non_differentiable(items)
        return loss, items

    @staticmethod
    def backward(ctx, gloss, _gitems):
        crit, st = ctx.crit, stream()
        dmaps, g = _det_backward(crit, ctx.det, gloss)
        mcr, proto = ctx.keep[0], ctx.keep[1]
        (B, A, nm), dev = mcr.shape, mcr.device
        dmc = torch.zeros((B, A, nm), dtype=mcr.dtype, device=dev)      # rows of anchors without a positive stay zero
        dp = ops.empty_nhwc(B, nm, proto.shape[2], proto.shape[3], proto.dtype, dev)
        call("dy_seg_loss_bwd", C.byref(ctx.desc), ptr(g), float(crit.hyp.box), ptr(dmc), nm, ptr(dp), ld_of(dp), st)
        ops.emu_round(dmc, dp)
        shape, mdt = ctx.mc_meta
        dmc_out = dmc.transpose(1, 2) if mdt == dmc.dtype else dmc.transpose(1, 2).to(mdt)
        ctx.keep = None
        return (None, None, None, *dmaps, dmc_out, dp)


class v8SegmentationLoss(v8DetectionLoss):
    """reference loss.py:196-288: the detection terms (dy_loss_fwd / dy_loss_bwd on the HIP assignment) plus the mask term on
    csrc/seg.hip.  Returns (loss.sum() * B, items [box, seg, cls, dfl]); `model.args` carries .box/.cls/.dfl and .overlap_mask
    (True by default, cfg/default.yaml)."""

    def __init__(self, model):
        super().__init__(model)
        self.nm = model.model[-1].nm
        self.overlap = bool(getattr(model.args, "overlap_mask", True))

    def __call__(self, preds, batch):
        feats, mc, proto = preds if len(preds) == 3 else preds[1]
        loss, items = _SegLossFn.apply(self, batch, len(feats), *feats, mc, proto)
        return loss, items


def _gt_keypoints(batch, K, dev):
    """batch['keypoints'] [N, K, 3] (normalised x, y and visibility; the label reader appends the visibility column for ndim 2
    as well, data/utils.py:122-128) as f32 on the device."""
    kp = batch.get("keypoints")
    if kp is None:
        raise ValueError("pose loss: the batch has no 'keypoints' (not a pose dataset?)")
    n = int(batch["batch_idx"].numel())
    if kp.dim() != 3 or kp.shape[0] != n or kp.shape[1] != K or kp.shape[2] != 3:
        raise ValueError(f"pose loss: batch['keypoints'] must be [N={n}, K={K}, 3] (normalised x, y, visibility) for the model's "
                         f"kpt_shape, got {tuple(kp.shape)}")
    return kp.to(dev, torch.float32, non_blocking=True).contiguous()


class _PoseLossFn(torch.autograd.Function):
    """(loss, items[box, pose, kobj, cls, dfl]) = f(maps..., kpt maps...); backward: one dy_loss_bwd for the Detect maps,
    dy_pose_loss_bwd for the keypoint maps (every element of each level's gradient map written)."""

    @staticmethod
    def forward(ctx, crit, batch, n_maps, *ts):
        maps = [ops.as_nhwc(m) for m in ts[:n_maps]]
        kpts = [ops.as_nhwc(k, maps[0].dtype) for k in ts[n_maps:2 * n_maps]]
        B, dev, st = maps[0].shape[0], maps[0].device, stream()
        kp = _gt_keypoints(batch, int(crit.kpt_shape[0]), dev)
        ctx.det, det = _det_forward(crit, batch, maps)
        _, strides, a, _ = ctx.det
        n_t, n_max, A = int(batch["batch_idx"].numel()), max(a.n_max, 1), a.fg_mask.shape[1]
        rows, pos, npos = _positives(a, batch["batch_idx"], with_rows=True)
        d = ops.pose_desc(kpts, strides, crit.kpt_shape)
        d.target_gt_idx, d.fg_mask, d.target_box = ptr(a.target_gt_idx), ptr(a.fg_mask), ptr(a.target_box)
        d.keypoints, d.n_targets = (kp.data_ptr() if n_t else None), n_t
        d.gt_rows, d.n_max = rows.data_ptr(), n_max
        d.img_h, d.img_w = maps[0].shape[2] * strides[0], maps[0].shape[3] * strides[0]
        sigma = crit.sigmas_on(dev)
        d.sigma, d.pos, d.npos = sigma.data_ptr(), pos.data_ptr(), npos.data_ptr()
        work = torch.empty(3 * B * A + 3 * B, dtype=torch.float32, device=dev)
        out = torch.empty(6, dtype=torch.float32, device=dev)
        call("dy_pose_loss_fwd", C.byref(d), float(crit.hyp.pose), float(crit.hyp.kobj), ptr(work), ptr(det), ptr(out), st)
        ctx.crit, ctx.desc, ctx.keep = crit, d, (kpts, kp, rows, pos, npos, sigma, work)
        loss, items = out[0], out[1:6]
        ctx.mark_non_differentiable(items)
        return loss, items

    @staticmethod
    def backward(ctx, gloss, _gitems):
        crit, st = ctx.crit, stream()
        dmaps, g = _det_backward(crit, ctx.det, gloss)
        kpts, work = ctx.keep[0], ctx.keep[-1]
        nk, dt, dev = kpts[0].shape[1], kpts[0].dtype, kpts[0].device
        nk_pad = ops.round_up(nk, ops.vec_elems(dt))
        dks = [ops.empty_nhwc(k.shape[0], nk_pad, k.shape[2], k.shape[3], dt, dev) for k in kpts]
        arr_k = (C.c_void_p * len(dks))(*[k.data_ptr() for k in dks])
        call("dy_pose_loss_bwd", C.byref(ctx.desc), ptr(work), ptr(g), float(crit.hyp.pose), float(crit.hyp.kobj), arr_k, nk_pad, st)
        ops.emu_round(*dks)
        ctx.keep = None
        return (None, None, None, *dmaps, *[k[:, :nk] for k in dks])


class v8PoseLoss(v8DetectionLoss):
    """reference loss.py:292-377 (KeypointLoss :87-99): the detection terms (dy_loss_fwd / dy_loss_bwd on the HIP assignment) plus
    the keypoint location and visibility terms on csrc/pose.hip.  Returns (loss.sum() * B, items [box, pose, kobj, cls, dfl]);
    `model.args` carries .box/.cls/.dfl/.pose/.kobj (cfg/default.yaml).  The OKS sigmas are metrics.oks_sigmas(kpt_shape)."""

    def __init__(self, model):
        super().__init__(model)
        from .metrics import oks_sigmas
        self.kpt_shape = model.model[-1].kpt_shape
        self.sigmas = torch.from_numpy(oks_sigmas(self.kpt_shape)).float()
        self._sigmas_dev = None

    def sigmas_on(self, dev):
        if self._sigmas_dev is None or self._sigmas_dev.device != dev:
            self._sigmas_dev = self.sigmas.to(dev, torch.float32).contiguous()
        return self._sigmas_dev

    def __call__(self, preds, batch):
        feats, pred_kpts = preds if isinstance(preds[0], list) else preds[1]
        if len(pred_kpts) != len(feats):
            raise ValueError(f"pose loss: {len(pred_kpts)} keypoint maps for {len(feats)} Detect levels")
        return _PoseLossFn.apply(self, batch, len(feats), *feats, *pred_kpts)


class _ClsLossFn(torch.autograd.Function):
    """loss = f(logits [B, nc], cls int64 [B]) on dy_cls_xent_fwd; backward: dy_cls_xent_bwd, scaled by the incoming gradient
    on the device (the fp16 loss scale arrives through it)."""

    @staticmethod
    def forward(ctx, logits, cls):
        loss, lse = ops.cls_xent_fwd(logits, cls)
        ctx.keep = (logits, cls, lse)
        return loss.view(())

    @staticmethod
    def backward(ctx, gloss):
        logits, cls, lse = ctx.keep
        ctx.keep = None
        if gloss.dtype != torch.float32 or not gloss.is_cuda:
            gloss = gloss.to(logits.device, torch.float32)
        return ops.cls_xent_bwd(logits, cls, lse, gloss.contiguous()), None


CLS_IGNORE_INDEX = -100      # torch.nn.functional.cross_entropy's default ignore_index


def check_host_class_labels(cls, nc):
    """ValueError for a HOST label tensor with an entry outside [0, nc) other than -100, before anything is launched (torch asserts on
    the device there); device labels are not read back: such a row adds nothing in the kernels."""
    if not cls.is_cuda:
        c = cls.reshape(-1)
        if c.numel() and bool(((c != CLS_IGNORE_INDEX) & ((c < 0) | (c >= nc))).any()):
            raise ValueError(f"classification labels must lie in [0, {nc}) (or be {CLS_IGNORE_INDEX})")


def classify_batch_to_device(batch, device, acc, nc=None):
    """The classify trainer's and validator's batch step (reference classify/train.py:87-91, classify/val.py:32-37): img to the device
    as f32 (a uint8 image becomes f32 / 255 there: dy_preprocess_batch, `acc` its f64 [1] scratch accumulator; a float image passes
    through), cls as a contiguous int64 [B] device tensor; host labels are range-checked when `nc` is given."""
    img = batch["img"].to(device, non_blocking=True)
    if img.dtype == torch.uint8:
        img = img.contiguous()
        out = torch.empty(img.shape, dtype=torch.float32, device=device)
        acc.zero_()
        call("dy_preprocess_batch", ptr(img), ptr(out), None, 1.0, 0, 0, ptr(acc), img.numel(), stream())
        img = out
    elif img.dtype != torch.float32:
        img = img.float()
    batch["img"] = img
    if nc is not None:
        check_host_class_labels(batch["cls"], nc)
    batch["cls"] = batch["cls"].to(device, non_blocking=True).reshape(-1).long().contiguous()
    return batch


class v8ClassificationLoss:
    """reference loss.py:380-385: cross_entropy(preds, batch['cls'], reduction='sum') / 64 -- the constant 64, not the batch size.
    Returns (loss, loss.detach()).  A label of -100 adds nothing; any other label outside [0, nc) raises ValueError when cls
    arrives on the host (torch asserts on the device there); on the device such a row adds nothing and indexes nothing."""

    def __call__(self, preds, batch):
        if isinstance(preds, (list, tuple)):
            preds = preds[1]
        cls = batch["cls"]
        nc = preds.shape[1]
        check_host_class_labels(cls, nc)
        if cls.dtype != torch.int64 or not cls.is_cuda or cls.dim() != 1 or not cls.is_contiguous():
            cls = cls.reshape(-1).to(preds.device, torch.int64).contiguous()
        loss = _ClsLossFn.apply(preds, cls)
        return loss, loss.detach()

class TaskAlignedAssigner:
    """reference tal.py:59-243 (topk must be 10, alpha 0.5, beta 6.0: the constants compiled into the kernel).

    `forward(pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt)` is the reference's own call (tal.py:84-132) on the
    HIP assigner (dy_tal_assign_decoded); the criterion itself goes from the raw Detect maps (`assign_from_maps`, no decoded
    [B,A,nc] score tensor is ever materialised there)."""

    def __init__(self, topk=13, num_classes=80, alpha=1.0, beta=6.0, eps=1e-9):
        if (topk, alpha, beta) != (10, 0.5, 6.0):
            raise NotImplementedError("HIP TaskAlignedAssigner is built for topk=10, alpha=0.5, beta=6.0 (loss.py:120)")
        self.topk, self.num_classes, self.alpha, self.beta, self.eps = topk, num_classes, alpha, beta, eps
        self.bg_idx = num_classes

    def assign_from_maps(self, maps, strides, batch_idx, cls, bboxes, n_max=None):
        return assign([ops.as_nhwc(m) for m in maps], [float(s) for s in strides], self.num_classes, batch_idx, cls, bboxes, n_max)

    @torch.no_grad()
    def forward(self, pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt):
        """Returns (target_labels [B,A] int64, target_bboxes [B,A,4], target_scores [B,A,nc], fg_mask [B,A] bool,
        target_gt_idx [B,A] int64) like tal.py:84-132."""
        ops.require_gpu(pd_scores)
        dev = pd_scores.device
        f32 = torch.float32
        B, A, nc = pd_scores.shape
        n = gt_bboxes.shape[1]
        if n == 0:                                            # tal.py:106-110
            return (torch.full((B, A), float(self.bg_idx), dtype=pd_scores.dtype, device=dev), torch.zeros_like(pd_bboxes),
                    torch.zeros_like(pd_scores), torch.zeros((B, A), dtype=pd_scores.dtype, device=dev),
                    torch.zeros((B, A), dtype=pd_scores.dtype, device=dev))
        sc = pd_scores.detach().to(dev, f32).contiguous()
        bx = pd_bboxes.detach().to(dev, f32).contiguous()
        an = anc_points.detach().to(dev, f32).contiguous()
        mk = mask_gt.to(dev, f32).reshape(B, n, 1)
        gt = torch.cat((gt_labels.to(dev, f32).reshape(B, n, 1), gt_bboxes.to(dev, f32) * mk), 2).contiguous()    # masked rows: zero box
        counts = torch.full((B,), n, dtype=torch.int32, device=dev)
        st = stream()
        tgi = torch.empty((B, A), dtype=torch.int32, device=dev)
        fg = torch.empty((B, A), dtype=torch.uint8, device=dev)
        norm = torch.empty((B, A), dtype=f32, device=dev)
        tl = torch.empty((B, A), dtype=torch.int32, device=dev)
        tb = torch.empty((B, A, 4), dtype=f32, device=dev)
        R = B * n * A
        work_f = torch.empty(2 * R + 2 * B * n, dtype=f32, device=dev)
        work_i = torch.empty(R, dtype=torch.int32, device=dev)
        work_b = torch.empty(R, dtype=torch.uint8, device=dev)
        call("dy_tal_assign_decoded", ptr(sc), ptr(bx), ptr(an), ptr(gt), ptr(counts), B, A, nc, n, ptr(work_f), ptr(work_i), ptr(work_b),
             ptr(tgi), ptr(fg), ptr(norm), ptr(tl), ptr(tb), st)
        fgb = fg.bool()
        labels = tl.long().clamp_(min=0)
        scores = torch.zeros((B, A, nc), dtype=f32, device=dev)
        scores.scatter_(2, labels.clamp(max=nc - 1).unsqueeze(-1), (norm * fgb).unsqueeze(-1))
        return labels, tb, scores, fgb, tgi.long()

    __call__ = forward
