"""Box and mask utilities and batched NMS with the call surface of the reference's ultralytics/utils/ops.py
(xywh2xyxy :374-389, xyxy2xywh :357-371, clip_boxes :281-297, scale_boxes :95-125, non_max_suppression :144-278, crop_mask :553-569,
process_mask / process_mask_upsample / process_mask_native :572-642, scale_masks :645-666).  Not here: scale_image (:319-354, a
cv2.resize on the host) and masks2segments (:704-727, cv2.findContours).

non_max_suppression runs the whole batch in three HIP launches (candidate keys -> segmented radix sort -> greedy scan,
csrc/nms.hip) instead of the reference's per-image Python loop around torchvision.ops.nms; there is no CPU fallback."""
import ctypes as C

import torch

from .._C import call
from ..ops import ptr, stream


def xywh2xyxy(x):
    y = torch.empty_like(x)
    dw, dh = x[..., 2] / 2, x[..., 3] / 2
    y[..., 0] = x[..., 0] - dw
    y[..., 1] = x[..., 1] - dh
    y[..., 2] = x[..., 0] + dw
    y[..., 3] = x[..., 1] + dh
    return y


def xyxy2xywh(x):
    y = torch.empty_like(x)
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


def clip_boxes(boxes, shape):
    """in place, like the reference (ops.py:281-297)"""
    boxes[..., 0].clamp_(0, shape[1])
    boxes[..., 1].clamp_(0, shape[0])
    boxes[..., 2].clamp_(0, shape[1])
    boxes[..., 3].clamp_(0, shape[0])
    return boxes


def scale_boxes(img1_shape, boxes, img0_shape, ratio_pad=None, padding=True):
    """Rescale xyxy boxes from the network input shape to the original image shape, in place (ops.py:95-125)."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1), round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1)
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    if padding:
        boxes[..., [0, 2]] -= pad[0]
        boxes[..., [1, 3]] -= pad[1]
    boxes[..., :4] /= gain
    return clip_boxes(boxes, img0_shape)


def clip_coords(coords, shape):
    """in place (reference ops.py:300-316): x to [0, w], y to [0, h]"""
    coords[..., 0].clamp_(0, shape[1])
    coords[..., 1].clamp_(0, shape[0])


def scale_coords(img1_shape, coords, img0_shape, ratio_pad=None, normalize=False, padding=True):
    """Rescale keypoint coordinates [..., >= 2] from the network input shape to the original image shape, in place (reference
    ops.py:669-701: the letterbox pad is not rounded here, unlike scale_boxes), clipped to the image."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    if padding:
        coords[..., 0] -= pad[0]
        coords[..., 1] -= pad[1]
    coords[..., 0] /= gain
    coords[..., 1] /= gain
    clip_coords(coords, img0_shape)
    if normalize:
        coords[..., 0] /= img0_shape[1]
        coords[..., 1] /= img0_shape[0]
    return coords


_ws = {}


def _workspace(key, nbytes, device):
    t = _ws.get(key)
    if t is None or t.numel() < nbytes or t.device != device:
        t = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        _ws[key] = t
    return t


def nms_batched(pred, conf_thres, iou_thres, multi_label, agnostic, max_det, max_nms, max_wh, return_indices=False):
    """pred [B, 4+nc, A] f32 (Detect eval output) -> (out [B,max_det,6], counts [B] int32[, keep_idx [B,max_det] int64]).
    keep_idx = anchor*nc + cls of every kept row (the integer output parity tests compare bit-exactly)."""
    if pred.dtype != torch.float32 or not pred.is_cuda:
        raise RuntimeError("nms_batched expects the f32 device tensor produced by Detect in eval mode")
    pred = pred.contiguous()
    B, no, A = pred.shape
    nc = no - 4
    dev = pred.device
    cap = A * nc if (multi_label and nc > 1) else A
    st = stream()
    keys = torch.empty((2, B, cap), dtype=torch.int64, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    call("dy_nms_candidates", ptr(pred), B, nc, A, float(conf_thres), int(bool(multi_label)), ptr(keys[0]), ptr(counts), cap, st)
    nbytes = C.c_size_t(0)
    call("dy_nms_sort", ptr(keys[0]), ptr(keys[1]), ptr(counts), B, cap, None, C.addressof(nbytes), st)
    ws = _workspace("sort", nbytes.value, dev)
    nbytes = C.c_size_t(ws.numel())
    call("dy_nms_sort", ptr(keys[0]), ptr(keys[1]), ptr(counts), B, cap, ptr(ws), C.addressof(nbytes), st)
    n_eff = min(cap, max_nms)
    boxes_ws = torch.empty((B, n_eff, 4), dtype=torch.float32, device=dev)
    dead_ws = torch.empty((B, n_eff), dtype=torch.uint8, device=dev)
    out = torch.zeros((B, max_det, 6), dtype=torch.float32, device=dev)
    keep = torch.full((B, max_det), -1, dtype=torch.int64, device=dev)
    ocnt = torch.empty(B, dtype=torch.int32, device=dev)
    call("dy_nms_greedy", ptr(pred), ptr(keys[1]), ptr(counts), B, nc, A, cap, float(iou_thres), n_eff, max_det, float(max_wh),
         int(bool(agnostic)), ptr(boxes_ws), ptr(dead_ws), ptr(out), ptr(keep), ptr(ocnt), st)
    return (out, ocnt, keep) if return_indices else (out, ocnt)


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, labels=(),
                        max_det=300, nc=0, max_time_img=0.05, max_nms=30000, max_wh=7680):
    """Reference signature (ops.py:144-156).  Returns a list with one [n,6] tensor (xyxy, conf, cls) per image.
    `max_time_img` is accepted and ignored: the wall-clock break of the reference (:274-276) makes its output depend on
    machine load."""
    assert 0 <= conf_thres <= 1, f"Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0"
    assert 0 <= iou_thres <= 1, f"Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0"
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    if classes is not None or (labels is not None and len(labels)):
        raise NotImplementedError("class filtering / hybrid autolabelling are outside the Dedark-YOLO hot path")
    nc = nc or (prediction.shape[1] - 4)
    nm = prediction.shape[1] - nc - 4
    if nm < 0:
        raise ValueError(f"non_max_suppression: nc={nc} does not fit {prediction.shape[1]} rows")
    if nm == 0:
        out, cnt = nms_batched(prediction, conf_thres, iou_thres, multi_label, agnostic, max_det, max_nms, max_wh)
        cnt = cnt.tolist()
        return [out[i, :cnt[i]] for i in range(len(cnt))]
    # mask coefficients (ops.py:200,234-241): the kernels run on the box / class rows; each kept row's coefficients are gathered by
    # its anchor (keep // nc) and appended -> [n, 6 + nm]
    out, cnt, keep = nms_batched(prediction[:, :4 + nc], conf_thres, iou_thres, multi_label, agnostic, max_det, max_nms, max_wh,
                                 return_indices=True)
    B = prediction.shape[0]
    anchor = (keep.clamp(min=0) // nc)                                          # [B, max_det]
    coef = torch.gather(prediction[:, 4 + nc:], 2, anchor.unsqueeze(1).expand(B, nm, anchor.shape[1]))     # [B, nm, max_det]
    full = torch.cat((out, coef.transpose(1, 2).to(out.dtype)), 2)
    cnt = cnt.tolist()
    return [full[i, :cnt[i]] for i in range(len(cnt))]


def crop_mask(masks, boxes):
    """Zero masks [n, h, w] outside their xyxy boxes [n, 4] (reference ops.py:553-569: columns x1 <= r < x2, rows y1 <= c < y2); f32
    device tensors, returns a new tensor (dy_seg_crop_mask)."""
    if not masks.is_cuda:
        raise RuntimeError("crop_mask needs device tensors (there is no CPU path)")
    n, h, w = masks.shape
    out = masks.float().contiguous().clone()
    bx = boxes.float().contiguous()
    call("dy_seg_crop_mask", ptr(out), ptr(bx), n, h, w, stream())
    return out


MASK_MODES = ("proto", "input", "upsample", "native")


def scale_masks_window(mh, mw, shape, padding=True):
    """(top, left, bottom, right) of the rows / columns of an mh x mw mask that scale_masks keeps before it resizes to `shape`
    (reference ops.py:655-663: gain = old / new, the letterbox padding halved and truncated with int())."""
    gain = min(mh / shape[0], mw / shape[1])
    pad = [mw - shape[1] * gain, mh - shape[0] * gain]
    if padding:
        pad[0] /= 2
        pad[1] /= 2
    top, left = (int(pad[1]), int(pad[0])) if padding else (0, 0)
    bottom, right = int(mh - pad[1]), int(mw - pad[0])
    return top, left, bottom, right


def _det_chunk(n_groups, max_group, oh, ow):
    """Detections one workgroup of dy_seg_mask_upsample walks: as many as keep about 2048 workgroups in flight, at least 8 (the proto
    tile it loads is then shared by that many detections)."""
    tiles = ((oh + 63) // 64) * ((ow + 63) // 64) * n_groups
    nsplit = max(1, min(max_group, -(-2048 // tiles)))
    return max(-(-max_group // nsplit), min(8, max_group))


def process_masks_batched(protos, dets, shape, mode="proto", out_shapes=None):
    """The masks of every image of a batch, uint8.  protos [B, nm, mh, mw] NHWC (any compute dtype), dets: one [n_i, 6+nm] tensor
    per image (non_max_suppression), shape = the network input (h, w) -> one uint8 [n_i, oh, ow] tensor per image.  mode:
      "proto"     process_mask(upsample=False): masks at the proto resolution (dy_seg_mask_decode, one launch);
      "input"     process_mask(upsample=True): crop at the proto resolution, bilinear resize to `shape`;
      "upsample"  process_mask_upsample: bilinear resize to `shape`, then crop;
      "native"    process_mask_native: scale_masks' padding crop, bilinear resize to out_shapes[i] (the original image), crop by the
                  boxes, which the caller has already scaled to that image.
    The three image-resolution modes run dy_seg_mask_upsample: one launch for the images whose output shape agrees (always one for
    "input" / "upsample"), the f32 [n, h, w] planes of the reference never exist."""
    from .. import ops as kops
    if mode not in MASK_MODES:
        raise ValueError(f"process_masks_batched: mode '{mode}' is not one of {MASK_MODES}")
    B, nm, mh, mw = protos.shape
    p = kops.as_nhwc(protos, protos.dtype)
    dev = p.device
    ns = [int(d.shape[0]) for d in dets]
    n = sum(ns)
    if mode == "proto":
        ih, iw = shape
        out = torch.empty((n, mh, mw), dtype=torch.uint8, device=dev)
        if n:
            det = torch.cat([d.float() for d in dets], 0).contiguous()
            img = torch.cat([torch.full((k,), i, dtype=torch.int32, device=dev) for i, k in enumerate(ns)])
            call("dy_seg_mask_decode", ptr(p), kops.ld_of(p), nm, mh, mw, ptr(det), det.shape[1], ptr(img), n, float(mw / iw), float(mh / ih),
                 kops.dt_id(p.dtype), ptr(out), stream())
        return list(out.split(ns, 0))
    if mode == "native":
        if out_shapes is None or len(out_shapes) != len(dets):
            raise ValueError("process_masks_batched(mode='native') needs out_shapes: one original (h, w) per image")
        shapes = [(int(s[0]), int(s[1])) for s in out_shapes]
    else:
        shapes = [(int(shape[0]), int(shape[1]))] * len(dets)
    res = [None] * len(dets)
    for hw in dict.fromkeys(shapes):                      # distinct output shapes, in order of appearance
        oh, ow = hw
        ids = [i for i, s in enumerate(shapes) if s == hw]
        live = [i for i in ids if ns[i]]
        cnt = [ns[i] for i in live]
        out = torch.empty((sum(cnt), oh, ow), dtype=torch.uint8, device=dev)
        if live:
            det = torch.cat([dets[i].float() for i in live], 0).contiguous()
            off = [0]
            for k in cnt:
                off.append(off[-1] + k)
            meta = torch.tensor(off + live, dtype=torch.int32, device=dev)
            if mode == "native":
                top, left, bottom, right = scale_masks_window(mh, mw, hw)
            else:
                top, left, bottom, right = 0, 0, mh, mw
            before = mode == "input"
            call("dy_seg_mask_upsample", ptr(p), kops.ld_of(p), nm, mh, mw, kops.dt_id(p.dtype), ptr(det), det.shape[1], ptr(meta),
                 ptr(meta[len(off):]), len(live), max(cnt), _det_chunk(len(live), max(cnt), oh, ow), int(before),
                 float(mw / shape[1]) if before else 1.0, float(mh / shape[0]) if before else 1.0, top, left, bottom, right, oh, ow,
                 int(not before), ptr(out), stream())
        parts = dict(zip(live, out.split(cnt, 0)))
        for i in ids:
            res[i] = parts[i] if i in parts else out[:0]
    return res


def _one_image(protos, masks_in, bboxes, shape, mode, out_shape=None):
    if not protos.is_cuda:
        raise RuntimeError(f"process_mask ({mode}) needs device tensors (there is no CPU path)")
    n = masks_in.shape[0]
    det = torch.zeros((n, 6 + masks_in.shape[1]), dtype=torch.float32, device=protos.device)
    det[:, :4] = bboxes.float()
    det[:, 6:] = masks_in.float()
    p = protos.float().unsqueeze(0).contiguous(memory_format=torch.channels_last)
    return process_masks_batched(p, [det], shape, mode=mode, out_shapes=None if out_shape is None else [out_shape])[0].float()


def process_mask(protos, masks_in, bboxes, shape, upsample=False):
    """Reference signature (ops.py:593-623): protos [nm, mh, mw], masks_in [n, nm], bboxes [n, 4] xyxy at the input size `shape`
    -> f32 of 0 / 1: sigmoid(c . P) cropped to the box scaled to the proto grid, then [n, mh, mw] thresholded at 0.5
    (upsample=False) or resized bilinearly to [n, *shape] and thresholded (upsample=True, dy_seg_mask_upsample)."""
    return _one_image(protos, masks_in, bboxes, shape, "input" if upsample else "proto")


def process_mask_upsample(protos, masks_in, bboxes, shape):
    """Reference signature (ops.py:572-590): sigmoid(c . P) resized bilinearly to `shape`, cropped to the boxes there, > 0.5
    -> [n, *shape] f32 of 0 / 1."""
    return _one_image(protos, masks_in, bboxes, shape, "upsample")


def process_mask_native(protos, masks_in, bboxes, shape):
    """Reference signature (ops.py:625-642): `shape` is the ORIGINAL image's (h, w) and bboxes are in its pixels; sigmoid(c . P)
    through scale_masks (letterbox padding removed, bilinear resize to `shape`), cropped, > 0.5 -> [n, *shape] f32 of 0 / 1."""
    return _one_image(protos, masks_in, bboxes, shape, "native", out_shape=shape)


def resize_masks(src, shape, m=None, window=None, binary=True):
    """Bilinear resize (align_corners=False) of mask planes on the device (dy_mask_resize).  src: uint8 / f32 planes [m, h, w], or
    with `m` given one index map [h, w] (uint8 / int32; plane k = (map == k + 1), the reference's torch.where(gt == index, 1.0, 0.0),
    segment/val.py:143-145).  window = (top, left, bottom, right) rows / columns of the source to resize (default: all).
    binary -> uint8 [m, *shape] of value > 0.5 (strict, like gt_(0.5)), else the f32 values."""
    if not src.is_cuda:
        raise RuntimeError("resize_masks needs device tensors (there is no CPU path)")
    if m is None:
        if src.dtype not in (torch.uint8, torch.float32):
            src = src.to(torch.float32 if src.is_floating_point() else torch.uint8)
        kind, planes = (0 if src.dtype == torch.uint8 else 3), int(src.shape[0])
    else:
        if src.dim() == 3 and src.shape[0] == 1:
            src = src[0]
        if src.dim() != 2:
            raise ValueError("resize_masks: an index map is [h, w]")
        if src.dtype not in (torch.uint8, torch.int32):
            src = src.to(torch.int32)
        kind, planes = (1 if src.dtype == torch.uint8 else 2), int(m)
    src = src.contiguous()
    h, w = int(src.shape[-2]), int(src.shape[-1])
    top, left, bottom, right = window if window is not None else (0, 0, h, w)
    oh, ow = int(shape[0]), int(shape[1])
    out = torch.empty((planes, oh, ow), dtype=torch.uint8 if binary else torch.float32, device=src.device)
    call("dy_mask_resize", ptr(src), kind, planes, h, w, int(top), int(left), int(bottom), int(right), ptr(out), int(not binary), oh, ow,
         stream())
    return out


def scale_masks(masks, shape, padding=True):
    """Reference signature (ops.py:645-666): masks [N, C, h, w] f32 -> [N, C, *shape] f32: the letterbox padding cropped
    (scale_masks_window), then a bilinear resize (dy_mask_resize)."""
    N, Cn, mh, mw = masks.shape
    win = scale_masks_window(mh, mw, shape, padding)
    out = resize_masks(masks.float().reshape(N * Cn, mh, mw), shape, window=win, binary=False)
    return out.view(N, Cn, int(shape[0]), int(shape[1]))


def mask_iou_binary(gt, pred, overlap, m):
    """IoU [m, n] of uint8 pred masks [n, h, w] against the gt: overlap -> index map [h, w] (label k == k + 1, uint8 / int32),
    else uint8 planes [m, h, w] (dy_seg_mask_iou: integer intersection counts, f32 ratio)."""
    n = pred.shape[0]
    dev = pred.device
    iou = torch.zeros((m, n), dtype=torch.float32, device=dev)
    if n == 0 or m == 0:
        return iou
    hw = pred.shape[1] * pred.shape[2]
    g = gt.contiguous()
    if g.dtype not in (torch.uint8, torch.int32):
        g = g.to(torch.int32 if overlap else torch.uint8)
    work = torch.empty(m * n + n, dtype=torch.int32, device=dev)
    call("dy_seg_mask_iou", ptr(pred.contiguous()), n, ptr(g), int(g.dtype == torch.int32), int(bool(overlap)), m, hw, ptr(work),
         ptr(iou), stream())
    return iou


def mask_iou(mask1, mask2, eps=1e-7):
    """Reference signature (metrics.py:131-147) for BINARY masks: mask1 [N, n] (gt), mask2 [M, n] (predictions) -> IoU [N, M].
    Integer counts on the device; eps is fixed at the reference's 1e-7."""
    if eps != 1e-7:
        raise NotImplementedError("mask_iou: eps is fixed at 1e-7")
    if not mask2.is_cuda:
        raise RuntimeError("mask_iou needs device tensors (there is no CPU path)")
    N, M = mask1.shape[0], mask2.shape[0]
    return mask_iou_binary(mask1.to(torch.uint8).view(N, 1, -1), mask2.to(torch.uint8).view(M, 1, -1), False, N)
