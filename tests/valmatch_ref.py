"""Plain f32 numpy statement of what csrc/valmatch.hip computes, for the tests of the validation matching: the box scaling of
utils/ops.scale_boxes, the IoU of utils/metrics.box_iou, and the two matching rules in the form the kernel evaluates them (one pass per
detection over the labels, then one pass over the detections in front of it / one pass per label over the detections).  Also the
reader of tests/golden/g27_valmatch.npz."""
import numpy as np

F = np.float32


def scale_record(img1_shape, img0_shape, ratio_pad=None):
    """(gain, pad_x, pad_y, h0, w0) as f32, by scale_boxes' rule"""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1), round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1)
    else:
        gain, pad = ratio_pad[0][0], ratio_pad[1]
    return np.array([gain, pad[0], pad[1], img0_shape[0], img0_shape[1]], dtype=F)


def scale_xyxy(boxes, rec):
    """input-space xyxy [n, 4] f32 -> native space: (v - pad) / gain, clamped to the original image"""
    b = np.asarray(boxes, dtype=F)
    gain, px, py, h0, w0 = (F(v) for v in rec)
    pad = np.array([px, py, px, py], dtype=F)
    hi = np.array([w0, h0, w0, h0], dtype=F)
    out = (b - pad) / gain
    assert out.dtype == F
    return np.minimum(np.maximum(out, F(0)), hi)


def label_boxes(xywh, H, W, rec):
    """normalised xywh [m, 4] f32 -> native-space xyxy: xywh2xyxy, x (W, H, W, H), scale_xyxy"""
    q = np.asarray(xywh, dtype=F).reshape(-1, 4)
    dw, dh = q[:, 2] / F(2), q[:, 3] / F(2)
    xyxy = np.stack([q[:, 0] - dw, q[:, 1] - dh, q[:, 0] + dw, q[:, 1] + dh], 1) * np.array([W, H, W, H], dtype=F)
    return scale_xyxy(xyxy, rec)


def box_iou(lab, det):
    """[M, N] f32: inter / (a1 + a2 - inter + 1e-7)"""
    lab, det = np.asarray(lab, dtype=F).reshape(-1, 4), np.asarray(det, dtype=F).reshape(-1, 4)
    lo = np.maximum(lab[:, None, :2], det[None, :, :2])
    hi = np.minimum(lab[:, None, 2:], det[None, :, 2:])
    wh = np.maximum(hi - lo, F(0))
    inter = wh[..., 0] * wh[..., 1]
    a1 = ((lab[:, 2] - lab[:, 0]) * (lab[:, 3] - lab[:, 1]))[:, None]
    a2 = ((det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1]))[None, :]
    out = inter / (a1 + a2 - inter + F(1e-7))
    assert out.dtype == F
    return out


def match(iou, lcls, dcls, iouv):
    """bool [N, T] the way the kernel gets it: a detection's label is its best one of equal class (last maximum), its mask the
    thresholds that IoU reaches; it then loses the thresholds taken by a detection of lower index with the same label."""
    iou, iouv = np.asarray(iou, dtype=F), np.asarray(iouv, dtype=F)
    M, N = iou.shape
    label, mask = np.full(N, -1), np.zeros((N, len(iouv)), dtype=bool)
    for j in range(N):
        best = F(-1)
        for i in range(M):
            if lcls[i] == dcls[j] and iou[i, j] >= best:
                best, label[j] = iou[i, j], i
        if label[j] >= 0:
            mask[j] = best >= iouv
    correct = mask.copy()
    for j in range(N):
        for j2 in range(j):
            if label[j2] == label[j] and label[j] >= 0:
                correct[j] &= ~mask[j2]
    return correct


def confusion(matrix, iou, conf, lcls, dcls, conf_thres=0.25, iou_thres=0.45):
    """the kernel's confusion pass on an int matrix [nc + 1, nc + 1], in place"""
    nc = matrix.shape[0] - 1
    iou = np.asarray(iou, dtype=F)
    M, N = iou.shape
    chosen, civ = np.full(N, -1), np.full(N, F(iou_thres))
    for j in range(N):
        if F(conf[j]) > F(conf_thres):
            for i in range(M):
                if iou[i, j] > civ[j]:
                    civ[j], chosen[j] = iou[i, j], i
    matched, any_match = np.zeros(N, dtype=bool), False
    for i in range(M):
        w = -1
        for j in range(N):
            if chosen[j] == i and (w < 0 or civ[j] > civ[w]):
                w = j
        if w >= 0:
            matched[w], any_match = True, True
            matrix[int(dcls[w]), int(lcls[i])] += 1
        else:
            matrix[nc, int(lcls[i])] += 1
    if any_match:
        for j in range(N):
            if not matched[j] and F(conf[j]) > F(conf_thres):
                matrix[int(dcls[j]), nc] += 1
    return matrix


def fixture_sets(g):
    """g27_valmatch.npz (util.gold) -> one dict per set: nc, H, W, batch (the validator's batch dict, host tensors), preds (list of
    [n, 6]), images (per image: predn [n, 6], labelsn [m, 5] as the reference scaled them, ori_shape, ratio_pad), and the reference's
    results (correct / conf / pcls / tcls rows, matrix, tp, fp, txt, txt_conf, json)."""
    import torch
    out = []
    for k in range(int(g["n_sets"])):
        p = f"s{k}_"
        counts = [int(v) for v in g[p + "counts"]]
        preds = list(g[p + "preds"].split(counts, 0))
        B = len(counts)
        ori = [tuple(int(v) for v in o) for o in g[p + "ori_shape"].tolist()]
        rp = [((r[0][0], r[0][1]), (r[1][0], r[1][1])) for r in g[p + "ratio_pad"].tolist()] if bool(g[p + "has_ratio_pad"]) else None
        H, W = int(g[p + "H"]), int(g[p + "W"])
        batch = dict(img=torch.zeros(B, 3, H, W), batch_idx=g[p + "batch_idx"], cls=g[p + "cls"], bboxes=g[p + "bboxes"], ori_shape=ori,
                     im_file=[str(f) for f in g[p + "files"]])
        if rp is not None:
            batch["ratio_pad"] = rp
        images = [dict(predn=g[f"{p}i{b}_predn"], labelsn=g[f"{p}i{b}_labelsn"], ori_shape=ori[b], ratio_pad=None if rp is None else rp[b],
                       cls=g[p + "cls"][g[p + "batch_idx"] == b].view(-1), bboxes=g[p + "bboxes"][g[p + "batch_idx"] == b])
                  for b in range(B)]
        out.append(dict(nc=int(g[p + "nc"]), H=H, W=W, batch=batch, preds=preds, images=images, seen=int(g[p + "seen"]),
                        **{key: g[p + key] for key in ("correct", "conf", "pcls", "tcls", "matrix", "tp", "fp", "txt", "txt_conf", "json")}))
    return out
