"""Test-time augmentation merge: `merge_aug_bboxes_3d` (mmdet3d/core/post_processing/merge_augs.py:7-91) for one scene, and the
front-end of csrc_post/merge.hip (`merge_sorted_segments`), the stable k-way merge the batched route
(Fcaf3DNeckWithHead.get_bboxes_aug) runs twice per batch.

Where the reference leaves a gap ("Test-time augmentation"): the merge NMS is FCAF3D's own BEV NMS (csrc/nms.hip, the
pcdet_nms semantics the first stage uses), rotated exactly when the boxes carry a yaw unless `test_cfg.use_rotate_nms` says
otherwise; `nms_thr` defaults to `iou_thr`, `max_num` to no cap; every sort is stable.

Box voting (no reference counterpart): with `test_cfg.vote_thr` set, every box the merge NMS keeps becomes the
score-weighted mean of the class's candidates whose BEV IoU with it reaches vote_thr.  `vote_boxes` states the rule per scene in
torch; `vote_segments` is the front-end of csrc_post/vote.hip, which the batched route runs between its NMS and its second merge."""
import math

import numpy as np
import torch

from . import _lib as L
from .boxes import bbox3d2result, bbox3d_mapping_back
from .nms import nms_bev

MERGE_TO_BOTTOM = 1          # include/fcaf3d_hip.h FC_MERGE_TO_BOTTOM
MERGE_WITH_YAW = 2           # FC_MERGE_WITH_YAW
XF_FLIP_H = 1 << 32          # FC_MERGE_XF_FLIP_H
XF_FLIP_V = 1 << 33          # FC_MERGE_XF_FLIP_V
VOTE_ROTATED = 1             # FC_VOTE_ROTATED
VOTE_WITH_YAW = 2            # FC_VOTE_WITH_YAW
PI32 = float(np.float32(math.pi))


def aug_params(meta):
    """(pcd_scale_factor, pcd_horizontal_flip, pcd_vertical_flip) of one augmented scene's meta; the reference passes
    img_metas[a] as a one-scene list.  A meta without the keys: scale 1, no flip."""
    if isinstance(meta, (list, tuple)):
        meta = meta[0]
    return (float(meta.get('pcd_scale_factor', 1.0)), bool(meta.get('pcd_horizontal_flip', False)),
            bool(meta.get('pcd_vertical_flip', False)))


def merge_cfg(test_cfg, with_yaw):
    """(nms_thr, use_rotate_nms, max_num or None) — FCAF3D's test_cfg holds only nms_pre / iou_thr / score_thr"""
    nms_thr = float(test_cfg.get('nms_thr', test_cfg['iou_thr']))
    rotated = bool(test_cfg.get('use_rotate_nms', with_yaw))
    max_num = test_cfg.get('max_num', None)
    return nms_thr, rotated, (None if max_num is None or max_num < 0 else int(max_num))


def vote_cfg(test_cfg):
    """test_cfg.vote_thr: None or absent = no box voting (the merge as the reference does it); else the IoU in (0, 1] from which a
    candidate votes for a kept box"""
    v = test_cfg.get('vote_thr', None)
    if v is None:
        return None
    v = float(v)
    if not 0.0 < v <= 1.0:
        raise ValueError(f'test_cfg.vote_thr must lie in (0, 1], got {v}')
    return v


def vote_boxes(boxes, scores, keep, vote_thr, rotated, with_yaw, iou=None, return_members=False):
    """Box voting for one NMS segment.  boxes (N, 7) (or (N, 6): yaw 0) and scores (N,) in the order the NMS saw them (descending
    score), keep: the kept positions.  For every kept i the members are i itself and every j with iou(i, j) >= vote_thr, where
    iou = nms.boxes_iou_bev(boxes[keep], boxes, rotated) (fp32; pass `iou` (len(keep), N) to supply the values: CPU tests), a NaN
    is no member; columns 0..5 of row i become fp32(sum_j score_j box_j / sum_j score_j), both sums in float64 over ascending j.
    with_yaw: d = remainder(yaw_j - yaw_i, fp32 pi) (IEEE remainder, |d| <= pi / 2); |d| > pi / 4: j contributes (l_j, w_j) for
    (w_j, l_j).  A weight sum that is not positive and finite leaves row i as it is.  Returns the whole table, every other row
    and the yaw column unchanged (and the member counts (len(keep),) int32 with return_members)."""
    keep = keep.long()
    K, N = len(keep), boxes.shape[0]
    out = boxes.clone()
    if K == 0:
        return (out, torch.zeros(0, dtype=torch.int32, device=boxes.device)) if return_members else out
    if iou is None:
        from .nms import boxes_iou_bev
        b7 = boxes if boxes.shape[1] == 7 else torch.cat((boxes, torch.zeros_like(boxes[:, :1])), 1)
        iou = boxes_iou_bev(b7[keep], b7, rotated=rotated)
    assert iou.shape == (K, N)
    rows = torch.arange(K, device=boxes.device)
    mem = iou.float() >= torch.tensor(vote_thr, dtype=torch.float32, device=boxes.device)
    mem[rows, keep] = True
    cnt = mem.sum(1)
    # member lists by ascending j, padded: the stable sort puts every member (key 0) before every non-member (key 1)
    idx = torch.sort((~mem).to(torch.uint8), dim=1, stable=True).indices[:, :int(cnt.max())]
    valid = torch.arange(idx.shape[1], device=boxes.device)[None, :] < cnt[:, None]
    b64, s64 = boxes[:, :6].double(), scores.double()
    swap = None
    if with_yaw and boxes.shape[1] == 7:
        d = (boxes[idx, 6] - boxes[keep, 6][:, None]).double()              # the fp32 difference
        d = d - torch.round(d / PI32) * PI32                                # IEEE remainder: exact in float64
        swap = d.abs() > float(np.float32(PI32) * np.float32(0.25))
    acc = torch.zeros((K, 6), dtype=torch.float64, device=boxes.device)
    den = torch.zeros(K, dtype=torch.float64, device=boxes.device)
    for m in range(idx.shape[1]):                                           # one member per pass: the order of every sum is ascending j
        j, ok = idx[:, m], valid[:, m]
        v = b64[j]
        if swap is not None:
            v = torch.where(swap[:, m, None], v[:, [0, 1, 2, 4, 3, 5]], v)
        w = s64[j]
        acc = torch.where(ok[:, None], acc + w[:, None] * v, acc)
        den = torch.where(ok, den + w, den)
    good = (den > 0) & torch.isfinite(den)
    res = (acc / den[:, None]).float()
    out[keep, :6] = torch.where(good[:, None], res, boxes[keep, :6])
    return (out, cnt.to(torch.int32)) if return_members else out


def vote_segments(boxes, scores, counts, keep, keep_counts, vote_thr, rotated, with_yaw, members=False):
    """csrc_post/vote.hip fc_vote_boxes on the tables of the merge NMS: boxes (nseg, stride, 7), scores (nseg, stride), counts
    (nseg,) int32, keep (nseg, keep_stride) int32, keep_counts (nseg,) int32, all on the device.  Returns the voted table (rows at
    or past a segment's count are undefined) and, with members=True, the member count per kept position (nseg, keep_stride)."""
    nseg, stride, seven = boxes.shape
    assert seven == 7 and scores.shape == (nseg, stride) and keep.shape[0] == nseg and keep.dtype == counts.dtype == torch.int32
    keep_stride = keep.shape[1]
    out = torch.empty_like(boxes)
    mem = torch.zeros((nseg, keep_stride), dtype=torch.int32, device=boxes.device) if members else None
    flags = (VOTE_ROTATED if rotated else 0) | (VOTE_WITH_YAW if with_yaw else 0)
    L.call('fc_vote_boxes', L.ptr(boxes), L.ptr(scores), L.ptr(counts), nseg, stride, stride, L.ptr(keep), L.ptr(keep_counts),
           keep_stride, keep_stride, float(vote_thr), flags, L.ptr(out), L.ptr(mem), L.stream())
    return (out, mem) if members else out


def transform_word(scale_factor, flip_h, flip_v):
    """word [3] of a merge segment descriptor: the fp32 bit pattern of 1 / scale_factor (reciprocal in double, as `tensor *= 1 / s`
    does) and the flip bits"""
    bits = int(np.array(1.0 / scale_factor, dtype=np.float32).view(np.uint32))
    return bits | (XF_FLIP_H if flip_h else 0) | (XF_FLIP_V if flip_v else 0)


def merge_sorted_segments(desc, K, counts, scores, boxes, *, max_total, stride_out, keep=None, keep_stride=0, order=None,
                          order_stride=0, score_stride=1, flags=0, cap=-1):
    """csrc_post/merge.hip fc_merge_sorted_segments: output segment o = stable descending merge of the input segments o*K .. o*K+K-1
    (desc: (nseg_out * K, 4) int64 on the device; see include/fcaf3d_hip.h).  Returns (boxes (nseg_out, stride_out, 7), scores
    (nseg_out, stride_out), src (nseg_out, stride_out, 2) int32 = (k, position), counts (nseg_out,) int32); rows past a segment's
    count are undefined."""
    assert desc.dtype == torch.int64 and desc.shape[1] == 4 and desc.shape[0] % K == 0
    nseg_out = desc.shape[0] // K
    dev = scores.device
    stride_out = max(1, int(stride_out))
    out_boxes = torch.empty((nseg_out, stride_out, 7), dtype=torch.float32, device=dev)
    out_scores = torch.empty((nseg_out, stride_out), dtype=torch.float32, device=dev)
    out_src = torch.empty((nseg_out, stride_out, 2), dtype=torch.int32, device=dev)
    out_count = torch.empty(nseg_out, dtype=torch.int32, device=dev)
    if nseg_out == 0:
        return out_boxes, out_scores, out_src, out_count
    ws = L.workspace(L.query('fc_merge_sorted_segments_ws_bytes', nseg_out, int(max_total)), dev)
    L.call('fc_merge_sorted_segments', L.ptr(desc), nseg_out, K, L.ptr(counts), L.ptr(keep), int(keep_stride), L.ptr(order),
           int(order_stride), L.ptr(scores), int(score_stride), L.ptr(boxes), int(flags), int(max_total), int(cap),
           L.ptr(out_boxes), L.ptr(out_scores), L.ptr(out_src), L.ptr(out_count), stride_out, L.ptr(ws), ws.numel(), L.stream())
    return out_boxes, out_scores, out_src, out_count


def merge_aug_single(aug_results, img_metas, test_cfg):
    """merge_aug_bboxes_3d on the device: (boxes, scores, labels) with the tensors where the NMS ran (cuda)."""
    assert len(aug_results) == len(img_metas), \
        f'"aug_results" should have the same length as "img_metas", got {len(aug_results)} and {len(img_metas)}'
    rb, rs, rl = [], [], []
    dev = None
    for res, meta in zip(aug_results, img_metas):
        s, h, v = aug_params(meta)
        b = res['boxes_3d']
        dev = dev or (b.tensor.device if b.tensor.is_cuda else torch.device('cuda', torch.cuda.current_device()))
        rb.append(bbox3d_mapping_back(b.to(dev), s, h, v))
        rs.append(res['scores_3d'].to(dev))
        rl.append(res['labels_3d'].to(dev).long())
    boxes = rb[0].cat(rb)
    scores, labels = torch.cat(rs), torch.cat(rl)
    if len(labels) == 0:
        return boxes, scores, labels
    nms_thr, rotated, max_num = merge_cfg(test_cfg, boxes.with_yaw)
    vote_thr = vote_cfg(test_cfg)
    mb, ms, ml = [], [], []
    for c in range(int(labels.max()) + 1):
        ids = labels == c
        t, sc = boxes.tensor[ids], scores[ids]
        if len(sc) == 0:
            continue
        keep = nms_bev(t, sc, nms_thr, rotated=rotated, stable=True)
        if vote_thr is not None:
            # the candidates in the order the NMS saw them (stable descending score): the order of the sums; counts, scores, labels
            # and order stay those of the un-voted merge
            o = sc.sort(dim=0, descending=True, stable=True)[1]
            pos = torch.empty_like(o)
            pos[o] = torch.arange(len(o), device=o.device)
            voted = vote_boxes(t[o], sc[o], pos[keep], vote_thr, rotated, boxes.with_yaw)
            t = voted[pos]
        mb.append(t[keep]); ms.append(sc[keep]); ml.append(labels[ids][keep])
    mt, ms, ml = torch.cat(mb), torch.cat(ms), torch.cat(ml)
    order = ms.sort(dim=0, descending=True, stable=True)[1]
    if max_num is not None:
        order = order[:min(max_num, len(boxes))]
    out = type(boxes)(mt[order], box_dim=mt.shape[1], with_yaw=boxes.with_yaw)
    return out, ms[order], ml[order]


def merge_aug_bboxes_3d(aug_results, img_metas, test_cfg):
    """merge_augs.py:7-91 for one scene.  aug_results[a]: dict(boxes_3d, scores_3d, labels_3d) found on augmentation a;
    img_metas[a]: its meta (or the reference's [meta]).  Each result is mapped back (bbox3d_mapping_back), the results are
    concatenated in augmentation order, every class 0..max(label) goes through the BEV NMS by descending score (class-major),
    then all by descending score, cut to max_num.  Returns bbox3d2result (tensors on the CPU)."""
    return bbox3d2result(*merge_aug_single(aug_results, img_metas, test_cfg))
