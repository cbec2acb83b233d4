"""Test-time augmentation merge: `merge_aug_bboxes_3d` (mmdet3d/core/post_processing/merge_augs.py:7-91) for one scene, and the
front-end of csrc_post/merge.hip (`merge_sorted_segments`), the stable k-way merge the batched route
(Fcaf3DNeckWithHead.get_bboxes_aug) runs twice per batch.

Where the reference leaves a gap ("Test-time augmentation"): the merge NMS is FCAF3D's own BEV NMS (csrc/nms.hip, the
pcdet_nms semantics the first stage uses), rotated exactly when the boxes carry a yaw unless `test_cfg.use_rotate_nms` says
otherwise; `nms_thr` defaults to `iou_thr`, `max_num` to no cap; every sort is stable."""
import numpy as np
import torch

from . import _lib as L
from .boxes import bbox3d2result, bbox3d_mapping_back
from .nms import nms_bev

MERGE_TO_BOTTOM = 1          # include/fcaf3d_hip.h FC_MERGE_TO_BOTTOM
MERGE_WITH_YAW = 2           # FC_MERGE_WITH_YAW
XF_FLIP_H = 1 << 32          # FC_MERGE_XF_FLIP_H
XF_FLIP_V = 1 << 33          # FC_MERGE_XF_FLIP_V


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
    mb, ms, ml = [], [], []
    for c in range(int(labels.max()) + 1):
        ids = labels == c
        t, sc = boxes.tensor[ids], scores[ids]
        if len(sc) == 0:
            continue
        keep = nms_bev(t, sc, nms_thr, rotated=rotated, stable=True)
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
