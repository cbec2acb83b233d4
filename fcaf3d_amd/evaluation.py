"""mAP / recall of indoor 3D detections — the step AFTER the hot path: what the reference's
`indoor_eval` (mmdet3d/core/evaluation/indoor_eval.py:55-309) reports for ScanNet / SUN RGB-D / S3DIS.

Same inputs, same result keys (`<cat>_AP_0.25`, `mAP_0.25`, `<cat>_rec_0.25`, `mAR_0.25`, ...), same matching rule
(detections in descending confidence; a detection is a true positive for a threshold iff its best-overlapping GT box of
the same class and scene exceeds the threshold and is not yet taken; VOC 'area' AP).  The pairwise 3D IoU of a scene is
one call of the HIP rotated-BEV kernel (`fcaf3d_amd.nms.boxes_iou3d_gpu`) instead of a per-box host loop; a different
`iou_fn(pred (n,7), gt (m,7)) -> (n,m)` on gravity-centre boxes can be passed (the CPU tests pass the oracle's).

`indoor_eval_device` (second half of this file) returns the same dict with the matching of the WHOLE set in one native call
(csrc_post/eval.hip) and one read-back; `runner.evaluate` drives a model into it.  `indoor_eval` stays as the yardstick.
"""
import numpy as np
import torch


def average_precision(recalls, precisions, mode='area'):
    """VOC AP (indoor_eval.py:7-52) of one curve (n,) or of several (num_scales, n) -> float32 (num_scales,).
    'area': area under the monotone precision envelope; '11points': mean of the best precision at recall >= 0, .1, ... 1.
    NB the reference divides by 11 INSIDE its loop over scales, so with S scales entry i ends up divided S - i times;
    kept, because its own test vector (tests/test_metrics/test_indoor_eval.py:183-188) encodes it."""
    r = np.atleast_2d(np.asarray(recalls, np.float64))
    p = np.atleast_2d(np.asarray(precisions, np.float64))
    assert r.shape == p.shape and r.ndim == 2
    S = r.shape[0]
    ap = np.zeros(S, np.float32)
    if mode == 'area':
        for i in range(S):
            mrec = np.concatenate(([0.0], r[i], [1.0]))
            mpre = np.concatenate(([0.0], p[i], [0.0]))
            mpre = np.maximum.accumulate(mpre[::-1])[::-1]            # envelope
            step = np.nonzero(mrec[1:] != mrec[:-1])[0]
            ap[i] = np.sum((mrec[step + 1] - mrec[step]) * mpre[step + 1])
    elif mode == '11points':
        for i in range(S):
            for thr in np.arange(0, 1 + 1e-3, 0.1):
                sel = p[i, r[i] >= thr]
                ap[i] += sel.max() if sel.size else 0.0
            ap /= 11
    else:
        raise ValueError('Unrecognized mode, only "area" and "11points" are supported')
    return ap


def _gravity7(boxes):
    """DepthInstance3DBoxes-like (bottom-centre .tensor) or (n,6|7) gravity-centre array -> (n,7) float32 gravity-centre"""
    if hasattr(boxes, 'tensor'):
        t = boxes.tensor.detach().float().cpu().clone()
        if t.dim() == 1:
            t = t[None]
        t[:, 2] = t[:, 2] + t[:, 5] * 0.5
        return t
    a = np.asarray(boxes.cpu() if hasattr(boxes, 'cpu') else boxes, np.float32)
    if a.size == 0:
        return torch.zeros((0, 7))
    t = torch.from_numpy(a.reshape(-1, a.shape[-1]).copy())
    if t.shape[1] == 6:
        t = torch.cat((t, t.new_zeros(t.shape[0], 1)), 1)
    return t


def _default_iou(pred, gt):
    if not torch.cuda.is_available():
        raise RuntimeError('indoor_eval computes its IoU matrices on the GPU (HIP); pass iou_fn= for a CPU evaluation')
    from .nms import boxes_iou3d_gpu
    dev = torch.device('cuda', torch.cuda.current_device())
    return boxes_iou3d_gpu(pred.to(dev), gt.to(dev)).cpu().numpy()


def eval_det_cls(pred, gt, iou_thr, iou_fn=None):
    """One class.  pred: {scene: (boxes (n,7) gravity-centre, scores (n,))}, gt: {scene: boxes (m,7)}.
    -> [(recall, precision, ap)] per threshold (indoor_eval.py:55-160)."""
    iou_fn = iou_fn or _default_iou
    npos = sum(len(b) for b in gt.values())
    scene_of, conf, best_iou, best_j = [], [], [], []
    for sid, (boxes, scores) in pred.items():
        n = len(boxes)
        if n == 0:
            continue
        g = gt.get(sid)
        if g is not None and len(g) > 0:
            iou = np.asarray(iou_fn(boxes, g), np.float64)
            j = iou.argmax(1)                                  # first maximum, as the reference's strict '>' scan
            bi = iou[np.arange(n), j]
        else:
            j = np.zeros(n, np.int64)
            bi = np.full(n, -np.inf) if g is None or len(g) == 0 else np.zeros(n)
        scene_of += [sid] * n
        conf.append(np.asarray(scores, np.float64).reshape(-1))
        best_iou.append(bi)
        best_j.append(j)
    if not scene_of:
        conf_all = np.zeros(0); best_iou = np.zeros(0); best_j = np.zeros(0, np.int64)
    else:
        conf_all = np.concatenate(conf); best_iou = np.concatenate(best_iou); best_j = np.concatenate(best_j)
    order = np.argsort(-conf_all)
    out = []
    for thr in iou_thr:
        taken = {sid: np.zeros(len(b), bool) for sid, b in gt.items()}
        tp = np.zeros(len(order)); fp = np.zeros(len(order))
        for d, i in enumerate(order):
            sid = scene_of[i]
            if best_iou[i] > thr and not taken[sid][best_j[i]]:
                tp[d] = 1.0
                taken[sid][best_j[i]] = True
            else:
                fp[d] = 1.0
        ctp, cfp = np.cumsum(tp), np.cumsum(fp)
        # (a class that is detected but has no GT box anywhere gives 0/0 = nan in the reference; 0 here)
        recall = ctp / float(npos) if npos else ctp * 0.0
        precision = ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps)
        out.append((recall, precision, average_precision(recall, precision)))
    return out


def indoor_eval(gt_annos, dt_annos, metric, label2cat, logger=None, box_type_3d=None, box_mode_3d=None, iou_fn=None):
    """indoor_eval.py:205-309.  gt_annos[i]: dict(gt_num, gt_boxes_upright_depth (m,6|7) gravity-centre, class (m,));
    dt_annos[i]: dict(boxes_3d (box object with bottom-centre .tensor, or (n,7) gravity-centre), scores_3d, labels_3d).
    box_type_3d / box_mode_3d are accepted for signature compatibility (boxes are Depth-mode already)."""
    assert len(dt_annos) == len(gt_annos)
    pred, gt = {}, {}
    for sid, (g, d) in enumerate(zip(gt_annos, dt_annos)):
        labels = np.asarray(d['labels_3d'].cpu() if hasattr(d['labels_3d'], 'cpu') else d['labels_3d']).astype(np.int64)
        scores = np.asarray(d['scores_3d'].cpu() if hasattr(d['scores_3d'], 'cpu') else d['scores_3d'], np.float64)
        boxes = _gravity7(d['boxes_3d'])
        for c in np.unique(labels):
            m = labels == c
            pred.setdefault(int(c), {})[sid] = (boxes[torch.from_numpy(m)], scores[m])
            gt.setdefault(int(c), {}).setdefault(sid, torch.zeros((0, 7)))     # the reference registers the class in gt too
        if g['gt_num'] != 0:
            gb = _gravity7(g['gt_boxes_upright_depth'])
            gl = np.asarray(g['class']).astype(np.int64)
            for c in np.unique(gl):
                gt.setdefault(int(c), {})[sid] = gb[torch.from_numpy(gl == c)]
    rec, prec, ap = [{} for _ in metric], [{} for _ in metric], [{} for _ in metric]
    for c in gt:
        if c in pred:
            res = eval_det_cls(pred[c], gt[c], metric, iou_fn)
        for i in range(len(metric)):
            if c in pred:
                rec[i][c], prec[i][c], ap[i][c] = res[i]
            else:
                rec[i][c] = prec[i][c] = ap[i][c] = np.zeros(1)
    ret = {}
    lines = []
    for i, thr in enumerate(metric):
        for c in ap[i]:
            ret[f'{label2cat[c]}_AP_{thr:.2f}'] = float(ap[i][c][0])
        ret[f'mAP_{thr:.2f}'] = float(np.mean([v[0] for v in ap[i].values()])) if ap[i] else float('nan')
        recs = []
        for c in rec[i]:
            r = float(rec[i][c][-1]) if len(rec[i][c]) else 0.0
            ret[f'{label2cat[c]}_rec_{thr:.2f}'] = r
            recs.append(r)
        ret[f'mAR_{thr:.2f}'] = float(np.mean(recs)) if recs else float('nan')
        lines.append(f'mAP_{thr:.2f} {ret[f"mAP_{thr:.2f}"]:.4f}  mAR_{thr:.2f} {ret[f"mAR_{thr:.2f}"]:.4f}')
    if logger is not None:
        (logger.info if hasattr(logger, 'info') else print)('\n'.join(lines))
    return ret


# ---- the same evaluation with the matching on the device (csrc_post/eval.hip) -------------------------------------------------------
#
# `indoor_eval` above is the yardstick: one IoU launch chain and one read-back per (scene, class), then a Python walk over every
# detection per threshold.  The walk only looks sequential: a detection claims nothing but its BEST box, and only when that IoU
# exceeds the threshold, so the true positive of a (box, threshold) is the first claimant in descending-score order — a minimum,
# which fc_eval_match takes on the device for all scenes at once.  What remains for the host is per class a sort, two cumulative
# sums and the AP, in float64 exactly as above.  The one deliberate difference: equal scores within a class are ordered (smaller
# (scene id, position) first) where the reference's `np.argsort(-confidence)` leaves them to an unstable sort.

EVAL_DET_BOTTOM = 1                     # include/fcaf3d_hip.h FC_EVAL_DET_BOTTOM
_DET_SIDE, _GT_SIDE = 0, 1


class MatchTable:
    """What the finisher needs of a set of scenes, as plain arrays (picklable: it travels through all_gather_object).
    One row per detection: scene (int64, GLOBAL scene id), pos (int32, position in the scene), label (int64), score (float32),
    tp_bits (uint8, bit t = true positive at threshold t).  npos {class: ground-truth boxes}; first_seen {class: (scene id, side)}
    of every class seen among the detections (side 0) or the ground truth (side 1) — the order indoor_eval meets the classes in."""

    def __init__(self, scene, pos, label, score, tp_bits, npos, first_seen, n_thr):
        self.scene = np.asarray(scene, np.int64)
        self.pos = np.asarray(pos, np.int32)
        self.label = np.asarray(label, np.int64)
        self.score = np.asarray(score, np.float32)
        self.tp_bits = np.asarray(tp_bits, np.uint8)
        assert self.scene.shape == self.pos.shape == self.label.shape == self.score.shape == self.tp_bits.shape
        self.npos, self.first_seen, self.n_thr = dict(npos), dict(first_seen), int(n_thr)

    def __len__(self):
        return len(self.scene)


def _see(first_seen, c, scene, side):
    key = (int(scene), side)
    if c not in first_seen or key < first_seen[c]:
        first_seen[c] = key


def _scene_ids(n, scene_ids):
    ids = np.arange(n, dtype=np.int64) if scene_ids is None else np.asarray(list(scene_ids), np.int64)
    assert ids.shape == (n,) and len(np.unique(ids)) == n, 'scene_ids: one distinct id per scene'
    return ids


def _gt_arrays(gt_annos, ids):
    """-> boxes (n_gt, 7) float32 gravity centre, labels (n_gt,) int32, counts per scene, npos, first_seen (ground-truth side)"""
    boxes, labels, counts, npos, first_seen = [], [], [], {}, {}
    for sid, g in zip(ids, gt_annos):
        if g['gt_num'] == 0:
            counts.append(0)
            continue
        gb = _gravity7(g['gt_boxes_upright_depth']).numpy()
        gl = np.asarray(g['class']).astype(np.int64).reshape(-1)
        assert len(gb) == len(gl)
        boxes.append(gb); labels.append(gl); counts.append(len(gl))
        for c, k in zip(*np.unique(gl, return_counts=True)):
            npos[int(c)] = npos.get(int(c), 0) + int(k)
            _see(first_seen, int(c), sid, _GT_SIDE)
    gb = np.concatenate(boxes).astype(np.float32) if boxes else np.zeros((0, 7), np.float32)
    gl = np.concatenate(labels).astype(np.int32) if labels else np.zeros(0, np.int32)
    return gb, gl, np.asarray(counts, np.int64), npos, first_seen


def _det_parts(d):
    """a dt_annos dict or a (boxes, scores, labels) triple -> (boxes, scores, labels)"""
    if isinstance(d, dict):
        return d['boxes_3d'], d['scores_3d'], d['labels_3d']
    boxes, scores, labels = d
    return boxes, scores, labels


def _ordered_key(score, pos):
    """the key fc_eval_match minimises: ~(order-preserving bits of the fp32 score) in the high word, the position in the low"""
    u = (np.asarray(score, np.float32) + np.float32(0)).view(np.uint32)
    ordered = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return ((~ordered).astype(np.uint64) << np.uint64(32)) | np.asarray(pos).astype(np.uint64)


def _table(ids, det_counts, label, score, tp_bits, npos, first_seen, n_thr):
    scene = np.repeat(ids, det_counts)
    starts = np.cumsum(det_counts) - det_counts
    pos = np.arange(int(det_counts.sum()), dtype=np.int64) - np.repeat(starts, det_counts)
    label = np.asarray(label, np.int64)
    for c in np.unique(label):
        _see(first_seen, int(c), scene[label == c].min(), _DET_SIDE)
    return MatchTable(scene, pos, label, score, tp_bits, npos, first_seen, n_thr)


def match_table_host(gt_annos, dt_annos, metric, iou_fn=None, scene_ids=None, return_match=False):
    """The host producer: the table of fc_eval_match's contract in vectorised numpy, the IoU from `iou_fn` as in indoor_eval (CPU
    tests, cross-checks).  Scores are taken as fp32.  return_match: -> (table, best_iou float64, best_gt int64) per detection."""
    assert len(gt_annos) == len(dt_annos) and 1 <= len(metric) <= 8
    iou_fn = iou_fn or _default_iou
    ids = _scene_ids(len(gt_annos), scene_ids)
    _, _, _, npos, first_seen = _gt_arrays(gt_annos, ids)
    thr = [float(t) for t in metric]
    counts, labels_all, scores_all, bits_all, iou_all, gt_all = [], [], [], [], [], []
    for g, d in zip(gt_annos, dt_annos):
        b, s, l = _det_parts(d)
        labels = np.asarray(l.cpu() if hasattr(l, 'cpu') else l).astype(np.int64).reshape(-1)
        scores = np.asarray(s.cpu() if hasattr(s, 'cpu') else s).astype(np.float32).reshape(-1)
        boxes = _gravity7(b)
        n = len(labels)
        assert len(scores) == n and len(boxes) == n
        bits = np.zeros(n, np.uint8)
        best_iou, best_gt = np.full(n, -np.inf), np.full(n, -1, np.int64)
        if n and g['gt_num'] != 0:
            gb = _gravity7(g['gt_boxes_upright_depth'])
            gl = np.asarray(g['class']).astype(np.int64).reshape(-1)
            for c in np.unique(labels):
                m, gi = np.flatnonzero(labels == c), np.flatnonzero(gl == c)
                if len(gi):
                    iou = np.asarray(iou_fn(boxes[torch.from_numpy(m)], gb[torch.from_numpy(gi)]), np.float64)
                    j = iou.argmax(1)                                      # first maximum
                    best_iou[m], best_gt[m] = iou[np.arange(len(m)), j], gi[j]
            key = _ordered_key(scores, np.arange(n))
            for t, th in enumerate(thr):
                cl = np.flatnonzero(best_iou > th)                         # the claimants
                if len(cl):
                    o = cl[np.lexsort((key[cl], best_gt[cl]))]             # by box, then by key
                    first = np.ones(len(o), bool)
                    first[1:] = best_gt[o[1:]] != best_gt[o[:-1]]
                    bits[o[first]] |= np.uint8(1 << t)
        counts.append(n); labels_all.append(labels); scores_all.append(scores); bits_all.append(bits)
        iou_all.append(best_iou); gt_all.append(best_gt)
    cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dt)
    table = _table(ids, np.asarray(counts, np.int64), cat(labels_all, np.int64), cat(scores_all, np.float32), cat(bits_all, np.uint8),
                   npos, first_seen, len(thr))
    return (table, cat(iou_all, np.float64), cat(gt_all, np.int64)) if return_match else table


def eval_match(det_boxes, det_scores, det_labels, gt_boxes, gt_labels, seg, thr, flags=0):
    """fc_eval_match.  Device tensors det_boxes (n_det, 6|7) fp32, det_scores (n_det,) fp32, det_labels (n_det,) int64, gt_boxes
    (n_gt, 7) fp32 gravity centre, gt_labels (n_gt,) int32; seg (n_scenes, 4) int64 ON THE HOST (numpy: det_start, det_count,
    gt_start, gt_count — checked here); thr: the thresholds (host floats).  -> device (best_iou fp32, best_gt int32, tp_bits uint8)"""
    from . import _lib as L
    if not det_boxes.is_cuda:
        raise RuntimeError('the evaluation matching runs on the GPU only (HIP); match_table_host is the CPU producer')
    dev = det_boxes.device
    n_det, n_gt = det_boxes.shape[0], gt_boxes.shape[0]
    seg = np.ascontiguousarray(seg, np.int64).reshape(-1, 4)
    assert det_boxes.dim() == 2 and det_boxes.shape[1] in (6, 7) and gt_boxes.shape[1:] == (7,)
    assert det_boxes.dtype == gt_boxes.dtype == det_scores.dtype == torch.float32
    assert det_labels.dtype == torch.int64 and gt_labels.dtype == torch.int32
    assert det_scores.shape == det_labels.shape == (n_det,) and gt_labels.shape == (n_gt,)
    assert (seg >= 0).all() and (seg[:, 0] + seg[:, 1] <= n_det).all() and (seg[:, 2] + seg[:, 3] <= n_gt).all(), 'seg out of range'
    for col, what in ((0, 'detection'), (2, 'ground-truth')):               # two scenes must not share rows
        r = seg[seg[:, col + 1] > 0][:, col:col + 2]
        r = r[np.argsort(r[:, 0], kind='stable')]
        assert (r[:-1, 0] + r[:-1, 1] <= r[1:, 0]).all(), f'seg: {what} ranges of two scenes overlap'
    thr = np.asarray([float(t) for t in thr], np.float64)
    best_iou = torch.empty(n_det, dtype=torch.float32, device=dev)
    best_gt = torch.empty(n_det, dtype=torch.int32, device=dev)
    tp_bits = torch.empty(n_det, dtype=torch.uint8, device=dev)
    if n_det == 0:
        return best_iou, best_gt, tp_bits
    with torch.cuda.device(dev):
        seg_d = L.upload(seg, dev) if len(seg) else None
        thr_d = L.upload(thr, dev)
        ws = L.workspace(L.query('fc_eval_match_ws_bytes', n_det, n_gt, len(thr)), dev)
        L.call('fc_eval_match', L.ptr(det_boxes.contiguous()), det_boxes.shape[1], L.ptr(det_scores.contiguous()),
               L.ptr(det_labels.contiguous()), L.ptr(gt_boxes.contiguous()) if n_gt else None,
               L.ptr(gt_labels.contiguous()) if n_gt else None, L.ptr(seg_d), len(seg), n_det, n_gt, L.ptr(thr_d), len(thr),
               int(flags), L.ptr(best_iou), L.ptr(best_gt), L.ptr(tp_bits), L.ptr(ws), ws.numel(), L.stream())
    return best_iou, best_gt, tp_bits


def _det_tensors(dets, dev):
    """every scene's detections as ONE (boxes (n_det, 6|7), scores, labels) on `dev`, their per-scene counts (host, from the
    shapes: nothing is read back) and the fc_eval_match flags.  A scene without detections adds a count of 0 and nothing else.
    Box objects carry the bottom-centre tensor: a set of nothing but box objects goes to the kernel as it is, with
    FC_EVAL_DET_BOTTOM; a set of nothing but gravity-centre arrays of one width goes as it is, without; any other mixture is first
    brought to gravity-centre 7 columns with the fp32 operations of _gravity7."""
    counts, boxes, scores, labels, bottom = [], [], [], [], []
    for d in dets:
        b, s, l = _det_parts(d)
        s = torch.as_tensor(s).detach().float().reshape(-1)
        counts.append(len(s))
        if len(s) == 0:
            continue
        bottom.append(hasattr(b, 'tensor'))
        b = torch.as_tensor(b.tensor if bottom[-1] else b).detach().float()
        b = b.reshape(-1, b.shape[-1])
        l = torch.as_tensor(l).detach().long().reshape(-1)
        assert b.shape[1] in (6, 7) and len(b) == len(s) == len(l)
        boxes.append(b); scores.append(s); labels.append(l)
    counts = np.asarray(counts, np.int64)
    if not boxes:
        return (torch.zeros((0, 7), device=dev), torch.zeros(0, device=dev), torch.zeros(0, dtype=torch.long, device=dev), counts, 0)
    flags = EVAL_DET_BOTTOM if all(bottom) else 0
    if len(set(bottom)) > 1 or len({b.shape[1] for b in boxes}) > 1:
        flags = 0
        for i, b in enumerate(boxes):
            if b.shape[1] == 6:
                b = torch.cat((b, b.new_zeros(len(b), 1)), 1)
            if bottom[i]:
                b = b.clone()
                b[:, 2] = b[:, 2] + b[:, 5] * 0.5
            boxes[i] = b

    def gather(parts):
        if all(not p.is_cuda for p in parts):
            return torch.cat(parts).to(dev)                                 # one upload
        return torch.cat([p.to(dev) for p in parts])
    return gather(boxes), gather(scores), gather(labels), counts, flags


def match_table_device(gt_annos, dets, metric, scene_ids=None, device=None, return_match=False):
    """The device producer: ONE fc_eval_match call for the whole set and ONE read-back (scores, labels and the true-positive bits
    in one buffer).  dets[i]: a dt_annos dict (tensors on either side) or the (boxes, scores, labels) triple of get_bboxes.
    return_match (tests): -> (table, best_iou fp32, best_gt) per detection, at the price of two more read-backs."""
    assert len(gt_annos) == len(dets) and 1 <= len(metric) <= 8
    if not torch.cuda.is_available():
        raise RuntimeError('indoor_eval_device matches on the GPU (HIP); match_table_host is the CPU producer')
    from . import _lib as L
    if device is None:
        first = next((t for d in dets for t in (_det_parts(d)[1],) if getattr(t, 'is_cuda', False)), None)
        device = first.device if first is not None else torch.device('cuda', torch.cuda.current_device())
    dev = torch.device(device)
    ids = _scene_ids(len(gt_annos), scene_ids)
    gb, gl, gcounts, npos, first_seen = _gt_arrays(gt_annos, ids)
    boxes, scores, labels, dcounts, flags = _det_tensors(dets, dev)
    seg = np.stack([np.cumsum(dcounts) - dcounts, dcounts, np.cumsum(gcounts) - gcounts, gcounts], 1) if len(ids) else np.zeros((0, 4), np.int64)
    n = int(dcounts.sum())
    if n == 0:
        table = _table(ids, dcounts, np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.uint8), npos, first_seen, len(metric))
        return (table, np.zeros(0, np.float32), np.zeros(0, np.int64)) if return_match else table
    with torch.cuda.device(dev):
        gb_d = L.upload(gb, dev) if len(gb) else torch.zeros((0, 7), device=dev)
        gl_d = L.upload(gl, dev) if len(gl) else torch.zeros(0, dtype=torch.int32, device=dev)
        best_iou, best_gt, tp_bits = eval_match(boxes, scores, labels, gb_d, gl_d, seg, metric, flags)
        packed = torch.stack((scores.view(torch.int32), labels.to(torch.int32), tp_bits.to(torch.int32))).cpu().numpy()   # the read-back
    table = _table(ids, dcounts, packed[1].astype(np.int64), packed[0].view(np.float32), packed[2].astype(np.uint8), npos, first_seen,
                   len(metric))
    return (table, best_iou.cpu().numpy(), best_gt.cpu().numpy().astype(np.int64)) if return_match else table


def merge_tables(tables):
    """concatenation of tables of disjoint scenes (shards, ranks), in any order: the finisher orders the rows itself"""
    tables = list(tables)
    assert tables and len({t.n_thr for t in tables}) == 1
    npos, first_seen = {}, {}
    for t in tables:
        for c, k in t.npos.items():
            npos[c] = npos.get(c, 0) + k
        for c, (sid, side) in t.first_seen.items():
            _see(first_seen, c, sid, side)
    cat = lambda name: np.concatenate([getattr(t, name) for t in tables])
    out = MatchTable(cat('scene'), cat('pos'), cat('label'), cat('score'), cat('tp_bits'), npos, first_seen, tables[0].n_thr)
    pairs = np.stack((out.scene, out.pos.astype(np.int64)), 1)
    assert len(np.unique(pairs, axis=0)) == len(pairs), 'merge_tables: the same (scene id, position) in two tables'
    return out


def finish_table(table, metric, label2cat=None, logger=None):
    """The finisher: per class the rows by descending score (equal scores: smaller (scene id, position) first), cumulative sums,
    recall, precision and VOC AP in float64 -> the dict indoor_eval returns (same keys, the zeros(1) entry of a class with
    ground truth but no detection, the same means, the classes in the order indoor_eval meets them)."""
    assert table.n_thr == len(metric)
    name = (lambda c: label2cat[c]) if label2cat is not None else str
    classes = sorted(table.first_seen, key=lambda c: table.first_seen[c] + (c,))
    rec, ap = [{} for _ in metric], [{} for _ in metric]
    for c in classes:
        rows = np.flatnonzero(table.label == c)
        if len(rows):
            rows = rows[np.lexsort((table.pos[rows], table.scene[rows], -table.score[rows].astype(np.float64)))]
            npos = table.npos.get(c, 0)
        for i in range(len(metric)):
            if not len(rows):
                rec[i][c] = ap[i][c] = np.zeros(1)
                continue
            tp = ((table.tp_bits[rows] >> i) & 1).astype(np.float64)
            ctp, cfp = np.cumsum(tp), np.cumsum(1.0 - tp)
            recall = ctp / float(npos) if npos else ctp * 0.0
            precision = ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps)
            rec[i][c], ap[i][c] = recall, average_precision(recall, precision)
    ret, lines = {}, []
    for i, thr in enumerate(metric):
        for c in ap[i]:
            ret[f'{name(c)}_AP_{thr:.2f}'] = float(ap[i][c][0])
        ret[f'mAP_{thr:.2f}'] = float(np.mean([v[0] for v in ap[i].values()])) if ap[i] else float('nan')
        recs = []
        for c in rec[i]:
            r = float(rec[i][c][-1]) if len(rec[i][c]) else 0.0
            ret[f'{name(c)}_rec_{thr:.2f}'] = r
            recs.append(r)
        ret[f'mAR_{thr:.2f}'] = float(np.mean(recs)) if recs else float('nan')
        lines.append(f'mAP_{thr:.2f} {ret[f"mAP_{thr:.2f}"]:.4f}  mAR_{thr:.2f} {ret[f"mAR_{thr:.2f}"]:.4f}')
    if logger is not None:
        (logger.info if hasattr(logger, 'info') else print)('\n'.join(lines))
    return ret


def _gathering(group):
    """(world size, rank) of the gather: group=None is the default process group when torch.distributed is initialised,
    group=False never gathers"""
    import torch.distributed as dist
    if group is False or not (dist.is_available() and dist.is_initialized()):
        return 1, 0
    return dist.get_world_size(group), dist.get_rank(group)


def gather_tables(table, group=None):
    """every rank's table, merged, on every rank: one all_gather_object over `group`, no other collective"""
    import torch.distributed as dist
    world, _ = _gathering(group)
    if world == 1:
        return table
    parts = [None] * world
    dist.all_gather_object(parts, table, group=group)
    return merge_tables(parts)


def default_scene_ids(n, group=None):
    """rank + world_size * i: the scenes a rank holds when a set is dealt out round-robin"""
    world, rank = _gathering(group)
    return rank + world * np.arange(n, dtype=np.int64)


def indoor_eval_device(gt_annos, dets, metric, label2cat, logger=None, scene_ids=None, group=None):
    """indoor_eval with the matching on the device: the device producer (one native call, one read-back), the gather of the ranks'
    tables over `group` when torch.distributed is initialised (each rank passes ITS scenes; scene_ids: their global ids, default
    rank + world_size * i; group=False: no gather), the finisher.  Every rank returns the same dict."""
    if scene_ids is None:
        scene_ids = default_scene_ids(len(gt_annos), group)
    table = match_table_device(gt_annos, dets, metric, scene_ids=scene_ids)
    return finish_table(gather_tables(table, group), metric, label2cat, logger)
