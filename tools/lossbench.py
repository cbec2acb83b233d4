"""Box-loss timings (tools/, not product): the enclosing-box kernel fc_eiou3d_fwd_bwd (GIoU, DIoU; csrc_post/eiou.hip) beside the rotated
IoU kernel fc_riou3d_fwd_bwd on the same rows, and the detector's forward_train + backward on the SUN RGB-D bench shape with IoU3DLoss,
GIoU3DLoss and DIoU3DLoss.  One JSON line.

    python tools/lossbench.py [--rows 250000] [--active 0.01 0.1 1.0] [--launches 50] [--rounds 7] [--no-model] [--steps 6]

Kernels: device events around `--launches` back-to-back launches of one kernel, after a warm pass of every kernel on the shape; the
kernels are alternated within a round and the round is repeated: the median over the rounds is reported with the smallest and largest
round, so that a difference can be told from the spread.  Rows: target centre U(-1,1)^3, sizes U(0.3,2)^3, yaw U(-3.1,3.1); pred = target
with the centre + U(-0.6,0.6), sizes x U(0.6,1.5), yaw + U(-0.5,0.5) (the distribution of tests/golden/make_golden_eiou.py); the active
rows (weight > 0) are drawn at random positions, as the positives of a scene lie among its locations.
Model: 8 scenes of 100 000 points, 4 levels (bench.py's sunrgbd-100k workload), one model per loss from the same seed, the losses
alternated within a round; wall time of forward_train + backward ending in a device synchronise, and device-event time of the loss_bbox
module alone (forward + backward) on the rows the head handed it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fcaf3d_amd as fa  # noqa: E402
from fcaf3d_amd import _lib as L  # noqa: E402


def pairs(rng, n):
    t = np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(0.3, 2, (n, 3)), rng.uniform(-3.1, 3.1, (n, 1))], 1)
    p = t.copy()
    p[:, :3] += rng.uniform(-0.6, 0.6, (n, 3))
    p[:, 3:6] *= rng.uniform(0.6, 1.5, (n, 3))
    p[:, 6] += rng.uniform(-0.5, 0.5, n)
    return p.astype(np.float32), t.astype(np.float32)


def stats(us):
    return dict(median_us=round(float(np.median(us)), 2), min_us=round(float(min(us)), 2), max_us=round(float(max(us)), 2))


def kernel_part(args, dev):
    rng = np.random.default_rng(0)
    n = args.rows
    p, t = pairs(rng, n)
    pred, target = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
    loss, iou = torch.empty(n, device=dev), torch.empty(n, device=dev)
    dpred = torch.empty((n, 7), device=dev)
    E = L.header_enums()
    out = {}
    for frac in args.active:
        w = np.zeros(n, np.float32)
        w[rng.permutation(n)[:max(1, int(round(frac * n)))]] = 1.0
        weight = torch.from_numpy(w).to(dev)
        s = L.stream()
        calls = {
            'riou3d': lambda: L.call('fc_riou3d_fwd_bwd', L.ptr(pred), L.ptr(target), L.ptr(weight), n, L.ptr(iou), L.ptr(dpred), s),
            'eiou3d_giou': lambda: L.call('fc_eiou3d_fwd_bwd', L.ptr(pred), L.ptr(target), 7, L.ptr(weight), n, 7, E['FC_EIOU_GIOU'],
                                          L.ptr(loss), L.ptr(iou), L.ptr(dpred), s),
            'eiou3d_diou': lambda: L.call('fc_eiou3d_fwd_bwd', L.ptr(pred), L.ptr(target), 7, L.ptr(weight), n, 7, E['FC_EIOU_DIOU'],
                                          L.ptr(loss), L.ptr(iou), L.ptr(dpred), s),
        }
        for fn in calls.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                e1.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
        row = {k: stats(v) for k, v in us.items()}
        for k in ('eiou3d_giou', 'eiou3d_diou'):
            row[k]['over_riou3d'] = round(row[k]['median_us'] / row['riou3d']['median_us'], 2)
        out[f'active_{frac:g}'] = dict(active_rows=int((w > 0).sum()), **row)
    return out


def model_part(args, dev):
    from fcaf3d_amd.synthetic import WORKLOADS, make_scene
    name = 'fcaf3d_sunrgbd-3d-10class'
    kw = WORKLOADS['sunrgbd-100k']['scene']
    scenes = [make_scene(7000 + i, **kw) for i in range(args.batch)]
    batch = dict(points=[torch.from_numpy(s[0]).to(dev) for s in scenes],
                 gt_bboxes_3d=[fa.DepthInstance3DBoxes(torch.from_numpy(s[1]), origin=(.5, .5, .5)) for s in scenes],
                 gt_labels_3d=[torch.from_numpy(s[2]).to(dev) for s in scenes],
                 img_metas=[dict(box_type_3d=fa.DepthInstance3DBoxes) for _ in scenes])
    models, seen = {}, {}
    for loss in ('IoU3DLoss', 'GIoU3DLoss', 'DIoU3DLoss'):
        torch.manual_seed(0)
        cfg = fa.get_config(name, voxel_size=0.02)
        cfg.model.neck_with_head['loss_bbox'] = dict(type=loss)
        model = fa.build_detector(cfg.model, train_cfg=cfg.model.get('train_cfg'), test_cfg=cfg.model.get('test_cfg')).to(dev).train()
        model.neck_with_head.loss_bbox.register_forward_pre_hook(
            lambda mod, a, k, loss=loss: seen.__setitem__(loss, (a[0].detach(), a[1], k['weight'], k['avg_factor'])), with_kwargs=True)
        models[loss] = model

    def step(model):
        model.zero_grad(set_to_none=True)
        losses = model(return_loss=True, **batch)
        sum(losses.values()).backward()
        return losses
    values = {}
    for loss, model in models.items():
        for _ in range(3):
            values[loss] = {k: round(float(v.detach()), 5) for k, v in step(model).items()}
    torch.cuda.synchronize()
    ms = {k: [] for k in models}
    for _ in range(args.steps):
        for loss, model in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(model)
            torch.cuda.synchronize()
            ms[loss].append((time.perf_counter() - t0) * 1e3)
    out = dict(workload='sunrgbd-100k, 8 scenes, 4 levels, voxel 0.02 m', steps=args.steps)
    # the loss_bbox module alone on the rows the head handed it: forward + backward, device events
    mod_us = {k: [] for k in models}
    for _ in range(args.rounds + 1):
        for loss, model in models.items():
            boxes, bt, weight, avg = seen[loss]
            boxes = boxes.clone().requires_grad_(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                model.neck_with_head.loss_bbox(boxes, bt, weight=weight, avg_factor=avg).backward()
            e1.record()
            e1.synchronize()
            mod_us[loss].append(e0.elapsed_time(e1) * 1e3 / 10)
    for loss in models:
        boxes, bt, weight, _ = seen[loss]
        out[loss] = dict(step_ms=dict(median=round(float(np.median(ms[loss])), 3), min=round(min(ms[loss]), 3), max=round(max(ms[loss]), 3)),
                         loss_bbox_module_fwd_bwd=stats(mod_us[loss][1:]), locations=int(boxes.shape[0]),
                         rows_with_weight=int((weight > 0).sum()), losses=values[loss])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=250000)
    ap.add_argument('--active', type=float, nargs='+', default=[0.01, 0.1, 1.0])
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-model', action='store_true')
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--batch', type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lossbench measures on the GPU; there is none here')
    dev = torch.device('cuda:0')
    line = dict(tool='lossbench', rows=args.rows, launches=args.launches, rounds=args.rounds, lib=os.path.basename(L.LIB_PATH),
                kernels=kernel_part(args, dev))
    if not args.no_model:
        line['model'] = model_part(args, dev)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
