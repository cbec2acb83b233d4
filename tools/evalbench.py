"""Evaluation wall time: `indoor_eval` (one IoU launch chain and read-back per (scene, class), a Python walk over every detection per
threshold) against `indoor_eval_device` (one fc_eval_match call, one read-back) on the SAME synthetic validation set, in the same
process; with --model also `runner.evaluate` against a loop of `simple_test_async` + `indoor_eval` over 32 scenes of 100 k points.
One JSON line (tools/, not product).

    python tools/evalbench.py [--scenes 312] [--classes 18] [--dets 2000] [--gts 14] [--reps 3] [--model] [--train-first N]

The defaults are a ScanNet validation pass: 312 scenes, 18 classes, ~2 000 boxes per scene surviving the NMS (README, inference and
test-time augmentation rows: 1 600 - 2 600), 14 ground-truth boxes per scene (synthetic.make_scene's 15, ScanNet's ~14).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fcaf3d_amd as fa  # noqa: E402
from fcaf3d_amd.evaluation import indoor_eval, indoor_eval_device  # noqa: E402

METRIC = (0.25, 0.5)


def synthetic_set(n_scenes, n_classes, n_det, n_gt, seed=0):
    """-> gt_annos, results as simple_test returns them (CPU dicts with bottom-centre box objects).  Per scene: n_gt axis-aligned
    boxes in a 6 x 5 x 2.7 m room; detections: two thirds jittered copies of ground-truth boxes under the box's class, one third
    clutter; scores uniform, copies scored higher on average."""
    rng = np.random.default_rng(seed)
    gt_annos, results = [], []
    for _ in range(n_scenes):
        gb = np.concatenate([rng.uniform((0, 0, .2), (6, 5, 2.2), (n_gt, 3)), rng.uniform(.3, 1.5, (n_gt, 3))], 1).astype(np.float32)
        gl = rng.integers(0, n_classes, n_gt)
        gt_annos.append({'gt_num': n_gt, 'gt_boxes_upright_depth': gb, 'class': gl})
        n_copy = (2 * n_det) // 3 if n_gt else 0
        src = rng.integers(0, max(n_gt, 1), n_copy)
        cb = gb[src].copy() if n_copy else np.zeros((0, 6), np.float32)
        cb[:, :3] += rng.normal(0, .08, (n_copy, 3)).astype(np.float32)
        cb[:, 3:] *= rng.uniform(.75, 1.25, (n_copy, 3)).astype(np.float32)
        n_cl = n_det - n_copy
        clutter = np.concatenate([rng.uniform((0, 0, .2), (6, 5, 2.2), (n_cl, 3)), rng.uniform(.3, 1.5, (n_cl, 3))], 1).astype(np.float32)
        db = np.concatenate([cb, clutter])
        dl = np.concatenate([gl[src] if n_copy else np.zeros(0, np.int64), rng.integers(0, n_classes, n_cl)])
        ds = np.concatenate([rng.uniform(.1, 1, n_copy), rng.uniform(.01, .5, n_cl)]).astype(np.float32)
        o = np.argsort(-ds, kind='stable')
        results.append(dict(boxes_3d=fa.DepthInstance3DBoxes(torch.from_numpy(db[o]), box_dim=6, with_yaw=False, origin=(.5, .5, .5)),
                            scores_3d=torch.from_numpy(ds[o]), labels_3d=torch.from_numpy(dl[o])))
    return gt_annos, results


def best_of(fn, reps):
    """-> (min wall seconds over `reps` calls after one warm call, last result)"""
    out = fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def agreement(a, b):
    """largest |difference| over the keys of two result dicts (equal scores may order differently: DESIGN.md section 15)"""
    assert sorted(a) == sorted(b)
    return max(abs(a[k] - b[k]) for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=312)
    ap.add_argument('--classes', type=int, default=18)
    ap.add_argument('--dets', type=int, default=2000, help='detections per scene')
    ap.add_argument('--gts', type=int, default=14, help='ground-truth boxes per scene')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--model', action='store_true', help='also time runner.evaluate against simple_test_async + indoor_eval')
    ap.add_argument('--model-scenes', type=int, default=32)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--points', type=int, default=100000)
    ap.add_argument('--train-first', type=int, default=0, help='training steps before the timed loops (trained weights keep more boxes)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    label2cat = {i: f'c{i}' for i in range(args.classes)}
    line = dict(tool='evalbench', scenes=args.scenes, classes=args.classes, dets_per_scene=args.dets, gts_per_scene=args.gts,
                thresholds=list(METRIC), reps=args.reps)

    gt_annos, results = synthetic_set(args.scenes, args.classes, args.dets, args.gts)
    # the same annotations as get_bboxes leaves them: (boxes, scores, labels) on the device
    triples = [(r['boxes_3d'].to(dev), r['scores_3d'].to(dev), r['labels_3d'].to(dev)) for r in results]
    t_host, ref = best_of(lambda: indoor_eval(gt_annos, results, METRIC, label2cat), args.reps)
    t_dev, got = best_of(lambda: indoor_eval_device(gt_annos, triples, METRIC, label2cat), args.reps)
    t_dev_cpu, got_cpu = best_of(lambda: indoor_eval_device(gt_annos, results, METRIC, label2cat), args.reps)
    line.update(indoor_eval_s=round(t_host, 4), indoor_eval_device_s=round(t_dev, 4),
                indoor_eval_device_from_cpu_results_s=round(t_dev_cpu, 4), speedup=round(t_host / t_dev, 1),
                speedup_from_cpu_results=round(t_host / t_dev_cpu, 1), max_abs_difference=agreement(ref, got),
                mAP_025=round(ref['mAP_0.25'], 4), mAP_050=round(ref['mAP_0.50'], 4))
    assert got == got_cpu
    # where the device path's time goes, as wall time: the device producer (annotations -> arrays, uploads, fc_eval_match, the
    # read-back) and the finisher (per-class sort + cumsum + AP on the host)
    from fcaf3d_amd.evaluation import finish_table, match_table_device
    table = match_table_device(gt_annos, triples, METRIC)
    t_finish, _ = best_of(lambda: finish_table(table, METRIC, label2cat), args.reps)
    t_match, _ = best_of(lambda: match_table_device(gt_annos, triples, METRIC), args.reps)
    line.update(device_producer_s=round(t_match, 4), finisher_s=round(t_finish, 4))

    if args.model:
        from fcaf3d_amd.runner import TrainStep, evaluate
        from fcaf3d_amd.synthetic import make_scene
        cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=0.02)
        torch.manual_seed(0)
        model = fa.build_detector(cfg.model, train_cfg=cfg.model.get('train_cfg'), test_cfg=cfg.model.get('test_cfg')).to(dev)
        scenes = [make_scene(5000 + i, n_points=args.points) for i in range(args.model_scenes)]
        pts = [torch.from_numpy(s[0]).to(dev) for s in scenes]
        metas = [dict(box_type_3d=fa.DepthInstance3DBoxes) for _ in scenes]
        B = args.batch
        batches = [(pts[i:i + B], metas[i:i + B]) for i in range(0, len(pts), B)]
        m_gt = [{'gt_num': len(s[1]), 'gt_boxes_upright_depth': s[1], 'class': s[2]} for s in scenes]
        if args.train_first:
            model.train()
            tr = TrainStep.from_config(model, cfg)
            for i in range(args.train_first):
                k = (i * B) % len(scenes)
                sc = scenes[k:k + B]
                tr(dict(points=pts[k:k + B], img_metas=metas[k:k + B],
                        gt_bboxes_3d=[fa.DepthInstance3DBoxes(torch.from_numpy(s[1]), origin=(.5, .5, .5)).to(dev) for s in sc],
                        gt_labels_3d=[torch.from_numpy(s[2]).to(dev) for s in sc]))
            torch.cuda.synchronize()
        model.eval()
        model.static_weights = True

        def reference_loop():
            with torch.no_grad():
                res, pending = [], None
                for points, img_metas in batches:
                    nxt = model.simple_test_async(points, img_metas)
                    if pending is not None:
                        res.extend(pending())
                    pending = nxt
                res.extend(pending())
            return indoor_eval(m_gt, res, METRIC, label2cat), res

        t_loop, (ref_m, res) = best_of(reference_loop, args.reps)
        t_eval, got_m = best_of(lambda: evaluate(model, batches, m_gt, METRIC, label2cat), args.reps)

        def forward_only():
            with torch.no_grad():
                for points, img_metas in batches:
                    model.simple_test(points, img_metas)
        t_fwd, _ = best_of(forward_only, args.reps)
        line['model'] = dict(scenes=len(scenes), points=args.points, batch=B, train_first=args.train_first,
                             survivors_per_scene=round(sum(len(r['scores_3d']) for r in res) / len(res), 1),
                             simple_test_async_plus_indoor_eval_s=round(t_loop, 4), evaluate_s=round(t_eval, 4),
                             speedup=round(t_loop / t_eval, 2), simple_test_only_s=round(t_fwd, 4),
                             max_abs_difference=agreement(ref_m, got_m))
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
