"""What test-time augmentation and box voting do to a validation pass: `runner.validate` over ONE synthetic resident validation set
(sized as `evalbench.py --model`: 32 scenes of 100 k points, 8 scenes per batch) three ways — the single-augmentation pipeline, A = 4
flips (MultiScaleFlipAug3D flip=True with both BEV flips: data.AugDeviceLoader), and A = 4 flips with test_cfg.vote_thr — in one
process.  One JSON line (tools/, not product):

    scenes/s of each pass (best of --reps wall times around a pass that ends in a device synchronise, after a warm pass)
    fc_vote_boxes ms per batch beside the merge NMS's ms on the same batches (device events around the launches, in a pass of
    their own after the timed ones), mean members per kept box (the kernel's own member counts)
    mAP@0.25 / mAP@0.5 of each pass

    python tools/ttaevalbench.py [--scenes 32] [--points 100000] [--batch 8] [--vote-thr 0.6] [--reps 3] [--train-first N]

The scenes are synthetic (synthetic.make_scene) and the weights random or trained for --train-first steps on the same scenes: the
mAP columns record what the stages do to THIS set; they say nothing about real data."""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fcaf3d_amd as fa  # noqa: E402
from fcaf3d_amd import data as DT  # noqa: E402
from fcaf3d_amd.build import source_hash  # noqa: E402
from fcaf3d_amd.runner import TrainStep, build_val_loader, validate  # noqa: E402

METRIC = (0.25, 0.5)
CLASSES = tuple(f'c{i}' for i in range(18))


def write_set(root, n_scenes, n_points):
    """the scenes of `evalbench.py --model` (synthetic.make_scene(5000 + i)) as .bin files + an info .pkl in the reference's layout"""
    from fcaf3d_amd.synthetic import make_scene
    os.makedirs(os.path.join(root, 'points'), exist_ok=True)
    infos = []
    for k in range(n_scenes):
        pts, gt, lab = make_scene(5000 + k, n_points=n_points)
        pts.astype(np.float32).tofile(os.path.join(root, 'points', f'{k:04d}.bin'))
        annos = dict(gt_num=len(gt), name=np.array([CLASSES[i] for i in lab]), gt_boxes_upright_depth=gt[:, :6].astype(np.float32),
                     **{'class': lab.astype(np.int64)})
        infos.append(dict(point_cloud=dict(num_features=6, lidar_idx=f'scene{k:04d}'), pts_path=f'points/{k:04d}.bin', annos=annos))
    ann = os.path.join(root, 'infos.pkl')
    with open(ann, 'wb') as f:
        pickle.dump(infos, f)
    return ann


def pipelines(n_points):
    load = dict(type='LoadPointsFromFile', coord_type='DEPTH', shift_height=False, use_color=True, load_dim=6, use_dim=[0, 1, 2, 3, 4, 5])
    train = [load, dict(type='LoadAnnotations3D', with_bbox_3d=True, with_label_3d=True),
             dict(type='IndoorPointSample', num_points=n_points),
             dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
             dict(type='GlobalRotScaleTrans', rot_range=[-0.087266, 0.087266], scale_ratio_range=[.9, 1.1], translation_std=[.1, .1, .1],
                  shift_height=False),
             dict(type='DefaultFormatBundle3D', class_names=CLASSES), dict(type='Collect3D', keys=['points', 'gt_bboxes_3d', 'gt_labels_3d'])]

    def test(flip):
        return [load, dict(type='MultiScaleFlipAug3D', img_scale=(1333, 800), pts_scale_ratio=1, flip=flip, pcd_horizontal_flip=flip,
                           pcd_vertical_flip=flip, transforms=[
                               dict(type='GlobalRotScaleTrans', rot_range=[0, 0], scale_ratio_range=[1., 1.], translation_std=[0, 0, 0]),
                               dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
                               dict(type='IndoorPointSample', num_points=n_points),
                               dict(type='DefaultFormatBundle3D', class_names=CLASSES, with_label=False),
                               dict(type='Collect3D', keys=['points'])])]
    return train, test(False), test(True)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=32)
    ap.add_argument('--points', type=int, default=100000)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--vote-thr', type=float, default=0.6)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--train-first', type=int, default=0, help='training steps before the timed passes (trained weights keep other boxes)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    label2cat = dict(enumerate(CLASSES))
    cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=0.02)
    torch.manual_seed(0)
    model = fa.build_detector(cfg.model, train_cfg=cfg.model.get('train_cfg'), test_cfg=cfg.model.get('test_cfg')).to(dev)
    nh = model.neck_with_head
    train_pipe, single_pipe, tta_pipe = pipelines(args.points)
    with tempfile.TemporaryDirectory() as root:
        ann = write_set(root, args.scenes, args.points)
        base = dict(type='ScanNetDataset', data_root=root, ann_file=ann, classes=CLASSES, box_type_3d='Depth')
        vs = DT.build_dataset(dict(base, pipeline=single_pipe, test_mode=True))
        rs = DT.ResidentScenes(vs, dev)
        if args.train_first:
            ts = DT.build_dataset(dict(base, pipeline=train_pipe, filter_empty_gt=True))
            tl = DT.DeviceLoader(DT.ResidentScenes(ts, dev), train_pipe, args.batch, seed=0)
            model.train()
            tr = TrainStep.from_config(model, cfg)
            done, epoch = 0, 0
            while done < args.train_first:
                bs = tl.batches(epoch)
                for k, b in enumerate(bs[:args.train_first - done]):
                    tr(b, bs[k + 1] if k + 1 < len(bs) else None)
                done += len(bs[:args.train_first - done])
                epoch += 1
            torch.cuda.synchronize()
    model.eval()
    model.static_weights = True
    loaders = dict(single=build_val_loader(rs, single_pipe, args.batch), tta4=build_val_loader(rs, tta_pipe, args.batch))
    assert type(loaders['single']) is DT.DeviceLoader and type(loaders['tta4']) is DT.AugDeviceLoader and len(loaders['tta4'].augs) == 4
    line = dict(tool='ttaevalbench', source_hash=source_hash(), scenes=args.scenes, points=args.points, batch=args.batch, augs=4,
                vote_thr=args.vote_thr, reps=args.reps, train_first=args.train_first, thresholds=list(METRIC))
    res = {}
    for name, ld, thr in (('single', loaders['single'], None), ('tta4', loaders['tta4'], None), ('tta4_vote', loaders['tta4'], args.vote_thr)):
        if thr is None:
            nh.test_cfg.pop('vote_thr', None)
        else:
            nh.test_cfg['vote_thr'] = thr
        t, out = best_of(lambda: validate(model, ld, METRIC, label2cat), args.reps)
        res[name] = dict(validate_s=round(t, 4), scenes_per_s=round(args.scenes / t, 2), mAP_025=round(float(out['mAP_0.25']), 4),
                         mAP_050=round(float(out['mAP_0.50']), 4), mAR_025=round(float(out['mAR_0.25']), 4),
                         mAR_050=round(float(out['mAR_0.50']), 4))
    # the voting launch beside the merge NMS it follows, on the same batches: device events, one more pass (vote_thr still set)
    nh.nms_events, nh.vote_events, nh.vote_members, nh.merge_events = [], [], [], []
    validate(model, loaders['tta4'], METRIC, label2cat)
    torch.cuda.synchronize()
    ms = lambda evs: [a.elapsed_time(b) for a, b in evs]
    kept = sum(int(kc.sum()) for _, kc in nh.vote_members)
    members = sum(int(m[torch.arange(m.shape[1], device=m.device)[None, :] < kc[:, None]].sum()) for m, kc in nh.vote_members)
    cand = sum(int(m.shape[1]) for m, _ in nh.vote_members)
    line.update(res, vote=dict(batches=len(nh.vote_events), fc_vote_boxes_ms_per_batch=round(float(np.mean(ms(nh.vote_events))), 4),
                               merge_nms_ms_per_batch=round(float(np.mean(ms(nh.nms_events))), 4),
                               merge_stage_ms_per_batch=round(float(np.mean(ms(nh.merge_events))), 4),
                               kept_per_scene=round(kept / args.scenes, 1), members_per_kept_box=round(members / max(kept, 1), 3),
                               longest_segment_mean=round(cand / max(len(nh.vote_members), 1), 1)))
    nh.nms_events = nh.vote_events = nh.vote_members = nh.merge_events = None
    nh.test_cfg.pop('vote_thr', None)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
