"""The input side of a training step, three ways, at bench.py's primary shape (8 scenes per step, 100 000 sampled points from
resident synthetic scenes of 150 000, 2 cm voxels, the full 4-level model) — one process, the variants alternated:

  A  TrainStep over PRE-BUILT resident batches (already sampled and augmented): what bench.py times; the yardstick
  B  the per-scene path: pipelines.TrainAugment.lazy on every scene of every batch (a randperm, two .tolist() read-backs, box
     launches and one fc_augment_voxelize launch per scene)
  C  runner.fit's loader: data.DeviceLoader over data.ResidentScenes (a descriptor table per batch, one fc_batch_augment_voxelize)

Per round every variant runs `--steps` steps behind its own warm-up, A twice (its two windows give A's run-to-run spread, the
yardstick of "within noise").  Printed: scenes/s per variant and round, TrainStep.phase_s per phase and step, and — counted on
one batch outside the timed windows — the device synchronisations (torch.cuda.set_sync_debug_mode) and the native input-stage
launches of building and voxelising it.  A counted launch or synchronisation is a count, not a speed-up; one JSON line at the end.

    python tools/trainbench.py [--rounds 3] [--steps 12] [--warmup 4] [--batch 8] [--points 100000] [--scene-points 150000]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--points', type=int, default=100000)
    ap.add_argument('--scene-points', type=int, default=150000)
    ap.add_argument('--scenes', type=int, default=16)
    ap.add_argument('--levels', type=int, default=4)
    ap.add_argument('--reserve-gb', type=float, default=32.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/trainbench.py measures on the GPU; there is none')
    import fcaf3d_amd as fa
    import fcaf3d_amd.functional as Fn
    from fcaf3d_amd import _lib as L
    from fcaf3d_amd import data as DT
    from fcaf3d_amd.pipelines import TrainAugment
    from fcaf3d_amd.runner import TrainStep, reserve_device_memory
    from fcaf3d_amd.synthetic import make_scene
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=0.02)
    if args.levels != 4:
        cfg.model.backbone['n_outs'] = args.levels
        cfg.model.neck_with_head['in_channels'] = (64, 128, 256, 512)[:args.levels]
        cfg.model.neck_with_head.assigner['n_scales'] = args.levels
    model = fa.build_detector(cfg.model, train_cfg=cfg.model.get('train_cfg'), test_cfg=cfg.model.get('test_cfg')).to(dev).train()
    model.async_maps, model.inputs_resident, Fn.WGRAD_ASYNC = True, True, True
    tr = TrainStep.from_config(model, cfg)
    if args.reserve_gb > 0:
        reserve_device_memory(args.reserve_gb, dev)

    # the scenes: on disk in the reference's layout (C), the same raw clouds as device tensors (A, B)
    tmp = tempfile.mkdtemp(prefix='trainbench_')
    import atexit
    import shutil
    atexit.register(shutil.rmtree, tmp, True)
    os.makedirs(os.path.join(tmp, 'points'))
    import pickle
    infos, raw, gts, labs = [], [], [], []
    for k in range(args.scenes):
        pts, gt, lab = make_scene(1000 + k, n_points=args.scene_points)
        pts.astype(np.float32).tofile(os.path.join(tmp, 'points', f'{k}.bin'))
        infos.append(dict(point_cloud=dict(num_features=6, lidar_idx=k), pts_path=f'points/{k}.bin',
                          annos=dict(gt_num=len(gt), gt_boxes_upright_depth=gt[:, :6].astype(np.float32), **{'class': lab.astype(np.int64)})))
        raw.append(torch.from_numpy(pts.astype(np.float32)).to(dev))
        b = fa.DepthInstance3DBoxes(torch.from_numpy(gt[:, :6].astype(np.float32)), box_dim=6, with_yaw=False, origin=(.5, .5, .5))
        gts.append(b.tensor.to(dev))
        labs.append(torch.from_numpy(lab.astype(np.int64)))
    with open(os.path.join(tmp, 'infos.pkl'), 'wb') as f:
        pickle.dump(infos, f)
    pipeline = [dict(type='LoadPointsFromFile', coord_type='DEPTH', load_dim=6, use_dim=[0, 1, 2, 3, 4, 5]),
                dict(type='LoadAnnotations3D'), dict(type='IndoorPointSample', num_points=args.points),
                dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
                dict(type='GlobalRotScaleTrans', rot_range=[-0.087266, 0.087266], scale_ratio_range=[.9, 1.1], translation_std=[.1, .1, .1]),
                dict(type='DefaultFormatBundle3D', class_names=None), dict(type='Collect3D', keys=['points', 'gt_bboxes_3d', 'gt_labels_3d'])]
    ds = DT.build_dataset(dict(type='ScanNetDataset', data_root=tmp, ann_file=os.path.join(tmp, 'infos.pkl'), pipeline=pipeline))
    loader = DT.DeviceLoader(DT.ResidentScenes(ds, dev), pipeline, args.batch, seed=0)
    aug = TrainAugment(num_points=args.points)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    order = [np.roll(np.arange(args.scenes), -args.batch * j)[:args.batch] for j in range(max(args.scenes // args.batch, 1))]

    def metas(n):
        return [dict(box_type_3d=fa.DepthInstance3DBoxes) for _ in range(n)]

    def box(t, to=None):
        g = fa.DepthInstance3DBoxes.__new__(fa.DepthInstance3DBoxes)
        g.tensor, g.box_dim, g.with_yaw = (t if to is None else t.to(to)), 7, False
        return g

    def batch_b(j):
        pts, bxs, lbs = [], [], []
        for i in order[j % len(order)]:
            lazy, bx, _ = aug.lazy(raw[i], gts[i], gen)
            pts.append(lazy); bxs.append(box(bx)); lbs.append(labs[i])
        return dict(points=pts, gt_bboxes_3d=bxs, gt_labels_3d=lbs, img_metas=metas(len(pts)))

    # A: the clouds B's path would feed, materialised once
    pre = []
    for j in range(len(order)):
        b = batch_b(j)
        pre.append(dict(b, points=[p.materialize() for p in b['points']], gt_bboxes_3d=[box(g.tensor, 'cpu') for g in b['gt_bboxes_3d']]))
    torch.cuda.synchronize()

    c_state = dict(epoch=0, queue=[])

    def batch_c(_):
        if not c_state['queue']:
            c_state['queue'] = loader.batches(c_state['epoch'])
            c_state['epoch'] += 1
        return c_state['queue'].pop(0)

    makers = dict(A=lambda j: pre[j % len(pre)], B=batch_b, C=batch_c)

    def window(name, n):
        """n steps of a variant, each with the next batch handed over for prefetch; -> (seconds, phase seconds per step)"""
        make = makers[name]
        torch.cuda.synchronize()
        ph0, t0 = list(tr.phase_s), time.perf_counter()
        nxt = make(0)
        for j in range(n):
            cur, nxt = nxt, (make(j + 1) if j + 1 < n else None)
            tr(cur, nxt)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, [(a - b) / n for a, b in zip(tr.phase_s, ph0)]

    def counts(name):
        """device synchronisations and native input-stage launches of building one batch and voxelising it (untimed)"""
        calls = []
        real = L.call

        def counting(fn, *a):
            if fn in ('fc_augment_voxelize', 'fc_batch_augment_voxelize', 'fc_voxelize'):
                calls.append(fn)
            return real(fn, *a)
        torch.cuda.synchronize()
        L.call = counting
        torch.cuda.set_sync_debug_mode('warn')
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter('always')
                b = makers[name](0)
                model.voxelize(b['points'])
            syncs = sum('synchroniz' in str(x.message) for x in w)
        finally:
            torch.cuda.set_sync_debug_mode('default')
            L.call = real
        torch.cuda.synchronize()
        return dict(syncs=syncs, native_input_launches=len(calls))

    res = {k: [] for k in ('A', 'A2', 'B', 'C')}
    phases = {k: [] for k in res}
    for r in range(args.rounds):
        for name in ('A', 'B', 'C', 'A2'):
            v = name[0]
            window(v, args.warmup)
            dt, ph = window(v, args.steps)
            res[name].append(args.batch * args.steps / dt)
            phases[name].append(ph)
            print(f'round {r} {name}: {res[name][-1]:8.1f} scenes/s   phase ms/step ' + ' '.join(f'{1e3 * p:6.2f}' for p in ph), flush=True)
    cnt = {v: counts(v) for v in ('A', 'B', 'C')}
    a_all = res['A'] + res['A2']
    spread = max(abs(x - y) / max(x, y) for x, y in zip(res['A'], res['A2']))
    out = dict(shape=dict(batch=args.batch, points=args.points, scene_points=args.scene_points, levels=args.levels, steps=args.steps,
                          rounds=args.rounds),
               scenes_per_s={k: [round(x, 1) for x in v] for k, v in res.items()},
               median={k: round(float(np.median(v)), 1) for k, v in dict(A=a_all, B=res['B'], C=res['C']).items()},
               a_spread_same_round=round(spread, 4), a_range=[round(min(a_all), 1), round(max(a_all), 1)],
               phase_ms_per_step={k: [round(1e3 * float(np.median([p[i] for p in v])), 3) for i in range(4)] for k, v in phases.items()},
               per_batch=cnt)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
