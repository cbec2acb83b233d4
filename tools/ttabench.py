"""Test-time augmentation throughput: simple_test scenes/s against aug_test scenes/s for A = 1, 2, 4 augmentations (A = 2: one
BEV flip, A = 4: both BEV directions, MultiScaleFlipAug3D's order), the merge stage's device time per batch (HIP events around
Fcaf3DNeckWithHead.get_bboxes_aug's merge: both merge launches and the merge NMS), and survivors per scene before / after the
merge.  One JSON line (tools/, not product).

    python tools/ttabench.py [--train-first N] [--reps R] [bench.py flags: --batch 8 --workload scannet-100k --voxel-size 0.02]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

AUGS = {1: [(False, False)], 2: [(False, False), (True, False)], 4: [(False, False), (False, True), (True, False), (True, True)]}


def _flip(p, h, v):
    """RandomFlip3D on a device point tensor (a fresh tensor: the inputs are not touched)"""
    q = p.clone()
    if h:
        q[:, 0] = -q[:, 0]
    if v:
        q[:, 1] = -q[:, 1]
    return q


def main():
    opts = {'--train-first': '0', '--reps': '6'}
    for flag in list(opts):
        if flag in sys.argv:
            k = sys.argv.index(flag)
            opts[flag] = sys.argv[k + 1]
            del sys.argv[k:k + 2]
    args = bench.parse()
    dev = torch.device('cuda:0')
    model, cfg = bench.build_model(args)
    model = model.to(dev)
    batches = bench.make_batches(args, 0, dev)
    if int(opts['--train-first']):
        from fcaf3d_amd.runner import TrainStep
        model.train()
        model.async_maps = True
        model.inputs_resident = True
        tr = TrainStep.from_config(model, cfg)
        for i in range(int(opts['--train-first'])):
            tr(batches[i % len(batches)])
        torch.cuda.synchronize()
    model = model.eval()
    model.static_weights = True
    reps = int(opts['--reps'])
    nh = model.neck_with_head
    B = args.batch
    # the augmented copies are made once, before the timed region (the pipeline's work, not the detector's)
    inputs = {}
    for A, augs in AUGS.items():
        inputs[A] = []
        for b in batches[:2]:
            pts = [[_flip(p, h, v) for p in b['points']] for h, v in augs]
            metas = [[dict(box_type_3d=m['box_type_3d'], pcd_scale_factor=1.0, pcd_horizontal_flip=h, pcd_vertical_flip=v)
                      for m in b['img_metas']] for h, v in augs]
            inputs[A].append((pts, metas))
    simple = [(b['points'], b['img_metas']) for b in batches[:2]]

    def timed(fn, items):
        with torch.no_grad():
            for i in range(3):                                # warm every shape (plans, executor programs, workspaces)
                fn(*items[i % len(items)])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = None
            for i in range(reps):
                out = fn(*items[i % len(items)])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps, out

    line = dict(tool='ttabench', batch=B, workload=args.workload, voxel_size=args.voxel_size, train_first=int(opts['--train-first']),
                reps=reps)
    dt, res = timed(model.simple_test, simple)
    line['simple_test_scenes_per_s'] = round(B / dt, 1)
    line['simple_test_survivors_per_scene'] = round(sum(len(r['scores_3d']) for r in res) / B, 1)
    for A in AUGS:
        dt, res = timed(model.aug_test, inputs[A])
        line[f'aug_test_A{A}_scenes_per_s'] = round(B / dt, 1)
        line[f'aug_test_A{A}_ms_per_batch'] = round(1e3 * dt, 2)
        line[f'aug_test_A{A}_survivors_after_merge_per_scene'] = round(sum(len(r['scores_3d']) for r in res) / B, 1)
        # merge-stage device time and the survivors entering the merge, from separate (un-timed) calls
        nh.merge_events = []
        before = []
        orig = nh._first_stage

        def first_stage(*a, **kw):
            out = orig(*a, **kw)
            before.append(int(out[4].sum()))
            return out
        nh._first_stage = first_stage
        try:
            with torch.no_grad():
                for i in range(reps):
                    model.aug_test(*inputs[A][i % len(inputs[A])])
            torch.cuda.synchronize()
        finally:
            del nh._first_stage
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in nh.merge_events)
        nh.merge_events = None
        line[f'aug_test_A{A}_merge_ms_per_batch'] = round(ms[len(ms) // 2], 3)
        line[f'aug_test_A{A}_survivors_before_merge_per_scene'] = round(sum(before) / len(before) / B, 1)
    line['aug_test_A4_vs_simple_test'] = round(line['aug_test_A4_scenes_per_s'] / line['simple_test_scenes_per_s'], 3)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
