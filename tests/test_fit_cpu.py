"""CPU: fcaf3d_amd.data (datasets, epoch order, draws, pipeline parsing, the resident arena) and runner.fit's host logic with a stub
model — no kernel runs.  The synthetic dataset written here (info .pkl + .bin scenes in the reference's layout, from
synthetic.make_scene) is the one tests/test_gpu_fit.py trains on."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from fcaf3d_amd import data as DT
from fcaf3d_amd.registry import _wrap

CLASSES = tuple(f'c{i}' for i in range(18))


def pipelines(num_points=4000, align=True):
    load = dict(type='LoadPointsFromFile', coord_type='DEPTH', shift_height=False, use_color=True, load_dim=6, use_dim=[0, 1, 2, 3, 4, 5])
    ga = [dict(type='GlobalAlignment', rotation_axis=2)] if align else []
    train = [load, dict(type='LoadAnnotations3D', with_bbox_3d=True, with_label_3d=True)] + ga + [
        dict(type='IndoorPointSample', num_points=num_points),
        dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
        dict(type='GlobalRotScaleTrans', rot_range=[-0.087266, 0.087266], scale_ratio_range=[.9, 1.1], translation_std=[.1, .1, .1],
             shift_height=False),
        dict(type='DefaultFormatBundle3D', class_names=CLASSES),
        dict(type='Collect3D', keys=['points', 'gt_bboxes_3d', 'gt_labels_3d'])]
    test = [load] + ga + [dict(type='MultiScaleFlipAug3D', img_scale=(1333, 800), pts_scale_ratio=1, flip=False, transforms=[
        dict(type='GlobalRotScaleTrans', rot_range=[0, 0], scale_ratio_range=[1., 1.], translation_std=[0, 0, 0]),
        dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
        dict(type='IndoorPointSample', num_points=num_points),
        dict(type='DefaultFormatBundle3D', class_names=CLASSES, with_label=False),
        dict(type='Collect3D', keys=['points'])])]
    return train, test


def write_dataset(root, sizes=(6000, 6000, 6000, 3000, 6000, 6000, 6000), empty=(2,), name='infos_train.pkl', seed0=300):
    """scenes of synthetic.make_scene as .bin files + an info .pkl in the layout of the reference's tools/create_data.py: the raw
    points are the scene moved by (+3, +2.5, 0), the axis-alignment matrix moves them back (a translation), boxes are aligned"""
    from fcaf3d_amd.synthetic import make_scene
    os.makedirs(os.path.join(root, 'points'), exist_ok=True)
    shift = np.array([3.0, 2.5, 0.0], np.float32)
    align = np.eye(4, dtype=np.float32)
    align[:3, 3] = -shift
    infos = []
    for k, n in enumerate(sizes):
        pts, gt, lab = make_scene(seed0 + k, n_points=n)
        raw = pts.astype(np.float32).copy()
        raw[:, :3] += shift
        raw.tofile(os.path.join(root, 'points', f'{k:04d}.bin'))
        annos = dict(gt_num=0, axis_align_matrix=align) if k in empty else \
            dict(gt_num=len(gt), name=np.array([CLASSES[i] for i in lab]), gt_boxes_upright_depth=gt[:, :6].astype(np.float32),
                 **{'class': lab.astype(np.int64)}, axis_align_matrix=align)
        infos.append(dict(point_cloud=dict(num_features=6, lidar_idx=f'scene{k:04d}'), pts_path=f'points/{k:04d}.bin', annos=annos))
    with open(os.path.join(root, name), 'wb') as f:
        pickle.dump(infos, f)
    return os.path.join(root, name)


def make_cfg(root, num_points=4000, samples_per_gpu=2, max_epochs=2, val=False, **over):
    train, test = pipelines(num_points)
    ann = os.path.join(root, 'infos_train.pkl')
    if not os.path.exists(ann):                       # (several ranks of a test share one directory: written once, by the parent)
        write_dataset(root)
    cfg = dict(
        data=dict(samples_per_gpu=samples_per_gpu, workers_per_gpu=0,
                  train=dict(type='RepeatDataset', times=1, dataset=dict(type='ScanNetDataset', data_root=str(root), ann_file=ann,
                                                                         pipeline=train, filter_empty_gt=True, classes=CLASSES,
                                                                         box_type_3d='Depth'))),
        optimizer=dict(type='AdamW', lr=0.001, weight_decay=0.0001),
        optimizer_config=dict(grad_clip=dict(max_norm=10, norm_type=2)),
        lr_config=dict(policy='step', warmup=None, step=[1]),
        runner=dict(type='EpochBasedRunner', max_epochs=max_epochs),
        checkpoint_config=dict(interval=1, max_keep_ckpts=1),
        log_config=dict(interval=2),
        evaluation=dict(interval=0))
    if val:
        cfg['data']['val'] = dict(type='ScanNetDataset', data_root=str(root), ann_file=ann, pipeline=test, classes=CLASSES, test_mode=True,
                                  box_type_3d='Depth')
        cfg['evaluation'] = dict(interval=1)
    cfg.update(over)
    return _wrap(cfg)


class Stub(torch.nn.Module):
    """a model with the detector's call surface whose loss depends on the weights and on which scenes it is shown"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(-1, 1, 8))
        self.seen = []

    def forward(self, return_loss=True, points=None, gt_bboxes_3d=None, gt_labels_3d=None, img_metas=None):
        assert return_loss and len(points) == len(gt_bboxes_3d) == len(gt_labels_3d) == len(img_metas)
        self.seen.append([m['dataset_index'] for m in img_metas])
        t = sum(float(b.tensor.sum()) for b in gt_bboxes_3d) / 1000.0
        return dict(loss_a=((self.w - t) ** 2).sum(), loss_b=self.w.abs().sum() * 0.1, aux=torch.tensor(1.0))


# ---- data ----------------------------------------------------------------------------------------------------------------------------------
def test_epoch_order_is_a_padded_permutation_sharded_by_rank():
    n, spg = 7, 2
    for world in (1, 2, 3):
        for epoch in (0, 1, 5):
            order = DT.epoch_order(n, 11, epoch, spg, world)
            g = torch.Generator(); g.manual_seed(11 + epoch)
            perm = torch.randperm(n, generator=g).numpy()
            unit = world * spg
            assert len(order) == -(-n // unit) * unit and len(order) % unit == 0
            assert np.array_equal(order[:n], perm) and np.array_equal(order[n:], perm[:len(order) - n])      # padded by wrapping
            shards = [order[r::world] for r in range(world)]
            assert all(len(s) == len(order) // world and len(s) % spg == 0 for s in shards)
            assert np.array_equal(np.sort(np.concatenate(shards)), np.sort(order))
        assert not np.array_equal(DT.epoch_order(n, 11, 0, spg, world), DT.epoch_order(n, 11, 1, spg, world))
    assert np.array_equal(DT.epoch_order(5, 0, 3, 2, 2, shuffle=False), np.arange(5))
    # an unshuffled TRAINING order is padded as well (every rank the same number of full steps); a validation order never is
    assert np.array_equal(DT.epoch_order(5, 0, 3, 2, 2, shuffle=False, pad=True), [0, 1, 2, 3, 4, 0, 1, 2])
    assert np.array_equal(DT.epoch_order(5, 0, 3, 2, 2, shuffle=True, pad=False), DT.epoch_order(5, 0, 3, 2, 2)[:5])


def test_datasets_wrappers_and_filter_empty_gt(tmp_path):
    train, test = pipelines()
    ann = write_dataset(tmp_path)
    base = dict(type='ScanNetDataset', data_root=str(tmp_path), ann_file=ann, pipeline=train, classes=CLASSES, box_type_3d='Depth')
    full = DT.build_dataset(dict(base, filter_empty_gt=False))
    kept = DT.build_dataset(dict(base, filter_empty_gt=True))
    assert len(full) == 7 and len(kept) == 6
    assert [i['point_cloud']['lidar_idx'] for i in kept.data_infos] == [f'scene{k:04d}' for k in (0, 1, 3, 4, 5, 6)]
    assert len(DT.build_dataset(dict(base, test_mode=True))) == 7                     # a validation set keeps every scene
    rep = DT.build_dataset(dict(type='RepeatDataset', times=3, dataset=dict(base)))
    assert len(rep) == 18 and all(rep.scene(i) == (rep.dataset, i % 6) for i in range(18))
    with pytest.raises(IndexError):
        rep.scene(18)
    cat = DT.build_dataset(dict(type='ConcatDataset', datasets=[dict(base), dict(base, filter_empty_gt=False)]))
    assert len(cat) == 13
    assert cat.scene(0) == (cat.datasets[0], 0) and cat.scene(5) == (cat.datasets[0], 5)
    assert cat.scene(6) == (cat.datasets[1], 0) and cat.scene(12) == (cat.datasets[1], 6)
    nested = DT.build_dataset(dict(type='RepeatDataset', times=2, dataset=dict(type='ConcatDataset', datasets=[dict(base), dict(base)])))
    assert len(nested) == 24 and nested.scene(19)[1] == 1
    assert len(DT.build_dataset(dict(base, ann_file=[ann, ann]))) == 12               # a list of info files: one dataset each
    with pytest.raises(KeyError):
        DT.build_dataset(dict(base, type='KittiDataset'))
    # the resident arena stores a scene once however many indices name it; raw points, alignment kept per scene
    rs = DT.ResidentScenes(rep, 'cpu')
    assert len(rs) == 18 and rs.arena.shape == (5 * 6000 + 3000, 6) and list(rs.count) == [6000, 6000, 3000, 6000, 6000, 6000]
    assert np.array_equal(rs.slot, np.arange(18) % 6)
    raw = np.fromfile(tmp_path / 'points' / '0003.bin', np.float32).reshape(-1, 6)
    assert np.array_equal(rs.arena[int(rs.start[2]):int(rs.start[2]) + 3000].numpy(), raw)
    assert rs.align[0].shape == (4, 4) and rs.boxes[0].shape[1] == 7 and len(rs.boxes[0]) == len(rs.labels[0]) > 0
    with pytest.raises(MemoryError, match='does not fit'):
        DT.ResidentScenes(rep, 'cpu', max_gb=1e-4)


def test_draws_are_a_pure_function_of_seed_epoch_and_index(tmp_path):
    cfg = make_cfg(tmp_path)
    ds = DT.build_dataset(cfg.data.train)
    rs = DT.ResidentScenes(ds, 'cpu')
    a = DT.DeviceLoader(rs, ds.pipeline, 2, seed=5)
    b = DT.DeviceLoader(rs, ds.pipeline, 2, seed=5)
    for _ in range(3):
        b.draw(0, 1)                                                   # draws made before do not matter
    assert a.draw(3, 4) == b.draw(3, 4)
    seen = {json.dumps(a.draw(e, i), sort_keys=True) for e in range(3) for i in range(6)}
    assert len(seen) == 18                                             # every (epoch, index) has its own
    assert a.draw(3, 4) != DT.DeviceLoader(rs, ds.pipeline, 2, seed=6).draw(3, 4)
    d = [a.draw(e, i) for e in range(40) for i in range(6)]
    P = a.P
    assert P['num_points'] == 4000 and P['align'] and P['train'] and (P['flip_h'], P['flip_v']) == (0.5, 0.5)
    assert all(P['rot_range'][0] <= x['angle'] <= P['rot_range'][1] and 0.9 <= x['scale'] <= 1.1 for x in d)
    assert 0.3 < np.mean([x['flip_h'] for x in d]) < 0.7 and 0.3 < np.mean([x['flip_v'] for x in d]) < 0.7
    assert 0.05 < np.std([x['trans'][0] for x in d]) < 0.15
    # the same epoch twice gives the same batches (descriptor tables, boxes, metas), another epoch others
    x, y, z = a.batches(1), b.batches(1), a.batches(2)
    assert len(x) == len(a) == 3 and all(len(bt['points']) == 2 for bt in x)
    assert all(np.array_equal(p['points'].desc, q['points'].desc) for p, q in zip(x, y))
    assert all(torch.equal(g.tensor, h.tensor) for p, q in zip(x, y) for g, h in zip(p['gt_bboxes_3d'], q['gt_bboxes_3d']))
    assert not all(np.array_equal(p['points'].desc, q['points'].desc) for p, q in zip(x, z))
    pts = x[0]['points']
    assert pts[0].shape == (4000, 6) and pts[0].device == torch.device('cpu') and hasattr(pts[0], 'voxelize_into') and hasattr(pts, 'voxelize_batch')
    assert list(pts.desc[:, 3]) == [0, 4000] and list(pts.desc[:, 2]) == [4000, 4000]
    # the validation pipeline: fixed draws, nothing random but the sample
    _, test = pipelines()
    v = DT.DeviceLoader(rs, test, 2, seed=5)
    assert not v.P['train'] and not v.shuffle and v.draw(0, 3) == v.draw(7, 3)
    dv = v.draw(0, 3)
    assert (dv['flip_h'], dv['flip_v'], dv['angle'], dv['scale'], dv['trans']) == (False, False, 0.0, 1.0, [0.0, 0.0, 0.0])
    assert 'gt_bboxes_3d' not in v.batches(0)[0]
    t = [DT.DeviceLoader(rs, ds.pipeline, 2, seed=5, rank=r, world_size=4, shuffle=False).indices(0) for r in range(4)]
    assert [list(x) for x in t] == [[0, 4], [1, 5], [2, 0], [3, 1]]          # 6 scenes, unshuffled training: padded to 8
    assert [len(DT.DeviceLoader(rs, test, 2, seed=5, rank=r, world_size=4).indices(0)) for r in range(4)] == [2, 2, 1, 1]


def test_rotation_is_drawn_but_not_applied_without_boxes(tmp_path):
    train, _ = pipelines()
    ann = write_dataset(tmp_path)
    ds = DT.build_dataset(dict(type='ScanNetDataset', data_root=str(tmp_path), ann_file=ann, pipeline=train, filter_empty_gt=False))
    ld = DT.DeviceLoader(DT.ResidentScenes(ds, 'cpu'), train, 7, seed=1, shuffle=False)
    bt = ld.batches(0)[0]
    xf = bt['points'].desc[:, 6:].copy().view(np.float32)
    assert ld.draw(0, 2)['angle'] != 0.0
    assert (xf[2, 15], xf[2, 16]) == (1.0, 0.0) and all(xf[k, 16] != 0.0 for k in (0, 1, 3))
    assert len(bt['gt_bboxes_3d'][2]) == 0 and xf[:, 12].all()


def test_unsupported_pipeline_step_is_named():
    train, test = pipelines()
    with pytest.raises(NotImplementedError, match="'PointShuffle'"):
        DT.parse_pipeline(train[:4] + [dict(type='PointShuffle')] + train[4:])
    with pytest.raises(NotImplementedError, match='RandomFlip3D'):
        DT.parse_pipeline([dict(type='RandomFlip3D', sync_2d=True)])
    with pytest.raises(NotImplementedError, match='MultiScaleFlipAug3D'):
        DT.parse_pipeline([dict(test[-1], flip=True)])
    assert DT.parse_pipeline(test)['num_points'] == 4000


# ---- runner ----------------------------------------------------------------------------------------------------------------------------------
def test_lr_values_with_and_without_warmup():
    from fcaf3d_amd.runner import build_lr_updater
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=0.01)
    plain = build_lr_updater(opt, dict(policy='step', warmup=None, step=[2, 3]))
    got = []
    for e in range(4):
        plain.set_epoch(e)
        plain.set_iter(e * 10)                                          # a no-op without warm-up
        got.append(opt.param_groups[0]['lr'])
    assert np.allclose(got, [0.01, 0.01, 0.001, 0.0001], rtol=1e-12)
    opt = torch.optim.SGD([w], lr=0.01)
    up = build_lr_updater(opt, dict(policy='step', warmup='linear', warmup_iters=4, warmup_ratio=0.25, step=[1]))
    lrs, it = [], 0
    for e in range(2):
        up.set_epoch(e)
        for _ in range(3):
            up.set_iter(it)
            lrs.append(opt.param_groups[0]['lr'])
            it += 1
    # mmcv: warmup_lr = regular_lr * (1 - (1 - it / warmup_iters) * (1 - warmup_ratio)) with the CURRENT epoch's regular rate
    k = [1 - (1 - i / 4) * 0.75 for i in range(4)]
    assert np.allclose(lrs, [0.01 * k[0], 0.01 * k[1], 0.01 * k[2], 0.001 * k[3], 0.001, 0.001], rtol=1e-12)
    with pytest.raises(KeyError):
        build_lr_updater(opt, dict(policy='step', warmup='exp', warmup_iters=4, step=[1]))


def test_fit_checkpoints_rotate_logs_on_cadence_and_resumes(tmp_path):
    from fcaf3d_amd import fit, load_checkpoint
    cfg = make_cfg(tmp_path / 'data', max_epochs=4, lr_config=dict(policy='step', warmup='linear', warmup_iters=4, warmup_ratio=0.5, step=[2]))
    work = tmp_path / 'work'
    torch.manual_seed(0)
    model = Stub()
    seen = []
    rec = fit(model, cfg, str(work), seed=3, device='cpu', on_batch=lambda e, it, b: seen.append((e, it)))
    # 6 scenes (one of 7 has no boxes), 2 per batch: 3 steps per epoch; log interval 2: a line at step 2 and at the epoch's end
    assert seen == [(e, 3 * e + k) for e in range(4) for k in range(3)]
    assert [(r['epoch'], r['iter']) for r in rec] == [(e, i) for e in range(1, 5) for i in (2, 3)] and all(r['mode'] == 'train' for r in rec)
    assert all({'lr', 'loss', 'loss_a', 'loss_b', 'aux', 'grad_norm', 'time', 'data_time'} <= set(r) for r in rec)
    assert all(abs(r['loss'] - r['loss_a'] - r['loss_b']) < 1e-5 * abs(r['loss']) for r in rec)      # `aux` is logged, not trained on
    k = [1 - (1 - i / 4) * 0.5 for i in range(4)]
    assert np.allclose([r['lr'] for r in rec], [0.001 * k[1], 0.001 * k[2], 0.001, 0.001, 1e-4, 1e-4, 1e-4, 1e-4], rtol=1e-9)
    logs = [f for f in os.listdir(work) if f.endswith('.log.json')]
    assert len(logs) == 1 and [json.loads(l) for l in open(work / logs[0])] == rec
    # max_keep_ckpts=1: the last epoch's file and latest.pth
    assert sorted(f for f in os.listdir(work) if f.endswith('.pth')) == ['epoch_4.pth', 'latest.pth']
    ck = load_checkpoint(Stub(), str(work / 'latest.pth'), map_location='cpu')
    assert ck['meta']['epoch'] == 4 and ck['meta']['iter'] == 12 and ck['meta']['seed'] == 3 and 'optimizer' in ck
    no_empty = {i for b in model.seen for i in b}
    assert no_empty == set(range(6)) and all(len(b) == 2 for b in model.seen)
    # two epochs, then two more from the checkpoint in a fresh model: the straight run's weights, batches and iteration count
    cfg2 = make_cfg(tmp_path / 'data', max_epochs=2, lr_config=cfg.lr_config, checkpoint_config=dict(interval=1, max_keep_ckpts=3))
    torch.manual_seed(0)
    first = Stub()
    fit(first, cfg2, str(tmp_path / 'w2'), seed=3, device='cpu')
    assert sorted(f for f in os.listdir(tmp_path / 'w2') if f.endswith('.pth')) == ['epoch_1.pth', 'epoch_2.pth', 'latest.pth']
    second = Stub()
    with torch.no_grad():
        second.w.zero_()
    cfg2.runner['max_epochs'] = 4
    rec2 = fit(second, cfg2, str(tmp_path / 'w2'), seed=3, device='cpu', resume_from=str(tmp_path / 'w2' / 'latest.pth'))
    assert torch.equal(second.w, model.w)
    assert first.seen + second.seen == model.seen
    assert [(r['epoch'], r['iter']) for r in rec2] == [(e, i) for e in (3, 4) for i in (2, 3)]
    assert load_checkpoint(Stub(), str(tmp_path / 'w2' / 'latest.pth'), map_location='cpu')['meta']['iter'] == 12
    assert sorted(f for f in os.listdir(tmp_path / 'w2') if f.endswith('.pth')) == ['epoch_2.pth', 'epoch_3.pth', 'epoch_4.pth', 'latest.pth']
