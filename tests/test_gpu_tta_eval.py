"""-m gpu: scoring test-time augmentation.  data.AugDeviceLoader batches (all A * B copies from the resident arena in one launch)
against the per-copy path, aug_test on them, box voting in the batched merge against the per-scene merge, runner.evaluate on nested
metas and fit with a flip=True validation pipeline — at the model scale of tests/test_gpu_tta.py: 3 synthetic scenes of 20 000
points written as .bin + infos, the 3-level ScanNet and SUN RGB-D models."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from fcaf3d_amd import data as DT
from fcaf3d_amd import pipelines as PP
from tests.test_aug_loader_cpu import tta_pipeline
from tests.test_fit_cpu import CLASSES, make_cfg, pipelines, write_dataset
from tests.test_gpu_tta import SUNRGBD_KW, _build

pytestmark = pytest.mark.gpu
NUM_POINTS = 16000                 # of 20 000: every copy really samples
VOTE_THR = 0.6
SEED = 4


def _write_sunrgbd(root):
    """3 single-view scenes with rotated boxes in the layout of the reference's SUN RGB-D infos (no axis alignment, 7-column boxes)"""
    from fcaf3d_amd.synthetic import make_scene
    os.makedirs(os.path.join(root, 'points'), exist_ok=True)
    infos = []
    for k in range(3):
        pts, gt, lab = make_scene(71 + k, n_points=20000, **SUNRGBD_KW)
        pts.astype(np.float32).tofile(os.path.join(root, 'points', f'{k:06d}.bin'))
        annos = dict(gt_num=len(gt), name=np.array([str(i) for i in lab]), gt_boxes_upright_depth=gt.astype(np.float32),
                     **{'class': lab.astype(np.int64)})
        infos.append(dict(point_cloud=dict(num_features=6, lidar_idx=k), pts_path=f'points/{k:06d}.bin', annos=annos))
    ann = os.path.join(root, 'infos_val.pkl')
    with open(ann, 'wb') as f:
        pickle.dump(infos, f)
    return ann


@pytest.fixture(scope='module', params=['scannet', 'sunrgbd'])
def setup(request, tmp_path_factory):
    """model (eval), resident validation set, the A = 4 flip loader over it (2 scenes per batch: batches of 2 and 1 scenes)"""
    dev = torch.device('cuda:0')
    root = tmp_path_factory.mktemp(request.param)
    if request.param == 'scannet':
        ann = write_dataset(root, sizes=(20000, 20000, 20000), empty=(), name='infos_val.pkl', seed0=400)
        test = tta_pipeline(NUM_POINTS, ratios=1)
        ds = DT.build_dataset(dict(type='ScanNetDataset', data_root=str(root), ann_file=ann, pipeline=test, classes=CLASSES, test_mode=True))
        model, _ = _build('fcaf3d_scannet-3d-18class')
    else:
        ann = _write_sunrgbd(root)
        test = copy.deepcopy(pipelines(NUM_POINTS, align=False)[1])
        test[-1].update(flip=True, pcd_horizontal_flip=True, pcd_vertical_flip=True)
        ds = DT.build_dataset(dict(type='SUNRGBDDataset', data_root=str(root), ann_file=ann, pipeline=test, test_mode=True))
        model, _ = _build('fcaf3d_sunrgbd-3d-10class')
    rs = DT.ResidentScenes(ds, dev)
    ld = DT.AugDeviceLoader(rs, test, 2, seed=SEED)
    assert ld.augs == [(1.0, False, False), (1.0, False, True), (1.0, True, False), (1.0, True, True)]
    return dict(name=request.param, dev=dev, model=model.to(dev).eval(), rs=rs, ld=ld, test=test, ds=ds, batches=ld.batches(0))


def _count_calls(monkeypatch):
    """every native entry point called from here on, by name, in order"""
    names, real = [], L.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(L, 'call', call)
    return names


def _per_copy_points(s, bt):
    """the copies of a batch as plain tensors: the rows the launch sampled (sample_out), then the reference's transforms one copy at a
    time in torch — GlobalAlignment, RandomFlip3D, GlobalRotScaleTrans — in the kernel's order"""
    rs, dev, flat = s['rs'], s['dev'], bt['points'].flat
    total = sum(p.shape[0] for p in flat)
    coords = torch.empty((total, 4), dtype=torch.int32, device=dev)
    feats = torch.empty((total, 3), dtype=torch.float32, device=dev)
    rows = torch.empty(total, dtype=torch.int32, device=dev)
    flat.voxelize_batch(s['model'].voxel_size, 255.0, coords, feats, sample_out=rows)
    metas = [m for ma in bt['img_metas'] for m in ma]
    out, o = [], 0
    for d, (p, meta) in enumerate(zip(flat, metas)):
        k = int(rs.slot[meta['dataset_index']])
        n = p.shape[0]
        raw = rs.arena[int(rs.start[k]):int(rs.start[k]) + int(rs.count[k])]
        r = rows[o:o + n].long()
        assert len(torch.unique(r)) == n == NUM_POINTS and int(r.max()) < int(rs.count[k])      # n distinct rows of the scene
        q = raw[r]
        if s['ld'].P['align']:
            q = PP.global_alignment(q, rs.align[k])
        none = q.new_zeros((0, 7))
        if meta['pcd_horizontal_flip']:
            q, _ = PP.flip_bev(q, none, 'horizontal', True)
        if meta['pcd_vertical_flip']:
            q, _ = PP.flip_bev(q, none, 'vertical', True)
        q, _ = PP.rot_scale_trans(q, none, 0.0, meta['pcd_scale_factor'], [0.0, 0.0, 0.0], True)
        out.append(q.contiguous())
        o += n
    return out, (coords, feats, rows)


def test_flat_batch_equals_the_per_copy_path_in_one_launch(setup, monkeypatch):
    """(a)"""
    s = setup
    model = s['model']
    for bt in s['batches']:
        A, B = len(bt['points']), len(bt['points'][0])
        assert A == 4 and len(bt['points'].flat) == A * B
        copies, (c0, f0, rows) = _per_copy_points(s, bt)
        names = _count_calls(monkeypatch)
        coords, feats = model.voxelize(bt['points'].flat)
        assert names == ['fc_batch_augment_voxelize']                                  # the whole input stage: ONE launch
        monkeypatch.undo()
        assert torch.equal(coords, c0) and torch.equal(feats, f0)
        c1, f1 = model.voxelize(copies)                                                # fc_voxelize per copy
        assert torch.equal(coords, c1) and torch.equal(feats, f1)
        assert coords[:, 0].unique().tolist() == list(range(A * B))
        # every copy of a scene draws its own rows
        n = NUM_POINTS
        for b in range(B):
            picks = [rows[(a * B + b) * n:(a * B + b + 1) * n] for a in range(A)]
            assert all(not torch.equal(picks[0], p) for p in picks[1:])
    # copy 0 is the scene the single-augmentation loader gives
    plain = DT.DeviceLoader(s['rs'], [dict(st, flip=False) if st['type'] == 'MultiScaleFlipAug3D' else st for st in s['test']], 2, seed=SEED)
    bt, pb = s['batches'][0], plain.batches(0)[0]
    ca, fa_ = model.voxelize(bt['points'][0])
    cp, fp = model.voxelize(pb['points'])
    assert torch.equal(ca, cp) and torch.equal(fa_, fp)


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x['scores_3d']) > 10
        assert torch.equal(x['scores_3d'], y['scores_3d']) and torch.equal(x['labels_3d'], y['labels_3d'])
        assert torch.equal(x['boxes_3d'].tensor, y['boxes_3d'].tensor)


def test_aug_test_through_flat_equals_aug_test_on_plain_tensors(setup, monkeypatch):
    """(b)"""
    s = setup
    model = s['model']
    bt = s['batches'][0]
    A, B = 4, 2
    copies, _ = _per_copy_points(s, bt)
    plain = [[copies[a * B + b] for b in range(B)] for a in range(A)]
    with torch.no_grad():
        names = _count_calls(monkeypatch)
        got = model.aug_test(bt['points'], bt['img_metas'])
        assert names.count('fc_batch_augment_voxelize') == 1 and 'fc_voxelize' not in names and 'fc_augment_voxelize' not in names
        monkeypatch.undo()
        ref = model.aug_test(plain, bt['img_metas'])
        fwd = model(return_loss=False, points=bt['points'], img_metas=bt['img_metas'])
    _same_results(got, ref)
    _same_results(fwd, ref)


def _vote_scale(nh, per, metas_b, thr):
    """per final row of one scene's merge, max_{j in M} |box_j[k]| (k = 0..5): the members of every kept box restated from the
    mapped-back candidates of its class (nms.nms_bev, nms.boxes_iou_bev); within a class the merge keeps the NMS's order"""
    from fcaf3d_amd.boxes import bbox3d_mapping_back
    from fcaf3d_amd.merge_augs import aug_params, merge_cfg
    from fcaf3d_amd.nms import boxes_iou_bev, nms_bev
    rb = [bbox3d_mapping_back(p[0], *aug_params(m)) for p, m in zip(per, metas_b)]
    boxes = rb[0].cat(rb)
    scores, labels = torch.cat([p[1] for p in per]), torch.cat([p[2] for p in per]).long()
    nms_thr, rotated, _ = merge_cfg(nh.test_cfg, boxes.with_yaw)
    out = {}
    for c in range(int(labels.max()) + 1):
        ids = labels == c
        if not ids.any():
            continue
        t, sc = boxes.tensor[ids], scores[ids]
        keep = nms_bev(t, sc, nms_thr, rotated=rotated, stable=True)
        mem = boxes_iou_bev(t[keep], t, rotated=rotated) >= torch.tensor(thr, dtype=torch.float32, device=t.device)
        mem[torch.arange(len(keep), device=t.device), keep] = True
        out[c] = (torch.where(mem[:, :, None], t[None, :, :6].abs().double(), t.new_zeros((), dtype=torch.float64)).amax(1), mem.sum(1))
    return out


def test_voting_in_the_batched_merge_equals_the_per_scene_merge(setup, monkeypatch):
    """(c)"""
    from fcaf3d_amd.merge_augs import merge_aug_single
    s = setup
    model, nh = s['model'], s['model'].neck_with_head
    bt = s['batches'][0]
    metas = bt['img_metas']
    A, B = 4, 2
    assert nh.test_cfg.get('vote_thr') is None
    try:
        with torch.no_grad():
            x = list(model.extract_feat(bt['points'].flat, [m for ma in metas for m in ma]))
            names = _count_calls(monkeypatch)
            plain = nh.get_bboxes_aug(*x, metas)
            today = names[names.index('fc_merge_sorted_segments'):]
            assert today == ['fc_merge_sorted_segments', 'fc_nms_bev', 'fc_merge_sorted_segments']          # no voting: today's launches
            nh.test_cfg['vote_thr'] = None
            del names[:]
            none = nh.get_bboxes_aug(*x, metas)
            assert names[names.index('fc_merge_sorted_segments'):] == today
            nh.test_cfg['vote_thr'] = VOTE_THR
            del names[:]
            nh.vote_members = []
            got = nh.get_bboxes_aug(*x, metas)
            assert names[names.index('fc_merge_sorted_segments'):] == ['fc_merge_sorted_segments', 'fc_nms_bev', 'fc_vote_boxes',
                                                                       'fc_merge_sorted_segments']
            monkeypatch.undo()
            per = [nh._get_bboxes_single([l[i] for l in x[0]], [l[i] for l in x[1]], [l[i] for l in x[2]], [l[i] for l in x[3]],
                                         metas[i // B][i % B]) for i in range(A * B)]
            moved = members = kept = 0
            for b in range(B):
                mine = [per[a * B + b] for a in range(A)]
                mb = [metas[a][b] for a in range(A)]
                ref = merge_aug_single([dict(boxes_3d=p[0], scores_3d=p[1], labels_3d=p[2]) for p in mine], mb, nh.test_cfg)
                gb, gs, gl = got[b]
                pb, ps, pl_ = plain[b]
                nb, ns, nl = none[b]
                # vote_thr None is vote_thr absent, bit for bit
                assert torch.equal(nb.tensor, pb.tensor) and torch.equal(ns, ps) and torch.equal(nl, pl_)
                # voting changes geometry only: counts, scores, labels and order are the un-voted merge's, and the yaws
                assert len(gs) == len(ps) > 10 and torch.equal(gs, ps) and torch.equal(gl, pl_)
                assert gb.tensor.shape == pb.tensor.shape and (gb.tensor.shape[1] < 7 or torch.equal(gb.tensor[:, 6], pb.tensor[:, 6]))
                # batched == per scene: counts, scores and labels bit-equal, boxes under 2^-23 * max_{j in M} |box_j[k]|
                assert torch.equal(gs, ref[1]) and torch.equal(gl, ref[2]) and gb.with_yaw == ref[0].with_yaw
                scale = _vote_scale(nh, mine, mb, VOTE_THR)
                bound = torch.zeros((len(gs), 6), dtype=torch.float64, device=gs.device)
                for c, (sc_c, cnt_c) in scale.items():
                    rows = (gl == c).nonzero()[:, 0]
                    assert len(rows) == len(sc_c)
                    bound[rows] = sc_c * 2.0 ** -23
                    members += int(cnt_c.sum())
                    kept += len(rows)
                err = (gb.tensor[:, :6].double() - ref[0].tensor[:, :6].double()).abs()
                assert (err <= bound).all(), float((err - bound).max())
                assert torch.equal(gb.tensor[:, 6:], ref[0].tensor[:, 6:])
                moved += int((gb.tensor[:, :6] != pb.tensor[:, :6]).any(1).sum())
            # the kernel's own member counts say the same
            mem, kc = nh.vote_members[0]
            valid = torch.arange(mem.shape[1], device=mem.device)[None, :] < kc[:, None]
            assert int(valid.sum()) == kept and int(mem[valid].sum()) == members
            print(f'{s["name"]}: {kept} kept boxes, {members / kept:.2f} members each, {moved} boxes moved by the vote')
            assert moved > 10 and members > kept
    finally:
        nh.test_cfg.pop('vote_thr', None)
        nh.vote_members = None


def _hand_eval(model, batches, annos, metric=(0.25, 0.5)):
    from fcaf3d_amd.evaluation import indoor_eval_device
    dets = []
    with torch.no_grad():
        for bt in batches:
            x = model.extract_feat(bt['points'].flat, [m for ma in bt['img_metas'] for m in ma])
            dets.extend(model.neck_with_head.get_bboxes_aug(*x, bt['img_metas']))
    torch.cuda.synchronize()
    return indoor_eval_device(annos, dets, metric, None), dets


@pytest.mark.parametrize('vote', [None, VOTE_THR])
def test_evaluate_over_the_aug_loader_equals_a_hand_loop(setup, vote):
    """(d)"""
    from fcaf3d_amd.runner import evaluate, validate
    s = setup
    model, nh = s['model'], s['model'].neck_with_head
    annos = s['ds'].gt_annos()
    assert len(annos) == 3 and [len(b['img_metas'][0]) for b in s['batches']] == [2, 1]
    try:
        if vote is not None:
            nh.test_cfg['vote_thr'] = vote
        want, dets = _hand_eval(model, s['batches'], annos)
        assert all(len(d[1]) > 10 for d in dets)
        got = evaluate(model, ((b['points'], b['img_metas']) for b in s['ld'].batches(0)), annos)
        assert {'mAP_0.25', 'mAR_0.25', 'mAP_0.50', 'mAR_0.50'} <= set(got) and list(got) == list(want)
        np.testing.assert_equal(got, want)
        np.testing.assert_equal(validate(model, s['ld']), want)
        assert not model.training
    finally:
        nh.test_cfg.pop('vote_thr', None)


def test_fit_with_a_flip_validation_pipeline_logs_what_validate_gives(tmp_path):
    """(e) two epochs of fit on the two-level model of tests/test_gpu_fit.py whose validation pipeline says flip=True: the loader is
    the augmenting one, and the 'val' records equal validate called by hand on the saved checkpoints"""
    import fcaf3d_amd as fa
    from fcaf3d_amd import fit, load_checkpoint
    from fcaf3d_amd.runner import build_val_loader, validate
    from tests.test_gpu_dist import _model
    dev = torch.device('cuda:0')
    cfg = make_cfg(tmp_path / 'data', val=True, log_config=dict(interval=1), checkpoint_config=dict(interval=1, max_keep_ckpts=2))
    cfg.data.val['pipeline'] = tta_pipeline(4000, ratios=1)
    model = _model(fa)[0].to(dev).train()
    rec = fit(model, cfg, str(tmp_path / 'work'), seed=7)
    torch.cuda.synchronize()
    assert model.training
    val = [r for r in rec if r['mode'] == 'val']
    assert [r['epoch'] for r in val] == [1, 2] and [r['mode'] for r in rec] == ['train'] * 3 + ['val'] + ['train'] * 3 + ['val']
    vs = DT.build_dataset(cfg.data.val)
    ld = build_val_loader(DT.ResidentScenes(vs, dev), vs.pipeline, 2, 7)
    assert type(ld) is DT.AugDeviceLoader and len(ld.augs) == 4 and len(vs) == 7
    for r in val:
        m = _model(fa)[0].to(dev).train()
        load_checkpoint(m, str(tmp_path / 'work' / f'epoch_{r["epoch"]}.pth'), map_location=dev, strict=True)
        res = validate(m, ld)
        assert {'mAP_0.25', 'mAR_0.25', 'mAP_0.50', 'mAR_0.50'} <= set(res)
        got = {k: v for k, v in r.items() if k not in ('mode', 'epoch', 'iter', 'lr')}
        assert set(got) == set(res)
        np.testing.assert_equal(got, {k: float(v) for k, v in res.items()})
        want, _ = _hand_eval(m.eval(), ld.batches(0), vs.gt_annos())
        np.testing.assert_equal(res, want)
