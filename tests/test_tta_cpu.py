"""CPU: test-time augmentation pieces that need no GPU — MultiScaleFlipAug3D's augmentation sequence and random draws
(mmdet3d/datasets/pipelines/test_time_aug.py:77-107), the box methods and bbox3d_mapping_back (core/bbox/transforms.py:4-23)
against their closed forms."""
import itertools
import math
import os
import warnings

import numpy as np
import torch

from fcaf3d_amd.boxes import DepthInstance3DBoxes

G = os.path.join(os.path.dirname(__file__), 'golden')


class _Record:
    """a transform that records the augmentation fields it is handed"""
    seen = []

    def __call__(self, results):
        _Record.seen.append(tuple(results[k] for k in ('scale', 'flip', 'pcd_scale_factor', 'flip_direction',
                                                       'pcd_horizontal_flip', 'pcd_vertical_flip')))
        return dict(points=results['points'], img_metas=dict(n=len(_Record.seen)))


def _restated(img_scale, pts_scale_ratio, flip, flip_direction, h, v):
    """test_time_aug.py:77-107, restated"""
    img_scale = img_scale if isinstance(img_scale, list) else [img_scale]
    ratios = pts_scale_ratio if isinstance(pts_scale_ratio, list) else [float(pts_scale_ratio)]
    dirs = flip_direction if isinstance(flip_direction, list) else [flip_direction]
    out = []
    for scale in img_scale:
        for r in ratios:
            for f in ([True] if flip else [False]):
                for hh in ([False, True] if flip and h else [False]):
                    for vv in ([False, True] if flip and v else [False]):
                        for d in dirs:
                            out.append((scale, f, r, d, hh, vv))
    return out


def test_multiscale_flip_aug3d_sequence():
    from fcaf3d_amd.pipelines import PIPELINES, MultiScaleFlipAug3D
    PIPELINES.register_module(name='TTARecord', force=True)(_Record)
    for flip, h, v, ratios, dirs, scales in itertools.product(
            (False, True), (False, True), (False, True), (1, [1.0, 0.95], [0.9, 1.0, 1.1]), ('horizontal', ['horizontal', 'vertical']),
            ((1333, 800), [(1333, 800), (800, 600)])):
        _Record.seen = []
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t = MultiScaleFlipAug3D([dict(type='TTARecord')], scales, ratios, flip=flip, flip_direction=dirs,
                                    pcd_horizontal_flip=h, pcd_vertical_flip=v)
        pts = torch.arange(12.).reshape(4, 3)
        results = dict(points=pts, sample_idx=3)
        out = t(results)
        want = _restated(scales, ratios, flip, dirs, h, v)
        assert _Record.seen == want
        assert set(out) == {'points', 'img_metas'} and len(out['points']) == len(want)
        assert results == dict(points=pts, sample_idx=3) and torch.equal(pts, torch.arange(12.).reshape(4, 3))   # untouched
        assert all(p is not pts for p in out['points'])                                                          # deep copies


def _tta_pipe(n_points):
    from fcaf3d_amd.pipelines import Compose
    return Compose([
        dict(type='LoadPointsFromFile', coord_type='DEPTH', load_dim=6, use_dim=[0, 1, 2, 3, 4, 5]),
        dict(type='MultiScaleFlipAug3D', img_scale=(1333, 800), pts_scale_ratio=[1.0, 0.95], flip=True, pcd_horizontal_flip=True,
             pcd_vertical_flip=True,
             transforms=[dict(type='GlobalRotScaleTrans', rot_range=[0, 0], scale_ratio_range=[1., 1.], translation_std=[0.1, 0.1, 0.1]),
                         dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
                         dict(type='IndoorPointSample', num_points=n_points),
                         dict(type='DefaultFormatBundle3D', class_names=('a',), with_label=False),
                         dict(type='Collect3D', keys=['points'])])])


def test_multiscale_flip_aug3d_draws():
    """Every augmentation takes the reference's draws in the reference's order — GlobalRotScaleTrans: rotation, (no scale draw:
    pcd_scale_factor is preset), translation; RandomFlip3D: no image-flip draw (`flip` is preset), no BEV draws (preset);
    IndoorPointSample: the choice — replayed here from the same seed."""
    from fcaf3d_amd.boxes import DepthInstance3DBoxes as D
    from fcaf3d_amd.pipelines import load_points_from_file
    path = os.path.join(G, 'scannet_scene0000_00.bin')
    raw = load_points_from_file(path, 6, (0, 1, 2, 3, 4, 5))
    np.random.seed(11)
    out = _tta_pipe(500)(dict(pts_filename=path, sample_idx=0, bbox3d_fields=[], box_type_3d=D))
    np.random.seed(11)
    k = 0
    for s in (1.0, 0.95):
        for h in (False, True):
            for v in (False, True):
                angle = np.random.uniform(0, 0)
                assert angle == 0
                trans = np.random.normal(scale=np.array([0.1, 0.1, 0.1], dtype=np.float32), size=3)
                choice = np.random.choice(raw.shape[0], 500, replace=raw.shape[0] < 500)
                meta = out['img_metas'][k]
                assert (meta['pcd_scale_factor'], meta['pcd_horizontal_flip'], meta['pcd_vertical_flip']) == (s, h, v)
                assert np.array_equal(meta['pcd_trans'], trans)
                p = raw.clone()
                p[:, :3] = p[:, :3] * s + torch.from_numpy(trans.astype(np.float32))
                if h:
                    p[:, 0] = -p[:, 0]
                if v:
                    p[:, 1] = -p[:, 1]
                assert torch.allclose(out['points'][k], p[torch.from_numpy(choice)], atol=1e-5), k
                k += 1
    assert k == len(out['points']) == 8
    # nothing else was drawn: the next draw equals the reference stream's next draw
    nxt = np.random.rand()
    np.random.seed(11)
    _tta_pipe(500)(dict(pts_filename=path, sample_idx=0, bbox3d_fields=[], box_type_3d=D))
    assert np.random.rand() == nxt


def test_random_flip3d_image_draw_only_without_flip():
    """mmdet's RandomFlip draws only when `flip` is not in results: train pipelines (no `flip`) keep their three draws"""
    from fcaf3d_amd.pipelines import RandomFlip3D
    f = RandomFlip3D(sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5)
    pts = torch.zeros((3, 6))
    np.random.seed(3)
    r = f(dict(points=pts.clone(), bbox3d_fields=[]))
    np.random.seed(3)
    np.random.rand()
    assert r['pcd_horizontal_flip'] == bool(np.random.rand() < 0.5)
    assert r['pcd_vertical_flip'] == bool(np.random.rand() < 0.5)
    np.random.seed(3)
    r = f(dict(points=pts.clone(), bbox3d_fields=[], flip=True))
    np.random.seed(3)
    assert r['pcd_horizontal_flip'] == bool(np.random.rand() < 0.5)
    assert r['pcd_vertical_flip'] == bool(np.random.rand() < 0.5)


def _rand_boxes(n, yaw, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(n, 7, generator=g)
    t[:, 3:6] = t[:, 3:6].abs() + 0.1
    return DepthInstance3DBoxes(t if yaw else t[:, :6], box_dim=7 if yaw else 6, with_yaw=yaw)


def test_box_methods_closed_forms():
    pi32 = torch.tensor(math.pi, dtype=torch.float32)
    for yaw in (False, True):
        b = _rand_boxes(20, yaw)
        t0 = b.tensor.clone()
        c = b.clone()
        assert torch.equal(c.tensor, t0) and c.tensor.data_ptr() != b.tensor.data_ptr() and c.with_yaw == yaw
        c.flip('horizontal')
        want = t0.clone(); want[:, 0] = -t0[:, 0]
        if yaw:
            want[:, 6] = -t0[:, 6] + pi32
        assert torch.equal(c.tensor, want)
        c = b.clone(); c.flip('vertical')
        want = t0.clone(); want[:, 1] = -t0[:, 1]
        if yaw:
            want[:, 6] = -t0[:, 6]
        assert torch.equal(c.tensor, want)
        c = b.clone(); c.scale(1 / 0.95)
        f = torch.tensor(1 / 0.95, dtype=torch.float32)
        want = t0.clone(); want[:, :6] = t0[:, :6] * f
        assert torch.equal(c.tensor, want)
        assert torch.equal(b.tensor, t0)                                    # clones: the original is untouched
        cat = DepthInstance3DBoxes.cat([b, c])
        assert torch.equal(cat.tensor, torch.cat([t0, want])) and cat.with_yaw == yaw and len(cat) == 40
        if not yaw:
            assert (cat.tensor[:, 6] == 0).all()


def test_bbox3d_mapping_back_closed_form():
    from fcaf3d_amd.boxes import bbox3d_mapping_back
    pi32 = torch.tensor(math.pi, dtype=torch.float32)
    for yaw in (False, True):
        b = _rand_boxes(30, yaw, seed=1)
        t0 = b.tensor.clone()
        for s, h, v in itertools.product((1.0, 0.95, 1.1), (False, True), (False, True)):
            m = bbox3d_mapping_back(b, s, h, v)
            want = t0.clone()
            if h:
                want[:, 0] = -want[:, 0]
                if yaw:
                    want[:, 6] = -want[:, 6] + pi32
            if v:
                want[:, 1] = -want[:, 1]
                if yaw:
                    want[:, 6] = -want[:, 6]
            want[:, :6] = want[:, :6] * torch.tensor(1 / s, dtype=torch.float32)
            assert torch.equal(m.tensor, want), (s, h, v, yaw)
            assert m.with_yaw == yaw
            assert torch.equal(b.tensor, t0)
