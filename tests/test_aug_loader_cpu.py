"""CPU: test-time augmentation batches from resident scenes (data.parse_aug_pipeline, data.AugDeviceLoader, runner.build_val_loader)
on the reference's ScanNet test pipeline with flip=True, both BEV flips and pts_scale_ratio=[1.0, 0.95] — host logic only, no
kernel runs."""
import copy

import numpy as np
import pytest
import torch

from fcaf3d_amd import data as DT
from fcaf3d_amd import pipelines as PP
from tests.test_fit_cpu import make_cfg, pipelines

RATIOS = [1.0, 0.95]


def tta_pipeline(num_points=4000, ratios=RATIOS, **over):
    """the single-augmentation test pipeline of tests/test_fit_cpu.py with MultiScaleFlipAug3D asking for flips and scales"""
    _, test = pipelines(num_points)
    test = copy.deepcopy(test)
    test[-1].update(dict(flip=True, pcd_horizontal_flip=True, pcd_vertical_flip=True, pts_scale_ratio=ratios), **over)
    return test


@pytest.fixture(scope='module')
def resident(tmp_path_factory):
    cfg = make_cfg(tmp_path_factory.mktemp('aug'), val=True)
    ds = DT.build_dataset(cfg.data.val)
    return DT.ResidentScenes(ds, 'cpu'), ds


def test_augmentation_list_and_metas_equal_the_reference_pipeline(resident):
    rs, ds = resident
    test = tta_pipeline()
    P, augs = DT.parse_aug_pipeline(test)
    assert augs == [(r, h, v) for r in RATIOS for h in (False, True) for v in (False, True)] and len(augs) == 8
    assert P == DT.parse_pipeline(pipelines()[1]) and not P['train'] and P['num_points'] == 4000 and P['align']
    # pipelines.MultiScaleFlipAug3D + collate_aug on the same scenes: the loop order and the metas the merge reads
    pipe = PP.Compose(test)
    idx = [4, 1, 6]
    np.random.seed(0)
    ref = PP.collate_aug([pipe(ds.pre_pipeline(i)) for i in idx])
    ld = DT.AugDeviceLoader(rs, test, 3, seed=5)
    bt = ld.batch(0, np.asarray(idx))
    assert len(bt['img_metas']) == len(ref['img_metas']) == 8 and all(len(m) == 3 for m in bt['img_metas'])
    for a in range(8):
        for b, i in enumerate(idx):
            got, want = bt['img_metas'][a][b], ref['img_metas'][a][b]
            for k in ('pcd_scale_factor', 'pcd_horizontal_flip', 'pcd_vertical_flip', 'sample_idx', 'box_type_3d', 'pts_filename'):
                assert got[k] == want[k] and type(got[k]) is type(want[k]), (a, b, k, got[k], want[k])
            assert (got['pcd_scale_factor'], got['pcd_horizontal_flip'], got['pcd_vertical_flip']) == augs[a]
            assert got['dataset_index'] == i
    # the points: A lists of B scenes over ONE flat batch, copy a of scene b at descriptor a * B + b
    pts = bt['points']
    assert len(pts) == 8 and all(len(pa) == 3 for pa in pts) and isinstance(pts.flat, DT.DeviceBatch) and len(pts.flat) == 24
    assert all(pts[a][b] is pts.flat[a * 3 + b] and pts[a][b].shape == (4000, 6) for a in range(8) for b in range(3))
    assert bt.keys() == {'points', 'img_metas'}
    # a pipeline without MultiScaleFlipAug3D's flips: one identity augmentation
    assert DT.parse_aug_pipeline(pipelines()[1])[1] == [(1.0, False, False)]
    assert DT.parse_aug_pipeline(tta_pipeline(ratios=1, pcd_vertical_flip=False))[1] == [(1.0, False, False), (1.0, True, False)]


def test_descriptors_copy_zero_is_the_plain_loader_and_every_copy_draws_its_own_sample(resident):
    rs, ds = resident
    test = tta_pipeline()
    plain = DT.DeviceLoader(rs, pipelines()[1], 3, seed=5)
    ld = DT.AugDeviceLoader(rs, test, 3, seed=5)
    assert len(ld) == len(plain) == 3 and not ld.shuffle and list(ld.indices(0)) == list(plain.indices(0)) == list(range(7))
    A = 8
    seeds = []
    for bt, pb in zip(ld.batches(0), plain.batches(0)):
        d, B = bt['points'].flat.desc, len(pb['points'])
        assert d.shape == (A * B, DT.DESC_WORDS)
        # augmentation 0 is the identity: copy 0's descriptor words are DeviceLoader's (same rows, same sample seed, same transform)
        assert np.array_equal(d[:B], pb['points'].desc)
        # output offsets back to back in descriptor order
        assert np.array_equal(d[:, 3], np.concatenate([[0], np.cumsum(d[:-1, 2])])) and (d[:, 2] == 4000).all()
        xf = d[:, 6:].copy().view(np.float32)
        for a, (s, h, v) in enumerate(ld.augs):
            sl = slice(a * B, (a + 1) * B)
            assert np.array_equal(d[sl, :2], d[:B, :2])                               # the same scenes' rows of the arena
            assert (xf[sl, 13] == float(h)).all() and (xf[sl, 14] == float(v)).all() and (xf[sl, 17] == np.float32(s)).all()
            assert (xf[sl, 15] == 1.0).all() and (xf[sl, 16] == 0.0).all() and (xf[sl, 18:21] == 0.0).all() and (xf[sl, 12] == 1.0).all()
        seeds.extend(d[:, 4].view(np.uint64).tolist())
    assert len(seeds) == 8 * 7 and len(set(seeds)) == len(seeds)                       # pairwise distinct
    again = [s for bt in DT.AugDeviceLoader(rs, test, 3, seed=5).batches(3) for s in bt['points'].flat.desc[:, 4].view(np.uint64).tolist()]
    assert again == seeds                                                              # reproducible, in every epoch
    assert ld.draw(0, 4, 5)['sample_seed'] == ld.draw(9, 4, 5)['sample_seed'] == DT.draw(ld.P, 5, 5, 4)['sample_seed']
    assert ld.draw(0, 4)['sample_seed'] == plain.draw(0, 4)['sample_seed']
    other = [s for bt in DT.AugDeviceLoader(rs, test, 3, seed=6).batches(0) for s in bt['points'].flat.desc[:, 4].view(np.uint64).tolist()]
    assert not set(other) & set(seeds)
    # ranks shard the scenes as DeviceLoader does
    assert [list(DT.AugDeviceLoader(rs, test, 2, seed=5, rank=r, world_size=2).indices(0)) for r in range(2)] == [[0, 2, 4, 6], [1, 3, 5]]


def test_more_than_256_copies_in_a_launch_is_refused(resident):
    rs, _ = resident
    test = tta_pipeline(ratios=[1.0])                                                  # A = 4
    DT.AugDeviceLoader(rs, test, 64)                                                   # 256 copies: the kernel's limit
    with pytest.raises(ValueError, match=r'4 augmentations x samples_per_gpu=65 = 260 .* 256'):
        DT.AugDeviceLoader(rs, test, 65)
    one = tta_pipeline(ratios=[1.0], flip=False)
    with pytest.raises(ValueError, match=r'1 augmentations x samples_per_gpu=257 = 257 .* 256'):
        DT.AugDeviceLoader(rs, one, 257)


def test_unsupported_steps_are_named_and_parse_pipeline_still_refuses():
    test = tta_pipeline()
    bad = copy.deepcopy(test)
    bad[-1]['transforms'].insert(2, dict(type='PointShuffle'))
    with pytest.raises(NotImplementedError, match="'PointShuffle'"):
        DT.parse_aug_pipeline(bad)
    with pytest.raises(NotImplementedError, match="2 entries in 'img_scale'"):
        DT.parse_aug_pipeline(tta_pipeline(img_scale=[(1333, 800), (666, 400)]))
    DT.parse_aug_pipeline(tta_pipeline(img_scale=[(1333, 800)]))
    noflip = copy.deepcopy(test)
    noflip[-1]['transforms'] = [t for t in noflip[-1]['transforms'] if t['type'] != 'RandomFlip3D']
    with pytest.raises(NotImplementedError, match="'RandomFlip3D'"):
        DT.parse_aug_pipeline(noflip)
    # the single-augmentation parser is what it was: the same dict is refused by name
    with pytest.raises(NotImplementedError, match='MultiScaleFlipAug3D'):
        DT.parse_pipeline(test)
    with pytest.raises(NotImplementedError, match='MultiScaleFlipAug3D'):
        DT.parse_pipeline([dict(pipelines()[1][-1], flip=True)])


def test_fits_validation_loader_helper_picks_the_loader(resident):
    from fcaf3d_amd.runner import build_val_loader
    rs, _ = resident
    single = build_val_loader(rs, pipelines()[1], 2, seed=3)
    assert type(single) is DT.DeviceLoader and not single.P['train'] and single.seed == 3
    tta = build_val_loader(rs, tta_pipeline(ratios=1), 2, 3, 1, 2)
    assert type(tta) is DT.AugDeviceLoader and len(tta.augs) == 4 and (tta.seed, tta.rank, tta.world_size) == (3, 1, 2)
    assert type(build_val_loader(rs, tta_pipeline(ratios=RATIOS, flip=False), 2)) is DT.AugDeviceLoader          # two scales, no flip
    assert type(build_val_loader(rs, tta_pipeline(ratios=[1.0], flip=False), 2)) is DT.DeviceLoader


def test_evaluate_takes_nested_metas_through_the_augmented_route(monkeypatch):
    """runner.evaluate on batches whose img_metas is nested: extract_feat on the flat batch, get_bboxes_aug with the nested metas, the
    next batch's `.flat` prefetched before this batch is collected — with a stub model, on the CPU"""
    from fcaf3d_amd import runner

    calls = []

    class Head:
        def get_bboxes_aug(self, tag, img_metas):
            calls.append(('aug', tag, len(img_metas), len(img_metas[0])))
            t = torch.zeros(0)
            return [(torch.zeros((0, 7)), t, t.long()) for _ in img_metas[0]]

    class Model(torch.nn.Module):
        neck_with_head = Head()

        def extract_feat(self, points, img_metas):
            calls.append(('feat', points.tag, len(points), len(img_metas)))
            return (points.tag,)

        def prefetch(self, points, gt=True):
            calls.append(('prefetch', points.tag, gt))

        def invalidate_images(self):
            pass

    class Flat(list):
        pass

    def batch(tag, B):
        flat = Flat(range(2 * B))
        flat.tag = tag
        pts = DT.AugBatch(flat, 2, B)
        return pts, [[dict(pcd_horizontal_flip=bool(a)) for _ in range(B)] for a in range(2)]

    seen = {}

    def fake_eval(gt_annos, dets, metric, label2cat, scene_ids=None, group=None):
        seen['n'] = len(dets)
        return dict(ok=1)
    import fcaf3d_amd.evaluation as EV
    monkeypatch.setattr(EV, 'indoor_eval_device', fake_eval)             # (evaluate imports it when called)
    res = runner.evaluate(Model(), iter([batch('x', 2), batch('y', 2), batch('z', 1)]), [dict(gt_num=0)] * 5)
    assert res == dict(ok=1) and seen['n'] == 5
    assert calls == [('feat', 'x', 4, 4), ('prefetch', 'y', False), ('aug', 'x', 2, 2),
                     ('feat', 'y', 4, 4), ('prefetch', 'z', False), ('aug', 'y', 2, 2),
                     ('feat', 'z', 2, 2), ('aug', 'z', 2, 1)]
