"""-m gpu: test-time augmentation — the merge kernel (csrc_post/merge.hip) bit for bit against cat + stable sort + mapping-back,
the batched merge (Fcaf3DNeckWithHead.get_bboxes_aug) bit for bit against the per-scene merge_aug_bboxes_3d, and aug_test end to
end against the CPU oracle (eval mode)."""
import os

import numpy as np
import pytest
import torch

import fcaf3d_amd as fa
from fcaf3d_amd.boxes import DepthInstance3DBoxes
from fcaf3d_amd.synthetic import make_scene
from oracle import bev, model_oracle as MO

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
SUNRGBD_KW = dict(rotated=True, single_view=True, rgb_unit=True, n_boxes=6, n_classes=10)
# (pcd_scale_factor, pcd_horizontal_flip, pcd_vertical_flip) of the augmentations used below
FLIPS4 = [(1.0, False, False), (1.0, False, True), (1.0, True, False), (1.0, True, True)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _rel(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max()) / max(1e-3, float(b.abs().max()))


def _build(name, voxel_size=0.02, n_levels=3, seed=0):
    torch.manual_seed(seed)
    cfg = fa.get_config(name, voxel_size=voxel_size)
    m = cfg.model
    m.backbone['n_outs'] = n_levels
    m.neck_with_head['in_channels'] = (64, 128, 256, 512)[:n_levels]
    m.neck_with_head.assigner['n_scales'] = n_levels
    model = fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg'))
    with torch.no_grad():
        model.neck_with_head.cls_conv.bias.fill_(0.0)         # as test_simple_test_parity: random init scores below score_thr
        model.neck_with_head.cls_conv.kernel.normal_(0, 0.3)
    return model, m


def _augment(p, s, h, v):
    """GlobalRotScaleTrans (scale) then RandomFlip3D (flips) on a (n, 6) fp32 CPU point tensor: the same fp32 operations on
    whichever side runs them"""
    q = p.clone()
    q[:, :3] = q[:, :3] * s
    if h:
        q[:, 0] = -q[:, 0]
    if v:
        q[:, 1] = -q[:, 1]
    return q


def _meta(s, h, v):
    return dict(box_type_3d=DepthInstance3DBoxes, pcd_scale_factor=s, pcd_horizontal_flip=h, pcd_vertical_flip=v)


def _aug_batch(pts, augs, dev):
    """points[a][b] (device) and img_metas[a][b] of numpy scenes `pts` under the augmentations `augs`"""
    points = [[_augment(torch.from_numpy(p), *aug).to(dev) for p in pts] for aug in augs]
    metas = [[_meta(*aug) for _ in pts] for aug in augs]
    return points, metas


def _scenes(seeds, **kw):
    return [make_scene(s, **kw)[0] for s in seeds]


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------
def _kernel_case(rng, nseg_out, K, lens, R, flags, cap, stride_out, dev):
    from fcaf3d_amd.merge_augs import merge_sorted_segments, transform_word
    nin = nseg_out * K
    # per input segment a table of R rows; scores quantised to force ties inside and across lists
    scores = torch.from_numpy(rng.integers(0, 40, size=(nin, R)).astype(np.float32) / 40)
    boxes = torch.from_numpy(rng.normal(size=(nin, R, 7)).astype(np.float32))
    boxes[:, :, 3:6] = boxes[:, :, 3:6].abs() + 0.1
    order = torch.empty((nin, R), dtype=torch.int64)
    keep = torch.zeros((nin, R), dtype=torch.int32)
    counts = torch.zeros(nin, dtype=torch.int32)
    xf, ref = [], []
    for g in range(nin):
        order[g] = torch.sort(scores[g], descending=True, stable=True).indices
        n = int(lens[g])
        pos = np.sort(rng.choice(R, size=n, replace=False)) if n else np.zeros(0, np.int64)
        keep[g, :n] = torch.from_numpy(pos.astype(np.int32))
        counts[g] = n
        aug = (float(rng.choice([1.0, 0.95, 1.07])), bool(rng.integers(2)), bool(rng.integers(2)))
        xf.append(transform_word(*aug))
        rows = order[g, torch.from_numpy(pos.astype(np.int64))]
        b = boxes[g, rows]
        with_yaw = bool(flags & 2)
        bb = DepthInstance3DBoxes(b, with_yaw=with_yaw, origin=(.5, .5, .5) if flags & 1 else (.5, .5, 0))
        ref.append((fa.boxes.bbox3d_mapping_back(bb, *aug).tensor, scores[g, rows], g % K, torch.arange(n)))
    g = np.arange(nin, dtype=np.int64)
    desc = torch.from_numpy(np.stack((g, g * R, g * R, np.array(xf, dtype=np.int64)), -1)).to(dev)
    lens_o = counts.view(nseg_out, K).sum(1)
    max_total = int(lens_o.max())
    ob, os_, osrc, oc = merge_sorted_segments(desc, K, counts.to(dev), scores.to(dev), boxes.to(dev), max_total=max_total,
                                              stride_out=stride_out, keep=keep.to(dev), keep_stride=R, order=order.to(dev),
                                              order_stride=R, flags=flags, cap=cap)
    oc = oc.cpu()
    for o in range(nseg_out):
        parts = ref[o * K:(o + 1) * K]
        rb = torch.cat([p[0] for p in parts]); rs = torch.cat([p[1] for p in parts])
        rk = torch.cat([torch.full((len(p[1]),), p[2], dtype=torch.int32) for p in parts])
        rp = torch.cat([p[3].to(torch.int32) for p in parts])
        srt = torch.sort(rs, descending=True, stable=True).indices
        lim = min(stride_out, cap if cap >= 0 else stride_out)
        srt = srt[:lim]
        n = len(srt)
        assert int(oc[o]) == n, (o, int(oc[o]), n)
        assert torch.equal(os_[o, :n].cpu(), rs[srt])
        assert torch.equal(ob[o, :n].cpu(), rb[srt]), (o, (ob[o, :n].cpu() - rb[srt]).abs().max())
        assert torch.equal(osrc[o, :n, 0].cpu(), rk[srt]) and torch.equal(osrc[o, :n, 1].cpu(), rp[srt])


@pytest.mark.parametrize('K', [1, 2, 4, 8, 18, 70])
def test_merge_sorted_segments_bit_exact(K):
    dev = _dev()
    rng = np.random.default_rng(K)
    nseg_out = 3
    for flags in (0, 1, 2, 3):
        R = 4000 if K <= 8 else 600
        lens = rng.integers(0, R + 1, size=nseg_out * K)
        lens[rng.random(nseg_out * K) < 0.25] = 0                  # empty lists
        if K >= 18:
            lens[1] = R                                             # one long list among many short ones
        lens[:K] = 0 if flags == 2 else lens[:K]                    # output segment 0 with every list empty
        total = int(lens.reshape(nseg_out, K).sum(1).max())
        _kernel_case(rng, nseg_out, K, lens, R, flags, -1, max(1, total), dev)                    # no cap
        _kernel_case(rng, nseg_out, K, lens, R, flags, max(0, total // 3), max(1, total), dev)   # cap below the total
        _kernel_case(rng, nseg_out, K, lens, R, flags, total + 5, total + 7, dev)                # cap above the total


def test_merge_sorted_segments_all_empty():
    dev = _dev()
    rng = np.random.default_rng(5)
    _kernel_case(rng, 2, 4, np.zeros(8, np.int64), 16, 3, -1, 1, dev)


# ---- 3. batched == per scene -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kw', [('fcaf3d_scannet-3d-18class', {}), ('fcaf3d_sunrgbd-3d-10class', SUNRGBD_KW)])
def test_get_bboxes_aug_equals_per_scene_merge(name, kw):
    from fcaf3d_amd.merge_augs import merge_aug_single
    dev = _dev()
    model, _ = _build(name)
    model = model.to(dev).eval()
    pts = _scenes([31, 32, 33], n_points=20000, **kw)
    augs = [(1.0, False, False), (1.0, True, False), (0.95, False, True), (1.05, True, True)]
    points, metas = _aug_batch(pts, augs, dev)
    A, B = len(augs), len(pts)
    nh = model.neck_with_head
    with torch.no_grad():
        x = list(model.extract_feat([p for pa in points for p in pa], [m for ma in metas for m in ma]))
        got = nh.get_bboxes_aug(*x, metas)
        per = [nh._get_bboxes_single([l[i] for l in x[0]], [l[i] for l in x[1]], [l[i] for l in x[2]], [l[i] for l in x[3]],
                                     metas[i // B][i % B]) for i in range(A * B)]
    assert len(got) == B
    for b in range(B):
        assert all(len(per[a * B + b][1]) > 10 for a in range(A))
        ref = merge_aug_single([dict(boxes_3d=per[a * B + b][0], scores_3d=per[a * B + b][1], labels_3d=per[a * B + b][2])
                                for a in range(A)], [metas[a][b] for a in range(A)], nh.test_cfg)
        gb, gs, gl = got[b]
        assert len(gs) == len(ref[1]) > 0
        assert gb.with_yaw == ref[0].with_yaw
        assert torch.equal(gl, ref[2])
        assert torch.equal(gs, ref[1])
        assert torch.equal(gb.tensor, ref[0].tensor)


# ---- 4. identity TTA ---------------------------------------------------------------------------------------------------
def test_identity_aug_test_is_simple_test_sorted():
    dev = _dev()
    model, _ = _build('fcaf3d_sunrgbd-3d-10class')
    model = model.to(dev).eval()
    pts = [torch.from_numpy(p).to(dev) for p in _scenes([41, 42], n_points=20000, **SUNRGBD_KW)]
    metas = [_meta(1.0, False, False) for _ in pts]
    with torch.no_grad():
        ref = model.simple_test(pts, metas)
        got = model.aug_test([pts], [metas])
    assert len(got) == len(ref) == 2
    for r, g in zip(ref, got):
        assert len(r['scores_3d']) > 10
        o = torch.sort(r['scores_3d'], descending=True, stable=True).indices
        assert torch.equal(g['scores_3d'], r['scores_3d'][o])
        assert torch.equal(g['labels_3d'], r['labels_3d'][o])
        assert torch.equal(g['boxes_3d'].tensor, r['boxes_3d'].tensor[o])


# ---- 5. a result merged with its exact mirror --------------------------------------------------------------------------
@pytest.mark.parametrize('with_yaw', [False, True])
def test_merge_with_mirror_returns_the_result_sorted(with_yaw):
    from fcaf3d_amd.merge_augs import merge_aug_bboxes_3d
    dev = _dev()
    rng = np.random.default_rng(7)
    n = 40
    t = np.zeros((n, 7), np.float32)
    t[:, 0] = np.arange(n) * 3.0 - 60.0                           # far apart: no two boxes of R overlap
    t[:, 1] = rng.normal(size=n); t[:, 2] = rng.normal(size=n)
    t[:, 3:6] = rng.uniform(0.5, 1.5, size=(n, 3))
    t[:, 6] = rng.uniform(-3, 3, size=n) if with_yaw else 0
    scores = torch.from_numpy(rng.permutation(n).astype(np.float32) / n + 0.01).to(dev)
    labels = torch.from_numpy(rng.integers(0, 5, size=n)).to(dev)
    r = DepthInstance3DBoxes(torch.from_numpy(t if with_yaw else t[:, :6]).to(dev), box_dim=7 if with_yaw else 6, with_yaw=with_yaw)
    mirror = r.clone()
    mirror.flip('horizontal')
    cfg = dict(nms_pre=1000, iou_thr=0.5, score_thr=0.01)
    res = merge_aug_bboxes_3d([dict(boxes_3d=r, scores_3d=scores, labels_3d=labels),
                               dict(boxes_3d=mirror, scores_3d=scores, labels_3d=labels)],
                              [dict(), dict(pcd_horizontal_flip=True)], cfg)
    o = torch.sort(scores, descending=True, stable=True).indices
    assert torch.equal(res['scores_3d'], scores[o].cpu())
    assert torch.equal(res['labels_3d'], labels[o].cpu())
    assert torch.equal(res['boxes_3d'].tensor, r.tensor[o].cpu())


# ---- 6. end to end against the oracle ------------------------------------------------------------------------------------
def _oracle_merge(per_aug, augs, tc, yaw):
    """merge_augs.py on numpy / torch CPU tensors with the oracle's BEV NMS (decision 1: pcdet semantics)"""
    bs, ss, ls = [], [], []
    for (b, s, l), aug in zip(per_aug, augs):
        b7 = b if b.shape[1] == 7 else torch.cat([b, torch.zeros_like(b[:, :1])], 1)
        bb = DepthInstance3DBoxes(b7, with_yaw=yaw, origin=(.5, .5, .5))
        bs.append(fa.boxes.bbox3d_mapping_back(bb, *aug).tensor); ss.append(s); ls.append(l)
    b, s, l = torch.cat(bs), torch.cat(ss), torch.cat(ls)
    mb, ms, ml = [], [], []
    for c in range(int(l.max()) + 1 if len(l) else 0):
        ids = (l == c).nonzero()[:, 0]
        if len(ids) == 0:
            continue
        keep = torch.from_numpy(bev.nms(b[ids].numpy(), s[ids].numpy(), tc['iou_thr'], rotated=yaw))
        mb.append(b[ids][keep]); ms.append(s[ids][keep]); ml.append(l[ids][keep])
    mb, ms, ml = torch.cat(mb), torch.cat(ms), torch.cat(ml)
    o = torch.from_numpy(np.argsort(-ms.numpy(), kind='stable'))
    return mb[o], ms[o], ml[o]


def _oracle_params(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize('name,kw', [('fcaf3d_scannet-3d-18class', {}), ('fcaf3d_sunrgbd-3d-10class', SUNRGBD_KW)])
def test_aug_test_vs_oracle(name, kw):
    dev = _dev()
    model, m = _build(name)
    P = _oracle_params(model)
    model = model.to(dev).eval()
    pts = _scenes([51, 52], n_points=20000, **kw)
    augs = [(s, h, v) for s in (1.0, 0.95) for (_, h, v) in FLIPS4]
    points, metas = _aug_batch(pts, augs, dev)
    with torch.no_grad():
        got = model.aug_test(points, metas)
    yaw = m.neck_with_head.get('n_reg_outs', 6) == 8
    MO.TRAINING = False
    try:
        per = [MO.simple_test(P, m, [_augment(torch.from_numpy(p), *aug).numpy() for p in pts]) for aug in augs]
    finally:
        MO.TRAINING = True
    for b in range(len(pts)):
        rb, rs, rl = _oracle_merge([per[a][b] for a in range(len(augs))], augs, m['test_cfg'], yaw)
        g = got[b]
        assert len(rs) > 10
        assert len(g['scores_3d']) == len(rs)
        assert (g['scores_3d'][1:] <= g['scores_3d'][:-1]).all()
        assert _rel(g['scores_3d'], rs) < 1e-4                    # the descending score sequences
        # scores of different classes may lie closer than the fp32 distance of the two routes (equal arithmetic, another order):
        # compare class-major, each class by descending score (the merge NMS's own output order)
        og = torch.sort(g['labels_3d'], stable=True).indices
        orf = torch.sort(rl, stable=True).indices
        assert torch.equal(g['labels_3d'][og], rl[orf])
        assert _rel(g['scores_3d'][og], rs[orf]) < 1e-4
        assert _rel(g['boxes_3d'].tensor[og], rb[orf]) < 1e-4
        print(f'{name} scene {b}: {len(rs)} boxes, {int((g["labels_3d"] != rl).sum())} places where the final order swaps '
              'near-equal scores of different classes')


# ---- 7. forward(return_loss=False) dispatch --------------------------------------------------------------------------------
def test_forward_test_dispatches_augmentations():
    dev = _dev()
    model, _ = _build('fcaf3d_scannet-3d-18class')
    model = model.to(dev).eval()
    pts = _scenes([61, 62], n_points=20000)
    points, metas = _aug_batch(pts, FLIPS4, dev)
    with torch.no_grad():
        a = model(return_loss=False, points=points, img_metas=metas)
        b = model.aug_test(points, metas)
        s1 = model(return_loss=False, points=points[:1], img_metas=metas[:1])
        s2 = model.simple_test(points[0], metas[0])
    assert len(a) == len(b) == len(s1) == len(s2) == 2
    for x, y in list(zip(a, b)) + list(zip(s1, s2)):
        assert len(x['scores_3d']) > 0
        assert torch.equal(x['scores_3d'], y['scores_3d']) and torch.equal(x['labels_3d'], y['labels_3d'])
        assert torch.equal(x['boxes_3d'].tensor, y['boxes_3d'].tensor)


# ---- 8. from a .bin file through the test pipeline --------------------------------------------------------------------------
def test_pipeline_to_aug_test_from_bin():
    from fcaf3d_amd.pipelines import Compose, collate_aug
    dev = _dev()
    model, _ = _build('fcaf3d_scannet-3d-18class')
    model = model.to(dev).eval()
    pipe = Compose([
        dict(type='LoadPointsFromFile', coord_type='DEPTH', load_dim=6, use_dim=[0, 1, 2, 3, 4, 5]),
        dict(type='MultiScaleFlipAug3D', img_scale=(1333, 800), pts_scale_ratio=1, flip=True, pcd_horizontal_flip=True,
             pcd_vertical_flip=True,
             transforms=[dict(type='GlobalRotScaleTrans', rot_range=[0, 0], scale_ratio_range=[1., 1.], translation_std=[0, 0, 0]),
                         dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
                         dict(type='IndoorPointSample', num_points=20000),
                         dict(type='DefaultFormatBundle3D', class_names=tuple(range(18)), with_label=False),
                         dict(type='Collect3D', keys=['points'])])], device=dev)
    np.random.seed(0)
    samples = [pipe(dict(pts_filename=os.path.join(G, 'scannet_scene0000_00.bin'), sample_idx=i, bbox3d_fields=[],
                         box_type_3d=DepthInstance3DBoxes)) for i in range(2)]
    batch = collate_aug(samples)
    assert len(batch['points']) == 4 and all(p.is_cuda for pa in batch['points'] for p in pa)
    with torch.no_grad():
        res = model(return_loss=False, **batch)
    assert len(res) == 2
    for r in res:
        assert len(r['scores_3d']) > 0
        assert torch.isfinite(r['boxes_3d'].tensor).all() and torch.isfinite(r['scores_3d']).all()
        assert (r['scores_3d'][1:] <= r['scores_3d'][:-1]).all()
