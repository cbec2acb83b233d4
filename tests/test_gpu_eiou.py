"""GPU: the enclosing-box losses GIoU3DLoss / DIoU3DLoss (csrc_post/eiou.hip, fc_eiou3d_fwd_bwd) against the float64 fixture
tests/golden/eiou3d.npz, against the IoU kernels, over sizes and weight patterns, as modules, and in the head."""
import functools

import numpy as np
import pytest
import torch

from tests.test_eiou_cpu import GROUPS, KINDS, PATTERNS, SIZES, check_against_fixture, fixture, pattern_weight

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda', torch.cuda.current_device())


def _fn(kind):
    import fcaf3d_amd as fa
    return fa.giou_3d if kind == 'giou' else fa.diou_3d


def _module(kind, **kw):
    import fcaf3d_amd as fa
    return fa.build_loss(dict(type='GIoU3DLoss' if kind == 'giou' else 'DIoU3DLoss', **kw))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@pytest.mark.parametrize('kind', KINDS)
def test_values_and_gradients_meet_the_float64_fixture(kind):
    """per group: loss and iou within 1e-5 of the reference's float64 run, d(sum w loss)/d pred within 1e-4 of the group's gradient scale,
    rows without weight exactly zero; the iou output equals rotated_iou_3d / axis_aligned_iou_3d on the same rows within 1e-6"""
    from fcaf3d_amd.losses import axis_aligned_iou_3d, rotated_iou_3d
    d = fixture()
    for g in GROUPS:
        pred = _t(d[f'{g}_pred']).requires_grad_(True)
        tgt, w = _t(d[f'{g}_target']), _t(d[f'{g}_w'])
        loss, iou = _fn(kind)(pred, tgt, w, return_iou=True)
        assert not iou.requires_grad
        (loss * w).sum().backward()
        check_against_fixture(d, g, kind, loss.detach().cpu().numpy(), iou.cpu().numpy(), pred.grad.cpu().numpy(), 'gpu')
        with torch.no_grad():
            other = axis_aligned_iou_3d(pred, tgt) if g == 'al' else rotated_iou_3d(pred, tgt, w)
        act = w > 0
        diff = float((iou[act] - other[act]).abs().max())
        print(f'gpu {g:8s} {kind}: iou output against the IoU kernel, max difference {diff:.2e}')
        assert diff <= 1e-6, (g, kind, diff)


@functools.lru_cache(maxsize=None)
def _dense(kind, g):
    """max(SIZES) rows of a group without weights: (pred, target, loss, iou, d loss/d pred) on the device, computed once"""
    d = fixture()
    n = max(SIZES)
    reps = -(-n // len(d[f'{g}_pred']))
    pred = _t(np.tile(d[f'{g}_pred'], (reps, 1))[:n]).requires_grad_(True)
    tgt = _t(np.tile(d[f'{g}_target'], (reps, 1))[:n])
    loss, iou = _fn(kind)(pred, tgt, None, return_iou=True)
    loss.sum().backward()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(pred.grad).all())
    return pred.detach(), tgt, loss.detach(), iou, pred.grad.clone()


@pytest.mark.parametrize('g', ('ro', 'al'))
@pytest.mark.parametrize('kind', KINDS)
def test_sizes_and_weight_patterns_with_poisoned_inactive_rows(kind, g):
    """n around the wave and past the workgroup's 1 024 rows, three weight patterns; the rows without weight hold NaN / inf boxes: value and
    every gradient there are exactly zero and finite, the active rows equal the dense call's rows bit for bit"""
    pred0, tgt0, loss0, iou0, grad0 = _dense(kind, g)
    for n in SIZES:
        for pattern in PATTERNS:
            w = _t(pattern_weight(pattern, n))
            off, on = w == 0, w > 0
            pred, tgt = pred0[:n].clone(), tgt0[:n].clone()
            pred[off] = float('nan')
            tgt[off] = float('inf')
            pred.requires_grad_(True)
            loss, iou = _fn(kind)(pred, tgt, w, return_iou=True)
            (loss * w).sum().backward()
            for got in (loss, iou, pred.grad):
                assert bool(torch.isfinite(got).all()) and bool((got[off] == 0).all()), (g, n, pattern)
            assert torch.equal(loss[on], loss0[:n][on]) and torch.equal(iou[on], iou0[:n][on]), (g, n, pattern)
            assert torch.equal(pred.grad[on], w[on, None] * grad0[:n][on]), (g, n, pattern)


def test_no_rows():
    import fcaf3d_amd as fa
    dev = _dev()
    for kind in KINDS:
        for bd in (6, 7):
            pred = torch.zeros((0, bd), device=dev, requires_grad=True)
            loss, iou = _fn(kind)(pred, torch.zeros((0, 7), device=dev), None, return_iou=True)
            assert loss.shape == iou.shape == (0,)
            out = _module(kind, with_yaw=bd == 7)(pred, torch.zeros((0, 7), device=dev), weight=torch.zeros(0, device=dev), avg_factor=1.0)
            out.backward()
            assert float(out.detach()) == 0.0 and pred.grad.shape == (0, bd)
    assert fa.GIoU3DLoss is type(_module('giou'))


@pytest.mark.parametrize('g', ('ro', 'al'))
@pytest.mark.parametrize('kind', KINDS)
def test_module_semantics_against_numpy(kind, g):
    """the three reductions, avg_factor, loss_weight, 2-D weights and the all-zero weight against numpy on the fixture's float64 rows.
    Bound: every row is within 1e-5 of its float64 value (the test above), so a weighted sum is within 1e-5 * sum(w), plus the float32
    summation of n = 256 terms (n * 2^-24 relative, taken as 2e-5 of the result)."""
    d = fixture()
    w64 = d[f'{g}_w'].astype(np.float64)
    rows = d[f'{g}_{kind}_loss64'] * w64
    tol = lambda want, scale=1.0: scale * 1e-5 * w64.sum() + 2e-5 * abs(want)
    tgt, w = _t(d[f'{g}_target']), _t(d[f'{g}_w'])
    lw = 1.7
    mod = _module(kind, with_yaw=g != 'al', loss_weight=lw)
    assert mod.reduction == 'mean'

    def run(**kw):
        pred = _t(d[f'{g}_pred']).requires_grad_(True)
        return pred, mod(pred, tgt, **kw)
    _, out = run(weight=w)
    assert abs(float(out) - lw * rows.mean()) <= tol(lw * rows.mean(), lw / len(rows))
    _, out = run(weight=w, reduction_override='sum')
    assert abs(float(out) - lw * rows.sum()) <= tol(lw * rows.sum(), lw)
    _, out = run(weight=w, reduction_override='none')
    assert out.shape == (len(rows),) and np.abs(out.detach().cpu().numpy() - lw * rows).max() <= lw * 1e-5 * w64.max() + 2e-5 * lw * rows.max()
    pred, out = run(weight=w, avg_factor=3.5)
    assert abs(float(out) - lw * rows.sum() / 3.5) <= tol(lw * rows.sum() / 3.5, lw / 3.5)
    out.backward()
    g64 = lw * d[f'{g}_{kind}_grad64'] / 3.5
    assert np.abs(pred.grad.cpu().numpy() - g64).max() <= 1e-4 * np.abs(g64).max()
    _, out = run(weight=w, avg_factor=3.5, reduction_override='none')
    assert out.shape == (len(rows),)
    with pytest.raises(ValueError):
        run(weight=w, avg_factor=3.5, reduction_override='sum')
    # 2-D weights are averaged over their last axis: columns w/2, w, 3w/2
    w2 = torch.stack((w * 0.5, w, w * 1.5), 1)
    _, out = run(weight=w2, reduction_override='sum')
    assert abs(float(out) - lw * rows.sum()) <= tol(lw * rows.sum(), lw) + 1e-6 * lw * rows.sum()
    _, out = run(reduction_override='sum')                               # no weights at all
    want = lw * d[f'{g}_{kind}_loss64'].sum()
    assert abs(float(out) - want) <= lw * 1e-5 * len(rows) + 2e-5 * want
    pred, out = run(weight=torch.zeros_like(w), avg_factor=3.0)          # iou3d_loss.py:53-54, the zero-weight early-out
    out.backward()
    assert float(out) == 0.0 and float(pred.grad.abs().sum()) == 0.0
    with pytest.raises(AssertionError, match='with_yaw'):
        _module(kind, with_yaw=g == 'al')(pred, tgt)


# ---- in the head -------------------------------------------------------------------------------------------------------------------

HEAD_CASES = [
    ('fcaf3d_sunrgbd-3d-10class', dict(rotated=True, n_boxes=6, n_classes=10), dict(type='GIoU3DLoss')),
    ('fcaf3d_sunrgbd-3d-10class', dict(rotated=True, n_boxes=6, n_classes=10), dict(type='DIoU3DLoss')),
    ('fcaf3d_scannet-3d-18class', {}, dict(type='DIoU3DLoss', with_yaw=False)),
    ('fcaf3d_scannet-3d-18class', {}, dict(type='GIoU3DLoss', with_yaw=False)),
]


def _forward_train(name, kw, loss_bbox, backward):
    """forward_train (extract_feat with the ground truth, then the head's loss: SingleStageSparse3DDetector.forward_train) of 2 scenes
    of 20 000 points on a 1-level model -> the losses, the parameter gradients, and loss_bbox once more from the module applied to
    `_bbox_pred_to_bbox` of the head's own outputs with the head's weights"""
    from tests.test_gpu_model import _build, _scenes, _to_gpu_batch
    dev = _dev()
    model, m = _build(name, 0.02, 1, seed=8, loss_bbox=loss_bbox)
    model = model.to(dev).train()
    head = model.neck_with_head
    head.fused_loss = False                  # the three loss modules for every loss type, so that loss_cls / loss_centerness are comparable bit for bit
    pts, gts, labs = _scenes([71, 72], n_points=20000, **kw)
    b = _to_gpu_batch(pts, gts, labs, dev)
    x = model.extract_feat(b['points'], b['img_metas'], (b['gt_bboxes_3d'], b['gt_labels_3d']))
    losses = head.loss(*x, b['gt_bboxes_3d'], b['gt_labels_3d'], b['img_metas'])
    grads = None
    with torch.no_grad():
        tg = head._targets([p.cmap for p in x[3]], b['gt_bboxes_3d'], b['gt_labels_3d'])
        boxes = head._bbox_pred_to_bbox(tg['pts'], torch.cat([v.full for v in x[1]]))
        weight = tg['ct'] * tg['inv_den'][tg['scene'].long()]
        again = head.loss_bbox(boxes, tg['bt'], weight=weight, avg_factor=1.0)
        active = int((weight > 0).sum())
    if backward:
        sum(losses.values()).backward()
        grads = [p.grad for p in model.parameters() if p.requires_grad]
    return {k: v.detach() for k, v in losses.items()}, grads, again, active, boxes.shape


@functools.lru_cache(maxsize=None)
def _iou_baseline(name):
    kw = dict(HEAD_CASES[0][1]) if 'sunrgbd' in name else {}
    return _forward_train(name, kw, dict(type='IoU3DLoss', with_yaw='sunrgbd' in name), False)[0]


@pytest.mark.parametrize('name,kw,loss_bbox', HEAD_CASES)
def test_head_with_an_enclosing_box_loss(name, kw, loss_bbox):
    """against the same model (same seed) with IoU3DLoss, all on the three-module path: loss_cls and loss_centerness bit-equal,
    loss_bbox not smaller (both penalties are non-negative; 1e-6 relative for the float32 sums), everything finite, and loss_bbox equal
    to the module applied to the decoded boxes of the head's own outputs (the same kernel on the same rows: 1e-6 relative for the order
    of the reductions)"""
    base = _iou_baseline(name)
    losses, grads, again, active, shape = _forward_train(name, kw, loss_bbox, True)
    print(f'{name} {loss_bbox}: {shape[0]} locations x {shape[1]}, {active} with weight; losses',
          {k: float(v) for k, v in losses.items()}, 'IoU3DLoss loss_bbox', float(base['loss_bbox']))
    assert active > 0 and shape[1] == (7 if loss_bbox.get('with_yaw', True) else 6)
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert torch.equal(losses['loss_cls'], base['loss_cls']) and torch.equal(losses['loss_centerness'], base['loss_centerness'])
    assert float(losses['loss_bbox']) >= float(base['loss_bbox']) * (1 - 1e-6)
    assert abs(float(again) - float(losses['loss_bbox'])) <= 1e-6 * abs(float(again))


@pytest.mark.parametrize('loss_bbox', [dict(type='GIoU3DLoss'), dict(type='DIoU3DLoss')])
def test_three_training_steps_stay_finite(loss_bbox):
    import fcaf3d_amd as fa
    from fcaf3d_amd.runner import TrainStep
    from tests.test_gpu_model import _build, _scenes, _to_gpu_batch
    dev = _dev()
    name = 'fcaf3d_sunrgbd-3d-10class'
    model, m = _build(name, 0.02, 1, seed=9, loss_bbox=loss_bbox)
    model = model.to(dev).train()
    tr = TrainStep.from_config(model, fa.get_config(name, voxel_size=0.02))
    traj = []
    for step in range(3):
        pts, gts, labs = _scenes([80 + step], n_points=12000, **HEAD_CASES[0][1])
        loss, _ = tr(_to_gpu_batch(pts, gts, labs, dev))
        traj.append(float(loss))
    print(loss_bbox['type'], 'loss trajectory', traj)
    assert all(np.isfinite(traj))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
