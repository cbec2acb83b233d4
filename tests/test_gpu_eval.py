"""GPU: the evaluation matching kernel (csrc_post/eval.hip, fc_eval_match) against the host producer and against indoor_eval;
indoor_eval_device on the goldens; runner.evaluate against simple_test + indoor_eval_device, in one process and in two ranks
sharing the GPU."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

METRIC = (0.25, 0.5)
# per-scene sizes around the kernel's tiles: 256 detections per workgroup, 64 ground-truth boxes per LDS chunk
DET_COUNTS = (0, 1, 63, 64, 65, 256, 257, 700, 300, 294, 0)
GT_COUNTS = (5, 0, 1, 64, 65, 130, 63, 129, 128, 20, 0)
L2C = {i: f'cat{i}' for i in range(5)}


def _dev():
    return torch.device('cuda', torch.cuda.current_device())


def _iou(a, b):
    from fcaf3d_amd.nms import boxes_iou3d_gpu
    return boxes_iou3d_gpu(torch.from_numpy(a).to(_dev()), torch.from_numpy(b).to(_dev())).cpu().numpy()


def _class_best(iou, dl, gl):
    """per detection: best IoU over the boxes of its class (first maximum), its index, the runner-up (-inf where there is none)"""
    n = len(dl)
    best, arg, second = np.full(n, -np.inf), np.full(n, -1, np.int64), np.full(n, -np.inf)
    if iou.shape[1] == 0:
        return best, arg, second
    m = np.where(dl[:, None] == gl[None, :], iou.astype(np.float64), -np.inf)
    arg = m.argmax(1)
    best = m[np.arange(n), arg]
    m2 = m.copy()
    m2[np.arange(n), arg] = -np.inf
    second = np.where(np.isfinite(best), m2.max(1), -1.0)            # (no box of the class: no runner-up to be near to)
    arg = np.where(np.isfinite(best), arg, -1)
    return best, arg, second


def _scene(rng, n_det, n_gt, yaw):
    """ground truth on a 12 x 12 grid of 2 m cells (no two boxes touch), classes 0-3; detections: copies of boxes of classes 0-2
    under the box's class, copies under ANOTHER class (the class filter), clutter far above the room under classes 0, 1, 2, 4.
    Class 3 exists in the ground truth only, class 4 among the detections only.  A copy's IoU with its box falls in one of
    three bands that keep clear of the thresholds by construction: 'tight' (shift <= 1 cm, sizes x [.97, 1.03], yaw +- .02:
    above .6), 'loose' (the box shrunk by s in [.70, .75] and moved inside its original, same yaw: s^3 in [.34, .42]) and
    'low' (s in [.50, .58]: [.12, .20]).  Nothing is filtered: the test asserts the margins on what is drawn."""
    cells = rng.permutation(144)[:n_gt]
    gb = np.zeros((n_gt, 7), np.float32)
    gb[:, 0] = (cells % 12) * 2.0 + rng.uniform(-.1, .1, n_gt)
    gb[:, 1] = (cells // 12) * 2.0 + rng.uniform(-.1, .1, n_gt)
    gb[:, 2] = rng.uniform(.5, 1.5, n_gt)
    gb[:, 3:6] = rng.uniform(.4, 1.0, (n_gt, 3))
    if yaw:
        gb[:, 6] = rng.uniform(-np.pi, np.pi, n_gt)
    gl = rng.integers(0, 4, n_gt)
    src = np.flatnonzero(gl < 3)
    kind = rng.choice(3, n_det, p=(.6, .1, .3)) if len(src) else np.full(n_det, 2)
    db = np.zeros((n_det, 7), np.float32)
    dl = np.zeros(n_det, np.int64)
    for i in range(n_det):
        if kind[i] == 2:
            db[i, :2] = rng.uniform(0, 24, 2)
            db[i, 2] = 50 + rng.uniform(0, 1)
            db[i, 3:6] = rng.uniform(.4, 1.0, 3)
            dl[i] = rng.choice((0, 1, 2, 4))
            continue
        j = src[rng.integers(len(src))]
        g = gb[j].astype(np.float64)
        band = rng.choice(3, p=(.6, .25, .15)) if kind[i] == 0 else 0
        if band == 0:
            shift, size = rng.uniform(-.01, .01, 3), g[3:6] * rng.uniform(.97, 1.03, 3)
            turn = rng.uniform(-.02, .02) if yaw else 0.0
        else:
            sc = rng.uniform(.70, .75) if band == 1 else rng.uniform(.50, .58)
            size, turn = g[3:6] * sc, 0.0
            shift = rng.uniform(-.8, .8, 3) * (1 - sc) / 2 * g[3:6]              # in the box's own axes: stays inside
        c, sn = np.cos(g[6]), np.sin(g[6])
        db[i, 0] = g[0] + c * shift[0] - sn * shift[1]
        db[i, 1] = g[1] + sn * shift[0] + c * shift[1]
        db[i, 2] = g[2] + shift[2]
        db[i, 3:6] = size
        db[i, 6] = g[6] + turn
        dl[i] = gl[j] if kind[i] == 0 else (gl[j] + 1) % 3
    return gb, gl, db, dl


@functools.lru_cache(maxsize=None)
def _crafted(yaw):
    """-> gt_annos, dt_annos (device tensors; 7 columns with yaw, or 6 columns), per-scene numpy (gb, gl, db7, dl)"""
    rng = np.random.default_rng(7 if yaw else 8)
    scenes = [_scene(rng, nd, ng, yaw) for nd, ng in zip(DET_COUNTS, GT_COUNTS)]
    n = sum(DET_COUNTS)
    scores = (rng.permutation(n) + 1).astype(np.float32) / np.float32(n)
    gt_annos, dt_annos, o = [], [], 0
    for gb, gl, db, dl in scenes:
        gt_annos.append({'gt_num': len(gb), 'gt_boxes_upright_depth': gb, 'class': gl})
        b = db if yaw else db[:, :6]
        dt_annos.append(dict(boxes_3d=torch.from_numpy(np.ascontiguousarray(b)).to(_dev()),
                             scores_3d=torch.from_numpy(scores[o:o + len(dl)]).to(_dev()), labels_3d=torch.from_numpy(dl).to(_dev())))
        o += len(dl)
    return gt_annos, dt_annos, scenes


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() or (np.isnan(a[k]) and np.isnan(b[k])), (k, a[k], b[k])


@pytest.mark.parametrize('yaw', [True, False])
def test_kernel_equals_the_host_producer_and_indoor_eval(yaw):
    from fcaf3d_amd.evaluation import finish_table, indoor_eval, match_table_device, match_table_host
    gt_annos, dt_annos, scenes = _crafted(yaw)
    assert sum(DET_COUNTS) == 2000 and len(scenes) == 11
    # the margins that make an exact comparison meaningful, on the host IoUs: 1e-3 = 20 x the 5e-5 this IoU is held to
    want_iou, want_gt = [], []
    for gb, gl, db, dl in scenes:
        best, arg, second = _class_best(_iou(db, gb) if len(gb) and len(db) else np.zeros((len(db), len(gb)), np.float32), dl, gl)
        for t in METRIC:
            assert (np.abs(best - t) > 1e-3).all()
        assert not ((best > 0) & (best - second < 1e-3)).any()
        want_iou.append(best); want_gt.append(arg)
    want_iou, want_gt = np.concatenate(want_iou), np.concatenate(want_gt)
    labels = np.concatenate([s[3] for s in scenes])
    assert (want_iou > 0.5).sum() > 300 and ((want_iou > 0.25) & (want_iou < 0.5)).sum() > 20 and (want_iou == 0).sum() > 50
    assert np.isinf(want_iou).sum() > 100 and set(labels) == {0, 1, 2, 4}

    host, h_iou, h_gt = match_table_host(gt_annos, dt_annos, METRIC, return_match=True)
    devt, d_iou, d_gt = match_table_device(gt_annos, dt_annos, METRIC, return_match=True)
    assert np.array_equal(h_gt, want_gt) and np.array_equal(d_gt, want_gt)
    fin = np.isfinite(want_iou)
    assert np.array_equal(np.isfinite(d_iou), fin) and (d_iou[~fin] == -np.inf).all()
    err = np.abs(d_iou[fin].astype(np.float64) - want_iou[fin]).max()
    print(f'yaw={yaw}: best_iou max |kernel - boxes_iou3d_gpu| = {err:.3e}, bit-equal: {np.array_equal(d_iou[fin], want_iou[fin].astype(np.float32))}')
    assert err <= 5e-5
    assert np.array_equal(devt.tp_bits, host.tp_bits) and devt.tp_bits.any()
    for name in ('scene', 'pos', 'label', 'score'):
        assert np.array_equal(getattr(devt, name), getattr(host, name)), name
    assert devt.npos == host.npos and devt.first_seen == host.first_seen
    ref = indoor_eval(gt_annos, dt_annos, METRIC, L2C)
    _same(finish_table(devt, METRIC, L2C), ref)
    assert 0 < ref['mAP_0.50'] < ref['mAP_0.25'] < 1 and 'cat3_AP_0.25' in ref and 'cat4_AP_0.25' in ref


def test_goldens_on_the_device_with_bottom_centre_boxes():
    """both cases of tests/golden/indoor_eval.npz and both vectors of the reference's own test: DepthInstance3DBoxes objects
    (bottom-centre tensor, FC_EVAL_DET_BOTTOM), on the CPU and moved to the device"""
    from fcaf3d_amd.evaluation import indoor_eval, indoor_eval_device
    from tests.test_oracle_golden import _indoor_eval_case, _ref_indoor_eval_vectors
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'indoor_eval.npz'))
    cases = [_indoor_eval_case(d, c) for c in (0, 1)] + [v + (None,) for v in _ref_indoor_eval_vectors()]
    for gt, dt, l2c, want in cases:
        ref = indoor_eval(gt, dt, METRIC, l2c)
        got = indoor_eval_device(gt, dt, METRIC, l2c)
        _same(got, ref)
        on_dev = [dict(boxes_3d=x['boxes_3d'].to(_dev()), scores_3d=x['scores_3d'].to(_dev()), labels_3d=x['labels_3d'].to(_dev())) for x in dt]
        _same(indoor_eval_device(gt, on_dev, METRIC, l2c), ref)
        triples = [(x['boxes_3d'], x['scores_3d'], x['labels_3d']) for x in on_dev]
        _same(indoor_eval_device(gt, triples, METRIC, l2c), ref)
        if want is not None:
            assert sorted(got) == sorted(want)
            for k in want:
                assert abs(got[k] - want[k]) < 1e-4, (k, got[k], want[k])
    r = indoor_eval_device(*cases[2][:2], METRIC, cases[2][2])
    assert np.isclose(r['cabinet_AP_0.25'], 0.666667) and np.isclose(r['mAP_0.25'], 0.708333) and np.isclose(r['mAR_0.25'], 0.833333)


def test_many_claimants_one_true_positive_and_no_second_choice():
    """five detections on box A (IoU .43 .82 .74 .67 .90 by position) and X, whose best box is A (.48) and whose second-best, B
    (.29), nobody claims: one true positive per (box, threshold) — at 0.25 the best-scored claimant, at 0.5 the best-scored
    among those above 0.5 — and X never falls back to B.  With equal scores the lowest position wins."""
    from fcaf3d_amd.evaluation import finish_table, indoor_eval, match_table_device
    A, B = [0, 0, 0, 1, 1, 1, 0], [.9, 0, 0, 1, 1, 1, 0]
    gt = [{'gt_num': 2, 'gt_boxes_upright_depth': np.array([A, B], np.float32), 'class': np.array([0, 0])}]
    shifts = (-.4, -.1, -.15, -.2, -.05)
    boxes = np.array([[s, 0, 0, 1, 1, 1, 0] for s in shifts] + [[.35, 0, 0, 1, 1, 1, 0]], np.float32)
    iou = _iou(boxes, np.array([A, B], np.float32))
    assert (iou.argmax(1) == 0).all() and .25 < iou[0, 0] < .5 and (iou[1:5, 0] > .5).all() and .25 < iou[5, 1] < iou[5, 0] < .5
    for scores, distinct in (([.9, .8, .7, .6, .5, .4], True), ([.5] * 6, False)):
        dt = [dict(boxes_3d=torch.from_numpy(boxes).to(_dev()), scores_3d=torch.tensor(scores, device=_dev()),
                   labels_3d=torch.zeros(6, dtype=torch.long, device=_dev()))]
        table, b_iou, b_gt = match_table_device(gt, dt, METRIC, return_match=True)
        assert b_gt.tolist() == [0] * 6
        assert table.tp_bits.tolist() == [1, 2, 0, 0, 0, 0]
        if distinct:
            l2c = {0: 'thing'}
            got = finish_table(table, METRIC, l2c)
            _same(got, indoor_eval(gt, dt, METRIC, l2c))
            assert got['thing_rec_0.25'] == 0.5                       # B stays unmatched


def _random_set(n_scenes, seed):
    rng = np.random.default_rng(seed)
    gt, dt = [], []
    for _ in range(n_scenes):
        gb = np.concatenate([rng.uniform(0, 5, (6, 3)), rng.uniform(.5, 1.5, (6, 3)), rng.uniform(-3, 3, (6, 1))], 1).astype(np.float32)
        gt.append({'gt_num': 6, 'gt_boxes_upright_depth': gb, 'class': rng.integers(0, 3, 6)})
        db = np.concatenate([rng.uniform(0, 5, (40, 3)), rng.uniform(.5, 1.5, (40, 3)), rng.uniform(-3, 3, (40, 1))], 1).astype(np.float32)
        dt.append(dict(boxes_3d=torch.from_numpy(db).to(_dev()), scores_3d=torch.from_numpy(rng.random(40).astype(np.float32)).to(_dev()),
                       labels_3d=torch.from_numpy(rng.integers(0, 3, 40)).to(_dev())))
    return gt, dt


def test_native_calls_do_not_grow_with_the_set(monkeypatch):
    from fcaf3d_amd import _lib as L
    from fcaf3d_amd.evaluation import indoor_eval_device
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    counts = []
    for n in (4, 32):
        gt, dt = _random_set(n, n)
        del calls[:]
        r = indoor_eval_device(gt, dt, METRIC, {0: 'a', 1: 'b', 2: 'c'})
        assert np.isfinite(r['mAP_0.25'])
        counts.append(list(calls))
    assert counts[0] == counts[1] == ['fc_eval_match']


# ---- the loop ---------------------------------------------------------------------------------------------------------------------
LOOP_SEEDS = (61, 62, 63, 64)
LOOP_IDS = (0, 2, 1, 3)          # batch 0 holds scenes 0 and 2, batch 1 scenes 1 and 3: the batches two round-robin ranks see
LOOP_L2C = {i: f'c{i}' for i in range(18)}


def _loop_inputs(dev, ids):
    """the scenes with global ids `ids`, two per batch -> batches [(points, img_metas)], gt_annos"""
    import fcaf3d_amd as fa
    from fcaf3d_amd.synthetic import make_scene
    sc = [make_scene(LOOP_SEEDS[i], n_points=20000) for i in ids]
    pts = [torch.from_numpy(s[0]).to(dev) for s in sc]
    metas = [dict(box_type_3d=fa.DepthInstance3DBoxes) for _ in sc]
    batches = [(pts[i:i + 2], metas[i:i + 2]) for i in range(0, len(sc), 2)]
    gt_annos = [{'gt_num': len(s[1]), 'gt_boxes_upright_depth': s[1], 'class': s[2]} for s in sc]
    return batches, gt_annos


def _loop_model(dev):
    from tests.test_gpu_tta import _build
    return _build('fcaf3d_scannet-3d-18class')[0].to(dev)


@functools.lru_cache(maxsize=None)
def _loop_reference():
    """indoor_eval_device over the simple_test results of the two batches (one process)"""
    from fcaf3d_amd.evaluation import indoor_eval_device
    dev = _dev()
    model = _loop_model(dev).eval()
    batches, gt_annos = _loop_inputs(dev, LOOP_IDS)
    with torch.no_grad():
        res = [r for points, metas in batches for r in model.simple_test(points, metas)]
    assert all(len(r['scores_3d']) > 10 for r in res)
    return indoor_eval_device(gt_annos, res, METRIC, LOOP_L2C, scene_ids=LOOP_IDS, group=False)


def test_evaluate_equals_simple_test_plus_indoor_eval_device():
    from fcaf3d_amd.runner import evaluate
    dev = _dev()
    ref = _loop_reference()
    assert len(ref) > 4
    model = _loop_model(dev).train()
    model.backbone.eval()                                    # a frozen part: its flags must come back as they were, too
    before = [m.training for m in model.modules()]
    assert any(before) and not all(before)
    batches, gt_annos = _loop_inputs(dev, LOOP_IDS)
    got2 = evaluate(model, batches, gt_annos, METRIC, LOOP_L2C, in_flight=2, scene_ids=LOOP_IDS)
    assert model.training and [m.training for m in model.modules()] == before
    _same(got2, ref)
    model.eval()
    got1 = evaluate(model, iter(batches), gt_annos, METRIC, LOOP_L2C, in_flight=1, scene_ids=LOOP_IDS)
    assert not model.training
    _same(got1, ref)


def _rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      FC_DIST_BACKEND='gloo')
    from fcaf3d_amd import dist as D
    from fcaf3d_amd.runner import evaluate
    D.init_dist(backend='gloo')
    dev = torch.device('cuda:0')
    model = _loop_model(dev).eval()
    batches, gt_annos = _loop_inputs(dev, [rank, rank + world])            # default scene ids: rank + world * i
    got = evaluate(model, batches, gt_annos, METRIC, LOOP_L2C)
    q.put((rank, got))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_on_one_gpu_return_the_single_process_result():
    import torch.multiprocessing as mp
    from tests.test_gpu_dist import _collect, _free_port
    ref = _loop_reference()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = _collect(q, procs, 2, 240)                # kills both ranks when one dies or the limit passes
    for p in procs:
        p.join(60)
        if p.is_alive():
            p.kill()
        assert p.exitcode == 0
    for rank, got in res:
        _same(got, ref)
