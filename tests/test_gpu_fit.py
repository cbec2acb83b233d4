"""GPU: runner.fit on the two-level model of tests/test_gpu_dist.py over 7 synthetic scenes written to disk (six of 6 000 points,
one of 3 000, one without boxes): num_points 4 000, 2 scenes per step, 2 epochs of 3 steps."""
import json
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.test_fit_cpu import make_cfg
from tests.test_gpu_dist import _collect, _free_port, _model

pytestmark = pytest.mark.gpu
SEED = 7


def _fresh(dev):
    import fcaf3d_amd as fa
    model, _ = _model(fa)
    return model.to(dev).train()


def _params(model):
    return [p.detach().clone() for p in model.parameters()] + [b.detach().clone() for b in model.buffers()]


@pytest.fixture(scope='module')
def straight(tmp_path_factory):
    """the straight two-epoch run with evaluation after every epoch; every step logged (interval 1), both checkpoints kept"""
    from fcaf3d_amd import fit
    root = tmp_path_factory.mktemp('fit')
    dev = torch.device('cuda:0')
    cfg = make_cfg(root / 'data', val=True, log_config=dict(interval=1), checkpoint_config=dict(interval=1, max_keep_ckpts=2))
    model = _fresh(dev)
    metas = []
    rec = fit(model, cfg, str(root / 'work'), seed=SEED, on_batch=lambda e, it, b: metas.append((e, it, b['img_metas'])))
    torch.cuda.synchronize()
    return dict(root=root, cfg=cfg, rec=rec, params=_params(model), metas=metas, dev=dev)


def test_fit_equals_a_hand_written_loop_of_train_steps(straight):
    """(a) losses of every step and the final parameters, bitwise"""
    from fcaf3d_amd import data as DT
    from fcaf3d_amd.runner import TrainStep
    cfg, dev = straight['cfg'], straight['dev']
    model = _fresh(dev)
    ds = DT.build_dataset(cfg.data.train)
    ld = DT.DeviceLoader(DT.ResidentScenes(ds, dev), ds.pipeline, 2, seed=SEED)
    tr = TrainStep.from_config(model, cfg)
    losses = []
    for epoch in range(2):
        tr.lr.set_epoch(epoch)
        bs = ld.batches(epoch)
        for k, b in enumerate(bs):
            loss, _ = tr(b, bs[k + 1] if k + 1 < len(bs) else None)
            losses.append(loss.detach())
        tr.epoch_end()
    losses = [float(l) for l in losses]
    train = [r for r in straight['rec'] if r['mode'] == 'train']
    assert len(train) == len(losses) == 6 and all(np.isfinite(losses))
    assert [r['loss'] for r in train] == losses
    assert [(r['epoch'], r['iter']) for r in train] == [(e, i) for e in (1, 2) for i in (1, 2, 3)]
    assert [r['lr'] for r in train] == [0.001] * 3 + [0.0001] * 3 and all(r['grad_norm'] > 0 for r in train)
    assert all(torch.equal(a, b) for a, b in zip(_params(model), straight['params']))


def test_resume_continues_the_straight_run_and_checkpoints_rotate(straight, tmp_path):
    """(b) one epoch, then a fresh model resumed from latest.pth for one more = the straight two epochs: parameters bitwise, the
    iteration count equal; (c) max_keep_ckpts=1 leaves the last epoch's file and latest.pth, which load_checkpoint reads"""
    from fcaf3d_amd import fit, load_checkpoint
    dev = straight['dev']
    cfg = make_cfg(straight['root'] / 'data', max_epochs=1, log_config=dict(interval=1))
    work = tmp_path / 'work'
    fit(_fresh(dev), cfg, str(work), seed=SEED)
    assert sorted(f for f in os.listdir(work) if f.endswith('.pth')) == ['epoch_1.pth', 'latest.pth']
    model = _fresh(dev)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.5)                                               # whatever the fresh model holds is replaced
    cfg.runner['max_epochs'] = 2
    rec = fit(model, cfg, str(work), seed=SEED, resume_from=str(work / 'latest.pth'))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(_params(model), straight['params']))
    train = [r for r in straight['rec'] if r['mode'] == 'train']
    assert [(r['epoch'], r['iter'], r['loss']) for r in rec] == [(r['epoch'], r['iter'], r['loss']) for r in train[3:]]
    assert sorted(f for f in os.listdir(work) if f.endswith('.pth')) == ['epoch_2.pth', 'latest.pth']
    ck = load_checkpoint(_fresh(dev), str(work / 'latest.pth'), map_location='cpu', strict=True)
    assert ck['meta']['epoch'] == 2 and ck['meta']['iter'] == 6 and ck['meta']['seed'] == SEED
    ck2 = torch.load(straight['root'] / 'work' / 'latest.pth', map_location='cpu', weights_only=False)
    assert ck2['meta']['iter'] == 6 and all(torch.equal(v, ck2['state_dict'][k]) for k, v in ck['state_dict'].items())


def test_evaluation_records_equal_evaluate_on_the_saved_weights(straight):
    """(d) one 'val' record per epoch with indoor_eval's keys, equal to runner.evaluate called by hand on that epoch's checkpoint"""
    from fcaf3d_amd import data as DT
    from fcaf3d_amd import load_checkpoint
    from fcaf3d_amd.runner import validate
    cfg, dev = straight['cfg'], straight['dev']
    val = [r for r in straight['rec'] if r['mode'] == 'val']
    assert [r['epoch'] for r in val] == [1, 2]
    vs = DT.build_dataset(cfg.data.val)
    assert len(vs) == 7                                               # the validation set keeps the scene without boxes
    ld = DT.DeviceLoader(DT.ResidentScenes(vs, dev), vs.pipeline, 2, seed=SEED)
    from fcaf3d_amd.runner import evaluate
    import pickle
    infos = pickle.load(open(cfg.data.val['ann_file'], 'rb'))             # ground truth and scene ids built here, from the info file
    annos = [i['annos'] for i in infos]
    assert len(annos) == 7 and annos[2]['gt_num'] == 0
    for r in val:
        model = _fresh(dev)
        load_checkpoint(model, str(straight['root'] / 'work' / f'epoch_{r["epoch"]}.pth'), map_location=dev, strict=True)
        batches = ld.batches(0)
        assert [m['sample_idx'] for b in batches for m in b['img_metas']] == [i['point_cloud']['lidar_idx'] for i in infos]
        res = evaluate(model, ((b['points'], b['img_metas']) for b in batches), annos, metric=(0.25, 0.5), scene_ids=list(range(7)))
        assert {'mAP_0.25', 'mAR_0.25', 'mAP_0.50', 'mAR_0.50'} <= set(res)
        got = {k: v for k, v in r.items() if k not in ('mode', 'epoch', 'iter', 'lr')}
        assert set(got) == set(res)
        np.testing.assert_equal(got, {k: float(v) for k, v in res.items()})
        np.testing.assert_equal(validate(model, ld), res)
    logs = [f for f in os.listdir(straight['root'] / 'work') if f.endswith('.log.json')]
    assert len(logs) == 1
    lines = [json.loads(l) for l in open(straight['root'] / 'work' / logs[0])]
    assert [l['mode'] for l in lines] == ['train'] * 3 + ['val'] + ['train'] * 3 + ['val']


def test_the_scene_without_boxes_is_never_trained_on(straight):
    """(e) filter_empty_gt"""
    from fcaf3d_amd import data as DT
    seen = [m['sample_idx'] for _, _, metas in straight['metas'] for m in metas]
    assert len(seen) == 12 and 'scene0002' not in seen and set(seen) == {f'scene{k:04d}' for k in (0, 1, 3, 4, 5, 6)}
    for e in (0, 1):
        order = DT.epoch_order(6, SEED, e, 2, 1)
        assert [m['dataset_index'] for ep, _, metas in straight['metas'] if ep == e for m in metas] == list(order)


def _worker(rank, world, port, q, root):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      FC_DIST_BACKEND='gloo')
    from fcaf3d_amd import dist as D
    from fcaf3d_amd import fit
    D.init_dist(backend='gloo')
    dev = torch.device('cuda:0')
    cfg = make_cfg(os.path.join(root, 'data'), max_epochs=1)
    model = _fresh(dev)
    if rank:
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.01)                                           # fit starts every rank from rank 0's weights
    seen = []
    rec = fit(model, cfg, os.path.join(root, 'work'), seed=SEED, on_batch=lambda e, it, b: seen.extend(m['dataset_index'] for m in b['img_metas']))
    torch.cuda.synchronize()
    import hashlib
    digest = hashlib.sha256(b''.join(t.detach().cpu().contiguous().numpy().tobytes() for t in model.parameters())).hexdigest()      # parameters; BatchNorm's running buffers follow each rank's own scenes
    q.put((rank, seen, digest, len(rec)))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_shard_the_epoch_and_keep_identical_parameters(tmp_path):
    """(f) two gloo ranks on one GPU: identical parameters after one epoch; the indices they saw are the padded permutation,
    rank r its [r::2]; rank 0 alone wrote files"""
    from fcaf3d_amd import data as DT
    make_cfg(tmp_path / 'data')                                        # the scenes are written once, here
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = _collect(q, procs, 2, 300)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, s0, d0, n0), (_, s1, d1, n1) = res
    assert d0 == d1, 'parameters diverged between the ranks'
    order = DT.epoch_order(6, SEED, 0, 2, 2)
    assert len(order) == 8 and s0 == list(order[0::2]) and s1 == list(order[1::2])
    assert sorted(s0 + s1) == sorted(order) and n0 == n1 == 1         # 2 steps per rank, log interval 2: one record each
    files = sorted(os.listdir(tmp_path / 'work'))
    assert [f for f in files if f.endswith('.pth')] == ['epoch_1.pth', 'latest.pth'] and sum(f.endswith('.log.json') for f in files) == 1


def test_loader_batches_are_planned_ahead_and_equal_the_in_line_path(straight):
    """TrainStep(batch, next_batch) with DeviceLoader batches: prefetch accepts the next batch's points, its plan (with the batch
    kernel's launch) is made on the lookahead worker thread, the following step's Lookahead.take finds it, and losses and parameters
    equal, bitwise, those of steps that plan in line"""
    import threading
    from fcaf3d_amd import data as DT
    from fcaf3d_amd import plan as PL
    from fcaf3d_amd.runner import TrainStep
    cfg, dev = straight['cfg'], straight['dev']
    ds = DT.build_dataset(cfg.data.train)
    ld = DT.DeviceLoader(DT.ResidentScenes(ds, dev), ds.pipeline, 2, seed=SEED)
    runs = {}
    for ahead in (True, False):
        model = _fresh(dev)
        tr = TrainStep.from_config(model, cfg)
        bs = ld.batches(0)
        planner = PL.planner_of(model)
        threads, real = [], planner.run

        def spy(points, *a, **kw):
            threads.append((threading.current_thread().name, id(points)))
            return real(points, *a, **kw)
        planner.run = spy
        if ahead:
            assert model.prefetch(bs[0]['points'], gt=True) is True             # a loader batch is accepted
            la = model._lookahead
            assert len(la.pending) == 1
        losses = []
        for k, b in enumerate(bs):
            loss, _ = tr(b, bs[k + 1] if ahead and k + 1 < len(bs) else None)
            losses.append(loss.detach())
            if ahead:
                assert len(la.pending) == (1 if k + 1 < len(bs) else 0)         # this step's plan was taken, the next one's is waiting
        torch.cuda.synchronize()
        assert [i for _, i in threads] == [id(b['points']) for b in bs]         # one plan per batch, none made twice
        assert all(n.startswith('fc-plan') for n, _ in threads) if ahead else all(n == threading.current_thread().name for n, _ in threads)
        runs[ahead] = ([float(l) for l in losses], _params(model))
    assert runs[True][0] == runs[False][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[True][1], runs[False][1]))
    assert runs[True][0] == [r['loss'] for r in straight['rec'] if r['mode'] == 'train'][:3]
