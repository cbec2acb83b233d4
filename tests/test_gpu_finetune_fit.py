"""GPU: runner.fit fine-tuning from a checkpoint (load_from) with backbone.frozen_stages=1 and the README's paramwise_cfg, on the
disk fixture of tests/test_gpu_fit.py (7 synthetic scenes, num_points 4 000, 2 scenes per step, 3 steps per epoch) and the
two-level model: against a hand-written loop of TrainSteps, across a resume, and on two gloo ranks."""
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.test_finetune_cpu import README_PARAMWISE, build_model
from tests.test_fit_cpu import make_cfg
from tests.test_gpu_dist import _collect, _free_port

pytestmark = pytest.mark.gpu
SEED = 7
FROZEN = ('backbone.conv1.', 'backbone.layer1.')
OPTIMIZER = dict(type='AdamW', lr=0.001, weight_decay=0.0001, paramwise_cfg=README_PARAMWISE)


def _fresh(dev):
    model, _ = build_model(1)
    return model.to(dev).train()


def _params(model):
    return [p.detach().clone() for p in model.parameters()] + [b.detach().clone() for b in model.buffers()]


def _cfg(data, ckpt, **over):
    return make_cfg(data, log_config=dict(interval=1), optimizer=dict(OPTIMIZER), load_from=ckpt, **over)


def _pretrain(root, dev):
    """one ordinary epoch of the unfrozen model: the checkpoint to fine-tune from"""
    from fcaf3d_amd import fit
    model, _ = build_model()
    fit(model.to(dev).train(), make_cfg(os.path.join(root, 'data'), max_epochs=1), os.path.join(root, 'pre'), seed=SEED + 1)
    torch.cuda.synchronize()
    return os.path.join(root, 'pre', 'epoch_1.pth')


@pytest.fixture(scope='module')
def tuned(tmp_path_factory):
    """the straight two-epoch fine-tuning run; every step logged, both checkpoints kept"""
    from fcaf3d_amd import fit
    root = tmp_path_factory.mktemp('finetune')
    dev = torch.device('cuda:0')
    ckpt = _pretrain(str(root), dev)
    cfg = _cfg(root / 'data', ckpt, checkpoint_config=dict(interval=1, max_keep_ckpts=2))
    model = _fresh(dev)
    rec = fit(model, cfg, str(root / 'work'), seed=SEED)
    torch.cuda.synchronize()
    return dict(root=root, cfg=cfg, rec=rec, params=_params(model), dev=dev, ckpt=ckpt, model=model)


def test_fit_from_a_checkpoint_equals_a_hand_written_loop(tuned):
    from fcaf3d_amd import data as DT
    from fcaf3d_amd import load_checkpoint
    from fcaf3d_amd.runner import TrainStep
    cfg, dev = tuned['cfg'], tuned['dev']
    rec = tuned['rec']
    assert rec[0]['mode'] == 'load' and rec[0]['mismatched'] == [] and rec[0]['missing'] == [] and rec[0]['unexpected'] == []
    model = _fresh(dev)
    load_checkpoint(model, tuned['ckpt'], map_location=dev, strict=False)
    ds = DT.build_dataset(cfg.data.train)
    ld = DT.DeviceLoader(DT.ResidentScenes(ds, dev), ds.pipeline, 2, seed=SEED)
    tr = TrainStep.from_config(model, cfg)
    assert tr.optimizer.table is not None and tr.optimizer.steps == 0
    losses = []
    for epoch in range(2):
        tr.lr.set_epoch(epoch)
        bs = ld.batches(epoch)
        for k, b in enumerate(bs):
            loss, _ = tr(b, bs[k + 1] if k + 1 < len(bs) else None)
            losses.append(loss.detach())
        tr.epoch_end()
    losses = [float(l) for l in losses]
    train = [r for r in rec if r['mode'] == 'train']
    assert len(train) == len(losses) == 6 and all(np.isfinite(losses))
    assert [r['loss'] for r in train] == losses
    assert [(r['epoch'], r['iter']) for r in train] == [(e, i) for e in (1, 2) for i in (1, 2, 3)]      # from epoch 1, iteration 1
    assert [r['lr'] for r in train] == [0.001] * 3 + [0.0001] * 3                                      # the ONE schedule group's rate
    assert all(torch.equal(a, b) for a, b in zip(_params(model), tuned['params']))
    # the frozen stages still hold the checkpoint's tensors, running statistics included; the rest moved
    saved = torch.load(tuned['ckpt'], map_location='cpu', weights_only=False)['state_dict']
    for key, v in tuned['model'].state_dict().items():
        same = torch.equal(v.cpu(), saved[key])
        assert same == key.startswith(FROZEN), key


def test_resume_continues_the_fine_tuning_run(tuned, tmp_path):
    from fcaf3d_amd import fit
    dev = tuned['dev']
    cfg = _cfg(tuned['root'] / 'data', tuned['ckpt'], max_epochs=1)
    work = tmp_path / 'work'
    fit(_fresh(dev), cfg, str(work), seed=SEED)
    model = _fresh(dev)
    cfg.runner['max_epochs'] = 2
    rec = fit(model, cfg, str(work), seed=SEED, resume_from=str(work / 'latest.pth'))      # cfg.load_from is set too: resume_from wins
    torch.cuda.synchronize()
    assert all(r['mode'] == 'train' for r in rec)
    assert all(torch.equal(a, b) for a, b in zip(_params(model), tuned['params']))
    train = [r for r in tuned['rec'] if r['mode'] == 'train']
    assert [(r['epoch'], r['iter'], r['loss']) for r in rec] == [(r['epoch'], r['iter'], r['loss']) for r in train[3:]]
    ck = torch.load(work / 'latest.pth', map_location='cpu', weights_only=False)
    groups = ck['optimizer']['param_groups']                 # torch's layout: one group per trainable parameter, effective rates
    n_train = sum(p.requires_grad for p in model.parameters())
    assert len(groups) == n_train and sorted({round(g['lr'] / 1e-4, 6) for g in groups}) == [0.1, 1.0]
    assert sorted({g['weight_decay'] for g in groups}) == [0.0, 0.0001]


def _digest(tensors):
    return hashlib.sha256(b''.join(t.detach().cpu().contiguous().numpy().tobytes() for t in tensors)).hexdigest()


def _worker(rank, world, port, q, root, ckpt):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      FC_DIST_BACKEND='gloo')
    from fcaf3d_amd import dist as D
    from fcaf3d_amd import fit
    D.init_dist(backend='gloo')
    dev = torch.device('cuda:0')
    cfg = _cfg(os.path.join(root, 'data'), ckpt, max_epochs=1)
    model = _fresh(dev)
    rec = fit(model, cfg, os.path.join(root, 'work'), seed=SEED)
    torch.cuda.synchronize()
    named = list(model.named_parameters())
    q.put((rank, _digest(p for _, p in named), _digest(p for n, p in named if n.startswith(FROZEN)),
           sum(r['mode'] == 'load' for r in rec)))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_fine_tune_to_identical_parameters(tmp_path):
    dev = torch.device('cuda:0')
    ckpt = _pretrain(str(tmp_path), dev)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, str(tmp_path), ckpt)) for r in range(2)]
    for p in procs:
        p.start()
    res = _collect(q, procs, 2, 300)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, d0, f0, l0), (_, d1, f1, l1) = res
    assert d0 == d1, 'parameters diverged between the ranks'
    saved = torch.load(ckpt, map_location='cpu', weights_only=False)['state_dict']
    model, _ = build_model(1)
    assert f0 == f1 == _digest(saved[n] for n, _ in model.named_parameters() if n.startswith(FROZEN)), 'a frozen parameter moved'
    assert l0 == l1 == 1
