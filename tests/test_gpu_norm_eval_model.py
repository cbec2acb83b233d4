"""-m gpu: training on running statistics and with a frozen neck on the model — the native executor against the
per-operator module path for every declared combination (comparison and bound of tests/test_gpu_finetune.py::_compare_paths), the
model against the CPU oracle whose eval-mode BatchNorm read the running statistics while gamma / beta stay leaves (bounds of
tests/test_gpu_model.py), hand-made flags on the module path, two iterations of runner.fit and two head-only TrainStep steps.  Scale of tests/test_gpu_finetune.py: the two-level model, two scenes of
6 000 points, every case starting from the state after two ordinary training steps, so no running statistic is 0 / 1."""
import copy

import numpy as np
import pytest
import torch

import fcaf3d_amd.functional as Fn
from fcaf3d_amd import executor as E
from fcaf3d_amd import nn as MEnn
from oracle import model_oracle as MO
from oracle.record import RecordDecisions

from tests.test_fit_cpu import make_cfg
from tests.test_gpu_finetune import _batch, _dev, _rel, _rel_model, _run, _scenes, trained      # noqa: F401 (trained: the fixture)
from tests.test_norm_eval_cpu import build, check_plan_program

pytestmark = pytest.mark.gpu

# (frozen_stages, norm_eval backbone, norm_eval neck, frozen_neck) of the two-level model
COMBOS = {
    'norm_eval-backbone': (-1, True, False, False),
    'norm_eval-both': (-1, True, True, False),
    'frozen1-norm_eval': (1, True, False, False),
    'frozen_neck': (-1, False, False, True),
    'head-only': (2, False, False, True),
}


def _model(trained, name, dev):
    k, ne_b, ne_n, fn = COMBOS[name]
    model, cfg = build(2, k, ne_b, ne_n, fn)
    model.load_state_dict(trained)
    return model.to(dev).train(), cfg


def _eval_norm_prefixes(model):
    return tuple(n + '.' for n, m in model.named_modules() if isinstance(m, MEnn.MinkowskiBatchNorm) and not m.training)


@pytest.mark.parametrize('overlap', [True, False], ids=['overlap', 'serial'])
@pytest.mark.parametrize('name', list(COMBOS))
def test_executor_equals_module_path(trained, name, overlap):
    dev = _dev()
    model, _ = _model(trained, name, dev)
    Fn.WGRAD_ASYNC = overlap
    model.neck_with_head.head_overlap = overlap
    model.async_maps = overlap
    try:
        p = E.program_for(model, True)
        assert p is not None and p.plan == E.freeze_plan(model) and p.plan is not None
        check_plan_program(model, p)
        batch = _batch(dev)
        state = copy.deepcopy(model.state_dict())
        ref = _run(model, batch, False)
        model.load_state_dict(state)                   # same running statistics at the start of both runs
        got = _run(model, batch, True)                 # (asserts through the _exec_forward spy that the executor ran)
    finally:
        Fn.WGRAD_ASYNC = False
    for kind in range(4):
        for l in range(2):
            assert torch.equal(got[0][kind][l], ref[0][kind][l]), f'forward output {kind} of level {l} differs'
    assert got[1] == ref[1], (got[1], ref[1])
    ev = _eval_norm_prefixes(model)
    assert ev
    for key, b in ref[3].items():
        assert torch.equal(got[3][key], b), f'buffer {key} differs between the paths'
        if key.startswith(ev):
            assert torch.equal(b, state[key]), f'buffer {key} of an eval-mode BatchNorm moved'
        elif key.endswith('num_batches_tracked'):
            assert int(b) == int(state[key]) + 2, key      # (_run makes two forward passes)
    frozen = {n for n, q in model.named_parameters() if not q.requires_grad}
    errs = {}
    for key, g in ref[2].items():
        assert (g is None) == (key in frozen) and (got[2][key] is None) == (key in frozen), key
        if key not in frozen:
            errs[key] = _rel(got[2][key], g)
    assert errs
    worst = max(errs, key=errs.get)
    print(f'{name} overlap={overlap}: worst gradient difference executor vs module path {errs[worst]:.2e} ({worst}); backward list '
          f'{len(p.ops_b)} rows')
    assert errs[worst] < 2e-5, (worst, errs[worst])


@pytest.mark.parametrize('name', ['norm_eval-both', 'frozen1-norm_eval', 'frozen_neck'])
def test_against_the_oracle(trained, name, monkeypatch):
    """losses and every trainable gradient against oracle.model_oracle.forward_train whose BatchNorm in eval mode read the running
    statistics (gamma / beta leaves wherever they train); equal discrete decisions (DecisionTape) and the fp64 arbitration of
    tests/test_gpu_finetune.py::test_frozen_prefix_against_the_oracle: the project's standing bounds"""
    dev = _dev()
    model, cfg = _model(trained, name, dev)
    m = cfg.model
    ev = _eval_norm_prefixes(model)
    frozen = {n for n, q in model.named_parameters() if not q.requires_grad}
    trainable = {n for n, q in model.named_parameters() if q.requires_grad}
    P = {key: v.detach().cpu().clone().requires_grad_(key in trainable) for key, v in model.state_dict().items()}
    orig_bn = MO.bn

    def bn(x, P_, pre, act=None, residual=None):
        MO.TRAINING = not (pre + '.').startswith(ev)
        try:
            return orig_bn(x, P_, pre, act=act, residual=residual)
        finally:
            MO.TRAINING = True
    monkeypatch.setattr(MO, 'bn', bn)
    pts, gts, labs = _scenes()
    rm0 = {key: v.clone() for key, v in model.state_dict().items() if 'running' in key or 'num_batches' in key}
    model.zero_grad(set_to_none=True)
    with RecordDecisions(model) as rec:
        losses_g = model(return_loss=True, **_batch(dev))
    sum(losses_g.values()).backward()
    torch.cuda.synchronize()
    for key, v in model.state_dict().items():
        if key in rm0 and key.startswith(ev):
            assert torch.equal(v, rm0[key]), f'{key} of an eval-mode BatchNorm moved'
    tape = rec.tape()
    MO.TAPE = tape
    try:
        losses_o = MO.forward_train(P, m, pts, gts, labs)
    finally:
        MO.TAPE = None
    assert tape.i == len(tape.relu), 'the oracle must have consumed every recorded ReLU'
    for key in ('loss_centerness', 'loss_bbox', 'loss_cls'):
        print(f'{name} {key}: HIP {float(losses_g[key]):.7f} oracle {float(losses_o[key]):.7f}')
        assert _rel_model(losses_g[key], losses_o[key]) < 1e-4, (key, float(losses_g[key]), float(losses_o[key]))
    sum(losses_o.values()).backward()
    errs = {}
    for key, p in model.named_parameters():
        if key in frozen:
            assert p.grad is None and P[key].grad is None, key
        else:
            errs[key] = _rel_model(p.grad, P[key].grad)
    worst = max(errs, key=errs.get)
    print(f'{name}: gradients vs the fp32 oracle with equal decisions: worst {errs[worst]:.2e} ({worst}), median {np.median(list(errs.values())):.2e}')
    over = [key for key, v in errs.items() if v >= 1e-4]
    if over:
        P64 = {key: (v.detach().double().requires_grad_(v.requires_grad) if v.dtype.is_floating_point else v) for key, v in P.items()}
        MO.TAPE = tape.replay()
        try:
            sum(MO.forward_train(P64, m, pts, gts, labs).values()).backward()
        finally:
            MO.TAPE = None
        named = dict(model.named_parameters())
        for key in over:
            e_hip, e_o = _rel_model(named[key].grad, P64[key].grad), _rel_model(P[key].grad, P64[key].grad)
            print(f'   {key}: vs the fp32 oracle {errs[key]:.2e}; vs the fp64 oracle (same decisions): HIP {e_hip:.2e}, fp32 oracle {e_o:.2e}')
            assert e_hip < max(1e-4, 2.0 * e_o), (key, e_hip, e_o)


def test_hand_made_flags_train_on_the_module_path(trained):
    """a lone layer2.eval() and one neck kernel frozen by hand on a model that declared nothing: no program, and autograd on the module
    path — which raised in the backward before fc_bn_eval_bwd — delivers every trainable gradient"""
    dev = _dev()
    model, _ = build(2)
    model.load_state_dict(trained)
    model = model.to(dev).train()
    model.backbone.layer2.eval()
    model.neck_with_head.out_block_0[0].kernel.requires_grad = False
    assert E.freeze_plan(model) is None
    state = copy.deepcopy(model.state_dict())
    taken = []
    orig = type(model)._exec_forward
    type(model)._exec_forward = lambda self, prog, st: taken.append(1) or orig(self, prog, st)
    try:
        losses = model(return_loss=True, **_batch(dev))
        sum(losses.values()).backward()
    finally:
        type(model)._exec_forward = orig
    torch.cuda.synchronize()
    assert not taken
    for key, q in model.named_parameters():
        assert (q.grad is None) == (key == 'neck_with_head.out_block_0.0.kernel'), key
        assert q.grad is None or bool(torch.isfinite(q.grad).all()), key
    for key, v in model.state_dict().items():
        if key.startswith('backbone.layer2.') and ('running' in key or 'num_batches' in key):
            assert torch.equal(v, state[key]), key


def test_fit_with_norm_eval_and_a_frozen_neck(trained, tmp_path):
    """two iterations of runner.fit on a norm_eval + frozen_neck config: the frozen blocks' parameters and every eval-mode BatchNorm's
    buffers are bit-unchanged, the head and the backbone moved, the executor ran, the checkpoint reloads"""
    from fcaf3d_amd import fit, load_checkpoint
    dev = _dev()
    cfg = make_cfg(tmp_path / 'data', samples_per_gpu=3, max_epochs=1, log_config=dict(interval=1))
    model, _ = build(2, -1, True, False, True)
    model.load_state_dict(trained)
    model = model.to(dev).train()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    taken = []
    orig = type(model)._exec_forward
    type(model)._exec_forward = lambda self, prog, st: taken.append(prog.plan) or orig(self, prog, st)
    try:
        rec = fit(model, cfg, str(tmp_path / 'work'), seed=7)
    finally:
        type(model)._exec_forward = orig
    torch.cuda.synchronize()
    train = [r for r in rec if r['mode'] == 'train']
    assert len(train) == 2 and all(np.isfinite(r['loss']) for r in train)
    assert len(taken) == 2 and all(t is not None and not isinstance(t, int) for t in taken)
    after = model.state_dict()
    neck = ('neck_with_head.up_block_', 'neck_with_head.out_block_')
    for key, v in before.items():
        if key.startswith(neck) or 'running' in key or 'num_batches' in key:
            assert torch.equal(after[key], v), f'{key} changed'
        else:
            assert not torch.equal(after[key], v), f'{key} did not change'
    fresh, _ = build(2, -1, True, False, True)
    ck = load_checkpoint(fresh, str(tmp_path / 'work' / 'latest.pth'), map_location='cpu', strict=True)
    assert ck['meta']['iter'] == 2
    assert all(torch.equal(v.cpu(), fresh.state_dict()[k]) for k, v in after.items())


def test_two_head_only_steps(trained):
    """runner.TrainStep (flat buffers, FlatAdamW, grad clip) over a trainable set that holds the head alone: two steps through the
    executor move the head's parameters and nothing else"""
    from fcaf3d_amd.runner import TrainStep
    dev = _dev()
    model, cfg = _model(trained, 'head-only', dev)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tr = TrainStep.from_config(model, cfg)
    trainable = {n for n, q in model.named_parameters() if q.requires_grad}
    assert len(tr.flat.params) == len(trainable) and all(n.startswith('neck_with_head.') and not n.startswith(('neck_with_head.up_block_', 'neck_with_head.out_block_')) for n in trainable)
    taken = []
    orig = type(model)._exec_forward
    type(model)._exec_forward = lambda self, prog, st: taken.append(len(prog.ops_b)) or orig(self, prog, st)
    try:
        for s in ((120, 121), (122, 123)):
            tr(_batch(dev, s))
    finally:
        type(model)._exec_forward = orig
    torch.cuda.synchronize()
    assert len(taken) == 2 and taken[0] == taken[1] < 40
    after = model.state_dict()
    for key, v in before.items():
        assert torch.equal(after[key], v) == (key not in trainable), key
    norm = float(torch.sqrt(sum((q.grad.double() ** 2).sum() for n, q in model.named_parameters() if n in trainable)))
    assert abs(float(tr.last_grad_norm) - norm) <= 1e-5 * norm
