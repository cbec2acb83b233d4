"""-m gpu: training with a frozen backbone prefix (MEResNet3D(frozen_stages=k)) — the rows the native
executor emits, the executor against the per-operator module path (comparison and bound of tests/test_gpu_exec.py), both against
the CPU oracle with the frozen stages' BatchNorm on their running statistics (bounds of tests/test_gpu_model.py), two optimizer
steps with the README's paramwise_cfg, and the pruned-tail program.  All on the two-level model of tests/test_gpu_dist.py with two
scenes of 6 000 points; the state every case starts from has seen two ordinary training steps, so no running statistic is 0 / 1."""
import copy

import numpy as np
import pytest
import torch

import fcaf3d_amd as fa
import fcaf3d_amd.functional as Fn
from fcaf3d_amd import executor as E
from fcaf3d_amd.runner import TrainStep
from fcaf3d_amd.synthetic import make_scene
from oracle import model_oracle as MO
from oracle.record import RecordDecisions

from tests.test_finetune_cpu import README_PARAMWISE, build_model, check_program_shape

pytestmark = pytest.mark.gpu

SEEDS = (100, 101)


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _rel(a, b):                       # tests/test_gpu_exec.py
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(1e-12, float(b.abs().max()))


def _rel_model(a, b):                 # tests/test_gpu_model.py
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / max(1e-3, float(b.abs().max()))


def _scenes(seeds=SEEDS):
    out = [make_scene(s, n_points=6000) for s in seeds]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def _batch(dev, seeds=SEEDS):
    pts, gts, labs = _scenes(seeds)
    return dict(points=[torch.from_numpy(p).to(dev) for p in pts],
                gt_bboxes_3d=[fa.DepthInstance3DBoxes(torch.from_numpy(g), origin=(.5, .5, .5)) for g in gts],
                gt_labels_3d=[torch.from_numpy(l).to(dev) for l in labs],
                img_metas=[dict(box_type_3d=fa.DepthInstance3DBoxes) for _ in pts])


@pytest.fixture(scope='module')
def trained():
    """the state dict (CPU) of the two-level model after two ordinary training steps"""
    dev = _dev()
    model, cfg = build_model()
    model = model.to(dev).train()
    tr = TrainStep.from_config(model, cfg)
    for s in ((110, 111), (112, 113)):
        tr(_batch(dev, s))
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert not any(bool((v == 0).all()) for k, v in sd.items() if k.endswith('running_mean'))
    return sd


def _frozen_model(trained, k, dev, **over):
    model, cfg = build_model(k)
    model.load_state_dict(trained)
    for key, v in over.items():
        setattr(model.neck_with_head, key, v)
    return model.to(dev).train(), cfg


def _frozen_prefixes(k):
    return ('backbone.conv1.',) * (k >= 0) + tuple(f'backbone.layer{i}.' for i in range(1, k + 1))


@pytest.mark.parametrize('k', [-1, 0, 1, 2])
def test_program_of_a_frozen_prefix(trained, k):
    dev = _dev()
    model, _ = _frozen_model(trained, k, dev)
    p = E.program_for(model, True)
    assert p is not None and p.frozen == k
    plain = None
    if k == -1:
        ref, _ = build_model()
        ref.load_state_dict(trained)
        plain = E.program_for(ref.to(dev).train(), True)
    check_program_shape(model, p, k, plain)


def _run(model, batch, use_exec, tail0=None):
    """tests/test_gpu_exec.py::_run, with `p.grad is None` recorded for a parameter that got no gradient"""
    E.ENABLED = use_exec
    try:
        model.zero_grad(set_to_none=True)
        taken = []
        orig = type(model)._exec_forward

        def spy(self, prog, st):
            taken.append(prog.tail0)
            return orig(self, prog, st)
        type(model)._exec_forward = spy
        try:
            feats = [list(v) for v in model.extract_feat(batch['points'], batch['img_metas'])]
            outs = [[lvl.full.detach().clone() for lvl in kind] for kind in feats]
            model.zero_grad(set_to_none=True)
            losses = model(return_loss=True, **batch)
            sum(losses.values()).backward()
        finally:
            type(model)._exec_forward = orig
        torch.cuda.synchronize()
        assert bool(taken) == use_exec, 'the path under test did not run'
        if use_exec and tail0 is not None:
            assert taken == [tail0, tail0], taken
        grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in model.named_parameters()}
        bufs = {k: v.detach().clone() for k, v in model.named_buffers()}
        return outs, {k: float(v) for k, v in losses.items()}, grads, bufs
    finally:
        E.ENABLED = True


def _compare_paths(model, batch, k, levels=2, tail0=None):
    state = copy.deepcopy(model.state_dict())
    ref = _run(model, batch, False)
    model.load_state_dict(state)                   # same running statistics at the start of both runs
    got = _run(model, batch, True, tail0)
    for kind in range(4):
        for l in range(levels):
            assert torch.equal(got[0][kind][l], ref[0][kind][l]), f'forward output {kind} of level {l} differs'
    assert got[1] == ref[1], (got[1], ref[1])
    for key, b in ref[3].items():
        assert torch.equal(got[3][key], b), f'buffer {key} (running statistics) differs'
        if key.startswith(_frozen_prefixes(k)):
            assert torch.equal(b, state[key]), f'buffer {key} of a frozen stage moved'
    errs = {}
    for key, g in ref[2].items():
        frozen = key.startswith(_frozen_prefixes(k))
        assert (g is None) == frozen and (got[2][key] is None) == frozen, key
        if not frozen:
            errs[key] = _rel(got[2][key], g)
    worst = max(errs, key=errs.get)
    print(f'frozen_stages={k} tail0={tail0}: worst gradient difference executor vs module path {errs[worst]:.2e} ({worst})')
    assert errs[worst] < 2e-5, (worst, errs[worst])


@pytest.mark.parametrize('k,overlap', [(0, True), (1, True), (2, True), (1, False), (2, False)])
def test_executor_equals_module_path_with_a_frozen_prefix(trained, k, overlap):
    dev = _dev()
    model, _ = _frozen_model(trained, k, dev)
    Fn.WGRAD_ASYNC = overlap
    model.neck_with_head.head_overlap = overlap
    model.async_maps = overlap
    try:
        _compare_paths(model, _batch(dev), k)
    finally:
        Fn.WGRAD_ASYNC = False


def test_pruned_tail_program_with_a_frozen_prefix(trained):
    dev = _dev()
    batch = _batch(dev)
    probe, _ = _frozen_model(trained, 1, dev)
    with torch.no_grad():
        feats = [list(v) for v in probe.extract_feat(batch['points'], batch['img_metas'])]
    n1 = int(feats[0][1].full.shape[0])            # rows of the coarse level over both scenes: each scene's share stays below it, and
    model, _ = _frozen_model(trained, 1, dev, pts_threshold=n1)      # each scene's finest level (8 x its share) exceeds it
    with torch.no_grad():
        model.neck_with_head.cls_conv.kernel.normal_(0, 0.5)         # spread the scores: no near-ties in the top-k
    _compare_paths(model, batch, 1, tail0=True)


@pytest.mark.parametrize('k', [0, 1, 2])
def test_frozen_prefix_against_the_oracle(trained, k, monkeypatch):
    """losses and every trainable gradient against oracle.model_oracle.forward_train whose BatchNorm of the frozen stages reads the
    running statistics; equal discrete decisions (DecisionTape) and the fp64 arbitration of
    tests/test_gpu_model.py::test_forward_train_parity: 1e-4 of the tensor's scale against the fp32 oracle, or as close to the fp64
    gradient as the fp32 oracle is"""
    dev = _dev()
    model, cfg = _frozen_model(trained, k, dev)
    m = cfg.model
    frozen = _frozen_prefixes(k)
    P = {key: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point and not key.startswith(frozen) and
                                                      not key.endswith(('running_mean', 'running_var')))
         for key, v in model.state_dict().items()}
    orig_bn = MO.bn

    def bn(x, P_, pre, act=None, residual=None):
        MO.TRAINING = not pre.startswith(frozen)
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
        if key in rm0 and key.startswith(frozen):
            assert torch.equal(v, rm0[key]), f'{key} of a frozen stage moved'
    tape = rec.tape()
    MO.TAPE = tape
    try:
        losses_o = MO.forward_train(P, m, pts, gts, labs)
    finally:
        MO.TAPE = None
    assert tape.i == len(tape.relu), 'the oracle must have consumed every recorded ReLU'
    for key in ('loss_centerness', 'loss_bbox', 'loss_cls'):
        print(f'frozen_stages={k} {key}: HIP {float(losses_g[key]):.7f} oracle {float(losses_o[key]):.7f}')
        assert _rel_model(losses_g[key], losses_o[key]) < 1e-4, (key, float(losses_g[key]), float(losses_o[key]))
    sum(losses_o.values()).backward()
    errs = {}
    for key, p in model.named_parameters():
        if key.startswith(frozen):
            assert p.grad is None and P[key].grad is None, key
        else:
            errs[key] = _rel_model(p.grad, P[key].grad)
    worst = max(errs, key=errs.get)
    print(f'frozen_stages={k}: gradients vs the fp32 oracle with equal decisions: worst {errs[worst]:.2e} ({worst}), median {np.median(list(errs.values())):.2e}')
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


def test_two_steps_with_a_frozen_stage_and_the_readme_recipe(trained):
    dev = _dev()
    model, cfg = _frozen_model(trained, 1, dev)
    cfg.optimizer['paramwise_cfg'] = README_PARAMWISE
    before = {key: v.detach().clone() for key, v in model.state_dict().items()}
    frozen = _frozen_prefixes(1)
    tr = TrainStep.from_config(model, cfg)
    assert tr.optimizer.table is not None
    assert all(p.requires_grad for p in tr.flat.params) and len(tr.flat.params) == sum(p.requires_grad for p in model.parameters())
    taken = []
    orig = type(model)._exec_forward

    def spy(self, prog, st):
        taken.append(prog.frozen)
        return orig(self, prog, st)
    type(model)._exec_forward = spy
    try:
        for s in ((120, 121), (122, 123)):
            tr(_batch(dev, s))
    finally:
        type(model)._exec_forward = orig
    torch.cuda.synchronize()
    assert taken == [1, 1]
    after = model.state_dict()
    for key, v in before.items():
        if key.startswith(frozen):
            assert torch.equal(after[key], v), f'{key} of a frozen stage changed'
        elif key.endswith('num_batches_tracked'):
            assert int(after[key]) == int(v) + 2, key
        else:
            assert not torch.equal(after[key], v), f'{key} did not change'
    named = dict(model.named_parameters())
    assert all(named[key].grad is None for key in named if key.startswith(frozen))
    norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for key, p in named.items() if not key.startswith(frozen))))
    print(f'last_grad_norm {float(tr.last_grad_norm):.6f}, 2-norm over the trainable gradients {norm:.6f}')
    assert abs(float(tr.last_grad_norm) - norm) <= 1e-5 * norm
