"""-m gpu: who builds the pre-split weight images, when and on which stream (fcaf3d_amd/weight_images.py), on the smallest training
case of tests/test_gpu_exec.py — two levels, one synthetic scene of 30 000 points, weight gradients on their own stream — through the
native executor and through the module path.  The launch lists and counts below were RECORDED at the commit before weight_images.py
existed (the same helpers, run against that tree): the single owner must enqueue exactly what the hand-threaded protocol did."""
import contextlib
import copy
import functools

import pytest
import torch

import fcaf3d_amd._lib as L
import fcaf3d_amd.functional as Fn
from fcaf3d_amd import executor as E
from fcaf3d_amd.runner import TrainStep
from tests.test_gpu_exec import _batch, _build, _dev

pytestmark = pytest.mark.gpu
PATHS = pytest.mark.parametrize('use_exec', [True, False], ids=['executor', 'modules'])

# image-build launches of the third and the fourth TrainStep call, in order, as recorded at the parent commit
_ALL, _ONE = 'fc_x6_weight_images', 'fc_x6_weight_image'
STEADY_STEP = {True: [(_ALL, 'side')], False: [(_ONE, 'main')] * 6 + [(_ALL, 'side')]}
# image-build launches per simple_test call in eval mode, as recorded at the parent commit:
# static_weights: call 1, call 2, the call after load_state_dict; not static: call 1, call 2
INFERENCE = {True: ([1, 0, 1], [1, 1]), False: ([22, 22, 22], [22, 22])}


@contextlib.contextmanager
def _census(dev):
    """-> the list that receives (entry point, 'main' | 'side') for every image-build launch made inside the block"""
    log, orig, side = [], L.call, Fn.wgrad_stream(dev).cuda_stream

    def logging_call(name, *a):
        if name.startswith('fc_x6_weight_image'):
            log.append((name, 'side' if a[-1] == side else 'main'))
        return orig(name, *a)
    L.call = logging_call
    try:
        yield log
    finally:
        L.call = orig


@contextlib.contextmanager
def _path(use_exec):
    """run the block on the executor or on the module path, weight gradients on their stream; afterwards: the intended path ran"""
    taken, orig = [], E.ENABLED
    from fcaf3d_amd.single_stage_sparse import SingleStageSparse3DDetector as Det
    inner = Det._exec_forward

    def spy(self, prog, st):
        taken.append(1)
        return inner(self, prog, st)
    E.ENABLED, Fn.WGRAD_ASYNC, Det._exec_forward = use_exec, True, spy
    try:
        yield
        torch.cuda.synchronize()
        assert bool(taken) == use_exec, 'the path under test did not run'
    finally:
        E.ENABLED, Fn.WGRAD_ASYNC, Det._exec_forward = orig, False, inner


def _trainer(dev, state=None):
    model, cfg = _build(levels=2)
    model = model.to(dev).train()
    if state is not None:
        model.load_state_dict(state)
    model.async_maps = True
    return model, TrainStep.from_config(model, cfg)


def _kernels(model):
    return [m.kernel for m in model.modules() if isinstance(getattr(m, 'kernel', None), torch.nn.Parameter)]


def steady_step_census(use_exec):
    """the image-build launches of each of four TrainStep calls"""
    dev = _dev()
    batch = _batch((81,), dev)
    with _path(use_exec):
        _, tr = _trainer(dev)
        logs = []
        for _ in range(4):
            with _census(dev) as log:
                tr(batch)
            logs.append(log)
    return logs


def inference_census(use_exec, static):
    dev = _dev()
    batch = _batch((82,), dev)
    model, _ = _build(levels=2)
    model = model.to(dev).eval()
    model.static_weights = static
    state = copy.deepcopy(model.state_dict())
    counts = []
    with _path(use_exec), torch.no_grad():
        for k in range(3 if static else 2):
            if k == 2:
                model.load_state_dict(state)
            with _census(dev) as log:
                model.simple_test(batch['points'], batch['img_metas'])
            counts.append(len(log))
    return counts


@PATHS
def test_steady_steps_launch_what_the_parent_launched(use_exec):
    logs = steady_step_census(use_exec)
    assert logs[2] == STEADY_STEP[use_exec] and logs[3] == STEADY_STEP[use_exec], logs


@functools.lru_cache(maxsize=None)
def _written_weights(use_exec):
    """runs A, A', B and C of the write test -> their step-3 losses.  Every run starts from the same seed and steps the same batch."""
    dev = _dev()
    batch = _batch((83,), dev)
    loss = {}
    with _path(use_exec):
        for run in ('A', "A'", 'B'):
            model, tr = _trainer(dev)
            tr(batch), tr(batch)
            if run == 'A':
                with torch.no_grad():
                    for p in _kernels(model):
                        p.mul_(0.5)                       # through torch: the version counters move
                state = copy.deepcopy(model.state_dict())
            elif run == 'B':
                for p in _kernels(model):
                    p.data.mul_(0.5)                      # behind torch's back: the caller has to say so
                tr.invalidate_images()
            loss[run] = float(tr(batch)[0])
        _, tr = _trainer(dev, state)
        loss['C'] = float(tr(batch)[0])
    return loss


@PATHS
def test_a_write_through_torch_is_seen(use_exec):
    loss = _written_weights(use_exec)
    print(loss)
    assert loss['A'] != loss["A'"], 'halving the kernels does not move the loss: the test is vacuous'
    assert loss['A'] == loss['B'] == loss['C'], loss


@PATHS
def test_invalidate_images_reaches_the_holder_after_the_program_cache_was_dropped(use_exec):
    """bench.py's sequence: drop the program cache, write the weights through .data, invalidate_images(), go on stepping.
    (Before the images had one owner the call did not reach the executor's holder once the cache was empty: this step read the
    old images there, loss 2.28212 instead of 2.44363.)"""
    dev = _dev()
    batch = _batch((83,), dev)
    with _path(use_exec):
        model, tr = _trainer(dev)
        tr(batch), tr(batch)
        model.__dict__.pop('_programs', None)
        for p in _kernels(model):
            p.data.mul_(0.5)
        tr.invalidate_images()
        loss = float(tr(batch)[0])
    assert loss == _written_weights(use_exec)['C'], (loss, _written_weights(use_exec))


@PATHS
def test_inference_builds_once_under_static_weights_and_always_without(use_exec):
    static, dynamic = INFERENCE[use_exec]
    assert inference_census(use_exec, True) == static
    assert inference_census(use_exec, False) == dynamic
    assert dynamic[1] > 0 and static[0] > 0 and static[2] > 0


@PATHS
def test_a_failed_step_leaves_nobody_trusted(use_exec):
    dev = _dev()
    batch = _batch((84,), dev)
    with _path(use_exec):
        model, tr = _trainer(dev)
        tr(batch)

        def fail(*a, **kw):
            raise RuntimeError('loss failed')
        model.neck_with_head.loss = fail
        try:
            with pytest.raises(RuntimeError, match='loss failed'):
                tr(batch)
        finally:
            del model.neck_with_head.loss
        with _census(dev) as log:
            model(return_loss=True, **batch)
        assert len(log) >= 1, 'a forward pass outside a TrainStep used images it had no right to trust'
