"""CPU: who waits for the weight images (fcaf3d_amd/executor.py IMAGE_WAIT).  A training program with the
weight gradients on their own stream carries one record on S_WGRAD / wait on S_MAIN of EV_IMG behind the stem's operators and in
front of the first operator that reads an image; every other program is the 'entry' program word for word."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import fcaf3d_amd as fa
from fcaf3d_amd import executor as E

OP, STREAM, EV = E.ROW_OP, E.ROW_STREAM, E.word(E.OP_WAIT, 'event')
IMAGE_READERS = (E.OP_CONV, E.OP_HEAD_FWD)        # OP_CONV is every convolution and GEMM launch of a program (its `img` word)
STEM = (E.OP_STEM_FWD, E.OP_COL_STATS, E.OP_NORM_POOL_FWD)


@functools.lru_cache(None)
def _model(levels):
    torch.manual_seed(0)
    cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=0.02)
    m = cfg.model
    m.backbone['n_outs'] = levels
    m.neck_with_head['in_channels'] = (64, 128, 256, 512)[:levels]
    m.neck_with_head.assigner['n_scales'] = levels
    return fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg'))


@contextlib.contextmanager
def _image_wait(mode):
    old, E.IMAGE_WAIT = E.IMAGE_WAIT, mode
    try:
        yield
    finally:
        E.IMAGE_WAIT = old


def _program(levels, training, wgrad_async, head_overlap, mode):
    return E.NetProgram(_model(levels), training, wgrad_async, head_overlap, image_wait=mode)


def _img_rows(ops):
    return [i for i, r in enumerate(ops) if r[OP] in (E.OP_RECORD, E.OP_WAIT) and r[EV] == E.EV_IMG]


def _same_program(a, b):
    """two builds of one model allocate their persistent scratch anew: equal up to those static addresses — the rows (which hold
    address INDICES), the tables' shapes and the dimension / map names"""
    assert np.array_equal(a.ops_f, b.ops_f) and np.array_equal(a.ops_b, b.ops_b)
    assert a.dim_names == b.dim_names and a.map_names == b.map_names and a.dyn == b.dyn
    assert a.n_addr == b.n_addr and a.arena == b.arena and a.alias == b.alias and a.grad_refs == b.grad_refs
    assert [i for i, _ in a.static] == [i for i, _ in b.static]


def test_the_default_is_the_first_reader_and_the_event_id_is_free():
    assert E.IMAGE_WAIT == 'first_reader'
    assert E.EV_BWD0 < E.EV_IMG < E.EV_HB and E.EV_IMG not in (E.EV_FORK, E.EV_HEAD_DONE, E.EV_W0, E.EV_W1, E.EV_WEND)


@pytest.mark.parametrize('head_overlap', [False, True])
@pytest.mark.parametrize('levels', [4, 2])
def test_training_program_with_wgrad_async_waits_at_the_first_reader(levels, head_overlap):
    p = _program(levels, True, True, head_overlap, 'first_reader')
    f, b = p.ops_f, p.ops_b
    assert p.img_pair
    at = _img_rows(f)
    assert len(at) == 2 and at[1] == at[0] + 1, 'exactly one pair, adjacent'
    rec, wait = f[at[0]], f[at[1]]
    assert (rec[OP], rec[STREAM]) == (E.OP_RECORD, E.S_WGRAD) and (wait[OP], wait[STREAM]) == (E.OP_WAIT, E.S_MAIN)
    assert not _img_rows(b), 'the backward list carries no image event'
    # behind the stem's operators, in front of every operator with an image word
    before = f[:at[0]]
    assert set(STEM) <= set(before[:, OP]) and not np.isin(before[:, OP], IMAGE_READERS).any()
    assert np.isin(f[at[1] + 1:, OP], IMAGE_READERS).any()
    assert f[at[1] + 1][OP] == E.OP_CONV, 'the pair stands directly in front of the first image reader'
    # every head-stream operator stands behind a fork that the main stream recorded after the wait
    head = [i for i, r in enumerate(f) if r[STREAM] == E.S_HEAD]
    assert bool(head) == head_overlap
    forks = [i for i, r in enumerate(f) if r[OP] == E.OP_RECORD and r[STREAM] == E.S_MAIN and E.EV_FORK <= r[EV] < E.EV_HEAD_DONE]
    for i in head:
        assert any(at[1] < k < i for k in forks), 'a head-stream operator in front of the image wait'
        if f[i][OP] == E.OP_WAIT:
            assert any(at[1] < k < i and f[k][EV] == f[i][EV] for k in forks)
    # without the two rows it is the 'entry' program
    q = _program(levels, True, True, head_overlap, 'entry')
    assert not q.img_pair and not _img_rows(q.ops_f) and not _img_rows(q.ops_b)
    # (one field of a forward row names a ROW, the convolution a BatchNorm takes its statistics from, stored + 1: it moves with the rows)
    g = np.delete(f, at, axis=0)
    link = E.word(E.OP_BN_FWD, 'producer')
    moved = (g[:, OP] == E.OP_BN_FWD) & (g[:, link] - 1 > at[1])
    g[moved, link] -= 2
    p.ops_f = g
    _same_program(p, q)


@pytest.mark.parametrize('head_overlap', [False, True])
@pytest.mark.parametrize('levels', [4, 2])
def test_programs_without_wgrad_async_and_inference_programs_are_the_entry_programs(levels, head_overlap):
    for training, wgrad_async in ((True, False), (False, False), (False, True)):
        if not training:
            _model(levels).eval()
        try:
            p = _program(levels, training, wgrad_async, head_overlap, 'first_reader')
            q = _program(levels, training, wgrad_async, head_overlap, 'entry')
        finally:
            _model(levels).train()
        assert not p.img_pair and not q.img_pair
        for ops in (p.ops_f, p.ops_b):
            assert not _img_rows(ops)
        _same_program(p, q)


def test_the_switch_is_part_of_the_program_cache_key():
    det = _model(2)
    import fcaf3d_amd.functional as Fn
    old = Fn.WGRAD_ASYNC
    Fn.WGRAD_ASYNC = True
    try:
        with _image_wait('first_reader'):
            a = E.program_for(det, True)
        with _image_wait('entry'):
            b = E.program_for(det, True)
        with _image_wait('first_reader'):
            c = E.program_for(det, True)
    finally:
        Fn.WGRAD_ASYNC = old
        det.__dict__.pop('_programs', None)
    assert a is c and a is not b and a.img_pair and not b.img_pair
