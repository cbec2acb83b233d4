"""CPU: the operator lists of the native executor (fcaf3d_amd/executor.py) are built from the module graph without a GPU —
structure checks of what fc_exec (csrc/exec.hip) will walk: operand indices in range, every trainable tensor has a place its
gradient is written to, forward / backward operator counts follow the model (the numerics are the GPU tests' business:
tests/test_gpu_exec.py compares the executor with the per-operator path bit for bit)."""
import functools

import numpy as np
import pytest
import torch

import fcaf3d_amd as fa
from fcaf3d_amd import executor as E
from fcaf3d_amd import nn as MEnn

OP, STREAM = E.ROW_OP, E.ROW_STREAM        # columns of an operator row: these two, then E.word(operator, field) (csrc/exec_ops.h)


def _model(levels=4, name='fcaf3d_scannet-3d-18class'):
    torch.manual_seed(0)
    cfg = fa.get_config(name, voxel_size=0.02)
    m = cfg.model
    m.backbone['n_outs'] = levels
    m.neck_with_head['in_channels'] = (64, 128, 256, 512)[:levels]
    m.neck_with_head.assigner['n_scales'] = levels
    return fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg'))


_cached_model = functools.lru_cache(None)(_model)       # for tests that only build programs from it


@pytest.mark.parametrize('levels,wgrad_async,head_overlap', [(4, False, False), (4, True, True), (2, True, True), (1, False, False)])
def test_training_program_structure(levels, wgrad_async, head_overlap):
    det = _model(levels)
    assert E.supported(det)
    p = E.NetProgram(det, True, wgrad_async, head_overlap)
    convs = [m for m in det.modules() if isinstance(m, MEnn.MinkowskiConvolution)]
    gents = [m for m in det.modules() if isinstance(m, MEnn.MinkowskiGenerativeConvolutionTranspose)]
    n_conv = len(convs) - 3 - 1                       # the three 1x1 head kernels run as one packed GEMM per level; the stem has its own operator
    n_gemm = len(gents) + levels                      # generative convolutions + the packed head GEMM of every level
    assert p.n_conv_f == n_conv + n_gemm
    assert p.n_conv_b == n_conv + n_gemm              # one backward-data launch per forward launch (the stem's input needs none)
    f, b = p.ops_f, p.ops_b
    assert int((b[:, OP] == E.OP_WGRAD).sum()) == n_conv + n_gemm and int((b[:, OP] == E.OP_STEM_WGRAD).sum()) == 1
    n_bn = len([m for m in det.modules() if isinstance(m, MEnn.MinkowskiBatchNorm)])
    assert int((f[:, OP] == E.OP_BN_FWD).sum()) == n_bn == int((b[:, OP] == E.OP_BN_BWD).sum())
    # every parameter that requires a gradient is written by some operator (or by the head's bias / scale reductions)
    nh = det.neck_with_head
    direct = {id(nh.cls_conv.bias)} | {id(s.scale) for s in nh.scales}
    reached = {off for _, off in p.grad_refs} | {int(o) // 4 for o in p._small_goff}
    for prm in det.parameters():
        assert id(prm) in direct or p._goff[id(prm)] in reached, 'a parameter has no gradient destination'
    # streams and events: cross-stream operators only in the overlapped program, every wait has its record
    for ops in (f, b):
        assert set(np.unique(ops[:, STREAM])) <= ({0, 1, 2} if (wgrad_async or head_overlap) and levels > 1 or wgrad_async else {0})
        rec = set(ops[ops[:, OP] == E.OP_RECORD][:, E.word(E.OP_RECORD, 'event')])
        assert set(ops[ops[:, OP] == E.OP_WAIT][:, E.word(E.OP_WAIT, 'event')]) <= rec
    if not (wgrad_async or head_overlap):
        assert not (f[:, OP] == E.OP_RECORD).any() and not (b[:, OP] == E.OP_RECORD).any()


def test_inference_program_has_no_backward_and_no_saved_statistics():
    det = _model(4).eval()
    p = E.NetProgram(det, False, False, True)
    assert len(p.ops_b) == 0 and not p.arena['b']
    bn = p.ops_f[p.ops_f[:, OP] == E.OP_BN_FWD]
    assert (bn[:, E.word(E.OP_BN_FWD, 'train')] == 0).all() and (bn[:, E.word(E.OP_BN_FWD, 'mean')] == -1).all()          # eval mode: running statistics, nothing saved


def test_bottleneck_and_wide_heads_fall_back():
    torch.manual_seed(0)
    cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=0.02)
    m = cfg.model
    m.backbone['depth'] = 50
    m.backbone['n_outs'] = 2
    m.neck_with_head['in_channels'] = (256, 512)
    m.neck_with_head.assigner['n_scales'] = 2
    assert not E.supported(fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg')))
    cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=0.02)
    cfg.model.neck_with_head['n_classes'] = 80
    assert not E.supported(fa.build_detector(cfg.model, train_cfg=cfg.model.get('train_cfg'), test_cfg=cfg.model.get('test_cfg')))


def test_batchnorm_fusions_are_wired_consistently():
    """r5: the static links of the BatchNorm fusions — every forward BatchNorm names the convolution that wrote its input and that
    convolution names a statistics table; a backward BatchNorm that names a producer names a backward-data convolution whose result
    has the layer's shape and which carries the layer's input / statistics; a second gradient contribution is either handed to the
    BatchNorm (gy2) or added by OP_ADD, never both; nothing is linked when FC_BN_FUSE is off."""
    import fcaf3d_amd.functional as Fn
    det = _model(4)
    CV, BF, BB = (functools.partial(E.word, op) for op in (E.OP_CONV, E.OP_BN_FWD, E.OP_BN_BWD))
    for wgrad_async, head_overlap in ((True, True), (False, False)):
        p = E.NetProgram(det, True, wgrad_async, head_overlap)
        f, b = p.ops_f, p.ops_b
        bn_f = f[f[:, OP] == E.OP_BN_FWD]
        assert (bn_f[:, BF('producer')] > 0).all(), 'every training-mode BatchNorm takes its statistics from a producer'
        for row in bn_f:
            prod = f[row[BF('producer')] - 1]
            assert prod[OP] == E.OP_CONV and prod[CV('dir')] == 0 and prod[CV('stats')] > 0 and prod[CV('out')] == row[BF('x')], \
                'the producer wrote the BatchNorm input'
            assert prod[CV('cout')] == row[BF('c')] * row[BF('groups')] and row[BF('groups')] in (1, 8)       # columns = groups x channels
        assert int(((f[:, OP] == E.OP_CONV) & (f[:, CV('stats')] > 0)).sum()) == len(bn_f)
        bn_b = b[b[:, OP] == E.OP_BN_BWD]
        linked = bn_b[bn_b[:, BB('producer')] > 0]
        assert len(linked) >= 36 and len(bn_b) == len(bn_f)
        for row in linked:
            prod = b[row[BB('producer')] - 1]
            assert prod[OP] == E.OP_CONV and prod[CV('dir')] == 1 and prod[CV('stats')] > 0
            assert prod[CV('bn_x')] - 1 == row[BB('x')] and prod[CV('bn_mean')] == row[BB('mean')] and prod[CV('bn_var')] == row[BB('var')] \
                and prod[CV('cout')] == row[BB('c')]                         # layer input, mean, var, channels
            # the contribution that arrived last = the producer's result
            last = row[BB('gy2')] - 1 if row[BB('gy2')] > 0 else row[BB('gy')]
            assert prod[CV('out')] == last
            if row[BB('gy2')] > 0:
                assert prod[CV('bn_add')] - 1 == row[BB('gy')], 'the earlier contribution rides along as `add`'
            assert (prod[CV('bn_y')] > 0) == (row[BB('y')] >= 0), "act' from the output exactly where the layer had a residual"
        # stream order: a linked producer precedes its BatchNorm and sits on the same stream
        idx = {tuple(r): i for i, r in enumerate(map(tuple, b))}
        for row in linked:
            assert row[BB('producer')] - 1 < idx[tuple(row)] and b[row[BB('producer')] - 1][STREAM] == row[STREAM]
    Fn.BN_FUSE = False
    try:
        p0 = E.NetProgram(det, True, True, True)
        assert not (p0.ops_f[:, CV('stats')][p0.ops_f[:, OP] == E.OP_CONV] > 0).any()
        assert not (p0.ops_f[:, BF('producer')][p0.ops_f[:, OP] == E.OP_BN_FWD] > 0).any()
        bb = p0.ops_b[p0.ops_b[:, OP] == E.OP_BN_BWD]
        assert not (bb[:, BB('gy2')] > 0).any() and not (bb[:, BB('producer')] > 0).any()
        assert int((p0.ops_b[:, OP] == E.OP_ADD).sum()) > int((p.ops_b[:, OP] == E.OP_ADD).sum())
    finally:
        Fn.BN_FUSE = True


_GRAD_FIELDS = {E.OP_WGRAD: ('gw',), E.OP_STEM_WGRAD: ('gw',), E.OP_PERMUTE_GENT: ('dst',), E.OP_HEAD_BWD: ('g_scale',),
                E.OP_HEAD_WFIN: ('g_cent', 'g_reg', 'g_cls', 'g_bias')}


@pytest.mark.parametrize('tail0', [False, True])
@pytest.mark.parametrize('head_overlap', [False, True])
@pytest.mark.parametrize('wgrad_async', [False, True])
@pytest.mark.parametrize('levels', [4, 2])
def test_gradient_readiness_covers_every_write(levels, wgrad_async, head_overlap, tail0):
    """`_pready` (what the data-parallel buckets leave by, NetProgram._bucket_ready) names exactly the parameters some backward
    operator writes, and no parameter counts as final before its last writer is enqueued — nor, when that writer runs on the head
    stream, before the main stream has waited for that head branch (the collectives are ordered behind the main and the
    weight-gradient stream only)."""
    p = E.NetProgram(_cached_model(levels), True, wgrad_async, head_overlap, tail0=tail0)
    b = p.ops_b
    param_at = {p._goff[id(q)]: q for q in p._params}
    ref = dict(p.grad_refs)                           # address index -> float offset into the gradient buffer
    writes = []                                       # (row, stream, parameter)
    for i, row in enumerate(b):
        op = int(row[OP])
        for f in _GRAD_FIELDS.get(op, ()):
            w, p1 = E.FIELDS[op][f]
            if int(row[w]) - p1 in ref:               # (a dense launch's weight gradient goes to a scratch tensor: OP_PERMUTE_GENT / OP_HEAD_WFIN deliver it)
                writes.append((i, int(row[STREAM]), param_at[ref[int(row[w]) - p1]]))
        if op == E.OP_SMALL_GRADS:
            first, count = (int(row[E.word(op, f)]) for f in ('first', 'count'))
            writes += [(i, int(row[STREAM]), param_at[int(o) // 4]) for o in p._small_goff[first:first + count]]
    assert {id(q) for _, _, q in writes} == set(p._pready)
    for i, _, q in writes:
        assert p._pready[id(q)] >= i + 1
    if p.head_overlap:
        ev = E.word(E.OP_WAIT, 'event')
        assert E.word(E.OP_RECORD, 'event') == ev
        # the head branches are enqueued one after the other on stream 1, each ended by the record of EV_HB + its level
        ends = [(i, int(r[ev])) for i, r in enumerate(b) if r[OP] == E.OP_RECORD and r[STREAM] == E.S_HEAD and r[ev] >= E.EV_HB]
        joins = {int(r[ev]): i for i, r in enumerate(b) if r[OP] == E.OP_WAIT and r[STREAM] == E.S_MAIN and r[ev] >= E.EV_HB}
        assert len(ends) == p.nl - 1 and {e for _, e in ends} == set(joins)
        on_head = [(i, q) for i, s, q in writes if s == E.S_HEAD]
        assert on_head
        for i, q in on_head:
            event = next(e for at, e in ends if at > i)
            assert p._pready[id(q)] >= joins[event] + 1
