"""CPU: training on running statistics and with a frozen neck — the constructors' flags
(MEResNet3D(norm_eval), Fcaf3DNeckWithHead(norm_eval, frozen_neck)), executor.freeze_plan, the operator lists a training program emits
for every declared combination (built without a GPU, as tests/test_finetune_cpu.py builds them), the default programs against the
hashes of the commit before this feature, and the routes of fc_bn_eval_bwd (pure host functions of the C ABI)."""
import hashlib

import numpy as np
import pytest
import torch

import fcaf3d_amd as fa
from fcaf3d_amd import _lib as L
from fcaf3d_amd import executor as E
from fcaf3d_amd import nn as MEnn

from tests.test_finetune_cpu import field

OP = E.ROW_OP


def build(levels=2, frozen_stages=None, bb_norm_eval=None, neck_norm_eval=None, frozen_neck=None):
    """the two-level model of tests/test_finetune_cpu.py::build_model, with the declarations under test in its config dicts"""
    torch.manual_seed(0)
    cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=0.02)
    m = cfg.model
    m.backbone['n_outs'] = levels
    m.neck_with_head['in_channels'] = (64, 128, 256, 512)[:levels]
    m.neck_with_head.assigner['n_scales'] = levels
    if frozen_stages is not None:
        m.backbone.update(frozen_stages=frozen_stages)
    if bb_norm_eval is not None:
        m.backbone.update(norm_eval=bb_norm_eval)
    if neck_norm_eval is not None:
        m.neck_with_head.update(norm_eval=neck_norm_eval)
    if frozen_neck is not None:
        m.neck_with_head.update(frozen_neck=frozen_neck)
    return fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg')), cfg


# the declared combinations: (levels, frozen_stages, norm_eval backbone, norm_eval neck, frozen_neck)
COMBOS = {
    'norm_eval-backbone': (2, -1, True, False, False),
    'norm_eval-both': (2, -1, True, True, False),
    'frozen1-norm_eval': (2, 1, True, False, False),
    'frozen_neck': (2, -1, False, False, True),
    'frozen_neck-frozen2of4': (4, 2, False, False, True),
    'head-only': (2, 2, False, False, True),
    'head-only-norm_eval': (2, 2, True, True, True),
}


def build_combo(name):
    lv, k, ne_b, ne_n, fn = COMBOS[name]
    return build(lv, k, ne_b, ne_n, fn)[0]


def _is_neck(name):
    return name.startswith(('neck_with_head.up_block_', 'neck_with_head.out_block_'))


# ---- flags ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(COMBOS))
def test_declarations_keep_the_state_dict_and_survive_train_eval_train(name):
    lv, k, ne_b, ne_n, fn = COMBOS[name]
    det, plain = build_combo(name), build(lv)[0]
    assert list(det.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in det.named_parameters()] == [n for n, _ in plain.named_parameters()]
    frozen_bb = ('backbone.conv1.',) * (k >= 0) + tuple(f'backbone.layer{i}.' for i in range(1, k + 1))

    def check():
        for n, q in det.named_parameters():
            assert q.requires_grad == (not (n.startswith(frozen_bb) or (fn and _is_neck(n)))), n
        for n, m in det.named_modules():
            if isinstance(m, MEnn.MinkowskiBatchNorm):
                ev = (ne_b or n.startswith(frozen_bb)) if n.startswith('backbone.') else (ne_n or fn)
                assert m.training == (not ev) and m.bn.training == m.training, n
            elif isinstance(m, (MEnn.MinkowskiConvolution, MEnn.MinkowskiGenerativeConvolutionTranspose)):
                # a convolution stays in training mode unless its whole block is frozen (mmdet's norm_eval touches the norms alone)
                assert m.training == (not (n.startswith(frozen_bb) or (fn and _is_neck(n)))), n
    det.train()
    check()
    det.eval()
    assert not any(m.training for m in det.modules())
    det.train()
    check()
    nh = det.neck_with_head
    for q in (nh.centerness_conv.kernel, nh.reg_conv.kernel, nh.cls_conv.kernel, nh.cls_conv.bias, *(s.scale for s in nh.scales)):
        assert q.requires_grad


def test_bad_values_raise():
    from fcaf3d_amd.fcaf3d_neck_with_head import Fcaf3DNeckWithHead
    from fcaf3d_amd.me_resnet import MEResNet3D
    for bad in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match='norm_eval'):
            MEResNet3D(3, 34, n_outs=2, norm_eval=bad)
        with pytest.raises(ValueError, match='norm_eval'):
            build(neck_norm_eval=bad if bad is not None else 2)
        with pytest.raises(ValueError, match='frozen_neck'):
            build(frozen_neck=bad if bad is not None else 2)
    assert MEResNet3D(3, 34, n_outs=2, norm_eval=True).norm_eval is True


# ---- freeze_plan ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [-1, 0, 1, 2])
def test_freeze_plan_is_the_frontier_where_there_is_one(k):
    det = build(2, k)[0].train()
    assert E.frontier(det) == k and E.freeze_plan(det) == k and isinstance(E.freeze_plan(det), int)


@pytest.mark.parametrize('name', list(COMBOS))
def test_freeze_plan_of_a_declared_combination(name):
    det = build_combo(name).train()
    assert E.frontier(det) is None
    plan = E.freeze_plan(det)
    assert plan is not None and hash(plan) is not None and E.freeze_plan(det) is plan          # cached per pair of tuples
    rg, tm = plan
    assert rg == tuple(q.requires_grad for g in det._frontier_lists[0] for q in g)
    assert tm == tuple(m.training for g in det._frontier_lists[1] for m in g)
    det.eval()
    det.train()
    assert E.freeze_plan(det) == plan


def test_freeze_plan_refuses_what_no_declaration_implies():
    det = build(2, 1)[0].train()
    det.backbone.layer2.eval()                                           # a lone layer2.eval()
    assert E.freeze_plan(det) is None and E.program_for(det, True) is None
    det.train()
    assert E.freeze_plan(det) == 1
    det.neck_with_head.out_block_0[0].kernel.requires_grad = False       # one neck kernel frozen by hand
    assert E.freeze_plan(det) is None
    det.neck_with_head.out_block_0[0].kernel.requires_grad = True
    det = build_combo('norm_eval-backbone').train()
    assert E.freeze_plan(det) is not None
    det.backbone.layer1[0].norm1.train()                                 # one norm back in training mode under norm_eval
    assert E.freeze_plan(det) is None
    det.train()
    det.neck_with_head.reg_conv.kernel.requires_grad = False             # a head kernel (the packed head GEMM): out of scope
    assert E.freeze_plan(det) is None
    det.neck_with_head.reg_conv.kernel.requires_grad = True
    det.neck_with_head.scales[0].scale.requires_grad = False
    assert E.freeze_plan(det) is None
    det.neck_with_head.scales[0].scale.requires_grad = True
    det.backbone.layer1[0].norm1.bn.weight.requires_grad = False         # gamma without beta
    assert E.freeze_plan(det) is None
    det.backbone.layer1[0].norm1.bn.weight.requires_grad = True
    det.backbone.conv1[1].weight.requires_grad = False                   # a stem whose convolution and norm differ
    assert E.freeze_plan(det) is None
    det.backbone.conv1[1].weight.requires_grad = True
    assert E.freeze_plan(det) is not None
    # a declaration changed by hand is a declaration: the flags follow it at the next train()
    det.neck_with_head.frozen_neck = True
    assert E.freeze_plan(det) is None
    det.train()
    assert E.freeze_plan(det) is not None


def test_program_cache_key_holds_the_plan():
    det = build_combo('norm_eval-backbone').train()
    built = []
    orig = E.NetProgram

    class Spy:
        def __init__(self, det, *a, **kw):
            built.append((kw.get('frozen'), kw.get('plan')))
            self._sig = E.NetProgram.signature(det)
    E.NetProgram = Spy
    Spy.signature = staticmethod(orig.signature)
    try:
        a = E.program_for(det, True)
        plan = E.freeze_plan(det)
        assert E.program_for(det, True) is a and built == [(-1, plan)]
        t0 = E.program_for(det, True, tail0=True)
        assert t0 is not a and built[-1] == (-1, plan)                   # a pruned-tail program takes the plan as it takes the frontier
        det.backbone.norm_eval = False
        det.train()
        b = E.program_for(det, True)
        assert b is not a and built[-1] == (-1, None)
        det.backbone.norm_eval = True
        det.train()
        assert E.program_for(det, True) is a
    finally:
        E.NetProgram = orig


# ---- the training programs of the declared combinations (built on the CPU) ------------------------------------------------------------------------
def check_plan_program(det, p):
    """what DESIGN.md section 19 says of a training program `p` of detector `det` whose flags follow its declarations"""
    f, b = p.ops_f, p.ops_b
    bb, nh = det.backbone, det.neck_with_head
    levels = min(bb.n_outs, 4)
    k = bb.frozen_stages
    heads = levels - (1 if p.tail0 else 0)
    outside = ('neck_with_head.out_block_0.',) if p.tail0 else ()
    static = dict(p.static)
    bns = {n: m for n, m in det.named_modules() if isinstance(m, MEnn.MinkowskiBatchNorm) and not n.startswith(outside)}
    frozen_bb = ('backbone.conv1.',) * (k >= 0) + tuple(f'backbone.layer{i}.' for i in range(1, k + 1))
    backbone_trains = k < levels
    # a layer is on the gradient path iff it has something to train or a trainable layer lies upstream: every neck layer is
    # downstream of the coarsest backbone level, a backbone layer of a frozen stage of nothing trainable
    def on_path(n, trains):
        return trains or (n.startswith('neck_with_head.') and backbone_trains)
    eval_path = {n: m for n, m in bns.items() if not m.training and on_path(n, m.bn.weight.requires_grad)}
    train_bn = {n: m for n, m in bns.items() if m.training}
    assert all(m.bn.weight.requires_grad for m in train_bn.values())
    rows = b[b[:, OP] == E.OP_BN_EVAL_BWD]
    assert len(rows) == len(eval_path) and int((b[:, OP] == E.OP_BN_BWD).sum()) == len(train_bn)
    by_rmean = {m.bn.running_mean.data_ptr(): (n, m) for n, m in bns.items()}
    seen, eval_x = set(), set()
    for r in rows:
        n, m = by_rmean[static[field(r, 'rmean')]]
        assert n in eval_path and n not in seen, n
        seen.add(n)
        assert static[field(r, 'rvar')] == m.bn.running_var.data_ptr() and static[field(r, 'gamma')] == m.bn.weight.data_ptr()
        assert (field(r, 'sums') == -1) == (not m.bn.weight.requires_grad), n         # sums exactly where gamma / beta train
        assert (field(r, 'y') == -1) == (field(r, 'gres') == -1)
        eval_x.add(field(r, 'x'))
    # no backward-data convolution carries the reductions of an eval-mode layer, and no eval-mode layer patched its producer in the forward list
    convs_b = b[b[:, OP] == E.OP_CONV]
    assert not any(field(r, 'bn_x') in eval_x for r in convs_b)
    assert int(sum(field(r, 'bn_x') >= 0 for r in convs_b)) == int(sum(field(r, 'producer') >= 0 for r in b[b[:, OP] == E.OP_BN_BWD]))
    n_patched = 0
    for r in f[f[:, OP] == E.OP_BN_FWD]:
        n, m = by_rmean[static[field(r, 'rmean')]]
        assert field(r, 'train') == (1 if m.training else 0), n
        assert (field(r, 'mean') == -1) == (not m.training) and (m.training or field(r, 'producer') == -1), n
        n_patched += field(r, 'producer') >= 0
    assert int(sum(field(r, 'stats') >= 0 for r in f[f[:, OP] == E.OP_CONV])) == n_patched
    # weight gradients only for trainable kernels; one launch per convolution on the path, backward-data unless nobody upstream needs its input
    convs = {n: m for n, m in det.named_modules() if isinstance(m, (MEnn.MinkowskiConvolution, MEnn.MinkowskiGenerativeConvolutionTranspose))
             and m is not bb.conv1[0] and m not in (nh.centerness_conv, nh.reg_conv, nh.cls_conv) and not n.startswith(outside)}
    n_wgrad = sum(m.kernel.requires_grad for m in convs.values()) + heads
    assert int((b[:, OP] == E.OP_WGRAD).sum()) == n_wgrad
    assert int((b[:, OP] == E.OP_PERMUTE_GENT).sum()) == sum(m.kernel.requires_grad for m in convs.values()
                                                            if isinstance(m, MEnn.MinkowskiGenerativeConvolutionTranspose))
    n_path = sum(on_path(n, m.kernel.requires_grad) for n, m in convs.items()) + heads
    if 0 <= k < levels:
        first = 2                                       # layer(k+1).0: conv1 and the downsample convolution read the frozen prefix
    elif k == levels:
        neck_trains = any(q.requires_grad for n, q in det.named_parameters() if _is_neck(n))
        first = (2 if levels > 1 else 1) if neck_trains else heads      # the coarsest level's blocks | every level's head GEMM
    else:
        first = 0
    assert len(convs_b) == n_path - first
    assert int((b[:, OP] == E.OP_STEM_WGRAD).sum()) == int((b[:, OP] == E.OP_POOL_NORM_BWD).sum()) == (0 if k >= 0 else 1)
    assert int((b[:, OP] == E.OP_GATHER).sum()) == (max(0, (levels - 1) - max(0, min(k, levels - 1))) if backbone_trains else 0)
    # every wait has its record
    for ops in (f, b):
        rec = set(ops[ops[:, OP] == E.OP_RECORD][:, E.word(E.OP_RECORD, 'event')])
        assert set(ops[ops[:, OP] == E.OP_WAIT][:, E.word(E.OP_WAIT, 'event')]) <= rec
    # gradient readiness: exactly the trainable parameters the program writes
    for n, q in det.named_parameters():
        out = p.tail0 and (n.startswith('neck_with_head.out_block_0.') or n == 'neck_with_head.scales.0.scale')
        assert (id(q) in p._pready) == (q.requires_grad and not out), n
    small = [(w, bi) for _, _, _, w, bi in p.small]
    assert all(w.requires_grad and bi.requires_grad for w, bi in small)
    n_affine = sum(m.bn.weight.requires_grad for m in bns.values())
    assert len(small) == n_affine + (0 if k >= 0 else 1)
    covered = int(sum(field(r, 'count') for r in b[b[:, OP] == E.OP_SMALL_GRADS]))
    assert covered == 2 * len(small)


STREAMS = [(True, True), (False, False)]


@pytest.mark.parametrize('args', STREAMS + [(True, True, True)], ids=['overlap', 'serial', 'tail0'])
@pytest.mark.parametrize('name', list(COMBOS))
def test_training_program_of_a_declared_combination(name, args):
    det = build_combo(name).train()
    assert E.supported(det)
    plan = E.freeze_plan(det)
    p = E.NetProgram(det, True, *args, frozen=det.backbone.frozen_stages, plan=plan)
    assert p.plan == plan and p.frozen == det.backbone.frozen_stages
    check_plan_program(det, p)
    full = E.NetProgram(build(COMBOS[name][0])[0].train(), True, *args)
    if COMBOS[name][4] or COMBOS[name][1] >= 0:
        assert len(p.ops_b) < len(full.ops_b)
    else:
        # norm_eval alone: the same launches but one backward operator per layer, none of them patched into a producer
        assert len(p.ops_f) == len(full.ops_f)


def test_head_only_program():
    det = build_combo('head-only').train()
    p = E.NetProgram(det, True, True, True, frozen=2, plan=E.freeze_plan(det))
    b = p.ops_b
    ops = set(b[:, OP].tolist())
    assert E.OP_BN_BWD not in ops and E.OP_BN_EVAL_BWD not in ops and E.OP_CONV not in ops and E.OP_GATHER not in ops
    assert E.OP_PERMUTE_GENT not in ops and E.OP_SMALL_GRADS not in ops
    wg = b[b[:, OP] == E.OP_WGRAD]
    assert len(wg) == 2 and all(field(r, 'map') == -1 and field(r, 'cout') == 64 for r in wg)      # the packed head GEMM of each level
    assert int((b[:, OP] == E.OP_HEAD_BWD).sum()) == 2 and int((b[:, OP] == E.OP_HEAD_WFIN).sum()) == 1
    nh = det.neck_with_head
    want = {id(q) for q in (nh.centerness_conv.kernel, nh.reg_conv.kernel, nh.cls_conv.kernel, nh.cls_conv.bias, *(s.scale for s in nh.scales))}
    assert set(p._pready) == want == {id(q) for q in det.parameters() if q.requires_grad}
    # the forward list is an inference program's but for the head
    assert (p.ops_f[p.ops_f[:, OP] == E.OP_BN_FWD][:, E.word(E.OP_BN_FWD, 'train')] == 0).all()


def test_trainable_only_parameter_sets_with_an_empty_backbone_and_neck():
    """FlatParams / build_optimizer / param_multipliers over a head-only model: only the head's parameters are packed and stepped"""
    from fcaf3d_amd import runner as R
    det, cfg = build(2, 2, False, False, True)
    det.train()
    trainable = [n for n, q in det.named_parameters() if q.requires_grad]
    assert trainable and all(n.startswith(('neck_with_head.centerness_conv', 'neck_with_head.reg_conv', 'neck_with_head.cls_conv',
                                           'neck_with_head.scales')) for n in trainable)
    opt = R.build_optimizer(det, dict(cfg.optimizer))
    assert sum(len(g['params']) for g in opt.param_groups) == len(trainable)


# ---- default programs: row for row those of the commit before this feature ---------------------------------------------------------------------------
def program_hash(p):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(p.ops_f).tobytes())
    h.update(np.ascontiguousarray(p.ops_b).tobytes())
    return h.hexdigest()[:16]


# sha256[:16] over ops_f / ops_b of the two-level default model's programs, computed on the parent commit with this very function
# (model built by `build()` above under torch.manual_seed(0); the rows hold table indices and immediates, no addresses)
PARENT_HASHES = {
    'train-11-tail0': '7859dd867d442017',
    'train-11-tail1': '52540dbbe7aaa2e5',
    'train-00-tail0': '74fd2ce8b83c0471',
    'train-00-tail1': '7cdc5d802cdc40f9',
    'infer-1-tail0': 'b340a0df7d8eabcf',
    'infer-1-tail1': '070627f954c2eedf',
    'infer-0-tail0': 'c9cf21784b2e84e0',
    'infer-0-tail1': 'c19278034c30f921',
}


def default_programs():
    det = build(2)[0]
    det.train()
    for args in ((True, True), (False, False)):
        for tail0 in (False, True):
            yield f'train-{int(args[0])}{int(args[1])}-tail{int(tail0)}', E.NetProgram(det, True, *args, tail0)
    det.eval()
    for overlap in (True, False):
        for tail0 in (False, True):
            yield f'infer-{int(overlap)}-tail{int(tail0)}', E.NetProgram(det, False, False, overlap, tail0)


def test_default_programs_are_the_parents_row_for_row():
    got = {k: program_hash(p) for k, p in default_programs()}
    assert got == PARENT_HASHES


# ---- routes of fc_bn_eval_bwd (host functions: no GPU) ---------------------------------------------------------------------------------------
SHAPES = [(0, 64), (1, 4), (63, 4), (64, 64), (65, 64), (257, 12), (1000, 128), (333, 512), (130, 1024), (65537, 4)]


@pytest.mark.parametrize('n,C', SHAPES, ids=[f'{n}x{C}' for n, C in SHAPES])
def test_eval_bwd_route(n, C):
    H = L.header_enums()
    rc, r = L.route('fc_bn_eval_bwd_route', n, C, 0)
    assert rc == 0 and r['sums'] == H['FC_NRED_NONE'] and r['ws_bytes'] == 0 == L.query('fc_bn_eval_bwd_ws_bytes', n, C, 0)
    if n == 0:
        assert r['launches'] == 0 and r['apply'] == H['FC_NBAPPLY_NONE']
    else:
        assert r['launches'] == 1 and r['apply'] == H['FC_NBAPPLY_ROWS'] and r['threads'] == 256 and r['lds'] == 0
        assert r['grid_x'] == -(-n * (C // 4) // 256) and r['grid_y'] == 1           # a thread per four channels of a row
    rc, r = L.route('fc_bn_eval_bwd_route', n, C, 1)
    assert rc == 0 and r['sums'] == H['FC_NRED_PARTIAL'] and r['ws_bytes'] == L.query('fc_bn_eval_bwd_ws_bytes', n, C, 1)
    if n == 0:
        assert r['launches'] == 0 and r['ws_bytes'] == 0
        return
    nb = min(-(-n // 64), 1024)
    rpb = -(-n // nb)
    # few row blocks of many channels: a block owns a window of 64 channels and grid.y walks the windows (csrc/norm_route.h ap_window)
    g64 = -(-n // 64)
    cg = 64 if (C >= 128 and C % 64 == 0 and g64 * (C // 64) <= 1024 and g64 < 128) else C
    c4n = cg // 4
    nrl = max(1, min(16, 256 // c4n))
    assert r['launches'] == 2 and r['cg'] == cg and r['threads'] == nrl * c4n and r['lds'] == nrl * 2 * cg * 4
    assert r['rpb'] == rpb and r['nb'] == r['np'] == r['grid_x'] == -(-n // rpb) and r['grid_y'] == C // cg
    assert (r['nb'] - 1) * rpb < n <= r['nb'] * rpb                                  # no empty block, every row covered
    assert r['ws_bytes'] == r['nb'] * 2 * C * 4 and r['amax'] == H['FC_NAMAX_FOLDED']
    if (n, C) == (257, 12):
        assert r['threads'] == 48
    if (n, C) in ((1000, 128), (333, 512), (130, 1024)):
        assert r['cg'] == 64 and r['threads'] == 256
    if (n, C) == (65537, 4):
        assert r['rpb'] > 64 and r['nb'] <= 1024


def test_eval_bwd_route_refusals():
    for n, C in ((64, 0), (64, 2), (64, 6), (64, 1028), (64, 2048), (-1, 64)):
        for ws in (0, 1):
            rc, r = L.route('fc_bn_eval_bwd_route', n, C, ws)
            assert rc == -1 and r['sums'] == 0 and r['launches'] == 0, (n, C, ws)
            assert L.query('fc_bn_eval_bwd_ws_bytes', n, C, ws) == 0
    assert L.route('fc_bn_eval_bwd_route', 64, 1024, 1)[0] == 0
