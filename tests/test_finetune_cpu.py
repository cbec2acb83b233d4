"""CPU: the host side of fine-tuning — runner.param_multipliers / build_optimizer with a paramwise_cfg,
MEResNet3D(frozen_stages), runner.fit(load_from), the run table of the grouped AdamW kernel (fc_adamw_groups_pack, a pure host
function) and the kernel's own text on the host (tools/optim_host_emu.cpp under AddressSanitizer and UBSan) against a numpy
restatement; and the operator lists a training program emits for a frozen prefix (built without a GPU, as tests/test_executor_cpu.py
builds them)."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fcaf3d_amd as fa
from fcaf3d_amd import _lib as L
from fcaf3d_amd import executor as E
from fcaf3d_amd import nn as MEnn
from fcaf3d_amd import runner as R

from tests.test_fit_cpu import make_cfg

OP = E.ROW_OP


def build_model(frozen_stages=None, levels=2, n_classes=None):
    """the two-level model of tests/test_gpu_dist.py::_model, optionally with backbone.frozen_stages / another class count"""
    torch.manual_seed(0)
    cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=0.02)
    m = cfg.model
    m.backbone['n_outs'] = levels
    if frozen_stages is not None:
        m.backbone['frozen_stages'] = frozen_stages
    if n_classes is not None:
        m.neck_with_head['n_classes'] = n_classes
    m.neck_with_head['in_channels'] = (64, 128, 256, 512)[:levels]
    m.neck_with_head.assigner['n_scales'] = levels
    return fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg')), cfg


# the README's fine-tuning recipe
README_PARAMWISE = dict(custom_keys={'backbone': dict(lr_mult=0.1)}, norm_decay_mult=0.)


# ---- paramwise_cfg ----------------------------------------------------------------------------------------------------------------------
PARAMWISE = dict(custom_keys={'backbone': dict(lr_mult=.1), 'backbone.layer2': dict(lr_mult=.5), 'neck_with_head.cls_conv': dict(decay_mult=0)},
                 norm_decay_mult=0, bias_lr_mult=2)


def test_param_multipliers_follow_mmcvs_constructor():
    det, _ = build_model()
    pm = R.param_multipliers(det, PARAMWISE)
    assert set(pm) == {n for n, _ in det.named_parameters()}
    assert pm['backbone.layer1.0.conv1.kernel'] == (0.1, 1.0)
    assert pm['backbone.layer2.0.conv1.kernel'] == (0.5, 1.0)                       # the longest matching key wins
    assert pm['backbone.layer2.0.norm1.bn.weight'] == (0.5, 1.0)                    # a custom key beats the norm rule ...
    assert pm['neck_with_head.cls_conv.bias'] == (1.0, 0.0)                         # ... and the bias rule
    assert pm['neck_with_head.cls_conv.kernel'] == (1.0, 0.0)
    assert pm['neck_with_head.out_block_0.1.bn.weight'] == (1.0, 0.0)               # a BatchNorm weight outside every key: no decay
    assert pm['neck_with_head.out_block_0.1.bn.bias'] == (1.0, 0.0)                 # (a norm layer's bias is not a `bias` to the bias rules)
    assert pm['neck_with_head.out_block_0.0.kernel'] == (1.0, 1.0)
    assert pm['backbone.conv1.1.bias'] == (0.1, 1.0)                                # (under the 'backbone' key)
    # without that key the stem's instance norm is a plain module to mmcv: its `bias` takes the bias multiplier, its weight nothing
    pm2 = R.param_multipliers(det, dict(norm_decay_mult=0, bias_lr_mult=2, bias_decay_mult=3))
    assert pm2['backbone.conv1.1.bias'] == (2.0, 3.0) and pm2['backbone.conv1.1.weight'] == (1.0, 1.0)
    assert pm2['backbone.layer1.0.norm1.bn.bias'] == (1.0, 0.0) and pm2['neck_with_head.cls_conv.bias'] == (2.0, 3.0)
    # ties in length are broken alphabetically
    pm3 = R.param_multipliers(det, dict(custom_keys={'norm2': dict(lr_mult=3), 'norm1': dict(lr_mult=5), 'layer': dict(lr_mult=7)}))
    assert pm3['backbone.layer1.0.norm1.bn.weight'] == (7.0, 1.0) == pm3['backbone.layer1.0.norm2.bn.weight']      # 'layer' < 'norm1'
    assert pm3['neck_with_head.up_block_1.1.bn.weight'] == (1.0, 1.0)
    pm4 = R.param_multipliers(det, dict(custom_keys={'norm2': dict(lr_mult=3), 'norm1': dict(lr_mult=5), 'mayer': dict(lr_mult=7), '0.nor': dict(decay_mult=9)}))
    assert pm4['backbone.layer1.0.norm1.bn.weight'] == (1.0, 9.0) and pm4['backbone.layer1.0.conv1.kernel'] == (1.0, 1.0)      # '0.nor' < 'norm1'
    assert set(R.param_multipliers(det, None).values()) == {(1.0, 1.0)}
    for bad in ('dwconv_decay_mult', 'dcn_offset_lr_mult', 'bypass_duplicate'):
        with pytest.raises(KeyError, match=bad):
            R.param_multipliers(det, {bad: 1})


def test_build_optimizer_on_the_cpu_builds_mmcvs_groups():
    det, _ = build_model()
    opt = R.build_optimizer(det, dict(type='AdamW', lr=1e-3, weight_decay=1e-4, paramwise_cfg=PARAMWISE))
    assert isinstance(opt, torch.optim.AdamW)
    pm = R.param_multipliers(det, PARAMWISE)
    names = {id(p): n for n, p in det.named_parameters()}
    assert len(opt.param_groups) == len(names)
    for g in opt.param_groups:
        (p,) = g['params']
        a, b = pm[names[id(p)]]
        assert g['lr'] == 1e-3 * a and g['weight_decay'] == 1e-4 * b, names[id(p)]
    sgd = R.build_optimizer(det, dict(type='SGD', lr=0.1, momentum=0.9, paramwise_cfg=dict(custom_keys={'backbone': dict(lr_mult=0.1)})))
    assert sorted({round(g['lr'], 6) for g in sgd.param_groups}) == [0.01, 0.1]
    plain = R.build_optimizer(det, dict(type='AdamW', lr=1e-3, weight_decay=1e-4))
    assert len(plain.param_groups) == 1                                               # no paramwise_cfg: as before
    with pytest.raises(KeyError, match='dwconv_decay_mult'):
        R.build_optimizer(det, dict(type='AdamW', lr=1e-3, paramwise_cfg=dict(dwconv_decay_mult=0.)))
    # the LR hook scales every group from its own base rate
    lr = R.build_lr_updater(opt, dict(policy='step', step=[1]))
    lr.set_epoch(1)
    assert all(abs(g['lr'] - 1e-4 * pm[names[id(g['params'][0])]][0]) < 1e-12 for g in opt.param_groups)


def test_group_runs_are_maximal_stretches():
    b, a, d = R.group_runs([0, 64, 192, 256, 320], [(1, 1), (1, 1), (.1, 1), (.1, 0), (.1, 0)])
    assert (b, a, d) == ([0, 192, 256], [1.0, .1, .1], [1.0, 1.0, 0.0])


# ---- frozen_stages ------------------------------------------------------------------------------------------------------------------------
def _frozen_names(k):
    return ('backbone.conv1.',) * (k >= 0) + tuple(f'backbone.layer{i}.' for i in range(1, k + 1))


@pytest.mark.parametrize('k', [-1, 0, 1, 2])
def test_frozen_stages_freeze_a_prefix_and_keep_it_in_eval_mode(k):
    det, _ = build_model(k)
    plain, _ = build_model()
    assert list(det.state_dict()) == list(plain.state_dict())
    frozen = {n for n, p in det.named_parameters() if not p.requires_grad}
    assert frozen == {n for n, _ in det.named_parameters() if n.startswith(_frozen_names(k))} if k >= 0 else not frozen
    if k == -1:
        assert [(n, p.requires_grad) for n, p in det.named_parameters()] == [(n, p.requires_grad) for n, p in plain.named_parameters()]

    def check():
        for n, m in det.named_modules():
            if isinstance(m, MEnn.MinkowskiBatchNorm):
                assert m.training == (not n.startswith(_frozen_names(k)) if k >= 0 else True), n
                assert m.bn.training == m.training
    det.train()
    check()
    det.eval()
    assert not any(m.training for m in det.modules())
    det.train()
    check()
    assert E.frontier(det) == k


def test_frozen_stages_out_of_range_raise():
    from fcaf3d_amd.me_resnet import MEResNet3D
    for bad in (3, -2, 5):
        with pytest.raises(ValueError, match='frozen_stages'):
            MEResNet3D(3, 34, n_outs=2, frozen_stages=bad)
    assert MEResNet3D(3, 34, n_outs=4, frozen_stages=4).frozen_stages == 4


def test_frontier_refuses_what_is_no_frozen_prefix():
    det, _ = build_model(1)
    det.train()
    assert E.frontier(det) == 1
    det.backbone.layer2.eval()                         # `norm_eval` of a trainable stage: no program (the module path raises in backward)
    assert E.frontier(det) is None
    det.train()
    assert E.frontier(det) == 1
    det.neck_with_head.out_block_0[0].kernel.requires_grad = False      # a frozen neck layer
    assert E.frontier(det) is None
    det.neck_with_head.out_block_0[0].kernel.requires_grad = True
    det.backbone.layer1[0].conv1.kernel.requires_grad = True             # thawed by hand, its BatchNorm still in eval mode
    assert E.frontier(det) is None


# ---- the training program of a frozen prefix (built on the CPU) -----------------------------------------------------------------------------
def field(row, name):
    """the value of a field of an operator row (a field the header codes as index + 1 decoded: -1 = none)"""
    w, p1 = E.FIELDS[int(row[OP])][name]
    return int(row[w]) - (1 if p1 else 0)


def check_program_shape(det, p, k, plain=None):
    """what DESIGN.md section 18 says of a training program `p` of detector `det` whose backbone is frozen up to stage k"""
    f, b = p.ops_f, p.ops_b
    bb = det.backbone
    frozen_mods = [bb.conv1] * (k >= 0) + [getattr(bb, f'layer{i}') for i in range(1, k + 1)]
    frozen_bn = [m for s in frozen_mods for m in s.modules() if isinstance(m, MEnn.MinkowskiBatchNorm)]
    all_bn = [m for m in det.modules() if isinstance(m, MEnn.MinkowskiBatchNorm)]
    convs = [m for m in det.modules() if isinstance(m, MEnn.MinkowskiConvolution)]
    gents = [m for m in det.modules() if isinstance(m, MEnn.MinkowskiGenerativeConvolutionTranspose)]
    levels = min(bb.n_outs, 4)
    heads = levels - (1 if p.tail0 else 0)
    # the three 1x1 head kernels are one packed GEMM per level, the stem has its own operator (tests/test_executor_cpu.py); with the
    # finest level's tail outside the program its out_block convolution is not in it either
    trainable = [m for m in convs if m.kernel.requires_grad and m is not bb.conv1[0]]
    n_wgrad = len(trainable) - 3 - (1 if p.tail0 else 0) + len(gents) + heads
    assert int((b[:, OP] == E.OP_WGRAD).sum()) == n_wgrad
    assert int((b[:, OP] == E.OP_STEM_WGRAD).sum()) == (0 if k >= 0 else 1)
    assert int((b[:, OP] == E.OP_POOL_NORM_BWD).sum()) == (0 if k >= 0 else 1)
    n_bn_prog = len(all_bn) - (1 if p.tail0 else 0)
    assert int((b[:, OP] == E.OP_BN_BWD).sum()) == n_bn_prog - len(frozen_bn)
    # every frozen norm's forward row reads its running statistics (train = 0, nothing saved), the others train
    rows = f[f[:, OP] == E.OP_BN_FWD]
    assert len(rows) == n_bn_prog
    static = dict(p.static)
    frozen_rm = {m.bn.running_mean.data_ptr() for m in frozen_bn}
    n_frozen_rows = 0
    for r in rows:
        is_frozen = static[field(r, 'rmean')] in frozen_rm
        n_frozen_rows += is_frozen
        assert field(r, 'train') == (0 if is_frozen else 1)
        assert (field(r, 'mean') == -1) == is_frozen
    assert n_frozen_rows == len(frozen_bn)
    # no backward-data convolution writes the gradient of a frozen layer's input: one backward-data row per trainable convolution
    # launch whose input lies behind a trainable layer
    bwd_data = int((b[:, OP] == E.OP_CONV).sum())
    first_consumers = 0
    if 0 <= k < levels:
        first_consumers = 2                                     # layer(k+1).0: conv1 and the downsample convolution read the frozen prefix
    elif k == levels:
        first_consumers = 2 if levels > 1 else 1                # the coarsest level's out_block and up_block read the backbone directly
    assert bwd_data == n_wgrad - first_consumers
    # the union's gather into a backbone tensor behind the frontier is dropped
    n_gather = int((b[:, OP] == E.OP_GATHER).sum())
    assert n_gather == max(0, (levels - 1) - max(0, min(k, levels - 1)))
    # the stem's statistics for the backward pass are not kept
    stem = f[f[:, OP] == E.OP_STEM_FWD][0]
    assert (field(stem, 'col') == -1) == (k >= 0)
    pool = f[f[:, OP] == E.OP_NORM_POOL_FWD][0]
    assert (field(pool, 'mask') == -1) == (k >= 0) and (field(pool, 'parent') == -1) == (k >= 0)
    assert (field(pool, 'arg') >= 0) == (k >= 0 or p.keep_state)      # ... and the pool kernel then stores its arg-max rows
    assert (p.in_sums is None) == (k >= 0)
    # gradient readiness: an entry for every trainable parameter the program writes, none for a frozen one
    for n, q in det.named_parameters():
        outside = p.tail0 and (n.startswith('neck_with_head.out_block_0.') or n == 'neck_with_head.scales.0.scale')
        assert (id(q) in p._pready) == (q.requires_grad and not outside), n
    small = [(w, bi) for _, _, _, w, bi in p.small]
    assert all(w.requires_grad and bi.requires_grad for w, bi in small)
    assert len(small) == n_bn_prog - len(frozen_bn) + (0 if k >= 0 else 1)
    if plain is not None and k == -1:
        assert np.array_equal(f, plain.ops_f) and np.array_equal(b, plain.ops_b)


@pytest.mark.parametrize('levels,k,args', [(2, -1, (True, True)), (2, 0, (True, True)), (2, 1, (True, True)), (2, 2, (True, True)),
                                           (2, 1, (False, False)), (2, 2, (False, False)), (4, 2, (True, True)), (4, 4, (True, True)),
                                           (2, 1, (True, True, True)), (1, 1, (False, False))])
def test_training_program_stops_at_the_frontier(levels, k, args):
    det, _ = build_model(k, levels)
    det.train()
    assert E.supported(det) and E.frontier(det) == k
    p = E.NetProgram(det, True, *args, frozen=k)
    plain = None
    if k == -1:
        ref, _ = build_model(None, levels)
        plain = E.NetProgram(ref.train(), True, *args)
    check_program_shape(det, p, k, plain)
    # every wait has its record, and a head branch whose neck tensor needs no gradient is still joined by the main stream
    b = p.ops_b
    rec = set(b[b[:, OP] == E.OP_RECORD][:, E.word(E.OP_RECORD, 'event')])
    waits = b[b[:, OP] == E.OP_WAIT]
    assert set(waits[:, E.word(E.OP_WAIT, 'event')]) <= rec
    if args[1] and levels > 1:
        for lvl in range(1, levels):
            assert ((waits[:, E.word(E.OP_WAIT, 'event')] == E.EV_HB + lvl) & (waits[:, E.ROW_STREAM] == E.S_MAIN)).sum() == 1, lvl
    # fewer backward rows the deeper the frontier
    if k >= 0:
        full, _ = build_model(None, levels)
        assert len(b) < len(E.NetProgram(full.train(), True, *args).ops_b)


def test_program_cache_key_holds_the_frontier():
    """E.program_for needs no GPU to pick its key: a stale program is never handed out after freezing or train() / eval() on a stage"""
    det, _ = build_model(1)
    det.train()
    built = []
    orig = E.NetProgram

    class Spy:
        def __init__(self, det, *a, **kw):
            built.append(kw.get('frozen'))
            self._sig = E.NetProgram.signature(det)
    E.NetProgram = Spy
    Spy.signature = staticmethod(orig.signature)
    try:
        a = E.program_for(det, True)
        assert E.program_for(det, True) is a and built == [1]
        det.backbone.frozen_stages = 0
        for q in det.backbone.layer1.parameters():
            q.requires_grad = True
        det.train()
        b = E.program_for(det, True)
        assert b is not a and built == [1, 0]
        det.backbone.layer2.eval()
        assert E.program_for(det, True) is None
        det.train()
        assert E.program_for(det, True) is b
        E.program_for(det, False)
        assert built == [1, 0, -1]
    finally:
        E.NetProgram = orig


# ---- load_from ----------------------------------------------------------------------------------------------------------------------------
class _Head(torch.nn.Module):
    def __init__(self, n_classes):
        super().__init__()
        self.cls_conv = torch.nn.Linear(4, n_classes)
        self.reg = torch.nn.Parameter(torch.zeros(3))


class Net(torch.nn.Module):
    """the detector's call surface and its two halves' names; the loss depends on every weight"""

    def __init__(self, n_classes):
        super().__init__()
        self.backbone = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4))
        self.neck_with_head = _Head(n_classes)

    def forward(self, return_loss=True, points=None, gt_bboxes_3d=None, gt_labels_3d=None, img_metas=None):
        x = torch.stack([b.tensor[:, :4].mean(0) for b in gt_bboxes_3d])
        y = self.neck_with_head.cls_conv(self.backbone(x))
        return dict(loss_cls=(y ** 2).mean(), loss_reg=((self.neck_with_head.reg - 1) ** 2).sum())


def test_fit_load_from_loads_weights_only_and_reports_the_mismatch(tmp_path, capsys):
    from fcaf3d_amd import fit, load_checkpoint
    cfg = make_cfg(tmp_path / 'data', max_epochs=1, checkpoint_config=dict(interval=1, max_keep_ckpts=3))
    torch.manual_seed(1)
    src = Net(18)
    fit(src, cfg, str(tmp_path / 'pre'), seed=3, device='cpu')
    ckpt = str(tmp_path / 'pre' / 'epoch_1.pth')
    saved = load_checkpoint(Net(18), ckpt, map_location='cpu')
    assert saved['load_report'] == dict(unexpected=[], missing=[], mismatched=[])
    torch.manual_seed(2)
    tuned = Net(5)
    head0 = {k: v.clone() for k, v in tuned.neck_with_head.state_dict().items()}
    seen = []

    def on_batch(e, it, b):
        if not seen:                                   # before the first step: the backbone is the checkpoint's, the head its own
            for k, v in tuned.backbone.state_dict().items():
                assert torch.equal(v, saved['state_dict']['backbone.' + k]), k
            assert torch.equal(tuned.neck_with_head.reg, saved['state_dict']['neck_with_head.reg'])
            assert torch.equal(tuned.neck_with_head.cls_conv.weight, head0['cls_conv.weight'])
        seen.append((e, it))
    cfg2 = make_cfg(tmp_path / 'data', max_epochs=2, checkpoint_config=dict(interval=1, max_keep_ckpts=3), load_from=ckpt)
    rec = fit(tuned, cfg2, str(tmp_path / 'tune'), seed=3, device='cpu', on_batch=on_batch)      # (load_from defaults to cfg.load_from)
    assert seen[0] == (0, 0) and len(seen) == 6
    load = rec[0]
    assert load['mode'] == 'load' and load['load_from'] == ckpt and load['unexpected'] == [] and load['missing'] == []
    assert sorted(m[0] for m in load['mismatched']) == ['neck_with_head.cls_conv.bias', 'neck_with_head.cls_conv.weight']
    assert [m for m in load['mismatched'] if m[0].endswith('weight')][0][1:] == [[18, 4], [5, 4]]
    assert sum(r['mode'] == 'load' for r in rec) == 1
    first = rec[1]
    assert (first['mode'], first['epoch'], first['iter']) == ('train', 1, 2) and first['lr'] == 0.001      # epoch 1, a fresh schedule
    logs = [f for f in os.listdir(tmp_path / 'tune') if f.endswith('.log.json')]
    assert [json.loads(l) for l in open(tmp_path / 'tune' / logs[0])] == rec
    assert load_checkpoint(Net(5), str(tmp_path / 'tune' / 'epoch_1.pth'), map_location='cpu')['meta']['iter'] == 3      # counted from 0
    # a fresh optimizer: the first step of the fine-tuning run moves `reg` by one AdamW step of lr from the checkpoint's value
    # resume_from wins over load_from: the run continues at epoch 2 and nothing is loaded from `ckpt`
    again = Net(5)
    cfg2.runner['max_epochs'] = 3
    rec3 = fit(again, cfg2, str(tmp_path / 'tune'), seed=3, device='cpu', resume_from=str(tmp_path / 'tune' / 'latest.pth'), load_from=ckpt)
    assert all(r['mode'] == 'train' for r in rec3) and [(r['epoch'], r['iter']) for r in rec3] == [(3, 2), (3, 3)]
    # strict resume of the 18-class file into the 5-class model still raises
    with pytest.raises(RuntimeError, match='size mismatch'):
        fit(Net(5), cfg2, str(tmp_path / 'w3'), seed=3, device='cpu', resume_from=ckpt)
    capsys.readouterr()


# ---- the run table ------------------------------------------------------------------------------------------------------------------------
def _pack(begin, lr, dec, n, out_bytes=None, R=None):
    R = len(begin) if R is None else R
    b = np.asarray(begin, np.int64)
    a, d = np.asarray(lr, np.float32), np.asarray(dec, np.float32)
    out = np.zeros(max(12 * max(R, 1), 1), np.uint8)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = L.lib().fc_adamw_groups_pack(vp(b), vp(a), vp(d), R, n, vp(out), out.nbytes if out_bytes is None else out_bytes)
    return rc, out[:12 * R]


def test_run_table_pack_validates_and_round_trips():
    cap = 1024
    assert 'FC_ADAMW_MAX_RUNS 1024' in open(L.HEADER).read() and R.MAX_RUNS == cap
    one = [1.0]
    ok = lambda *a, **k: _pack(*a, **k)[0]
    assert ok([0], one, one, 64) == 0
    assert ok([64], one, one, 256) == -1                                           # the first offset is not 0
    assert ok([0, 128, 128], one * 3, one * 3, 256) == -1                          # not strictly ascending
    assert ok([0, 128, 64], one * 3, one * 3, 256) == -1
    assert ok([0, 96], one * 2, one * 2, 256) == -1                                # no multiple of 64 floats
    assert ok([0, 256], one * 2, one * 2, 256) == -1 and ok([0, 192], one * 2, one * 2, 256) == 0      # an offset >= n
    assert ok([0], one, one, 0) == -1
    assert ok([], [], [], 256, R=0) == -1 and ok([0], one, one, 256, R=-1) == -1   # R < 1
    many = list(range(0, 64 * (cap + 1), 64))
    assert ok(many, one * (cap + 1), one * (cap + 1), 64 * (cap + 2)) == -1 and ok(many[:cap], one * cap, one * cap, 64 * cap) == 0      # the cap
    for bad in (-0.5, float('nan'), float('inf'), -float('inf')):
        assert ok([0, 64], [1.0, bad], one * 2, 256) == -1 and ok([0, 64], one * 2, [bad, 1.0], 256) == -1
    assert ok([0], one, one, 66) == -1                                             # n % 4
    assert ok([0, 64], one * 2, one * 2, 256, out_bytes=23) == -2                  # the table does not fit
    assert L.lib().fc_adamw_groups_table_bytes(3) == 36 and L.lib().fc_adamw_groups_table_bytes(0) == 0 == L.lib().fc_adamw_groups_table_bytes(cap + 1)
    rc, out = _pack([0, 192, 6400], [1.0, 0.0, 0.25], [1.0, 0.5, 0.0], 6464)
    assert rc == 0
    words = out.view(np.uint32)
    assert list(words[:3]) == [0, 3, 100]
    assert list(words[3:6].view(np.float32)) == [1.0, 0.0, 0.25] and list(words[6:9].view(np.float32)) == [1.0, 0.5, 0.0]
    assert np.array_equal(R.pack_runs([0, 192, 6400], [1.0, 0.0, 0.25], [1.0, 0.5, 0.0], 6464), out)
    with pytest.raises(ValueError):
        R.pack_runs([0, 96], one * 2, one * 2, 256)


# ---- the kernel's text on the host ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def emulator(tmp_path_factory):
    """csrc_post/optim_groups.hip from its ADAMW_* constants to the end of its anonymous namespace, compiled for the host with
    AddressSanitizer and UBSan: the emulator restates nothing of the kernel"""
    from fcaf3d_amd import build as B
    tmp = tmp_path_factory.mktemp('optim_emu')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(B.CSRC_POST, 'optim_groups.hip')).read()
    end = '}  // namespace'
    body = src[src.index('#define ADAMW_THREADS'):src.index(end) + len(end)]
    assert '#include' not in body and '#define ADAMW_MAX_RUNS 1024' in body and 'k_adamw_groups' in body, 'optim_groups.hip was reordered'
    (tmp / 'kernels.inc').write_text(body)
    cxx = os.path.join(os.path.dirname(os.path.dirname(B.HIPCC)), 'llvm', 'bin', 'clang++')
    cxx = cxx if os.path.exists(cxx) else shutil.which('clang++')
    exe = str(tmp / 'optim_host_emu')
    subprocess.check_call([cxx, '-std=c++20', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-pthread', f'-I{tmp}', os.path.join(root, 'tools', 'optim_host_emu.cpp'), '-o', exe])
    return exe, tmp


HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=3)


def adamw_groups_numpy(p, g, m, v, begin, lr_mult, dec_mult, clip=None, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=3):
    """k_adamw_groups in numpy: fp32 throughout, the kernel's operations in the kernel's order (no fused multiply-add)"""
    f = np.float32
    n = len(p)
    bc1, bc2s = f(1.0 - b1 ** step), np.sqrt(f(1.0 - b2 ** step))
    run = np.searchsorted(np.asarray(begin, np.int64), np.arange(n), side='right') - 1
    lr_r = f(lr) * np.asarray(lr_mult, f)[run]
    wd_r = f(wd) * np.asarray(dec_mult, f)[run]
    decay = f(1) - lr_r * wd_r
    step_size = lr_r / bc1
    gg = g * (f(clip[1]) if clip is not None else f(1))
    pp = p * decay
    mm = m + (gg - m) * (f(1) - f(b1))
    v2 = v * f(b2) + (f(1) - f(b2)) * gg * gg
    denom = np.sqrt(v2) / bc2s + f(eps)
    pp = pp - step_size * (mm / denom)
    assert pp.dtype == mm.dtype == v2.dtype == np.float32
    return pp, mm, v2


def _emulate(emulator, p, g, m, v, begin, lr_mult, dec_mult, clip=None, table=None, **hyper):
    exe, tmp = emulator
    h = dict(HYPER, **hyper)
    n, R_ = len(p), len(begin)
    if table is None:
        rc, table = _pack(begin, lr_mult, dec_mult, n)
        assert rc == 0
    with open(tmp / 'in.bin', 'wb') as f:
        np.array([n, R_, 0 if clip is None else 1, 0], np.int64).tofile(f)
        c = (0.0, 1.0) if clip is None else clip
        np.array([h['lr'], h['b1'], h['b2'], h['eps'], h['wd'], 1.0 - h['b1'] ** h['step'], 1.0 - h['b2'] ** h['step'], c[0], c[1], 0], np.float32).tofile(f)
        table.tofile(f)
        for a in (p, g, m, v):
            a.astype(np.float32).tofile(f)
    r = subprocess.run([exe, str(tmp / 'in.bin'), str(tmp / 'out.bin')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = np.fromfile(tmp / 'out.bin', np.float32)
    assert len(out) == 3 * n
    return out[:n], out[n:2 * n], out[2 * n:]


def _state(n, seed):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 0.1).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 * 0.01).astype(np.float32)
    return p, g, m, v


def _mults(R_, seed):
    rng = np.random.default_rng(seed)
    a = rng.choice(np.array([0.0, 0.1, 0.5, 1.0, 2.0], np.float32), R_)
    d = rng.choice(np.array([0.0, 1.0, 3.0], np.float32), R_)
    a[1:] = np.where((a[1:] == a[:-1]) & (d[1:] == d[:-1]), a[1:] + 1, a[1:])      # neighbours differ: maximal runs
    return a, d


EMU_CASES = {
    'one run': (4096, [0]),
    'runs of exactly one slice': (64 * 40, list(range(0, 64 * 40, 64))),
    # a boundary at vector index 255 cannot be (a run starts on a 16-vector slice): the slices around the edge of the first workgroup
    # (vectors 240, 256, 272), and an edge inside the second
    'boundaries around a workgroup edge': (4 * 256 * 3, [0, 4 * 240, 4 * 256, 4 * 272, 4 * 400]),
    'last workgroup partially filled': (4 * (256 * 2 + 16), [0, 4 * 496, 4 * 512]),
    'one vector short of a workgroup': (4 * 255 + 60, [0, 64]),
}


@pytest.mark.parametrize('case', list(EMU_CASES))
@pytest.mark.parametrize('clip', [None, (12.5, 0.8)])
def test_kernel_text_on_the_host_equals_numpy(emulator, case, clip):
    n, begin = EMU_CASES[case]
    p, g, m, v = _state(n, 5)
    a, d = _mults(len(begin), 6)
    got = _emulate(emulator, p, g, m, v, begin, a, d, clip)
    want = adamw_groups_numpy(p, g, m, v, begin, a, d, clip)
    for x, y, name in zip(got, want, 'pmv'):
        assert np.array_equal(x, y), (case, name, int((x != y).sum()))
    assert not np.array_equal(got[1], m) and not np.array_equal(got[2], v)


def test_kernel_text_on_the_host_edge_sizes(emulator):
    # the boundaries the flat layout cannot produce but the table format can hold are the kernel's to survive: vector 255 / 257
    # lie INSIDE slices 15 / 16, so a run starting at slice 15 or 16 puts its edge inside and at the end of the first workgroup
    n = 4 * 600
    p, g, m, v = _state(n, 7)
    for begin in ([0, 64 * 15], [0, 64 * 16], [0, 64 * 15, 64 * 16, 64 * 17]):
        a, d = _mults(len(begin), 8)
        got = _emulate(emulator, p, g, m, v, begin, a, d, (3.0, 0.25))
        want = adamw_groups_numpy(p, g, m, v, begin, a, d, (3.0, 0.25))
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), begin
    # n = 0: nothing is launched, nothing is read (the table is one packed for another n)
    z = np.zeros(0, np.float32)
    _, tab = _pack([0], [1.0], [1.0], 64)
    assert all(len(x) == 0 for x in _emulate(emulator, z, z, z, z, [0], [1.0], [1.0], table=tab))
    # lr_mult = 0: p keeps its bits (p * 1 - 0 * finite), m and v advance — also with weight decay on that run
    n = 64 * 6
    p, g, m, v = _state(n, 9)
    begin, a, d = [0, 128, 256], [1.0, 0.0, 0.5], [1.0, 1.0, 0.0]
    got = _emulate(emulator, p, g, m, v, begin, a, d, (20.0, 0.5))
    assert np.array_equal(got[0][128:256].view(np.uint32), p[128:256].view(np.uint32))
    assert not (got[1][128:256] == m[128:256]).any() and not (got[2][128:256] == v[128:256]).any()
    assert not (got[0][:128] == p[:128]).all() and not (got[0][256:] == p[256:]).all()
    assert all(np.array_equal(x, y) for x, y in zip(got, adamw_groups_numpy(p, g, m, v, begin, a, d, (20.0, 0.5))))
    # padding floats (p = g = m = v = 0) stay zero whatever the run's rates
    p[60:64] = g[60:64] = m[60:64] = v[60:64] = 0
    got = _emulate(emulator, p, g, m, v, begin, a, d)
    assert all((x[60:64] == 0).all() for x in got)


def test_kernel_text_on_the_host_at_the_run_cap(emulator):
    cap = R.MAX_RUNS
    n = 64 * cap + 64 * 3 + 8                            # every run one slice but the last; a partially filled last workgroup
    begin = list(range(0, 64 * cap, 64))
    p, g, m, v = _state(n, 10)
    a, d = _mults(cap, 11)
    got = _emulate(emulator, p, g, m, v, begin, a, d, (11.0, 0.9))
    want = adamw_groups_numpy(p, g, m, v, begin, a, d, (11.0, 0.9))
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
