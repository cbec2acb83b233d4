"""-m gpu: the stem's tail with a per-child arg-max mask between the directions (csrc/pool_rows.h k_norm_act_maxpool8_fwd<true>,
csrc/norm_rows.h POOL_MASK) against the arg-max-row forms it stands beside, through the C ABI on identical inputs.

A. fc_norm_act_maxpool8_mask_fwd: out, parent, y and the amax word torch.equal to fc_norm_act_maxpool8_fwd's; mask[r] bit c set exactly
   where argrow[parent[r]][c] == r, argrow taken from fc_norm_act_maxpool8_fwd; argrow stored when a pointer is passed, untouched when not.
B. fc_maxpool8_mask_norm_act_bwd: gx and the two sums torch.equal to fc_maxpool8_norm_act_bwd's on random floats (the same launches and
   summation order; only the loads differ).
C. C != 64 answers FC_EINVAL from both.
D. one executor step of a training program (mask, no arg-max rows) against one built under KEEP_STATE (both): every parameter
   gradient torch.equal.
Pooled rows in {1, 5, 3001} at 2 and 8 scenes: absent children, a pooled row with one child, a pooled row without children, all-negative
rows (ties at 0 behind the ReLU: the first child in offset order wins), a partial last block."""
import numpy as np
import pytest
import torch

import fcaf3d_amd as fa
from fcaf3d_amd import _lib as L
from fcaf3d_amd import executor as E
from fcaf3d_amd.synthetic import make_scene
from tests import pool_cases as PC

pytestmark = pytest.mark.gpu
C = 64
EPS = 1e-5
RELU = 1
SHAPES = [(nseg, n_out) for n_out in (1, 5, 3001) for nseg in (2, 8)]


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _amax_word(slot):
    return int(slot.view(32, 16)[:, 0].max())


@pytest.fixture(scope='module', params=SHAPES, ids=[f'scenes{s}-pooled{n}' for s, n in SHAPES])
def case(request):
    """the inputs of one shape and what the arg-max-row entry points make of them (computed once, read by A and B)"""
    nseg, n_out = request.param
    dev = _dev()
    single = nseg if n_out > nseg + 1 else None
    t = PC.pool_table(n_out, nseg, 100 + nseg + n_out, single_child_row=single)
    n_in = t['n_in']
    assert (n_out * (C // 4)) % 256 != 0, 'the last block must be partial'
    rng = np.random.default_rng(7 + n_out)
    scale, shift = 0.5 + np.arange(nseg), np.linspace(-1.0, 2.0, nseg)
    x = rng.standard_normal((n_in, C)) * scale[t['seg_in']][:, None] + shift[t['seg_in']][:, None]
    low = np.zeros(n_out, dtype=bool)
    low[rng.permutation(n_out)[:max(1, n_out // 10)]] = True          # pooled rows all of whose children are negative before the ReLU
    low &= t['kcount'] > 0
    if not low.any():
        low[0] = True
    x[low[t['parent']]] = -100.0 - rng.random((int(low[t['parent']].sum()), C))
    seg_in = np.zeros((n_in, 4), dtype=np.int32)
    seg_in[:, 0] = t['seg_in']
    d = dict(x=torch.from_numpy(x.astype(np.float32)), nbr=torch.from_numpy(t['nbr']), seg_in=torch.from_numpy(seg_in),
             gamma=torch.from_numpy((0.5 + rng.random(C)).astype(np.float32)), beta=torch.from_numpy((0.2 * rng.standard_normal(C)).astype(np.float32)),
             g_pool=torch.from_numpy(rng.standard_normal((n_out, C)).astype(np.float32)))
    d = {k: v.contiguous().to(dev) for k, v in d.items()}
    # the statistics are inputs of both directions: each scene's nominal ones, not those of the rows (a scene of a few rows, all of them
    # far below its mean, would be normalised back to both signs and tie nowhere)
    mean = torch.from_numpy(np.repeat(shift[:, None], C, 1).astype(np.float32)).to(dev)
    var = torch.from_numpy(np.repeat(scale[:, None] ** 2, C, 1).astype(np.float32)).to(dev)
    cnt = torch.from_numpy(np.bincount(t['seg_in'], minlength=nseg).astype(np.float32)).to(dev)
    d.update(mean=mean.contiguous(), var=var.contiguous(), cnt=cnt.contiguous(), n_in=n_in, n_out=n_out, nseg=nseg, low=torch.from_numpy(low).to(dev),
             kcount=t['kcount'], parent_ref=torch.from_numpy(t['parent']).int().to(dev))
    # the arg-max-row forms
    out0 = torch.full((n_out, C), float('nan'), device=dev)
    arg0 = torch.full((n_out, C), -7, dtype=torch.int32, device=dev)
    y0 = torch.full((n_in, C), float('nan'), device=dev)
    parent0 = torch.full((n_in,), -7, dtype=torch.int32, device=dev)
    slot0 = torch.zeros(512, dtype=torch.int32, device=dev)
    L.call('fc_amax_out_hint', L.ptr(slot0))
    L.call('fc_norm_act_maxpool8_fwd', *_fwd_head(d), L.ptr(out0), L.ptr(arg0), L.ptr(y0), L.ptr(parent0), L.stream())
    gx0 = torch.full((n_in, C), float('nan'), device=dev)
    sums0 = torch.full((nseg, 2, C), float('nan'), device=dev)
    ws = L.workspace(L.query('fc_maxpool8_norm_act_bwd_ws_bytes', n_in, C, nseg), dev)
    L.call('fc_maxpool8_norm_act_bwd', L.ptr(d['x']), L.ptr(d['g_pool']), L.ptr(arg0), L.ptr(parent0), *_bwd_tail(d), L.ptr(gx0), L.ptr(sums0),
           L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    d.update(out0=out0, arg0=arg0, y0=y0, parent0=parent0, word0=_amax_word(slot0), gx0=gx0, sums0=sums0)
    return d


def _fwd_head(d, channels=C):
    return (L.ptr(d['x']), L.ptr(d['seg_in']), 4, channels, L.ptr(d['mean']), L.ptr(d['var']), EPS, L.ptr(d['gamma']), L.ptr(d['beta']), RELU,
            L.ptr(d['nbr']), d['n_out'])


def _bwd_tail(d, channels=C):
    return (L.ptr(d['seg_in']), 4, d['n_in'], channels, d['nseg'], L.ptr(d['mean']), L.ptr(d['var']), L.ptr(d['cnt']), EPS, L.ptr(d['gamma']),
            L.ptr(d['beta']), RELU)


def test_the_inputs_are_what_they_claim(case):
    d = case
    assert torch.equal(d['parent0'], d['parent_ref']), 'every input row is the child of one pooled row'
    assert float(d['out0'][d['low']].abs().max()) == 0.0, 'all-negative rows tie at 0'
    kc = d['kcount']
    assert (kc < 8).any() or d['n_out'] == 1, 'absent children'
    if d['n_out'] > d['nseg'] + 1:
        assert (kc == 1).any(), 'a pooled row with one child'
    if d['n_out'] > 3 * d['nseg']:
        assert int((d['arg0'] < 0).all(1).sum()) >= 1, 'a pooled row without children'
    # ties at 0: the winner is the first present child in offset order
    nbr = d['nbr'].long()
    first_present = nbr[(nbr >= 0).int().argmax(0), torch.arange(d['n_out'], device=nbr.device)]
    assert torch.equal(d['arg0'][d['low']].long(), first_present[d['low']][:, None].expand(-1, C).contiguous())


@pytest.mark.parametrize('with_argrow', [True, False], ids=['argrow', 'no-argrow'])
def test_mask_forward(case, with_argrow):
    d, dev = case, _dev()
    n_in, n_out = d['n_in'], d['n_out']
    out = torch.full((n_out, C), float('nan'), device=dev)
    arg = torch.full((n_out, C), -7, dtype=torch.int32, device=dev)
    y = torch.full((n_in, C), float('nan'), device=dev)
    parent = torch.full((n_in,), -7, dtype=torch.int32, device=dev)
    mask = torch.full((n_in,), 0x5555555555555555, dtype=torch.int64, device=dev)
    slot = torch.zeros(512, dtype=torch.int32, device=dev)
    L.call('fc_amax_out_hint', L.ptr(slot))
    L.call('fc_norm_act_maxpool8_mask_fwd', *_fwd_head(d), L.ptr(out), L.ptr(arg) if with_argrow else None, L.ptr(y), L.ptr(parent),
           L.ptr(mask), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(out, d['out0'])
    assert torch.equal(parent, d['parent0'])
    assert torch.equal(y, d['y0'])
    assert _amax_word(slot) == d['word0']
    if n_out > 1:
        assert d['word0'] != 0
    if with_argrow:
        assert torch.equal(arg, d['arg0'])
    else:
        assert int((arg != -7).sum()) == 0, 'no arg-max row is stored without a pointer'
    assert torch.equal(mask, PC.mask_from_argrow(d['arg0'], d['parent0']))
    # every channel of a pooled row with children is won by exactly one of them
    won = torch.zeros((n_out, C), dtype=torch.int64, device=dev)
    bits = (mask[:, None] >> torch.arange(C, device=dev)) & 1
    won.index_add_(0, parent.long(), bits)
    has = torch.from_numpy(d['kcount'] > 0).to(dev)
    assert torch.equal(won, has.long()[:, None].expand(-1, C).contiguous())


def test_mask_backward(case):
    d, dev = case, _dev()
    n_in, nseg = d['n_in'], d['nseg']
    mask = PC.mask_from_argrow(d['arg0'], d['parent0']).contiguous()
    gx = torch.full((n_in, C), float('nan'), device=dev)
    sums = torch.full((nseg, 2, C), float('nan'), device=dev)
    ws = L.workspace(L.query('fc_maxpool8_norm_act_bwd_ws_bytes', n_in, C, nseg), dev)
    ws.fill_(255)
    L.call('fc_maxpool8_mask_norm_act_bwd', L.ptr(d['x']), L.ptr(d['g_pool']), L.ptr(mask), L.ptr(d['parent0']), *_bwd_tail(d), L.ptr(gx),
           L.ptr(sums), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(d['gx0']).all() and torch.isfinite(d['sums0']).all()
    assert torch.equal(sums, d['sums0'])
    assert torch.equal(gx, d['gx0'])


def test_other_channel_counts_are_refused():
    dev = _dev()
    l = L.lib()
    z = torch.zeros(4096, device=dev)
    zi = torch.zeros(4096, dtype=torch.int32, device=dev)
    zm = torch.zeros(64, dtype=torch.int64, device=dev)
    p = L.ptr
    for channels in (4, 32, 60, 68, 128):
        assert l.fc_norm_act_maxpool8_mask_fwd(p(z), None, 0, channels, p(z), p(z), EPS, p(z), p(z), RELU, p(zi), 1, p(z), p(zi), None, p(zi), p(zm),
                                               L.stream()) == -1
        assert l.fc_maxpool8_mask_norm_act_bwd(p(z), p(z), p(zm), p(zi), None, 0, 1, channels, 1, p(z), p(z), p(z), EPS, p(z), p(z), RELU, p(z), p(z),
                                               p(z), 4096 * 4, L.stream()) == -1
    # ... and a missing mask or parent map
    assert l.fc_norm_act_maxpool8_mask_fwd(p(z), None, 0, C, p(z), p(z), EPS, p(z), p(z), RELU, p(zi), 1, p(z), p(zi), None, p(zi), None, L.stream()) == -1
    assert l.fc_norm_act_maxpool8_mask_fwd(p(z), None, 0, C, p(z), p(z), EPS, p(z), p(z), RELU, p(zi), 1, p(z), p(zi), None, None, p(zm), L.stream()) == -1
    torch.cuda.synchronize()


def test_executor_step_with_the_mask_equals_one_with_the_argmax_rows():
    dev = _dev()
    torch.manual_seed(0)
    cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=0.02)
    m = cfg.model
    m.backbone['n_outs'] = 2
    m.neck_with_head['in_channels'] = (64, 128)
    m.neck_with_head.assigner['n_scales'] = 2
    model = fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg')).to(dev).train()
    sc = [make_scene(s, n_points=20000) for s in (21, 22)]
    batch = dict(points=[torch.from_numpy(s[0]).to(dev) for s in sc],
                 gt_bboxes_3d=[fa.DepthInstance3DBoxes(torch.from_numpy(s[1]), origin=(.5, .5, .5)) for s in sc],
                 gt_labels_3d=[torch.from_numpy(s[2]).to(dev) for s in sc], img_metas=[dict(box_type_3d=fa.DepthInstance3DBoxes) for _ in sc])
    got = {}
    old = E.KEEP_STATE
    try:
        for keep in (False, True):
            E.KEEP_STATE = keep
            model.zero_grad(set_to_none=True)
            losses = model(return_loss=True, **batch)
            sum(losses.values()).backward()
            torch.cuda.synchronize()
            prog = E.program_for(model, True)
            tail = prog.ops_f[list(prog.ops_f[:, E.ROW_OP]).index(E.OP_NORM_POOL_FWD)]
            assert prog.keep_state == keep and tail[E.word(E.OP_NORM_POOL_FWD, 'mask')] > 0
            assert (tail[E.word(E.OP_NORM_POOL_FWD, 'arg')] >= 0) == keep
            got[keep] = ({k: float(v) for k, v in losses.items()}, {k: p.grad.detach().clone() for k, p in model.named_parameters()})
    finally:
        E.KEEP_STATE = old
    assert got[False][0] == got[True][0]
    assert set(got[False][1]) == set(got[True][1]) and len(got[False][1]) > 10
    for k, g in got[False][1].items():
        assert torch.equal(g, got[True][1][k]), k
