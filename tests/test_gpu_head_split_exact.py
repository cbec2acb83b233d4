"""-m gpu: the head epilogue (csrc/head.hip: k_head_split_fwd, k_head_split_bwd, k_head_split_bwd_sums + k_head_sums_final) through the C
ABI on small-integer operands (tests/head_cases.py head_case), against float64.

Rows 1, 3, 4, 5 (the four rows a wave keeps in flight), 63, 64, 65 (the 64-row workgroup), 127, 129; row lengths 64, 32 and 25 — the last
with 1 + n_reg + n_cls == ld, no pad column, as is (64, 6, 57) —, eight regression columns, scale 0.5 and 2.  y's pad columns are nonzero
and must not be read; every sum and product is an integer or a half below 2^24, so everything but exp() is compared with torch.equal:
centerness, cls_score, cls_max, bbox[:, 6:], gy (exact zeros in the pad columns), gscale_row, gbias, gscale; bbox[:, :6] against float64
exp at the bound test_head_split_matches_torch applies (1e-4 of the scale).  The two backward entry points give bit-identical gy.  Each
incoming gradient passed as NULL gives exact zeros in its columns.  fc_amax_out_hint before fc_head_split_bwd_sums leaves the bits of
max |gy| in the slot — the word the backward-data GEMM scales by —, and without the hint no slot is touched.

Every output has 64 guard rows past n and starts as NaN, the workspace as 0xFF bytes: a store past the rows shows as a guard row that is
no longer NaN, not as a fault."""
import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from tests import head_cases as HC
from tests.amax_slots import _amax_bits, _amax_word, _new_slot

pytestmark = pytest.mark.gpu
NAN = float('nan')
G = HC.HEAD_GUARD


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _f(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _nan(*shape):
    return torch.full(shape, NAN, device=_dev())


def _stop_after_a_gpu_fault(e):
    """a HIP error leaves the process without a usable device: nothing more is launched from this session"""
    text = str(e)
    if 'hipError' in text or 'HIP error' in text or 'illegal memory access' in text:
        pytest.exit(f'GPU fault, no further launches: {text[:300]}', returncode=3)


def _exact(name, got, want, n):
    """'' if rows [0, n) of `got` equal `want` (float64) bit for bit after its cast to fp32 and every guard row is still NaN"""
    want = torch.from_numpy(np.ascontiguousarray(want, dtype=np.float32)).reshape(got[:n].shape)
    g = got.cpu()
    if not torch.equal(g[:n], want):
        bad = (g[:n] != want)
        return f'{name}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(g[:n]).sum())} NaN)'
    if not bool(torch.isnan(g[n:]).all()):
        return f'{name}: {int((~torch.isnan(g[n:])).sum())} elements past row {n} were written'
    return ''


def _forward(d):
    n, ld, n_reg, n_cls = d['n'], d['ld'], d['n_reg'], d['n_cls']
    y, bias, scale = _f(d['y']), _f(d['bias']), _f([d['scale']])
    cent, bbox, cls, cmax = _nan(n + G), _nan(n + G, n_reg), _nan(n + G, n_cls), _nan(n + G)
    L.call('fc_head_split_fwd', L.ptr(y), ld, L.ptr(bias), L.ptr(scale), n, n_reg, n_cls, L.ptr(cent), L.ptr(bbox), L.ptr(cls), L.ptr(cmax), L.stream())
    torch.cuda.synchronize()
    f = d['fwd']
    fails = [_exact('centerness', cent, f['centerness'], n), _exact('cls_score', cls, f['cls'], n), _exact('cls_max', cmax, f['cls_max'], n)]
    b = bbox.cpu()
    fails.append(_exact('bbox[:, 6:]', b[:, 6:].contiguous(), f['bbox_rest'], n))
    if not bool(torch.isnan(b[n:]).all()):
        fails.append('bbox: rows past n were written')
    got, want = b[:n, :6].double().numpy(), f['bbox_exp']
    err, scale_ = float(np.abs(got - want).max()), max(1.0, float(np.abs(want).max()))
    if not err <= 1e-4 * scale_:                       # (_close of tests/test_gpu_ops.py)
        fails.append(f'bbox[:, :6]: max err {err:.3e} vs scale {scale_:.3e}')
    return [m for m in fails if m]


def _backward(d, with_cent=True, with_bbox=True, with_cls=True, hint=False):
    """both entry points on the same operands; returns (findings, gy of fc_head_split_bwd_sums)"""
    n, ld, n_reg, n_cls = d['n'], d['ld'], d['n_reg'], d['n_cls']
    want = HC.head_backward(d, with_cent, with_bbox, with_cls)
    y, scale, bbox = _f(d['y']), _f([d['scale']]), _f(d['bbox_pred'])
    gc = _f(d['g_cent']) if with_cent else None
    gb = _f(d['g_bbox']) if with_bbox else None
    gk = _f(d['g_cls']) if with_cls else None
    gy1, row = _nan(n + G, ld), _nan(n + G)
    L.call('fc_head_split_bwd', L.ptr(y), ld, L.ptr(scale), L.ptr(bbox), L.ptr(gc), L.ptr(gb), L.ptr(gk), n, n_reg, n_cls, L.ptr(gy1), L.ptr(row), L.stream())
    gy2, gbias, gscale = _nan(n + G, ld), _nan(n_cls + G), _nan(1 + G)
    nbytes = L.query('fc_head_split_bwd_sums_ws_bytes', n)
    ws = torch.full((nbytes + 256,), 255, dtype=torch.uint8, device=_dev())
    slot = _new_slot()
    if hint:
        L.call('fc_amax_out_hint', L.ptr(slot))
    L.call('fc_head_split_bwd_sums', L.ptr(y), ld, L.ptr(scale), L.ptr(bbox), L.ptr(gc), L.ptr(gb), L.ptr(gk), n, n_reg, n_cls, L.ptr(gy2), L.ptr(gbias),
           L.ptr(gscale), L.ptr(ws), nbytes, L.stream())
    torch.cuda.synchronize()
    fails = [_exact('gy (bwd)', gy1, want['gy'], n), _exact('gscale_row', row, want['gscale_row'], n), _exact('gy (bwd_sums)', gy2, want['gy'], n),
             _exact('gbias', gbias, want['gbias'], n_cls), _exact('gscale', gscale, want['gscale'], 1)]
    if not torch.equal(gy1[:n].view(torch.int32), gy2[:n].view(torch.int32)):
        fails.append('gy differs between the two entry points')
    if not bool((ws[nbytes:] == 255).all()):
        fails.append('the workspace was written past its size')
    for name, on, lo_, hi_ in (('g_centerness', with_cent, 0, 1), ('g_bbox', with_bbox, 1, 1 + n_reg), ('g_cls', with_cls, 1 + n_reg, 1 + n_reg + n_cls)):
        if not on and not bool((gy2[:n, lo_:hi_] == 0).all() and (gy1[:n, lo_:hi_] == 0).all()):
            fails.append(f'NULL {name}: its columns of gy are not exact zeros')
    word = _amax_word(slot)
    if hint and word != _amax_bits(gy2[:n]):
        fails.append(f'amax word {word:#x}, max |gy| {_amax_bits(gy2[:n]):#x}')
    if not hint and word != 0:
        fails.append(f'no hint was given, and a slot holds {word:#x}')
    return [m for m in fails if m]


@pytest.mark.parametrize('ld,n_reg,n_cls', HC.HEAD_SHAPES)
def test_head_split_is_exact_on_integer_operands(ld, n_reg, n_cls):
    fails, launched = [], 0
    try:
        for n in HC.HEAD_ROWS:
            for scale in (0.5, 2.0):
                d = HC.head_case(n, ld, n_reg, n_cls, scale)
                assert float(np.abs(d['y'][:, 1 + n_reg + n_cls:]).min(initial=1.0)) > 0            # the pad columns hold something
                tag = f'n {n} scale {scale}'
                fails += [f'{tag} forward {m}' for m in _forward(d)]
                fails += [f'{tag} backward {m}' for m in _backward(d, hint=True)]
                fails += [f'{tag} backward without a hint {m}' for m in _backward(d)]
                launched += 3
            d = HC.head_case(n, ld, n_reg, n_cls, 2.0, seed=1)
            for k, name in enumerate(('g_centerness', 'g_bbox', 'g_cls')):
                on = [True, True, True]
                on[k] = False
                fails += [f'n {n} NULL {name}: {m}' for m in _backward(d, *on, hint=True)]
                launched += 1
    except RuntimeError as e:
        _stop_after_a_gpu_fault(e)
        raise
    print(f'ld {ld} n_reg {n_reg} n_cls {n_cls}: {launched} launches, rows {HC.HEAD_ROWS}')
    assert not fails, f'{len(fails)} findings:\n' + '\n'.join(fails[:40])
