"""-m gpu: every instantiation of k_norm_bwd_partial (csrc/norm_rows.h: pooled or not x reads y x reads gy2) through the existing entry
points, on small-integer operands — every sum is exact in any order — against a float64 evaluation on the CPU.

  fc_bn_train_bwd (small_elems = 0)   plain, y or not, gy2 or not          one segment
  fc_norm_act_bwd                     plain, y or not                      2 and 8 segments, a boundary on a block edge and one inside a block
  fc_maxpool8_norm_act_bwd            pooled through the arg-max rows      2 scenes, 301 pooled rows, absent children
  fc_maxpool8_mask_norm_act_bwd       pooled through the per-child mask    the same

C in {4, 64, 256, 1024} (1, 16, 64, 256 channel lanes: 16, 16, 4, 1 row lanes), n in {1, 63, 64, 65, 129, 4 nrl + 1, 4097}.

Held to torch.equal: the two sums always, gres always, and gx wherever the apply step divides by the `cnt` it is given (a power of two
here: every segment form, the pooled forms, and fc_bn_train_bwd from 65 row blocks on) or n is a power of two.  fc_bn_train_bwd on at
most 64 row blocks applies through k_bn1_bwd_apply, which multiplies by fl(1 / n): for the other n its gx is held to 2^-21 of
max |gamma invstd| (max |g'| + max |S1| / n + max |xhat| max |S2| / n) — five roundings of 2^-24 relative each (1 / n, two products
with it, two subtractions), doubled, on terms of at most that size; the kernel under test there is the one that makes the sums.

One case per instantiation on random floats: max-abs error over the tensor's maximum against float64, at most twice the error of the
same call on the kernels before the change (PARENT_ERR, measured on MI355X: profiles/r7_notes.md section 12).  It guards the loads."""
import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from tests import pool_cases as PC

pytestmark = pytest.mark.gpu
RELU = 1
NAN = float('nan')


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _nrl(C):
    return max(1, min(16, 256 // (C // 4)))


def _rpb(n):
    """rows per block of the reduction (csrc/norm_route.h row_blocks, cap 1 024)"""
    g = min(1024, -(-n // 64))
    return -(-n // g)


def _t(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_dev())


def _segments(n, nseg):
    """segment of every row, contiguous.  Two segments: the boundary inside a block; more: the first boundary on a block edge, the second
    inside a block, the rest spread.  Short matrices leave the last segments empty"""
    if nseg == 1:
        return np.zeros(n, dtype=np.int64)
    rpb = _rpb(n)
    inside = rpb + max(1, rpb // 2)
    cuts = [inside] if nseg == 2 else [rpb, inside] + [inside + (i + 1) * max(1, (n - 2 * rpb) // nseg) for i in range(nseg - 3)]
    seg = np.zeros(n, dtype=np.int64)
    for c in cuts:
        if c < n:
            seg[c:] += 1
    return seg


def _operands(n, C, nseg, seed, integers):
    rng = np.random.default_rng(seed)
    if integers:
        d = dict(x=rng.integers(-4, 5, (n, C)), gy=rng.integers(-2, 3, (n, C)), gy2=rng.integers(-1, 2, (n, C)), y=rng.integers(-1, 3, (n, C)),
                 mean=rng.integers(0, 2, (nseg, C)), var=np.full((nseg, C), 4.0), gamma=2.0 ** rng.integers(0, 2, C), beta=rng.integers(-1, 2, C),
                 cnt=2.0 ** (6 + np.arange(nseg) % 3), eps=0.0)
    else:
        d = dict(x=rng.standard_normal((n, C)) * 1.5 + 0.5, gy=rng.standard_normal((n, C)), gy2=rng.standard_normal((n, C)),
                 y=rng.standard_normal((n, C)), mean=0.5 + 0.1 * rng.standard_normal((nseg, C)), var=2.25 + 0.2 * rng.random((nseg, C)),
                 gamma=0.5 + rng.random(C), beta=0.2 * rng.standard_normal(C), cnt=None, eps=1e-5)
    return {k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _reference(d, seg, nseg, g, from_y, cnt):
    """float64: sums (nseg, 2, C), gx, gres of the normalisation backward with ReLU; operands as the device reads them (fp32 values)"""
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    x, mu, va, gm, bt = f32(d['x']), f32(d['mean'])[seg], f32(d['var'])[seg], f32(d['gamma']), f32(d['beta'])
    inv_std = 1.0 / np.sqrt(va + np.float64(np.float32(d['eps'])))
    xh = (x - mu) * inv_std
    on = f32(d['y']) > 0 if from_y else xh * gm + bt > 0
    gp = g * on
    sums = np.zeros((nseg, 2, x.shape[1]))
    np.add.at(sums[:, 0], seg, gp)
    np.add.at(sums[:, 1], seg, gp * xh)
    c = cnt[seg][:, None]
    gx = gm * inv_std * (gp - sums[seg, 0] / c - xh * sums[seg, 1] / c)
    return dict(sums=sums, gx=gx, gres=gp, xh=xh, scale=gm * inv_std)


def _launch(entry, d, n, C, nseg, seg, from_y, with_gy2, cnt, pool=None):
    """one call of `entry` on NaN-filled outputs -> dict(sums, gx, gres | None)"""
    dev = _dev()
    x, y, gy, gy2 = _t(d['x']), (_t(d['y']) if from_y else None), _t(d['gy']), (_t(d['gy2']) if with_gy2 else None)
    mean, var, gamma, beta, cn = _t(d['mean']), _t(d['var']), _t(d['gamma']), _t(d['beta']), _t(cnt)
    gx, sums = torch.full((n, C), NAN, device=dev), torch.full((nseg, 2, C), NAN, device=dev)
    gres = torch.full((n, C), NAN, device=dev) if pool is None else None
    p, eps = L.ptr, float(d['eps'])
    if entry == 'fc_bn_train_bwd':
        ws = L.workspace(L.query('fc_bn_train_ws_bytes', n, C), dev)
        ws.fill_(255)
        L.call(entry, p(x), p(y), p(gy), p(gy2), n, C, p(mean), p(var), p(cn), eps, p(gamma), p(beta), RELU, p(gx), p(gres), p(sums), None, 0, 0,
               p(ws), ws.numel(), L.stream())
    elif entry == 'fc_norm_act_bwd':
        sg = _t(seg, np.int32)
        ws = L.workspace(L.query('fc_norm_act_bwd_ws_bytes', n, C, nseg), dev)
        ws.fill_(255)
        L.call(entry, p(x), p(y), p(gy), p(sg), 1, n, C, nseg, p(mean), p(var), p(cn), eps, p(gamma), p(beta), RELU, p(gx), p(gres), p(sums),
               p(ws), ws.numel(), L.stream())
    else:
        sg = _t(seg, np.int32)
        ws = L.workspace(L.query('fc_maxpool8_norm_act_bwd_ws_bytes', n, C, nseg), dev)
        ws.fill_(255)
        L.call(entry, p(x), p(pool['g_pool']), p(pool['mask'] if 'mask' in entry else pool['argrow']), p(pool['parent']), p(sg), 1, n, C, nseg,
               p(mean), p(var), p(cn), eps, p(gamma), p(beta), RELU, p(gx), p(sums), p(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return dict(sums=sums, gx=gx, gres=gres)


def _equal(got, want):
    return np.array_equal(got.cpu().numpy(), want.astype(np.float32))


SHAPES = [(C, n) for C in (4, 64, 256, 1024) for n in sorted({1, 63, 64, 65, 129, 4 * _nrl(C) + 1, 4097})]


@pytest.mark.parametrize('C,n', SHAPES, ids=[f'C{C}-n{n}' for C, n in SHAPES])
def test_plain_forms_are_exact_on_integer_operands(C, n):
    fails = []
    for nseg in (1, 2, 8):
        d = _operands(n, C, nseg, 1000 * C + n + nseg, integers=True)
        seg = _segments(n, nseg)
        for from_y in (False, True):
            for with_gy2 in ((False, True) if nseg == 1 else (False,)):
                entry = 'fc_bn_train_bwd' if nseg == 1 else 'fc_norm_act_bwd'
                g = d['gy'] + (d['gy2'] if with_gy2 else 0.0)
                by_n = entry == 'fc_bn_train_bwd' and -(-n // _rpb(n)) <= 64          # k_bn1_bwd_apply: 1 / n, not cnt
                cnt = np.array([float(n)]) if by_n else d['cnt']
                ref = _reference(d, seg, nseg, g, from_y, cnt)
                out = _launch(entry, d, n, C, nseg, seg, from_y, with_gy2, cnt)
                what = f'{entry} C={C} n={n} nseg={nseg} y={from_y} gy2={with_gy2}'
                for k in ('sums', 'gres'):
                    if not _equal(out[k], ref[k]):
                        fails.append(f'{what}: {k} differs')
                if not by_n or n & (n - 1) == 0:
                    if not _equal(out['gx'], ref['gx']):
                        fails.append(f'{what}: gx differs')
                else:
                    s = ref['sums']
                    bound = 2.0 ** -21 * np.abs(ref['scale']).max() * (np.abs(ref['gres']).max() + np.abs(s[:, 0]).max() / n
                                                                     + np.abs(ref['xh']).max() * np.abs(s[:, 1]).max() / n)
                    err = np.abs(out['gx'].cpu().numpy().astype(np.float64) - ref['gx']).max()
                    if not err <= bound:
                        fails.append(f'{what}: gx off by {err:.3e}, bound {bound:.3e}')
    assert not fails, '\n'.join(fails)


def _pooled_case(n_out, nseg, seed, integers):
    t = PC.pool_table(n_out, nseg, seed, single_child_row=nseg)
    n, rng = t['n_in'], np.random.default_rng(seed + 1)
    d = _operands(n, 64, nseg, seed + 2, integers)
    # arg-max rows: any present child per (pooled row, channel), -1 for a row without children — a legal input of the backward pass
    nbr = t['nbr']                                                       # (8, n_out)
    pick = np.argsort(np.where(nbr >= 0, rng.random((64, 8, n_out)), 2.0), axis=1)[:, 0, :]      # (64, n_out): a present slot per channel
    argrow = nbr[pick, np.arange(n_out)[None, :]].T                     # (n_out, 64)
    g_pool = rng.integers(-2, 3, (n_out, 64)).astype(np.float64) if integers else rng.standard_normal((n_out, 64))
    g = np.zeros((n, 64))
    ok = argrow >= 0
    g[argrow[ok], np.broadcast_to(np.arange(64), argrow.shape)[ok]] = g_pool.astype(np.float32).astype(np.float64)[ok]
    argrow_t, parent_t = _t(argrow, np.int32), _t(t['parent'], np.int32)
    pool = dict(g_pool=_t(g_pool), argrow=argrow_t, parent=parent_t, mask=PC.mask_from_argrow(argrow_t, parent_t).contiguous())
    return d, t, g, pool


@pytest.mark.parametrize('entry', ['fc_maxpool8_norm_act_bwd', 'fc_maxpool8_mask_norm_act_bwd'])
def test_pooled_forms_are_exact_on_integer_operands(entry):
    nseg, n_out = 2, 301
    d, t, g, pool = _pooled_case(n_out, nseg, 77, integers=True)
    assert (t['kcount'] < 8).any() and (t['kcount'] == 0).any(), 'absent children'
    ref = _reference(d, t['seg_in'], nseg, g, False, d['cnt'])
    out = _launch(entry, d, t['n_in'], 64, nseg, t['seg_in'], False, False, d['cnt'], pool)
    assert _equal(out['sums'], ref['sums'])
    assert _equal(out['gx'], ref['gx'])


# max-abs error / tensor maximum against float64 of the same calls on the kernels before this change (MI355X), (sums, gx)
PARENT_ERR = {('fc_bn_train_bwd', False, False): (2.124e-07, 1.188e-07), ('fc_bn_train_bwd', False, True): (1.387e-07, 1.306e-07),
              ('fc_bn_train_bwd', True, False): (1.889e-07, 1.179e-07), ('fc_bn_train_bwd', True, True): (1.752e-07, 1.654e-07),
              'fc_maxpool8_norm_act_bwd': (2.890e-07, 1.233e-07)}
RANDOM = [('fc_bn_train_bwd', False, False), ('fc_bn_train_bwd', False, True), ('fc_bn_train_bwd', True, False), ('fc_bn_train_bwd', True, True),
          ('fc_maxpool8_norm_act_bwd', False, False), ('fc_maxpool8_mask_norm_act_bwd', False, False)]


@pytest.mark.parametrize('entry,from_y,with_gy2', RANDOM, ids=[f'{e}-y{int(a)}-gy2{int(b)}' for e, a, b in RANDOM])
def test_random_floats_against_float64(entry, from_y, with_gy2):
    if 'maxpool8' in entry:
        nseg, n_out = 2, 3001
        d, t, g, pool = _pooled_case(n_out, nseg, 91, integers=False)
        n, C, seg = t['n_in'], 64, t['seg_in']
        cnt = np.bincount(seg, minlength=nseg).astype(np.float64)
    else:
        n, C, nseg, pool = 20011, 64, 1, None
        d = _operands(n, C, nseg, 93, integers=False)
        seg, cnt = np.zeros(n, dtype=np.int64), np.array([float(n)])
        g = (d['gy'].astype(np.float32) + (d['gy2'].astype(np.float32) if with_gy2 else np.float32(0))).astype(np.float64)   # the device's fp32 add
    ref = _reference(d, seg, nseg, g, from_y, cnt)
    out = _launch(entry, d, n, C, nseg, seg, from_y, with_gy2, cnt, pool)
    err = {k: float(np.abs(out[k].cpu().numpy().astype(np.float64) - ref[k]).max() / np.abs(ref[k]).max()) for k in ('sums', 'gx')}
    print(f'partial forms, random floats: {entry} y={from_y} gy2={with_gy2} n={n}: sums {err["sums"]:.3e} gx {err["gx"]:.3e}')
    key = 'fc_maxpool8_norm_act_bwd' if 'maxpool8' in entry else (entry, from_y, with_gy2)      # the mask form: the arg-max-row call's error
    assert key in PARENT_ERR, 'no recorded error of the kernels before the change'
    e_sums, e_gx = PARENT_ERR[key]
    assert np.isfinite(out['gx'].cpu().numpy()).all() and err['sums'] <= 2.0 * e_sums and err['gx'] <= 2.0 * e_gx, (err, PARENT_ERR[key])
