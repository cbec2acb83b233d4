"""-m gpu: fc_bn_eval_bwd — the backward through a BatchNorm that reads its running statistics (csrc/norm_eval.h) — through the C ABI
against a float64 restatement, and _NormAct with constant statistics through autograd against torch's own eval-mode batch_norm.

Shapes (n, C) sit on the block, wave and cap edges of the two geometries: no rows; one thread; 63 / 64 / 65 rows around the 64-row
block floor; (257, 12) with 48 threads per block (no wave multiple); 128, 512 and the cap of 1 024 channels (16, 2 and 1 row lanes);
(65537, 4) with more than 64 rows per block (the 1 024-block cap).  Every shape runs act none / relu / elu x residual or not x gy2 or
not x sums or not.

Bounds, with u = 2^-24 (half an ulp of fp32, the relative error of one rounding), derived and not tuned:
  gx, gres  elementwise <= 8 u |reference|: the roundings of gy + gy2, of the product with act', of gamma rstd and of the product with
            it, plus rstd itself (an add, a square root and a division: under 3 u) — 7 u, and one more for ELU's y + 1;
  d beta    bit-equal to float64 for act none / relu: gy and gy2 are integers with n max|gy + gy2| < 2^24, every partial sum is
            exact; for ELU (g' is no integer) the bound of a sum of n fp32 terms, (n + 8) u sum|g'|;
  d gamma   <= (n + 8) u sum|g' xhat|: n additions in some order, and the eight roundings inside a term.
Every ReLU pre-activation is at least 2^-6 from zero in float64 (asserted), so that no element's decision can differ and none is left
out of the comparison."""
import itertools

import numpy as np
import pytest
import torch

import fcaf3d_amd.functional as Fn
from fcaf3d_amd import _lib as L

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EPS = 1e-5
SHAPES = [(0, 64), (1, 4), (63, 4), (64, 64), (65, 64), (257, 12), (1000, 128), (333, 512), (130, 1024), (65537, 4)]
VARIANTS = list(itertools.product((0, 1, 2), (False, True), (False, True), (False, True)))      # act, residual, gy2, sums
NAN = float('nan')


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _act64(p, act):
    return p if act == 0 else np.maximum(p, 0.0) if act == 1 else np.where(p > 0, p, np.expm1(np.minimum(p, 0.0)))


def make_case(n, C, act, has_res, seed):
    """fp32 operands (as float64 arrays holding fp32 values) with every activation argument at least 2^-6 from zero"""
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    rmean = f32(rng.uniform(-1, 1, C))
    rvar = f32(rng.uniform(0.5, 2.0, C))
    gamma = f32(rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C))
    beta = f32(rng.uniform(-0.5, 0.5, C))
    x = f32(rmean + np.sqrt(rvar) * rng.standard_normal((n, C)))
    res = f32(rng.standard_normal((n, C))) if has_res else None
    rstd = 1.0 / np.sqrt(rvar + np.float64(np.float32(EPS)))

    def pre_of(xx):
        return (xx - rmean) * rstd * gamma + beta + (res if has_res else 0.0)
    # an argument inside the band moves out of it: 0.25 in x is at least 0.25 * 0.5 * 0.7 = 0.0875 in the argument, away from zero
    pre = pre_of(x)
    near = np.abs(pre) < 2.0 ** -4
    x = f32(np.where(near, x + 0.25 * np.sign(gamma) * np.where(pre >= 0, 1.0, -1.0), x))
    pre = pre_of(x)
    y = f32(_act64(pre, act)) if has_res else None        # what the forward kernel would have stored (read only behind a residual)
    gy = rng.integers(-8, 9, (n, C)).astype(np.float64)
    gy2 = rng.integers(-8, 9, (n, C)).astype(np.float64)
    return dict(x=x, y=y, res=res, gy=gy, gy2=gy2, rmean=rmean, rvar=rvar, gamma=gamma, beta=beta, rstd=rstd, pre=pre)


def reference(c, act, has_res, has_gy2):
    """the issue's arithmetic in float64; act' from y behind a residual (as the kernels), else from the pre-activation"""
    g = c['gy'] + (c['gy2'] if has_gy2 else 0.0)
    if act == 1:
        d = ((c['y'] if has_res else c['pre']) > 0).astype(np.float64)
    elif act == 2:
        d = np.where(c['y'] > 0, 1.0, c['y'] + 1.0) if has_res else np.where(c['pre'] > 0, 1.0, np.exp(np.minimum(c['pre'], 0.0)))
    else:
        d = 1.0
    gp = g * d
    xh = (c['x'] - c['rmean']) * c['rstd']
    return dict(gx=gp * c['gamma'] * c['rstd'], gres=gp, dbeta=gp.sum(0), dgamma=(gp * xh).sum(0), abs_b=np.abs(gp).sum(0),
                abs_g=np.abs(gp * xh).sum(0))


def launch(c, n, C, act, has_res, has_gy2, want_sums, dev_ops=None, ws_bytes=None, amax=None):
    """one fc_bn_eval_bwd call on NaN-filled outputs and a 0xFF-filled workspace -> (rc, gx, gres, sums)"""
    d = dev_ops or {k: _t(c[k]) for k in ('x', 'y', 'gy', 'gy2', 'rmean', 'rvar', 'gamma', 'beta')}
    gx = torch.full((n, C), NAN, device=_dev())
    gres = torch.full((n, C), NAN, device=_dev()) if has_res else None
    sums = torch.full((2, C), NAN, device=_dev()) if want_sums else None
    need = L.query('fc_bn_eval_bwd_ws_bytes', n, C, int(want_sums))
    ws = L.workspace(max(need, 16), _dev())
    ws.fill_(255)
    rc = L.lib().fc_bn_eval_bwd(L.ptr(d['x']), L.ptr(d['y']) if has_res else None, L.ptr(d['gy']), L.ptr(d['gy2']) if has_gy2 else None, n, C,
                                L.ptr(d['rmean']), L.ptr(d['rvar']), EPS, L.ptr(d['gamma']), L.ptr(d['beta']), act, L.ptr(gx), L.ptr(gres),
                                L.ptr(sums), L.ptr(amax), L.ptr(ws), need if ws_bytes is None else ws_bytes, L.stream())
    torch.cuda.synchronize()
    return rc, gx, gres, sums


def _rel_miss(name, got, want, k):
    g = got.cpu().numpy().astype(np.float64)
    err = np.abs(g - want)
    lim = k * U * np.abs(want)
    worst = float((err / np.maximum(np.abs(want), 1e-300)).max() / U) if want.size else 0.0
    print(f'    {name}: worst relative error {worst:.2f} u (bound {k} u)')
    bad = ~(err <= lim)
    return [] if not bad.any() else [f'{name}: {int(bad.sum())} of {bad.size} elements over {k} u |reference|, worst {worst:.2f} u']


ELU_FROM_X = [v for v in VARIANTS if v[0] == 2 and not v[1]]      # act' = exp(pre) from x: see test_entry_point_elu_recomputed_from_x


@pytest.mark.parametrize('n,C', SHAPES, ids=[f'{n}x{C}' for n, C in SHAPES])
def test_entry_point_against_float64(n, C):
    check_variants(n, C, [v for v in VARIANTS if v not in ELU_FROM_X])


@pytest.mark.parametrize('n,C', SHAPES, ids=[f'{n}x{C}' for n, C in SHAPES])
def test_entry_point_elu_recomputed_from_x(n, C):
    """ELU without a residual: act' = exp(pre) below zero, and exp turns the ABSOLUTE error of pre into a relative error of act'.  Formed
    in fp32 by bn_pre (about 4.5 u |xhat gamma| + u |pre| of absolute error) the worst elements were at 10 to 14 u on five of these shapes;
    the kernel therefore takes the derivative's value from a pre-activation formed in fp64 and split into head and tail (csrc/norm_eval.h),
    the sign decision staying bn_pre's.  Measured on the MI355X since: 4.8 u at the worst element of any shape."""
    check_variants(n, C, ELU_FROM_X)


def check_variants(n, C, variants):
    fails = []
    for act, has_res, has_gy2, want_sums in variants:
        what = f'act {act} res {int(has_res)} gy2 {int(has_gy2)} sums {int(want_sums)}'
        c = make_case(n, C, act, has_res, seed=1000 * C + n % 1000 + 7 * act + has_res)
        if act == 1:
            assert n == 0 or np.abs(c['pre']).min() >= 2.0 ** -6, what
        assert n * 16 < 2 ** 24
        ref = reference(c, act, has_res, has_gy2)
        slot = torch.zeros(512, dtype=torch.int32, device=_dev())
        rc, gx, gres, sums = launch(c, n, C, act, has_res, has_gy2, want_sums, amax=slot)
        assert rc == 0, what
        print(what)
        f = _rel_miss('gx', gx, ref['gx'], 8)
        if has_res:
            f += _rel_miss('gres', gres, ref['gres'], 8)
        if want_sums:
            s = sums.cpu().numpy().astype(np.float64)
            if act != 2:
                if not np.array_equal(s[0], ref['dbeta']):
                    f.append(f'd beta: {int((s[0] != ref["dbeta"]).sum())} of {C} channels differ from the exact sum')
            elif not (np.abs(s[0] - ref['dbeta']) <= (n + 8) * U * ref['abs_b']).all():
                f.append(f'd beta: error {np.abs(s[0] - ref["dbeta"]).max():.3e} over (n + 8) u sum|g\'|')
            eg = np.abs(s[1] - ref['dgamma'])
            print(f'    d gamma: worst error / ((n + 8) u sum|g\' xhat|) = {float((eg / np.maximum((n + 8) * U * ref["abs_g"], 1e-300)).max()) if n else 0.0:.3f}')
            if not (eg <= (n + 8) * U * ref['abs_g']).all():
                f.append(f'd gamma: error {eg.max():.3e} over (n + 8) u sum|g\' xhat|')
        # the amax word is max |gx| of the tensor returned
        word = int(slot.view(32, 16)[:, 0].max())
        want_word = int(gx.abs().max().reshape(1).view(torch.int32)) if n else 0
        if word != want_word:
            f.append(f'amax word {word:#x}, max |gx| {want_word:#x}')
        fails += [f'{what}: {m}' for m in f]
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('n,C', [(65, 64), (257, 12), (333, 512), (65537, 4)], ids=lambda v: str(v))
def test_two_calls_on_equal_inputs_are_bit_equal(n, C):
    c = make_case(n, C, 2, True, seed=5)
    c['gy'] = c['gy'] + np.random.default_rng(1).standard_normal((n, C)).astype(np.float32)      # no integers: the order of the sums shows
    a = launch(c, n, C, 2, True, True, True)
    b = launch(c, n, C, 2, True, True, True)
    assert a[0] == b[0] == 0
    for p, q in zip(a[1:], b[1:]):
        assert torch.equal(p, q)
    assert torch.isfinite(a[3]).all()


def test_refused_calls_leave_gx_untouched():
    c = make_case(64, 64, 1, False, seed=3)
    ops = {k: _t(c[k]) for k in ('x', 'gy', 'gy2', 'rmean', 'rvar', 'gamma', 'beta')}
    ops['y'] = None
    for n, C, act in ((64, 2, 1), (64, 6, 1), (64, 1028, 1), (-1, 64, 1), (64, 64, 3), (64, 64, -1)):
        for want_sums in (False, True):
            gx = torch.full((64, 64), NAN, device=_dev())
            sums = torch.full((2, 64), NAN, device=_dev()) if want_sums else None
            ws = L.workspace(1 << 20, _dev())
            rc = L.lib().fc_bn_eval_bwd(L.ptr(ops['x']), None, L.ptr(ops['gy']), None, n, C, L.ptr(ops['rmean']), L.ptr(ops['rvar']), EPS,
                                        L.ptr(ops['gamma']), L.ptr(ops['beta']), act, L.ptr(gx), None, L.ptr(sums), None, L.ptr(ws), 1 << 20,
                                        L.stream())
            torch.cuda.synchronize()
            assert rc == -1, (n, C, act, want_sums)
            assert torch.isnan(gx).all() and (sums is None or torch.isnan(sums).all())
    need = L.query('fc_bn_eval_bwd_ws_bytes', 64, 64, 1)
    assert need > 0
    rc, gx, _, sums = launch(c, 64, 64, 1, False, False, True, dev_ops=ops, ws_bytes=need - 1)
    assert rc == -2 and torch.isnan(gx).all() and torch.isnan(sums).all()
    rc, gx, _, _ = launch(c, 64, 64, 1, False, False, False, dev_ops=ops, ws_bytes=0)      # no sums: no workspace
    assert rc == 0 and torch.isfinite(gx).all()


AUTOGRAD_CASES = [(None, False), ('relu', False), ('elu', False), (None, True), ('relu', True)]


@pytest.mark.parametrize('act,has_res', AUTOGRAD_CASES, ids=[f'{a}-{"residual" if r else "plain"}' for a, r in AUTOGRAD_CASES])
def test_autograd_through_constant_statistics_matches_torch_eval_batch_norm(act, has_res):
    """Fn.norm_act with stats given (what MinkowskiBatchNorm runs in eval mode), forward and backward through autograd, against
    torch.nn.functional.batch_norm(training=False) autograd in float64 — within the bounds of the entry point.  Also with gamma / beta
    frozen: their gradients are None and gx holds the same bound.
    The forms are the model's (BasicBlock: relu, residual + relu; the neck: elu) and the plain ones.  ELU behind a residual is not among
    them: there act' is y + 1 of the STORED fp32 y, whose rounding (2^-25 absolute) is not bounded relative to exp(pre) — that form is
    held to the same bounds against the restatement that reads the same y (test_entry_point_against_float64)."""
    n, C = 257, 64
    a = {None: 0, 'relu': 1, 'elu': 2}[act]
    c = make_case(n, C, a, has_res, seed=11)
    t64 = lambda k: torch.from_numpy(c[k]).requires_grad_(True)
    x64, g64, b64 = t64('x'), t64('gamma'), t64('beta')
    r64 = t64('res') if has_res else None
    pre = torch.nn.functional.batch_norm(x64, torch.from_numpy(c['rmean']), torch.from_numpy(c['rvar']), g64, b64, False, 0.0, float(np.float32(EPS)))
    if has_res:
        pre = pre + r64
    y64 = pre if a == 0 else torch.relu(pre) if a == 1 else torch.nn.functional.elu(pre)
    gy = torch.from_numpy(c['gy'])
    y64.backward(gy)
    if a == 1:
        assert float(pre.detach().abs().min()) >= 2.0 ** -6
    gp = r64.grad if has_res else (gy * (1.0 if a == 0 else (pre > 0).double() if a == 1 else torch.where(pre > 0, 1.0, torch.exp(pre)))).detach()
    xh = ((x64 - torch.from_numpy(c['rmean'])) * torch.from_numpy(c['rstd'])).detach()
    for train_affine in (True, False):
        x = _t(c['x']).requires_grad_(True)
        gm = _t(c['gamma']).requires_grad_(train_affine)
        bt = _t(c['beta']).requires_grad_(train_affine)
        res = _t(c['res']).requires_grad_(True) if has_res else None
        stats = (_t(c['rmean']).reshape(1, C), _t(c['rvar']).reshape(1, C), torch.ones(1, device=_dev()))
        y, _ = Fn.norm_act(x, gm, bt, residual=res, eps=EPS, act=act, stats=stats)
        y.backward(_t(c['gy']))
        torch.cuda.synchronize()
        print(f'train_affine {train_affine}')
        fails = _rel_miss('gx', x.grad, x64.grad.numpy(), 8)
        if has_res:
            fails += _rel_miss('gres', res.grad, r64.grad.numpy(), 8)
        if train_affine:
            eb = (bt.grad.cpu().double() - b64.grad).abs()
            eg = (gm.grad.cpu().double() - g64.grad).abs()
            if a != 2 and not bool((eb == 0).all()):
                fails.append('d beta differs from the exact sum')
            if a == 2 and not bool((eb <= (n + 8) * U * gp.abs().sum(0)).all()):
                fails.append('d beta over its bound')
            if not bool((eg <= (n + 8) * U * (gp * xh).abs().sum(0)).all()):
                fails.append('d gamma over its bound')
        else:
            assert gm.grad is None and bt.grad is None
        assert not fails, f'train_affine {train_affine}: ' + '; '.join(fails)
