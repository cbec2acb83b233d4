"""-m gpu: every normalisation route class (tests/norm_cases.py: the census of csrc/norm_route.h and of the branches the block geometry
picks inside csrc/norm.hip) on integer operands with marker rows, against float64 numpy.

What is held bit-exact (torch.equal): the backward column sums (per segment too) for every n; gx / gres where n — every segment's
count — is a power of two; forward mean / var / count / running_mean where n is a power of two; the count, num_batches_tracked (+1,
once) and the amax word (max |.| of what the kernel wrote) always; fc_seg_col_sums always; the fused max pool's out / argrow / y on
integer statistics.  Everything else at the project's two bounds: 1e-5 of the tensor's scale for batch statistics, 1e-4 for y / gx.

One item per class, the class as its id.  Every launch of an item
  * is asserted, through the route query, to BE in the class before it is made,
  * finds every output at NaN, the counters at a known value and the whole cached workspace at 0xFF bytes,
  * goes through the C ABI: fc_bn_train_fwd / fc_bn_train_add_fwd, fc_bn_train_bwd, fc_bn_act_train_bwd, fc_norm_act_bwd, fc_col_stats,
    fc_seg_col_sums.
Further items: the segment forms with 64 segments (empty ones in the middle and at the end), ids unsorted inside a block, a block over
three segments, seg_stride 1 and 4, and both fused max-pool forms; n = 0; tables over 64 groups; Fn.bn_train / Fn.norm_act + autograd.
DESIGN.md section 5, "Exact-integer route tests"."""
import functools

import numpy as np
import pytest
import torch

import fcaf3d_amd.functional as Fn
from fcaf3d_amd import _lib as L
from tests import norm_cases as NC
from tests.amax_slots import _amax_bits, _amax_word, _new_slot

pytestmark = pytest.mark.gpu
SWEPT = NC.sweep()
PARAMS = [pytest.param(d, cls, id=NC.class_id(cls)) for d in NC.DIRECTIONS for cls in SWEPT[d]]
NAN = float('nan')
MOMENTUM = 0.25
NBT0 = 5


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _f(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _i(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(_dev())


def _nan(*shape):
    return torch.full(shape, NAN, device=_dev())


def _poisoned_workspace(nbytes):
    ws = L.workspace(max(int(nbytes), 16), _dev())
    ws.fill_(255)                                  # the WHOLE cached buffer: 0xFFFFFFFF is a NaN
    return ws


def _miss(name, got, want, bound):
    """'' if `got` (tensor) holds `want` (float64 numpy) to its bound (0: bit-equal after the cast to fp32), else what differs"""
    g = got.detach().cpu().numpy().reshape(want.shape)
    if bound == 0:
        w = want.astype(np.float32)
        if np.array_equal(g, w):
            return ''
        bad = ~(g == w)
        rows = np.nonzero(bad.reshape(bad.shape[0], -1).any(1))[0] if bad.ndim > 1 else np.nonzero(bad)[0]
        return f'{name}: {int(bad.sum())} of {bad.size} elements differ ({int(np.isnan(g).sum())} NaN), first indices {rows[:6].tolist()}'
    err, scale = float(np.abs(g.astype(np.float64) - want).max()) if g.size else 0.0, float(np.abs(want).max()) if want.size else 0.0
    if np.isfinite(g).all() and err <= bound * scale:
        return ''
    return f'{name}: max-abs error {err:.3e} over {bound:g} of the scale {scale:.3e} ({int((~np.isfinite(g)).sum())} non-finite)'


def _check(outs, exp, bnd, what):
    return [f'{what} {m}' for m in (_miss(k, outs[k], exp[k], bnd[k]) for k in exp) if m]


def _seg_args(inp, rep, case):
    if rep.nseg == 1:
        return None, 0
    return _i(NC.strided(inp['seg'], case.stride)), case.stride


# ---- one launch per case ----------------------------------------------------------------------------------------------------------------
def _run_fwd(cls, rep, case):
    n, C = case.n, rep.C
    inp, exp, bnd, _ = NC.build(rep, case)
    rc, r = NC.route_fields(rep, n)
    assert rc == 0 and NC.route_class(rep, n) == cls, f'{case}: the call left its class'
    x, gamma, beta, res = _f(inp['x']), _f(inp['gamma']), _f(inp['beta']), _f(inp.get('res'))
    part, add_inv, add_src = _f(inp.get('part')), _i(inp.get('add_inv')), _f(inp.get('add_src'))
    run = 'rmean' in inp
    rmean, rvar = _f(inp.get('rmean')), _f(inp.get('rvar'))
    nbt = torch.full((1,), NBT0, dtype=torch.int64, device=_dev()) if run else None
    y, mean, var, cnt = _nan(n, C), _nan(C), _nan(C), _nan(1)
    ws, slot = _poisoned_workspace(r['ws_bytes']), _new_slot()
    head = (L.ptr(x), n, C, NC.EPS_FWD, L.ptr(gamma), L.ptr(beta), L.ptr(res), inp['act'], MOMENTUM, L.ptr(y), L.ptr(mean), L.ptr(var), L.ptr(cnt),
            L.ptr(rmean), L.ptr(rvar), L.ptr(nbt), L.ptr(part), rep.nb_part, rep.groups, rep.small_elems)
    L.call('fc_amax_out_hint', L.ptr(slot))
    if add_inv is not None:
        L.call('fc_bn_train_add_fwd', *head, L.ptr(add_inv), L.ptr(add_src), L.ptr(ws), ws.numel(), L.stream())
    else:
        L.call('fc_bn_train_fwd', *head, L.ptr(ws), ws.numel(), L.stream())
    fails = _check({'y': y, 'mean': mean, 'var': var, 'cnt': cnt, 'rmean': rmean, 'rvar': rvar}, exp, bnd, f'{case}')
    if run and int(nbt) != NBT0 + 1:
        fails.append(f'{case} num_batches_tracked went from {NBT0} to {int(nbt)}')
    if _amax_word(slot) != _amax_bits(y):
        fails.append(f'{case} amax word {_amax_word(slot):#x}, max |y| {_amax_bits(y):#x}')
    return fails


def _run_bwd(cls, rep, case):
    n, C, nseg = case.n, rep.C, rep.nseg
    inp, exp, bnd, _ = NC.build(rep, case)
    rc, r = NC.route_fields(rep, n)
    assert rc == 0 and NC.route_class(rep, n) == cls, f'{case}: the call left its class'
    x, gy, gy2, y = _f(inp['x']), _f(inp['gy']), _f(inp.get('gy2')), _f(inp.get('y'))
    gamma, beta, mean, var, cnt = _f(inp['gamma']), _f(inp['beta']), _f(inp['mean']), _f(inp['var']), _f(inp['cnt'])
    part = _f(inp.get('part'))
    gx, gres, sums = _nan(n, C), (_nan(n, C) if 'gres' in exp else None), _nan(nseg, 2, C)
    ws, slot = _poisoned_workspace(r['ws_bytes']), _new_slot()
    tail = (0.0, L.ptr(gamma), L.ptr(beta), inp['act'], L.ptr(gx), L.ptr(gres), L.ptr(sums))
    L.call('fc_amax_out_hint', L.ptr(slot))
    if rep.entry == 'train':
        L.call('fc_bn_train_bwd', L.ptr(x), L.ptr(y), L.ptr(gy), L.ptr(gy2), n, C, L.ptr(mean), L.ptr(var), L.ptr(cnt), *tail, L.ptr(part),
               rep.nb_part, rep.small_elems, L.ptr(ws), ws.numel(), L.stream())
    elif rep.entry == 'small':
        L.call('fc_bn_act_train_bwd', L.ptr(x), L.ptr(y), L.ptr(gy), n, C, L.ptr(mean), L.ptr(var), *tail, L.ptr(ws), ws.numel(), L.stream())
    else:
        seg, stride = _seg_args(inp, rep, case)
        L.call('fc_norm_act_bwd', L.ptr(x), L.ptr(y), L.ptr(gy), L.ptr(seg), stride, n, C, nseg, L.ptr(mean), L.ptr(var), L.ptr(cnt), *tail,
               L.ptr(ws), ws.numel(), L.stream())
    fails = _check({'gx': gx, 'gres': gres, 'sums': sums}, exp, bnd, f'{case}')
    if _amax_word(slot) != _amax_bits(gx):
        fails.append(f'{case} amax word {_amax_word(slot):#x}, max |gx| {_amax_bits(gx):#x}')
    return fails


def _run_stats(cls, rep, case):
    n, C, nseg = case.n, rep.C, rep.nseg
    inp, exp, bnd, _ = NC.build(rep, case)
    assert NC.route_class(rep, n) == cls, f'{case}: the call left its class'
    x = _f(inp['x'])
    seg, stride = _seg_args(inp, rep, case)
    ws = _poisoned_workspace(L.query('fc_col_stats_ws_bytes', n, C, nseg))
    if rep.entry == 'col_stats':
        mean, var, cnt = _nan(nseg, C), _nan(nseg, C), _nan(nseg)
        L.call('fc_col_stats', L.ptr(x), L.ptr(seg), stride, n, C, nseg, L.ptr(mean), L.ptr(var), L.ptr(cnt), L.ptr(ws), ws.numel(), L.stream())
        fails = _check({'mean': mean, 'var': var, 'cnt': cnt}, exp, bnd, f'{case}')
        # whatever the other segments' counts: a segment whose own count is a power of two (or zero) is exact
        p2 = [s for s, c in enumerate(exp['cnt']) if c == 0 or NC.is_pow2(int(c))]
        fails += _check({'mean': mean[p2], 'var': var[p2]}, {'mean': exp['mean'][p2], 'var': exp['var'][p2]}, {'mean': 0, 'var': 0}, f'{case} pow2 segments')
        return fails
    out = _nan(nseg, C)
    L.call('fc_seg_col_sums', L.ptr(x), L.ptr(seg), stride, n, C, nseg, L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
    return _check({'sums': out}, exp, bnd, f'{case}')


def _stop_after_a_gpu_fault(e):
    """a HIP error leaves the process without a usable device: nothing more is launched from this session"""
    text = str(e)
    if 'hipError' in text or 'HIP error' in text or 'illegal memory access' in text:
        pytest.exit(f'GPU fault, no further launches: {text[:300]}', returncode=3)


def _guarded(test):
    """a HIP error surfaces where the host next waits for the device — often in the comparison, not at the launch"""
    @functools.wraps(test)
    def run(*a, **kw):
        try:
            return test(*a, **kw)
        except RuntimeError as e:
            _stop_after_a_gpu_fault(e)
            raise
    return run


_RUN = {NC.FWD: _run_fwd, NC.BWD: _run_bwd, NC.STATS: _run_stats}


@pytest.mark.parametrize('direction,cls', PARAMS)
@_guarded
def test_route_class_is_exact_on_integer_operands(direction, cls):
    rep = SWEPT[direction][cls]
    case_list = NC.cases(cls, rep)
    fails, launched = [], 0
    try:
        for case in case_list:
            fails += _RUN[direction](cls, rep, case)
            launched += 1
    except RuntimeError as e:
        _stop_after_a_gpu_fault(e)
        raise
    print(f'{rep}: {launched} cases, rows {sorted({c.n for c in case_list})}')
    assert not fails, f'{rep}: {len(fails)} findings in {launched} cases:\n' + '\n'.join(fails[:40])


# the sweep's classes take the first group count that reaches them (3): k_bn2_apply, windowed and not, and k_bn2_finalize once more on 64
# groups — (rows, channels, blocks of the table)
GROUPS64 = [(260, 64, 2), (260, 128, 2), (8321, 8, 65), (128, 128, 1)]


@pytest.mark.parametrize('n,C,nb_part', GROUPS64, ids=[f'n{n}-C{C}-table{b}' for n, C, b in GROUPS64])
@_guarded
def test_sixty_four_groups(n, C, nb_part):
    rep = NC.Rep('fwd', n, C, nb_part, 64, 1 << 20, 1)
    cls = NC.route_class(rep)
    assert cls is not None and cls.grouped and cls.windowed == (C == 128) and (cls.fin == 'bn2_finalize') == (nb_part > 64)
    fails = []
    for opts in (('res', 'add', 'run', 'relu'), ()):
        fails += _run_fwd(cls, rep, NC.Case(n, opts, 'one', 0))
    assert not fails, '\n'.join(fails)


# ---- the segment forms --------------------------------------------------------------------------------------------------------------------
# (rows or None: the 'pow2' table's own, channels, segments, table, seg_stride)
SEG_ITEMS = [(1000, 64, 64, 'contig', 1), (1000, 64, 64, 'contig', 4), (None, 8, 64, 'pow2', 4), (None, 128, 5, 'pow2', 1), (300, 68, 64, 'unsorted', 4),
             (200, 1024, 3, 'straddle', 1), (131, 4, 64, 'straddle', 4)]


@pytest.mark.parametrize('n,C,nseg,table,stride', SEG_ITEMS, ids=[f'{t}-n{n}-C{C}-nseg{s}-stride{st}' for n, C, s, t, st in SEG_ITEMS])
@_guarded
def test_segment_forms_are_exact_on_integer_operands(n, C, nseg, table, stride):
    """fc_col_stats, fc_seg_col_sums, fc_norm_act_fwd, fc_norm_act_bwd, fc_norm_act_maxpool8_fwd and fc_maxpool8_norm_act_bwd on one
    crafted segment table"""
    n = NC.pow2_rows(nseg) if n is None else n
    fails = []
    try:
        for entry in ('col_stats', 'seg_col_sums'):
            rep, case = NC.Rep(entry, n, C, 0, 1, 0, nseg), NC.Case(n, (), table, stride)
            fails += _run_stats(NC.route_class(rep), rep, case)
        rep = NC.Rep('seg', n, C, 0, 1, 0, nseg)
        for opts in (('y', 'gres', 'relu'), ('relu',), ('gres',)):
            fails += _run_bwd(NC.route_class(rep), rep, NC.Case(n, opts, table, stride))
        case = NC.Case(n, ('relu',), table, stride)
        inp, exp, bnd, _ = NC.build(rep, case)
        if table == 'pow2':
            assert bnd['gx'] == 0, 'the power-of-two table must hold gx to equality'
        x, gamma, beta, mean, var, cnt = (_f(inp[k]) for k in ('x', 'gamma', 'beta', 'mean', 'var', 'cnt'))
        seg, _ = _seg_args(inp, rep, case)
        ids = inp['seg']
        # k_norm_act_fwd with per-segment statistics, a residual and ReLU: integers and halves, exact
        res = NC.int_matrix((n, C), 11)
        y_ref = NC.ref_fwd_y(inp['x'], inp['mean'][ids], inp['var'][ids], 0.0, inp['gamma'], inp['beta'], NC.RELU, res)
        y, slot, res_t = _nan(n, C), _new_slot(), _f(res)          # (every operand in a variable: it must outlive its launch)
        L.call('fc_amax_out_hint', L.ptr(slot))
        L.call('fc_norm_act_fwd', L.ptr(x), L.ptr(seg), stride, n, C, L.ptr(mean), L.ptr(var), 0.0, L.ptr(gamma), L.ptr(beta), L.ptr(res_t), NC.RELU,
               L.ptr(y), L.stream())
        fails += _check({'y': y}, {'y': y_ref}, {'y': 0}, 'fc_norm_act_fwd')
        if _amax_word(slot) != _amax_bits(y):
            fails.append('fc_norm_act_fwd amax word')
        # the fused forward: normalise + ReLU + k2s2 max pool
        nbr, parent = NC.pool_table(ids, n + C)
        n_out = nbr.shape[1]
        nbr_t, parent_t = _i(nbr), _i(parent)
        y_ref = NC.ref_fwd_y(inp['x'], inp['mean'][ids], inp['var'][ids], 0.0, inp['gamma'], inp['beta'], NC.RELU)
        out_ref, arg_ref = NC.ref_pool(y_ref, nbr)
        out, yy, slot = _nan(n_out, C), _nan(n, C), _new_slot()
        arg = torch.full((n_out, C), -7, dtype=torch.int32, device=_dev())
        par = torch.full((n,), -7, dtype=torch.int32, device=_dev())
        L.call('fc_amax_out_hint', L.ptr(slot))
        L.call('fc_norm_act_maxpool8_fwd', L.ptr(x), L.ptr(seg), stride, C, L.ptr(mean), L.ptr(var), 0.0, L.ptr(gamma), L.ptr(beta), NC.RELU,
               L.ptr(nbr_t), n_out, L.ptr(out), L.ptr(arg), L.ptr(yy), L.ptr(par), L.stream())
        fails += _check({'out': out, 'y': yy}, {'out': out_ref, 'y': y_ref}, {'out': 0, 'y': 0}, 'fc_norm_act_maxpool8_fwd')
        if not np.array_equal(arg.cpu().numpy(), arg_ref) or (C >= 32 and not np.array_equal(par.cpu().numpy(), parent)):
            fails.append('fc_norm_act_maxpool8_fwd argrow / parent')
        if _amax_word(slot) != _amax_bits(out):
            fails.append('fc_norm_act_maxpool8_fwd amax word')
        # ... and its backward: the pooled gradient read through argrow / parent
        g_pool = NC.int_matrix((n_out, C), 13)
        g_pool_t, arg_t = _f(g_pool), _i(arg_ref)
        r = NC.ref_bwd(inp['x'], NC.pooled_gradient(g_pool, arg_ref, parent), inp['mean'], inp['var'], inp['gamma'], inp['beta'], NC.RELU, ids, nseg,
                       inp['cnt'])
        gx, sums = _nan(n, C), _nan(nseg, 2, C)
        ws = _poisoned_workspace(L.query('fc_maxpool8_norm_act_bwd_ws_bytes', n, C, nseg))
        L.call('fc_maxpool8_norm_act_bwd', L.ptr(x), L.ptr(g_pool_t), L.ptr(arg_t), L.ptr(parent_t), L.ptr(seg), stride, n, C, nseg, L.ptr(mean),
               L.ptr(var), L.ptr(cnt), 0.0, L.ptr(gamma), L.ptr(beta), NC.RELU, L.ptr(gx), L.ptr(sums), L.ptr(ws), ws.numel(), L.stream())
        exact = table == 'pow2' and NC.gx_premise(r, ids, inp['cnt'])
        fails += _check({'gx': gx, 'sums': sums}, {'gx': r['gx'], 'sums': r['sums']}, {'gx': 0 if exact else NC.REL_SCALE, 'sums': 0}, 'fc_maxpool8_norm_act_bwd')
    except RuntimeError as e:
        _stop_after_a_gpu_fault(e)
        raise
    assert not fails, '\n'.join(fails[:40])


@_guarded
def test_segment_forms_without_rows():
    """n = 0: the sums (mean, var, count) are zero-filled and nothing else is written"""
    C, nseg = 64, 3
    one = torch.zeros((1, C), device=_dev())          # (a valid address for the operands nobody reads)
    seg = torch.zeros((1,), dtype=torch.int32, device=_dev())
    mean, var, cnt, sums, gx = _nan(nseg, C), _nan(nseg, C), _nan(nseg), _nan(nseg, 2, C), _nan(1, C)
    ws = _poisoned_workspace(L.query('fc_col_stats_ws_bytes', 0, C, nseg))
    try:
        L.call('fc_col_stats', L.ptr(one), L.ptr(seg), 1, 0, C, nseg, L.ptr(mean), L.ptr(var), L.ptr(cnt), L.ptr(ws), ws.numel(), L.stream())
        assert not mean.any() and not var.any() and not cnt.any()
        out = _nan(nseg, C)
        L.call('fc_seg_col_sums', L.ptr(one), L.ptr(seg), 1, 0, C, nseg, L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
        assert not out.any()
        rc, r = L.route('fc_bn_train_bwd_route', 0, C, nseg, 0, 0, 0, NC.E['FC_NFORM_SEG'])
        assert rc == 0 and r['apply'] == NC.E['FC_NBAPPLY_NONE'] and r['launches'] == 0
        L.call('fc_norm_act_bwd', L.ptr(one), None, L.ptr(one), L.ptr(seg), 1, 0, C, nseg, L.ptr(mean), L.ptr(var), L.ptr(cnt), 0.0, None, None, 1,
               L.ptr(gx), None, L.ptr(sums), L.ptr(ws), ws.numel(), L.stream())
        assert not sums.any() and bool(torch.isnan(gx).all())
        y = _nan(1, C)
        L.call('fc_norm_act_fwd', L.ptr(one), L.ptr(seg), 1, 0, C, L.ptr(mean), L.ptr(var), 0.0, None, None, None, 1, L.ptr(y), L.stream())
        arg = torch.full((1, C), -7, dtype=torch.int32, device=_dev())
        L.call('fc_norm_act_maxpool8_fwd', L.ptr(one), L.ptr(seg), 1, C, L.ptr(mean), L.ptr(var), 0.0, None, None, 1, L.ptr(arg), 0, L.ptr(y), L.ptr(arg),
               None, None, L.stream())
        assert bool(torch.isnan(y).all()) and bool((arg == -7).all())
    except RuntimeError as e:
        _stop_after_a_gpu_fault(e)
        raise


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [False, True], ids=['small', 'table'])
@_guarded
def test_python_layer_on_integer_operands(fused):
    """Fn.bn_train (+ autograd) at a power-of-two n: the batch statistics and running_mean bit-equal to float64, y and the gradients
    (through the statistics) at 1e-4 of scale; Fn.norm_act over three segments likewise"""
    n, C = 256, 64
    rep = NC.Rep('fwd', n, C, 3 if fused else 0, 1, Fn.BN_SMALL_ELEMS, 1)
    case = NC.Case(n, ('res', 'run', 'relu'), 'one', 0)
    inp, exp, bnd, _ = NC.build(rep, case)
    assert bnd['mean'] == 0
    x, res = _f(inp['x']).requires_grad_(True), _f(inp['res']).requires_grad_(True)
    gamma, beta = _f(inp['gamma']).requires_grad_(True), _f(inp['beta']).requires_grad_(True)
    rmean, rvar, nbt = _f(inp['rmean']), _f(inp['rvar']), torch.zeros((), dtype=torch.long, device=_dev())
    go = NC.int_matrix((n, C), 5)
    try:
        _poisoned_workspace(0)
        y, (mean, var, cnt) = Fn.bn_train(x, gamma, beta, res, NC.EPS_FWD, 'relu', MOMENTUM, rmean, rvar, nbt, _f(inp.get('part')), 1)
        gx, gg, gb, gr = torch.autograd.grad(y, [x, gamma, beta, res], _f(go))
    except RuntimeError as e:
        _stop_after_a_gpu_fault(e)
        raise
    fails = _check({'y': y, 'mean': mean, 'var': var, 'cnt': cnt, 'rmean': rmean, 'rvar': rvar}, exp, bnd, 'bn_train')
    assert int(nbt) == 1
    mu, va = exp['mean'], exp['var']
    is_ = 1.0 / np.sqrt(va + NC.EPS_FWD)
    xh = (inp['x'] - mu) * is_
    gp = go * NC.act_grad(xh * inp['gamma'] + inp['beta'] + inp['res'], NC.RELU)
    s0, s1 = gp.sum(0), (gp * xh).sum(0)
    want = {'gx': inp['gamma'] * is_ * (gp - s0 / n - xh * s1 / n), 'ggamma': s1, 'gbeta': s0, 'gres': gp}
    fails += _check({'gx': gx, 'ggamma': gg, 'gbeta': gb, 'gres': gr}, want, {k: NC.REL_SCALE for k in want}, 'bn_train backward')
    if not fused:
        # Fn.norm_act: batch statistics per segment (fc_col_stats), three segments of 64, 128, 64 rows
        ids = np.repeat(np.arange(3, dtype=np.int32), (64, 128, 64))
        xs = _f(inp['x']).requires_grad_(True)
        seg = _i(NC.strided(ids, 4))          # the Python layer's ids are column 0 of the (n, 4) voxel coordinates: it passes seg_stride 4
        y, (mean, var, cnt) = Fn.norm_act(xs, _f(inp['gamma']), _f(inp['beta']), None, seg, 3, NC.EPS_FWD, 'relu')
        st = NC.ref_seg_stats(inp['x'], ids, 3)
        fails += _check({'mean': mean, 'var': var, 'cnt': cnt}, {k: st[k] for k in ('mean', 'var', 'cnt')}, {'mean': 0, 'var': 0, 'cnt': 0}, 'norm_act')
        m32, v32 = (st[k].astype(np.float32).astype(np.float64)[ids] for k in ('mean', 'var'))
        fails += _check({'y': y}, {'y': NC.ref_fwd_y(inp['x'], m32, v32, NC.EPS_FWD, inp['gamma'], inp['beta'], NC.RELU)}, {'y': NC.REL_SCALE}, 'norm_act')
        gx, = torch.autograd.grad(y, [xs], _f(go))
        is_ = 1.0 / np.sqrt(st['var'] + NC.EPS_FWD)[ids]
        xh = (inp['x'] - st['mean'][ids]) * is_
        gp = go * NC.act_grad(xh * inp['gamma'] + inp['beta'], NC.RELU)
        s0, s1 = np.zeros((3, C)), np.zeros((3, C))
        np.add.at(s0, ids, gp)
        np.add.at(s1, ids, gp * xh)
        cn = st['cnt'][ids][:, None]
        fails += _check({'gx': gx}, {'gx': inp['gamma'] * is_ * (gp - s0[ids] / cn - xh * s1[ids] / cn)}, {'gx': NC.REL_SCALE}, 'norm_act backward')
    assert not fails, '\n'.join(fails)
