"""-m gpu: every convolution route class (tests/conv_cases.py: the census of csrc/conv_route.h) on operands on which every
arithmetic mode is exact — small integers stored as fp32 — against a float64 reference with torch.equal.  No tolerance: one missed,
doubled or misaddressed contribution changes an integer.

One item per class, the class as its id.  Every launch of an item
  * is asserted, through the route query, to BE in the class before it is made,
  * finds `out` / `gW` / the statistics table prefilled with NaN and the cached workspace with 0xFF bytes (NaN), so that a row, tile
    or slab nobody writes shows as NaN instead of the previous launch's plausible numbers,
  * goes through the C ABI: fc_conv_fwd (dense tables, tables in a row order of the test's choosing through fc_permute_nbr, table-free
    GEMMs), fc_conv_fwd_pairs_tiles (live_tiles 0 and exact), their *_stats and *_bn_bwd_stats twins, fc_stem_conv_fwd, fc_conv_wgrad,
    fc_conv_wgrad_pairs, fc_stem_conv_wgrad; weight images from Fn._x6_image, FC_CONV_WT operands as a transposed copy.
A dense-table class runs every case a second time through out_index where the route query puts that call in the same class.  A
linear pair-list class has no case without a pair: live_tiles = 0 IS the 3-D launch, which its sibling class runs (conv_cases.cases).
A class with a statistics epilogue runs its statistics cases a third time through the BACKWARD form of that epilogue (the two
reductions of a BatchNorm backward pass: column sums of g' = (g + add) act'(.) and of g' xhat), on inputs on which every term is a
multiple of 1/4 (conv_cases, "the backward form of the statistics epilogue"): `out` still equals the plain reference, every entry of
the table is finite and a multiple of 1/4, and the column totals of both planes equal the float64 reference.  Four further items
chain the table into fc_bn_train_bwd(part = ...), one per producer of it (the tile epilogues of k_conv_x6 and k_conv_h3r,
k_sum_parts_stats, k_sum_pairs_stats).
A further item runs the Python layer (KernelMap + Fn.sparse_conv + autograd) on injective tables.
References are computed once per (shape, table, operands) and shared by the classes that launch them; the file's 302 items take
11.1 s on an MI355X (9.4 s for the 298 items before the backward form).  DESIGN.md section 5, "Exact-integer route tests"."""
import functools

import numpy as np
import pytest
import torch

import fcaf3d_amd.functional as Fn
from fcaf3d_amd import _lib as L
from tests import conv_cases as CC

pytestmark = pytest.mark.gpu
E = CC.E
SWEPT = CC.sweep()
PARAMS = [pytest.param(d, cls, id=f'{d}-{CC.class_id(d, cls)}') for d in (CC.FWD, CC.WGRAD) for cls in SWEPT[d]]
NAN = float('nan')


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


# ---- inputs and references, shared between the classes that launch the same shape --------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _operands(n_in, n_out, K, Cin, Cout, variant):
    return tuple(torch.from_numpy(np.array(a)).to(_dev()) for a in CC.operands(n_in, n_out, K, Cin, Cout, variant))


@functools.lru_cache(maxsize=256)
def _table(name, K, n_in, n_out, tile, S):
    return torch.from_numpy(np.array(CC.make_table(name, K, n_in, n_out, tile, S))).to(_dev())


@functools.lru_cache(maxsize=256)
def _pairs(name, K, n_in, n_out, tile, S):
    """fc_kernel_map_pairs of a table -> (pair_in, pair_out, pair_pos, cnt), the unused tail of every list at -1"""
    nbr, dev = _table(name, K, n_in, n_out, tile, S), _dev()
    pi, po, pos = (torch.full_like(nbr, -1) for _ in range(3))
    cnt = torch.full((K,), -1, dtype=torch.int32, device=dev)
    ws = L.workspace(L.query('fc_kernel_map_pairs_ws_bytes', n_out, K), dev)
    L.call('fc_kernel_map_pairs', L.ptr(nbr), n_out, K, L.ptr(pi), L.ptr(po), L.ptr(pos), L.ptr(cnt), L.ptr(ws), ws.numel(), L.stream())
    assert cnt.cpu().tolist() == np.count_nonzero(CC.make_table(name, K, n_in, n_out, tile, S) >= 0, axis=1).tolist()
    return pi, po, pos, cnt


@functools.lru_cache(maxsize=256)
def _sorted(name, K, n_in, n_out, tile, S):
    """the table in a row order of the test's own choosing (a seeded permutation) through fc_permute_nbr -> (table, order)"""
    nbr, dev = _table(name, K, n_in, n_out, tile, S), _dev()
    order = torch.from_numpy(CC.sorted_order(n_out)).to(dev)
    tab = torch.full_like(nbr, -1)
    L.call('fc_permute_nbr', L.ptr(nbr), L.ptr(order), n_out, K, L.ptr(tab), L.stream())
    return tab, order


@functools.lru_cache(maxsize=1024)
def _ref(what, n_in, n_out, K, Cin, Cout, variant, name, tile, S):
    """the exact reference of one launch ('y', 'gw', 'col') on the device"""
    x, w, go = CC.operands(n_in, n_out, K, Cin, Cout, variant)
    nbr = None if name == 'identity' else CC.make_table(name, K, n_in, n_out, tile, S)
    r = CC.ref_fwd(x, w, nbr) if what == 'y' else CC.ref_wgrad(x, go, nbr, K) if what == 'gw' else CC.ref_stem_col(x, nbr)
    return r.to(_dev())


@functools.lru_cache(maxsize=512)
def _bn(n_in, n_out, K, Cin, Cout, name, tile, S, variant):
    """the epilogue inputs of a backward-epilogue case on the device (None where the option combination passes none) and the float64
    column totals of both planes -> (combo, bn_x, mean, var, gamma, beta, add, bn_y, totals (2, Cout))"""
    bc = CC.bn_case(n_in, n_out, K, Cin, Cout, name, tile, S, variant)
    f = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())
    assert CC.bn_cap(bc) < 1.0, 'backward-epilogue reference leaves the exact multiples of 1/4'
    return (bc.combo, f(bc.x), f(bc.mean), f(bc.var), f(bc.gamma if bc.combo.affine else None), f(bc.beta if bc.combo.affine else None),
            f(bc.add), f(bc.y), torch.from_numpy(CC.bn_sums(bc)).to(_dev()))


def _poisoned_workspace(nbytes):
    ws = L.workspace(max(int(nbytes), 16), _dev())
    ws.fill_(255)                                  # the WHOLE cached buffer: 0xFFFFFFFF is a NaN
    return ws


def _diff(got, ref):
    """'' if bit-equal integers, else what differs"""
    if torch.equal(got, ref):
        return ''
    bad = (got != ref) | torch.isnan(got)
    rows = bad.reshape(bad.shape[0], -1).any(1).nonzero().flatten()
    return (f'{int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN), first dim indices '
            f'{rows[:6].tolist()}{"..." if len(rows) > 6 else ""} of {bad.shape[0]}')


def _weight_operand(w, flags):
    if (flags & Fn.CONV_SPLIT) and (flags & Fn.CONV_IMAGE) and w.shape[1] % 32 == 0 and w.shape[2] % 64 == 0:
        return Fn._x6_image(w, False)              # built under the current split mode
    if flags & Fn.CONV_WT:
        return w.transpose(1, 2).contiguous()      # W[k] stored (Cout, Cin)
    return w


def _check_stats(tab, ref, what):
    r64 = ref.double()
    s1, s2 = r64.sum(0), (r64 * r64).sum(0)
    assert float(r64.abs().sum(0).max()) < CC.EXACT and float(s2.max()) < CC.EXACT, 'statistics reference leaves the exact fp32 integers'
    if not bool(torch.isfinite(tab).all()):
        return f'{what}: statistics table has {int((~torch.isfinite(tab)).sum())} non-finite entries'
    if not torch.equal(tab, tab.round()):
        return f'{what}: statistics table holds non-integers'
    t = tab.double().sum(0)
    if not (torch.equal(t[0], s1) and torch.equal(t[1], s2)):
        return f'{what}: column sums differ (sum {int((t[0] != s1).sum())}, squares {int((t[1] != s2).sum())} of {s1.numel()} columns)'
    return ''


def _check_bn_stats(tab, want, what):
    """the backward form: every entry finite and a multiple of 1/4, the column totals of both planes equal to the float64 reference"""
    if not bool(torch.isfinite(tab).all()):
        return f'{what}: statistics table has {int((~torch.isfinite(tab)).sum())} non-finite entries'
    if not torch.equal(tab * 4, (tab * 4).round()):
        return f'{what}: statistics table holds entries that are no multiple of 1/4'
    t = tab.double().sum(0)
    if not torch.equal(t, want):
        return (f"{what}: column sums differ (g' {int((t[0] != want[0]).sum())}, g' xhat {int((t[1] != want[1]).sum())} of {want.shape[1]} "
                f'columns)')
    return ''


def _run_fwd(cls, rep, case, tile, S, keep=None):
    """-> list of failure texts of one case (every launch kind the class has for it); keep: a list that takes (kind, out, table, row
    blocks) of every launch"""
    dev, K, Cin, Cout, flags = _dev(), rep.K, rep.Cin, rep.Cout, rep.flags
    n_in, n_out = case.n_in, case.n_out
    key = (case.table, K, n_in, n_out, tile, S)
    opv = CC.operand_variant(case.variant)
    x, w, _ = _operands(n_in, n_out, K, Cin, Cout, opv)
    ref = _ref('y', n_in, n_out, K, Cin, Cout, opv, case.table, tile, S)
    wop = _weight_operand(w, flags)
    bn = _bn(n_in, n_out, K, Cin, Cout, case.table, tile, S, case.variant) if CC.is_bn(case.variant) else None
    stats = case.variant == 'stats' or bn is not None
    bn_tail = ()
    if bn is not None:                             # (stats, bn_x, mean, var, gamma, beta, eps = 0, act, add, bn_y)
        bn_tail = (*(L.ptr(a) for a in bn[1:6]), 0.0, bn[0].act, L.ptr(bn[6]), L.ptr(bn[7]))
    kinds = [rep.kind]
    if rep.kind == 'dense' and CC.fast_class(CC.FWD, n_in, n_out, K, Cin, Cout, flags, 'sorted', 0, stats) == cls:
        kinds.append('sorted')                     # the same class through out_index
    fails = []
    for kind in kinds:
        pairs = kind.startswith('pairs')
        live = CC.live_tiles_of(CC.make_table(*key)) if kind == 'pairs_linear' else 0
        rc, r = CC.route_fields(CC.FWD, n_in, n_out, K, Cin, Cout, flags, kind, live, stats)
        got_cls = CC.route_class(CC.FWD, n_in, n_out, K, Cin, Cout, flags, kind, live, stats)
        assert rc == 0 and got_cls == cls, f'{case} {kind}: the call left its class: {got_cls}'
        what = f'{case} {kind} live_tiles={live}'
        nbr = oidx = lists = None
        if pairs:
            lists = _pairs(*key)
        elif kind == 'sorted':
            nbr, oidx = _sorted(*key)
        elif kind == 'dense':
            nbr = _table(*key)
        tab = None
        if stats:
            nb = L.query('fc_conv_stats_blocks', n_out, K, Cin, Cout, flags, 1 if pairs else 0)
            assert nb > 0, what
            tab = torch.full((nb, 2, Cout), NAN, device=dev)
        out = torch.full((n_out, Cout), NAN, device=dev)
        ws = _poisoned_workspace(r['s'] * n_out * Cout * 4 if (pairs or r['s'] > 1) else 0)
        if pairs:
            pi, _, pos, cnt = lists
            head = (L.ptr(x), L.ptr(wop), L.ptr(pi), L.ptr(cnt), L.ptr(pos), L.ptr(out), n_in, n_out, K, Cin, Cout, live, flags,
                    L.ptr(ws), ws.numel())
            if bn is not None:
                L.call('fc_conv_fwd_pairs_tiles_bn_bwd_stats', *head, L.ptr(tab), *bn_tail, L.stream())
            elif stats:
                L.call('fc_conv_fwd_pairs_tiles_stats', *head, L.ptr(tab), L.stream())
            else:
                L.call('fc_conv_fwd_pairs_tiles', *head, L.stream())
        else:
            head = (L.ptr(x), L.ptr(wop), L.ptr(nbr), L.ptr(oidx), L.ptr(out), n_in, n_out, K, Cin, Cout, flags, L.ptr(ws), ws.numel())
            if bn is not None:
                L.call('fc_conv_fwd_bn_bwd_stats', *head, L.ptr(tab), *bn_tail, L.stream())
            elif stats:
                L.call('fc_conv_fwd_stats', *head, L.ptr(tab), L.stream())
            else:
                L.call('fc_conv_fwd', *head, L.stream())
        if keep is not None:
            keep.append((kind, out, tab, nb if stats else 0))
        d = _diff(out, ref)
        if d:
            fails.append(f'{what}: {d}')
        if stats:
            d = _check_bn_stats(tab, bn[8], what) if bn is not None else _check_stats(tab, ref, what)
            if d:
                fails.append(d)
    if cls.family == E['FC_FAM_STEM'] and not stats:
        # the training-mode twin of the stem launch: the same rows, and the gathered inputs saved for the weight gradient
        for with_col in (False, True):
            out = torch.full((n_out, Cout), NAN, device=dev)
            col = torch.full((n_out, 84), NAN, device=dev) if with_col else None
            L.call('fc_stem_conv_fwd', L.ptr(x), L.ptr(w), L.ptr(_table(*key)), L.ptr(out), L.ptr(col), n_in, n_out, K, L.stream())
            d = _diff(out, ref)
            if with_col and not d:
                d = _diff(col, _ref('col', n_in, n_out, K, Cin, Cout, case.variant, case.table, tile, S))
            if d:
                fails.append(f'{case} fc_stem_conv_fwd col={with_col}: {d}')
    return fails


def _run_wgrad(cls, rep, case, tile, S):
    dev, K, Cin, Cout, flags, kind = _dev(), rep.K, rep.Cin, rep.Cout, rep.flags, rep.kind
    n_in, n_out = case.n_in, case.n_out
    key = (case.table, K, n_in, n_out, tile, S)
    x, _, go = _operands(n_in, n_out, K, Cin, Cout, case.variant)
    ref = _ref('gw', n_in, n_out, K, Cin, Cout, case.variant, case.table, tile, S)
    rc, r = CC.route_fields(CC.WGRAD, n_in, n_out, K, Cin, Cout, flags, kind)
    got_cls = CC.route_class(CC.WGRAD, n_in, n_out, K, Cin, Cout, flags, kind)
    assert rc == 0 and got_cls == cls, f'{case}: the call left its class: {got_cls}'
    gw = torch.full((K, Cin, Cout), NAN, device=dev)
    ws = _poisoned_workspace(max(r['s'] * K * Cin * Cout * 4, L.query('fc_conv_wgrad_ws_bytes', n_out, K, Cin, Cout, flags)))
    if kind == 'pairs':
        pi, po, _, cnt = _pairs(*key)
        L.call('fc_conv_wgrad_pairs', L.ptr(x), L.ptr(go), L.ptr(pi), L.ptr(po), L.ptr(cnt), L.ptr(gw), n_in, n_out, K, Cin, Cout, flags,
               L.ptr(ws), ws.numel(), L.stream())
    else:
        nbr = _table(*key) if kind == 'dense' else None
        L.call('fc_conv_wgrad', L.ptr(x), L.ptr(go), L.ptr(nbr), None, L.ptr(gw), n_in, n_out, K, Cin, Cout, flags, L.ptr(ws), ws.numel(),
               L.stream())
    fails = []
    d = _diff(gw, ref)
    if d:
        fails.append(f'{case}: {d}')
    if cls.family == E['FC_WFAM_STEM']:
        # ... and the stem's training route: the weight gradient streamed from the forward's saved gathered inputs
        out = torch.full((n_out, Cout), NAN, device=dev)
        col = torch.full((n_out, 84), NAN, device=dev)
        w = _operands(n_in, n_out, K, Cin, Cout, case.variant)[1]
        L.call('fc_stem_conv_fwd', L.ptr(x), L.ptr(w), L.ptr(_table(*key)), L.ptr(out), L.ptr(col), n_in, n_out, K, L.stream())
        gw = torch.full((K, Cin, Cout), NAN, device=dev)
        ws = _poisoned_workspace(L.query('fc_stem_conv_wgrad_ws_bytes', n_out, K))
        L.call('fc_stem_conv_wgrad', L.ptr(col), L.ptr(go), L.ptr(gw), n_out, K, L.ptr(ws), ws.numel(), L.stream())
        d = _diff(gw, ref)
        if d:
            fails.append(f'{case} fc_stem_conv_wgrad: {d}')
    return fails


def _stop_after_a_gpu_fault(e):
    """a HIP error leaves the process without a usable device: nothing more is launched from this session"""
    text = str(e)
    if 'hipError' in text or 'HIP error' in text or 'illegal memory access' in text:
        pytest.exit(f'GPU fault, no further launches: {text[:300]}', returncode=3)


@pytest.mark.parametrize('direction,cls', PARAMS)
def test_route_class_is_exact_on_integer_operands(direction, cls):
    rep = SWEPT[direction][cls]
    fails, launched, case_list = [], 0, []
    try:
        CC.set_env(rep.env)
        tile, S = CC.tile_of(direction, rep)
        case_list = CC.cases(direction, cls, rep)
        assert len({c.n_out for c in case_list}) >= 2 and CC.required_tables(direction, rep) <= {c.table for c in case_list}
        for case in case_list:
            fails += (_run_fwd if direction == CC.FWD else _run_wgrad)(cls, rep, case, tile, S)
            launched += 1
    except RuntimeError as e:
        _stop_after_a_gpu_fault(e)
        raise
    finally:
        CC.set_env(CC.ENV_DEFAULT)
    print(f'{rep}: {launched} cases, rows {sorted({c.n_out for c in case_list})}')
    assert not fails, f'{rep}: {len(fails)} of {launched} cases are not exact:\n' + '\n'.join(fails[:40])


@pytest.mark.parametrize('x6', [True, False], ids=['split', 'fp32'])
def test_python_layer_is_exact_on_integer_operands(x6):
    """KernelMap + Fn.sparse_conv + autograd on injective (`perm`) tables: out_index of the mask-sorted tables, nbr_t, pairs_t and the
    image of the transposed operator, with sort_rows / use_pairs in all four combinations, at three row counts (square, strided,
    generative shape)"""
    from fcaf3d_amd.sparse import KernelMap
    dev, K, Cin, Cout = _dev(), 27, 64, 128
    fails = []
    x6_0 = Fn.X6
    try:
        Fn.X6 = x6
        for n_out, n_in in ((129, 129), (300, 603), (1000, 126)):
            key = ('perm', K, n_in, n_out, 128, 27)
            nbr_np = CC.make_table(*key)
            x, w, go = _operands(n_in, n_out, K, Cin, Cout, 'int')
            want = (CC.ref_fwd(*CC.operands(n_in, n_out, K, Cin, Cout, 'int')[:2], nbr_np).to(dev),
                    CC.ref_dgrad(CC.operands(n_in, n_out, K, Cin, Cout, 'int')[2], CC.operands(n_in, n_out, K, Cin, Cout, 'int')[1], nbr_np, n_in).to(dev),
                    _ref('gw', n_in, n_out, K, Cin, Cout, 'int', 'perm', 128, 27))
            for sort_rows in (False, True):
                for use_pairs in (False, True):
                    km = KernelMap(_table(*key).clone(), n_in, n_out)
                    km.sort_rows, km.use_pairs = sort_rows, use_pairs
                    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
                    _poisoned_workspace(0)
                    y = Fn.sparse_conv(xg, wg, km, n_out)
                    gx, gw = torch.autograd.grad(y, [xg, wg], go)
                    for name, got, ref in zip(('y', 'gx', 'gW'), (y.detach(), gx, gw), want):
                        d = _diff(got, ref)
                        if d:
                            fails.append(f'n_out={n_out} n_in={n_in} sort_rows={sort_rows} use_pairs={use_pairs} {name}: {d}')
    except RuntimeError as e:
        _stop_after_a_gpu_fault(e)
        raise
    finally:
        Fn.X6 = x6_0
    assert not fails, '\n'.join(fails)


# ---- producer and consumer of the table: the convolution epilogue into fc_bn_train_bwd(part = ...) -----------------------------------------
CHAIN_ROWS = (4096, 1024, 256, 128)
_FAMILY = lambda c: CC.class_id(CC.FWD, c).split('-')[0]
CHAIN_KINDS = {
    'x6_tile_epilogue': lambda c, r: _FAMILY(c) == 'x6' and c.epi == E['FC_EPI_KERNEL'] and r.kind == 'dense',
    'h3r_tile_epilogue': lambda c, r: _FAMILY(c) == 'h3r' and c.epi == E['FC_EPI_KERNEL'] and r.kind == 'dense',
    'k_sum_parts_stats': lambda c, r: c.epi == E['FC_EPI_SUM'] and r.kind == 'dense',
    'k_sum_pairs_stats': lambda c, r: c.epi == E['FC_EPI_SUM'] and r.kind == 'pairs',
}


def _chain_pick(kind_id):
    """the first class of the epilogue kind that keeps a power-of-two row count of CHAIN_ROWS (the largest: the longest table), by the
    route query -> (class, representative, rows)"""
    for cls, rep in SWEPT[CC.FWD].items():
        if CHAIN_KINDS[kind_id](cls, rep):
            CC.set_env(rep.env)
            for n in CHAIN_ROWS:
                if CC.route_class(CC.FWD, n, n, rep.K, rep.Cin, rep.Cout, rep.flags, rep.kind, 0, True) == cls:
                    return cls, rep, n
    raise AssertionError(f'no class of {kind_id} keeps a row count of {CHAIN_ROWS}')


@pytest.mark.parametrize('kind_id', list(CHAIN_KINDS))
def test_backward_epilogue_table_feeds_the_batchnorm_backward(kind_id):
    """the one place that holds producer and consumer to the same layout and entry count: the table a backward-data launch leaves
    (ReLU with the layer's output given, and recomputed; `add` passed) goes to fc_bn_train_bwd(part = table, nb_part =
    fc_conv_stats_blocks(...)) with gy = out and gy2 = add.  gx, gres and the sums against the float64 backward reference of
    tests/norm_cases.py at a power-of-two row count: torch.equal where norm_cases declares the quantity exact there (the sums and
    gres: integers; gx: where gx_premise holds), its REL_SCALE bound otherwise."""
    from tests import norm_cases as NC
    dev, fails = _dev(), []
    try:
        cls, rep, n = _chain_pick(kind_id)
        tile, S = CC.tile_of(CC.FWD, rep)
        C = rep.Cout
        for variant in (CC.bn_variant(3), CC.bn_variant(8)):          # (ReLU, add, bn_y), (ReLU, add, recomputed)
            combo = CC.bn_combo(variant)
            assert combo.act == CC.RELU and combo.add and combo.affine
            case = CC.Case(n, n, 'full', variant)
            keep = []
            fails += _run_fwd(cls, rep, case, tile, S, keep)
            kind, out, tab, nb = keep[0]
            assert kind == rep.kind and nb == L.query('fc_conv_stats_blocks', n, rep.K, rep.Cin, C, rep.flags, 1 if kind == 'pairs' else 0)
            bc = CC.bn_case(n, n, rep.K, rep.Cin, C, 'full', tile, S, variant)
            _, bn_x, mean, var, gamma, beta, add, bn_y, _ = _bn(n, n, rep.K, rep.Cin, C, 'full', tile, S, variant)
            # the reference: NC.ref_bwd on the incoming gradient g + add; with bn_y = relu(pre + res), act'(pre + res) IS bn_y > 0
            r = NC.ref_bwd(bc.x, bc.g + bc.add, bc.mean[None], bc.var[None], bc.gamma, bc.beta, NC.RELU, np.zeros(n, np.int64), 1, [n],
                           bc.res if combo.y == 'y' else None)
            assert NC.is_pow2(n) and np.abs(r['gres']).sum(0).max() < NC.EXACT and np.abs(r['gres'] * r['xh']).sum(0).max() < NC.EXACT
            bound = {'sums': 0, 'gres': 0, 'gx': 0 if NC.gx_premise(r, np.zeros(n, np.int64), [n]) else NC.REL_SCALE}
            gx, gres, sums = (torch.full((n, C), NAN, device=dev), torch.full((n, C), NAN, device=dev), torch.full((1, 2, C), NAN, device=dev))
            cnt = torch.full((1,), float(n), device=dev)
            ws = _poisoned_workspace(L.query('fc_bn_train_ws_bytes', n, C))
            L.call('fc_bn_train_bwd', L.ptr(bn_x), L.ptr(bn_y), L.ptr(out), L.ptr(add), n, C, L.ptr(mean), L.ptr(var), L.ptr(cnt), 0.0,
                   L.ptr(gamma), L.ptr(beta), combo.act, L.ptr(gx), L.ptr(gres), L.ptr(sums), L.ptr(tab), nb, Fn.BN_SMALL_ELEMS, L.ptr(ws),
                   ws.numel(), L.stream())
            for name, got in (('sums', sums), ('gres', gres), ('gx', gx)):
                g64 = got.double().cpu().numpy().reshape(r[name].shape)
                err = float(np.abs(g64 - r[name]).max()) if np.isfinite(g64).all() else float('inf')
                print(f'{kind_id} n={n} {variant} {name}: bound {bound[name]:g}, max-abs error {err:.3e} of scale {np.abs(r[name]).max():.3e}')
                if not np.isfinite(g64).all() or NC.differs(g64, r[name], bound[name]):
                    fails.append(f'{rep} n={n} {variant} fc_bn_train_bwd {name}: bound {bound[name]:g}, max-abs error {err:.3e} of scale '
                                 f'{np.abs(r[name]).max():.3e}, {int((~np.isfinite(g64)).sum())} non-finite')
    except RuntimeError as e:
        _stop_after_a_gpu_fault(e)
        raise
    finally:
        CC.set_env(CC.ENV_DEFAULT)
    assert not fails, '\n'.join(fails)
