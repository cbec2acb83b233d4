"""-m gpu: every convolution route class (tests/conv_cases.py: the census of csrc/conv_route.h) on operands on which every
arithmetic mode is exact — small integers stored as fp32 — against a float64 reference with torch.equal.  No tolerance: one missed,
doubled or misaddressed contribution changes an integer.

One item per class, the class as its id.  Every launch of an item
  * is asserted, through the route query, to BE in the class before it is made,
  * finds `out` / `gW` / the statistics table prefilled with NaN and the cached workspace with 0xFF bytes (NaN), so that a row, tile
    or slab nobody writes shows as NaN instead of the previous launch's plausible numbers,
  * goes through the C ABI: fc_conv_fwd (dense tables, tables in a row order of the test's choosing through fc_permute_nbr, table-free
    GEMMs), fc_conv_fwd_pairs_tiles (live_tiles 0 and exact), their *_stats twins, fc_stem_conv_fwd, fc_conv_wgrad,
    fc_conv_wgrad_pairs, fc_stem_conv_wgrad; weight images from Fn._x6_image, FC_CONV_WT operands as a transposed copy.
A dense-table class runs every case a second time through out_index where the route query puts that call in the same class.  A
linear pair-list class has no case without a pair: live_tiles = 0 IS the 3-D launch, which its sibling class runs (conv_cases.cases).
A further item runs the Python layer (KernelMap + Fn.sparse_conv + autograd) on injective tables.
References are computed once per (shape, table, operands) and shared by the classes that launch them; the file's 298 items take
about 12 s on an MI355X.  DESIGN.md section 5, "Exact-integer route tests"."""
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
    order = torch.from_numpy(np.random.default_rng(n_out).permutation(n_out).astype(np.int32)).to(dev)
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


def _run_fwd(cls, rep, case, tile, S):
    """-> list of failure texts of one case (every launch kind the class has for it)"""
    dev, K, Cin, Cout, flags = _dev(), rep.K, rep.Cin, rep.Cout, rep.flags
    n_in, n_out = case.n_in, case.n_out
    key = (case.table, K, n_in, n_out, tile, S)
    x, w, _ = _operands(n_in, n_out, K, Cin, Cout, case.variant)
    ref = _ref('y', n_in, n_out, K, Cin, Cout, case.variant, case.table, tile, S)
    wop = _weight_operand(w, flags)
    stats = case.variant == 'stats'
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
            if stats:
                L.call('fc_conv_fwd_pairs_tiles_stats', *head, L.ptr(tab), L.stream())
            else:
                L.call('fc_conv_fwd_pairs_tiles', *head, L.stream())
        else:
            head = (L.ptr(x), L.ptr(wop), L.ptr(nbr), L.ptr(oidx), L.ptr(out), n_in, n_out, K, Cin, Cout, flags, L.ptr(ws), ws.numel())
            if stats:
                L.call('fc_conv_fwd_stats', *head, L.ptr(tab), L.stream())
            else:
                L.call('fc_conv_fwd', *head, L.stream())
        d = _diff(out, ref)
        if d:
            fails.append(f'{what}: {d}')
        if stats:
            d = _check_stats(tab, ref, what)
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
