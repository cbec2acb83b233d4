"""What tests/test_gpu_coords_exact.py and tests/test_gpu_plan_exact.py share: both coordinate phases leave the same object graph
(sparse.CoordMap / sparse.KernelMap), so one walk compares either with the numpy references of tests/coord_cases.py.  Every comparison
is torch.equal / np.array_equal on integers (or copied floats); nothing here has a tolerance."""
import contextlib

import numpy as np
import torch

from fcaf3d_amd import _lib as L
from fcaf3d_amd import sparse as SP
from tests import coord_cases as CC


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def npy(t):
    return t.detach().cpu().numpy()


def eq(got, want, what):
    got = npy(got) if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want.astype(got.dtype)), what


@contextlib.contextmanager
def thresholds(sort_min, pair_rows):
    """sparse.SORT_MIN_ROWS / PAIR_CONV_ROWS for the duration: both table kinds on small sets"""
    saved = SP.SORT_MIN_ROWS, SP.PAIR_CONV_ROWS
    SP.SORT_MIN_ROWS, SP.PAIR_CONV_ROWS = sort_min, pair_rows
    try:
        yield
    finally:
        SP.SORT_MIN_ROWS, SP.PAIR_CONV_ROWS = saved


def lookup_all(cm, q):
    """row of every query voxel through the set's hash: fc_kernel_map with one zero offset, into a buffer of sentinels"""
    q = q.contiguous()
    nbr = torch.full((1, q.shape[0]), CC.SENT, dtype=torch.int32, device=q.device)
    offs = torch.zeros((1, 3), dtype=torch.int32, device=q.device)
    L.call('fc_kernel_map', L.ptr(q), q.shape[0], L.ptr(cm.keys), L.ptr(cm.vals), cm.cap, L.ptr(offs), 1, L.ptr(nbr), L.stream())
    return nbr[0]


def check_table(cm, coords, cap, what):
    """the voxel hash of a set, read back: capacity, one slot per voxel whose value is the voxel's row and whose key is fc_pack of that
    row (numpy's), every key on the probe path from its numpy-computed home slot; then the lookups: members -> their row, the same
    voxels in a scene the batch does not have -> -1"""
    keys = npy(cm.keys).view(np.uint64)
    vals = npy(cm.vals)
    assert len(keys) == len(vals) == cap == cm.cap, (what, len(keys), cap)
    occ = np.nonzero(keys != CC.EMPTY)[0]
    assert len(occ) == len(coords), what
    assert sorted(vals[occ].tolist()) == list(range(len(coords))), what
    assert np.array_equal(keys[occ], CC.fc_pack(coords[vals[occ]])), what
    assert CC.probe_path_ok(keys), what
    if len(coords):
        d = cm.coords.device
        eq(lookup_all(cm, torch.from_numpy(np.ascontiguousarray(coords)).to(d)), np.arange(len(coords)), what + ' lookup')
        far = coords.copy()
        far[:, 0] += 400
        eq(lookup_all(cm, torch.from_numpy(far).to(d)), np.full(len(coords), -1), what + ' absent')
    return keys, vals


def pairs_direct(tab):
    """fc_kernel_map_pairs into buffers of sentinels -> (pair_in, pair_out, pos, cnt) as numpy"""
    K, n = tab.shape
    d = tab.device
    pi, po, pos = (torch.full((K, n), CC.SENT, dtype=torch.int32, device=d) for _ in range(3))
    cnt = torch.full((K,), CC.SENT, dtype=torch.int32, device=d)
    ws = L.workspace(L.query('fc_kernel_map_pairs_ws_bytes', n, K), d)
    L.call('fc_kernel_map_pairs', L.ptr(tab), n, K, L.ptr(pi), L.ptr(po), L.ptr(pos), L.ptr(cnt), L.ptr(ws), ws.numel(), L.stream())
    return npy(pi), npy(po), npy(pos), npy(cnt)


def check_pairs(got, want, what):
    """pair lists up to their counts (what lies behind a list belongs to nobody), positions and counts in full"""
    (pi, po, pos, cnt), (wi, wo, wpos, wcnt) = [npy(t) for t in got], want
    eq(cnt, wcnt, what + ' cnt')
    eq(pos, wpos, what + ' pos')
    for k, c in enumerate(wcnt.tolist()):
        assert np.array_equal(pi[k, :c], wi[k, :c]) and np.array_equal(po[k, :c], wo[k, :c]), f'{what} list {k}'


def _has(km, name):
    return name in km.__dict__.get('_lazy', {}) or km.__dict__.get(name) is not None


def check_map(km, nbr, n_in, what, derived, backward, planned=False, direct=False):
    """a kernel map against its numpy table.  derived: the 27-offset tables of a convolution map (nbr_t, pair lists both ways, live
    tiles, the mask-sorted tables).  planned: the map comes from the native plan, which builds, of these, what its row thresholds
    ask for — only tables the plan itself made are read (an accessor would build a missing one with the per-operator kernels).
    direct: the per-operator entry points once more into sentinel buffers of the test's own"""
    assert (km.K, km.n_in, km.n_out) == (nbr.shape[0], n_in, nbr.shape[1]), what
    eq(km.nbr, nbr, what + ' nbr')
    nt = CC.transpose(nbr, n_in)
    if backward and (not planned or _has(km, '_nbr_t')):
        eq(km.nbr_t, nt, what + ' nbr_t')
    if not derived or km.K != 27:
        return
    want, want_t = CC.pair_lists(nbr), CC.pair_lists(nt)
    if not planned or _has(km, '_pairs'):
        check_pairs(km.pairs(), want, what + ' pairs')
    if backward and (not planned or _has(km, '_pairs_t')):
        check_pairs(km.pairs_t(), want_t, what + ' pairs_t')
    if not planned or km.__dict__.get('_tiles') is not None:
        assert km.pair_tiles() == CC.live_tiles(want[3]), what + ' tiles'
    if backward and (not planned or km.__dict__.get('_tiles_t') is not None):
        assert km.pair_tiles(True) == CC.live_tiles(want_t[3]), what + ' tiles_t'
    if km.sort_rows and (not planned or _has(km, '_sorted')):
        tab, order = km.sorted_fwd()
        wt, wo = CC.mask_sorted(nbr)
        eq(order, wo, what + ' sorted order')
        eq(tab, wt, what + ' sorted table')
    if km.sort_rows and backward and (not planned or _has(km, '_sorted_t')):
        tab, order = km.sorted_bwd()
        wt, wo = CC.mask_sorted(nt)
        eq(order, wo, what + ' sorted_t order')
        eq(tab, wt, what + ' sorted_t table')
    if direct:
        for tab, w, nm in ((km.nbr, want, 'pairs'), (km.nbr_t, want_t, 'pairs_t')):
            pi, po, pos, cnt = pairs_direct(tab.contiguous())
            eq(cnt, w[3], f'{what} direct {nm} cnt')
            eq(pos, w[2], f'{what} direct {nm} pos')
            eq(pi, w[0], f'{what} direct {nm} in (sentinels behind the lists)')
            eq(po, w[1], f'{what} direct {nm} out (sentinels behind the lists)')
        t = torch.full((km.K, n_in), CC.SENT, dtype=torch.int32, device=km.nbr.device)
        L.call('fc_kernel_map_transpose', L.ptr(km.nbr), km.n_out, n_in, km.K, L.ptr(t), L.stream())
        eq(t, nt, what + ' direct transpose')
        m = torch.full((km.n_out,), CC.SENT, dtype=torch.int32, device=km.nbr.device)
        L.call('fc_nbr_row_masks', L.ptr(km.nbr), km.n_out, km.K, L.ptr(m), L.stream())
        eq(m, CC.row_masks(nbr), what + ' direct masks')


def walk_sets(cm0, nl):
    sets = [cm0]
    for _ in range(2 + nl):
        sets.append(sets[-1].strided(2))
    return sets


def check_graph(name, cm0, backward=True, planned=False, direct=False, tables=True):
    """the whole graph under the level-0 set cm0 against coord_cases.expected(name)"""
    c = CC.case_of(name)
    ex = CC.expected(name)
    nl = c.nl
    sets = walk_sets(cm0, nl)
    for s, (cm, st) in enumerate(zip(sets, ex['sets'])):
        assert (cm.n, cm.stride, cm.batch_size) == (len(st.coords), 1 << s, c.B), (s, cm.n, len(st.coords))
        eq(cm.coords, st.coords, f'set {s}')
        assert list(cm.scene_counts) == ex['rows_per_scene'][s].tolist(), s
        if tables:
            check_table(cm, st.coords, ex['caps'][s], f'table {s}')
    for mname, (i, o, ks, nbr) in ex['maps'].items():
        km = sets[i].kernel_map(sets[o], ks)
        conv = mname not in ('stem', 'pool')
        check_map(km, nbr, sets[i].n, mname, derived=conv or not planned, backward=backward and (conv or not planned), planned=planned, direct=direct)
    par = sets[-1]
    for gi, g in enumerate(ex['gen']):
        gm = par.generate()
        assert (gm.n, gm.stride) == (len(g['coords']), g['stride'])
        eq(gm.coords, g['coords'], f'generated set {gi}')
        check_map(gm.kernel_map(gm, 3), g['nbr'], gm.n, f'gsame {gi}', derived=True, backward=backward, planned=planned)
        u, rows, swapped = sets[g['level']].union(gm)
        assert swapped and u is gm, f'union {gi}'
        eq(rows, g['rows'], f'union rows {gi}')
        par = gm
    torch.cuda.synchronize()
    return sets
