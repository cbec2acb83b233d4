"""No GPU: the census of normalisation route classes behind tests/test_gpu_norm_exact.py, the premise of its exact comparisons, the
weight of its marker rows and its crafted segment tables (tests/norm_cases.py; DESIGN.md section 5, "Exact-integer route tests")."""
import os

import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from tests import norm_cases as NC

CENSUS = {NC.FWD: 67, NC.BWD: 102, NC.STATS: 60}          # DESIGN.md section 5 records these


@pytest.fixture(scope='module')
def swept():
    return NC.sweep()


def test_census_gpu_case_list_covers_every_swept_class(swept):
    """the class counts are the recorded ones (a new class, or a rule of norm_route.h that moves, shows here first) and DESIGN.md states
    them; every class keeps its cases — at least two row counts unless its last block must be full —, every case answers its class
    through the route query proper (L.route) and stays within the size limit"""
    counts = {d: len(swept[d]) for d in NC.DIRECTIONS}
    launches = sum(len(NC.cases(c, r)) for d in NC.DIRECTIONS for c, r in swept[d].items())
    print(f'route classes: {counts}; {launches} GPU launches derived')
    assert counts == CENSUS
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'DESIGN.md')).read()
    assert f'{counts[NC.FWD]} forward, {counts[NC.BWD]} backward and {counts[NC.STATS]} segment-statistics classes' in design
    ids = [NC.class_id(c) for d in NC.DIRECTIONS for c in swept[d]]
    assert len(set(ids)) == len(ids)
    I = {k[len('FC_NROUTE_'):].lower(): v for k, v in NC.E.items() if k.startswith('FC_NROUTE_')}
    for d in NC.DIRECTIONS:
        for cls, rep in swept[d].items():
            cs = NC.cases(cls, rep)
            assert cs and cs[0].n == rep.n and rep.n in NC.N_LIST and rep.C in NC.C_LIST, (NC.class_id(cls), rep)
            assert len({c.n for c in cs}) >= 2 or cls.last == 'full', (NC.class_id(cls), rep)
            assert all(c.n <= NC.MAX_ROWS and c.n * rep.C <= NC.MAX_ELEMS for c in cs)
            opts = {o for c in cs for o in c.opts}
            if d == NC.FWD:
                assert {'res', 'add', 'run', 'relu', 'elu'} <= opts and any('run' not in c.opts for c in cs) or rep.n * rep.C > NC.BIG_ELEMS
            elif d == NC.BWD:
                assert ({'y', 'gres', 'relu', 'elu'} <= opts and any('y' not in c.opts for c in cs) and
                        (('gy2' in opts) == (rep.entry == 'train'))) or rep.n * rep.C > NC.BIG_ELEMS
            if cls.segs:
                assert {c.table for c in cs} == set(NC.SEG_TABLES) and {c.stride for c in cs} == {1, 4}
            for c in cs:
                assert NC.route_class(rep, c.n) == cls, (NC.class_id(cls), rep, c)
                if d != NC.STATS:          # the short way (raw out[]) against the dictionary of L.route
                    rc, r = NC.route_fields(rep, c.n)
                    o = NC._query(rep, c.n)
                    assert rc == 0 and all(r[k] == o[i] for k, i in I.items())
    # every crossed option reaches a windowed and an unwindowed class of each prologue-reducing apply kernel
    for d, apply in ((NC.FWD, 'bn2'), (NC.BWD, 'prologue')):
        for win in (False, True):
            assert any(c.apply == apply and c.windowed == win and r.n * r.C <= NC.BIG_ELEMS for c, r in swept[d].items())
    assert any(c.grouped and r.groups == 3 for c, r in swept[NC.FWD].items())


def test_restated_launch_geometry_is_the_route_s(swept):
    """row_blocks / stats_geometry as restated in tests/norm_cases.py against the route query: the two-launch backward form blocks n
    rows by row_blocks(n, 64) with stats_geometry(C) threads; the table routes by row_blocks(n, 256)"""
    for C in NC.C_LIST:
        for n in (1, 63, 64, 65, 4096, 4097, 4160, 4161, 8128, 8129, 16384, 16385, 16641):
            if n * C > NC.MAX_ELEMS:
                continue
            rc, r = L.route('fc_bn_train_bwd_route', n, C, 1, 0, 0, 0, NC.E['FC_NFORM_SMALL'])
            assert rc == 0 and (r['nb'], r['rpb']) == NC.row_blocks(n, NC.BN1_MAXB) and r['threads'] == NC.stats_geometry(C)[0]
            rc, r = L.route('fc_bn_train_fwd_route', n, C, 1, 4, 1, 0)
            assert rc == 0 and (r['nb'], r['rpb']) == NC.row_blocks(n, NC.AP_MAXB)
            g = NC.cdiv(n, 64)
            assert r['cg'] == (64 if C >= 128 and C % 64 == 0 and g * (C // 64) <= 1024 and g < 128 else C)
            assert L.query('fc_col_stats_ws_bytes', n, C, 2) == NC.row_blocks(n, NC.MAXBLOCKS)[0] * 2 * (2 * C + 1) * 4
    assert NC.stats_geometry(4) == (16, 16) and NC.stats_geometry(68) == (255, 15) and NC.stats_geometry(1020) == (255, 1)
    assert NC.stats_geometry(1024) == (256, 1) and NC.stats_geometry(192)[1] == 5


def test_representatives_sit_where_the_rules_of_norm_route_h_put_them(swept):
    """a moved rule moves these: the window rule's switch at 128 row groups, the prologue caps, the finalise kernels' unrolled loops"""
    by_id = {NC.class_id(c): r for d in NC.DIRECTIONS for c, r in swept[d].items()}
    at = lambda **kw: sorted((r.n, r.C) for i, r in by_id.items() if all(f'-{v}-' in f'-{i}-' for v in kw.values()))
    # the first unwindowed 128-channel launch of k_bn2_apply with a short last block: 8 129 rows (g = 128)
    assert (8129, 128) in at(a='bn2', b='all', c='short', d='nrlmid') and (8192, 128) in at(a='bn2', b='all', c='full', d='nrlmid')
    # 1 024 channels stay windowed up to 4 096 rows (g * 16 <= 1 024)
    assert (4097, 1024) in at(a='bn2', b='all', c='nrl1') and min(at(a='bn2', b='win')) == (1, 128)
    # k_bn_finalize: 16 slices, unrolled from 49 blocks; k_stats_final / k_bn2_finalize: 64 slices, unrolled from 193 entries
    assert min(at(a='bn_finalize', b='tail'))[0] == 16 * 64 + 1 and min(at(a='bn_finalize', b='unrolled'))[0] == 48 * 64 + 1
    assert min(at(a='seg', b='stats_final', c='tail'))[0] == 64 * 64 + 1 and min(at(a='seg', b='stats_final', c='unrolled'))[0] == 192 * 64 + 1
    assert {r.nb_part * r.groups for i, r in by_id.items() if '-bn2_finalize-' in i} == {65, 193, 195}
    # bn1_reduce_parts reads past the L1 up to 32 KB of table: 4 blocks of 1 024 channels, not 5
    assert min(at(a='bn1', b='l1', c='nrl1-wave'))[0] == 257


def _orders(a):
    """the column sums of a (rows, C) float64 matrix of integers, reduced in fp32 front to back and back to front"""
    a32 = a.astype(np.float32)
    return np.cumsum(a32, 0, dtype=np.float32)[-1], np.cumsum(a32[::-1], 0, dtype=np.float32)[-1]


def _sensitive(rep, case, inp, exp, bnd, rows):
    """every UNIT a kernel of the call adds up — a marker row, or behind a table of sums an entry of the table (all of them: the
    first, the last, both sides of every slice and unroll edge) — dropped from the reduction or counted twice, moves a compared
    output by more than 100 x its bound (an output held to equality: makes it unequal) -> the units that do not.
    The forward statistics are modelled as the kernels form them: from the table's entries, or from the sums of x - x[0] (row 0
    itself adds nothing to those and is no unit there); the divisor stays n."""
    d, n, C = NC.direction_of(rep.entry), case.n, rep.C
    K = np.array(rows)
    table = None
    if 'part' in inp:
        table = inp['part'].reshape(rep.nb_part, 2, -1, C).transpose(0, 2, 1, 3).reshape(-1, 2, C)          # [entry][2][C]
        assert len(table) == NC.table_entries(rep)
    bad = set()
    for sign in (-1.0, 1.0):
        if d == NC.FWD:
            x = inp['x']
            if table is not None:
                base, S1, S2, u1, u2, units = 0.0, x.sum(0), (x * x).sum(0), table[:, 0], table[:, 1], np.arange(len(table))
            else:
                sh, units = x - x[0], K[K > 0]
                base, S1, S2, u1, u2 = x[0], sh.sum(0), (sh * sh).sum(0), sh[units], sh[units] ** 2
            dm = (S1 + sign * u1) / n
            got = {'mean': base + dm, 'var': np.maximum((S2 + sign * u2) / n - dm * dm, 0.0)}
            hit = np.zeros(len(units), bool)
            for name in ('mean', 'var'):
                if bnd[name] == 0:
                    hit |= (got[name].astype(np.float32) != exp[name].astype(np.float32)).any(1)
                else:
                    hit |= np.abs(got[name] - exp[name]).max(1) > 100 * bnd[name] * np.abs(exp[name]).max()
        elif d == NC.STATS:
            units = K
            hit = (inp['x'][K] != 0).any(1)          # the column sums and (fc_col_stats: k_stats_partial counts in the same loop) the count are held to equality
        else:
            assert bnd['sums'] == 0                  # the sums are held to equality: a unit with a non-zero g' changes an integer
            if table is not None:
                units, hit = np.arange(len(table)), (table != 0).any((1, 2))
            else:
                units, hit = K, (inp['ref_gres'][K] != 0).any(1)
                if n * C <= 1 << 16:                 # ... which is what the reference itself says with the row's weight at 0 / 2 (first and last marker row)
                    for k in (K[0], K[-1]):
                        w = np.ones(n)
                        w[k] += sign
                        r = NC.ref_bwd(inp['x'], inp['gy'] + inp.get('gy2', 0.0), inp['mean'], inp['var'], inp['gamma'], inp['beta'], inp['act'],
                                       inp['seg'], rep.nseg, inp['cnt'], inp['ref_res'], w)
                        assert NC.differs(r['sums'], exp['sums'], 0) == bool((inp['ref_gres'][k] != 0).any())
        bad |= set(units[~hit].tolist())
    return sorted(bad)


@pytest.mark.parametrize('direction', NC.DIRECTIONS)
def test_premise_and_sensitivity_of_every_case(swept, direction):
    """The premise: wherever an output is held to equality the reductions behind it, carried out in fp32 in two different orders, equal
    float64 — every sum stays below 2^24.  The sensitivity: a condition on the INPUTS — each marker row weighs more than 100 bounds.
    (The ELU items are tolerance items on top of every class: their arithmetic is not integer and they are not part of either.)"""
    checked = 0
    for cls, rep in swept[direction].items():
        for case in NC.cases(cls, rep):
            if 'elu' in case.opts:
                continue
            inp, exp, bnd, rows = NC.build(rep, case)
            what = (NC.class_id(cls), case)
            if direction == NC.FWD:
                x = inp['x']
                if bnd['mean'] == 0:
                    sh = x - x[0]
                    for a, want in ((sh, sh.sum(0)), (sh * sh, (sh * sh).sum(0)), (x, x.sum(0)), (x * x, (x * x).sum(0))):
                        f, b = _orders(a)
                        assert np.array_equal(f, want) and np.array_equal(b, want), what
                    # mean = x[0] + S1 / n and var = S2 / n - (S1 / n)^2 evaluated in fp32 step by step are the float64 values
                    d32 = (sh.sum(0).astype(np.float32) * np.float32(1.0 / case.n))
                    q32 = ((sh * sh).sum(0).astype(np.float32) * np.float32(1.0 / case.n))
                    assert np.array_equal(x[0].astype(np.float32) + d32, exp['mean'].astype(np.float32)), what
                    assert np.array_equal((d32 * d32).astype(np.float64), d32.astype(np.float64) ** 2), what
                    assert np.array_equal(np.maximum(q32 - d32 * d32, np.float32(0)), exp['var'].astype(np.float32)), what
                if 'part' in inp:
                    t = inp['part'].reshape(rep.nb_part, 2, rep.groups, rep.C).sum((0, 2))
                    assert np.array_equal(t[0], x.sum(0)) and np.array_equal(t[1], (x * x).sum(0)) and np.abs(inp['part']).max() < NC.EXACT, what
                    assert np.array_equal(inp['part'], np.rint(inp['part'])) and case.n >= 2 * NC.table_entries(rep) - 1
                    assert inp['part'][:, 1].reshape(-1, rep.C).any(1).all(), what          # no entry is all zero: each has a marker row
            elif direction == NC.STATS:
                x = inp['x']
                for s in range(rep.nseg):
                    xs = x[inp['seg'] == s]
                    if len(xs):
                        for a in (xs, xs * xs):
                            f, b = _orders(a)
                            assert np.array_equal(f, a.sum(0)) and np.array_equal(b, a.sum(0)), what
            else:
                r = {'xh': inp['ref_xh'], 'pre': inp['ref_pre']}
                assert np.array_equal(r['xh'], np.rint(r['xh'])) and np.array_equal(inp['gy'], np.rint(inp['gy'])), what
                assert bnd['sums'] == 0 and np.array_equal(exp['sums'], np.rint(exp['sums'])) and np.abs(exp['sums']).max() < NC.EXACT, what
                gp = inp['ref_gres']
                if rep.nseg == 1:
                    for a, want in ((gp, exp['sums'][0, 0]), (gp * r['xh'], exp['sums'][0, 1])):
                        f, b = _orders(a)
                        assert np.array_equal(f, want) and np.array_equal(b, want), what
                if inp['act'] == NC.RELU and case.n >= 64:
                    assert (r['pre'] == 0).any(), what          # exact zeros in front of the ReLU: act'(0) = 0 is exercised
                if bnd['gx'] == 0:          # the bracket of gx in fp32, step by step, is the float64 value
                    cn = np.float32(1.0) / inp['cnt'].astype(np.float32)[inp['seg']][:, None]
                    g32, xh32 = gp.astype(np.float32), r['xh'].astype(np.float32)
                    s1, s2 = exp['sums'].astype(np.float32)[inp['seg'], 0], exp['sums'].astype(np.float32)[inp['seg'], 1]
                    a = (g32 - s1 * cn - xh32 * s2 * cn) * (inp['gamma'] / np.sqrt(inp['var'][inp['seg']])).astype(np.float32)
                    b = (g32 - s1 * cn - xh32 * (s2 * cn)) * (inp['gamma'] / np.sqrt(inp['var'][inp['seg']])).astype(np.float32)
                    assert np.array_equal(a, exp['gx'].astype(np.float32)) and np.array_equal(b, a), what
            assert set(rows) >= {0, case.n - 1}
            assert not _sensitive(rep, case, inp, exp, bnd, rows), (what, _sensitive(rep, case, inp, exp, bnd, rows)[:8])
            checked += 1
    print(f'{direction}: {checked} cases')
    assert checked


SEG_SHAPES = [(1000, 64, 64), (300, 64, 64), (200, 3, 64), (131, 64, 64), (65, 2, 64), (4161, 2, 65), (1, 64, 1), (40, 2, 64)]


@pytest.mark.parametrize('n,nseg,rpb', SEG_SHAPES)
def test_crafted_segment_tables_keep_their_promises(n, nseg, rpb):
    tabs = {k: NC.seg_table(k, n, nseg, rpb) for k in NC.SEG_TABLES}
    for k, ids in tabs.items():
        assert ids.shape == (n,) and ids.dtype == np.int32 and ids.min() >= 0 and ids.max() < nseg, k
    c = tabs['contig']
    assert (np.diff(c) >= 0).all()
    if nseg >= 4:
        for k in ('contig', 'unsorted'):
            assert not (tabs[k] == nseg // 2).any() and not (tabs[k] == nseg - 1).any()          # the empty segments are empty
        assert np.array_equal(np.bincount(tabs['unsorted'], minlength=nseg), np.bincount(c, minlength=nseg))
        assert np.array_equal(tabs['unsorted'][rpb:], c[rpb:])
    s = tabs['straddle']
    head = s[:rpb]
    if n >= 3:
        assert len(np.unique(head)) == min(3, nseg), 'the first block holds three segments'
    for b in range(1, NC.cdiv(n, rpb)):
        assert len(np.unique(s[b * rpb:(b + 1) * rpb])) == 1, 'a later block lies inside one segment'
    assert (np.diff(s) >= 0).all()
    m = NC.strided(c, 4)
    assert m.shape == (n, 4) and np.array_equal(m[:, 0], c) and (m[:, 1:] == 12345).all() and NC.strided(c, 1).shape == (n,)
    # the power-of-two table: every count a power of two or, in the two named segments, zero
    p = NC.seg_table('pow2', NC.pow2_rows(nseg), nseg, rpb)
    cnt = np.bincount(p, minlength=nseg)
    assert all(NC.is_pow2(int(v)) or (nseg >= 4 and i in (nseg // 2, nseg - 1) and v == 0) for i, v in enumerate(cnt))


def test_segment_tables_of_the_derived_cases_straddle_at_their_own_block_size(swept):
    """a 'straddle' case's first block — at the rows per block its launch really has — holds min(3, nseg) segments; an 'unsorted' one's is
    not sorted"""
    seen = 0
    for d in (NC.BWD, NC.STATS):
        for cls, rep in swept[d].items():
            if not cls.segs:
                continue
            for case in NC.cases(cls, rep):
                ids, rpb = NC.case_seg(rep, case)
                assert rpb == NC.layouts(rep, case.n)[-1][1] and ids.max() < rep.nseg
                if case.table == 'straddle' and case.n >= 3:
                    assert len(np.unique(ids[:rpb])) == min(3, rep.nseg)
                    seen += 1
    assert seen


def test_references_agree_with_autograd_and_a_brute_force_pool():
    """ref_fwd_stats / ref_fwd_y / ref_bwd against torch's float64 batch norm + autograd; ref_pool / pooled_gradient against loops"""
    n, C = 37, 8
    x, res, go = NC.int_matrix((n, C), 1) + 0.25, NC.int_matrix((n, C), 2).copy(), NC.int_matrix((n, C), 3).copy()
    gamma, beta = NC.affine(C)
    st = NC.ref_fwd_stats(x, None, 0.25, np.ones(C), np.full(C, 2.0))
    bn = torch.nn.BatchNorm1d(C, eps=1e-30, momentum=0.25).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta)); bn.running_mean.fill_(1.0); bn.running_var.fill_(2.0)
    xt, rt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(res).requires_grad_(True)
    y = torch.relu(bn(xt) + rt)
    gx, gr = torch.autograd.grad(y, [xt, rt], torch.from_numpy(go))
    assert np.allclose(st['rmean'], bn.running_mean.numpy(), rtol=1e-12) and np.allclose(st['rvar'], bn.running_var.numpy(), rtol=1e-12)
    assert np.allclose(NC.ref_fwd_y(x, st['mean'], st['var'], 0.0, gamma, beta, NC.RELU, res), y.detach().numpy(), atol=1e-12)
    seg = np.zeros(n, np.int32)
    r = NC.ref_bwd(x, go, st['mean'][None], st['var'][None], gamma, beta, NC.RELU, seg, 1, [n], res)
    assert np.allclose(r['gx'], gx.numpy(), atol=1e-10) and np.allclose(r['gres'], gr.numpy(), atol=1e-12)
    # dropped / doubled rows enter the sums 0 / 2 times, the divisor stays n
    w = np.ones(n); w[5] = 0.0; w[9] = 2.0
    assert np.allclose(NC.ref_fwd_stats(x, w)['mean'], (x.sum(0) - x[5] + x[9]) / n)
    ids = NC.seg_table('contig', 90, 5, 64)
    nbr, parent = NC.pool_table(ids, 3)
    assert sorted(nbr[nbr >= 0].tolist()) == list(range(90)) and (nbr >= 0).sum(0).min() == 0 and (nbr >= 0).sum(0).max() == 8
    yv = NC.int_matrix((90, 4), 4, amp=2)                 # (small amplitude: ties)
    out, arg = NC.ref_pool(yv, nbr)
    for o in range(nbr.shape[1]):
        kids = [int(i) for i in nbr[:, o] if i >= 0]
        assert len({ids[i] for i in kids}) <= 1 and all(parent[i] == o for i in kids)
        for c in range(4):
            best, a = 0.0, -1
            for i in kids:
                if a < 0 or yv[i, c] > best:
                    best, a = yv[i, c], i
            assert out[o, c] == best and arg[o, c] == a
    g = NC.pooled_gradient(np.ones_like(out), arg, parent)
    assert g.sum() == (arg >= 0).sum() and all(g[arg[o, c], c] == 1 for o in range(nbr.shape[1]) for c in range(4) if arg[o, c] >= 0)
