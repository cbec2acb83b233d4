"""No GPU: the census of convolution route classes behind tests/test_gpu_conv_exact.py, the premise of its exact comparison, and
its crafted tables (tests/conv_cases.py; DESIGN.md section 5, "Exact-integer route tests")."""
import numpy as np
import pytest
import torch

from oracle import x6_oracle as X
from tests import conv_cases as CC


@pytest.fixture(scope='module')
def swept():
    return CC.sweep()


def _cases_by_class(swept):
    out = {}
    try:
        for d in (CC.FWD, CC.WGRAD):
            for cls, rep in swept[d].items():
                CC.set_env(rep.env)
                out[(d, cls)] = CC.cases(d, cls, rep)
    finally:
        CC.set_env(CC.ENV_DEFAULT)
    return out


def test_census_gpu_case_list_covers_every_swept_class(swept):
    """the classes the GPU case list hits == the classes the sweep finds; every class keeps at least two row counts and its tables;
    every case answers its class through the route query proper (L.route), FC_TABLE_STATS included where the class has a
    statistics epilogue"""
    by_class = _cases_by_class(swept)
    print(f'route classes: {len(swept[CC.FWD])} forward / backward-data, {len(swept[CC.WGRAD])} weight gradient; '
          f'{sum(len(v) for v in by_class.values())} GPU launches derived')
    fam = lambda d: sorted({CC.class_id(d, c).split('-')[0] for c in swept[d]})
    assert fam(CC.FWD) == ['fma', 'glds', 'h3r', 'mfma', 'mfma_p', 'stem', 'x6']
    assert fam(CC.WGRAD) == ['fma', 'mfma', 'mfma_p', 'multi', 'stem', 'x6t']
    hit = {CC.FWD: set(), CC.WGRAD: set()}
    try:
        for (d, cls), cs in by_class.items():
            rep = swept[d][cls]
            CC.set_env(rep.env)
            assert len({c.n_out for c in cs}) >= 2, (CC.class_id(d, cls), rep, 'fewer than two row counts')
            assert CC.required_tables(d, rep) <= {c.table for c in cs}, (CC.class_id(d, cls), rep, sorted({c.table for c in cs}))
            assert all(c.n_out <= CC.N_MAX and c.n_in <= 2 * CC.N_MAX + 3 for c in cs)
            if CC.has_stats(d, cls):
                assert any(c.variant == 'stats' for c in cs), CC.class_id(d, cls)
                # FC_TABLE_STATS never moves a call to another class
                assert CC.route_class(d, rep.n, rep.n, rep.K, rep.Cin, rep.Cout, rep.flags, rep.kind,
                                      CC.full_live_tiles(rep.n, rep.K) if rep.kind == 'pairs_linear' else 0, stats=True) == cls
            tile, S = CC.tile_of(d, rep)
            for c in cs[:4] + cs[-4:]:               # (all of them go through the short way in `cases`; the GPU test asserts each)
                live = CC.live_tiles_of(CC.make_table(c.table, rep.K, c.n_in, c.n_out, tile, S)) if rep.kind == 'pairs_linear' else 0
                got = CC.route_class(d, c.n_in, c.n_out, rep.K, rep.Cin, rep.Cout, rep.flags, rep.kind, live, c.variant == 'stats')
                assert got == cls, (CC.class_id(d, cls), rep, c)
                hit[d].add(got)
    finally:
        CC.set_env(CC.ENV_DEFAULT)
    assert hit[CC.FWD] == set(swept[CC.FWD]) and hit[CC.WGRAD] == set(swept[CC.WGRAD])
    # the process-global switches are back where every other test expects them
    import fcaf3d_amd.functional as Fn
    assert Fn.split_mode() == 2


def test_representatives_are_the_smallest_calls_and_ids_are_unique(swept):
    for d in (CC.FWD, CC.WGRAD):
        ids = [CC.class_id(d, c) for c in swept[d]]
        assert len(set(ids)) == len(ids)
        assert all(rep.n in CC.N_LIST and (rep.Cin, rep.Cout) in CC.CHANNELS and rep.K in CC.KS for rep in swept[d].values())
    # classes that exist from a minimum size on keep the reachable row counts: the multi-offset weight gradient starts at 4 096 rows
    multi = [(c, r) for c, r in swept[CC.WGRAD].items() if CC.class_id(CC.WGRAD, c).startswith('multi')]
    assert multi and all(r.n == 4096 for _, r in multi)
    c, r = multi[0]
    assert CC.row_counts(CC.WGRAD, c, r) == [4096, 4097, CC.N_MAX]


@pytest.mark.parametrize('red', [32, 64, 27 * 256])
def test_premise_every_split_arithmetic_is_exact_on_the_integer_operands(red):
    """the project's restatements of the six-product and h3 arithmetic (oracle/x6_oracle.py) give exactly the float64 product on the
    generator's operands — the all-zero operand, whose amax word of 0 runs the h3 scale into its clamp, included"""
    a = CC.int_operand((24, red), 8, 1)
    b = CC.int_operand((red, 16), 4, 2)
    g = CC.int_operand((red, 16), 8, 3)          # (a weight gradient multiplies two operands of amplitude 8)
    for lhs, rhs in ((a, b), (np.zeros_like(a), b), (a, g), (a, np.zeros_like(g))):
        want = lhs.astype(np.float64) @ rhs.astype(np.float64)
        assert np.abs(want).max() < CC.EXACT
        for fn in (X.matmul_x6, X.matmul_h3):
            got = fn(lhs, rhs)
            assert np.isfinite(got).all() and np.array_equal(got.astype(np.float64), want), fn.__name__
    # bf16-fast keeps the first bf16 piece only: it holds the whole operand
    assert all(np.array_equal(X.split3(v)[0], v) and not X.split3(v)[1].any() for v in (a, b, g))
    # the statistics variant: 0 / 1 and -1 / 0 / 1
    x, w, _ = CC.operands(40, 40, 3, 32, 64, 'stats')
    assert set(np.unique(x)) <= {0.0, 1.0} and set(np.unique(w)) <= {-1.0, 0.0, 1.0}
    x, w, go = CC.operands(40, 40, 3, 32, 64, 'int')
    assert np.abs(x).max() == 8 and np.abs(w).max() == 4 and np.abs(go).max() == 8 and 0.25 < (x == 0).mean() < 0.5
    assert not CC.operands(40, 40, 3, 32, 64, 'zero')[0].any()


SHAPES = [(27, 300, 300, 128, 9), (27, 129, 261, 128, 27), (8, 257, 33, 64, 1), (1, 65, 65, 64, 1), (27, 1, 1, 128, 27), (27, 513, 513, 512, 2)]


@pytest.mark.parametrize('K,n_out,n_in,tile,S', SHAPES)
def test_crafted_tables_keep_their_promises(K, n_out, n_in, tile, S):
    names = ('full', 'empty', 'last_only', 'first_only', 'tile_holes', 'offset_holes', 'offset_holes_b', 'fan_in', 'perm')
    tabs = {t: CC.make_table(t, K, n_in, n_out, tile, S) for t in names}
    for t, nbr in tabs.items():
        assert nbr.shape == (K, n_out) and nbr.dtype == np.int32 and nbr.min() >= -1 and nbr.max() < n_in, t
    cnt = {t: np.count_nonzero(nbr >= 0, axis=1) for t, nbr in tabs.items()}
    assert (tabs['full'] >= 0).all() and not cnt['empty'].any()
    assert cnt['last_only'].sum() == 1 and tabs['last_only'][K - 1, n_out - 1] == n_in - 1
    assert cnt['first_only'].sum() == 1 and tabs['first_only'][0, 0] == 0
    assert set(np.unique(tabs['fan_in'])) <= {-1, n_in - 1}
    for k in range(K):                             # injective per offset: it can go through fc_kernel_map_transpose
        v = tabs['perm'][k][tabs['perm'][k] >= 0]
        assert len(np.unique(v)) == len(v) == min(round(0.6 * n_out), n_in)
    # tile_holes: odd tiles without any neighbour, even tile t with offset (t / 2) % K alone, on every row
    th = tabs['tile_holes']
    for t in range((n_out + tile - 1) // tile):
        blk = th[:, t * tile:(t + 1) * tile] >= 0
        if t % 2:
            assert not blk.any()
        else:
            assert blk[(t // 2) % K].all() and blk.sum() == blk.shape[1]
    # offset_holes: k = 1 (mod max(S, 2)) empty, the rest cycling through {0, 1, tile - 1, tile, tile + 1} (clipped to n_out)
    for name, last in (('offset_holes', 0), ('offset_holes_b', min(tile + 1, n_out))):
        c = cnt[name]
        live = [k for k in range(K) if k % max(S, 2) != 1]
        assert all(c[k] == 0 for k in range(K) if k not in live)
        cyc = [min(v, n_out) for v in (0, 1, tile - 1, tile, tile + 1)]
        assert list(c) == CC.offset_hole_counts(K, n_out, tile, S, name.endswith('_b'))
        assert all(v in cyc for v in c[live])
        if live[-1] == K - 1:
            assert c[K - 1] == last                # offset K - 1: among the empty ones / the fullest
        steps = [cyc.index(v) for v in c[live]] if len(set(cyc)) == 5 else None
        if steps:
            assert all((b - a) % 5 == 1 for a, b in zip(steps, steps[1:]))
        if len(live) >= 5 and n_out > tile:
            assert set(c[live]) == set(cyc)


def test_references_agree_with_a_dense_restatement():
    """ref_fwd / ref_wgrad / ref_dgrad / ref_stem_col against one-hot gather matrices in float64"""
    K, n_in, n_out, Cin, Cout = 5, 23, 17, 3, 4
    nbr = CC.make_table('perm', K, n_in, n_out, 8, 2)
    x, w, go = (np.asarray(a) for a in CC.operands(n_in, n_out, K, Cin, Cout, 'int'))
    G = np.zeros((K, n_out, n_in))
    for k in range(K):
        o = np.nonzero(nbr[k] >= 0)[0]
        G[k, o, nbr[k, o]] = 1
    y = sum(G[k] @ x @ w[k] for k in range(K))
    assert np.array_equal(CC.ref_fwd(x, w, nbr).numpy(), y.astype(np.float32))
    assert np.array_equal(CC.ref_wgrad(x, go, nbr, K).numpy(), np.stack([(G[k] @ x).T @ go for k in range(K)]).astype(np.float32))
    assert np.array_equal(CC.ref_dgrad(go, w, nbr, n_in).numpy(), sum(G[k].T @ go @ w[k].T for k in range(K)).astype(np.float32))
    col = CC.ref_stem_col(x, nbr).numpy()
    assert col.shape == (n_out, 84) and np.array_equal(col[:, :3 * K], np.concatenate([G[k] @ x for k in range(K)], axis=1).astype(np.float32))
    assert not col[:, 3 * K:].any()
    assert torch.equal(CC.ref_fwd(x[:n_out], w[:1], None), torch.from_numpy((x[:n_out].astype(np.float64) @ w[0]).astype(np.float32)))


# ---- the backward form of the statistics epilogue (conv_cases: "the backward form ...") ---------------------------------------------------
def _bn_launch_kinds(cls, rep, case):
    """the launch kinds tests/test_gpu_conv_exact.py runs a case through (a dense class: also `sorted` where the route query agrees)"""
    kinds = [rep.kind]
    if rep.kind == 'dense' and CC.fast_class(CC.FWD, case.n_in, case.n_out, rep.K, rep.Cin, rep.Cout, rep.flags, 'sorted', 0, True) == cls:
        kinds.append('sorted')
    return tuple(kinds)


_BN_CHECKED = {}


def _check_bn_case(rep, case, tile, S, kinds):
    """cap, branch facts and mutations of one case -> the mutations that were live (cached: the classes share most of their cases)"""
    key = (case, rep.K, rep.Cin, rep.Cout, tile, S, kinds)
    if key in _BN_CHECKED:
        return _BN_CHECKED[key]
    bc = CC.bn_case(case.n_in, case.n_out, rep.K, rep.Cin, rep.Cout, case.table, tile, S, case.variant)
    combo, n = bc.combo, case.n_out
    nbr = None if case.table == 'identity' else CC.make_table(case.table, rep.K, case.n_in, n, tile, S)
    what = (rep, case)
    # the inputs keep to their design
    lim8 = None if (combo.act == CC.ELU and combo.y is None) else 8          # (ELU recomputed plants bn_x <= -260 and add = -g)
    for a, lim in ((bc.x, lim8), (bc.add, lim8), (bc.mean, 2), (bc.beta, 2)):
        if a is not None:
            assert np.array_equal(a, np.rint(a)) and (lim is None or np.abs(a).max() <= lim), what
    assert set(np.unique(bc.var)) <= {1.0, 0.25} and set(np.unique(bc.gamma)) <= {1.0, 2.0, 0.5}
    assert combo.affine or (np.all(bc.gamma == 1) and not bc.beta.any())
    assert (bc.add is not None) == combo.add and (bc.y is not None) == (combo.y is not None)
    # the cap: every partial sum is a multiple of 1/4 below 2^22
    gp, gx = CC.bn_terms(bc)
    assert CC.bn_cap(bc) < 1.0, (what, CC.bn_cap(bc))
    assert np.array_equal(gp * 4, np.rint(gp * 4)) and np.array_equal(gx * 4, np.rint(gx * 4)), what
    # the branch facts
    f = CC.bn_facts(bc, nbr)
    if combo.affine:
        assert f['pre_zero_blocks'], what
    if combo.y == 'nan':
        assert np.isnan(bc.y).all() and combo.act == CC.NONE
    if combo.y == 'y':
        assert f['y_disagrees'] > 0.1 or n * rep.Cout < 256, (what, f)          # (a visible share: a one-row case has 64 elements)
        assert f['y_disagrees'] > 0 and f['y_zero'] > 0, (what, f)
        if combo.act == CC.ELU:
            assert f['y_values'] <= {0.0, -0.5, -0.75} and (f['y_values'] >= {-0.5, -0.75} or n < 4), (what, f)
            assert set(np.unique(np.where(bc.y > 0, 1.0, bc.y + 1.0))) <= {1.0, 0.5, 0.25}
    if combo.act == CC.ELU and combo.y is None:
        assert f['big_negative'] > 0 and f['small_negative'] == 0, (what, f)
        if combo.add and (nbr is None or (nbr >= 0).any()):
            assert f['add_cancels'] > 0, (what, f)
    elif combo.y is None:
        assert f['big_negative'] == 0
    if combo.add and n > 1 and (case.table in ('empty', 'last_only', 'first_only') or (case.table == 'tile_holes' and n > tile)):
        assert f['lonely_rows'] > 0, (what, f)          # the sparse tables: a result row without any neighbour still adds `add` act'
    # the mutations
    order = CC.sorted_order(n)
    ref = CC.bn_sums(bc)
    live = []
    for m in CC.MUTATIONS:
        if CC.mutation_live(m, bc, nbr, kinds, order):
            got = CC.bn_sums(bc, m, nbr, order)
            assert not np.array_equal(got, ref), (what, m, 'a live mutation leaves every column total as it was')
            live.append(m)
    _BN_CHECKED[key] = tuple(live)
    return _BN_CHECKED[key]


def test_backward_epilogue_cases_reject_what_they_are_there_to_reject(swept):
    """every class with a statistics epilogue, every case of its backward-epilogue list: the exactness cap holds (4 x the column sums
    of |g'| and |g' xhat| below 2^24), the branch facts each option combination claims are there, and every one-token mutation of the
    REFERENCE (conv_cases.MUTATIONS) changes at least one column total in every case where its branch is live.  No kernel is built or
    run; per class, every mutation that one of its launch kinds can show is live in at least one case."""
    by_class = _cases_by_class(swept)
    n_cases = 0
    try:
        for (d, cls), cs in by_class.items():
            if not CC.has_stats(d, cls):
                assert not any(CC.is_bn(c.variant) for c in cs)
                continue
            rep = swept[d][cls]
            CC.set_env(rep.env)
            tile, S = CC.tile_of(d, rep)
            bn = [c for c in cs if CC.is_bn(c.variant)]
            st = [c for c in cs if c.variant == 'stats']
            # coverage: every statistics case has its backward twin; the perm shapes, fan_in and first_only; every combination
            assert {(c.n_in, c.n_out, c.table) for c in st} <= {(c.n_in, c.n_out, c.table) for c in bn}, CC.class_id(d, cls)
            assert {c.variant for c in bn} == {CC.bn_variant(i) for i in range(len(CC.BN_COMBOS))}, CC.class_id(d, cls)
            assert all(CC.bn_combo(c.variant).add for c in bn if c.table == 'empty')
            if rep.kind not in ('none', 'pairs_linear'):
                assert {(2 * rep.n + 3, 'perm'), (rep.n // 8 + 1, 'perm'), (rep.n, 'fan_in'), (rep.n, 'first_only')} <= {(c.n_in, c.table) for c in bn}
            live = set()
            for c in bn:
                live.update(_check_bn_case(rep, c, tile, S, _bn_launch_kinds(cls, rep, c)))
                n_cases += 1
            want = set(CC.MUTATIONS) - {'launch_row', 'o16_dropped'}
            if rep.kind == 'none':
                want -= {'skip_no_neighbour'}
            if rep.kind == 'dense':
                want.add('launch_row')
            if rep.kind.startswith('pairs') and any(c.n_out > 1024 for c in bn):
                want.add('o16_dropped')
            assert want <= live, (CC.class_id(d, cls), sorted(want - live))
    finally:
        CC.set_env(CC.ENV_DEFAULT)
    print(f'{n_cases} backward-epilogue launches, {len(_BN_CHECKED)} distinct')


def test_backward_epilogue_cap_at_the_largest_shape():
    """the cap's headroom at the largest call of the sweep's grid: a `full` table at 4 097 rows, K = 27, 256 -> 256 channels"""
    worst = 0.0
    for variant in (CC.bn_variant(i) for i in (3, 6, 7)):
        bc = CC.bn_case(4097, 4097, 27, 256, 256, 'full', 128, 1, variant)
        worst = max(worst, CC.bn_cap(bc))
    print(f'4 sum |g\' xhat| / 2^24 = {worst:.3f}, max |g| = {np.abs(bc.g).max():.0f}')
    assert worst < 1.0


def test_backward_epilogue_row_facts():
    """conv_cases restates fc_stat_rb and the two-rows-per-pass loop of k_sum_pairs_stats: the row counts added for them do what they
    are there for"""
    assert [CC.stat_rb(n) for n in (1, 1024, 1025, 4096, 4097)] == [16, 16, 64, 64, 32]
    assert CC.o16_rows(1047).tolist() == list(range(1040, 1047)) and CC.o16_rows(4095).tolist() == list(range(4080, 4095))
    assert all(len(CC.o16_rows(n)) == 0 for n in (1, 16, 17, 1024, 1025, 4096, 4097, CC.N_MAX))
    order = CC.sorted_order(257)
    assert sorted(order.tolist()) == list(range(257)) and (order != np.arange(257)).any()
