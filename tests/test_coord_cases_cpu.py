"""No GPU: tests/coord_cases.py is what the exact coordinate tests believe, so it is pinned here.
  * its restatements of the shared rules and its references against oracle/me_oracle.py, on every case;
  * the branch facts every builder claims, recomputed: chain length, wrap and the home slot of each absent key; 27 n mod 4; pair-list
    blocks above 64; coarse counts above 1 024; which offsets are empty; r = 0 and r = s on negative coordinates; ...
  * every case REJECTS the one-token change it is there for: the reference is evaluated again under the mutation (numpy only — nothing
    mutated is built or run on a GPU) and the expected tables must differ."""
import numpy as np
import pytest
import torch

from oracle import me_oracle as mo
from tests import coord_cases as CC

CASES = CC.cases()
GRAPH = sorted(n for n, c in CASES.items() if c.kind == 'graph')


def _co(name):
    return [s.coords for s in CC.expected(name)['sets']]


# ---- restatements ---------------------------------------------------------------------------------------------------------------------
def test_pack_mix_capacity_and_the_table_restatement():
    rng = np.random.default_rng(0)
    c = np.concatenate([rng.integers(0, 300, size=(500, 1)), rng.integers(-CC.LIMIT - 1, CC.LIMIT + 1, size=(500, 3))], axis=1)
    assert np.array_equal(CC.fc_pack(c).astype(np.int64), mo.pack_keys(c))                      # same fields, same order
    assert np.array_equal(np.argsort(CC.fc_pack(c), kind='stable'), np.argsort(CC.wide_keys(c), kind='stable'))   # lexicographic in (b, x, y, z)
    # fc_mix is a bijection of 64-bit words with fixed point 0 (xor-shift and odd multipliers); two published values of this finaliser
    assert int(CC.fc_mix(0)[0]) == 0 and len(np.unique(CC.fc_mix(np.arange(1 << 16)))) == 1 << 16
    assert int(CC.fc_mix(1)[0]) == 0xb456bcfc34c2cb2c and int(CC.fc_mix(2)[0]) == 0x3abf2a20650683e7
    from fcaf3d_amd import sparse as SP
    for n in (0, 1, 2, 3, 16, 17, 32, 33, 1 << 20, (1 << 20) + 1500):
        assert CC.capacity(n) == SP._next_pow2(max(2 * n, 2)) and CC.capacity(n) >= max(2 * n, 2)
    u = CC.unique_first(c.astype(np.int32))[0]
    keys, vals, slot = CC.table_insert(u, CC.capacity(len(u)))
    assert CC.probe_path_ok(keys) and np.array_equal(CC.table_lookup(keys, vals, u), np.arange(len(u)))
    far = u.copy(); far[:, 0] += 301
    assert (CC.table_lookup(keys, vals, far) == -1).all()
    assert np.array_equal(keys[slot], CC.fc_pack(u))


def test_quantiser_and_range_restatements():
    x = np.arange(-200, 200)
    c = np.stack([np.zeros_like(x), x, -x, x // 3], axis=1).astype(np.int32)
    for q in (1, 2, 4, 8, 16, 32, 64):
        want = c.copy(); want[:, 1:] = np.floor_divide(want[:, 1:], q) * q
        assert np.array_equal(CC.quantize(c, q), want)
        got = CC.quantize(c, q)[:, 1:]
        assert (got <= c[:, 1:]).all() and (c[:, 1:] - got < q).all() and (got % q == 0).all()
    assert int(CC.quantize([[0, -CC.LIMIT, CC.LIMIT, 0]], 64)[0, 1]) == -32640
    e = np.array([[0, CC.LIMIT, -CC.LIMIT, 0], [0, CC.LIMIT + 1, 0, 0], [0, 0, 0, -CC.LIMIT - 1], [-1, 0, 0, 0], [32767, 0, 0, 0], [32768, 0, 0, 0]])
    assert CC.out_of_range(e).tolist() == [False, True, True, True, False, True]


@pytest.mark.parametrize('case', GRAPH)
def test_references_equal_the_oracle(case):
    c = CASES[case]
    ex = CC.expected(case)
    cur = c.rows
    for s, st in enumerate(ex['sets']):
        q = cur.copy(); q[:, 1:] = np.floor_divide(q[:, 1:], 1 << s) * (1 << s)
        uc, first, inv = mo.unique_first(q)
        assert np.array_equal(st.coords, uc) and np.array_equal(st.first, first) and np.array_equal(st.inverse, inv), s
        assert ex['caps'][s] == CC.capacity(len(cur)) and st.n_in == len(cur)
        assert np.array_equal(ex['rows_per_scene'][s], np.bincount(uc[:, 0], minlength=c.B))
        assert (np.diff(uc[:, 0]) >= 0).all(), 'rows of a set are grouped by scene'
        if s:
            assert np.array_equal(uc, mo.stride_coords(cur, 1 << (s - 1), 2))
        cur = uc
    co = _co(case)
    for name, (i, o, ks, nbr) in ex['maps'].items():
        want = mo.kernel_map(co[i], co[o], mo.kernel_offsets(ks, 1 << i))
        assert np.array_equal(nbr, want), name
        assert np.array_equal(CC.offsets(ks, 1 << i), mo.kernel_offsets(ks, 1 << i))
        if i != o and ks > 1:                        # the input-side construction of the plan builds the same table
            assert np.array_equal(CC.strided_map_from_input(co[i], co[o], ks, 1 << i), want), name
        # derived tables, by the assertions of tests/test_gpu_ops.py::test_kernel_map_pairs_bit_exact
        nt = CC.transpose(nbr, len(co[i]))
        pi, po, pos, cnt = CC.pair_lists(nbr)
        pit, pot, post, cntt = CC.pair_lists(nt)
        for k in range(nbr.shape[0]):
            rows = np.nonzero(nbr[k] >= 0)[0]
            assert cnt[k] == cntt[k] == len(rows)
            assert np.array_equal(po[k, :len(rows)], rows) and np.array_equal(pi[k, :len(rows)], nbr[k, rows])
            assert (pi[k, len(rows):] == CC.SENT).all() and (po[k, len(rows):] == CC.SENT).all()
            w = np.full(nbr.shape[1], -1, np.int32); w[rows] = np.arange(len(rows))
            assert np.array_equal(pos[k], w)
            order = np.argsort(nbr[k, rows], kind='stable')
            assert np.array_equal(pot[k, :len(rows)], nbr[k, rows][order]) and np.array_equal(pit[k, :len(rows)], rows[order])
            assert all(nt[k, nbr[k, r]] == r for r in rows[:50])
        if i == o and ks == 3:
            assert np.array_equal(nt, nbr[::-1]), 'a centred kernel on one set: the transposed table is the table with its offsets reversed'
        assert CC.live_tiles(cnt) == sum(-(-int(v) // 128) for v in cnt)
        m = CC.row_masks(nbr)
        assert all(int(m[r]) == sum(1 << k for k in range(nbr.shape[0]) if nbr[k, r] >= 0) for r in range(0, len(m), max(len(m) // 40, 1)))
        tab, order = CC.mask_sorted(nbr)
        assert sorted(order.tolist()) == list(range(len(m))) and all((m[a], a) < (m[b], b) for a, b in zip(order[:-1], order[1:]))
        assert np.array_equal(tab, nbr[:, order])
    par, stride = co[-1], 1 << (len(co) - 1)
    for g in ex['gen']:
        want = mo.gen_conv_transpose_coords(par, stride)
        assert np.array_equal(g['coords'], want) and g['stride'] == stride // 2
        assert np.array_equal(g['nbr'], mo.kernel_map(want, want, mo.kernel_offsets(3, stride // 2)))
        lv = co[g['level']]
        assert (g['rows'] >= 0).all() and np.array_equal(want[g['rows']], lv), 'every backbone voxel lies inside the generated set'
        uc, _ = mo.union_add(lv, torch.zeros(len(lv), 1), want, torch.zeros(len(want), 1))
        if len(want) > len(lv):
            assert np.array_equal(uc, want), 'the union is the generated set, in its order'
        else:                                        # (the level fills the generated set: the oracle keeps the level's order, the product the set's)
            assert sorted(CC.wide_keys(uc).tolist()) == sorted(CC.wide_keys(want).tolist())
        par, stride = want, stride // 2
    levels = [g['coords'] for g in ex['gen']][::-1] + [co[-1]]
    h = CC.head_arrays(levels, c.B, 0.01)
    assert len(h['pts']) == sum(len(x) for x in levels) and h['seg_start'][-1] == len(h['pts']) and h['pts'].dtype == np.float32
    for l in range(len(levels)):
        for b in range(c.B):
            a, e = h['seg_start'][l * c.B + b], h['seg_start'][l * c.B + b + 1]
            assert (h['level'][a:e] == l).all() and (h['scene'][a:e] == b).all()


# ---- branch facts -----------------------------------------------------------------------------------------------------------------
def _neg_r(coords, s):
    """which of r = 0 / r = s occur on NEGATIVE coordinates, per axis, for a map of stride s -> 2 s"""
    x = coords[:, 1:].astype(np.int64)
    r = x - np.floor_divide(x, 2 * s) * 2 * s
    return [set(r[x[:, a] < 0, a].tolist()) for a in range(3)]


@pytest.mark.parametrize('case', sorted(n for n, c in CASES.items() if 'sign' in c.facts))
def test_sign_and_parity_facts(case):
    c = CASES[case]
    x = c.rows[:, 1:]
    if c.facts['sign'] == 'negative':
        assert (x < 0).all()
    else:
        assert (x < 0).any(axis=0).all() and (x > 0).any(axis=0).all()
    if c.facts.get('odd'):
        assert (x % 2 == 1).all()
    if case.startswith('block3') and 'negative' not in case:
        s = int(case.split('_s')[1])
        assert sorted(map(tuple, x.tolist())) == sorted((a, b, d) for a in (-s, 0, s) for b in (-s, 0, s) for d in (-s, 0, s))
    if case.startswith('isolated'):
        s = int(case.split('_s')[1])
        assert {(-1, -1, -1), (-2 * s, -2 * s, -2 * s), (-2 * s - 1, -2 * s - 1, -2 * s - 1)} <= set(map(tuple, x.tolist()))
    if c.facts.get('both_r'):
        co = _co(case)
        for si in (0, 1, 2):                         # the inputs of the stem (ks 3), the pool (ks 2) and down1 (ks 3)
            assert all(r == {0, 1 << si} for r in _neg_r(co[si], 1 << si)), si
    # rejecting: a truncating quantiser gives other sets; truncating division in the strided-map candidate gives another table
    good, bad = CC.chain(c.rows, 4), CC.chain(c.rows, 4, trunc=True)
    assert any(not np.array_equal(a.coords, b.coords) for a, b in zip(good, bad))
    co = [s.coords for s in good]
    diff = False
    for si, ks in ((0, 3), (1, 2), (2, 3)):
        want = CC.kernel_map(co[si], co[si + 1], ks, 1 << si)
        diff |= not np.array_equal(CC.strided_map_from_input(co[si], co[si + 1], ks, 1 << si, trunc=True), want)
    assert diff


def test_range_facts():
    c = CASES['range_limit']
    x = c.rows[:, 1:]
    for a in range(3):
        assert x[:, a].max() == CC.LIMIT and x[:, a].min() == -CC.LIMIT
    assert not CC.out_of_range(c.rows).any() and c.nl == 4
    co = _co('range_limit')
    assert len(co) == 7 and co[6][:, 1:].min() == -32640 and co[6][:, 1:].max() == 32576
    for s, cs in enumerate(co):                      # every key field holds the largest kernel offset, and the strided maps' candidate q + 2 s
        assert cs[:, 1:].min() - (1 << s) + 32768 >= 0 and cs[:, 1:].max() + 2 * (1 << s) + 32768 <= 65535
    same4 = CC.expected('range_limit')['maps']['same4'][3]
    assert (same4[13] == np.arange(same4.shape[1])).all() and (np.delete(same4, 13, axis=0) >= 0).sum() > 0   # real neighbours at stride 64
    assert len(set(co[0][:, 0].tolist())) == 3       # together in one scene and in neighbouring scenes
    # 16-bit fields that WRAPPED would make the far corners neighbours: -32640 - 64 = 32832 (mod 65536)?  no voxel sits there, but
    # +32576 + 64 = 32640 and -32640 differ by 65280 != 65536: the wide-key reference and a wrapped key agree that they are no pair
    edges = {n: k for n, k in CASES.items() if n.startswith('edge_')}
    assert len(edges) == 13
    for n, k in edges.items():
        bad = CC.out_of_range(k.rows)
        assert int(bad.sum()) == (1 if k.kind == 'refuse' else 0), n
        if k.kind == 'refuse':
            row = k.rows[bad][0]
            assert (row[0] == -1) if k.facts['axis'] < 0 else (abs(int(row[1 + k.facts['axis']])) == CC.LIMIT + 1 and row[1 + k.facts['axis']] == k.facts['value'])
            if k.facts['axis'] >= 0:                 # rejecting: a limit of 32 640 accepts the row
                assert not CC.out_of_range(k.rows, limit=CC.LIMIT + 1).any()
        else:
            assert np.abs(k.rows[:, 1:]).max() == CC.LIMIT and (k.rows[:, 1 + k.facts['axis']] == k.facts['value']).sum() == 1
    assert {(k.facts['axis'], int(np.sign(k.facts['value'])), k.kind) for k in edges.values() if k.facts['axis'] >= 0} == \
        {(a, s, kd) for a in range(3) for s in (-1, 1) for kd in ('graph', 'refuse')}


@pytest.mark.parametrize('case', ['hash_chain_level0', 'hash_chain_stride2'])
def test_hash_case_facts(case):
    c = CASES[case]
    sets = CC.chain(c.rows, 2)
    t = c.facts['table']
    rows_in_ = c.rows if t == 0 else sets[0].coords                 # the rows the table's insert pass sees
    q = 1 << t
    cap = CC.capacity(len(rows_in_))
    assert cap == 64 and CC.capacity(len(c.rows)) == (64 if t == 0 else 128)
    members = sets[t].coords
    assert (members[:, 1:] % q == 0).all() and (t == 0 or (c.rows[:, 1:] % 2 == 0).all(axis=1).sum() == len(c.rows) - 3)
    hm = CC.home(members, cap)
    assert (hm == c.facts['chain_home']).sum() == c.facts['chain_len'] >= 8 and c.facts['chain_home'] >= cap - 3
    keys, vals, slot = CC.table_insert(CC.quantize(rows_in_, q), cap)
    occ = np.nonzero(keys != CC.EMPTY)[0].tolist()
    assert occ == c.facts['occupied'] and {cap - 1, 0} <= set(occ) and 11 not in occ
    assert CC.probe_path_ok(keys)
    # the occupied slots do not depend on the order of insertion (what lets a test predict them for a parallel insert)
    perm = np.random.default_rng(3).permutation(len(rows_in_))
    assert np.nonzero(CC.table_insert(CC.quantize(rows_in_, q)[perm], cap)[0] != CC.EMPTY)[0].tolist() == occ
    # duplicates: of the key at the end of the chain among them; the smallest row wins
    qk = CC.fc_pack(CC.quantize(rows_in_, q))
    dup = [k for k in np.unique(qk) if (qk == k).sum() > 1]
    assert len(dup) >= 3 and any((hm[CC.fc_pack(members) == k] == c.facts['chain_home']).all() for k in dup)
    first = np.array([np.nonzero(qk == k)[0][0] for k in CC.fc_pack(members)])
    assert np.array_equal(vals[[int(np.nonzero(keys == k)[0][0]) for k in CC.fc_pack(members)]], first)
    assert np.array_equal(first, sets[t].first)
    # absent keys: homes at the first slot of the run, in the middle, at its last slot, at an empty slot
    ab = c.facts['absent']
    assert CC.home(ab, cap).tolist() == [61, 2, 10, 11, 40] and (CC.rows_in(members, ab) == -1).all() and (ab[:, 1:] % q == 0).all()
    final = vals.copy(); final[slot[first]] = np.arange(len(members))          # after the finalize pass: key -> row of the set
    assert np.array_equal(CC.table_lookup(keys, final, members), np.arange(len(members)))
    assert (CC.table_lookup(keys, final, ab) == -1).all()
    # rejecting: a lookup that stops at the first other key, one that does not wrap, an insert where the last occurrence wins
    assert (CC.table_lookup(keys, final, members, stop_at_first=True) == -1).sum() >= 8
    lost = CC.table_lookup(keys, final, members, no_wrap=True) == -1
    assert lost.sum() >= 6 and set(slot[first][lost].tolist()) <= set(range(0, 11))
    assert not np.array_equal(CC.table_insert(CC.quantize(rows_in_, q), cap, last_wins=True)[1], vals)
    lw = CC.unique_first(CC.quantize(rows_in_, q).astype(np.int32), last_wins=True)
    assert not np.array_equal(lw[1], sets[t].first)


def test_chain_block_facts():
    c = CASES['chain_1m']
    n = len(c.rows)
    assert n == (1 << 20) + 1500 and (n + 1023) // 1024 == 1026 > 1024
    x = c.rows[:1 << 20, 1:]
    assert len(np.unique(CC.wide_keys(c.rows[:1 << 20]))) == 1 << 20 and (x.min(0) < 0).all() and (x.max(0) > 0).all()
    uc, first, inv = CC.unique_first(c.rows)
    flags = np.zeros(n, dtype=np.int64); flags[first] = 1
    tail = flags[1 << 20:]
    assert tail[:1024].sum() > 0 and tail[1024:].sum() > 0 and 0 < tail.sum() < 1500, 'winners and duplicates in each of the last two blocks'
    pos, total = CC.winner_positions(flags)
    assert total == len(uc) and np.array_equal(pos, np.arange(len(uc)))
    # rejecting: a sum over at most 1 024 coarse counts misplaces the winners of the last block and loses rows of the set
    pos_m, total_m = CC.winner_positions(flags, max_coarse=1024)
    assert total_m < total and not np.array_equal(pos_m, pos) and np.array_equal(pos_m[:1 << 20], pos[:1 << 20])
    assert (pos_m != pos).nonzero()[0].min() >= (1 << 20) + tail[:1024].sum()
    # rejecting: last occurrence wins
    assert not np.array_equal(CC.unique_first(c.rows, last_wins=True)[1], first)


def test_map_size_facts():
    mods = set()
    for n in (1, 2, 3, 5, 255, 256, 257, 1023, 1024, 1025, 2049):
        name = f'map_rows_{n}'
        co = _co(name)
        assert len(co[3]) == n == CASES[name].facts['n_out'] and len(co[0]) == len(co[2]) > n
        mods.add(27 * n % 4)
        i, o, ks, nbr = CC.expected(name)['maps']['down1']
        assert nbr.shape == (27, n)
        got = CC.strided_map_from_input(co[2], co[3], 3, 4, prefill_tail=False)
        if 27 * n % 4:                               # rejecting: a prefill that skips the tail leaves entries that nobody writes
            assert not np.array_equal(got, nbr) and (got.reshape(-1)[-(27 * n % 4):] == CC.SENT).any()
        else:
            assert np.array_equal(got, nbr)
    assert mods == {0, 1, 2, 3}
    assert {-(-n // 256) for n in (255, 256, 257)} == {1, 2} and {-(-n // 1024) for n in (1023, 1024, 1025, 2049)} == {1, 2, 3}
    for n in (31, 32, 33):
        co = _co(f'strided_map_in_{n}')
        assert len(co[2]) == n and -(-8 * n // 256) == (1 if n <= 32 else 2)      # eight threads per input row, 256 per block


@pytest.mark.parametrize('nb', [64, 65])
def test_pair_list_block_facts(nb):
    c = CASES[f'same_map_{nb}_blocks_plus_1']
    n = len(c.rows)
    assert n == nb * 1024 + 1 and -(-n // 1024) == nb + 1 == c.facts['blocks'] > 64
    assert len(np.unique(CC.wide_keys(c.rows))) == n and c.rows[:, 1:].min() < 0 < c.rows[:, 1:].max()
    assert (c.rows[:, 1:] % 8 == 0).all() and c.nl == 1
    nbr = CC.kernel_map(c.rows, c.rows, 3, 8)
    assert (nbr[:, -1] >= 0).sum() >= 2 and (nbr[13] == np.arange(n)).all(), 'pairs in the last block'
    assert np.array_equal(nbr, mo.kernel_map(c.rows, c.rows, mo.kernel_offsets(3, 8)))
    good, bad = CC.pair_lists(nbr), CC.pair_lists(nbr, max_prefix_blocks=64)
    same = all(np.array_equal(a, b) for a, b in zip(good, bad))
    # the last block has index nb: its prefix covers nb blocks — 64 is the last size one pass of the 64-lane loop covers
    assert same == (nb == 64)


def test_offset_sparsity_facts():
    for name in ('offsets_centre_only', 'offsets_line_x', 'offsets_single_pair_last_row', 'offsets_full_cube'):
        c = CASES[name]
        nbr = CC.expected(name)['maps']['same1'][3]                   # the set of stride 8 onto itself
        cnt = (nbr >= 0).sum(axis=1)
        assert np.nonzero(cnt)[0].tolist() == c.facts['present'], name
        if 'single' in c.facts:
            last = nbr.shape[1] - 1
            for k in c.facts['single']:
                assert cnt[k] == 1
            assert nbr[14, 0] == last and nbr[12, last] == 0
            down = CC.expected(name)['maps']['down1'][3]              # stride 4 -> 8: the same voxels; one pair per row, centre only
            assert np.nonzero((down >= 0).sum(axis=1))[0].tolist() == [13]
    assert (CC.expected('offsets_full_cube')['maps']['same1'][3] >= 0).sum(axis=1).min() > 0


def test_raw_case_facts():
    rc = CC.raw_cases()
    assert {B for B, _ in rc.values()} >= {32, 33, 65}
    B, sc = rc['raw_empty_first_middle_last']
    assert [len(s) for s in sc][0] == 0 and len(sc[2]) == 0 and len(sc[-1]) == 0 and len(sc[1]) and len(sc[3]) and B == 5
    assert [len(s) for s in rc['raw_scene_of_one_point'][1]][1] == 1
    for B, sc in rc.values():
        assert len(sc) == B and all((s[:, 0] == b).all() for b, s in enumerate(sc))
        pts = np.concatenate(sc)[:, 1:].astype(np.float32) + np.float32(0.5)
        assert np.array_equal(np.floor(pts / np.float32(1.0)).astype(np.int32), np.concatenate(sc)[:, 1:])     # floorf(p / vs) is exact


def test_argsort_pattern_facts():
    for n in CC.ARGSORT_SIZES:
        p = CC.mask_patterns(n)
        assert len(set(p['equal'].tolist())) == 1 and (np.diff(p['ascending']) > 0).all() and (np.diff(p['descending']) < 0).all()
        assert all(0 <= int(v.min()) and int(v.max()) < (1 << 27) and len(v) == n for v in p.values())
        if n > 1:
            assert len(set(p['alternating'].tolist())) == 2 and p['alternating'][0] > p['alternating'][1]
            want = np.concatenate([np.arange(1, n, 2), np.arange(0, n, 2)])
            assert np.array_equal(np.argsort(p['alternating'], kind='stable'), want)


def test_every_case_has_a_kind_the_gpu_tests_run():
    assert {c.kind for c in CASES.values()} == {'graph', 'hash', 'chain_big', 'map_big', 'refuse'}
    assert all(len(c.rows) <= 4200 for c in CASES.values() if c.kind in ('graph', 'hash', 'refuse'))
    assert all(c.nl in (1, 2, 4) and (c.rows[:, 0] < c.B).all() for c in CASES.values())
