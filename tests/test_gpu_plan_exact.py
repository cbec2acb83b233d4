"""-m gpu: the native coordinate plan (fcaf3d_amd/plan.py over csrc/plan.hip, plan_chain.h, plan_maps.h, plan_radix.h) against the
numpy references of tests/coord_cases.py — not against the per-operator path, with which it shares csrc/coord_rules.h and the hash of
csrc/fc_common.h.  The cases of tests/test_gpu_coords_exact.py go through fc_plan_levels + fc_plan_maps as pre-voxelised rows
(C_COORDS_IN: row positions are exact; tests/plan_abi.py), the scene cases (32 / 33 / 65 scenes, empty scenes, a scene of one point)
through the plan's own collate, and a small detector takes three cases through Planner.run, training and inference.

Compared, all exact: sets and level-0 features (feature = input row: they name the winners), rows per scene, the tables read back and
their lookups, every map — the k1 map is row 13 of the k3 table —, nbr_t, pair lists, live tiles, mask-sorted tables (the plan
builds what its row thresholds ask for: every case runs with pair lists for both convolution passes and again with mask-sorted
tables), generated sets and their maps, union rows, the head arrays and seg_start.  Each item ends by holding the two phases to each
other as tests/test_gpu_plan.py does, so that test keeps its meaning.

Measured on an MI355X: the 62 items of this file take 6.5 s together; the slowest is a four-level detector (0.45 s)."""
import numpy as np
import pytest
import torch

import fcaf3d_amd as fa
from fcaf3d_amd import _lib as L
from fcaf3d_amd import plan as PL
from fcaf3d_amd import sparse as SP
from tests import coord_cases as CC
from tests import coord_check as CK
from tests.plan_abi import plan_levels, plan_step

pytestmark = pytest.mark.gpu

CASES = CC.cases()
VS_HEAD = 0.01


def _names(*kinds):
    return sorted(n for n, c in CASES.items() if c.kind in kinds)


def _check_head(sp, name, B):
    ex = CC.expected(name)
    levels = [g['coords'] for g in ex['gen']][::-1] + [ex['sets'][-1].coords]
    want = CC.head_arrays(levels, B, VS_HEAD)
    assert sp.structured and sp.prune_level is None and sp.targets is not None
    assert [m.n for m in sp.head_maps] == [len(x) for x in levels]
    for k, w in want.items():
        got = CK.npy(sp.targets[k])
        assert got.dtype == w.dtype and got.shape == w.shape and np.array_equal(got, w), k      # pts: float32(c) * float32(vs), bit for bit


def _check_against_the_other_phase(sp, rows, B, nl, backward):
    """tests/test_gpu_plan.py's comparison, on this case: sets, tables as lookups, maps"""
    cm, first, _ = SP.CoordMap.from_coords(rows, 1, B, want_first=True)
    a, b = CK.walk_sets(cm, nl), CK.walk_sets(sp.sets[0], nl)
    for s, (x, y) in enumerate(zip(a, b)):
        assert (x.n, x.stride, x.cap) == (y.n, y.stride, y.cap), s
        assert torch.equal(x.coords, y.coords) and x.scene_counts == y.scene_counts, s
        assert torch.equal(CK.lookup_all(y, x.coords), torch.arange(x.n, dtype=torch.int32, device=rows.device)), s
    maps = [(0, 1, 3), (1, 2, 2)] + [t for li in range(1, nl + 1) for t in ((1 + li, 2 + li, 3), (1 + li, 2 + li, 1), (2 + li, 2 + li, 3))]
    for i, o, ks in maps:
        x, y = a[i].kernel_map(a[o], ks), b[i].kernel_map(b[o], ks)
        assert (x.sort_rows, x.use_pairs) == (y.sort_rows, y.use_pairs) and torch.equal(x.nbr, y.nbr), (i, o, ks)
        if backward and i >= 2:
            assert torch.equal(x.nbr_t, y.nbr_t), (i, o, ks)
    return first


def _run_case(name, rows_np, B, nl, points=None, F0_want=None):
    d = CK.dev()
    rows = torch.from_numpy(rows_np).to(d)
    feats = torch.arange(len(rows_np), dtype=torch.float32, device=d).view(-1, 1)      # feature = input row: F0 names the winners
    ex = CC.expected(name)
    # (sort from 1 row, pair convolutions up to 2^30 rows): pair lists both ways; (1, 0): mask-sorted tables + the weight gradient's lists
    for pair_rows in (1 << 30, 0):
        with CK.thresholds(1, pair_rows):
            sp = plan_step(B, nl, points=points, vs=1.0, vs_head=VS_HEAD) if points is not None else \
                plan_step(B, nl, coords=rows, feats=feats, vs_head=VS_HEAD)
            assert sp.backward and len(sp.sets) == 3 + nl + max(nl - 1, 0) and len(sp.maps) == 2 + 3 * nl + max(nl - 1, 0)
            F0 = sp.x.F
            want = ex['sets'][0].first.astype(np.float32)[:, None] if F0_want is None else F0_want[ex['sets'][0].first]
            got = CK.npy(F0)
            assert got.shape == want.shape and np.array_equal(got, want), 'level-0 features'
            CK.check_graph(name, sp.sets[0], backward=True, planned=True)
            for km in sp.maps[2:]:                   # what this pass is there for was built by the plan
                if km.K == 27 and km.use_pairs:
                    assert CK._has(km, '_pairs') and CK._has(km, '_pairs_t') == (pair_rows > 0) and CK._has(km, '_sorted') == (pair_rows == 0)
                    assert CK._has(km, '_sorted_t') == (pair_rows == 0) and km.sort_rows
            ds = [km for km in sp.maps if km.K == 1]
            down = [sp.maps[sp.maps.index(km) - 1] for km in ds]
            for a, b in zip(ds, down):               # the k1 map IS row 13 of the k3 table
                assert a.nbr.data_ptr() == b.nbr.data_ptr() + 13 * 4 * b.n_out and a.nbr_t.data_ptr() == b.nbr_t.data_ptr() + 13 * 4 * b.n_in
            _check_head(sp, name, B)
            first = _check_against_the_other_phase(sp, rows, B, nl, True)
            CK.eq(first, ex['sets'][0].first, 'first of the other phase')
    # inference: no backward tables, the same sets and maps
    with CK.thresholds(1, 1 << 30):
        sp = plan_step(B, nl, points=points, vs=1.0, backward=False, targets=False) if points is not None else \
            plan_step(B, nl, coords=rows, feats=feats, backward=False, targets=False)
        assert not sp.backward and sp.targets is None
        CK.check_graph(name, sp.sets[0], backward=False, planned=True, tables=False)
    torch.cuda.synchronize()
    return sp


@pytest.mark.parametrize('case', _names('graph', 'hash'))
def test_native_plan_equals_numpy(case):
    c = CASES[case]
    sp = _run_case(case, c.rows, c.B, c.nl)
    if c.kind == 'hash':
        t = c.facts['table']
        keys = CK.npy(sp.sets[t].keys).view(np.uint64)
        assert len(keys) == 64 and np.nonzero(keys != CC.EMPTY)[0].tolist() == c.facts['occupied'], 'the chain fills the predicted slots'
        CK.eq(CK.lookup_all(sp.sets[t], torch.from_numpy(c.facts['absent']).to(CK.dev())), np.full(len(c.facts['absent']), -1), 'absent keys')
        assert sp.sets[0].cap == (64 if t == 0 else 128)


@pytest.mark.parametrize('case', sorted(CC.raw_cases()))
def test_native_plan_collate_equals_numpy(case):
    """raw points: voxel size 1.0, points at voxel + 0.5 (floorf(p / vs) is exact), feature = global row / 255"""
    B, scenes = CC.raw_cases()[case]
    d = CK.dev()
    off, pts = 0, []
    for s in scenes:
        p = np.concatenate([s[:, 1:].astype(np.float32) + np.float32(0.5), np.arange(off, off + len(s), dtype=np.float32)[:, None]], axis=1)
        pts.append(torch.from_numpy(np.ascontiguousarray(p.reshape(-1, 4))).to(d))
        off += len(s)
    F0 = (np.arange(off, dtype=np.float32) / np.float32(255.0))[:, None]
    _run_case(case, np.concatenate(scenes), B, 2, points=pts, F0_want=F0)


@pytest.mark.parametrize('case', _names('refuse'))
def test_native_plan_refuses_rows_outside_the_range(case):
    c = CASES[case]
    d = CK.dev()
    rows = torch.from_numpy(c.rows).to(d)
    feats = torch.zeros((len(c.rows), 1), dtype=torch.float32, device=d)
    with pytest.raises(ValueError):
        plan_step(c.B, 2, coords=rows, feats=feats)
    torch.cuda.synchronize()


def test_native_plan_a_million_rows_and_a_tail():
    """1 026 coarse counts: the sum loop of k_plan_finalize runs twice, and the winners of the last block depend on it"""
    c = CASES['chain_1m']
    d = CK.dev()
    rows = torch.from_numpy(c.rows).to(d)
    feats = torch.arange(len(c.rows), dtype=torch.float32, device=d).view(-1, 1)        # exact below 2^24
    sets, per_scene, F0 = plan_levels(rows, feats, c.B, c.nl)
    want = CC.chain(c.rows, 3 + c.nl)
    for s, st in enumerate(want):
        CK.eq(sets[s], st.coords, f'set {s}')
        assert per_scene[s].tolist() == [len(st.coords)]
    CK.eq(F0[:, 0], want[0].first.astype(np.float32), 'winners')
    torch.cuda.synchronize()


@pytest.mark.parametrize('case', _names('map_big'))
def test_native_plan_pair_lists_over_more_than_64_blocks(case):
    """`same1` of a one-level plan on 64 x 1 024 + 1 / 65 x 1 024 + 1 voxels of stride 8"""
    c = CASES[case]
    d = CK.dev()
    rows = torch.from_numpy(c.rows).to(d)
    feats = torch.zeros((len(c.rows), 1), dtype=torch.float32, device=d)
    with CK.thresholds(1 << 30, 1 << 30):
        sp = plan_step(c.B, 1, coords=rows, feats=feats, targets=False)
    assert [m.n for m in sp.sets] == [len(c.rows)] * 4
    km = sp.sets[3].kernel_map(sp.sets[3], 3)
    assert km is sp.maps[-1] and CK._has(km, '_pairs') and CK._has(km, '_pairs_t')
    nbr = CC.kernel_map(c.rows, c.rows, 3, 8)
    CK.eq(km.nbr, nbr, 'nbr')
    CK.eq(km.nbr_t, nbr[::-1], 'nbr_t')
    want = CC.pair_lists(nbr)
    CK.check_pairs(km.pairs(), want, 'pairs')
    CK.check_pairs(km.pairs_t(), CC.pair_lists(nbr[::-1].copy()), 'pairs_t')
    assert km.pair_tiles() == CC.live_tiles(want[3])
    torch.cuda.synchronize()


@pytest.mark.parametrize('n', CC.ARGSORT_SIZES)
def test_argsort27_on_crafted_masks(n):
    d = CK.dev()
    for name, keys in CC.mask_patterns(n).items():
        k = torch.from_numpy(keys).to(d)
        order = torch.full((n,), CC.SENT, dtype=torch.int32, device=d)
        ws = torch.empty(L.query('fc_argsort27_ws_bytes', n), dtype=torch.uint8, device=d)
        L.call('fc_argsort27', L.ptr(k), n, L.ptr(order), L.ptr(ws), ws.numel(), L.stream())
        CK.eq(order, np.argsort(keys, kind='stable'), f'{name} {n}')


def _detector(levels):
    torch.manual_seed(0)
    cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=1.0)
    m = cfg.model
    m.backbone['n_outs'] = levels
    m.neck_with_head['in_channels'] = (64, 128, 256, 512)[:levels]
    m.neck_with_head.assigner['n_scales'] = levels
    return fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg'))


@pytest.mark.parametrize('levels,case,training', [(1, 'negative_cloud', True), (2, 'symmetric_cloud', True), (2, 'symmetric_cloud', False),
                                                  (4, 'range_limit', True), (4, 'range_limit', False)])
def test_planner_run_on_a_small_detector_equals_numpy(levels, case, training):
    """the product's own route to the two native calls (Planner.run, raw points): 1, 2 and 4 levels, training and inference"""
    c = CASES[case]
    d = CK.dev()
    det = _detector(levels).to(d).train(training)
    pts = []
    for b in range(c.B):
        r = c.rows[c.rows[:, 0] == b]
        p = np.concatenate([r[:, 1:].astype(np.float32) + np.float32(0.5), np.zeros((len(r), 3), np.float32)], axis=1)
        pts.append(torch.from_numpy(np.ascontiguousarray(p)).to(d))
    with torch.set_grad_enabled(training):
        sp = PL.planner_of(det).run(pts, training, want_targets=training)
    torch.cuda.synchronize()
    assert sp.backward == training and len(sp.sets) == 3 + levels + levels - 1
    want = CC.chain(c.rows, 3 + levels)
    for s, st in enumerate(want):
        CK.eq(sp.sets[s].coords, st.coords, f'set {s}')
        assert sp.sets[s].scene_counts == np.bincount(st.coords[:, 0], minlength=c.B).tolist()
        CK.check_table(sp.sets[s], st.coords, CC.capacity(st.n_in), f'table {s}')
    co = [st.coords for st in want]
    for li in range(1, levels + 1):
        p, m = 1 + li, 2 + li
        CK.eq(sp.sets[p].kernel_map(sp.sets[m], 3).nbr, CC.kernel_map(co[p], co[m], 3, 1 << p), f'down{li}')
        CK.eq(sp.sets[m].kernel_map(sp.sets[m], 3).nbr, CC.kernel_map(co[m], co[m], 3, 1 << m), f'same{li}')
    if levels == c.nl:
        CK.check_graph(case, sp.sets[0], backward=training, planned=True, tables=False)
    torch.cuda.synchronize()
