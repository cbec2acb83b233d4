"""-m gpu: the per-operator coordinate phase (fcaf3d_amd/sparse.py over csrc/coords.hip) against the numpy references of
tests/coord_cases.py, on crafted rows: negative and odd coordinates (fc_floor_div), the range limit, probe chains that wrap through
slot 0, duplicates, the block edges of the scans and of the pair-list kernels, offsets without pairs.  One item per case.

Compared, all exact: from_coords with first / inverse at every stride of the pyramid, the tables read back (capacity, keys on their
probe paths from the numpy-computed home slots, values), batched lookups of members and absent keys, kernel maps for ks 3 / 2 / 1,
nbr_t, pairs() / pairs_t(), live tiles, the mask-sorted tables, generate() with its map, the union rows — and the entry points once
more into buffers of the test's own, pre-filled with a sentinel.  tests/test_coord_cases_cpu.py shows, without a GPU, that every
case changes its expected tables under the mistake it is there for.

Measured on an MI355X: the 48 items of this file take 4.8 s together; the slowest are the million-row chain (0.5 s) and the first
item, which loads the library (0.3 s)."""
import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from fcaf3d_amd import sparse as SP
from tests import coord_cases as CC
from tests import coord_check as CK

pytestmark = pytest.mark.gpu

CASES = CC.cases()


def _names(*kinds):
    return sorted(n for n, c in CASES.items() if c.kind in kinds)


def _level0(c, d):
    """from_coords on the case's rows with first / inverse, then the pyramid by from_coords with q = 2 x stride (what strided() calls),
    first / inverse checked at every stride.  The sets are NOT linked: the graph walk builds its own through strided(2)"""
    sets = CC.chain(c.rows, 3 + c.nl)
    rows = torch.from_numpy(c.rows).to(d)
    cm0, first, inv = SP.CoordMap.from_coords(rows, 1, c.B, want_first=True, want_inverse=True)
    CK.eq(first, sets[0].first, 'first 0')
    CK.eq(inv, sets[0].inverse, 'inverse 0')
    cm = cm0
    for s in range(1, len(sets)):
        nx, first, inv = SP.CoordMap.from_coords(cm.coords, cm.stride * 2, c.B, q=cm.stride * 2, want_first=True, want_inverse=True)
        CK.eq(nx.coords, sets[s].coords, f'set {s}')
        CK.eq(first, sets[s].first, f'first {s}')
        CK.eq(inv, sets[s].inverse, f'inverse {s}')
        cm = nx
    return cm0


@pytest.mark.parametrize('case', _names('graph', 'hash'))
def test_per_operator_phase_equals_numpy(case):
    c = CASES[case]
    d = CK.dev()
    with CK.thresholds(1, 1 << 30):                  # every 27-offset map: mask-sorted tables AND pair lists
        cm0 = _level0(c, d)
        sets = CK.check_graph(case, cm0, backward=True, direct=True)
    if c.kind == 'hash':
        t = c.facts['table']
        cm = sets[t]
        keys = CK.npy(cm.keys).view(np.uint64)
        assert len(keys) == 64 and np.nonzero(keys != CC.EMPTY)[0].tolist() == c.facts['occupied'], 'the chain fills the predicted slots'
        assert keys[63] != CC.EMPTY and keys[0] != CC.EMPTY and keys[11] == CC.EMPTY
        CK.eq(CK.lookup_all(cm, torch.from_numpy(c.facts['absent']).to(d)), np.full(len(c.facts['absent']), -1), 'absent keys')
        assert CK.npy(sets[0].keys).size == (64 if t == 0 else 128)
    torch.cuda.synchronize()


def _hash_unique_count(rows, d):
    """fc_hash_unique through the C ABI -> the count word"""
    n = rows.shape[0]
    cap = CC.capacity(n)
    keys = torch.empty(cap, dtype=torch.int64, device=d)
    vals = torch.empty(cap, dtype=torch.int32, device=d)
    out = torch.full((n, 4), CC.SENT, dtype=torch.int32, device=d)
    cnt = torch.zeros(1, dtype=torch.int32, device=d)
    ws = L.workspace(L.query('fc_hash_unique_ws_bytes', n), d)
    L.call('fc_hash_unique', L.ptr(rows), n, 1, L.ptr(keys), L.ptr(vals), cap, L.ptr(out), None, None, L.ptr(cnt), L.ptr(ws), ws.numel(), L.stream())
    return int(cnt.item())


@pytest.mark.parametrize('case', _names('refuse'))
def test_rows_outside_the_range_are_refused(case):
    """a row at +-32 640 on any axis, or with batch index -1: the count is -1 and from_coords raises; the same rows with the offender at
    +-32 639 are the edge_*_32639 cases of the test above, accepted down to stride 64"""
    c = CASES[case]
    d = CK.dev()
    rows = torch.from_numpy(c.rows).to(d)
    assert _hash_unique_count(rows, d) == -1
    with pytest.raises(ValueError):
        SP.CoordMap.from_coords(rows, 1, c.B)
    ok = torch.from_numpy(c.rows[~CC.out_of_range(c.rows)]).to(d)
    assert _hash_unique_count(ok, d) == len(np.unique(CC.wide_keys(c.rows[~CC.out_of_range(c.rows)])))
    torch.cuda.synchronize()


def test_a_million_rows_and_a_tail():
    """1 048 576 distinct voxels and 1 500 rows of duplicates and new voxels: 1 026 blocks of 1 024 input rows; first / inverse of level 0
    and the sets down to stride 64"""
    c = CASES['chain_1m']
    d = CK.dev()
    cm0 = _level0(c, d)
    assert cm0.cap == 1 << 22
    sets = CC.chain(c.rows, 3 + c.nl)
    for s, cm in enumerate(CK.walk_sets(cm0, c.nl)):                 # strided(2) itself, down to stride 64
        CK.eq(cm.coords, sets[s].coords, f'strided set {s}')
        assert cm.cap == CC.capacity(sets[s].n_in)
    torch.cuda.synchronize()


@pytest.mark.parametrize('case', _names('map_big'))
def test_pair_lists_over_more_than_64_blocks(case):
    """a same-set map of 64 x 1 024 + 1 / 65 x 1 024 + 1 rows: the last block's prefix covers 64 / 65 block counts"""
    c = CASES[case]
    d = CK.dev()
    cm, _, _ = SP.CoordMap.from_coords(torch.from_numpy(c.rows).to(d), 8, c.B)
    CK.eq(cm.coords, c.rows, 'rows are distinct')
    nbr = CC.kernel_map(c.rows, c.rows, 3, 8)
    km = cm.kernel_map(cm, 3)
    CK.eq(km.nbr, nbr, 'nbr')
    want = CC.pair_lists(nbr)
    CK.check_pairs(km.pairs(), want, 'pairs')
    pi, po, pos, cnt = CK.pairs_direct(km.nbr)
    for got, w, nm in ((cnt, want[3], 'cnt'), (pos, want[2], 'pos'), (pi, want[0], 'in'), (po, want[1], 'out')):
        CK.eq(got, w, 'direct ' + nm)
    assert km.pair_tiles() == CC.live_tiles(want[3])
    torch.cuda.synchronize()
