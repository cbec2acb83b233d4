"""CPU: the table layouts of the native coordinate phase have ONE declaration (fcaf3d_amd/csrc/plan_layout.h) that csrc/plan.hip compiles
and fcaf3d_amd/plan.py reads, and the sizing pass of fc_plan_maps (fc_plan_stage2_bytes: pure host code, no device needed) decides the
same sets, maps, flags and arena size as it did before it was taken apart — the literals below were recorded from the library of the
commit before (the buffers themselves are the GPU tests' business: tests/test_gpu_plan.py)."""
import ast

import numpy as np
import pytest

from fcaf3d_amd import _lib as L
from fcaf3d_amd import plan as PL
from fcaf3d_amd import sparse as SP

LAYOUT = {k: v for block in L.parse_enums(L.PLAN_LAYOUT) for k, v in block.items()}


def test_plan_py_takes_every_layout_name_from_the_header():
    assert len(LAYOUT) > 90
    for k, v in LAYOUT.items():
        assert getattr(PL, k) == v, k
    tree = ast.parse(open(PL.__file__.replace('.pyc', '.py')).read())
    assigned = {n.id for node in tree.body for n in ast.walk(node) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store)}
    assert not assigned & set(LAYOUT), assigned & set(LAYOUT)
    assert len(PL.PROBE_KINDS) == LAYOUT['PK_KINDS']


def test_both_descriptors_fit_inside_a_map_record():
    assert LAYOUT['MW_FLAGS'] < LAYOUT['MW_DESC_F']
    assert LAYOUT['MW_DESC_F'] + SP.MAPW <= LAYOUT['MW_DESC_B']
    assert LAYOUT['MW_DESC_B'] + SP.MAPW <= LAYOUT['MAPR']


@pytest.mark.parametrize('B,nl', [(1, 1), (2, 2), (3, 4), (8, 4), (64, 4)])
def test_pinned_buffers_hold_the_counter_blocks(B, nl):
    S, maps = 3 + nl, LAYOUT['MAPS_FIXED'] + LAYOUT['MAPS_PER_LEVEL'] * nl
    n_counts, n_cnt = PL.pinned_words(B, nl)
    assert n_counts >= LAYOUT['METAW'] * S + S * B
    # the counters of every map and the tail, then the nl * B + 1 segment starts staged behind them
    assert n_cnt >= LAYOUT['CNT_MAP'] * maps + LAYOUT['CNT_TAIL'] + nl * B + 1
    assert LAYOUT['CNT_T'] + 27 <= LAYOUT['CNT_MAP'] and 27 <= LAYOUT['CNT_T']
    assert L.lib().fc_plan_out_words(B, nl) >= LAYOUT['HDR'] + LAYOUT['SETW'] * LAYOUT['MAXSETS'] + LAYOUT['MAPR'] * maps


def sizing_pass(lib, B, nl, rows, backward=1, targets=1, pts_thr=-1, threshold=8192):
    """fc_plan_stage2_bytes on synthetic counts: set s of the chain has rows[s] rows, spread evenly over the scenes -> (bytes, out)"""
    S = 3 + nl
    assert len(rows) == S
    cfg = np.zeros(lib.fc_plan_cfg_words(), dtype=np.int64)
    cfg[PL.C_B], cfg[PL.C_NL], cfg[PL.C_NFEAT], cfg[PL.C_TOTAL] = B, nl, 3, 2 * rows[0]
    cfg[PL.C_BACKWARD], cfg[PL.C_TARGETS], cfg[PL.C_PTS_THR], cfg[PL.C_NECK] = backward, targets, pts_thr, 1
    cfg[PL.C_SORT_MIN] = cfg[PL.C_PAIR_ROWS] = threshold
    out = np.zeros(lib.fc_plan_out_words(B, nl), dtype=np.int64)
    counts = np.zeros(PL.pinned_words(B, nl)[0], dtype=np.int32)
    out[PL.H_S] = S
    for s in range(S):
        o = out[PL.HDR + PL.SETW * s:]
        o[PL.S_N], o[PL.S_STRIDE], o[PL.S_PARENT] = rows[s], 1 << s, -1
        counts[PL.METAW * s + PL.META_ROWS] = rows[s]
        for b in range(B):
            counts[PL.METAW * S + s * B + b] = rows[s] // B + (1 if b < rows[s] % B else 0)
    need = lib.fc_plan_stage2_bytes(cfg.ctypes.data, out.ctypes.data, counts.ctypes.data)
    return int(need), out


def _maps(out):
    base = PL.HDR + PL.SETW * PL.MAXSETS
    return [out[base + PL.MAPR * m:base + PL.MAPR * (m + 1)] for m in range(int(out[PL.H_NMAPS]))]


BIG = [300000, 120000, 40000, 14000, 4000, 1000, 200]


@pytest.mark.parametrize('B,nl,rows,kw,want,flags', [
    (2, 2, [20000, 9000, 3000, 900, 250], {}, (4774656, 6, 9, -1, 2250), [3, 0, 2, 0, 2, 2, 0, 2, 4]),
    (3, 4, BIG, {}, (83122944, 10, 17, -1, 117000), [3, 0, 3, 0, 3, 2, 0, 2, 2, 0, 2, 2, 0, 2, 4, 4, 4]),
    (3, 4, BIG, dict(backward=0, targets=0), (39927552, 10, 17, -1, 117000), [3, 0, 3, 0, 3, 2, 0, 2, 2, 0, 2, 2, 0, 2, 4, 4, 4]),
    (1, 1, [5000, 2000, 700, 200], {}, (811520, 4, 5, -1, 200), [2, 0, 2, 0, 2]),
    (2, 2, [0, 0, 0, 0, 0], {}, (5120, 6, 9, -1, 0), None),
    (2, 3, [20000, 9000, 3000, 900, 250, 60], dict(pts_thr=1000), (5449472, 8, 13, 0, 0), None),
    (2, 4, [60000, 25000, 9000, 2500, 600, 130, 25], dict(pts_thr=5000), (12991744, 10, 17, 0, 0), None),
])
def test_sizing_pass_decides_what_it_always_did(B, nl, rows, kw, want, flags):
    need, out = sizing_pass(L.lib(), B, nl, rows, **kw)
    assert (need, out[PL.H_S], out[PL.H_NMAPS], out[PL.H_PRUNE], out[PL.H_NALL]) == want
    if flags is not None:
        assert [int(o[PL.MW_FLAGS]) for o in _maps(out)] == flags
    for m, o in enumerate(_maps(out)):
        # no arena: every address word of the records and of both descriptors is null, the sizes are not; the counter words are the
        # map's place in the (null) counter block
        for d in (o[PL.MW_DESC_F:PL.MW_DESC_F + SP.MAPW], o[PL.MW_DESC_B:PL.MW_DESC_B + SP.MAPW]):
            assert (d[SP.MAP_N_IN], d[SP.MAP_N_OUT], d[SP.MAP_K]) == (o[PL.MW_NIN], o[PL.MW_NOUT], o[PL.MW_K])
            assert not d[SP.MAP_NBR:].any()
        assert o[PL.MW_CNT] in (0, 4 * PL.CNT_MAP * m) and o[PL.MW_TCNT] in (0, 4 * (PL.CNT_MAP * m + PL.CNT_T))
        assert not any(o[w] for w in range(PL.MW_NBR, PL.MW_FLAGS) if w not in (PL.MW_CNT, PL.MW_TCNT))


def test_sizing_pass_map_records():
    _, out = sizing_pass(L.lib(), 2, 2, [20000, 9000, 3000, 900, 250])
    got = [tuple(int(o[w]) for w in (PL.MW_IN, PL.MW_OUT, PL.MW_K, PL.MW_NIN, PL.MW_NOUT)) for o in _maps(out)]
    assert got == [(0, 1, 27, 20000, 9000), (1, 2, 8, 9000, 3000), (2, 3, 27, 3000, 900), (2, 3, 1, 3000, 900), (3, 3, 27, 900, 900),
                   (3, 4, 27, 900, 250), (3, 4, 1, 900, 250), (4, 4, 27, 250, 250), (5, 5, 27, 2000, 2000)]
