"""The native coordinate plan through its C ABI, for tests that hand it exact rows: fc_plan_levels alone (`plan_levels`) or followed by
fc_plan_maps (`plan_step`), on pre-voxelised coordinates (C_COORDS_IN: row positions are exact) or on raw points (the plan's own
collate).  `plan_step` wraps the result as plan.Planner.run does, so a test walks the same object graph a detector would get."""
import types

import numpy as np
import torch

from fcaf3d_amd import _lib as L
from fcaf3d_amd import plan as PL
from fcaf3d_amd import sparse as SP


def _stage1(B, nl, coords, feats, points, vs, backward, targets, vs_head):
    lib = L.lib()
    cfg = np.zeros(lib.fc_plan_cfg_words(), dtype=np.int64)
    scenes = np.zeros((max(B, 1), 3), dtype=np.int64)
    if points is not None:
        assert len(points) == B and all(p.dtype == torch.float32 and p.dim() == 2 and p.is_contiguous() for p in points)
        dev, total, nfeat = points[0].device, sum(p.shape[0] for p in points), points[0].shape[1] - 3
        cfg[PL.C_PT_STRIDE] = points[0].shape[1]
        for b, p in enumerate(points):
            scenes[b] = (p.data_ptr(), p.shape[0], p.shape[1])
    else:
        assert coords.dtype == torch.int32 and coords.is_contiguous() and feats.dtype == torch.float32 and feats.is_contiguous()
        dev, total, nfeat = coords.device, coords.shape[0], feats.shape[1]
        cfg[PL.C_COORDS_IN], cfg[PL.C_FEATS_IN] = coords.data_ptr(), feats.data_ptr()
    cfg[PL.C_B], cfg[PL.C_NL], cfg[PL.C_NFEAT], cfg[PL.C_TOTAL] = B, nl, nfeat, total
    cfg[PL.C_VS], cfg[PL.C_FEATDIV] = PL._f64_bits(float(vs)), PL._f64_bits(255.0)
    cfg[PL.C_BACKWARD], cfg[PL.C_TARGETS], cfg[PL.C_NECK] = int(backward), int(targets), 1
    cfg[PL.C_SORT_MIN], cfg[PL.C_PAIR_ROWS], cfg[PL.C_PTS_THR] = SP.SORT_MIN_ROWS, SP.PAIR_CONV_ROWS, -1
    cfg[PL.C_VS_HEAD] = PL._f64_bits(float(vs if vs_head is None else vs_head))
    out = np.zeros(lib.fc_plan_out_words(B, nl), dtype=np.int64)
    counts, cnt = (torch.zeros(n, dtype=torch.int32).pin_memory() for n in PL.pinned_words(B, nl))
    a1 = torch.empty(L.query('fc_plan_stage1_bytes', total, B, nl, nfeat), dtype=torch.uint8, device=dev)
    rc = lib.fc_plan_levels(cfg.ctypes.data, scenes.ctypes.data, a1.data_ptr(), a1.numel(), out.ctypes.data, counts.data_ptr(), L.stream())
    assert rc == 0, rc
    if out[PL.H_BAD]:
        torch.cuda.synchronize()
        raise ValueError('voxel coordinate outside the range of the hash keys')
    return types.SimpleNamespace(cfg=cfg, out=out, counts=counts, cnt=cnt, a1=a1, dev=dev, nfeat=nfeat, B=B, nl=nl)


def plan_levels(coords, feats, B, nl=4):
    """fc_plan_levels alone on pre-voxelised rows -> (coordinate sets, rows per (set, scene), level-0 features)"""
    S = 3 + nl
    st = _stage1(B, nl, coords, feats, None, 1.0, False, False, None)
    out, a1 = st.out, st.a1
    assert out[PL.H_S] == S
    torch.cuda.synchronize()
    ar = PL._Arenas(a1, a1)
    cn = st.counts.numpy()
    sets = []
    for s in range(S):
        o = out[PL.HDR + PL.SETW * s:PL.HDR + PL.SETW * (s + 1)]
        assert int(o[PL.S_N]) == int(cn[PL.METAW * s + PL.META_ROWS]) and int(o[PL.S_STRIDE]) == 1 << s
        sets.append(ar.view(int(o[PL.S_COORDS]), (int(o[PL.S_N]), 4)).clone())
    per_scene = cn[PL.METAW * S:PL.METAW * S + S * B].reshape(S, B).copy()
    F0 = ar.view(int(out[PL.H_F0]), (sets[0].shape[0], st.nfeat), torch.float32).clone()
    return sets, per_scene, F0


def plan_step(B, nl, coords=None, feats=None, points=None, vs=1.0, backward=True, targets=True, vs_head=None):
    """fc_plan_levels + fc_plan_maps -> plan.StepPlan (sets, maps, head arrays as views of the plan's arenas).  The row thresholds are
    read from sparse.SORT_MIN_ROWS / sparse.PAIR_CONV_ROWS, as the product does.  ValueError when the plan refuses a coordinate."""
    st = _stage1(B, nl, coords, feats, points, vs, backward, targets, vs_head)
    lib = L.lib()
    need = int(lib.fc_plan_stage2_bytes(st.cfg.ctypes.data, st.out.ctypes.data, st.counts.data_ptr()))
    assert need >= 0
    a2 = torch.empty(need + 256, dtype=torch.uint8, device=st.dev)
    rc = lib.fc_plan_maps(st.cfg.ctypes.data, st.out.ctypes.data, st.counts.data_ptr(), a2.data_ptr(), a2.numel(), st.cnt.data_ptr(), L.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return PL.Planner(None)._wrap(st.out.copy(), st.counts.numpy().copy(), PL._Arenas(st.a1, a2), B, nl, st.nfeat, bool(backward), bool(targets), st.dev)
