"""GPU: fc_batch_augment_voxelize (csrc_post/batch.hip) against the numpy sampler of tests/test_batch_cpu.py and against per-scene
fc_augment_voxelize with the same rows (bit-equal), and the detector's voxelize on a DeviceLoader batch."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_batch_cpu import POISON_F, POISON_I, expected_rows, make_batch

pytestmark = pytest.mark.gpu
VS, FD = 0.02, 255.0


def _run(bt, sample_idx=None):
    from fcaf3d_amd import _lib as L
    dev = torch.device('cuda:0')
    R, nf = bt['out_rows'], bt['nfeat']
    arena, desc = torch.from_numpy(bt['arena']).to(dev), torch.from_numpy(bt['desc']).to(dev)
    idx = torch.from_numpy(sample_idx.astype(np.int32)).to(dev) if sample_idx is not None else None
    coords = torch.full((R, 4), POISON_I, dtype=torch.int32, device=dev)
    feats = torch.full((R, nf), float(POISON_F), dtype=torch.float32, device=dev)
    sample_out = torch.full((R,), POISON_I, dtype=torch.int32, device=dev)
    points = torch.full((R, 3 + nf), float(POISON_F), dtype=torch.float32, device=dev)
    L.call('fc_batch_augment_voxelize', L.ptr(arena), arena.shape[0], 3 + nf, L.ptr(desc), bt['B'], bt['total_out'], R, L.ptr(idx),
           0 if idx is None else idx.numel(), VS, FD, nf, L.ptr(coords), L.ptr(feats) if nf else None, L.ptr(sample_out), L.ptr(points),
           L.stream())
    torch.cuda.synchronize()
    return coords.cpu().numpy(), feats.cpu().numpy(), sample_out.cpu().numpy(), points.cpu().numpy()


def _per_scene(bt, rows):
    """B calls of fc_augment_voxelize with the given rows -> per scene (coords, feats, points)"""
    from fcaf3d_amd import _lib as L
    dev = torch.device('cuda:0')
    nf = bt['nfeat']
    arena = torch.from_numpy(bt['arena']).to(dev)
    out = []
    for s in range(bt['B']):
        n = bt['n_out'][s]
        raw = arena[int(bt['src_off'][s]):int(bt['src_off'][s]) + bt['n_src'][s]]
        idx = torch.from_numpy(rows[s].astype(np.int32)).to(dev)
        coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
        feats = torch.empty((n, nf), dtype=torch.float32, device=dev)
        points = torch.empty((n, 3 + nf), dtype=torch.float32, device=dev)
        xf = np.ascontiguousarray(bt['xf'][s])
        L.call('fc_augment_voxelize', L.ptr(raw), raw.shape[0], 3 + nf, L.ptr(idx), n, xf.ctypes.data, s, VS, FD, nf, L.ptr(coords),
               L.ptr(feats) if nf else None, L.ptr(points), L.stream())
        torch.cuda.synchronize()
        out.append((coords.cpu().numpy(), feats.cpu().numpy(), points.cpu().numpy()))
    return out


def _check(bt, rows, got):
    coords, feats, sample_out, points = got
    ref = _per_scene(bt, rows)
    live = np.zeros(bt['out_rows'], bool)
    for s in range(bt['B']):
        sl = slice(int(bt['out_off'][s]), int(bt['out_off'][s]) + bt['n_out'][s])
        live[sl] = True
        assert np.array_equal(sample_out[sl], rows[s]), s
        assert np.array_equal(coords[sl], ref[s][0]), s                                   # bit-equal: integers
        assert np.array_equal(feats[sl].view(np.int32), ref[s][1].view(np.int32)), s
        assert np.array_equal(points[sl].view(np.int32), ref[s][2].view(np.int32)), s
        assert (coords[sl, 0] == s).all()
    assert live.sum() == bt['total_out'] and (~live).sum() > 0
    assert (coords[~live] == POISON_I).all() and (sample_out[~live] == POISON_I).all()      # rows outside every scene: untouched
    assert (feats[~live] == POISON_F).all() and (points[~live] == POISON_F).all()


@pytest.mark.parametrize('variant', [0, 1])
def test_ragged_batch_draws_the_documented_rows_and_equals_per_scene_calls(variant):
    """B = 5: a one-row scene, two scenes sampled with replacement, one without, an exact permutation; workgroups straddle scene
    boundaries; one scene is aligned; the two variants together hold every flip / rotation combination"""
    bt = make_batch(variant=variant)
    rows = expected_rows(bt)
    assert len(set(rows[2])) == 4000 and np.array_equal(np.sort(rows[4]), np.arange(4097))
    _check(bt, rows, _run(bt))


def test_one_scene_without_features_and_explicit_indices():
    one = make_batch(n_src=(700,), n_out=(300,), nfeat=0, gaps=(0, 2))
    _check(one, expected_rows(one), _run(one))
    bt = make_batch()
    rng = np.random.default_rng(5)
    pos, parts = 2, []
    for s in range(bt['B']):
        bt['desc'][s, 5] = pos
        parts.append((pos, rng.integers(0, bt['n_src'][s], bt['n_out'][s])))
        pos += bt['n_out'][s] + 3
    sample_idx = np.full(pos, 1 << 30, np.int32)
    for o, v in parts:
        sample_idx[o:o + len(v)] = v
    _check(bt, expected_rows(bt, sample_idx), _run(bt, sample_idx))


def test_bad_arguments_are_refused_without_a_launch():
    from fcaf3d_amd import _lib as L
    bt = make_batch()
    dev = torch.device('cuda:0')
    arena, desc = torch.from_numpy(bt['arena']).to(dev), torch.from_numpy(bt['desc']).to(dev)
    R = bt['out_rows']
    coords = torch.full((R, 4), POISON_I, dtype=torch.int32, device=dev)
    feats = torch.full((R, 3), float(POISON_F), dtype=torch.float32, device=dev)
    fn = L.lib().fc_batch_augment_voxelize
    ok = [arena.data_ptr(), arena.shape[0], 6, desc.data_ptr(), bt['B'], bt['total_out'], R, None, 0, VS, FD, 3, coords.data_ptr(),
          feats.data_ptr(), None, None, ctypes.c_void_p(L.stream())]
    for pos, val in ((4, 257), (4, -1), (5, R + 1), (5, -1), (2, 5), (9, 0.0), (0, None), (3, None), (12, None), (13, None), (11, 4)):
        a = list(ok)
        a[pos] = val
        assert fn(*a) == -1, (pos, val)
    for pos, val in ((4, 0), (5, 0)):                                  # nothing to do: accepted, nothing launched
        a = list(ok)
        a[pos] = val
        assert fn(*a) == 0
    torch.cuda.synchronize()
    assert (coords == POISON_I).all() and (feats == float(POISON_F)).all()


def test_detector_voxelize_on_a_loader_batch_equals_the_per_scene_lazy_path(tmp_path):
    """SingleStageSparse3DDetector.voxelize on a DeviceLoader batch (one launch, the hook of the list) = on the per-scene
    LazyAugmentedPoints of the same draws and rows (fc_augment_voxelize per scene) = on the batch's elements as a plain list"""
    import fcaf3d_amd as fa
    from fcaf3d_amd import data as DT
    from fcaf3d_amd.pipelines import LazyAugmentedPoints
    from tests.test_fit_cpu import make_cfg
    from tests.test_gpu_dist import _model
    dev = torch.device('cuda:0')
    cfg = make_cfg(tmp_path, samples_per_gpu=3)
    ds = DT.build_dataset(cfg.data.train)
    rs = DT.ResidentScenes(ds, dev)
    ld = DT.DeviceLoader(rs, ds.pipeline, 3, seed=9)
    model, _ = _model(fa)
    model = model.to(dev)
    for bt in ld.batches(1):
        pts = bt['points']
        total = sum(p.shape[0] for p in pts)
        assert total == 3 * 4000
        c0 = torch.empty((total, 4), dtype=torch.int32, device=dev)
        f0 = torch.empty((total, 3), dtype=torch.float32, device=dev)
        rows = torch.empty(total, dtype=torch.int32, device=dev)
        pts.voxelize_batch(model.voxel_size, 255.0, c0, f0, sample_out=rows)
        coords, feats = model.voxelize(pts)
        assert torch.equal(coords, c0) and torch.equal(feats, f0)
        lazy = []
        for b, meta in enumerate(bt['img_metas']):
            i = meta['dataset_index']
            k = int(rs.slot[i])
            p = ld.draw(1, i)
            raw = rs.arena[int(rs.start[k]):int(rs.start[k]) + int(rs.count[k])]
            lazy.append(LazyAugmentedPoints(raw, rows[4000 * b:4000 * (b + 1)], p, rs.align[k]))
            if rs.count[k] >= 4000:
                assert len(set(rows[4000 * b:4000 * (b + 1)].tolist())) == 4000                 # without replacement
        c1, f1 = model.voxelize(lazy)
        assert torch.equal(coords, c1) and torch.equal(feats, f1)
        c2, f2 = model.voxelize(list(pts))                             # no hook: the elements' own voxelize_into
        assert torch.equal(coords, c2) and torch.equal(feats, f2)
        assert torch.equal(pts[1].materialize(), lazy[1].materialize())
