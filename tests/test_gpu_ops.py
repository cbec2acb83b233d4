"""-m gpu: HIP operators (through the C ABI) against the CPU oracle on identical inputs.
Integer results (coordinates, hash order, kernel maps, argmax) must be bit-exact; fp32 features
within 1e-4 relative to the tensor scale (BASELINE.json north_star)."""
import numpy as np
import pytest
import torch

import fcaf3d_amd.functional as Fn
from oracle import loss_oracle as lo
from oracle import me_oracle as mo

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _close(a, b, tol=TOL, what=''):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * scale, f'{what}: max err {err:.3e} vs scale {scale:.3e}'


def _scene_coords(seed, n_points=20000, B=2, vs=0.02):
    from fcaf3d_amd.synthetic import make_scene
    pts = [make_scene(seed + b, n_points=n_points)[0] for b in range(B)]
    c, f = mo.batch_sparse_collate([p[:, :3] / np.float32(vs) for p in pts], [p[:, 3:] / np.float32(255.) for p in pts])
    return pts, c, f


def test_voxelize_and_unique():
    from fcaf3d_amd import _lib as L
    from fcaf3d_amd.sparse import CoordMap
    dev = _dev()
    pts, c_ref, f_ref = _scene_coords(0)
    coords = torch.empty((len(c_ref), 4), dtype=torch.int32, device=dev)
    feats = torch.empty((len(c_ref), 3), dtype=torch.float32, device=dev)
    off = 0
    for b, p in enumerate(pts):
        t = torch.from_numpy(p).to(dev)
        L.call('fc_voxelize', L.ptr(t), len(p), 6, b, 0.02, 255.0, 3, L.ptr(coords[off:]), L.ptr(feats[off:]), L.stream())
        off += len(p)
    assert np.array_equal(coords.cpu().numpy(), c_ref)
    assert np.array_equal(feats.cpu().numpy(), f_ref)
    for q in (1, 2, 4):
        cq = c_ref.copy(); cq[:, 1:] = np.floor_divide(cq[:, 1:], q) * q
        uc, first, inv = mo.unique_first(cq)
        cm, gfirst, ginv = CoordMap.from_coords(coords, q, 2, q=q, want_first=True, want_inverse=True)
        assert cm.n == len(uc)
        assert np.array_equal(cm.coords.cpu().numpy(), uc)
        assert np.array_equal(gfirst.cpu().numpy(), first)
        assert np.array_equal(ginv.cpu().numpy(), inv)


def test_unique_edge_cases():
    from fcaf3d_amd.sparse import CoordMap
    dev = _dev()
    cm, _, _ = CoordMap.from_coords(torch.zeros((0, 4), dtype=torch.int32, device=dev), 1, 1)
    assert cm.n == 0
    c = torch.tensor([[0, -1, -3, 5]] * 7 + [[1, -1, -3, 5]], dtype=torch.int32, device=dev)
    cm, first, inv = CoordMap.from_coords(c, 1, 2, want_first=True, want_inverse=True)
    assert cm.coords.cpu().tolist() == [[0, -1, -3, 5], [1, -1, -3, 5]]
    assert first.cpu().tolist() == [0, 7] and inv.cpu().tolist() == [0] * 7 + [1]
    cm2, _, _ = CoordMap.from_coords(c, 2, 2, q=2)
    assert cm2.coords.cpu().tolist() == [[0, -2, -4, 4], [1, -2, -4, 4]]


@pytest.mark.parametrize('ks,s', [(3, 1), (3, 2), (2, 2), (1, 2)])
def test_kernel_maps_exact(ks, s):
    from fcaf3d_amd.sparse import CoordMap
    dev = _dev()
    _, c_ref, _ = _scene_coords(3)
    uc, _, _ = mo.unique_first(c_ref)
    cm, _, _ = CoordMap.from_coords(torch.from_numpy(c_ref).to(dev), 1, 2)
    out_ref = mo.stride_coords(uc, 1, s) if s > 1 else uc
    om = cm.strided(s)
    assert np.array_equal(om.coords.cpu().numpy(), out_ref)
    nbr_ref = mo.kernel_map(uc, out_ref, mo.kernel_offsets(ks, 1))
    km = cm.kernel_map(om, ks)
    assert np.array_equal(km.nbr.cpu().numpy(), nbr_ref)
    # transpose property: nbr_t[k][i] == o  <=>  nbr[k][o] == i
    nt = km.nbr_t.cpu().numpy()
    K = nbr_ref.shape[0]
    ref_t = np.full((K, len(uc)), -1, np.int32)
    for k in range(K):
        o = np.nonzero(nbr_ref[k] >= 0)[0]
        ref_t[k, nbr_ref[k, o]] = o
    assert np.array_equal(nt, ref_t)


def _layer_routes(km, n_in, n_out, K, Cin, Cout, flags, x6):
    """What the route query (fc_conv_fwd_route / fc_conv_wgrad_route, csrc/conv_route.h) says the forward, backward-data and
    weight-gradient launches of Fn.sparse_conv on this map become, with the table kind and flags functional._SparseConv hands them
    -> {'fwd' | 'dgrad' | 'wgrad': fields, the enums by their header names}"""
    import fcaf3d_amd.functional as Fn
    from fcaf3d_amd import _lib as L
    from fcaf3d_amd.sparse import PAIR_CONV_ROWS
    E = L.header_enums()
    names = {'family': 'FC_FAM_', 'wsrc': 'FC_WSRC_', 'mode': 'FC_MODE_', 'epi': 'FC_EPI_'}

    def named(r, over={}):
        pre = dict(names, **over)
        return {k: next((e for e, x in E.items() if k in pre and e.startswith(pre[k]) and x == v), v) for k, v in r.items()}

    def conv(n_i, n_o, ci, co, pair_rows, transposed):
        mfma = not (flags & Fn.CONV_FMA) and ci % 32 == 0 and co % 64 == 0
        fl = flags | Fn.CONV_X6 if (x6 and mfma) else flags | Fn.CONV_WT if (transposed and Fn.DGRAD_WT) else flags
        kind, live = E['FC_TABLE_SORTED' if (mfma and km.sort_rows) else 'FC_TABLE_DENSE'], 0
        if km.use_pairs and pair_rows <= PAIR_CONV_ROWS and mfma:
            kind, live = E['FC_TABLE_PAIRS'], km.pair_tiles(transposed=transposed)
        rc, r = L.route('fc_conv_fwd_route', n_i, n_o, K, ci, co, fl, kind, live)
        assert rc == 0
        return named(r)
    wpairs = km.use_pairs and not (flags & Fn.CONV_FMA) and Cin % 64 == 0 and Cout % 64 == 0
    rc, w = L.route('fc_conv_wgrad_route', n_in, n_out, K, Cin, Cout, flags | Fn.WGRAD_X6 if x6 else flags,
                    E['FC_TABLE_PAIRS' if wpairs else 'FC_TABLE_DENSE'])
    assert rc == 0
    return {'fwd': conv(n_in, n_out, Cin, Cout, n_out, False), 'dgrad': conv(n_out, n_in, Cout, Cin, n_in, True),
            'wgrad': named(w, {'family': 'FC_WFAM_', 'table': 'FC_TABLE_'})}


def _conv_case(dev, n_points, Cin, Cout, ks, s, flags, seed=5, B=2, level_q=1, x6=None, routes=None):
    """x6: None = the default route (split-bf16 kernels where they exist), False = the fp32 MFMA / FMA kernels.
    routes: {'fwd' | 'dgrad' | 'wgrad': {route field: value}} the launches of this case must take (`_layer_routes`): the case names
    the kernels it claims to test and fails, before it launches, once the routing rules send the shape elsewhere"""
    import fcaf3d_amd.functional as Fn
    from fcaf3d_amd.sparse import CoordMap
    _, c_ref, _ = _scene_coords(seed, n_points=n_points, B=B)
    if level_q > 1:
        c_ref = c_ref.copy(); c_ref[:, 1:] = np.floor_divide(c_ref[:, 1:], level_q) * level_q
    uc, _, _ = mo.unique_first(c_ref)
    T = level_q
    cm, _, _ = CoordMap.from_coords(torch.from_numpy(uc).to(dev), T, B)
    om = cm.strided(s)
    out_ref_c = mo.stride_coords(uc, T, s) if s > 1 else uc
    nbr = mo.kernel_map(uc, out_ref_c, mo.kernel_offsets(ks, T))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(len(uc), Cin, generator=g)
    w = torch.randn(ks ** 3, Cin, Cout, generator=g) / np.sqrt(Cin * ks ** 3)
    go = torch.randn(len(out_ref_c), Cout, generator=g)
    xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
    out_r = mo.conv(xr, wr, nbr)
    gx_r, gw_r = torch.autograd.grad(out_r, [xr, wr], go)
    xg = x.to(dev).requires_grad_(True); wg = w.to(dev).requires_grad_(True)
    Fn.FLAGS = flags
    x6_0 = Fn.X6
    if x6 is not None:
        Fn.X6 = x6
    try:
        km = cm.kernel_map(om, ks)
        if routes:
            got = _layer_routes(km, cm.n, om.n, ks ** 3, Cin, Cout, flags, Fn.X6)
            for part, want in routes.items():
                assert {k: got[part][k] for k in want} == want, (part, got[part], want)
        out_g = Fn.sparse_conv(xg, wg, km, om.n)
        gx_g, gw_g = torch.autograd.grad(out_g, [xg, wg], go.to(dev))
    finally:
        Fn.FLAGS, Fn.X6 = 0, x6_0
    tag = f'conv n={len(uc)} {Cin}->{Cout} k{ks}s{s} flags={flags} x6={x6}'
    _close(out_g, out_r, what=tag + ' fwd')
    _close(gx_g, gx_r, what=tag + ' dgrad')
    _close(gw_g, gw_r, what=tag + ' wgrad')


def test_kernel_map_pairs_bit_exact():
    """pair lists == np.nonzero of the oracle's table, offset by offset, in ascending output row (bit-exact)"""
    from fcaf3d_amd.sparse import CoordMap
    dev = _dev()
    _, c_ref, _ = _scene_coords(11, n_points=30000, B=2)
    c_ref = c_ref.copy(); c_ref[:, 1:] = np.floor_divide(c_ref[:, 1:], 4) * 4
    uc, _, _ = mo.unique_first(c_ref)
    cm, _, _ = CoordMap.from_coords(torch.from_numpy(uc).to(dev), 4, 2)
    for s in (1, 2):
        om = cm.strided(s)
        oc = mo.stride_coords(uc, 4, s) if s > 1 else uc
        nbr = mo.kernel_map(uc, oc, mo.kernel_offsets(3, 4))
        km = cm.kernel_map(om, 3)
        pi, po, pos, cnt = (t.cpu().numpy() for t in km.pairs())
        for k in range(27):
            o = np.nonzero(nbr[k] >= 0)[0]
            assert cnt[k] == len(o)
            assert np.array_equal(po[k, :len(o)], o) and np.array_equal(pi[k, :len(o)], nbr[k, o])
            want = np.full(nbr.shape[1], -1, np.int32); want[o] = np.arange(len(o))
            assert np.array_equal(pos[k], want)
        # the transposed lists: ascending in the input row, same pair multiset
        pit, pot, _, cntt = (t.cpu().numpy() for t in km.pairs_t())
        for k in range(27):
            o = np.nonzero(nbr[k] >= 0)[0]
            i = nbr[k, o]
            order = np.argsort(i, kind='stable')
            assert cntt[k] == len(o)
            assert np.array_equal(pot[k, :len(o)], i[order]) and np.array_equal(pit[k, :len(o)], o[order])


@pytest.mark.parametrize('Cin,Cout', [(64, 64), (64, 128), (128, 128), (128, 64), (32, 64), (256, 256)])
def test_conv_mfma_small_tiles(Cin, Cout):
    _conv_case(_dev(), 6000, Cin, Cout, 3, 1, 0, level_q=4)


def test_conv_backward_data_with_a_transposed_weight_copy():
    """default: the backward-data pass reads the layer's own kernel as its transpose (CONV_WT, every other conv test
    here); this is the other route — fc_transpose_weight + the plain operand — on a dense-table and a pair-list map"""
    import fcaf3d_amd.functional as Fn
    assert Fn.DGRAD_WT
    Fn.DGRAD_WT = False
    try:
        _conv_case(_dev(), 6000, 64, 128, 3, 1, 0, level_q=4)
        _conv_case(_dev(), 100000, 128, 64, 3, 1, 0, B=1)
        _conv_case(_dev(), 8000, 64, 128, 3, 2, 0, level_q=2)
    finally:
        Fn.DGRAD_WT = True


def test_conv_mfma_k3s2_and_k1s2():
    _conv_case(_dev(), 8000, 64, 128, 3, 2, 0, level_q=2)
    _conv_case(_dev(), 8000, 64, 64, 1, 2, 0, level_q=2)


@pytest.mark.parametrize('Cin,Cout,n,q', [(64, 64, 6000, 4), (128, 128, 6000, 4), (256, 256, 6000, 4), (64, 128, 100000, 1)])
def test_conv_fp32_mfma_route(Cin, Cout, n, q):
    """the fp32 MFMA kernels (v_mfma_f32_32x32x2_f32; FC_X6=0) stay a tested route.  What the route query says these shapes take, on
    their mask-sorted tables: 10.9k rows — an offset-split launch of 128-row tiles inside the 768...1536-workgroup band, so
    k_conv_glds forward and k_conv_mfma backward-data (the LDS-DMA image cannot be read transposed); 92.5k rows — unsplit,
    k_conv_mfma_p both ways; the weight gradients walk the pair lists on the fp32 kernels"""
    big = n > 50000
    fwd, dgrad = ('FC_FAM_MFMA_P', 'FC_FAM_MFMA_P') if big else ('FC_FAM_GLDS', 'FC_FAM_MFMA')
    _conv_case(_dev(), n, Cin, Cout, 3, 1, 0, level_q=q, B=1 if big else 2, x6=False,
               routes={'fwd': dict(family=fwd, bm=128, mode='FC_MODE_FP32', wsrc='FC_WSRC_FP32'),
                       'dgrad': dict(family=dgrad, bm=128, mode='FC_MODE_FP32', wsrc='FC_WSRC_FP32_T'),
                       'wgrad': dict(mode='FC_MODE_FP32', table='FC_TABLE_PAIRS')})


def test_split_bf16_convolution_sits_at_fp32_rounding_level_against_fp64():
    """csrc/conv_x6.h / wgrad_x6.h: fp32 products as six exact bf16 x bf16 products with fp32 accumulation.  Forward,
    backward-data and backward-weights of a 27-offset convolution against the SAME computation in fp64: both routes sit at
    fp32 rounding level (rms error 2...5e-8 of the output scale, fp32 epsilon = 6e-8); which one is closer depends on the
    pass (r3, 64->128 on ReLU-like inputs: forward 2.5e-8 vs 2.1e-8, backward-data 3.5e-8 vs 4.1e-8, backward-weights
    4.5e-8 vs 2.8e-8; tools/nbench on the 441k-row benchmark layers: forward 1.6e-7 vs 1.8e-7).  Bound: within 2x of the
    fp32 MFMA route and below 1e-7, on ReLU-like activations (half the inputs exactly zero) and on dense ones."""
    import fcaf3d_amd.functional as Fn
    from fcaf3d_amd.sparse import CoordMap
    dev = _dev()
    _, c_ref, _ = _scene_coords(11, n_points=60000, B=2)
    uc, _, _ = mo.unique_first(c_ref)
    cm, _, _ = CoordMap.from_coords(torch.from_numpy(uc).to(dev), 1, 2)
    km = cm.kernel_map(cm, 3)
    nbr = km.nbr.cpu().numpy()
    g = torch.Generator().manual_seed(3)
    for Cin, Cout, relu in ((64, 128, True), (128, 64, False)):
        x = torch.randn(len(uc), Cin, generator=g)
        if relu:
            x = x.clamp(min=0)
        w = torch.randn(27, Cin, Cout, generator=g) / np.sqrt(27 * Cin)
        go = torch.randn(len(uc), Cout, generator=g)
        x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
        out64 = mo.conv(x64, w64, nbr)
        gx64, gw64 = torch.autograd.grad(out64, [x64, w64], go.double())
        errs = {}
        for x6 in (True, False):
            Fn.X6 = x6
            try:
                xg, wg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
                out = Fn.sparse_conv(xg, wg, km, cm.n)
                gx, gw = torch.autograd.grad(out, [xg, wg], go.to(dev))
            finally:
                Fn.X6 = True
            errs[x6] = [float((a.double().cpu() - b).pow(2).mean().sqrt() / b.abs().max())
                        for a, b in ((out, out64.detach()), (gx, gx64), (gw, gw64))]
        print(f'{Cin}->{Cout} relu={relu}: rms error / scale vs fp64 (fwd, dgrad, wgrad): split-bf16 {errs[True]}, fp32 MFMA {errs[False]}')
        for e6, e32 in zip(errs[True], errs[False]):
            assert e6 <= 2.0 * e32 + 1e-9 and e6 < 1e-7, (errs[True], errs[False])


@pytest.mark.parametrize('Cin,Cout', [(64, 64), (64, 128)])
def test_conv_mfma_large_tiles(Cin, Cout):
    # 92.5k rows on the mask-sorted table: UNSPLIT launches (S = 1, statistics epilogue in the kernel) of 128-row tiles on the split
    # route through buffer descriptors — k_conv_x6 on 64-column tiles, k_conv_h3r on 128-column ones (conv_route.h takes 128-row
    # tiles from n > 64 and four tiles on, not from a row count) — and k_wgrad_x6t over the pair lists
    fam = {64: 'FC_FAM_X6', 128: 'FC_FAM_H3R'}
    _conv_case(_dev(), 100000, Cin, Cout, 3, 1, 0, B=1,
               routes={'fwd': dict(family=fam[Cout], bm=128, bn=Cout, s=1, mode='FC_MODE_H3', wsrc='FC_WSRC_IMAGE', buf=1, epi='FC_EPI_KERNEL'),
                       'dgrad': dict(family='FC_FAM_X6', bm=128, bn=64, s=1, mode='FC_MODE_H3', wsrc='FC_WSRC_IMAGE', buf=1),
                       'wgrad': dict(family='FC_WFAM_X6T', bm=64, bn=Cout, table='FC_TABLE_PAIRS', mode='FC_MODE_H3')})


_BM128, _BM256 = 2 << Fn.CONV_BM_SHIFT, 3 << Fn.CONV_BM_SHIFT


_PAIRS_FP32 = dict(table='FC_TABLE_PAIRS', mode='FC_MODE_FP32')
# The launch each flag of test_conv_kernel_variants_behind_flags is about, as the route query names it on that test's shapes.  The
# backward-data pass reads the kernel transposed, which k_conv_glds cannot: it stays on k_conv_mfma.  The layer's weight gradient
# walks the pair lists there, so FC_CONV_WGRAD_MULTI_OFF has nothing to switch (the dense-table kernels behind it:
# test_dense_table_weight_gradient_kernels, tests/test_gpu_conv_exact.py) and the pipe flags pick k_wgrad_mfma / k_wgrad_mfma_p.
_FLAG_ROUTES = {
    _BM256: {'fwd': dict(family='FC_FAM_GLDS', bm=256, bn=64, wm=4), 'dgrad': dict(family='FC_FAM_MFMA', bm=256, bn=64, wm=4)},
    Fn.CONV_WGRAD_MULTI_OFF: {'wgrad': dict(_PAIRS_FP32, ko=1)},
    Fn.CONV_PIPE_ON: {'fwd': dict(family='FC_FAM_MFMA_P', bm=128), 'dgrad': dict(family='FC_FAM_MFMA_P', bm=128)},
    Fn.CONV_PIPE_ON | _BM128: {'fwd': dict(family='FC_FAM_MFMA_P', bm=128), 'dgrad': dict(family='FC_FAM_MFMA_P', bm=128)},
    Fn.CONV_PIPE_ON | _BM256: {'fwd': dict(family='FC_FAM_MFMA_P', bm=256, bn=64), 'dgrad': dict(family='FC_FAM_MFMA_P', bm=256, bn=64)},
    Fn.CONV_GLDS: {'fwd': dict(family='FC_FAM_GLDS', bm=128), 'dgrad': dict(family='FC_FAM_MFMA', bm=128)},
    Fn.CONV_GLDS | _BM256: {'fwd': dict(family='FC_FAM_GLDS', bm=256, bn=64), 'dgrad': dict(family='FC_FAM_MFMA', bm=256, bn=64)},
    Fn.CONV_PIPE_OFF: {'fwd': dict(family='FC_FAM_MFMA', bm=128), 'dgrad': dict(family='FC_FAM_MFMA', bm=128)},
    Fn.CONV_WGRAD_PIPE_OFF: {'wgrad': dict(_PAIRS_FP32, family='FC_WFAM_MFMA')},
    Fn.CONV_WGRAD_PIPE_ON: {'wgrad': dict(_PAIRS_FP32, family='FC_WFAM_MFMA_P')},
    Fn.CONV_WGRAD_PIPE_OFF | Fn.CONV_WGRAD_MULTI_OFF: {'wgrad': dict(_PAIRS_FP32, family='FC_WFAM_MFMA', ko=1)},
}


@pytest.mark.parametrize('flags,what', [(_BM256, '256x64 LDS tile (4x1 waves)'),
                                        (Fn.CONV_WGRAD_MULTI_OFF, 'one-offset dense weight gradient'),
                                        (Fn.CONV_PIPE_ON, 'deeper-pipelined LDS kernel forced on'),
                                        (Fn.CONV_PIPE_ON | _BM128, 'deeper-pipelined LDS kernel, 128-row tiles'),
                                        (Fn.CONV_PIPE_ON | _BM256, 'deeper-pipelined LDS kernel, 256x64 tiles'),
                                        (Fn.CONV_GLDS, 'LDS-DMA kernel (global_load_lds, two stage buffers)'),
                                        (Fn.CONV_GLDS | _BM256, 'LDS-DMA kernel, 256x64 tiles'),
                                        (Fn.CONV_PIPE_OFF, 'r1 LDS kernel forced'), (Fn.CONV_WGRAD_PIPE_OFF, 'r1 weight-gradient kernel'),
                                        (Fn.CONV_WGRAD_PIPE_ON, 'pipelined weight-gradient kernel wherever it applies'),
                                        (Fn.CONV_WGRAD_PIPE_OFF | Fn.CONV_WGRAD_MULTI_OFF, 'r1 weight-gradient kernel, one offset per workgroup')])
def test_conv_kernel_variants_behind_flags(flags, what):
    """every flag-selected kernel variant (conv.hip; the defaults are chosen by measurement) against the oracle,
    forward + backward-data + backward-weights, on a strided and an unstrided map (15.4k result rows each: offset-split launches on
    the mask-sorted tables, weight gradients over the pair lists).  _FLAG_ROUTES: what the route query must say the flag did there"""
    _conv_case(_dev(), 9000, 64, 128, 3, 1, flags, level_q=4, x6=False, routes=_FLAG_ROUTES[flags])
    _conv_case(_dev(), 9000, 64, 64, 3, 2, flags, level_q=2, x6=False, routes=_FLAG_ROUTES[flags])


def test_pair_list_convolution_linear_live_tile_launch():
    """fc_conv_fwd_pairs_tiles (3-D grid and the linear list of live (offset, tile) workgroups) == the generic FMA kernel
    (CONV_FMA; itself checked against the oracle by the tests above — a transitive check, stated here on purpose)."""
    from fcaf3d_amd import _lib as L
    from fcaf3d_amd.sparse import CoordMap
    dev = _dev()
    _, c_ref, _ = _scene_coords(21, n_points=20000, B=2)
    c_ref = c_ref.copy(); c_ref[:, 1:] = np.floor_divide(c_ref[:, 1:], 4) * 4
    uc, _, _ = mo.unique_first(c_ref)
    cm, _, _ = CoordMap.from_coords(torch.from_numpy(uc).to(dev), 4, 2)
    km = cm.kernel_map(cm, 3)
    n, K = cm.n, 27
    for Cin, Cout in ((64, 128), (128, 64)):
        g = torch.Generator().manual_seed(1)
        x = torch.randn(n, Cin, generator=g).to(dev)
        w = (torch.randn(K, Cin, Cout, generator=g) / np.sqrt(Cin * K)).to(dev)
        ref = torch.empty(n, Cout, device=dev)
        L.call('fc_conv_fwd', L.ptr(x), L.ptr(w), L.ptr(km.nbr), None, L.ptr(ref), n, n, K, Cin, Cout, 1, None, 0, L.stream())
        pi, _, pos, cnt = km.pairs()
        for live in (0, km.pair_tiles()):
            out = torch.full((n, Cout), float('nan'), device=dev)
            ws = L.workspace(L.query('fc_conv_fwd_pairs_ws_bytes', n, K, Cout), dev)
            L.call('fc_conv_fwd_pairs_tiles', L.ptr(x), L.ptr(w), L.ptr(pi), L.ptr(cnt), L.ptr(pos), L.ptr(out), n, n, K, Cin, Cout,
                   live, 0, L.ptr(ws), ws.numel(), L.stream())
            _close(out, ref.cpu(), what=f'pair conv live_tiles={live}')


@pytest.mark.parametrize('Cin,Cout', [(64, 64), (128, 128), (256, 128), (128, 64)])
def test_dense_table_weight_gradient_kernels(Cin, Cout):
    """fc_conv_wgrad over a dense neighbour table: the multi-offset kernel (default from 4096 rows), the one-offset kernels
    (CONV_WGRAD_MULTI_OFF, and with CONV_WGRAD_PIPE_OFF) and the row-range split override == the generic FMA kernel (CONV_FMA)."""
    from fcaf3d_amd import _lib as L
    from fcaf3d_amd.sparse import CoordMap
    dev = _dev()
    _, c_ref, _ = _scene_coords(23, n_points=30000, B=2)
    c_ref = c_ref.copy(); c_ref[:, 1:] = np.floor_divide(c_ref[:, 1:], 2) * 2
    uc, _, _ = mo.unique_first(c_ref)
    cm, _, _ = CoordMap.from_coords(torch.from_numpy(uc).to(dev), 2, 2)
    km = cm.kernel_map(cm, 3)
    n, K = cm.n, 27
    assert n >= 4096
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n, Cin, generator=g).to(dev)
    go = torch.randn(n, Cout, generator=g).to(dev)

    def run(flags):
        gw = torch.full((K, Cin, Cout), float('nan'), device=dev)
        ws = L.workspace(max(L.query('fc_conv_wgrad_ws_bytes', n, K, Cin, Cout, flags), 16), dev)
        L.call('fc_conv_wgrad', L.ptr(x), L.ptr(go), L.ptr(km.nbr), None, L.ptr(gw), n, n, K, Cin, Cout, flags, L.ptr(ws), ws.numel(),
               L.stream())
        return gw.cpu()
    ref = run(Fn.CONV_FMA)
    off, s = Fn.CONV_WGRAD_MULTI_OFF, Fn.CONV_S_SHIFT
    for fl in (0, off, off | Fn.CONV_WGRAD_PIPE_OFF, Fn.CONV_WGRAD_MULTI_FIRST, 3 << s, (5 << s) | off):
        got = run(fl)
        _close(got, ref, what=f'dense-table wgrad {Cin}->{Cout} flags={fl:#x}')
        assert torch.equal(got, run(fl)), f'weight gradient not repeatable bit for bit, flags={fl:#x}'


@pytest.mark.parametrize('n_points,B', [(5000, 2), (150000, 1)])
def test_stem_convolution_both_weight_gradient_routes(n_points, B):
    """the 3 -> 64 k3s2 stem on the matrix cores (k_stem_fwd): default = the forward saves the gathered inputs (col) and the
    weight gradient streams them (fc_stem_conv_fwd / fc_stem_conv_wgrad); FC_STEM_COL=0 = gathers in both passes
    (fc_conv_fwd / fc_conv_wgrad).  Both against the oracle, one split and one many-split launch."""
    import fcaf3d_amd.functional as Fn
    assert Fn.STEM_COL
    _conv_case(_dev(), n_points, 3, 64, 3, 2, 0, B=B)
    Fn.STEM_COL = False
    try:
        _conv_case(_dev(), n_points, 3, 64, 3, 2, 0, B=B)
    finally:
        Fn.STEM_COL = True


@pytest.mark.parametrize('Cin,Cout,ks,s', [(3, 64, 3, 2), (64, 64, 3, 1), (16, 24, 3, 1)])
def test_conv_generic_fma(Cin, Cout, ks, s):
    _conv_case(_dev(), 4000, Cin, Cout, ks, s, 1, level_q=2)


def test_conv_identity_dense_gemm():
    import fcaf3d_amd.functional as Fn
    dev = _dev()
    g = torch.Generator().manual_seed(1)
    for n, Cin, Cout in ((1000, 128, 512), (70000, 128, 64), (333, 64, 64), (5, 512, 2048)):
        x = torch.randn(n, Cin, generator=g); w = torch.randn(1, Cin, Cout, generator=g) / 10
        go = torch.randn(n, Cout, generator=g)
        xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
        out_r = xr @ wr[0]
        gx_r, gw_r = torch.autograd.grad(out_r, [xr, wr], go)
        xg = x.to(dev).requires_grad_(True); wg = w.to(dev).requires_grad_(True)
        out_g = Fn.sparse_conv(xg, wg, None, n)
        gx_g, gw_g = torch.autograd.grad(out_g, [xg, wg], go.to(dev))
        _close(out_g, out_r, what=f'gemm {n}x{Cin}x{Cout} fwd')
        _close(gx_g, gx_r, what='gemm dgrad'); _close(gw_g, gw_r, what='gemm wgrad')


@pytest.mark.parametrize('C,nseg,act,res', [(64, 1, 'relu', False), (64, 1, 'relu', True), (128, 1, 'elu', False),
                                            (512, 1, None, False), (64, 3, 'relu', False), (256, 1, 'elu', True)])
def test_norm_act(C, nseg, act, res):
    import fcaf3d_amd.functional as Fn
    dev = _dev()
    g = torch.Generator().manual_seed(2)
    n = 5003
    x = torch.randn(n, C, generator=g) * 2 + 0.5
    gamma = torch.rand(C, generator=g) + 0.5; beta = torch.randn(C, generator=g)
    r = torch.randn(n, C, generator=g) if res else None
    go = torch.randn(n, C, generator=g)
    b = np.sort(np.random.default_rng(0).integers(0, nseg, n)).astype(np.int32)
    coords = np.zeros((n, 4), np.int32); coords[:, 0] = b
    eps = 1e-8 if nseg > 1 else 1e-5
    xr = x.clone().requires_grad_(True); gr = gamma.clone().requires_grad_(True); br = beta.clone().requires_grad_(True)
    rr = r.clone().requires_grad_(True) if res else None
    if nseg > 1:
        y = mo.instance_norm(xr, b, gr[None], br[None], eps)
    else:
        y = mo.batch_norm(xr, gr, br, eps)
    if res:
        y = y + rr
    y = {'relu': torch.relu, 'elu': torch.nn.functional.elu, None: lambda t: t}[act](y)
    grads_r = torch.autograd.grad(y, [xr, gr, br] + ([rr] if res else []), go)
    xg = x.to(dev).requires_grad_(True); gg = gamma.to(dev).requires_grad_(True); bg = beta.to(dev).requires_grad_(True)
    rg = r.to(dev).requires_grad_(True) if res else None
    seg = torch.from_numpy(coords).to(dev) if nseg > 1 else None
    yg, stats = Fn.norm_act(xg, gg, bg, residual=rg, seg=seg, nseg=nseg, eps=eps, act=act)
    grads_g = torch.autograd.grad(yg, [xg, gg, bg] + ([rg] if res else []), go.to(dev))
    _close(yg, y, what='norm fwd')
    for a, bb, nm in zip(grads_g, grads_r, ['gx', 'ggamma', 'gbeta', 'gres']):
        _close(a, bb, tol=2e-4, what=f'norm {nm} C={C} nseg={nseg}')
    _close(stats[0], torch.stack([x[torch.from_numpy(b.astype(np.int64)) == s].mean(0) for s in range(nseg)]), what='mean')


def test_maxpool():
    import fcaf3d_amd.functional as Fn
    from fcaf3d_amd.sparse import CoordMap
    dev = _dev()
    _, c_ref, _ = _scene_coords(7, n_points=8000)
    uc, _, _ = mo.unique_first(c_ref)
    out_c = mo.stride_coords(uc, 1, 2)
    nbr = mo.kernel_map(uc, out_c, mo.kernel_offsets(2, 1))
    x = torch.randn(len(uc), 64)
    xr = x.clone().requires_grad_(True)
    y = mo.max_pool(xr, nbr)
    go = torch.randn_like(y)
    gx_r, = torch.autograd.grad(y, xr, go)
    cm, _, _ = CoordMap.from_coords(torch.from_numpy(uc).to(dev), 1, 2)
    km = cm.kernel_map(cm.strided(2), 2)
    xg = x.to(dev).requires_grad_(True)
    yg = Fn.max_pool(xg, km)
    gx_g, = torch.autograd.grad(yg, xg, go.to(dev))
    assert torch.equal(yg.cpu(), y.detach())
    assert torch.equal(gx_g.cpu(), gx_r)


def test_generate_union_interp_prune():
    import fcaf3d_amd.functional as Fn
    from fcaf3d_amd.sparse import CoordMap, SparseTensor, compact_mask
    dev = _dev()
    _, c_ref, _ = _scene_coords(9, n_points=6000)
    c4 = c_ref.copy(); c4[:, 1:] = np.floor_divide(c4[:, 1:], 4) * 4
    fine, _, _ = mo.unique_first(c4)                       # stride 4 (backbone level)
    coarse = mo.stride_coords(fine, 4, 2)                  # stride 8
    # drop some coarse voxels so that the union really adds rows
    keep = np.random.default_rng(1).random(len(coarse)) < 0.7
    coarse_p = coarse[keep]
    gen_ref = mo.gen_conv_transpose_coords(coarse_p, 8)
    cmc, _, _ = CoordMap.from_coords(torch.from_numpy(coarse_p).to(dev), 8, 2)
    gen = cmc.generate()
    assert gen.stride == 4 and np.array_equal(gen.coords.cpu().numpy(), gen_ref)
    fa = torch.randn(len(fine), 8); fb = torch.randn(len(gen_ref), 8)
    far = fa.clone().requires_grad_(True); fbr = fb.clone().requires_grad_(True)
    uc_ref, uf_ref = mo.union_add(fine, far, gen_ref, fbr)
    go = torch.randn_like(uf_ref)
    ga_r, gb_r = torch.autograd.grad(uf_ref, [far, fbr], go)
    cmf, _, _ = CoordMap.from_coords(torch.from_numpy(fine).to(dev), 4, 2)
    fag = fa.to(dev).requires_grad_(True); fbg = fb.to(dev).requires_grad_(True)
    u = SparseTensor(fag, coordinate_map_key=cmf) + SparseTensor(fbg, coordinate_map_key=gen)
    assert len(uc_ref) > len(fine)
    assert np.array_equal(u.C.cpu().numpy(), uc_ref)
    ga_g, gb_g = torch.autograd.grad(u.F, [fag, fbg], go.to(dev))
    assert torch.equal(u.F.detach().cpu(), uf_ref.detach())
    assert torch.equal(ga_g.cpu(), ga_r) and torch.equal(gb_g.cpu(), gb_r)
    # the same union in CANONICAL order against a coordinate-keyed sum that shares no row-order rule with either
    # implementation (np.unique over the concatenated sets + np.add.at): the oracle cannot drift together with the product
    uniq, inv = np.unique(np.concatenate([fine, gen_ref]), axis=0, return_inverse=True)
    dense = np.zeros((len(uniq), 8), np.float64)
    np.add.at(dense, inv.reshape(-1), np.concatenate([fa.numpy(), fb.numpy()]).astype(np.float64))
    ucg = u.C.cpu().numpy()
    so = np.lexsort(ucg.T[::-1])
    assert np.array_equal(ucg[so], uniq)
    assert np.abs(u.F.detach().cpu().numpy()[so].astype(np.float64) - dense).max() <= 1e-6
    # interpolation of a 1-channel coarse tensor at the union coordinates
    sc = torch.randn(len(coarse_p), 1)
    ref = mo.features_at_coordinates(coarse_p, sc, 8, uc_ref.astype(np.float32))
    got = SparseTensor(sc.to(dev), coordinate_map_key=cmc).features_at_coordinates(u.C.float())
    _close(got, ref, tol=1e-6, what='interp')
    # prune
    mask = np.random.default_rng(2).random(len(uc_ref)) < 0.4
    pc_ref, pf_ref = mo.prune(uc_ref, uf_ref.detach(), mask)
    kept = compact_mask(torch.from_numpy(mask).to(dev))
    assert np.array_equal(kept.cpu().numpy(), np.nonzero(mask)[0])
    pm = u.cmap.pruned(kept)
    assert np.array_equal(pm.coords.cpu().numpy(), pc_ref)
    pf = Fn.gather_rows(u.F, kept)
    assert torch.equal(pf.detach().cpu(), pf_ref)
    perms = pm.decomposition_permutations
    assert sum(len(p) for p in perms) == pm.n


def test_generated_set_maps_by_index_arithmetic_equal_hashed_sets_of_the_same_rows():
    """r3: the k3 kernel map of a generated children set (fc_kernel_map_children, from the parent level's table) and the
    rows of a backbone level inside it (fc_child_rows, from the parent level's hash) against (a) the generic hash-probe
    path on sets over the same coordinates built by CoordMap.from_coords (no parent link: fc_kernel_map / the union probe)
    and (b) the oracle's kernel map — exact; two generations deep, as the neck chains them; and a union that really adds
    rows still takes the generic path."""
    from fcaf3d_amd.sparse import CoordMap
    dev = _dev()
    _, c_ref, _ = _scene_coords(13, n_points=8000)
    c16 = c_ref.copy(); c16[:, 1:] = np.floor_divide(c16[:, 1:], 16) * 16
    top, _, _ = mo.unique_first(c16)                                   # stride 16
    c8 = c_ref.copy(); c8[:, 1:] = np.floor_divide(c8[:, 1:], 8) * 8
    mid, _, _ = mo.unique_first(c8)                                    # stride 8: every voxel lies in a child of `top`

    def build(structured):
        cm_top, _, _ = CoordMap.from_coords(torch.from_numpy(top).to(dev), 16, 2)
        g1 = cm_top.generate()
        if not structured:                                             # the same rows, hashed: no _gen_parent
            g1, _, _ = CoordMap.from_coords(g1.coords.clone(), 8, 2)
        cm_mid, _, _ = CoordMap.from_coords(torch.from_numpy(mid).to(dev), 8, 2)
        u, rows, swapped = cm_mid.union(g1)
        g2 = u.generate()
        if not structured:
            g2, _, _ = CoordMap.from_coords(g2.coords.clone(), 4, 2)
        assert (g1._gen_parent is not None) == (g2._gen_parent is not None) == structured
        return (g1.kernel_map(g1, 3).nbr.cpu().numpy(), rows.cpu().numpy(), swapped, u is g1,
                g2.kernel_map(g2, 3).nbr.cpu().numpy(), g1.coords.cpu().numpy(), g2.coords.cpu().numpy(), g1._keys is None)
    a = build(True)
    b = build(False)
    assert a[2] and a[3] and b[2] and b[3], 'the strided level lies inside the generated set'
    assert a[7] and not b[7], 'structured path must not build the generated set\'s hash; the generic path does'
    for x, y in zip(a[:7], b[:7]):
        assert np.array_equal(x, y)
    g1_ref = mo.gen_conv_transpose_coords(top, 16)
    assert np.array_equal(a[5], g1_ref)
    assert np.array_equal(a[0], mo.kernel_map(g1_ref, g1_ref, mo.kernel_offsets(3, 8)))
    g2_ref = mo.gen_conv_transpose_coords(g1_ref, 8)
    assert np.array_equal(a[4], mo.kernel_map(g2_ref, g2_ref, mo.kernel_offsets(3, 4)))
    # rows: where each stride-8 voxel sits in g1
    lut = {tuple(c): i for i, c in enumerate(g1_ref.tolist())}
    assert np.array_equal(a[1], np.array([lut[tuple(c)] for c in mid.tolist()], np.int32))
    # a level with a voxel OUTSIDE the generated set: generic union (rows appended)
    extra = np.concatenate([mid, np.array([[0, 4000, 4000, 4000]], np.int32)])
    cm_top, _, _ = CoordMap.from_coords(torch.from_numpy(top).to(dev), 16, 2)
    g1 = cm_top.generate()
    cm_x, _, _ = CoordMap.from_coords(torch.from_numpy(extra).to(dev), 8, 2)
    u, rows, swapped = cm_x.union(g1)
    uc_ref, _ = mo.union_add(extra, torch.zeros(len(extra), 1), g1_ref, torch.zeros(len(g1_ref), 1))
    assert not swapped and np.array_equal(u.coords.cpu().numpy(), uc_ref)


def test_no_cpu_fallback():
    import fcaf3d_amd.functional as Fn
    with pytest.raises(RuntimeError):
        Fn.sparse_conv(torch.zeros(4, 64), torch.zeros(1, 64, 64), None, 4)


@pytest.mark.parametrize('n,C,act,res', [(5003, 64, 'relu', True), (853, 512, 'elu', False), (70, 128, None, False),
                                         (1500, 256, 'relu', True), (14884, 128, 'relu', True),
                                         (40000, 256, 'elu', False)])      # last one: > 4M elements -> six-launch path
# (ELU there: with ReLU one of the 10M pre-activations lands within 1 ulp of 0 and the 0/1 derivative flips)
def test_bn_train_fused_paths(n, C, act, res):
    """Training-mode BatchNorm (two-launch small path and the general path): output, gradients and the
    nn.BatchNorm1d buffer update against torch on the CPU."""
    import fcaf3d_amd.functional as Fn
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, C, generator=g) * 3 + 1.5
    gamma = torch.rand(C, generator=g) + 0.5; beta = torch.randn(C, generator=g)
    r = torch.randn(n, C, generator=g) if res else None
    go = torch.randn(n, C, generator=g)
    bn = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    xr = x.clone().requires_grad_(True); rr = r.clone().requires_grad_(True) if res else None
    y = bn(xr)
    if res:
        y = y + rr
    y = {'relu': torch.relu, 'elu': torch.nn.functional.elu, None: lambda t: t}[act](y)
    grads_r = torch.autograd.grad(y, [xr, bn.weight, bn.bias] + ([rr] if res else []), go)
    xg = x.to(dev).requires_grad_(True); gg = gamma.to(dev).requires_grad_(True); bg = beta.to(dev).requires_grad_(True)
    rg = r.to(dev).requires_grad_(True) if res else None
    rmean = torch.zeros(C, device=dev); rvar = torch.ones(C, device=dev); nbt = torch.zeros((), dtype=torch.long, device=dev)
    yg, (mean, var, cnt) = Fn.bn_train(xg, gg, bg, rg, 1e-5, act, 0.1, rmean, rvar, nbt)
    grads_g = torch.autograd.grad(yg, [xg, gg, bg] + ([rg] if res else []), go.to(dev))
    _close(yg, y, what='bn fwd')
    for a, b, nm in zip(grads_g, grads_r, ['gx', 'ggamma', 'gbeta', 'gres']):
        _close(a, b, tol=2e-4, what=f'bn {nm} n={n} C={C}')
    _close(rmean, bn.running_mean, tol=1e-5, what='running_mean')
    _close(rvar, bn.running_var, tol=1e-5, what='running_var')
    assert int(nbt) == 1 and float(cnt[0]) == n
    _close(mean[0], x.mean(0), tol=1e-5, what='batch mean')
    _close(var[0], x.var(0, unbiased=False), tol=1e-5, what='batch var')


def test_sort_v_matches_restatement():
    """standalone sort_v (Rotated_IoU cuda_ext, box_intersection_2d.py:147): indices bit-exact vs the Appendix-D
    restatement on random rotated pairs, and the shoelace area of the selected polygon equals the IoU kernel's."""
    from fcaf3d_amd.losses import sort_v
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    n = 4000
    b1 = torch.cat([torch.rand(n, 2, generator=g) * 2, torch.rand(n, 2, generator=g) * 2 + 0.3,
                    (torch.rand(n, 1, generator=g) - 0.5) * 6.28], 1)
    b2 = torch.cat([b1[:, :2] + (torch.rand(n, 2, generator=g) - 0.5) * 1.5, torch.rand(n, 2, generator=g) * 2 + 0.3,
                    (torch.rand(n, 1, generator=g) - 0.5) * 6.28], 1)
    b2[:50] = b1[:50]                                   # identical boxes: every corner listed twice
    b2[50:100, :2] += 10.0                              # disjoint: fewer than 3 valid vertices
    verts, mask = lo.intersection_vertices(b1, b2)
    nv = mask.sum(1).int()
    ctr = (verts * mask[..., None]).sum(1, keepdim=True) / nv.clamp(min=1)[:, None, None]
    vc = (verts - ctr) * mask[..., None]
    want = lo.sort_v(vc[None].numpy(), mask[None].numpy(), nv[None].numpy())[0]
    got = sort_v(vc[None].to(dev), mask[None].to(dev), nv[None].to(dev))[0].cpu().numpy()
    # the angular key is built from +, *, / in float32 on both sides (no libm): every index of every pair is equal
    assert np.array_equal(want, got), float((want == got).all(1).mean())
    sel = np.take_along_axis(vc.numpy(), got[:, :, None].astype(np.int64), 1)
    area = np.abs((sel[:, :-1, 0] * sel[:, 1:, 1] - sel[:, :-1, 1] * sel[:, 1:, 0]).sum(1)) / 2
    sel_w = np.take_along_axis(vc.numpy(), want[:, :, None].astype(np.int64), 1)
    area_w = np.abs((sel_w[:, :-1, 0] * sel_w[:, 1:, 1] - sel_w[:, :-1, 1] * sel_w[:, 1:, 0]).sum(1)) / 2
    assert np.abs(area - area_w).max() < 1e-5
    assert (got[50:100] >= 8).all() and (got[50:100] == got[50:100, :1]).all()     # all pad


@pytest.mark.parametrize('n_reg,n_cls', [(6, 18), (8, 10), (6, 5)])
def test_head_split_matches_torch(n_reg, n_cls):
    """fused head epilogue (fcaf3d_neck_with_head.py:256-279) == the slice / exp(scale*reg) / +bias / max torch ops,
    values and gradients (y, bias, scale)"""
    import fcaf3d_amd.functional as Fn
    dev = _dev()
    g = torch.Generator().manual_seed(n_reg + n_cls)
    n = 5003
    y = torch.randn(n, 64, generator=g)
    bias = torch.randn(1, n_cls, generator=g)
    scale = torch.tensor(1.3)
    go = [torch.randn(n, 1, generator=g), torch.randn(n, n_reg, generator=g), torch.randn(n, n_cls, generator=g)]

    def ref(y, bias, scale):
        reg = y[:, 1:1 + n_reg]
        cls = y[:, 1 + n_reg:1 + n_reg + n_cls] + bias
        return y[:, :1], torch.cat((torch.exp(reg[:, :6] * scale), reg[:, 6:]), 1), cls
    yr, br, sr = y.clone().requires_grad_(True), bias.clone().requires_grad_(True), scale.clone().requires_grad_(True)
    outs_r = ref(yr, br, sr)
    grads_r = torch.autograd.grad(outs_r, [yr, br, sr], go)
    yg, bg, sg = (t.clone().to(dev).requires_grad_(True) for t in (y, bias, scale))
    c, b, s, m = Fn.head_split(yg, bg, sg, n_reg, n_cls)
    grads_g = torch.autograd.grad((c, b, s), [yg, bg, sg], [t.to(dev) for t in go])
    for a, r_, what in zip((c, b, s), outs_r, ('centerness', 'bbox', 'cls')):
        _close(a, r_, what='head ' + what)
    assert torch.equal(m.cpu(), outs_r[2].max(1, keepdim=True).values.detach())
    assert not m.requires_grad
    for a, r_, what in zip(grads_g, grads_r, ('gy', 'gbias', 'gscale')):
        _close(a, r_, what='head ' + what)


def test_empty_and_degenerate_inputs():
    """edge cases through the C ABI: zero rows, a one-voxel map (26 of 27 offsets have no pair: the pair-list
    paths see empty lists), empty NMS / IoU / head / sort_v calls"""
    import fcaf3d_amd.functional as Fn
    from fcaf3d_amd import _lib as L
    from fcaf3d_amd.losses import sort_v
    from fcaf3d_amd.nms import boxes_iou_bev, nms_bev, pcdet_nms_gpu
    from fcaf3d_amd.sparse import CoordMap
    dev = _dev()
    # conv / wgrad with zero output rows
    x = torch.randn(5, 64, device=dev); w = torch.randn(27, 64, 64, device=dev)
    nbr = torch.empty((27, 0), dtype=torch.int32, device=dev)
    out = torch.empty((0, 64), device=dev)
    L.call('fc_conv_fwd', L.ptr(x), L.ptr(w), L.ptr(nbr), None, L.ptr(out), 5, 0, 27, 64, 64, 0, None, 0, L.stream())
    gw = torch.full_like(w, 7.0)
    L.call('fc_conv_wgrad', L.ptr(x), L.ptr(out), L.ptr(nbr), None, L.ptr(gw), 5, 0, 27, 64, 64, 0, None, 0, L.stream())
    assert float(gw.abs().max()) == 0.0
    # one voxel per scene, two scenes: only the centre offset has pairs
    uc = np.array([[0, 4, 8, 12], [1, -4, 0, 4]], np.int32)
    cm, _, _ = CoordMap.from_coords(torch.from_numpy(uc).to(dev), 4, 2)
    km = cm.kernel_map(cm, 3)
    assert km.use_pairs
    pi, po, pos, cnt = (t.cpu().numpy() for t in km.pairs())
    assert cnt.tolist() == [0] * 13 + [2] + [0] * 13 and po[13, :2].tolist() == [0, 1] and (pos[13] == [0, 1]).all()
    g = torch.Generator().manual_seed(0)
    xf = torch.randn(2, 64, generator=g); wf = torch.randn(27, 64, 128, generator=g); go = torch.randn(2, 128, generator=g)
    xr, wr = xf.clone().requires_grad_(True), wf.clone().requires_grad_(True)
    ref = mo.conv(xr, wr, mo.kernel_map(uc, uc, mo.kernel_offsets(3, 4)))
    gx_r, gw_r = torch.autograd.grad(ref, [xr, wr], go)
    xg, wg = xf.to(dev).requires_grad_(True), wf.to(dev).requires_grad_(True)
    got = Fn.sparse_conv(xg, wg, km, 2)                       # pair mode (2 rows <= PAIR_CONV_ROWS)
    gx_g, gw_g = torch.autograd.grad(got, [xg, wg], go.to(dev))
    _close(got, ref, what='1-voxel conv'); _close(gx_g, gx_r, what='1-voxel dgrad'); _close(gw_g, gw_r, what='1-voxel wgrad')
    assert float(gw_g[:13].abs().max()) == 0.0 and float(gw_g[14:].abs().max()) == 0.0
    # empty NMS / IoU / head epilogue / sort_v
    eb = torch.zeros((0, 7), device=dev); es = torch.zeros(0, device=dev)
    assert nms_bev(eb, es, 0.5).numel() == 0 and pcdet_nms_gpu(eb, es, 0.5)[0].numel() == 0
    assert boxes_iou_bev(eb, torch.rand(3, 7, device=dev)).shape == (0, 3)
    c, b, s, m = Fn.head_split(torch.zeros((0, 64), device=dev), torch.zeros(1, 18, device=dev), torch.tensor(1.0, device=dev), 6, 18)
    assert c.shape == (0, 1) and b.shape == (0, 6) and s.shape == (0, 18) and m.shape == (0, 1)
    idx = sort_v(torch.zeros((1, 0, 24, 2), device=dev), torch.zeros((1, 0, 24), dtype=torch.bool, device=dev),
                 torch.zeros((1, 0), dtype=torch.int32, device=dev))
    assert idx.shape == (1, 0, 9)
    torch.cuda.synchronize()


# ---- r5: BatchNorm statistics out of the convolution's epilogue, two-consumer gradient add inside the BatchNorm backward ----------
def _stats_case(dev, n_points, Cin, Cout, level_q, seed, B=2):
    """-> (x, weight, kernel map, coordinate map) of a k3 s1 convolution on a synthetic level"""
    from fcaf3d_amd.sparse import CoordMap
    _, c_ref, _ = _scene_coords(seed, n_points=n_points, B=B)
    if level_q > 1:
        c_ref = c_ref.copy(); c_ref[:, 1:] = np.floor_divide(c_ref[:, 1:], level_q) * level_q
    uc, _, _ = mo.unique_first(c_ref)
    cm, _, _ = CoordMap.from_coords(torch.from_numpy(uc).to(dev), level_q, B)
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(len(uc), Cin, generator=g) + 0.5).to(dev)
    w = (torch.randn(27, Cin, Cout, generator=g) / np.sqrt(Cin * 27)).to(dev)
    return x, w, cm.kernel_map(cm, 3), cm


@pytest.mark.parametrize('n_points,Cin,Cout,q,route', [
    # what the route query says (fc_conv_fwd_route | FC_TABLE_STATS; the labels are the test ids and stay as they were):
    (100000, 64, 64, 4, 'tile epilogue'),           # 62.4k rows: unsplit k_conv_x6 on the mask-sorted table, epilogue in the kernel
    (100000, 128, 128, 8, 'pair lists'),            # 15.4k rows, above PAIR_CONV_ROWS since r6: offset-split (S = 8) k_conv_h3r on the
                                                    # mask-sorted table, k_sum_parts_stats — no longer a pair-list launch
    (100000, 256, 256, 16, 'pair lists, 64-row blocks'),   # 3.6k rows: per offset over the pair lists, k_sum_pairs_stats
    (100000, 256, 256, 32, 'pair lists, few rows'),  # 870 rows: the same, <= 64 row blocks of 16 rows
])
def test_conv_statistics_epilogue(n_points, Cin, Cout, q, route):
    """fc_conv_fwd_stats / fc_conv_fwd_pairs_tiles_stats: the result is bit for bit the plain launch's, and the table holds the
    column sums of the result and of its square (fp32 sums per row block; checked against fp64 over the result to 2e-6)"""
    import fcaf3d_amd.functional as Fn
    dev = _dev()
    x, w, km, cm = _stats_case(dev, n_points, Cin, Cout, q, seed=17)
    with torch.no_grad():
        ref = Fn.sparse_conv(x, w, km, cm.n)
        out, tab = Fn.sparse_conv(x, w, km, cm.n, True, want_stats=True)
    assert tab is not None, 'this launch must have a statistics epilogue'
    assert torch.equal(out, ref), route
    o = out.double()
    s1, s2 = tab[:, 0].double().sum(0), tab[:, 1].double().sum(0)
    print(f'{route}: n = {cm.n}, row blocks = {tab.shape[0]}')
    assert float((s1 - o.sum(0)).abs().max()) <= 2e-6 * float(o.abs().sum(0).max())
    assert float((s2 - (o * o).sum(0)).abs().max()) <= 2e-6 * float((o * o).sum(0).max())


@pytest.mark.parametrize('ratio,bound', [(3.0, 2e-5), (30.0, 5e-4), (1000.0, 2e-1)])
def test_epilogue_statistics_with_a_large_mean(ratio, bound):
    """the BatchNorm statistics that come out of the convolution epilogues are E[x^2] - mean^2 over fp32 sums per row
    block (combined in fp64, norm.hip bn2_stats), where torch.nn.BatchNorm1d centres first.  For channels with |mean| >> std the
    subtraction cancels: this pins HOW MUCH, against fp64 — at the |mean| / std the network's pre-normalisation activations show
    (O(1): convolution outputs of normalised inputs) the variance agrees to 2e-5, at 30 to 5e-4, and at 1e3 it is good to a few per
    cent only (known limitation; a shifted sum in the epilogue would remove it)."""
    import fcaf3d_amd.functional as Fn
    dev = _dev()
    n, C, rb = 20000, 64, 128
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(n, C, generator=g) + ratio).to(dev)
    blocks = (n + rb - 1) // rb
    pad = torch.zeros(blocks * rb - n, C, device=dev)
    xb = torch.cat((x, pad)).view(blocks, rb, C)
    tab = torch.stack((xb.sum(1), (xb * xb).sum(1)), dim=1).contiguous()          # what an epilogue leaves: fp32 sums per row block
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    rmean = torch.zeros(C, device=dev); rvar = torch.ones(C, device=dev); nbt = torch.zeros((), dtype=torch.long, device=dev)
    y, (mean, var, cnt) = Fn.bn_train(x, gamma, beta, None, 1e-5, None, 0.1, rmean, rvar, nbt, part=tab)
    x64 = x.double()
    m64, v64 = x64.mean(0), x64.var(0, unbiased=False)
    e_m = float(((mean[0].double() - m64).abs() / m64.abs()).max())
    e_v = float(((var[0].double() - v64).abs() / v64).max())
    y64 = (x64 - m64) / torch.sqrt(v64 + 1e-5)
    e_y = float((y.double() - y64).abs().max())
    print(f'|mean| / std = {ratio:g}: mean {e_m:.1e}, variance {e_v:.1e} (relative), normalised output {e_y:.1e} (absolute) against fp64')
    assert e_m < 1e-6 and e_v < bound, (ratio, e_m, e_v)


def test_offset_split_statistics_epilogue_and_dense_gemm_groups():
    """the two remaining producers: an offset-split launch (few rows on a DENSE map: k_sum_parts_stats) and the table-free dense
    GEMM of a generative transposed convolution, whose (n, 8 C) result is normalised as (8 n, C): 8 column groups per channel"""
    import fcaf3d_amd.functional as Fn
    from fcaf3d_amd.sparse import CoordMap
    dev = _dev()
    x, w, km, cm = _stats_case(dev, 12000, 256, 256, 32, seed=19)
    g = cm.generate()                                             # children set: 94 % dense, ~8k rows -> offset split
    kg = g.kernel_map(g, 3)
    assert not kg.use_pairs
    xg = torch.randn(g.n, 128, device=dev)
    wg = torch.randn(27, 128, 128, device=dev) / 60.0
    with torch.no_grad():
        ref = Fn.sparse_conv(xg, wg, kg, g.n)
        out, tab = Fn.sparse_conv(xg, wg, kg, g.n, True, want_stats=True)
    assert tab is not None and torch.equal(out, ref)
    o = out.double()
    assert float((tab[:, 0].double().sum(0) - o.sum(0)).abs().max()) <= 2e-6 * float(o.abs().sum(0).max())
    assert float((tab[:, 1].double().sum(0) - (o * o).sum(0)).abs().max()) <= 2e-6 * float((o * o).sum(0).max())
    # dense GEMM (n, 256) x (256, 8 * 64) + BatchNorm over (8 n, 64) from the table, against BatchNorm from the matrix itself
    import fcaf3d_amd.nn as MEnn
    torch.manual_seed(3)
    gen = MEnn.MinkowskiGenerativeConvolutionTranspose(256, 64).to(dev).train()
    bn_a, bn_b = MEnn.MinkowskiBatchNorm(64).to(dev).train(), MEnn.MinkowskiBatchNorm(64).to(dev).train()
    from fcaf3d_amd.sparse import SparseTensor
    xin = SparseTensor(x, coordinate_map_key=cm)
    t = gen(xin, want_stats=True)
    assert getattr(t, 'stats', None) is not None and t.stats[1] == 8
    ya = bn_a(t, act='elu').F
    t.stats = None
    yb = bn_b(t, act='elu').F
    _close(ya, yb, tol=2e-6, what='BatchNorm from the GEMM epilogue table vs from the matrix')
    _close(bn_a.bn.running_var, bn_b.bn.running_var, tol=2e-6, what='running_var')


@pytest.mark.parametrize('n,C,res', [(3000, 256, True), (60000, 64, True), (9000, 128, False)])
def test_batchnorm_backward_adds_a_second_gradient_on_the_fly(n, C, res):
    """fc_bn_train_bwd(gy, gy2) == fc_bn_train_bwd(gy + gy2): bit for bit (the executor's OP_ADD folded into the kernels)"""
    from fcaf3d_amd import _lib as L
    import fcaf3d_amd.functional as Fn
    dev = _dev()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, C, generator=g).to(dev)
    r = torch.randn(n, C, generator=g).to(dev) if res else None
    gam, bet = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
    g1, g2 = torch.randn(n, C, generator=g).to(dev), torch.randn(n, C, generator=g).to(dev)
    y = torch.empty_like(x)
    st = torch.empty((2, C), device=dev); cnt = torch.empty(1, device=dev)
    ws = L.workspace(L.query('fc_bn_train_ws_bytes', n, C), dev)
    L.call('fc_bn_train_fwd', L.ptr(x), n, C, 1e-5, L.ptr(gam), L.ptr(bet), L.ptr(r), 1, 0.1, L.ptr(y), L.ptr(st[0]), L.ptr(st[1]),
           L.ptr(cnt), None, None, None, None, 0, 1, Fn.BN_SMALL_ELEMS, L.ptr(ws), ws.numel(), L.stream())
    outs = []
    for a, b in ((g1 + g2, None), (g1, g2)):
        gx, gr, sums = torch.empty_like(x), torch.empty_like(x), torch.empty((2, C), device=dev)
        L.call('fc_bn_train_bwd', L.ptr(x), L.ptr(y) if res else None, L.ptr(a), L.ptr(b), n, C, L.ptr(st[0]), L.ptr(st[1]), L.ptr(cnt),
               1e-5, L.ptr(gam), L.ptr(bet), 1, L.ptr(gx), L.ptr(gr) if res else None, L.ptr(sums), None, 0, Fn.BN_SMALL_ELEMS,
               L.ptr(ws), ws.numel(), L.stream())
        outs.append((gx, gr if res else gx, sums))
    for u, v in zip(*outs):
        assert torch.equal(u, v)


def test_head_backward_with_bias_and_scale_sums():
    """fc_head_split_bwd_sums == fc_head_split_bwd + the two reductions autograd runs over its outputs"""
    from fcaf3d_amd import _lib as L
    dev = _dev()
    n, n_reg, n_cls, ld = 70001, 6, 18, 64
    g = torch.Generator().manual_seed(1)
    y = torch.randn(n, ld, generator=g).to(dev)
    bbox = torch.rand(n, n_reg, generator=g).to(dev) + 0.1
    gc, gb, gk = (torch.randn(n, c, generator=g).to(dev) for c in (1, n_reg, n_cls))
    sc = torch.tensor([1.3], device=dev)
    gy0, gs_row = torch.empty_like(y), torch.empty(n, device=dev)
    L.call('fc_head_split_bwd', L.ptr(y), ld, L.ptr(sc), L.ptr(bbox), L.ptr(gc), L.ptr(gb), L.ptr(gk), n, n_reg, n_cls, L.ptr(gy0),
           L.ptr(gs_row), L.stream())
    gy1, gbias, gscale = torch.empty_like(y), torch.empty(n_cls, device=dev), torch.empty(1, device=dev)
    ws = L.workspace(L.query('fc_head_split_bwd_sums_ws_bytes', n), dev)
    L.call('fc_head_split_bwd_sums', L.ptr(y), ld, L.ptr(sc), L.ptr(bbox), L.ptr(gc), L.ptr(gb), L.ptr(gk), n, n_reg, n_cls,
           L.ptr(gy1), L.ptr(gbias), L.ptr(gscale), L.ptr(ws), ws.numel(), L.stream())
    assert torch.equal(gy0, gy1)
    _close(gbias, gk.double().sum(0).float(), tol=2e-6, what='class-bias gradient')
    ref = float(gs_row.double().sum())
    assert abs(float(gscale) - ref) <= 2e-6 * float(gs_row.double().abs().sum()), (float(gscale), ref)


def test_bf16_fast_mode_is_a_flagged_non_parity_route():
    """with fc_set_bf16_fast(1) the split-bf16 launches multiply bf16-rounded operands only (one MFMA
    product instead of six).  NOT a parity route: bounded here at 2e-2 of the output scale (bf16 has 8 significand bits; a 27 x
    64...256-term sum of products of rounded operands sits at ~3e-3), and clearly different from the exact route."""
    from fcaf3d_amd import _lib as L
    import fcaf3d_amd.functional as Fn
    dev = _dev()
    x, w, km, cm = _stats_case(dev, 100000, 128, 128, 8, seed=23)
    go = torch.randn(cm.n, 128, device=dev)
    res = {}
    for mode in (0, 1):
        L.lib().fc_set_bf16_fast(mode)
        try:
            xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
            out = Fn.sparse_conv(xr, wr, km, cm.n)
            gx, gw = torch.autograd.grad(out, [xr, wr], go)
            torch.cuda.synchronize()
            res[mode] = (out.detach(), gx, gw)
        finally:
            L.lib().fc_set_bf16_fast(0)
    for a, b, what in zip(res[1], res[0], ('forward', 'backward data', 'backward weights')):
        err = float((a - b).abs().max()) / float(b.abs().max())
        print(f'bf16 fast mode, {what}: max difference to the exact route {err:.2e} of the tensor scale')
        assert 1e-5 < err < 2e-2, (what, err)


def test_non_finite_activations_on_the_split_route():
    """csrc/conv_x6.h:14-15, documented behaviour: an overflowed activation (+-inf) splits into (inf, nan, nan), so the split-bf16
    route yields NaN in every output row that gathers it where the fp32 MFMA route yields +-inf (or NaN where inf meets -inf / 0);
    a NaN activation yields NaN on both.  Rows that gather no non-finite input are untouched on both routes."""
    import fcaf3d_amd.functional as Fn
    dev = _dev()
    x, w, km, cm = _stats_case(dev, 100000, 64, 64, 8, seed=29)
    w = w.abs()                                        # no inf - inf on the fp32 route: it must produce +inf exactly
    x = x.clone()
    x[5, 3] = float('inf')
    x[9, 7] = float('nan')
    nbr = km.nbr.cpu().numpy()
    hit_inf, hit_nan = np.unique(np.nonzero(nbr == 5)[1]), np.unique(np.nonzero(nbr == 9)[1])
    clean = np.setdiff1d(np.arange(cm.n), np.union1d(hit_inf, hit_nan))
    only_inf = np.setdiff1d(hit_inf, hit_nan)
    outs = {}
    for x6 in (True, False):
        x6_0, Fn.X6 = Fn.X6, x6
        try:
            with torch.no_grad():
                outs[x6] = Fn.sparse_conv(x, w, km, cm.n).cpu().numpy()
        finally:
            Fn.X6 = x6_0
    assert len(only_inf) > 0 and len(clean) > 0
    for x6 in (True, False):
        assert np.isfinite(outs[x6][clean]).all(), 'rows without a non-finite neighbour must be finite'
        assert np.isnan(outs[x6][hit_nan]).any(axis=1).all(), 'a NaN input reaches every row that gathers it'
    assert np.isposinf(outs[False][only_inf]).any(axis=1).all(), 'fp32 MFMA route: +inf'
    assert np.isnan(outs[True][only_inf]).any(axis=1).all(), 'split-bf16 route: NaN (documented difference)'
    np.testing.assert_allclose(outs[True][clean], outs[False][clean], rtol=0, atol=1e-4 * np.abs(outs[False][clean]).max())


@pytest.mark.parametrize('n_points,Cin,Cout,q', [(100000, 64, 64, 4), (100000, 64, 128, 4), (100000, 128, 128, 8), (100000, 256, 256, 32),
                                                  (3000, 64, 64, 8), (777, 128, 64, 2)])
def test_buffer_and_flat_addressing_are_bit_identical(n_points, Cin, Cout, q):
    """csrc/conv_x6.h BUF (r5): gathering launches on a weight image read the rows and the image through buffer descriptors (32-bit
    row offsets, absent neighbours = an offset past the descriptor: zeros); CONV_FLAT = the flat 64-bit addresses operands of
    2 GB and more take.  Forward and backward-data, dense tables and pair lists, full and ragged tiles: the same bits."""
    import fcaf3d_amd.functional as Fn
    dev = _dev()
    x, w, km, cm = _stats_case(dev, n_points, Cin, Cout, q, seed=31)
    g = torch.randn(cm.n, Cout, generator=torch.Generator().manual_seed(5)).to(dev)
    res = {}
    f0 = Fn.FLAGS
    try:
        for flat in (False, True):
            Fn.FLAGS = f0 | (Fn.CONV_FLAT if flat else 0)
            xx = x.clone().requires_grad_(True)
            y = Fn.sparse_conv(xx, w, km, cm.n)
            y.backward(g)
            res[flat] = (y.detach().clone(), xx.grad.clone())
    finally:
        Fn.FLAGS = f0
    assert torch.isfinite(res[False][0]).all() and float(res[False][0].abs().max()) > 0
    assert torch.equal(res[False][0], res[True][0]), 'forward'
    assert torch.equal(res[False][1], res[True][1]), 'backward data'


@pytest.mark.parametrize('q,C,route', [(4, 64, 'tile epilogue'), (8, 128, 'pair lists'), (32, 256, 'pair lists, few rows')])
@pytest.mark.parametrize('act,with_add,from_y', [(1, False, False), (2, False, False), (1, True, True)])
def test_batchnorm_backward_sums_out_of_the_convolution_epilogue(q, C, route, act, with_add, from_y):
    """fc_conv_fwd_bn_bwd_stats / fc_conv_fwd_pairs_tiles_bn_bwd_stats: a launch whose result g is the gradient arriving at a
    BatchNorm (+ ReLU / ELU) layer also leaves, per row block, the column sums of g' = (g + add) act'(.) and of g' xhat — that
    layer's two backward reductions.  Checked against the same sums in float64 (2e-5 of the column scale), the result itself bit
    for bit against the plain launch, and fc_bn_train_bwd fed with the table against fc_bn_train_bwd reducing on its own."""
    from fcaf3d_amd import _lib as L
    import fcaf3d_amd.functional as Fn
    dev = _dev()
    x, w, km, cm = _stats_case(dev, 100000, C, C, q, seed=31)
    n = cm.n
    g = torch.Generator().manual_seed(q)
    bn_x = torch.randn(n, C, generator=g).to(dev)
    mean, var = bn_x.mean(0).contiguous(), bn_x.var(0, unbiased=False).contiguous()
    gam, bet = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.3).to(dev)
    add = torch.randn(n, C, generator=g).to(dev) if with_add else None
    res = torch.randn(n, C, generator=g).to(dev) if from_y else None
    eps = 1e-5
    pre = (bn_x - mean) / torch.sqrt(var + eps) * gam + bet + (res if res is not None else 0)
    bn_y = (torch.relu(pre) if act == 1 else torch.nn.functional.elu(pre)).contiguous()
    fl = Fn.FLAGS | Fn.CONV_X6
    img = Fn._x6_image(w, False)
    pairs = Fn._pair_conv(km, n, C, C)
    nb = L.query('fc_conv_stats_blocks', n, 27, C, C, fl, 1 if pairs else 0)
    assert nb > 0
    stats = torch.full((nb, 2, C), float('nan'), device=dev)
    out = torch.full((n, C), float('nan'), device=dev)
    with torch.no_grad():
        ref = Fn.sparse_conv(x, w, km, n)
    if pairs:
        pi, _, pos, cnt = km.pairs()
        ws = L.workspace(L.query('fc_conv_fwd_pairs_ws_bytes', n, 27, C), dev)
        L.call('fc_conv_fwd_pairs_tiles_bn_bwd_stats', L.ptr(x), L.ptr(img), L.ptr(pi), L.ptr(cnt), L.ptr(pos), L.ptr(out), n, n, 27, C, C,
               km.pair_tiles(), fl, L.ptr(ws), ws.numel(), L.ptr(stats), L.ptr(bn_x), L.ptr(mean), L.ptr(var), L.ptr(gam), L.ptr(bet), eps,
               act, L.ptr(add), L.ptr(bn_y) if from_y else None, L.stream())
    else:
        nbr, oidx = km.sorted_fwd()
        wsb = L.query('fc_conv_fwd_ws_bytes', n, 27, C, C, fl)
        ws = L.workspace(max(wsb, 1), dev)
        L.call('fc_conv_fwd_bn_bwd_stats', L.ptr(x), L.ptr(img), L.ptr(nbr), L.ptr(oidx), L.ptr(out), n, n, 27, C, C, fl, L.ptr(ws),
               ws.numel(), L.ptr(stats), L.ptr(bn_x), L.ptr(mean), L.ptr(var), L.ptr(gam), L.ptr(bet), eps, act, L.ptr(add),
               L.ptr(bn_y) if from_y else None, L.stream())
    assert torch.equal(out, ref), route
    gsum = out.double() + (add.double() if add is not None else 0)
    xh = ((bn_x - mean) / torch.sqrt(var + eps)).double()
    if from_y:
        d = (bn_y > 0).double() if act == 1 else torch.where(bn_y > 0, torch.ones_like(bn_y), bn_y + 1).double()
    else:
        p0 = ((bn_x - mean) / torch.sqrt(var + eps) * gam + bet)
        d = (p0 > 0).double() if act == 1 else torch.where(p0 > 0, torch.ones_like(p0), torch.exp(p0)).double()
    gp = gsum * d
    s1, s2 = stats[:, 0].double().sum(0), stats[:, 1].double().sum(0)
    sc1, sc2 = float(gp.abs().sum(0).max()), float((gp * xh).abs().sum(0).max())
    # (a ReLU decision on a pre-activation at rounding level may differ between torch's expression and the kernel's fused
    # multiply-add: a handful of elements of ~4e6, each worth one |g| — allowed for on top of the 2e-5)
    slack = 4.0 * float(gsum.abs().max()) if (act == 1 and not from_y) else 0.0
    assert float((s1 - gp.sum(0)).abs().max()) <= 2e-5 * sc1 + slack, (route, float((s1 - gp.sum(0)).abs().max()), sc1)
    assert float((s2 - (gp * xh).sum(0)).abs().max()) <= 2e-5 * sc2 + slack * float(xh.abs().max()), route
    # the BatchNorm backward fed with the table == the one that reduces on its own (to summation order)
    cntt = torch.full((1,), float(n), device=dev)
    res_out = []
    for part in (None, stats):
        gx, gr, sums = torch.empty_like(bn_x), torch.empty_like(bn_x), torch.empty((2, C), device=dev)
        wsb = L.workspace(L.query('fc_bn_train_ws_bytes', n, C), dev)
        L.call('fc_bn_train_bwd', L.ptr(bn_x), L.ptr(bn_y) if from_y else None, L.ptr(out), L.ptr(add), n, C, L.ptr(mean), L.ptr(var),
               L.ptr(cntt), eps, L.ptr(gam), L.ptr(bet), act, L.ptr(gx), L.ptr(gr) if from_y else None, L.ptr(sums),
               L.ptr(part), nb if part is not None else 0, Fn.BN_SMALL_ELEMS, L.ptr(wsb), wsb.numel(), L.stream())
        res_out.append((gx, sums))
    _close(res_out[1][0], res_out[0][0], tol=2e-5, what='gx: table from the epilogue vs own reduction')
    _close(res_out[1][1], res_out[0][1], tol=2e-5, what='d beta / d gamma')
