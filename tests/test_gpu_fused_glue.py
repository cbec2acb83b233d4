"""-m gpu: the fused glue kernels of the two finest resolutions (csrc/norm.hip, r7) against the operator sequences they replace,
through the C ABI on identical inputs.

A. fc_norm_act_maxpool8_fwd  ==  fc_norm_act_fwd + fc_maxpool_fwd                      bit for bit (out, argrow, amax word, y)
B. fc_maxpool8_norm_act_bwd  ==  zero fill + fc_maxpool_bwd + fc_norm_act_bwd          bit for bit, and both against fp64 on the CPU
C. fc_inverse_rows + fc_bn_train_add_fwd / fc_norm_act_add_fwd  ==  normalisation + copy + fc_scatter_rows_add + fc_amax   bit for bit
"""
import pytest
import torch

import fcaf3d_amd.functional as Fn
from fcaf3d_amd import _lib as L

pytestmark = pytest.mark.gpu
C = 64
EPS = 1e-5
RELU, ELU = 1, 2


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _amax_word(slot):
    """the operand's amax as its consumers read it: the maximum of the slot's 32 sub-words (fc_common.h fc_amax_read)"""
    return int(slot.view(32, 16)[:, 0].max())


def _new_slot(dev):
    return torch.zeros(512, dtype=torch.int32, device=dev)


def _stem_tail_inputs(nseg, n_out, seed, dev):
    """a k2s2-like pooling table: every input row is the child of exactly one pooled row, 0..8 children per pooled row in random
    offset slots (absent children, a few pooled rows without any child), children of a pooled row in one scene; pooled rows nearly
    scene-contiguous; x with per-scene statistics, and a share of pooled rows whose children are all far below the mean (all
    negative before the ReLU: exact ties at 0)."""
    g = torch.Generator().manual_seed(seed)
    kcount = torch.randint(1, 9, (n_out,), generator=g)
    kcount[nseg + torch.randperm(n_out - nseg, generator=g)[:7]] = 0         # rows without children: 0 / -1
    seg_out = torch.sort(torch.randint(0, nseg, (n_out,), generator=g))[0]
    swap = torch.randperm(n_out, generator=g)[:64]                           # ... nearly: some rows out of place
    seg_out[swap] = seg_out[swap.flip(0)]
    seg_out[:nseg] = torch.arange(nseg)                                      # every scene is there
    kcount[:nseg] = torch.clamp(kcount[:nseg], min=2)
    n_in = int(kcount.sum())
    child_ids = torch.randperm(n_in, generator=g)
    nbr = torch.full((8, n_out), -1, dtype=torch.int32)
    parent = torch.empty(n_in, dtype=torch.long)
    pos = 0
    for o in range(n_out):
        k = int(kcount[o])
        if k == 0:
            continue
        slots = torch.randperm(8, generator=g)[:k]
        ids = child_ids[pos:pos + k]
        nbr[slots, o] = ids.int()
        parent[ids] = o
        pos += k
    seg_in = seg_out[parent]
    scale = 0.5 + torch.arange(nseg).float()
    shift = torch.linspace(-1.0, 2.0, nseg)
    x = torch.randn(n_in, C, generator=g) * scale[seg_in][:, None] + shift[seg_in][:, None]
    low = torch.randperm(n_out, generator=g)[:n_out // 10]                   # pooled rows that are all-negative before the ReLU
    is_low = torch.zeros(n_out, dtype=torch.bool)
    is_low[low] = True
    x[is_low[parent]] = -40.0 - torch.rand(int(is_low[parent].sum()), C, generator=g)
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    coords_in = torch.zeros((n_in, 4), dtype=torch.int32)
    coords_in[:, 0] = seg_in.int()
    coords_out = torch.zeros((n_out, 4), dtype=torch.int32)
    coords_out[:, 0] = seg_out.int()
    t = dict(x=x, nbr=nbr, seg_in=coords_in, seg_out=coords_out, gamma=gamma, beta=beta, g_pool=torch.randn(n_out, C, generator=g))
    t = {k: v.contiguous().to(dev) for k, v in t.items()}
    t.update(n_in=n_in, n_out=n_out, nseg=nseg, is_low=is_low)
    mean, var, cnt = Fn.col_stats(t['x'], t['seg_in'], nseg)
    t.update(mean=mean.contiguous(), var=var.contiguous(), cnt=cnt.contiguous())
    return t


def _two_step_forward(t, dev):
    n_in, n_out = t['n_in'], t['n_out']
    y = torch.empty((n_in, C), dtype=torch.float32, device=dev)
    L.call('fc_norm_act_fwd', L.ptr(t['x']), L.ptr(t['seg_in']), 4, n_in, C, L.ptr(t['mean']), L.ptr(t['var']), EPS, L.ptr(t['gamma']),
           L.ptr(t['beta']), None, RELU, L.ptr(y), L.stream())
    out = torch.empty((n_out, C), dtype=torch.float32, device=dev)
    arg = torch.empty((n_out, C), dtype=torch.int32, device=dev)
    slot = _new_slot(dev)
    L.call('fc_amax_out_hint', L.ptr(slot))
    L.call('fc_maxpool_fwd', L.ptr(y), L.ptr(t['nbr']), n_out, 8, C, L.ptr(out), L.ptr(arg), L.stream())
    return y, out, arg, slot


@pytest.mark.parametrize('nseg,n_out', [(2, 3001), (5, 20011), (8, 40013)])
def test_stem_tail_forward_is_bit_identical(nseg, n_out):
    dev = _dev()
    t = _stem_tail_inputs(nseg, n_out, 10 + nseg, dev)
    assert (n_out * (C // 4)) % 256 != 0, 'the last block must be partial'
    y0, out0, arg0, slot0 = _two_step_forward(t, dev)
    # the inputs are what they claim: ties at 0 on the all-negative rows, rows without children
    assert float(out0[t['is_low'].to(dev)].abs().max()) == 0.0 and int((arg0 < 0).all(1).sum()) == 7
    for want_y in (False, True):
        out = torch.full((n_out, C), float('nan'), dtype=torch.float32, device=dev)
        arg = torch.full((n_out, C), -7, dtype=torch.int32, device=dev)
        y = torch.full((t['n_in'], C), float('nan'), dtype=torch.float32, device=dev) if want_y else None
        parent = torch.full((t['n_in'],), -7, dtype=torch.int32, device=dev) if want_y else None
        slot = _new_slot(dev)
        L.call('fc_amax_out_hint', L.ptr(slot))
        L.call('fc_norm_act_maxpool8_fwd', L.ptr(t['x']), L.ptr(t['seg_in']), 4, C, L.ptr(t['mean']), L.ptr(t['var']), EPS,
               L.ptr(t['gamma']), L.ptr(t['beta']), RELU, L.ptr(t['nbr']), n_out, L.ptr(out), L.ptr(arg), L.ptr(y), L.ptr(parent),
               L.stream())
        assert torch.equal(out, out0)
        assert torch.equal(arg, arg0)
        assert _amax_word(slot) == _amax_word(slot0) != 0
        if want_y:
            assert torch.equal(y, y0)
            # the child -> parent map inverts the pool table
            nbr = t['nbr'].long()
            o = torch.arange(n_out, device=dev).expand(8, n_out)
            ref = torch.full((t['n_in'],), -1, dtype=torch.int32, device=dev)
            ref[nbr[nbr >= 0]] = o[nbr >= 0].int()
            assert torch.equal(parent, ref) and int((ref < 0).sum()) == 0


@pytest.mark.parametrize('nseg,n_out', [(2, 3001), (5, 20011), (8, 40013)])
def test_stem_tail_backward_is_as_accurate_as_the_three_operators(nseg, n_out):
    """The fused backward reads the pooled gradient through the child -> parent map and sums in the order of fc_norm_act_bwd: gx and
    sums are bit for bit the three operators' (a training run of many steps amplifies any reordered sum far beyond rounding).
    Both are also compared with an fp64 evaluation (same forward decisions: the ReLU mask and the arg-max rows of the device's
    forward pass); bound: the fused path's max-abs error relative to the tensor's maximum is at most twice the three-operator
    path's.  Measured on MI355X: profiles/r7_notes.md."""
    dev = _dev()
    t = _stem_tail_inputs(nseg, n_out, 20 + nseg, dev)
    n_in = t['n_in']
    y0, out0, arg0, _ = _two_step_forward(t, dev)
    parent = torch.empty((n_in,), dtype=torch.int32, device=dev)
    out1, arg1 = torch.empty_like(out0), torch.empty_like(arg0)
    L.call('fc_norm_act_maxpool8_fwd', L.ptr(t['x']), L.ptr(t['seg_in']), 4, C, L.ptr(t['mean']), L.ptr(t['var']), EPS, L.ptr(t['gamma']),
           L.ptr(t['beta']), RELU, L.ptr(t['nbr']), n_out, L.ptr(out1), L.ptr(arg1), None, L.ptr(parent), L.stream())
    # three operators: zero fill, scatter, normalisation backward
    g_in = torch.zeros((n_in, C), dtype=torch.float32, device=dev)
    L.call('fc_maxpool_bwd', L.ptr(t['g_pool']), L.ptr(arg0), n_out, C, L.ptr(g_in), L.stream())
    gx0 = torch.empty((n_in, C), dtype=torch.float32, device=dev)
    sums0 = torch.empty((nseg, 2, C), dtype=torch.float32, device=dev)
    nb = L.query('fc_norm_act_bwd_ws_bytes', n_in, C, nseg)
    ws = L.workspace(nb, dev)
    L.call('fc_norm_act_bwd', L.ptr(t['x']), None, L.ptr(g_in), L.ptr(t['seg_in']), 4, n_in, C, nseg, L.ptr(t['mean']), L.ptr(t['var']),
           L.ptr(t['cnt']), EPS, L.ptr(t['gamma']), L.ptr(t['beta']), RELU, L.ptr(gx0), None, L.ptr(sums0), L.ptr(ws), ws.numel(), L.stream())
    # fused
    gx1 = torch.full((n_in, C), float('nan'), dtype=torch.float32, device=dev)
    sums1 = torch.full((nseg, 2, C), float('nan'), dtype=torch.float32, device=dev)
    nb = L.query('fc_maxpool8_norm_act_bwd_ws_bytes', n_in, C, nseg)
    ws = L.workspace(nb, dev)
    L.call('fc_maxpool8_norm_act_bwd', L.ptr(t['x']), L.ptr(t['g_pool']), L.ptr(arg1), L.ptr(parent), L.ptr(t['seg_in']), 4, n_in, C,
           nseg, L.ptr(t['mean']), L.ptr(t['var']), L.ptr(t['cnt']), EPS, L.ptr(t['gamma']), L.ptr(t['beta']), RELU, L.ptr(gx1),
           L.ptr(sums1), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    # fp64 on the CPU
    x = t['x'].cpu().double()
    seg = t['seg_in'][:, 0].cpu().long()
    mu, va, cnt = t['mean'].cpu().double()[seg], t['var'].cpu().double()[seg], t['cnt'].cpu().double().reshape(-1)
    inv_std = 1.0 / torch.sqrt(va + EPS)
    xh = (x - mu) * inv_std
    arg = arg0.cpu().long()
    g = torch.zeros((n_in, C), dtype=torch.float64)
    cols = torch.arange(C).expand(n_out, C)
    ok = arg >= 0
    g[arg[ok], cols[ok]] = t['g_pool'].cpu().double()[ok]
    g = g * (y0.cpu() > 0)
    sums = torch.zeros((nseg, 2, C), dtype=torch.float64)
    sums[:, 0].index_add_(0, seg, g)
    sums[:, 1].index_add_(0, seg, g * xh)
    gamma = t['gamma'].cpu().double()
    gx = gamma * inv_std * (g - sums[seg, 0] / cnt[seg][:, None] - xh * sums[seg, 1] / cnt[seg][:, None])

    def err(a, ref):
        return float((a.cpu().double() - ref).abs().max()) / float(ref.abs().max())
    e_gx0, e_gx1, e_s0, e_s1 = err(gx0, gx), err(gx1, gx), err(sums0, sums), err(sums1, sums)
    print(f'stem tail backward nseg={nseg} n_out={n_out} n_in={n_in}: gx fused {e_gx1:.3e} three-operator {e_gx0:.3e}; '
          f'sums fused {e_s1:.3e} three-operator {e_s0:.3e}')
    assert torch.isfinite(gx1).all() and torch.isfinite(sums1).all()
    assert e_gx1 <= 2.0 * e_gx0, (e_gx1, e_gx0)
    assert e_s1 <= 2.0 * e_s0, (e_s1, e_s0)
    assert torch.equal(sums1, sums0)
    assert torch.equal(gx1, gx0)


def _union_inputs(n_g, n_b, Cc, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n_g, Cc, generator=g) * 1.5 + 0.3).to(dev)
    fb = (torch.randn(n_b, Cc, generator=g) * 3.0).to(dev)
    rows = torch.randperm(n_g, generator=g)[:n_b].int().to(dev)
    gamma = (0.5 + torch.rand(Cc, generator=g)).to(dev)
    beta = (0.2 * torch.randn(Cc, generator=g)).to(dev)
    return x, fb, rows, gamma, beta


def _part_table(x, nb):
    """column sums of x and x^2 per row block, [nb][2][C]: what a convolution's statistics epilogue leaves"""
    n, Cc = x.shape
    part = torch.zeros((nb, 2, Cc), dtype=torch.float32, device=x.device)
    edges = torch.linspace(0, n, nb + 1).long().tolist()
    for b in range(nb):
        blk = x[edges[b]:edges[b + 1]]
        part[b, 0], part[b, 1] = blk.sum(0), (blk * blk).sum(0)
    return part.contiguous()


def _inverse(rows, n_g, dev):
    inv = torch.full((n_g,), 12345, dtype=torch.int32, device=dev)
    L.call('fc_inverse_rows', L.ptr(rows), rows.numel(), n_g, L.ptr(inv), L.stream())
    return inv


# the three union levels' shapes (rows of the generated set, rows of the backbone level, channels), scaled down, times the routes
# of fc_bn_train_fwd: statistics table of <= 64 blocks (one launch, with and without channel windows), of more (two launches),
# no table (small: two launches + amax pass; large: three)
@pytest.mark.parametrize('n_g,n_b,Cc,nb_part', [(50003, 17001, 64, 200), (50003, 17001, 64, 0), (9001, 3100, 128, 40), (9001, 3100, 128, 0),
                                                (1501, 500, 256, 12), (1501, 500, 256, 0), (3001, 1000, 64, 30)])
def test_union_written_by_the_normalisation_is_bit_identical_training(n_g, n_b, Cc, nb_part):
    dev = _dev()
    x, fb, rows, gamma, beta = _union_inputs(n_g, n_b, Cc, n_g + nb_part, dev)
    inv = _inverse(rows, n_g, dev)
    ref_inv = torch.full((n_g,), -1, dtype=torch.int32, device=dev)
    ref_inv[rows.long()] = torch.arange(n_b, dtype=torch.int32, device=dev)
    assert torch.equal(inv, ref_inv) and int((inv >= 0).sum()) == n_b
    part = _part_table(x, nb_part) if nb_part else None
    ws = L.workspace(L.query('fc_bn_train_ws_bytes', n_g, Cc), dev)
    res = []
    for fused in (False, True):
        y = torch.full((n_g, Cc), float('nan'), dtype=torch.float32, device=dev)
        mean, var = torch.empty(Cc, device=dev), torch.empty(Cc, device=dev)
        cnt = torch.empty(1, device=dev)
        rmean, rvar = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)
        nbt = torch.zeros(1, dtype=torch.int64, device=dev)
        slot = _new_slot(dev)
        head = (L.ptr(x), n_g, Cc, EPS, L.ptr(gamma), L.ptr(beta), None, ELU, 0.1, L.ptr(y), L.ptr(mean), L.ptr(var), L.ptr(cnt), L.ptr(rmean),
                L.ptr(rvar), L.ptr(nbt), L.ptr(part), nb_part, 1, Fn.BN_SMALL_ELEMS)
        if fused:
            L.call('fc_amax_out_hint', L.ptr(slot))
            L.call('fc_bn_train_add_fwd', *head, L.ptr(inv), L.ptr(fb), L.ptr(ws), ws.numel(), L.stream())
            u = y
        else:
            L.call('fc_bn_train_fwd', *head, L.ptr(ws), ws.numel(), L.stream())
            u = torch.empty_like(y)
            u.copy_(y)                                                  # OP_UNION_FWD: copy, scatter-add, then a stand-alone amax pass
            L.call('fc_scatter_rows_add', L.ptr(fb), L.ptr(rows), n_b, Cc, L.ptr(u), L.stream())
            L.call('fc_amax', L.ptr(u), n_g * Cc, L.ptr(slot), L.stream())
        res.append((u, _amax_word(slot), mean, var, rmean, rvar, nbt))
    (u0, a0, *s0), (u1, a1, *s1) = res
    assert torch.isfinite(u0).all() and not torch.equal(u0[rows.long()], u0[rows.long()] - fb)
    assert torch.equal(u1, u0)
    assert a1 == a0 != 0
    for p, q in zip(s0, s1):
        assert torch.equal(p, q)


@pytest.mark.parametrize('n_g,n_b,Cc', [(50003, 17001, 64), (9001, 3100, 128), (1501, 500, 256)])
def test_union_written_by_the_normalisation_is_bit_identical_eval(n_g, n_b, Cc):
    dev = _dev()
    x, fb, rows, gamma, beta = _union_inputs(n_g, n_b, Cc, 7 + n_g, dev)
    inv = _inverse(rows, n_g, dev)
    rmean, rvar = x.mean(0).contiguous(), x.var(0).contiguous()
    u0 = torch.empty((n_g, Cc), dtype=torch.float32, device=dev)
    y = torch.empty_like(u0)
    L.call('fc_norm_act_fwd', L.ptr(x), None, 0, n_g, Cc, L.ptr(rmean), L.ptr(rvar), EPS, L.ptr(gamma), L.ptr(beta), None, ELU, L.ptr(y), L.stream())
    u0.copy_(y)
    L.call('fc_scatter_rows_add', L.ptr(fb), L.ptr(rows), n_b, Cc, L.ptr(u0), L.stream())
    slot0, slot1 = _new_slot(dev), _new_slot(dev)
    L.call('fc_amax', L.ptr(u0), n_g * Cc, L.ptr(slot0), L.stream())
    u1 = torch.full((n_g, Cc), float('nan'), dtype=torch.float32, device=dev)
    L.call('fc_amax_out_hint', L.ptr(slot1))
    L.call('fc_norm_act_add_fwd', L.ptr(x), None, 0, n_g, Cc, L.ptr(rmean), L.ptr(rvar), EPS, L.ptr(gamma), L.ptr(beta), None, ELU, L.ptr(inv),
           L.ptr(fb), L.ptr(u1), L.stream())
    assert torch.equal(u1, u0)
    assert _amax_word(slot1) == _amax_word(slot0) != 0


# ---- every route of csrc/norm_route.h once, at the smallest shape that reaches it ------------------------------------------------------

def _route_case_inputs(n, Cc, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, Cc, generator=g) * 1.5 + 0.3).to(dev)
    gy = torch.randn(n, Cc, generator=g).to(dev)
    gamma = (0.5 + torch.rand(Cc, generator=g)).to(dev)
    beta = (0.2 * torch.randn(Cc, generator=g)).to(dev)
    return x, gy, gamma, beta


def _close(a, ref, what):
    """the project's bound: max-abs error within 1e-4 of the tensor's scale, against float64 numpy"""
    import numpy as np
    a = a.detach().cpu().double().numpy().reshape(ref.shape)
    err, scale = float(np.abs(a - ref).max()), float(np.abs(ref).max())
    print(f'{what}: max-abs error {err:.3e}, scale {scale:.3e}')
    assert np.isfinite(a).all() and err <= 1e-4 * scale, (what, err, scale)


def _amax_bits(t):
    t = t[torch.isfinite(t)].abs().max().reshape(1)
    return int(t.view(torch.int32))


def _elu_grad(pre):
    import numpy as np
    return np.where(pre > 0, 1.0, np.exp(np.minimum(pre, 0.0)))


def test_every_batchnorm_route_against_fp64():
    """Each family of norm_fwd_route / norm_bwd_route once (selected through small_elems and a torch-built table, so no shape is large):
    y / gx, mean, var and sums against float64 numpy; the amax word (folded by the apply kernel, or the small route's pass of its own) bit-equal to max |.| of the tensor the
    kernel wrote; the route query's workspace bytes are what the launch needs — it runs on exactly that many and answers one byte
    less with FC_EWS, writing nothing."""
    import numpy as np
    dev = _dev()
    E = L.header_enums()
    l = L.lib()
    TRAIN, SEG = E['FC_NFORM_TRAIN'], E['FC_NFORM_SEG']
    nan = float('nan')

    # ---- forward: (n, C, blocks of the table or 0, small_elems) -> the family it must reach
    fwd_cases = [(100, 8, 0, 1 << 20, 'FC_NSTATS_PARTIAL_SMALL', 'FC_NAPPLY_BN1', 'FC_NAMAX_PASS', 8),
                 (100, 8, 0, 0, 'FC_NSTATS_PARTIAL', 'FC_NAPPLY_ROWS', 'FC_NAMAX_FOLDED', 8),
                 (130, 8, 65, 1 << 20, 'FC_NSTATS_TABLE', 'FC_NAPPLY_ROWS', 'FC_NAMAX_FOLDED', 8),
                 (128, 64, 4, 1 << 20, 'FC_NSTATS_PROLOGUE', 'FC_NAPPLY_BN2', 'FC_NAMAX_FOLDED', 64),
                 (70, 128, 2, 1 << 20, 'FC_NSTATS_PROLOGUE', 'FC_NAPPLY_BN2', 'FC_NAMAX_FOLDED', 64)]
    for n, Cc, nbp, small, stats, apply, amax, cg in fwd_cases:
        x, _, gamma, beta = _route_case_inputs(n, Cc, 100 + n + Cc + nbp, dev)
        part = _part_table(x, nbp) if nbp else None
        rc, r = L.route('fc_bn_train_fwd_route', n, Cc, 1 if nbp else 0, nbp, 1, small)
        assert rc == 0 and (r['sums'], r['apply'], r['amax'], r['cg']) == (E[stats], E[apply], E[amax], cg), (n, Cc, nbp, small, r)
        need = r['ws_bytes']
        assert (need > 0) == (nbp == 0)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        y = torch.full((n, Cc), nan, device=dev)
        mean, var, cnt = torch.full((Cc,), nan, device=dev), torch.full((Cc,), nan, device=dev), torch.full((1,), nan, device=dev)
        slot = _new_slot(dev)
        args = (L.ptr(x), n, Cc, EPS, L.ptr(gamma), L.ptr(beta), None, ELU, 0.1, L.ptr(y), L.ptr(mean), L.ptr(var), L.ptr(cnt), None, None, None,
                L.ptr(part), nbp, 1, small, L.ptr(ws))
        if need:
            L.call('fc_amax_out_hint', L.ptr(slot))
            assert l.fc_bn_train_fwd(*args, need - 1, L.stream()) == -2
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(t).all()) for t in (y, mean, var, cnt)) and _amax_word(slot) == 0
        L.call('fc_amax_out_hint', L.ptr(slot))
        L.call('fc_bn_train_fwd', *args, need, L.stream())
        torch.cuda.synchronize()
        xd = x.cpu().double().numpy()
        mu, va = xd.mean(0), xd.var(0)
        pre = (xd - mu) / np.sqrt(va + EPS) * gamma.cpu().double().numpy() + beta.cpu().double().numpy()
        tag = f'forward {n} x {Cc}, table {nbp}, small_elems {small}'
        _close(y, np.where(pre > 0, pre, np.expm1(np.minimum(pre, 0.0))), tag + ' y')
        _close(mean, mu, tag + ' mean')
        _close(var, va, tag + ' var')
        assert float(cnt) == n
        assert _amax_word(slot) == _amax_bits(y) != 0, tag          # folded by the apply kernel, or the small route's pass of its own

    # ---- backward: (n, C, blocks of the producer's table or 0, small_elems)
    bwd_cases = [(100, 8, 0, 1 << 20, 'FC_NRED_PARTIAL', 'FC_NBAPPLY_PROLOGUE', 2, 8),
                 (4097, 4, 0, 0, 'FC_NRED_PARTIAL', 'FC_NBAPPLY_FINAL', 65, 4),
                 (70, 128, 2, 1 << 20, 'FC_NRED_TABLE', 'FC_NBAPPLY_PROLOGUE', 2, 64)]
    for n, Cc, nbp, small, reduce, apply, np_blocks, cg in bwd_cases:
        x, gy, gamma, beta = _route_case_inputs(n, Cc, 200 + n + Cc + nbp, dev)
        xd, gd = x.cpu().double().numpy(), gy.cpu().double().numpy()
        mean, var = torch.from_numpy(xd.mean(0)).float().to(dev), torch.from_numpy(xd.var(0)).float().to(dev)
        cnt = torch.full((1,), float(n), device=dev)
        mu, va = mean.cpu().double().numpy(), var.cpu().double().numpy()          # (the fp32 statistics the kernels are given)
        inv_std = 1.0 / np.sqrt(va + EPS)
        xh = (xd - mu) * inv_std
        gp = gd * _elu_grad(xh * gamma.cpu().double().numpy() + beta.cpu().double().numpy())
        s0, s1 = gp.sum(0), (gp * xh).sum(0)
        gx_ref = gamma.cpu().double().numpy() * inv_std * (gp - s0 / n - xh * s1 / n)
        part = None
        if nbp:                                                                    # [nb][2][C]: column sums of g' and g' xhat per row block
            gp_t = torch.from_numpy(gp).float().to(dev)
            xh_t = torch.from_numpy(xh).float().to(dev)
            edges = torch.linspace(0, n, nbp + 1).long().tolist()
            part = torch.stack([torch.stack([gp_t[a:b].sum(0), (gp_t[a:b] * xh_t[a:b]).sum(0)]) for a, b in zip(edges[:-1], edges[1:])]).contiguous()
        rc, r = L.route('fc_bn_train_bwd_route', n, Cc, 1, 1 if nbp else 0, nbp, small, TRAIN)
        assert rc == 0 and (r['sums'], r['apply'], r['np'], r['cg']) == (E[reduce], E[apply], np_blocks, cg), (n, Cc, nbp, small, r)
        need = r['ws_bytes']
        assert (need > 0) == (nbp == 0)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        gx, sums = torch.full((n, Cc), nan, device=dev), torch.full((2, Cc), nan, device=dev)
        slot = _new_slot(dev)
        args = (L.ptr(x), None, L.ptr(gy), None, n, Cc, L.ptr(mean), L.ptr(var), L.ptr(cnt), EPS, L.ptr(gamma), L.ptr(beta), ELU, L.ptr(gx), None,
                L.ptr(sums), L.ptr(part), nbp, small, L.ptr(ws))
        if need:
            L.call('fc_amax_out_hint', L.ptr(slot))
            assert l.fc_bn_train_bwd(*args, need - 1, L.stream()) == -2
            torch.cuda.synchronize()
            assert bool(torch.isnan(gx).all()) and bool(torch.isnan(sums).all()) and _amax_word(slot) == 0
        L.call('fc_amax_out_hint', L.ptr(slot))
        L.call('fc_bn_train_bwd', *args, need, L.stream())
        torch.cuda.synchronize()
        tag = f'backward {n} x {Cc}, table {nbp}, small_elems {small}'
        _close(gx, gx_ref, tag + ' gx')
        _close(sums, np.stack([s0, s1]), tag + ' sums')
        assert _amax_word(slot) == _amax_bits(gx) != 0, tag                          # (both apply kernels fold)

    # ---- the pooled stem form: 8 parents x 8 children, 2 scenes
    n_out, n_in, Cc, nseg = 8, 64, 8, 2
    g = torch.Generator().manual_seed(77)
    x, _, gamma, beta = _route_case_inputs(n_in, Cc, 300, dev)
    child = torch.randperm(n_in, generator=g).reshape(n_out, 8)                     # child[o][k]: the input row at offset k of pooled row o
    parent = torch.empty(n_in, dtype=torch.long)
    parent[child.reshape(-1)] = torch.arange(n_out).repeat_interleave(8)
    arg = child.gather(1, torch.randint(0, 8, (n_out, Cc), generator=g))            # the winning child per pooled row and channel
    g_pool = torch.randn(n_out, Cc, generator=g)
    seg_in = torch.zeros((n_in, 4), dtype=torch.int32)
    seg_in[:, 0] = (parent >= n_out // 2).int()
    scene = seg_in[:, 0].long().numpy()
    xd = x.cpu().double().numpy()
    mean = torch.from_numpy(np.stack([xd[scene == s].mean(0) for s in range(nseg)])).float().to(dev)
    var = torch.from_numpy(np.stack([xd[scene == s].var(0) for s in range(nseg)])).float().to(dev)
    cnt = torch.tensor([float((scene == s).sum()) for s in range(nseg)], device=dev)
    mu, va, cn = mean.cpu().double().numpy()[scene], var.cpu().double().numpy()[scene], cnt.cpu().double().numpy()[scene][:, None]
    inv_std = 1.0 / np.sqrt(va + EPS)
    xh = (xd - mu) * inv_std
    gin = np.where(arg.numpy()[parent.numpy()] == np.arange(n_in)[:, None], g_pool.double().numpy()[parent.numpy()], 0.0)
    gp = gin * _elu_grad(xh * gamma.cpu().double().numpy() + beta.cpu().double().numpy())
    sums_ref = np.stack([np.stack([gp[scene == s].sum(0), (gp * xh)[scene == s].sum(0)]) for s in range(nseg)])
    gx_ref = gamma.cpu().double().numpy() * inv_std * (gp - sums_ref[scene, 0] / cn - xh * sums_ref[scene, 1] / cn)
    rc, r = L.route('fc_bn_train_bwd_route', n_in, Cc, nseg, 0, 0, 0, SEG)
    assert rc == 0 and (r['sums'], r['apply'], r['launches']) == (E['FC_NRED_PARTIAL'], E['FC_NBAPPLY_FINAL'], 3)
    need = r['ws_bytes']
    assert need == L.query('fc_maxpool8_norm_act_bwd_ws_bytes', n_in, Cc, nseg) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    gx, sums = torch.full((n_in, Cc), nan, device=dev), torch.full((nseg, 2, Cc), nan, device=dev)
    t = [v.contiguous().to(dev) for v in (g_pool, arg.int(), parent.int(), seg_in)]
    args = (L.ptr(x), L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), 4, n_in, Cc, nseg, L.ptr(mean), L.ptr(var), L.ptr(cnt), EPS, L.ptr(gamma),
            L.ptr(beta), ELU, L.ptr(gx), L.ptr(sums), L.ptr(ws))
    assert l.fc_maxpool8_norm_act_bwd(*args, need - 1, L.stream()) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(gx).all()) and bool(torch.isnan(sums).all())
    L.call('fc_maxpool8_norm_act_bwd', *args, need, L.stream())
    torch.cuda.synchronize()
    _close(gx, gx_ref, 'pooled backward gx')
    _close(sums, sums_ref, 'pooled backward sums')
