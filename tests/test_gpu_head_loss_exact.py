"""-m gpu: the loss kernels of the head (csrc/loss.hip: k_fcaf3d_loss_fwd / _final / _bwd, k_focal_fwd / _bwd, k_aiou3d, k_riou3d) through
the C ABI against the float64 references of tests/head_cases.py.  N in {1, 255, 256, 257, 513} (one block, its edge, three blocks);
C in {1, 18, 32, 33}: 32 is the last width staged through LDS, 33 the first that is not, and at C = 1 the backward's grid of N C elements
is exactly the row grid.  Three scenes mixed row by row, scene 1 without a positive, positives of weight 0, labels from {-1, 0, C - 1}.
Every (N, C) item holds general rows, IoU edge rows on dyadic coordinates (identical boxes, one / two / three shared faces, touching,
disjoint, contained both ways, boxes of size 2^-7 whose union is below eps) and saturated rows (logits +-30, +-80, +-100, +-200 under
positive and negative labels); a single row cannot hold them all, so N = 1 is one launch per row class.  Outputs start as NaN with 64
guard rows, the workspace as 0xFF bytes.

The bound of every gradient element.  The reference is evaluated in float64 IN THE KERNEL'S OPERATION ORDER, and every intermediate
carries a bound on what fp32 may make of it (head_cases.E, running error analysis): an operation hands on its operands' bounds —
a product |a| eb + |b| ea + ea eb, a quotient (ea + |a / b| eb) / (|b| - eb), exp e^v (e^ea - 1), log -log(1 - ea / |a|) — and adds
its own rounding: u = 2^-24 of the magnitude for + - * / (round to nearest), 2 u for expf, logf, log1pf (one ulp, the accuracy HIP
documents for them).  No constant is fitted; the three terms the bound consists of come out of that as follows.
  * A few ulps of |ref|: a class gradient passes about ten roundings (exp, 1 + e, 1 / ., 1 - p, the square, two products and the
    difference inside the parenthesis, two products for lw g0 inv_pos, the last product), 10 .. 12 u where nothing cancels.
  * The cancellation of 1 - p: p = 1 / (1 + e^-x) carries up to 4 u p, which 1 - p keeps as an ABSOLUTE error: relative
    4 u p / (1 - p).  (1 - p)^2 doubles it, log(1 - p) turns it into an absolute 4 u p / (1 - p) of the log, which is multiplied by
    the factor in front of the log — (1 - alpha) p^2 gamma (1 - p) in the negative branch.  At x = 12, 1 - p = 6.1e-6: 4 % of (1 - p),
    so the bound is relative there, not a few ulps; the second-order parts above keep it rigorous at that size.
  * IoU gradients: on the edge rows every face, extent, volume and tie weight (1, 1/2, 0) is exact in fp32 — dyadic operands — and the
    only roundings are the last products and the division by U^2; the bound still counts a rounding per operation: a few ulps of the
    gradient, plus a few ulps of the face COORDINATES where an extent is their difference (relative to the 2^-8 overlap of the
    below-eps rows that is 1e-4 — the widest bound among the edge rows, and a clamp that wrongly passes moves that row by 40 %).
    On general rows every comparison is decided by more than 1e-5 (head_cases.loss_violations), 20 times the bound of the compared
    values, so fp32 takes the reference's branches.
The sums: a row's value passes C sequential adds, the row weight, 6 shuffle levels and 2 levels over the four waves, then double over
the blocks, the cast to float and the loss weight: (8 u) sum |row| + 2 u |sum| on top of the sum of the rows' own bounds
(k eps32 sum |term| with k = (C + 8 + 2) / 2 for the additions, the C adds being part of the row's bound).  The rows' own bounds are
needed: a negative at x = 12 is 0.75 p^2 log(1 - p) with 4 % of 1 - p uncertain in fp32 — 0.3 % of that one term, which a single-row
launch consists of.
Rows of weight 0 are == 0.0 in gbbox, label -1 rows == 0.0 in gcent, and a NULL g0 / g1 / g2 leaves its gradient array exactly zero.

Saturated rows are compared with the oracle's own fp32 restatement (oracle/loss_oracle.py::sigmoid_focal_loss_sum on CPU float32), at
relative 1e-6 (+ FLT_MIN: a denormal result has no relative precision), not with float64: mmcv clamps the argument of the log at
FLT_MIN, and at |x| >= 30 the fp32 value of 1 - p is exactly 0 or 1 on any correct libm, so the clamp — log(FLT_MIN) = -87.3 — defines
the value where float64 would still see log(1 - p) = -x.  Everything must be finite.

fc_riou3d_fwd_bwd only where it is well-posed: both yaws 0, partial overlap or containment without a shared face — IoU within 1e-5 and
the six non-yaw gradients within 1e-4 of the gradient's scale of the axis-aligned float64 reference (the bars of
test_iou_losses_vs_reference_goldens); disjoint pairs give IoU 0 and zero gradient; rows of weight 0 exact zeros even under a NaN pred."""
import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from oracle import loss_oracle as lo
from tests import head_cases as HC

pytestmark = pytest.mark.gpu
NAN = float('nan')
G = 64
SHAPES = [(N, C) for N in (1, 255, 256, 257, 513) for C in (1, 18, 32, 33)]


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _nan(*shape):
    return torch.full(shape, NAN, device=_dev())


def _stop_after_a_gpu_fault(e):
    """a HIP error leaves the process without a usable device: nothing more is launched from this session"""
    text = str(e)
    if 'hipError' in text or 'HIP error' in text or 'illegal memory access' in text:
        pytest.exit(f'GPU fault, no further launches: {text[:300]}', returncode=3)


def _held(name, got, ref, n, stats):
    """'' if rows [0, n) of `got` lie within the reference's own bound, element by element, and the guard rows are still NaN"""
    g = got.cpu().numpy().astype(np.float64)
    v, e = ref.v.reshape(g[:n].shape), ref.e.reshape(g[:n].shape)
    if not np.isfinite(g[:n]).all():
        return f'{name}: {int((~np.isfinite(g[:n])).sum())} non-finite elements'
    if not np.isnan(g[n:]).all():
        return f'{name}: rows past {n} were written'
    err = np.abs(g[:n] - v)
    ratio = float((err[e > 0] / e[e > 0]).max()) if (e > 0).any() else 0.0
    stats[name] = max(stats.get(name, 0.0), ratio)
    bad = err > e
    if bad.any():
        i = int(np.argmax(np.where(bad, err / np.maximum(e, 1e-300), 0)))
        return (f'{name}: {int(bad.sum())} of {bad.size} elements miss their bound; worst at flat index {i}: got {g[:n].ravel()[i]:.9e}, '
                f'reference {v.ravel()[i]:.9e}, error {err.ravel()[i]:.3e}, bound {e.ravel()[i]:.3e}')
    return ''


class _Device:
    def __init__(self, c):
        self.points, self.bbox_pred, self.centerness, self.cls = _up(c.points), _up(c.bbox_pred), _up(c.centerness), _up(c.cls)
        self.ct, self.bt, self.labels, self.scene = _up(c.ct), _up(c.bt), _up(c.labels), _up(c.scene)
        self.inv_pos, self.inv_den = _up(c.inv_pos), _up(c.inv_den)
        assert self.labels.dtype == torch.int64 and self.scene.dtype == torch.int32 and self.cls.dtype == torch.float32
        assert self.cls.shape == (c.N, c.C) and self.bt.shape == (c.N, 7) and int(c.scene.max()) < 3 and int(c.scene.min()) >= 0

    def head(self, c):
        return (L.ptr(self.points), L.ptr(self.bbox_pred), L.ptr(self.centerness), L.ptr(self.cls), L.ptr(self.ct), L.ptr(self.bt), L.ptr(self.labels),
                L.ptr(self.scene), L.ptr(self.inv_pos), L.ptr(self.inv_den), c.N, c.C, HC.GAMMA, HC.ALPHA, *HC.LW)


def _fused(c, stats, nulls):
    N, C = c.N, c.C
    d = _Device(c)
    fails = []
    ref = HC.loss_reference(c)
    # forward
    out = _nan(3 + G)
    nbytes = L.query('fc_fcaf3d_loss_ws_bytes', N)
    ws = torch.full((nbytes + 256,), 255, dtype=torch.uint8, device=_dev())
    L.call('fc_fcaf3d_loss_fwd', *d.head(c), L.ptr(out[0:]), L.ptr(out[1:]), L.ptr(out[2:]), L.ptr(ws), nbytes, L.stream())
    torch.cuda.synchronize()
    o = out.cpu().numpy().astype(np.float64)
    if not np.isnan(o[3:]).all() or not bool((ws[nbytes:] == 255).all()):
        fails.append('forward: a store past the three sums or past the workspace')
    for j, key in enumerate(('loss_cls', 'loss_cent', 'loss_bbox')):
        want, bound = float(ref[key].v), float(ref[key].e)
        k_only = (C + 8 + 2) / 2 * HC.EPS32 * abs(HC.LW[j]) * float(np.abs(ref['rows'][j].v).sum())
        print(f'N {N} C {C} {key}: got {o[j]:.9e}, reference {want:.9e}, error {abs(o[j] - want):.3e}, bound {bound:.3e} (summation part alone {k_only:.3e})')
        stats[key] = max(stats.get(key, 0.0), abs(o[j] - want) / bound)
        if not (np.isfinite(o[j]) and abs(o[j] - want) <= bound):
            fails.append(f'{key}: got {o[j]:.9e}, reference {want:.9e}, error {abs(o[j] - want):.3e} over the bound {bound:.3e}')
    # backward, every loss in the objective
    g = [_up(np.array([v], dtype=np.float32)) for v in HC.G_IN]

    def backward(g_ptrs):
        gcls, gcent, gbbox = _nan(N + G, C), _nan(N + G), _nan(N + G, 6)
        L.call('fc_fcaf3d_loss_bwd', *d.head(c), *g_ptrs, L.ptr(gcls), L.ptr(gcent), L.ptr(gbbox), L.stream())
        torch.cuda.synchronize()
        return gcls, gcent, gbbox
    gcls, gcent, gbbox = backward([L.ptr(t) for t in g])
    fails += [m for m in (_held('gcls', gcls, ref['gcls'], N, stats), _held('gcent', gcent, ref['gcent'], N, stats), _held('gbbox', gbbox, ref['gbbox'], N, stats)) if m]
    if not bool((gbbox[:N][_up(c.ct == 0)] == 0.0).all()):
        fails.append('gbbox: a row of weight 0 is not exactly zero')
    if not bool((gcent[:N][_up(c.labels < 0)] == 0.0).all()):
        fails.append('gcent: a label -1 row is not exactly zero')
    # saturated rows: the oracle's fp32 restatement, with the same fp32 products in the same order
    sat = c.sat_rows
    if len(sat):
        is_pos = c.labels[sat, None] == np.arange(C)[None, :]
        s0 = (np.float32(HC.G_IN[0]) * np.float32(HC.LW[0])) * c.inv_pos[c.scene[sat]]
        with np.errstate(under='ignore'):
            want = (HC.focal_fp32(c.cls[sat], is_pos, True).astype(np.float32) * s0[:, None]).astype(np.float64)
        got = gcls[:N].cpu().numpy()[sat].astype(np.float64)
        if not (np.isfinite(got).all() and np.all(np.abs(got - want) <= 1e-6 * np.abs(want) + HC.FLT_MIN)):
            fails.append(f'gcls on saturated rows: max relative error {float((np.abs(got - want) / np.maximum(np.abs(want), HC.FLT_MIN)).max()):.3e}')
    # NULL g0 / g1 / g2 in turn
    if nulls:
        for k, name in enumerate(('gcls', 'gcent', 'gbbox')):
            ptrs = [L.ptr(t) for t in g]
            ptrs[k] = None
            outs = backward(ptrs)
            gg = list(HC.G_IN)
            gg[k] = None
            r = HC.loss_reference(c, g=tuple(gg))
            if not bool((outs[k][:N] == 0.0).all()):
                fails.append(f'NULL g{k}: {name} is not exactly zero')
            fails += [f'NULL g{k}: {m}' for m in (_held('gcls', outs[0], r['gcls'], N, stats), _held('gcent', outs[1], r['gcent'], N, stats),
                                                 _held('gbbox', outs[2], r['gbbox'], N, stats)) if m]
    return fails, d


def _standalone(c, d, stats):
    N, C = c.N, c.C
    fails = []
    gscale = 0.75
    rows_ref, grad_ref = HC.focal_reference(c, gscale)
    w = _up(c.inv_pos[c.scene])
    rows, gx, gs = _nan(N + G), _nan(N + G, C), _up(np.array([gscale], dtype=np.float32))
    L.call('fc_focal_loss_fwd', L.ptr(d.cls), L.ptr(d.labels), L.ptr(w), N, C, HC.GAMMA, HC.ALPHA, L.ptr(rows), L.stream())
    L.call('fc_focal_loss_bwd', L.ptr(d.cls), L.ptr(d.labels), L.ptr(w), N, C, HC.GAMMA, HC.ALPHA, L.ptr(gs), L.ptr(gx), L.stream())
    torch.cuda.synchronize()
    fails += [m for m in (_held('focal rows', rows, rows_ref, N, stats), _held('focal gx', gx, grad_ref, N, stats)) if m]
    # the saturated logits one element per row (C = 1), against the oracle run on CPU float32 element by element
    x = np.array(HC.SAT_LOGITS * 2, dtype=np.float32).reshape(-1, 1)
    lab = np.array([0] * 8 + [-1] * 8, dtype=np.int64)
    dx, dl = _up(x), _up(lab)
    one, sat_rows, sat_gx = _up(np.ones(1, dtype=np.float32)), _nan(16), _nan(16, 1)
    L.call('fc_focal_loss_fwd', L.ptr(dx), L.ptr(dl), None, 16, 1, HC.GAMMA, HC.ALPHA, L.ptr(sat_rows), L.stream())
    L.call('fc_focal_loss_bwd', L.ptr(dx), L.ptr(dl), None, 16, 1, HC.GAMMA, HC.ALPHA, L.ptr(one), L.ptr(sat_gx), L.stream())
    torch.cuda.synchronize()
    for k in range(16):
        xr = torch.from_numpy(x[k:k + 1]).clone().requires_grad_(True)
        val = lo.sigmoid_focal_loss_sum(xr, torch.from_numpy(lab[k:k + 1]))
        val.backward()
        for what, got, want in (('loss', float(sat_rows[k]), float(val.detach())), ('gradient', float(sat_gx[k, 0]), float(xr.grad))):
            if not (np.isfinite(got) and abs(got - want) <= 1e-6 * abs(want) + HC.FLT_MIN):
                fails.append(f'saturated {what} at x = {float(x[k, 0])}, label {int(lab[k])}: got {got:.9e}, the oracle in float32 {want:.9e}')
    # axis-aligned IoU on the decoded boxes, target rows of 6 and of 7 floats
    pred = HC.decoded_boxes(c)
    iou_ref, dp_ref = HC.aiou_reference(pred, c.bt[:, :6])
    dpred = _up(pred)
    for stride, tgt in ((6, _up(c.bt[:, :6])), (7, d.bt)):
        iou, dp = _nan(N + G), _nan(N + G, 6)
        L.call('fc_aiou3d_fwd_bwd', L.ptr(dpred), L.ptr(tgt), stride, N, HC.IOU_EPS, L.ptr(iou), L.ptr(dp), L.stream())
        torch.cuda.synchronize()
        fails += [f'stride {stride} {m}' for m in (_held('IoU', iou, iou_ref, N, stats), _held('d IoU', dp, dp_ref, N, stats)) if m]
    return fails


@pytest.mark.parametrize('N,C', SHAPES)
def test_fused_and_standalone_losses_within_derived_bounds(N, C):
    fails, stats = [], {}
    try:
        for k, c in enumerate(HC.loss_items(N, C)):
            assert HC.loss_violations(c) == []
            tag = f'launch {k} (row class {int(c.kind[0])}, {HC.EDGE_KINDS[c.edge[0]] if c.edge[0] >= 0 else "-"})' if N == 1 else 'all row classes'
            found, d = _fused(c, stats, nulls=k < 2)
            found += _standalone(c, d, stats)
            fails += [f'{tag}: {m}' for m in found]
    except RuntimeError as e:
        _stop_after_a_gpu_fault(e)
        raise
    print(f'N {N} C {C}: largest error / bound per output: ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(stats.items())))
    assert not fails, f'{len(fails)} findings:\n' + '\n'.join(fails[:30])


def test_rotated_iou_where_it_is_well_posed():
    r = HC.riou_cases()
    n = len(r['pred'])
    pred, tgt = r['pred'].copy(), r['target']
    weight = np.ones(n, dtype=np.float32)
    dead = np.arange(n) % 5 == 4
    weight[dead] = 0.0
    pred[dead & (np.arange(n) % 2 == 0)] = np.nan               # a row without weight is never evaluated
    iou, dp = _nan(n + G), _nan(n + G, 7)
    try:
        d_pred, d_tgt, d_w = _up(pred), _up(tgt), _up(weight)
        L.call('fc_riou3d_fwd_bwd', L.ptr(d_pred), L.ptr(d_tgt), L.ptr(d_w), n, L.ptr(iou), L.ptr(dp), L.stream())
        torch.cuda.synchronize()
    except RuntimeError as e:
        _stop_after_a_gpu_fault(e)
        raise
    gi, gd = iou.cpu().numpy().astype(np.float64), dp.cpu().numpy().astype(np.float64)
    assert np.isnan(gi[n:]).all() and np.isnan(gd[n:]).all()
    assert np.all(gi[:n][dead] == 0.0) and np.all(gd[:n][dead] == 0.0)
    live = ~dead
    disjoint = live & (r['kind'] == 3)
    assert disjoint.any() and np.all(gi[:n][disjoint] == 0.0) and np.all(gd[:n][disjoint] == 0.0)
    assert all((live & (r['kind'] == k)).any() for k in range(3))
    err_iou = float(np.abs(gi[:n][live] - r['iou'][live]).max())
    err_g, scale = float(np.abs(gd[:n, :6][live] - r['grad'][live]).max()), float(np.abs(r['grad'][live]).max())
    print(f'rotated IoU at yaw 0: max IoU error {err_iou:.2e}, max gradient error {err_g:.2e} at gradient scale {scale:.3f}')
    assert err_iou <= 1e-5 and err_g <= 1e-4 * scale
