"""Generates tests/golden/eiou3d.npz: the enclosing-box losses of the reference, run by the reference's own code in FLOAT64 on
float32-representable inputs (build container only — the reference never travels).

Run:  python tests/golden/make_golden_eiou.py

Imported through make_golden.load_reference():
  * mmdet3d/ops/rotated_iou/oriented_iou_loss.py   cal_giou_3d, cal_diou_3d (and cal_iou_3d for the corners)
  * mmdet3d/ops/rotated_iou/min_enclosing_box.py   gather_lines_points, point_line_projection_range, point_line_distance_range, LINES
  * mmdet3d/core/bbox/iou_calculators/iou3d_calculator.py   axis_aligned_bbox_overlaps_3d(mode='giou' / 'iou', is_aligned=True)

Groups (all rows: pred, target, w; per kind k in (giou, diou): loss64, grad64 = d(sum w loss)/d pred in float64, loss32 / grad32 = the
reference's own float32 run; iou64):
  ro       256 rotated pairs of the base distribution
  ro_far   64 pairs moved 2.5-5 in x and y (disjoint in BEV) + 64 pairs moved 3 in z: IoU 0, a non-zero gradient on every active row
  ro_axis  64 pairs with the target yaw exactly 0, pi/2, -pi/2 or pi and the pred yaw off by +-U(0.1, 0.5)
  al       256 axis-aligned pairs, 64 of them disjoint, no two compared coordinates closer than 1e-3.  The aligned DIoU has no
           reference function of its own: 1 - iou + d2 / max(c2, eps) over the reference's aligned IoU, checked here against
           cal_diou_3d(enclosing_type='aligned') at yaw 0

A gradient is only defined away from the kink where two different enclosing rectangles tie (parallel boxes are one such place).  A
rotated pair is kept only if, of the 24 candidate areas in float64, the winner is the only one within MARGIN (relative) of the minimum,
or the winner is an edge of one box and every other candidate within the margin is an edge of the same box (the same rectangle, hence
the same derivative).  Dropped pairs are replaced by fresh draws; at most 10 % of a group may be dropped; the counts are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference  # noqa: E402

MARGIN = 1e-4
KINDS = ('giou', 'diou')


def base_pairs(rng, n):
    t = np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(0.3, 2, (n, 3)), rng.uniform(-3.1, 3.1, (n, 1))], 1).astype(np.float32)
    p = t.astype(np.float64).copy()
    p[:, :3] += rng.uniform(-0.6, 0.6, (n, 3))
    p[:, 3:6] *= rng.uniform(0.6, 1.5, (n, 3))
    p[:, 6] += rng.uniform(-0.5, 0.5, n)
    return p.astype(np.float32), t


def weights(rng, n):
    w = rng.uniform(0.1, 1, n).astype(np.float32)
    w[rng.permutation(n)[:n // 4]] = 0
    return w


def draw_ro(rng, n):
    return base_pairs(rng, n)


def draw_far_xy(rng, n):
    p, t = base_pairs(rng, n)
    p[:, :2] = (t[:, :2] + rng.uniform(2.5, 5, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))).astype(np.float32)
    return p, t


def draw_far_z(rng, n):
    p, t = base_pairs(rng, n)
    p[:, 2] = (t[:, 2] + 3.0 * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return p, t


def draw_axis(rng, n):
    p, t = base_pairs(rng, n)
    t[:, 6] = rng.choice(np.array([0, np.pi / 2, -np.pi / 2, np.pi], np.float32), n)
    p[:, 6] = (t[:, 6] + rng.uniform(0.1, 0.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return p, t


def candidate_areas(riou, meb, p, t):
    """the 24 candidate areas of smallest_bounding_box in float64, zero areas replaced by 1e8"""
    P, T = torch.from_numpy(p).double()[None], torch.from_numpy(t).double()[None]
    _, c1, c2, _, _ = riou.cal_iou_3d(P, T, verbose=True)
    lines, points, _, _ = meb.gather_lines_points(torch.cat([c1, c2], dim=-2))
    area = meb.point_line_projection_range(lines, points) * meb.point_line_distance_range(lines, points)
    area = area + (area == 0).double() * 1e8
    return area[0].numpy()


def clear_winner(meb, area):
    lines = np.asarray(meb.LINES)
    same_box_edge = lambda k: (lines[k] // 4)[0] == (lines[k] // 4)[1]          # both ends on one box: an edge (diagonals are not listed)
    keep = np.zeros(len(area), bool)
    for r, a in enumerate(area):
        w = int(np.argmin(a))
        near = [k for k in np.nonzero(a <= a[w] * (1 + MARGIN))[0] if k != w]
        if not near:
            keep[r] = True
        elif same_box_edge(w) and all(same_box_edge(k) and lines[k][0] // 4 == lines[w][0] // 4 for k in near):
            keep[r] = True
    return keep


def rotated_group(riou, meb, rng, draw, n):
    ps, ts, have, dropped = [], [], 0, 0
    while have < n:
        p, t = draw(rng, n - have)
        keep = clear_winner(meb, candidate_areas(riou, meb, p, t))
        dropped += int((~keep).sum())
        ps.append(p[keep]); ts.append(t[keep]); have += int(keep.sum())
    assert dropped <= 0.1 * n, (draw.__name__, dropped, n)
    return np.concatenate(ps), np.concatenate(ts), dropped


def run_rotated(riou, p, t, w, dtype):
    out = {}
    for kind, fn in zip(KINDS, (riou.cal_giou_3d, riou.cal_diou_3d)):
        P = torch.from_numpy(p).to(dtype).requires_grad_(True)
        loss, iou = fn(P[None], torch.from_numpy(t).to(dtype)[None])
        (loss[0] * torch.from_numpy(w).to(dtype)).sum().backward()
        out[kind] = (loss[0].detach().numpy(), iou[0].detach().numpy(), P.grad.numpy())
    return out


def corners6(x):
    return torch.cat([x[:, :3] - x[:, 3:6] / 2, x[:, :3] + x[:, 3:6] / 2], 1)


def run_aligned(aiou, riou, p, t, w, dtype):
    out = {}
    T = torch.from_numpy(t).to(dtype)
    W = torch.from_numpy(w).to(dtype)
    P = torch.from_numpy(p).to(dtype).requires_grad_(True)
    loss = 1 - aiou(corners6(P), corners6(T), mode='giou', is_aligned=True)
    (loss * W).sum().backward()
    iou = aiou(corners6(P), corners6(T), mode='iou', is_aligned=True).detach()
    out['giou'] = (loss.detach().numpy(), iou.numpy(), P.grad.numpy())
    P = torch.from_numpy(p).to(dtype).requires_grad_(True)
    cp, ct = corners6(P), corners6(T)
    i = aiou(cp, ct, mode='iou', is_aligned=True)
    enc = (torch.max(cp[:, 3:], ct[:, 3:]) - torch.min(cp[:, :3], ct[:, :3])).clamp(min=0)
    c2 = torch.max((enc * enc).sum(1), enc.new_tensor([1e-6]))
    loss = 1 - i + ((P[:, :3] - T[:, :3]) ** 2).sum(1) / c2
    (loss * W).sum().backward()
    out['diou'] = (loss.detach().numpy(), i.detach().numpy(), P.grad.numpy())
    if dtype == torch.float64:          # the same quantity through the reference's cal_diou_3d(enclosing_type='aligned') at yaw 0
        z = torch.zeros(len(p), 1, dtype=dtype)
        ref, _ = riou.cal_diou_3d(torch.cat([P.detach(), z], 1)[None], torch.cat([T, z], 1)[None], enclosing_type='aligned')
        assert float((ref[0] - loss.detach()).abs().max()) < 1e-5
    return out


def aligned_part(rng, n, far):
    ps, ts, have = [], [], 0
    while have < n:
        m = n - have
        p, t = base_pairs(rng, m)
        p, t = p[:, :6].copy(), t[:, :6].copy()
        if far:
            p[:, :3] = (t[:, :3] + rng.uniform(2.5, 5, (m, 3)) * rng.choice([-1.0, 1.0], (m, 3))).astype(np.float32)
        a, b = corners6(torch.from_numpy(p).double()).numpy(), corners6(torch.from_numpy(t).double()).numpy()
        # every pair of coordinates a max / min / clamp compares: the two low faces, the two high faces, each high face with the other low
        gaps = np.concatenate([np.abs(a - b), np.abs(a[:, 3:] - b[:, :3]), np.abs(b[:, 3:] - a[:, :3])], 1).min(1)
        keep = gaps >= 1e-3
        ps.append(p[keep]); ts.append(t[keep]); have += int(keep.sum())
    return np.concatenate(ps), np.concatenate(ts)


def aligned_group(rng, n, n_far):
    pf, tf = aligned_part(rng, n_far, True)
    pn, tn = aligned_part(rng, n - n_far, False)
    return np.concatenate([pf, pn]), np.concatenate([tf, tn])


def main():
    head, utils, aiou, riou = load_reference()
    meb = sys.modules['rotated_iou.min_enclosing_box']
    rng = np.random.default_rng(16)
    d = {'margin': np.float64(MARGIN)}
    groups = {}
    p, t, dr = rotated_group(riou, meb, rng, draw_ro, 256)
    groups['ro'] = (p, t); d['ro_dropped'] = np.int64(dr)
    pa, ta, da = rotated_group(riou, meb, rng, draw_far_xy, 64)
    pb, tb, db = rotated_group(riou, meb, rng, draw_far_z, 64)
    groups['ro_far'] = (np.concatenate([pa, pb]), np.concatenate([ta, tb])); d['ro_far_dropped'] = np.int64(da + db)
    p, t, dr = rotated_group(riou, meb, rng, draw_axis, 64)
    groups['ro_axis'] = (p, t); d['ro_axis_dropped'] = np.int64(dr)
    groups['al'] = aligned_group(rng, 256, 64)
    for g, (p, t) in groups.items():
        w = weights(rng, len(p))
        run = (lambda dt: run_aligned(aiou, riou, p, t, w, dt)) if g == 'al' else (lambda dt: run_rotated(riou, p, t, w, dt))
        r64, r32 = run(torch.float64), run(torch.float32)
        d.update({f'{g}_pred': p, f'{g}_target': t, f'{g}_w': w, f'{g}_iou64': r64['giou'][1]})
        for k in KINDS:
            l64, i64, g64 = r64[k]
            l32, _, g32 = r32[k]
            assert np.isfinite(l64).all() and np.isfinite(g64).all(), (g, k)
            assert np.abs(i64 - r64['giou'][1]).max() < 1e-12
            scale = np.abs(g64).max()
            print(f'{g:8s} {k}: rows {len(p)} dropped {int(d.get(g + "_dropped", 0))}  grad scale {scale:.3f}  reference fp32 vs fp64: '
                  f'loss {np.abs(l32 - l64).max():.2e}  grad {np.abs(g32 - g64).max():.2e} ({np.abs(g32 - g64).max() / scale:.2e} of scale)')
            d.update({f'{g}_{k}_loss64': l64, f'{g}_{k}_grad64': g64, f'{g}_{k}_loss32': l32.astype(np.float32),
                      f'{g}_{k}_grad32': g32.astype(np.float32)})
            if g == 'ro_far':
                assert (i64 == 0).all(), 'ro_far must be disjoint'
                assert (np.abs(g64[w > 0]).max(1) > 0).all(), 'every active disjoint row must carry a gradient'
            assert (g64[w == 0] == 0).all()
    n_far = 64
    assert (d['al_iou64'][:n_far] == 0).all() and (d['al_iou64'][n_far:] > 0).sum() > 100
    out = os.path.join(HERE, 'eiou3d.npz')
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) < 200 * 1024


if __name__ == '__main__':
    main()
