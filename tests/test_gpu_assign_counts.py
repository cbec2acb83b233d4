"""-m gpu: the inside-location counters of the target assignment (csrc/assign.hip k_count: counts[scene][box][level], the lanes of
a wave that hit the same counter add once) read back from the workspace of fc_assign_targets and held against a numpy inside test.
2 scenes, 3 boxes, 2 levels; coordinates and box sizes are multiples of 1/8 and no location lies on a face, so the fp32 inside test
of the kernel and the float64 one here cannot disagree."""
import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L

pytestmark = pytest.mark.gpu

B, M, LV = 2, 3, 2
# [cx, cy, cz, w, l, h, yaw] (gravity centre): scene 0: box 1 contains box 2, box 0 apart; scene 1: three boxes apart
BOXES = np.array([[[2, 2, 1, 1, 1, 1, 0], [10, 2, 1, 4, 2, 2, 0], [9, 2, 1, 1, 1, 1, 0]],
                  [[2, 10, 1, 2, 2, 2, 0], [10, 10, 1, 1, 1, 1, 0], [20, 10, 1, 1, 1, 1, 0]]], dtype=np.float32)


def _line(n, x0, y, z=1.0, step=0.0):
    p = np.empty((n, 3), dtype=np.float32)
    p[:, 0] = x0 + step * np.arange(n)
    p[:, 1] = y
    p[:, 2] = z
    return p


def _inside(p, box):
    return np.all(np.abs(p.astype(np.float64) - box[:3]) < box[3:6] / 2, axis=1)


def _alternating(n, xa, xb, y):
    p = _line(n, xa, y)
    p[1::2, 0] = xb
    return p


CASES = {
    # 200 consecutive locations inside box 1 of scene 0, the first 100 of them inside box 2 as well: whole waves on one counter, a
    # wave whose lanes 36.. leave box 2, and a level with a handful of hits
    'one_box': {(0, 0): np.concatenate([_line(100, 8.75, 2.0, step=1 / 256), _line(100, 10.5, 2.25, step=1 / 256), _line(30, 30.0, 30.0)]),
                (0, 1): _line(70, 40.0, 2.0), (1, 0): _line(5, 10.0, 2.0), (1, 1): _line(3, 2.0, 10.0)},
    # locations alternating between boxes 0 and 2 of scene 0 (two counters inside every wave), and between a box and nowhere in scene 1
    'two_boxes': {(0, 0): _alternating(333, 2.0, 9.0, 2.0), (0, 1): _alternating(64, 10.0, 20.0, 10.0),
                  (1, 0): _alternating(130, 9.25, 1.75, 2.25), (1, 1): _alternating(65, 50.0, 2.0, 10.0)},
    # no location inside any box of its OWN scene (scene 1's locations sit in scene 0's box 1, scene 0's level-1 ones in scene 1's box 0)
    'none': {(0, 0): _line(300, 30.0, 30.0, step=1 / 8), (0, 1): _line(10, 10.0, 2.0),
             (1, 0): _line(129, 2.0, 10.0), (1, 1): _line(1, 10.0, 2.0)},
}
# keys: (level, scene)


@pytest.mark.parametrize('case', sorted(CASES))
def test_inside_counters_equal_a_numpy_inside_test(case):
    dev = torch.device('cuda:0')
    segs = CASES[case]
    pts, scene, level, seg_start = [], [], [], [0]
    for l in range(LV):                                  # rows grouped by (level, scene), as the head's location arrays are
        for s in range(B):
            p = segs[(l, s)]
            pts.append(p)
            scene += [s] * len(p)
            level += [l] * len(p)
            seg_start.append(seg_start[-1] + len(p))
    pts = np.concatenate(pts)
    scene, level = np.array(scene, dtype=np.int32), np.array(level, dtype=np.int32)
    N = len(pts)
    want = np.zeros((B, M, LV), dtype=np.int64)
    for s in range(B):
        for j in range(M):
            hit = _inside(pts, BOXES[s, j].astype(np.float64)) & (scene == s)
            for l in range(LV):
                want[s, j, l] = int((hit & (level == l)).sum())
    if case == 'none':
        assert want.sum() == 0
    elif case == 'one_box':
        assert want[0, 1, 0] == 200 and want[0, 2, 0] == 100 and want[0, 1, 1] == 5
    else:
        assert want[0, 0, 0] == 167 and want[0, 2, 0] == 166

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    d_pts, d_scene, d_level = up(pts, torch.float32), up(scene, torch.int32), up(level, torch.int32)
    d_boxes, d_labels = up(BOXES, torch.float32), torch.zeros((B, M), dtype=torch.int64, device=dev)
    d_cnt, d_order, d_seg = up(np.full(B, M), torch.int32), torch.arange(N, dtype=torch.int32, device=dev), up(np.array(seg_start), torch.int32)
    ct = torch.empty(N, dtype=torch.float32, device=dev)
    bt = torch.empty((N, 7), dtype=torch.float32, device=dev)
    lab = torch.empty(N, dtype=torch.int64, device=dev)
    ws = torch.full((L.query('fc_assign_ws_bytes', B, M, LV),), 0x5a, dtype=torch.uint8, device=dev)
    L.call('fc_assign_targets', L.ptr(d_pts), L.ptr(d_scene), L.ptr(d_level), N, L.ptr(d_boxes), L.ptr(d_labels), L.ptr(d_cnt), B, M, LV,
           L.ptr(d_order), L.ptr(d_seg), 27, 18, L.ptr(ct), L.ptr(bt), L.ptr(lab), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    got = ws[:B * M * LV * 4].view(torch.int32).view(B, M, LV).cpu().numpy()
    print(case, 'counts', got.tolist())
    assert got.tolist() == want.tolist()
    # what the counters feed: a location is labelled iff some box of its scene holds it (every box here has < topk candidates
    # on its best level or the location is among them; background otherwise) — with no hit at all, everything is background
    if case == 'none':
        assert int((lab >= 0).sum()) == 0 and float(ct.abs().sum()) == 0.0
