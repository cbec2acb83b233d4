"""-m gpu: the box-voting kernel alone (csrc_post/vote.hip fc_vote_boxes) against merge_augs.vote_boxes, the per-segment statement of
the rule in torch, on the sets of tests/vote_cases.py.  Membership on both sides comes from the same fp32 IoUs
(nms.boxes_iou_bev = csrc/nms.hip's geometry, csrc/bev_geom.h, which vote.hip includes too); the C oracle's IoUs show first that no pair
lies within 1e-5 of the threshold, so that a last-bit difference could not move a member anyway."""
import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from tests import vote_cases as VC

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0


def _run(T, thr, rotated, with_yaw, dev):
    """fc_vote_boxes on the tables of a case, the output pre-filled with a sentinel -> (boxes, members, initial fill) as numpy"""
    t = {k: torch.from_numpy(v).to(dev) for k, v in T.items()}
    nseg, stride, _ = T['boxes'].shape
    out = torch.full((nseg, stride, 7), SENTINEL, dtype=torch.float32, device=dev)
    init = out.cpu().numpy()
    mem = torch.full((nseg, T['keep'].shape[1]), -1, dtype=torch.int32, device=dev)
    flags = (1 if rotated else 0) | (2 if with_yaw else 0)
    L.call('fc_vote_boxes', L.ptr(t['boxes']), L.ptr(t['scores']), L.ptr(t['counts']), nseg, stride, stride, L.ptr(t['keep']),
           L.ptr(t['kcounts']), T['keep'].shape[1], T['keep'].shape[1], float(thr), flags, L.ptr(out), L.ptr(mem), L.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), mem.cpu().numpy(), init


def _case(T, thr, rotated, with_yaw, exact_bits=False):
    dev = torch.device('cuda:0')
    want = VC.expected(T, thr, rotated, with_yaw, device=dev)
    got, mem, init = _run(T, thr, rotated, with_yaw, dev)
    worst = VC.check(T, got, mem, init, want, exact_bits=exact_bits)
    again, mem2, _ = _run(T, thr, rotated, with_yaw, dev)
    assert got.tobytes() == again.tobytes() and mem.tobytes() == mem2.tobytes(), 'a second call gave other bits'
    n_mem = sum(int(c.sum()) for _, c, _ in want)
    n_kept = int(T['kcounts'].sum())
    print(f'rotated={rotated} with_yaw={with_yaw}: {n_kept} kept boxes, {n_mem / max(n_kept, 1):.2f} members each, worst error '
          f'{worst:.3f} of the bound')
    return want


def test_the_cases_mirror_the_kernels_constants():
    assert VC.constants_of_the_kernel() == (VC.TILE, VC.WAVES, VC.KEPT_PER_BLOCK)


@pytest.mark.parametrize('with_yaw', [True, False])
def test_crafted_segments(with_yaw):
    """lengths 0, 1, T-1, T, T+1, 2T+1; kept counts 0, 1, all, one more than a workgroup's waves, one more than a round of the grid;
    empty segments between full ones; stride > count with NaN padding; 7-column boxes with yaws pi/2 and pi apart and exchanged
    sides (rotated IoU), and the 6-column use (yaw 0, axis-aligned IoU)"""
    T = VC.crafted(with_yaw)
    VC.assert_clear_of_threshold(T, VC.THR, rotated=with_yaw)
    want = _case(T, VC.THR, with_yaw, with_yaw)
    assert max(int(c.max()) for _, c, _ in want if len(c)) >= 3
    if with_yaw:
        # some member votes with exchanged sides, some with a yaw half a turn on
        seen_q = seen_h = False
        for k, (_, _, mem) in enumerate(want):
            n, kc = int(T['counts'][k]), int(T['kcounts'][k])
            if not kc:
                continue
            yaw = T['boxes'][k, :n, 6].astype(np.float64)
            d = np.abs(yaw[None, :] - yaw[T['keep'][k, :kc]][:, None])[mem.numpy()]
            seen_q |= bool((np.abs(d - np.pi / 2) < 0.3).any())
            seen_h |= bool((np.abs(d - np.pi) < 0.3).any())
        assert seen_q and seen_h


@pytest.mark.parametrize('seed', VC.GENERAL_SEEDS)
@pytest.mark.parametrize('with_yaw', [True, False])
def test_random_segments(seed, with_yaw):
    T = VC.general(seed, with_yaw)
    VC.assert_clear_of_threshold(T, VC.THR, rotated=with_yaw)
    _case(T, VC.THR, with_yaw, with_yaw)


def test_exact_duplicates_vote_at_threshold_one_bit_for_bit():
    """equality with the threshold votes: at vote_thr = 1.0 the members are exactly the duplicates of a footprint; binary-fraction
    boxes and power-of-two scores make every sum exact, so the kernel's output equals the statement's to the bit"""
    from oracle import bev
    T = VC.exact()
    dup = 0
    for k in range(len(T['counts'])):
        n = int(T['counts'][k])
        iou = bev.iou_matrix(T['boxes'][k, :n], T['boxes'][k, :n], rotated=False)
        assert ((iou == 1.0) | (iou < 1.0 - 1e-5)).all()
        dup += int((iou == 1.0).sum()) - n
    assert dup > 20
    want = _case(T, 1.0, False, False, exact_bits=True)
    assert max(int(c.max()) for _, c, _ in want) >= 3
    changed = sum(int((o[:, :6] != torch.from_numpy(T['boxes'][k, :len(o), :6])).any(1).sum()) for k, (o, _, _) in enumerate(want))
    assert changed > 5                                                  # the vote moved boxes: bit-equality is not that of a copy


def test_a_weight_sum_that_is_not_positive_leaves_the_box():
    rng = np.random.default_rng(3)
    b, s = VC.random_boxes(rng, 12, True)
    s[:] = 0.0
    s[5:] = -0.25
    T = VC.pack([(b, s, np.arange(0, 12, 2))])
    got, mem, _ = _run(T, 0.3, True, True, torch.device('cuda:0'))
    assert np.array_equal(got[0, :12], b) and (mem[0, :6] >= 1).all()
    want = VC.expected(T, 0.3, True, True, device=torch.device('cuda:0'))
    assert torch.equal(want[0][0], torch.from_numpy(b)) and np.array_equal(mem[0, :6], want[0][1].numpy())
