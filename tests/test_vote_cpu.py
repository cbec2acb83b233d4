"""CPU: box voting for the test-time augmentation merge.  merge_augs.vote_boxes on hand-computed cases (IoUs passed in: no GPU), the
argument checks of fc_vote_boxes (which return before any launch), and the kernel's text compiled for the host under
AddressSanitizer and UBSan (tools/vote_host_emu.cpp) on the segment sets tests/test_gpu_vote.py runs on the GPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from fcaf3d_amd.merge_augs import vote_boxes, vote_cfg
from tests import vote_cases as VC

NAN = float('nan')


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def _seq(scores, values):
    """fp32(sum_j s_j v_j / sum_j s_j), both sums in float64 in the order given"""
    acc = den = 0.0
    for w, v in zip(scores.tolist(), values):
        acc += w * v
        den += w
    return float(np.float32(acc / den))


def test_vote_boxes_by_hand():
    boxes = _f32([[0., 0., 0., 2., 1., 1., 0.], [1., 0., 1., 2., 1., 2., 0.], [4., 4., 0., 1., 1., 1., 0.], [5., 4., 2., 1., 3., 1., 0.]])
    scores = _f32([0.5, 0.25, 0.25, 0.125])
    keep = torch.tensor([0, 2])
    # row 0: itself though its own IoU is NaN, and box 1; row 2: box 1 by EQUALITY with the threshold, itself, box 3; NaN is no member
    iou = _f32([[NAN, 0.7, 0.2, NAN], [0.1, 0.5, 0.0, 0.6]])
    out, cnt = vote_boxes(boxes, scores, keep, 0.5, False, False, iou=iou, return_members=True)
    assert cnt.tolist() == [2, 3] and cnt.dtype == torch.int32
    w0 = (0.5 * boxes[0, :6].double() + 0.25 * boxes[1, :6].double()) / 0.75
    w2 = (0.25 * boxes[1, :6].double() + 0.25 * boxes[2, :6].double() + 0.125 * boxes[3, :6].double()) / 0.625
    assert torch.equal(out[0, :6], w0.float()) and torch.equal(out[2, :6], w2.float())
    assert out[0, :6].tolist() == [np.float32(1 / 3), 0.0, np.float32(1 / 3), 2.0, 1.0, np.float32(4 / 3)]
    assert torch.equal(out[[1, 3]], boxes[[1, 3]]) and torch.equal(out[:, 6], boxes[:, 6])         # rows not kept, the yaw column
    # six columns in, six columns out
    out6 = vote_boxes(boxes[:, :6], scores, keep, 0.5, False, False, iou=iou)
    assert out6.shape == (4, 6) and torch.equal(out6, out[:, :6])
    # nothing kept, nothing there
    assert torch.equal(vote_boxes(boxes, scores, keep[:0], 0.5, False, False, iou=iou[:0]), boxes)
    assert vote_boxes(boxes[:0], scores[:0], keep[:0], 0.5, False, False, iou=iou[:0, :0]).shape == (0, 7)


def test_vote_boxes_exchanges_the_sides_of_a_quarter_turn():
    pi = math.pi
    # one rectangle (2 x 1 at yaw 0.1) written three more ways: sides exchanged at +pi/2 and at -pi/2, and as it is half a turn on
    boxes = _f32([[0., 0., 0., 2., 1., 1., 0.1], [0., 0., 0., 1., 2., 1., 0.1 + pi / 2], [0., 0., 0., 1., 2., 1., 0.1 - pi / 2],
                  [0., 0., 0., 2., 1., 1., 0.1 + pi], [0., 0., 0., 4., 1., 1., 0.1 + 0.7]])
    scores = _f32([0.5, 0.4, 0.3, 0.2, 0.1])
    iou = torch.full((1, 5), 0.9)
    out = vote_boxes(boxes, scores, torch.tensor([0]), 0.5, True, True, iou=iou)
    # box 4 (0.7 rad off: under pi/4) votes as it is: l = (2 * 1.4 + 4 * 0.1) / 1.5, w = 1
    assert out[0, 3:5].tolist() == [_seq(scores, [2, 2, 2, 2, 4]), 1.0]
    assert abs(out[0, 3] - 3.2 / 1.5) < 1e-6
    assert out[0, 6] == boxes[0, 6]
    # without yaws nothing is exchanged
    flat = vote_boxes(boxes, scores, torch.tensor([0]), 0.5, True, False, iou=iou)
    assert flat[0, 3:5].tolist() == [_seq(scores, [2, 1, 1, 2, 4]), _seq(scores, [1, 2, 2, 1, 1])]
    assert abs(flat[0, 3] - (2 * 0.7 + 1 * 0.7 + 4 * 0.1) / 1.5) < 1e-6 and abs(flat[0, 4] - (1 * 0.8 + 2 * 0.7) / 1.5) < 1e-6


def test_vote_boxes_leaves_a_box_whose_weights_do_not_sum_to_a_positive_finite_number():
    boxes = _f32([[0., 0., 0., 2., 1., 1., 0.], [1., 0., 1., 2., 1., 2., 0.]])
    iou = torch.full((1, 2), 0.9)
    for s in ([0.0, 0.0], [0.5, -0.5], [0.25, -0.5], [float('inf'), 1.0], [NAN, 1.0]):
        out, cnt = vote_boxes(boxes, _f32(s), torch.tensor([0]), 0.5, False, False, iou=iou, return_members=True)
        assert torch.equal(out, boxes) and cnt.tolist() == [2], s


def test_vote_cfg_reads_the_threshold():
    assert vote_cfg(dict(iou_thr=0.5)) is None and vote_cfg(dict(vote_thr=None)) is None
    assert vote_cfg(dict(vote_thr=0.6)) == 0.6 and vote_cfg(dict(vote_thr=1)) == 1.0
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match='vote_thr'):
            vote_cfg(dict(vote_thr=bad))


def test_library_checks_need_no_gpu():
    fn = L.lib().fc_vote_boxes
    p = 0x1000                       # never dereferenced: every call below returns before a launch

    def call(nseg=2, stride=8, max_count=8, keep_stride=8, max_keep=8, thr=0.5, flags=3):
        return fn(p, p, p, nseg, stride, max_count, p, p, keep_stride, max_keep, thr, flags, p, None, None)
    assert call(nseg=-1) == -1 and call(stride=-1) == -1 and call(keep_stride=-1) == -1 and call(max_count=-1) == -1 and call(max_keep=-1) == -1
    assert call(stride=7) == -1 and call(keep_stride=7) == -1              # strides below counts
    assert call(thr=0.0) == -1 and call(thr=1.0001) == -1 and call(thr=NAN) == -1 and call(thr=-0.5) == -1
    assert call(flags=4) == -1
    assert call(nseg=0) == 0 and call(max_count=0, stride=0) == 0          # nothing to do: nothing launched
    E = L.parse_header()
    assert 'fc_vote_boxes' in E and L.ABI_VERSION == 19


# ---- the kernel's text on the host (tools/vote_host_emu.cpp) -----------------------------------------------------------------------------

def _build_emulator(tmp):
    """csrc_post/vote.hip from its VOTE_* constants to the end of its anonymous namespace (constants, grid helper, kernel), compiled for
    the host with AddressSanitizer and UBSan: the emulator restates none of them"""
    from fcaf3d_amd import build as B
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(B.CSRC_POST, 'vote.hip')).read()
    end = '}  // namespace'
    body = src[src.index('#define VOTE_THREADS'):src.index(end) + len(end)]
    assert '#include' not in body and all(f'#define {n} ' in body for n in ('VOTE_TILE', 'VOTE_WAVES', 'VOTE_KEPT_PER_BLOCK')), 'vote.hip was reordered'
    (tmp / 'kernels.inc').write_text(body)
    (tmp / 'hip').mkdir()
    (tmp / 'hip' / 'hip_runtime.h').write_text('#pragma once\n#include <cmath>\n')
    cxx = os.path.join(os.path.dirname(os.path.dirname(B.HIPCC)), 'llvm', 'bin', 'clang++')
    cxx = cxx if os.path.exists(cxx) else shutil.which('clang++')
    exe = str(tmp / 'vote_host_emu')
    subprocess.check_call([cxx, '-std=c++20', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-pthread', f'-I{tmp}', f'-I{B.CSRC_POST}', f"-I{os.path.join(root, 'include')}",
                           os.path.join(root, 'tools', 'vote_host_emu.cpp'), '-o', exe])
    return exe


SENTINEL = 12345.0


def _emulate(exe, tmp, T, thr, rotated, with_yaw):
    nseg, stride, _ = T['boxes'].shape
    ks = T['keep'].shape[1]
    init = np.full((nseg, stride, 7), SENTINEL, np.float32)
    flags = (1 if rotated else 0) | (2 if with_yaw else 0)
    with open(tmp / 'in.bin', 'wb') as f:
        np.array([nseg, stride, stride, ks, ks, flags, 1, int(np.float32(thr).view(np.uint32))], np.int64).tofile(f)
        for a in (T['boxes'], T['scores'], T['counts'], T['keep'], T['kcounts'], init):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([exe, str(tmp / 'in.bin'), str(tmp / 'out.bin')], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    raw = open(tmp / 'out.bin', 'rb').read()
    nb = nseg * stride * 7 * 4
    return (np.frombuffer(raw[:nb], np.float32).reshape(nseg, stride, 7), np.frombuffer(raw[nb:], np.int32).reshape(nseg, ks), init)


def test_kernel_text_on_the_host_equals_the_float64_statement(tmp_path):
    """the kernel of csrc_post/vote.hip, compiled for the host under AddressSanitizer and UBSan (a thread per GPU thread, a barrier
    for __syncthreads, a barrier per 64 threads for __ballot), on the GPU test's crafted segments (7 columns with yaws and the
    rotated IoU; yaw 0 and the axis-aligned IoU) and on its exact set: no access leaves its table (the tables are allocated at their
    exact sizes, the padding rows are NaN), member counts equal merge_augs.vote_boxes's on the C oracle's IoUs (no pair within 1e-5
    of the threshold; the host-libm IoU of the emulator differs from the oracle's by far less), outputs within
    2^-23 * max_{j in M} |box_j[k]|, bit-equal on the exact set."""
    from oracle import bev
    assert VC.constants_of_the_kernel() == (VC.TILE, VC.WAVES, VC.KEPT_PER_BLOCK)
    exe = _build_emulator(tmp_path)
    for with_yaw in (True, False):
        T = VC.crafted(with_yaw)
        ious = VC.assert_clear_of_threshold(T, VC.THR, rotated=with_yaw)
        want = VC.expected(T, VC.THR, with_yaw, with_yaw, ious=ious)
        got, mem, init = _emulate(exe, tmp_path, T, VC.THR, with_yaw, with_yaw)
        worst = VC.check(T, got, mem, init, want)
        print(f'crafted, with_yaw={with_yaw}: worst error {worst:.3f} of the bound')
    T = VC.exact()
    ious = [bev.iou_matrix(T['boxes'][k, :n][T['keep'][k, :kc]], T['boxes'][k, :n], rotated=False)
            for k, (n, kc) in enumerate(zip(T['counts'], T['kcounts']))]
    assert all(((i == 1.0) | (i < 1.0 - 1e-5)).all() for i in ious)
    want = VC.expected(T, 1.0, False, False, ious=ious)
    got, mem, init = _emulate(exe, tmp_path, T, 1.0, False, False)
    VC.check(T, got, mem, init, want, exact_bits=True)
    assert max(int(c.max()) for _, c, _ in want) >= 3
