"""CPU: the enclosing-box losses (GIoU3DLoss, DIoU3DLoss; fcaf3d_amd/csrc_post/eiou.hip) as far as they go without a GPU: the registry,
the refusal of CPU tensors, the enum, the argument checks of fc_eiou3d_fwd_bwd (which return before any launch), and the kernel's text
compiled for the host under AddressSanitizer and UBSan (tools/eiou_host_emu.cpp) against the float64 fixture
tests/golden/eiou3d.npz (tests/golden/make_golden_eiou.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KINDS = ('giou', 'diou')
GROUPS = ('ro', 'ro_far', 'ro_axis', 'al')
SIZES = (1, 63, 64, 65, 257, 2100)          # 2100: three workgroups of 1024 rows, the last one partly filled
PATTERNS = ('all zero', 'last row', 'alternating')


def fixture():
    return np.load(os.path.join(G, 'eiou3d.npz'))


def pattern_weight(pattern, n):
    """the three weight patterns of the size tests"""
    w = np.zeros(n, np.float32)
    if pattern == 'last row':
        w[-1] = 0.5
    elif pattern == 'alternating':
        w[::2] = 0.25 + 0.5 * (np.arange(len(w[::2])) % 2)
    return w


def check_against_fixture(d, g, kind, loss, iou, wgrad, report=None):
    """loss and iou within 1e-5 of the float64 values, wgrad = d(sum w loss)/d pred within 1e-4 of the group's gradient scale (the bars
    tests/test_gpu_model.py::test_iou_losses_vs_reference_goldens holds IoU3DLoss to); rows without weight exactly zero"""
    w = d[f'{g}_w']
    act = w > 0
    l64, i64, g64 = d[f'{g}_{kind}_loss64'], d[f'{g}_iou64'], d[f'{g}_{kind}_grad64']
    scale = float(np.abs(g64).max())
    e_loss = float(np.abs(loss[act].astype(np.float64) - l64[act]).max())
    e_iou = float(np.abs(iou[act].astype(np.float64) - i64[act]).max())
    e_grad = float(np.abs(wgrad.astype(np.float64) - g64).max())
    r_loss = float(np.abs(d[f'{g}_{kind}_loss32'].astype(np.float64) - l64).max())
    r_grad = float(np.abs(d[f'{g}_{kind}_grad32'].astype(np.float64) - g64).max())
    print(f'{report or "eiou"} {g:8s} {kind}: loss {e_loss:.2e} iou {e_iou:.2e} grad {e_grad:.2e} = {e_grad / scale:.2e} of the scale {scale:.3f}'
          f'   (the reference in float32: loss {r_loss:.2e} grad {r_grad / scale:.2e} of the scale)')
    assert (loss[~act] == 0).all() and (iou[~act] == 0).all() and (wgrad[~act] == 0).all(), (g, kind)
    assert np.isfinite(loss).all() and np.isfinite(wgrad).all(), (g, kind)
    assert e_loss < 1e-5 and e_iou < 1e-5, (g, kind, e_loss, e_iou)
    assert e_grad <= 1e-4 * scale, (g, kind, e_grad, scale)


def test_the_new_losses_are_registered_and_refuse_cpu_tensors():
    import fcaf3d_amd as fa
    g = fa.build_loss(dict(type='GIoU3DLoss'))
    dl = fa.build_loss(dict(type='DIoU3DLoss', with_yaw=False))
    assert type(g) is fa.GIoU3DLoss and g.with_yaw and g.reduction == 'mean' and g.loss_weight == 1.0
    assert type(dl) is fa.DIoU3DLoss and not dl.with_yaw
    d = fixture()
    p7, t7 = torch.from_numpy(d['ro_pred']), torch.from_numpy(d['ro_target'])
    for fn in (lambda: g(p7, t7), lambda: dl(p7[:, :6], t7), lambda: fa.giou_3d(p7, t7), lambda: fa.diou_3d(p7[:, :6], t7[:, :6])):
        with pytest.raises(RuntimeError, match='GPU only'):
            fn()
    with pytest.raises(AssertionError, match='with_yaw'):                  # the box width must match with_yaw
        dl(p7, t7)
    with pytest.raises(AssertionError, match='with_yaw'):
        g(p7[:, :6], t7)
    assert float(g(p7[:0], t7[:0])) == 0.0                                  # an empty prediction needs no kernel


def test_the_kinds_are_header_enums_and_the_argument_checks_need_no_gpu():
    from fcaf3d_amd import _lib as L
    E = L.header_enums()
    assert E['FC_EIOU_GIOU'] == 0 and E['FC_EIOU_DIOU'] == 1
    fn = L.lib().fc_eiou3d_fwd_bwd
    p = 0x1000                       # never dereferenced: every call below returns before a launch

    def call(n=0, box_dim=7, kind=0, stride=7, w=p):
        return fn(p, p, stride, w, n, box_dim, kind, p, p, p, None)
    assert call() == 0 and call(box_dim=6, stride=6) == 0 and call(box_dim=6, stride=7, kind=1) == 0 and call(w=None) == 0
    assert call(n=-1) == -1
    assert call(box_dim=5) == -1 and call(box_dim=8, stride=8) == -1
    assert call(kind=2) == -1 and call(kind=-1) == -1
    assert call(box_dim=6, stride=5) == -1 and call(n=10, box_dim=6, stride=5) == -1 and call(n=10, box_dim=7, stride=6) == -1
    assert call(n=10, kind=3) == -1


# ---- the kernel's text on the host (tools/eiou_host_emu.cpp) -------------------------------------------------------------------------

@pytest.fixture(scope='module')
def emulator(tmp_path_factory):
    """csrc_post/eiou.hip from its EIOU_* constants to the end of its anonymous namespace, compiled for the host with AddressSanitizer
    and UBSan: the emulator restates nothing of it"""
    from fcaf3d_amd import build as B
    tmp = tmp_path_factory.mktemp('eiou_emu')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(B.CSRC_POST, 'eiou.hip')).read()
    end = '}  // namespace'
    body = src[src.index('#define EIOU_THREADS'):src.index(end) + len(end)]
    assert '#include' not in body and '#define EIOU_ROWS' in body and 'k_eiou3d' in body, 'eiou.hip was reordered'
    (tmp / 'kernels.inc').write_text(body)
    cxx = os.path.join(os.path.dirname(os.path.dirname(B.HIPCC)), 'llvm', 'bin', 'clang++')
    cxx = cxx if os.path.exists(cxx) else shutil.which('clang++')
    exe = str(tmp / 'eiou_host_emu')
    subprocess.check_call([cxx, '-std=c++20', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-pthread', f'-I{tmp}', f"-I{os.path.join(root, 'include')}", os.path.join(root, 'tools', 'eiou_host_emu.cpp'),
                           '-o', exe])
    return exe, tmp


def emulate(emulator, pred, target, weight, kind):
    exe, tmp = emulator
    n, bd = pred.shape
    with open(tmp / 'in.bin', 'wb') as f:
        np.array([n, bd, target.shape[1], KINDS.index(kind), weight is not None], np.int64).tofile(f)
        np.ascontiguousarray(pred, np.float32).tofile(f)
        np.ascontiguousarray(target, np.float32).tofile(f)
        if weight is not None:
            np.ascontiguousarray(weight, np.float32).tofile(f)
    r = subprocess.run([exe, str(tmp / 'in.bin'), str(tmp / 'out.bin')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    raw = np.fromfile(tmp / 'out.bin', np.float32)
    assert len(raw) == n * (2 + bd)
    return raw[:n], raw[n:2 * n], raw[2 * n:].reshape(n, bd)


@pytest.mark.parametrize('kind', KINDS)
def test_kernel_text_on_the_host_meets_the_float64_fixture(emulator, kind):
    """every fixture group through the kernel's own text, no sanitizer report; the aligned group also with the 7-column targets the head
    hands to a yaw-less loss"""
    d = fixture()
    for g in GROUPS:
        loss, iou, dpred = emulate(emulator, d[f'{g}_pred'], d[f'{g}_target'], d[f'{g}_w'], kind)
        assert (dpred[d[f'{g}_w'] == 0] == 0).all()
        check_against_fixture(d, g, kind, loss, iou, d[f'{g}_w'][:, None] * dpred, 'host')
    t7 = np.concatenate([d['al_target'], np.full((len(d['al_target']), 1), np.nan, np.float32)], 1)
    again = emulate(emulator, d['al_pred'], t7, d['al_w'], kind)
    for a, b in zip(again, emulate(emulator, d['al_pred'], d['al_target'], d['al_w'], kind)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('kind', KINDS)
def test_kernel_text_on_the_host_sizes_and_weight_patterns(emulator, kind):
    """n = 1, 63, 64, 65, 257 and 2100 rows cut from `ro` (and from `al`) under three weight patterns: rows without weight are exactly zero
    although their boxes hold NaN / inf, active rows equal the dense call's rows bit for bit, every output word is written"""
    d = fixture()
    for g in ('ro', 'al'):
        reps = -(-max(SIZES) // len(d[f'{g}_pred']))
        pred, target = np.tile(d[f'{g}_pred'], (reps, 1)), np.tile(d[f'{g}_target'], (reps, 1))
        dense = emulate(emulator, pred[:max(SIZES)], target[:max(SIZES)], None, kind)
        assert all(np.isfinite(x).all() for x in dense)
        for n in SIZES:
            for pattern in PATTERNS:
                w = pattern_weight(pattern, n)
                p, t = pred[:n].copy(), target[:n].copy()
                p[w == 0] = np.nan
                t[w == 0] = np.inf
                out = emulate(emulator, p, t, w, kind)
                for got, want in zip(out, dense):
                    assert (got[w == 0] == 0).all(), (g, n, pattern)
                    assert np.array_equal(got[w > 0], want[:n][w > 0]), (g, n, pattern)
