"""CPU: gradient accumulation, mmcv's GradientCumulativeOptimizerHook — the rule's table and the config checks,
the text of the kernels of csrc_post/optim_accum.hip on the host (tools/accum_host_emu.cpp, a stand-alone program under
AddressSanitizer and UBSan) against numpy restatements bit for bit, the entry points' refusals, and runner.fit with the hook on the
CPU: the stepping iterations, the log's grad_norm, the open group in the checkpoint, resume, the weight average's cadence."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from fcaf3d_amd import runner as R

from tests.test_ema_cpu import bits, draw, ema_numpy, sd_of, stub
from tests.test_fit_cpu import Stub, make_cfg

f32 = np.float32
HOOK = 'GradientCumulativeOptimizerHook'
CLIP = dict(max_norm=10, norm_type=2)


# ---- 1. the rule and the config -------------------------------------------------------------------------------------------------------------
# (k, T): (the iterations after which the optimizer steps, every iteration's factor)
RULE = {
    (1, 6): ([0, 1, 2, 3, 4, 5], [1, 1, 1, 1, 1, 1]),
    (1, 7): ([0, 1, 2, 3, 4, 5, 6], [1, 1, 1, 1, 1, 1, 1]),
    (1, 8): ([0, 1, 2, 3, 4, 5, 6, 7], [1, 1, 1, 1, 1, 1, 1, 1]),
    (2, 6): ([1, 3, 5], [2, 2, 2, 2, 2, 2]),
    (2, 7): ([1, 3, 5, 6], [2, 2, 2, 2, 2, 2, 1]),
    (2, 8): ([1, 3, 5, 7], [2, 2, 2, 2, 2, 2, 2, 2]),
    (3, 6): ([2, 5], [3, 3, 3, 3, 3, 3]),
    (3, 7): ([2, 5, 6], [3, 3, 3, 3, 3, 3, 1]),
    (3, 8): ([2, 5, 7], [3, 3, 3, 3, 3, 3, 2, 2]),
}


@pytest.mark.parametrize('k,T', sorted(RULE))
def test_stepping_iterations_and_factors_follow_the_table(k, T):
    steps, factors = RULE[(k, T)]
    assert [it for it in range(T) if R.accum_steps(it, k, T)] == steps
    assert [R.accum_factor(it, k, T) for it in range(T)] == factors
    # without a total: k throughout, every k-th iteration steps
    assert [R.accum_factor(it, k) for it in range(T)] == [k] * T
    assert [it for it in range(T) if R.accum_steps(it, k)] == [it for it in range(T) if (it + 1) % k == 0]
    # a group's factors are its length, and the stepped sum of g / f over a group weighs its iterations to 1
    start = 0
    for s in steps:
        assert factors[start:s + 1] == [s + 1 - start] * (s + 1 - start)
        start = s + 1
    assert start == T


def test_optimizer_config_is_checked():
    assert R.cumulative_iters_of(None) == 1 and R.cumulative_iters_of({}) == 1 and R.cumulative_iters_of(dict(grad_clip=CLIP)) == 1
    assert R.cumulative_iters_of(dict(type='OptimizerHook', grad_clip=CLIP)) == 1
    assert R.cumulative_iters_of(dict(type=HOOK, grad_clip=CLIP)) == 1 and R.cumulative_iters_of(dict(type=HOOK, cumulative_iters=1)) == 1
    assert R.cumulative_iters_of(dict(type=HOOK, cumulative_iters=4, grad_clip=CLIP)) == 4
    with pytest.raises(KeyError, match='Fp16OptimizerHook'):
        R.cumulative_iters_of(dict(type='Fp16OptimizerHook', grad_clip=CLIP))
    with pytest.raises(KeyError, match='detect_anomalous_params'):
        R.cumulative_iters_of(dict(type=HOOK, cumulative_iters=2, detect_anomalous_params=True))
    with pytest.raises(KeyError, match='loss_scale'):
        R.cumulative_iters_of(dict(grad_clip=CLIP, loss_scale=512.0))
    for bad in (0, -1, 1.5, 2.0, True, '2', None):
        with pytest.raises(ValueError, match='cumulative_iters'):
            R.cumulative_iters_of(dict(type=HOOK, cumulative_iters=bad))
    with pytest.raises(KeyError, match='cumulative_iters'):
        R.cumulative_iters_of(dict(type='OptimizerHook', cumulative_iters=2))
    # TrainStep parses it; the default allocates nothing and divides by nothing
    tr = R.TrainStep(Stub(), dict(type='AdamW', lr=1e-3), dict(type=HOOK, cumulative_iters=3, grad_clip=CLIP), max_iters=7)
    assert (tr.cumulative_iters, tr.max_iters, tr.acc_iters, tr.max_norm) == (3, 7, 0, 10)
    plain = R.TrainStep(Stub(), dict(type='AdamW', lr=1e-3), dict(grad_clip=CLIP))
    assert (plain.cumulative_iters, plain.max_iters, plain.acc_iters) == (1, None, 0) and 'grad_accum' not in plain.state_dict()
    with pytest.raises(KeyError, match='Fp16OptimizerHook'):
        R.TrainStep(Stub(), dict(type='AdamW', lr=1e-3), dict(type='Fp16OptimizerHook'))


# ---- 2. the kernels' text on the host -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def emulator(tmp_path_factory):
    """csrc_post/optim_accum.hip from its ACC_THREADS constant to the end of its anonymous namespace, compiled for the host with
    AddressSanitizer and UBSan into a stand-alone program: the emulator restates nothing of the kernels"""
    from fcaf3d_amd import build as B
    tmp = tmp_path_factory.mktemp('accum_emu')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(B.CSRC_POST, 'optim_accum.hip')).read()
    end = '}  // namespace'
    body = src[src.index('#define ACC_THREADS'):src.index(end) + len(end)]
    assert '#include' not in body and 'extern "C"' not in body
    assert all(k in body for k in ('k_grad_accum', 'k_grad_accum_sum', 'k_accum_sqsum_partial', 'k_accum_sqsum_final'))
    for h in ('accum_elem.h', 'ema_elem.h'):
        assert 'fp contract(off)' in open(os.path.join(B.CSRC_POST, h)).read()
    (tmp / 'accum_kernels.inc').write_text(body)
    cxx = os.path.join(os.path.dirname(os.path.dirname(B.HIPCC)), 'llvm', 'bin', 'clang++')
    cxx = cxx if os.path.exists(cxx) else shutil.which('clang++')
    exe = str(tmp / 'accum_host_emu')
    subprocess.check_call([cxx, '-std=c++20', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-pthread', f'-I{tmp}', os.path.join(root, 'tools', 'accum_host_emu.cpp'), '-o', exe])
    return exe, tmp


SIZES = (64, 192, 1024, 1088, 4160, 4096, 4100)      # tests/test_ema_cpu.py's, and the edge of the norm pass's block count cdiv(n / 4, 1024)
SCALES = (0.5, 1.0 / 3.0)


def emulate(emulator, mode, arrays, scale, first=0, mu=None, max_norm=10.0):
    """mode 0: (acc, g[, ema, p]) -> acc, g[, ema]; mode 1: (g, acc) -> g, acc, out2; mode 2: (g, acc) -> g, acc"""
    exe, tmp = emulator
    n = len(arrays[0])
    has_ema = mode == 0 and len(arrays) == 4
    with open(tmp / 'in.bin', 'wb') as f:
        np.array([n, first, int(has_ema), mode], np.int64).tofile(f)
        np.array([f32(scale), f32(mu if has_ema else 0.0), f32(1.0 - mu if has_ema else 0.0), max_norm], f32).tofile(f)
        for a in arrays:
            np.ascontiguousarray(a, f32).tofile(f)
    r = subprocess.run([exe, str(tmp / 'in.bin'), str(tmp / 'out.bin')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = np.fromfile(tmp / 'out.bin', f32)
    k = (3 if has_ema else 2) if mode != 1 else 2
    assert len(out) == k * n + (2 if mode == 1 else 0)
    return [out[j * n:(j + 1) * n] for j in range(k)] + ([out[k * n:]] if mode == 1 else [])


def accum_numpy(acc, g, scale, first):
    """the rule: acc <- fl32(g * s), or fl32( acc + fl32(g * s) ), s = fl32(scale)"""
    scaled = g.astype(f32) * f32(scale)
    out = scaled if first else acc.astype(f32) + scaled
    assert scaled.dtype == out.dtype == np.float32
    return out


def norm_numpy(G, max_norm):
    """fc_grad_norm's two floats in its own order (csrc_post/sqsum_order.h): blocks = min(cdiv(n4, 1024), 1024) of 256 threads;
    thread (b, t) walks float4 j = b * 256 + t + sweep * 4 * stride + u * stride (u = 0 .. 3, stride = blocks * 256), squares and adds
    each vector's four floats in fp32 as ((x0^2 + x1^2) + x2^2) + x3^2 and sums those as doubles; the butterfly over the 64 lanes
    (xor 32, 16, ... 1), the four waves as (0 + 1) + (2 + 3); then one block of 1 024 threads: thread t takes the partial sums
    t, t + 1024, ..., the same butterfly, the 16 waves in sequence, fl32(sqrt), and the clip coefficient in fp32"""
    n4 = len(G) // 4
    nb = min(max(-(-max(n4, 1) // 1024), 1), 1024)
    stride = nb * 256
    x = np.ascontiguousarray(G, f32).reshape(n4, 4)
    sq = x * x
    s = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]
    assert s.dtype == np.float32
    i0 = np.arange(nb * 256, dtype=np.int64)
    acc = np.zeros(nb * 256, np.float64)
    base = 0
    while base < n4:
        for u in range(4):
            j = i0 + base + u * stride
            m = j < n4
            acc[m] = acc[m] + s[j[m]].astype(np.float64)
        base += 4 * stride
    lanes = np.arange(64)

    def butterfly(a):                      # a[..., 64] -> lane 0's sum
        for off in (32, 16, 8, 4, 2, 1):
            a = a + a[..., lanes ^ off]
        return a[..., 0]
    w = butterfly(acc.reshape(nb, 4, 64))
    part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    th = np.zeros(1024, np.float64)
    for i in range(nb):
        th[i % 1024] = th[i % 1024] + part[i]
    red = butterfly(th.reshape(16, 64))
    t = np.float64(0.0)
    for v in red:
        t = t + v
    norm = f32(np.sqrt(t))
    c = f32(1.0)
    if max_norm > 0:
        c = min(f32(max_norm) / (norm + f32(1e-6)), f32(1.0))
    return np.array([norm, c], f32)


def lanes_of(n, seed):
    """acc, g, ema, p of tests/test_ema_cpu.py's draw (magnitudes 1e-3 .. 1e3, nothing subnormal), with one -0.0 lane in g and acc"""
    p, g, _, _, e = draw(n, seed)
    acc = draw(n, seed + 1)[1]
    g[5], acc[5] = f32(-0.0), f32(-0.0)
    return acc, g, e, p


@pytest.mark.parametrize('n', SIZES)
def test_accumulation_kernel_text_on_the_host_equals_numpy(emulator, n):
    acc, g, e, p = lanes_of(n, 31 + n)
    g[n - 3] = np.float32('nan')                     # one NaN lane: passes through, touches no neighbour
    for scale in SCALES:
        for first in (0, 1):
            want = accum_numpy(acc, g, scale, first)
            a1, g1 = emulate(emulator, 0, (acc, g), scale, first)
            assert np.array_equal(bits(a1), bits(want)), (n, scale, first, int((bits(a1) != bits(want)).sum()))
            assert np.array_equal(bits(g1), bits(g))                                         # g is read only
            assert np.isnan(a1[n - 3]) and np.isfinite(np.delete(a1, n - 3)).all()
            assert bits(a1)[5] == 0x80000000                                                 # -0 * s = -0, and -0 + -0 = -0
            if first:
                assert np.array_equal(bits(a1), bits(emulate(emulator, 0, (np.full(n, np.nan, f32), g), scale, 1)[0]))      # acc is not read
            for mu in (0.5, 0.0002):
                a2, g2, e2 = emulate(emulator, 0, (acc, g, e, p), scale, first, mu=mu)
                assert np.array_equal(bits(a2), bits(want)) and np.array_equal(bits(g2), bits(g))
                assert np.array_equal(bits(e2), bits(ema_numpy(e, p, mu))), (n, scale, first, mu)
    ok = np.delete(accum_numpy(acc, g, 1.0 / 3.0, 0), n - 3)
    assert (np.abs(ok[ok != 0]) >= np.finfo(f32).tiny).all()                                 # no subnormal in sight


@pytest.mark.parametrize('n', SIZES)
def test_stepping_kernel_text_on_the_host_equals_numpy_in_the_norms_order(emulator, n):
    acc, g, _, _ = lanes_of(n, 57 + n)
    for scale in SCALES:
        G = accum_numpy(acc, g, scale, 0)
        for max_norm in (10.0, 0.0):
            g1, a1, out2 = emulate(emulator, 1, (g, acc), scale, max_norm=max_norm)
            assert np.array_equal(bits(g1), bits(G)), (n, scale, int((bits(g1) != bits(G)).sum()))
            assert np.array_equal(bits(a1), bits(acc))                                       # acc is read only
            want = norm_numpy(G, max_norm)
            assert np.array_equal(bits(out2), bits(want)), (n, scale, max_norm, out2, want)
            assert out2[0] > 10.0 and (out2[1] < 1.0 if max_norm else out2[1] == 1.0)
        g2, a2 = emulate(emulator, 2, (g, acc), scale)                                        # no clip configured: the sum alone
        assert np.array_equal(bits(g2), bits(G)) and np.array_equal(bits(a2), bits(acc))
    # the order matters to the last bit: the plain float64 sum rounds differently for some of these sizes, never by more than 1 ulp
    plain = f32(np.sqrt((G.astype(np.float64) ** 2).sum()))
    assert abs(int(bits(norm_numpy(G, 10.0))[0]) - int(bits(plain)[0])) <= 1


def test_stepping_kernel_text_passes_a_nan_lane_through(emulator):
    acc, g, _, _ = lanes_of(192, 7)
    acc[100] = np.float32('nan')
    g1, _, out2 = emulate(emulator, 1, (g, acc), 0.5)
    G = accum_numpy(acc, g, 0.5, 0)
    assert np.array_equal(bits(g1), bits(G)) and np.isnan(g1[100]) and np.isfinite(np.delete(g1, 100)).all()
    assert np.isnan(out2[0])
    acc[:], g[:] = 0, 0                               # padding: zero in, zero out
    g1, _, out2 = emulate(emulator, 1, (g, acc), 1.0 / 3.0)
    assert not g1.any() and out2[0] == 0 and out2[1] == 1.0
    assert not emulate(emulator, 0, (acc, g), 1.0 / 3.0, 0)[0].any()


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """the argument checks return before anything is launched: they run here, on fake addresses that are never dereferenced"""
    l = L.lib()
    P = [ctypes.c_void_p(0x100000 * (k + 1)) for k in range(5)]
    inf, nan = float('inf'), float('nan')

    def accum(acc=P[0], g=P[1], n=64, scale=0.5, first=0, ema=None, p=None, mu=0.0, keep=0.0):
        return l.fc_grad_accum(acc, g, n, scale, first, ema, p, mu, keep, None)
    assert accum(n=66) == -1 and accum(n=-4) == -1
    for bad in (0.0, -0.5, nan, inf, -inf):
        assert accum(scale=bad) == -1
    for bad in (-0.1, 1.5, nan, inf, -inf):
        assert accum(mu=bad) == -1 and accum(keep=bad) == -1
        assert accum(ema=P[2], p=P[3], mu=bad, keep=0.5) == -1 and accum(ema=P[2], p=P[3], mu=0.5, keep=bad) == -1
    assert accum(acc=P[0], g=P[0]) == -1                                                    # acc is g
    assert accum(g=ctypes.c_void_p(0x100000 + 16)) == -1 and accum(acc=ctypes.c_void_p(0x200000 + 252)) == -1      # overlap
    assert accum(ema=P[2], p=None, mu=0.5, keep=0.5) == -1                                   # an average without the parameters
    assert accum(ema=P[2], p=None, n=0) == -1
    assert accum(ema=P[0], p=P[3]) == -1 and accum(ema=P[1], p=P[3]) == -1 and accum(ema=P[3], p=P[3]) == -1
    assert accum(acc=None) == -1 and accum(g=None) == -1
    assert accum(n=0) == 0 and accum(acc=None, g=None, n=0) == 0                             # nothing to launch
    assert accum(n=0, scale=0.0) == -1 and accum(n=0, mu=2.0) == -1

    def norm(g=P[0], acc=P[1], n=64, scale=0.5, max_norm=10.0, out2=P[2], ws=P[3], ws_bytes=8192):
        return l.fc_grad_accum_norm(g, acc, n, scale, max_norm, out2, ws, ws_bytes, None)
    assert l.fc_grad_accum_norm_ws_bytes(64) == l.fc_grad_norm_ws_bytes(64) == 8192
    assert norm(n=66) == -1 and norm(n=-4) == -1
    for bad in (0.0, -0.5, nan, inf, -inf):
        assert norm(scale=bad) == -1 and norm(scale=bad, out2=None) == -1
    assert norm(g=P[0], acc=P[0]) == -1 and norm(acc=ctypes.c_void_p(0x100000 + 16)) == -1 and norm(g=ctypes.c_void_p(0x200000 + 252)) == -1
    assert norm(g=None) == -1 and norm(acc=None) == -1
    assert norm(ws_bytes=8191) == -2 and norm(ws=None) == -2                                 # (sum only needs no workspace, but would launch)
    assert norm(n=0) == 0 and norm(n=0, g=None, acc=None, out2=None, ws=None, ws_bytes=0) == 0
    assert norm(n=0, scale=nan) == -1


# ---- 3. fit on the CPU ----------------------------------------------------------------------------------------------------------------------
def cfg_of(tmp_path, k, max_epochs, **over):
    oc = dict(type=HOOK, cumulative_iters=k, grad_clip=dict(CLIP)) if k is not None else dict(grad_clip=dict(CLIP))
    return make_cfg(tmp_path / 'data', max_epochs=max_epochs, checkpoint_config=dict(interval=1, max_keep_ckpts=4), optimizer_config=oc, **over)


def replay(batches, k, T, ipe=3):
    """the hand-written loop: torch.optim.AdamW, (loss / f).backward(), clip_grad_norm_, a step on the rule's iterations
    -> the model, the clip norms by iteration"""
    model = stub()
    opt = torch.optim.AdamW(model.parameters(), lr=0.001, weight_decay=0.0001)
    norms = {}
    for it, batch in enumerate(batches):
        opt.param_groups[0]['lr'] = 0.001 * 0.1 ** (1 if it // ipe >= 1 else 0)              # lr_config step=[1], gamma 0.1
        f = k if it < T - T % k else T % k
        loss = R.parse_losses(model(return_loss=True, **batch))
        (loss / f).backward()
        if (it + 1) % k == 0 or it == T - 1:
            norms[it] = float(torch.nn.utils.clip_grad_norm_(model.parameters(), 10, norm_type=2))
            opt.step()
            opt.zero_grad()
    return model, norms


@pytest.fixture(scope='module')
def straight(tmp_path_factory):
    """k = 2 over 4 epochs of 3 iterations (T = 12: a group is open at the epoch-1 and epoch-3 boundaries)"""
    from fcaf3d_amd import fit
    tmp = tmp_path_factory.mktemp('accum_fit')
    model, batches = stub(), []
    rec = fit(model, cfg_of(tmp, 2, 4), str(tmp / 'straight'), seed=3, device='cpu', on_batch=lambda e, it, b: batches.append(b))
    return dict(tmp=tmp, model=model, batches=batches, rec=rec, work=tmp / 'straight')


def test_fit_equals_the_hand_written_loop_and_logs_the_norm_of_the_steps(straight):
    assert len(straight['batches']) == 12
    twin, norms = replay(straight['batches'], 2, 12)
    assert sorted(norms) == [1, 3, 5, 7, 9, 11]
    assert torch.equal(straight['model'].w.detach(), twin.w.detach())
    plain, _ = replay(straight['batches'], 1, 12)
    assert not torch.equal(plain.w.detach(), twin.w.detach())
    # log interval 2: a line over iterations (3 e, 3 e + 1) and one over 3 e + 2; grad_norm only where a step fell inside
    rec = straight['rec']
    assert [(r['epoch'], r['iter']) for r in rec] == [(e, i) for e in range(1, 5) for i in (2, 3)] and all(r['mode'] == 'train' for r in rec)
    stepped = [[1], [], [3], [5], [7], [], [9], [11]]
    for r, its in zip(rec, stepped):
        assert ('grad_norm' in r) == bool(its), r
        if its:
            assert abs(r['grad_norm'] - np.mean([norms[i] for i in its])) <= 1e-6 * r['grad_norm']
        assert {'loss', 'loss_a', 'loss_b', 'aux', 'lr', 'time', 'data_time'} <= set(r)
    # the losses are logged unscaled: a line's loss is the mean of its iterations' full losses
    m = stub()                                       # iterations 0 and 1 both run on the initial weights: no step falls before either pass
    full = [float(R.parse_losses(m(return_loss=True, **b)).detach()) for b in straight['batches'][:2]]
    assert abs(rec[0]['loss'] - (full[0] + full[1]) / 2) <= 1e-5 * abs(rec[0]['loss'])
    ck = torch.load(straight['work'] / 'epoch_1.pth', map_location='cpu', weights_only=False)
    assert ck['grad_accum']['iters'] == 1 and len(ck['grad_accum']['grads']) == 1 and ck['meta']['iter'] == 3
    assert 'grad_accum' not in torch.load(straight['work'] / 'epoch_2.pth', map_location='cpu', weights_only=False)


def test_fit_resume_restores_the_open_group(straight):
    from fcaf3d_amd import fit
    tmp = straight['tmp']
    work = tmp / 'resumed'
    fit(stub(), cfg_of(tmp, 2, 2), str(work), seed=3, device='cpu')                           # T = 6
    ck1 = torch.load(work / 'epoch_1.pth', map_location='cpu', weights_only=False)
    assert ck1['grad_accum']['iters'] == 1 and ck1['grad_accum']['grads'][0].shape == (8,)
    assert 'grad_accum' not in torch.load(work / 'epoch_2.pth', map_location='cpu', weights_only=False)
    model = Stub()
    with torch.no_grad():
        model.w.zero_()
    rec = fit(model, cfg_of(tmp, 2, 4), str(work), seed=3, device='cpu', resume_from=str(work / 'latest.pth'))      # T = 12
    assert torch.equal(model.w.detach(), straight['model'].w.detach()) and all(r['mode'] == 'train' for r in rec)
    a, b = sd_of(work / 'epoch_4.pth'), sd_of(straight['work'] / 'epoch_4.pth')
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # from the epoch-1 file, where a group is open: the partial sum is put back, the straight run's weights again
    again = Stub()
    fit(again, cfg_of(tmp, 2, 4), str(tmp / 'resumed_open'), seed=3, device='cpu', resume_from=str(work / 'epoch_1.pth'))
    assert torch.equal(again.w.detach(), straight['model'].w.detach())
    # the same file with the key deleted: mmcv's behaviour, said in the log; the weights differ
    del ck1['grad_accum']
    torch.save(ck1, tmp / 'no_key.pth')
    lost = Stub()
    rec = fit(lost, cfg_of(tmp, 2, 4), str(tmp / 'resumed_lost'), seed=3, device='cpu', resume_from=str(tmp / 'no_key.pth'))
    assert rec[0]['mode'] == 'accum' and rec[0]['resume_from'] == str(tmp / 'no_key.pth') and sum(r['mode'] == 'accum' for r in rec) == 1
    assert not torch.equal(lost.w.detach(), straight['model'].w.detach())
    # a file written at a group's edge needs no note, with or without the key
    rec = fit(Stub(), cfg_of(tmp, 2, 4), str(tmp / 'resumed_edge'), seed=3, device='cpu', resume_from=str(work / 'epoch_2.pth'))
    assert all(r['mode'] == 'train' for r in rec)


def test_fit_steps_the_last_iteration_alone_with_factor_one(tmp_path):
    from fcaf3d_amd import fit
    model, batches = stub(), []
    rec = fit(model, cfg_of(tmp_path, 2, 1), str(tmp_path / 'w'), seed=3, device='cpu', on_batch=lambda e, it, b: batches.append(b))      # T = 3
    twin, norms = replay(batches, 2, 3)
    assert sorted(norms) == [1, 2] and torch.equal(model.w.detach(), twin.w.detach())
    assert ['grad_norm' in r for r in rec] == [True, True]
    assert 'grad_accum' not in torch.load(tmp_path / 'w' / 'epoch_1.pth', map_location='cpu', weights_only=False)
    # k = 1 under the hook's name and the plain config are one path
    a, b = stub(), stub()
    fit(a, cfg_of(tmp_path, 1, 1), str(tmp_path / 'k1'), seed=3, device='cpu')
    fit(b, cfg_of(tmp_path, None, 1), str(tmp_path / 'plain'), seed=3, device='cpu')
    assert torch.equal(a.w.detach(), b.w.detach()) and torch.equal(a.w.detach(), replay(batches, 1, 3)[0].w.detach())


def micro(tr, model, s):
    """one micro-iteration of the per-tensor path, by hand: open, the loss over the factor, close"""
    tr.set_iter(s)
    tr.open()
    ((model.w ** 2).sum() / tr.factor()).backward()
    tr.close(None)


def test_the_average_moves_towards_the_unchanged_weights_when_no_step_falls(tmp_path):
    model = stub()
    tr = R.TrainStep(model, dict(type='AdamW', lr=0.01), dict(type=HOOK, cumulative_iters=2, grad_clip=dict(CLIP)),
                     ema=dict(type='EMAHook', momentum=0.5, interval=1, warm_up=0))
    e = model.w.detach().numpy().copy()
    for s in range(4):
        w_before = model.w.detach().clone()
        micro(tr, model, s)
        got = tr.ema.state_dict()['ema_w']
        if s % 2 == 0:
            assert torch.equal(model.w.detach(), w_before) and tr.last_grad_norm is None and tr.acc_iters == 1
            assert model.w.grad is not None                                                  # the sum waits in p.grad
        else:
            assert not torch.equal(model.w.detach(), w_before) and tr.last_grad_norm is not None and tr.acc_iters == 0
        e = ema_numpy(e, model.w.detach().numpy(), 0.5)
        assert np.array_equal(bits(got.numpy()), bits(e)), s
    assert tr.it == 4 and len(tr.optimizer.state_dict()['state']) == 1 and int(tr.optimizer.state_dict()['state'][0]['step']) == 2


def test_flush_steps_an_open_group_and_the_state_carries_it():
    model = stub()
    tr = R.TrainStep(model, dict(type='AdamW', lr=0.01, weight_decay=0.0), dict(type=HOOK, cumulative_iters=3, grad_clip=dict(CLIP)))
    assert tr.flush() is False
    w0 = model.w.detach().clone()
    micro(tr, model, 0)
    assert tr.factor() == 3 and tr.acc_iters == 1 and torch.equal(model.w.detach(), w0)
    sd = tr.state_dict()
    t = w0.clone().requires_grad_()
    ((t ** 2).sum() / 3).backward()
    assert sd['grad_accum']['iters'] == 1 and torch.equal(sd['grad_accum']['grads'][0], t.grad)
    # a second TrainStep takes the open group over
    other = stub()
    tr2 = R.TrainStep(other, dict(type='AdamW', lr=0.01, weight_decay=0.0), dict(type=HOOK, cumulative_iters=3, grad_clip=dict(CLIP)))
    tr2.load_state_dict(sd)
    assert tr2.acc_iters == 1 and torch.equal(other.w.grad, sd['grad_accum']['grads'][0])
    for t, m in ((tr, model), (tr2, other)):
        assert t.flush() is True and t.acc_iters == 0 and 'grad_accum' not in t.state_dict()
        assert not torch.equal(m.w.detach(), w0)
    assert torch.equal(model.w.detach(), other.w.detach())
    twin = stub()
    opt = torch.optim.AdamW(twin.parameters(), lr=0.01, weight_decay=0.0)
    ((twin.w ** 2).sum() / 3).backward()
    torch.nn.utils.clip_grad_norm_(twin.parameters(), 10, norm_type=2)
    opt.step()
    assert torch.equal(model.w.detach(), twin.w.detach())
    # a plain TrainStep ignores a group it is handed
    plain = R.TrainStep(stub(), dict(type='AdamW', lr=0.01), dict(grad_clip=dict(CLIP)))
    plain.load_state_dict(sd)
    assert plain.acc_iters == 0
