"""CPU: the weight average of mmcv's EMAHook — the schedule and the config checks of runner.WeightEma, the text
of the kernels of csrc_post/optim_ema.hip on the host (tools/ema_host_emu.cpp, a stand-alone program under AddressSanitizer and
UBSan) against numpy restatements bit for bit, and runner.fit with the hook on the CPU: swap order, checkpoint entries, resume,
load_from."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from fcaf3d_amd import runner as R

from tests.test_finetune_cpu import adamw_groups_numpy
from tests.test_fit_cpu import Stub, make_cfg

f32 = np.float32


def ema_numpy(e, p_new, mu):
    """the rule: e <- fl32( fl32(e * fl32(1 - mu)) + fl32(fl32(mu) * p_new) ), 1 - mu formed in double"""
    keep, m = f32(1.0 - mu), f32(mu)
    kept = e.astype(f32) * keep
    added = m * p_new.astype(f32)
    out = kept + added
    assert kept.dtype == added.dtype == out.dtype == np.float32
    return out


# ---- 1. the schedule and the config ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('momentum,interval,warm_up', [(0.0002, 1, 100), (0.5, 1, 0), (0.5, 2, 4), (0.01, 3, 100)])
def test_momentum_follows_mmcvs_schedule(momentum, interval, warm_up):
    h = R.WeightEma(momentum=momentum, interval=interval, warm_up=warm_up)
    M = momentum ** interval
    assert h.momentum == M
    for s in range(13):
        if s % interval:
            assert h.momentum_at(s) is None and h.coeffs(s) is None
            continue
        bound = (1 + s) / (warm_up + s) if warm_up + s else float('inf')      # mmcv divides by zero there; no bound is the limit
        mu = min(M, bound)
        assert h.momentum_at(s) == mu
        assert h.coeffs(s) == (float(f32(mu)), float(f32(1.0 - mu)))
    if warm_up == 100 and interval == 1:
        assert h.momentum_at(0) == 0.0002 and h.momentum_at(10 ** 6) == 0.0002          # (1 + s) / (100 + s) >= 0.01 > M throughout
    if (momentum, interval, warm_up) == (0.5, 2, 4):
        assert [h.momentum_at(s) for s in (0, 2, 4)] == [0.25, 0.25, 0.25]             # (1 + 0) / 4 = M exactly, then above it
    if (momentum, interval, warm_up) == (0.01, 3, 100):
        assert h.momentum == 0.01 ** 3 and h.momentum_at(3) == 0.01 ** 3


def test_hook_config_is_checked():
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match='momentum'):
            R.WeightEma(momentum=bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='interval'):
            R.WeightEma(interval=bad)
    with pytest.raises(KeyError, match='ExpMomentumEMAHook'):
        R.ema_hook_of([dict(type='ExpMomentumEMAHook', momentum=0.1)])
    with pytest.raises(KeyError, match='SyncBuffersHook'):
        R.ema_hook_of([dict(type='EMAHook'), dict(type='SyncBuffersHook')])
    with pytest.raises(KeyError, match='skip_buffers'):
        R.ema_hook_of([dict(type='EMAHook', skip_buffers=True)])
    with pytest.raises(KeyError, match='total_iters'):
        R.WeightEma.from_config(dict(type='EMAHook', total_iters=5))
    assert R.ema_hook_of(None) is None and R.ema_hook_of([]) is None
    h = R.WeightEma.from_config(dict(type='EMAHook', momentum=0.1, interval=2, warm_up=7, resume_from='x.pth'))
    assert (h.momentum, h.interval, h.warm_up, h.resume_from) == (0.1 ** 2, 2, 7, 'x.pth')
    d = R.WeightEma.from_config(dict(type='EMAHook'))
    assert (d.momentum, d.interval, d.warm_up, d.resume_from) == (0.0002, 1, 100, None)
    assert R.WeightEma.name_of('backbone.layer1.0.conv1.kernel') == 'ema_backbone_layer1_0_conv1_kernel'
    import fcaf3d_amd as fa
    assert fa.WeightEma is R.WeightEma and fa.TrainStep is R.TrainStep


class _Clash(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(2, 2)
        self.a_weight = torch.nn.Parameter(torch.zeros(1))


def test_two_parameters_under_one_buffer_name_raise():
    with pytest.raises(ValueError, match='ema_a_weight'):
        R.TrainStep(_Clash(), dict(type='AdamW', lr=1e-3), ema=dict(type='EMAHook'))


# ---- 2. the kernels' text on the host -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def emulator(tmp_path_factory):
    """csrc_post/optim_ema.hip from its EMA_* constants to the end of its anonymous namespace, compiled for the host with
    AddressSanitizer and UBSan into a stand-alone program: the emulator restates nothing of the kernels"""
    from fcaf3d_amd import build as B
    tmp = tmp_path_factory.mktemp('ema_emu')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(B.CSRC_POST, 'optim_ema.hip')).read()
    end = '}  // namespace'
    body = src[src.index('#define EMA_THREADS'):src.index(end) + len(end)]
    assert '#include' not in body and '#define EMA_MAX_RUNS 1024' in body and 'k_adamw_ema' in body and 'k_swap_f32' in body
    assert 'fp contract(off)' in open(os.path.join(B.CSRC_POST, 'ema_elem.h')).read()
    (tmp / 'ema_kernels.inc').write_text(body)
    cxx = os.path.join(os.path.dirname(os.path.dirname(B.HIPCC)), 'llvm', 'bin', 'clang++')
    cxx = cxx if os.path.exists(cxx) else shutil.which('clang++')
    exe = str(tmp / 'ema_host_emu')
    subprocess.check_call([cxx, '-std=c++20', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-pthread', f'-I{tmp}', os.path.join(root, 'tools', 'ema_host_emu.cpp'), '-o', exe])
    return exe, tmp


HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=3)
SIZES = (64, 192, 1024, 1088, 4160)      # a workgroup covers 1 024 floats: one slice, a partial workgroup, one workgroup, + one slice, 4 + one slice
TABLES = ('none', 'R1', 'R3')
MUS = (0.0002, 0.01, 0.5)
CLIPS = (None, (12.5, 0.8))


def draw(n, seed):
    """p, g, m, v, ema with magnitudes in [1e-3, 1e3]: no intermediate of either rule is subnormal"""
    rng = np.random.default_rng(seed)

    def mag():
        return (10.0 ** rng.uniform(-3, 3, n)).astype(f32)

    def signed():
        return mag() * rng.choice(np.array([-1, 1], f32), n)
    return signed(), signed(), signed(), mag(), signed()


def packed_table(begin, lr_mult, dec_mult, n):
    """the table as fc_adamw_groups_pack lays it out.  The kernel reads whatever runs it is given; where the pack accepts them (every
    run starts inside the buffer) its output is the one used"""
    words = np.concatenate([(np.asarray(begin, np.int64) // 64).astype(np.uint32), np.asarray(lr_mult, f32).view(np.uint32),
                            np.asarray(dec_mult, f32).view(np.uint32)]).view(np.uint8)
    if begin[-1] < n:
        assert np.array_equal(R.pack_runs(list(begin), list(lr_mult), list(dec_mult), n), words)
    return words


def table_of(kind, n=None):
    """-> (begin, lr_mult, decay_mult) in floats, or None.  R3: runs start at slice 1 and at slice 16, the workgroup edge"""
    if kind == 'none':
        return None
    if kind == 'R1':
        return [0], [0.5], [3.0]
    if kind == 'R3':
        return [0, 64, 1024], [1.0, 0.1, 2.0], [1.0, 0.0, 3.0]
    assert kind == 'cap'
    rng = np.random.default_rng(11)
    a = rng.choice(np.array([0.0, 0.1, 0.5, 1.0, 2.0], f32), R.MAX_RUNS)
    d = rng.choice(np.array([0.0, 1.0, 3.0], f32), R.MAX_RUNS)
    return list(range(0, 64 * R.MAX_RUNS, 64)), list(a), list(d)


def scalars(clip, mu, **hyper):
    h = dict(HYPER, **hyper)
    c = (0.0, 1.0) if clip is None else clip
    return np.array([h['lr'], h['b1'], h['b2'], h['eps'], h['wd'], 1.0 - h['b1'] ** h['step'], 1.0 - h['b2'] ** h['step'], c[0], c[1],
                     f32(mu), f32(1.0 - mu), 0], f32)


def emulate(emulator, arrays, table=None, clip=None, mu=0.5, mode=0):
    exe, tmp = emulator
    n = len(arrays[0])
    tab = packed_table(*table, n) if table is not None else np.zeros(0, np.uint8)
    with open(tmp / 'in.bin', 'wb') as f:
        np.array([n, len(table[0]) if table is not None else 0, 0 if clip is None else 1, mode], np.int64).tofile(f)
        scalars(clip, mu).tofile(f)
        if mode == 0:
            tab.tofile(f)
        for a in arrays:
            a.astype(f32).tofile(f)
    r = subprocess.run([exe, str(tmp / 'in.bin'), str(tmp / 'out.bin')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = np.fromfile(tmp / 'out.bin', f32)
    k = 4 if mode == 0 else 2
    assert len(out) == k * n
    return [out[j * n:(j + 1) * n] for j in range(k)]


def reference(p, g, m, v, e, table, clip, mu):
    """numpy: adamw_elem as tests/test_finetune_cpu.py restates it (no table: one run of multipliers 1), then the EMA rule on its p"""
    begin, a, d = table if table is not None else ([0], [1.0], [1.0])
    pp, mm, vv = adamw_groups_numpy(p, g, m, v, begin, a, d, clip, **HYPER)
    return pp, mm, vv, ema_numpy(e, pp, mu)


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


@pytest.mark.parametrize('clip', CLIPS, ids=['noclip', 'clip'])
@pytest.mark.parametrize('kind', TABLES)
@pytest.mark.parametrize('n', SIZES)
def test_kernel_text_on_the_host_equals_numpy(emulator, n, kind, clip):
    p, g, m, v, e = draw(n, 5 + n)
    table = table_of(kind)
    for mu in MUS:
        got = emulate(emulator, (p, g, m, v, e), table, clip, mu)
        want = reference(p, g, m, v, e, table, clip, mu)
        for x, y, name in zip(got, want, ('p', 'm', 'v', 'ema')):
            assert np.array_equal(bits(x), bits(y)), (n, kind, mu, name, int((bits(x) != bits(y)).sum()))
        assert not np.array_equal(got[3], e) and np.isfinite(got[3]).all()
        for x in got[:3] + [ema_numpy(e, got[0], mu), e.astype(f32) * f32(1.0 - mu), f32(mu) * got[0]]:
            assert (np.abs(x[x != 0]) >= np.finfo(f32).tiny).all()                          # no subnormal in sight


@pytest.mark.parametrize('clip', CLIPS, ids=['noclip', 'clip'])
def test_kernel_text_on_the_host_at_the_run_cap(emulator, clip):
    n = 65536
    assert R.MAX_RUNS * 64 == n                      # every slice its own run
    p, g, m, v, e = draw(n, 3)
    table = table_of('cap')
    got = emulate(emulator, (p, g, m, v, e), table, clip, 0.01)
    want = reference(p, g, m, v, e, table, clip, 0.01)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, want))


def test_padding_stays_zero_and_a_frozen_rate_averages_the_unchanged_parameter(emulator):
    n = 192
    p, g, m, v, e = draw(n, 17)
    for a in (p, g, m, v, e):
        a[60:64] = 0                                 # the padding floats of a parameter of 60 floats
    table = ([0, 64], [1.0, 0.0], [1.0, 1.0])
    got = emulate(emulator, (p, g, m, v, e), table, (3.0, 0.25), 0.5)
    assert all((x[60:64] == 0).all() for x in got)
    assert np.array_equal(bits(got[0][64:]), bits(p[64:]))                                  # lr_mult 0: the parameter keeps its bits
    assert np.array_equal(bits(got[3][64:]), bits(ema_numpy(e[64:], p[64:], 0.5)))


@pytest.mark.parametrize('n', SIZES + (0,))
def test_swap_kernel_text_exchanges_and_two_swaps_restore_every_bit(emulator, n):
    a, b = draw(n, 23 + n)[:2]
    if n:
        a[0], b[-1] = np.float32('nan'), -0.0        # bits, not values
    a1, b1 = emulate(emulator, (a, b), mode=1)
    assert np.array_equal(bits(a1), bits(b)) and np.array_equal(bits(b1), bits(a))
    a2, b2 = emulate(emulator, (a1, b1), mode=1)
    assert np.array_equal(bits(a2), bits(a)) and np.array_equal(bits(b2), bits(b))


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """the argument checks return before anything is launched: they run here, on fake addresses that are never dereferenced"""
    l = L.lib()
    P = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(6)]
    ok = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.1, 0.001)

    def ema(n=64, p=P[:5], hyper=ok, table=None, R_=0, mu=0.5, keep=0.5):
        return l.fc_adamw_ema_step(*p[:4], p[4], n, *hyper, None, table, R_, mu, keep, None)
    assert ema(n=66) == -1 and ema(n=-4) == -1
    assert ema(hyper=ok[:5] + (0.0, 0.001)) == -1 and ema(hyper=ok[:5] + (0.1, 0.0)) == -1
    assert ema(p=P[:4] + [None]) == -1                                                     # a null average with n > 0
    assert ema(n=0, p=[None] * 5) == 0                                                     # ... is fine with n == 0: nothing is launched
    assert ema(R_=1) == -1 and ema(table=P[5], R_=0) == -1 and ema(table=P[5], R_=R.MAX_RUNS + 1) == -1 and ema(table=P[5], R_=-1) == -1
    for bad in (-0.1, 1.5, float('nan'), float('inf'), -float('inf')):
        assert ema(mu=bad) == -1 and ema(keep=bad) == -1
    assert ema(n=0, mu=2.0) == -1
    swap = l.fc_swap_f32
    assert swap(P[0], P[0], 64, None) == -1 and swap(P[0], P[0], 0, None) == -1            # a == b
    assert swap(P[0], P[1], 66, None) == -1 and swap(P[0], P[1], -4, None) == -1
    assert swap(P[0], ctypes.c_void_p(0x1000 + 16), 64, None) == -1 and swap(ctypes.c_void_p(0x1000 + 252), P[0], 64, None) == -1      # overlap
    assert swap(None, P[1], 64, None) == -1 and swap(P[0], None, 64, None) == -1
    assert swap(P[0], P[1], 0, None) == 0                                                  # nothing to launch


# ---- 3. fit on the CPU ----------------------------------------------------------------------------------------------------------------------
HOOK = dict(type='EMAHook', momentum=0.5, warm_up=0)


def cfg_of(tmp_path, max_epochs=2, hook=HOOK, **over):
    if hook is not None:
        over['custom_hooks'] = [dict(hook)]
    return make_cfg(tmp_path / 'data', max_epochs=max_epochs, checkpoint_config=dict(interval=1, max_keep_ckpts=3), **over)


def stub():
    torch.manual_seed(0)
    return Stub()


def sd_of(path):
    return torch.load(path, map_location='cpu', weights_only=False)['state_dict']


@pytest.fixture(scope='module')
def hooked(tmp_path_factory):
    """the straight two-epoch run with the hook; the raw parameter before every step"""
    from fcaf3d_amd import fit
    tmp = tmp_path_factory.mktemp('ema_fit')
    model, raw = stub(), []
    rec = fit(model, cfg_of(tmp), str(tmp / 'hooked'), seed=3, device='cpu', on_batch=lambda e, it, b: raw.append(model.w.detach().clone()))
    return dict(tmp=tmp, model=model, raw=raw, rec=rec, work=tmp / 'hooked')


def test_fit_checkpoint_holds_the_average_and_the_raw_weights(hooked):
    from fcaf3d_amd import fit
    tmp = hooked['tmp']
    plain = stub()
    fit(plain, cfg_of(tmp, hook=None), str(tmp / 'plain'), seed=3, device='cpu')
    sd = sd_of(hooked['work'] / 'epoch_2.pth')
    assert list(sd) == ['w', 'ema_w']                                  # one ema_* entry per parameter, under mmcv's name
    assert torch.equal(sd['ema_w'], plain.w.detach())                  # the raw weights: training is not perturbed
    assert len(hooked['raw']) == 6 and torch.equal(hooked['raw'][0], stub().w.detach())
    # the replay: e starts as the initial parameter; after step s the parameter is what the NEXT step found (the last: the final raw)
    after = [t.numpy() for t in hooked['raw'][1:]] + [sd['ema_w'].numpy()]
    e = hooked['raw'][0].numpy().copy()
    mid = None
    for s, p in enumerate(after):
        e = ema_numpy(e, p, 0.5)
        if s == 2:
            mid = e.copy()
    assert np.array_equal(bits(sd['w'].numpy()), bits(e))
    assert not np.array_equal(sd['w'].numpy(), sd['ema_w'].numpy())
    sd1 = sd_of(hooked['work'] / 'epoch_1.pth')
    assert np.array_equal(bits(sd1['w'].numpy()), bits(mid)) and np.array_equal(bits(sd1['ema_w'].numpy()), bits(after[2]))
    assert torch.equal(hooked['model'].w.detach(), sd['w'])            # nothing swaps back after the last epoch
    assert all(r['mode'] == 'train' for r in hooked['rec'])
    assert sd_of(tmp / 'plain' / 'epoch_2.pth').keys() == {'w'}        # without the hook the file is what it was


def test_fit_resume_equals_the_straight_hooked_run(hooked):
    from fcaf3d_amd import fit
    tmp = hooked['tmp']
    work = tmp / 'resumed'
    fit(stub(), cfg_of(tmp, max_epochs=1), str(work), seed=3, device='cpu')
    model, seen = Stub(), []
    with torch.no_grad():
        model.w.zero_()
    raw1 = sd_of(work / 'epoch_1.pth')['ema_w']

    def on_batch(e, it, b):
        if not seen:
            assert torch.equal(model.w.detach(), raw1)                 # swapped back: the epoch trains on the raw weights
        seen.append(it)
    rec = fit(model, cfg_of(tmp, max_epochs=2), str(work), seed=3, device='cpu', resume_from=str(work / 'latest.pth'), on_batch=on_batch)
    assert seen == [3, 4, 5] and all(r['mode'] == 'train' for r in rec)
    a, b = sd_of(work / 'epoch_2.pth'), sd_of(hooked['work'] / 'epoch_2.pth')
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # the hook's own resume_from key is fit's when fit has none
    again = Stub()
    hook = dict(HOOK, resume_from=str(work / 'epoch_1.pth'))
    work2 = tmp / 'resumed_by_key'
    fit(again, cfg_of(tmp, max_epochs=2, hook=hook), str(work2), seed=3, device='cpu')
    c = sd_of(work2 / 'epoch_2.pth')
    assert all(torch.equal(c[k], b[k]) for k in b)
    fit(Stub(), cfg_of(tmp, max_epochs=2, hook=hook), str(tmp / 'w3'), seed=3, device='cpu', resume_from=str(work / 'epoch_1.pth'))      # equal: accepted
    with pytest.raises(ValueError, match='resume_from'):
        fit(Stub(), cfg_of(tmp, max_epochs=2, hook=hook), str(tmp / 'w4'), seed=3, device='cpu', resume_from=str(work / 'latest.pth'))


def test_fit_resume_from_a_file_without_the_average_says_so(hooked):
    from fcaf3d_amd import fit
    tmp = hooked['tmp']
    work = tmp / 'plain1'
    first = stub()
    fit(first, cfg_of(tmp, max_epochs=1, hook=None), str(work), seed=3, device='cpu')
    model, raw = Stub(), []
    rec = fit(model, cfg_of(tmp, max_epochs=2), str(work), seed=3, device='cpu', resume_from=str(work / 'latest.pth'),
              on_batch=lambda e, it, b: raw.append(model.w.detach().clone()))
    assert rec[0]['mode'] == 'ema' and rec[0]['resume_from'] == str(work / 'latest.pth') and sum(r['mode'] == 'ema' for r in rec) == 1
    assert torch.equal(raw[0], first.w.detach())
    sd = sd_of(work / 'epoch_2.pth')
    e = raw[0].numpy().copy()                                          # the average starts from the loaded weights
    for p in [t.numpy() for t in raw[1:]] + [sd['ema_w'].numpy()]:
        e = ema_numpy(e, p, 0.5)
    assert np.array_equal(bits(sd['w'].numpy()), bits(e))
    # a hooked checkpoint into a run without the hook: the strict load names the entry
    with pytest.raises(RuntimeError, match='ema_w'):
        fit(Stub(), cfg_of(tmp, max_epochs=3, hook=None), str(tmp / 'w5'), seed=3, device='cpu', resume_from=str(work / 'epoch_2.pth'))


def test_fit_load_from_a_hooked_checkpoint_starts_from_the_average(hooked, capsys):
    from fcaf3d_amd import fit
    tmp = hooked['tmp']
    ckpt = str(hooked['work'] / 'epoch_2.pth')
    model, first = Stub(), []
    with torch.no_grad():
        model.w.zero_()
    rec = fit(model, cfg_of(tmp, max_epochs=1, hook=None, load_from=ckpt), str(tmp / 'tuned'), seed=3, device='cpu',
              on_batch=lambda e, it, b: first.append(model.w.detach().clone()))
    assert rec[0]['mode'] == 'load' and rec[0]['unexpected'] == ['ema_w'] and rec[0]['missing'] == [] and rec[0]['mismatched'] == []
    assert torch.equal(first[0], sd_of(ckpt)['w'])
    capsys.readouterr()


def test_interval_skips_the_steps_that_are_not_due(tmp_path):
    """interval=2 on the per-tensor path: the average moves on steps 0, 2, 4 only, by M = momentum ** 2"""
    torch.manual_seed(0)
    model = Stub()
    tr = R.TrainStep(model, dict(type='AdamW', lr=0.01), ema=dict(type='EMAHook', momentum=0.5, interval=2, warm_up=0))
    e = model.w.detach().numpy().copy()
    for s in range(5):
        tr.set_iter(s)
        tr.optimizer.zero_grad()
        (model.w ** 2).sum().backward()
        before = tr.ema.state_dict()['ema_w'].clone()
        tr.close(None)
        got = tr.ema.state_dict()['ema_w']
        if s % 2:
            assert torch.equal(got, before)
        else:
            e = ema_numpy(e, model.w.detach().numpy(), 0.25)
            assert np.array_equal(bits(got.numpy()), bits(e)) and not torch.equal(got, before)
    w, avg = model.w.detach().clone(), tr.ema.state_dict()['ema_w']
    tr.ema.swap()
    assert tr.ema.swapped and torch.equal(model.w.detach(), avg) and torch.equal(tr.ema.state_dict()['ema_w'], w)
    tr.ema.swap()
    assert not tr.ema.swapped and torch.equal(model.w.detach(), w) and torch.equal(tr.ema.state_dict()['ema_w'], avg)
