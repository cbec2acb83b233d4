"""GPU: gradient accumulation, mmcv's GradientCumulativeOptimizerHook — fc_grad_accum / fc_grad_accum_norm on the
sizes of tests/test_accum_cpu.py and past the norm pass's first sweep, against numpy and against fc_grad_norm on the materialised
sum, bit for bit; runner.FlatAdamW with accumulation against a twin that is handed the sum; runner.TrainStep on the two-level model of
tests/test_gpu_fit.py against a twin that forms the sum with torch ops; runner.fit with the hook, resumed inside a group; and the
default path's launches."""
import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from fcaf3d_amd import runner as R
from fcaf3d_amd.flat import FlatParams

from tests.test_accum_cpu import CLIP, HOOK, SCALES, SIZES, accum_numpy, lanes_of
from tests.test_ema_cpu import bits, ema_numpy
from tests.test_fit_cpu import make_cfg
from tests.test_gpu_fit import SEED, _fresh, _params

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
f32 = np.float32
# one float4 past the norm pass's first grid-stride sweep at the 1 024-block cap (1 024 blocks x 256 threads x 4 vectors): the masked second sweep runs
PAST_ONE_SWEEP = 4 * (1024 * 256 * 4) + 4


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).to(DEV)


def _host(t):
    return t.cpu().numpy()


def _grad_norm(G, max_norm):
    """fc_grad_norm on a materialised gradient -> its two floats"""
    out = torch.full((2,), -1.0, device=DEV)
    ws = L.workspace(L.query('fc_grad_norm_ws_bytes', G.numel()), G.device)
    L.call('fc_grad_norm', L.ptr(G), G.numel(), float(max_norm), L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
    return _host(out)


# ---- 1. the entry points --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES + (65536, PAST_ONE_SWEEP))
def test_entry_points_equal_numpy_and_the_plain_norm_bit_for_bit(n):
    acc, g, e, p = lanes_of(n, 31 + n)
    g[n - 3] = np.float32('nan')                     # passes through the accumulation
    clean = g.copy()
    clean[n - 3] = f32(0.25)                         # (the norm is compared on a finite gradient)
    for scale in SCALES:
        s = float(f32(scale))
        for first in (0, 1):
            want = accum_numpy(acc, g, scale, first)
            ta, tg = _dev(acc), _dev(g)
            L.call('fc_grad_accum', L.ptr(ta), L.ptr(tg), n, s, first, None, None, 0.0, 0.0, L.stream())
            assert np.array_equal(bits(_host(ta)), bits(want)), (n, scale, first)
            assert np.array_equal(bits(_host(tg)), bits(g))                                 # g is unchanged
            ta, tg, te, tp = _dev(acc), _dev(g), _dev(e), _dev(p)
            mu = 0.5 if first else 0.0002
            L.call('fc_grad_accum', L.ptr(ta), L.ptr(tg), n, s, first, L.ptr(te), L.ptr(tp), float(f32(mu)), float(f32(1.0 - mu)), L.stream())
            assert np.array_equal(bits(_host(ta)), bits(want)) and np.array_equal(bits(_host(tg)), bits(g))
            assert np.array_equal(bits(_host(tp)), bits(p))
            assert np.array_equal(bits(_host(te)), bits(ema_numpy(e, p, mu))), (n, scale, first, 'ema')
        G = accum_numpy(acc, clean, scale, 0)
        for max_norm in (10.0, 0.0):
            tg, ta, out2 = _dev(clean), _dev(acc), torch.full((2,), -1.0, device=DEV)
            ws = L.workspace(L.query('fc_grad_accum_norm_ws_bytes', n), tg.device)
            L.call('fc_grad_accum_norm', L.ptr(tg), L.ptr(ta), n, s, max_norm, L.ptr(out2), L.ptr(ws), ws.numel(), L.stream())
            got = _host(out2)
            assert np.array_equal(bits(_host(tg)), bits(G)), (n, scale)
            assert np.array_equal(bits(_host(ta)), bits(acc))                               # acc is unchanged
            want2 = _grad_norm(_dev(G), max_norm)
            assert np.array_equal(bits(got), bits(want2)), (n, scale, max_norm, got, want2)
            assert got[0] > 0 and (got[1] == 1.0 if max_norm == 0.0 else got[1] < 1.0)
        tg, ta = _dev(g), _dev(acc)                  # no clip configured: the sum alone, the NaN lane through it
        L.call('fc_grad_accum_norm', L.ptr(tg), L.ptr(ta), n, s, 0.0, None, None, 0, L.stream())
        assert np.array_equal(bits(_host(tg)), bits(accum_numpy(acc, g, scale, 0))) and np.array_equal(bits(_host(ta)), bits(acc))


def test_refused_arguments_launch_nothing():
    n = 1024
    arrays = lanes_of(n, 1)
    t = [_dev(x) for x in arrays]
    big = torch.cat([_dev(arrays[0]), _dev(arrays[1])])
    out2 = torch.full((2,), -1.0, device=DEV)
    ws = torch.zeros(8192, dtype=torch.uint8, device=DEV)
    l = L.lib()
    acc, g, e, p = (L.ptr(x) for x in t)
    st = L.stream()
    inf, nan = float('inf'), float('nan')
    assert l.fc_grad_accum(acc, g, n - 2, 0.5, 0, None, None, 0.0, 0.0, st) == -1
    for bad in (0.0, -0.5, nan, inf):
        assert l.fc_grad_accum(acc, g, n, bad, 0, None, None, 0.0, 0.0, st) == -1
        assert l.fc_grad_accum_norm(g, acc, n, bad, 10.0, L.ptr(out2), L.ptr(ws), ws.numel(), st) == -1
        assert l.fc_grad_accum_norm(g, acc, n, bad, 10.0, None, None, 0, st) == -1
    for bad in (-0.1, 1.5, nan, inf):
        assert l.fc_grad_accum(acc, g, n, 0.5, 0, e, p, bad, 0.5, st) == -1 and l.fc_grad_accum(acc, g, n, 0.5, 0, e, p, 0.5, bad, st) == -1
    assert l.fc_grad_accum(acc, acc, n, 0.5, 0, None, None, 0.0, 0.0, st) == -1
    assert l.fc_grad_accum(big.data_ptr(), big.data_ptr() + 4 * (n - 4), n, 0.5, 0, None, None, 0.0, 0.0, st) == -1      # the ranges share 16 bytes
    assert l.fc_grad_accum(acc, g, n, 0.5, 0, e, None, 0.5, 0.5, st) == -1                  # an average without the parameters
    assert l.fc_grad_accum(acc, g, n, 0.5, 0, acc, p, 0.5, 0.5, st) == -1 and l.fc_grad_accum(acc, g, n, 0.5, 0, g, p, 0.5, 0.5, st) == -1
    assert l.fc_grad_accum(None, g, n, 0.5, 0, None, None, 0.0, 0.0, st) == -1
    assert l.fc_grad_accum_norm(g, acc, n - 2, 0.5, 10.0, L.ptr(out2), L.ptr(ws), ws.numel(), st) == -1
    assert l.fc_grad_accum_norm(g, g, n, 0.5, 10.0, L.ptr(out2), L.ptr(ws), ws.numel(), st) == -1
    assert l.fc_grad_accum_norm(big.data_ptr() + 4 * (n - 4), big.data_ptr(), n, 0.5, 10.0, L.ptr(out2), L.ptr(ws), ws.numel(), st) == -1
    assert l.fc_grad_accum_norm(g, acc, n, 0.5, 10.0, L.ptr(out2), L.ptr(ws), ws.numel() - 1, st) == -2
    assert l.fc_grad_accum_norm(g, acc, n, 0.5, 10.0, L.ptr(out2), None, 0, st) == -2
    assert l.fc_grad_accum(acc, g, 0, 0.5, 0, None, None, 0.0, 0.0, st) == 0                 # nothing to do: nothing launched
    assert l.fc_grad_accum_norm(g, acc, 0, 0.5, 10.0, L.ptr(out2), L.ptr(ws), ws.numel(), st) == 0
    torch.cuda.synchronize()
    assert all(np.array_equal(bits(_host(x)), bits(y)) for x, y in zip(t, arrays))
    assert np.array_equal(bits(_host(big)), bits(np.concatenate(arrays[:2])))
    assert _host(out2).tolist() == [-1.0, -1.0] and not ws.any()


# ---- 2. FlatAdamW with accumulation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('average', [True, False], ids=['average', 'no_average'])
@pytest.mark.parametrize('mults', [[(1.0, 1.0), (0.1, 1.0), (0.1, 0.0)], None], ids=['multipliers', 'plain'])
def test_flat_adamw_accumulating_equals_a_twin_that_is_handed_the_sum(mults, average):
    def make():
        torch.manual_seed(3)
        ps = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in ((60,), (7, 9), (130,))]
        flat = FlatParams(ps)
        return flat, R.FlatAdamW(flat, lr=1e-2, weight_decay=1e-2, multipliers=mults)
    (fa_, a), (fb, b) = make(), make()
    assert fa_.n == 320 and a.acc is None
    sched = R.WeightEma(momentum=0.5, interval=1, warm_up=0) if average else None
    avg = a.enable_ema() if average else None
    e = _host(avg).copy() if average else None
    gen = torch.Generator(device='cpu').manual_seed(9)
    live = torch.zeros(320, dtype=torch.bool)
    for p, o in zip(fa_.params, fa_.offsets):
        live[o:o + p.numel()] = True
    it = steps = 0
    for k in (2, 3):
        s = float(f32(1.0 / k))
        total = None
        for j in range(6):
            g = (torch.randn(320, generator=gen) * live).to(DEV)             # padding zero, as a backward pass leaves it
            fa_.grad.copy_(g)
            scaled = torch.mul(g, s)
            total = scaled if total is None else torch.add(total, scaled)
            c = sched.coeffs(it) if average else None
            it += 1
            if (j + 1) % k:
                before = [t.clone() for t in (fa_.data, a.exp_avg, a.exp_avg_sq)]
                assert a.accumulate(s, j % k == 0, gathered=True, ema=c) is None
                assert torch.equal(a.acc, total) and torch.equal(fa_.grad, g), (k, j)
                assert all(torch.equal(x, y) for x, y in zip(before, (fa_.data, a.exp_avg, a.exp_avg_sq)))      # nothing stepped
                assert not a.acc[~live.to(DEV)].any()
            else:
                na = a.step(10.0, gathered=True, ema=c, accum_scale=s)
                fb.grad.copy_(total)
                nb = b.step(10.0, gathered=True)
                steps += 1
                assert torch.equal(fa_.grad, total), (k, j)                  # G stands where the gradient stood
                assert torch.equal(fa_.data, fb.data) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq), (k, j)
                assert torch.equal(na, nb) and float(na) > 0
                total = None
            if average:
                e = ema_numpy(e, _host(fa_.data), 0.5)                       # due every iteration: towards the parameters as they stand
                assert np.array_equal(bits(_host(avg)), bits(e)), (k, j)
                assert (_host(avg)[~live.numpy()] == 0).all()
    assert a.steps == b.steps == steps == 5 and not a.acc[~live.to(DEV)].any()
    assert b.acc is None
    with pytest.raises(RuntimeError, match='accumulate'):
        b.step(10.0, gathered=True, accum_scale=0.5)
    with pytest.raises(RuntimeError, match='open group'):
        b.accumulate(0.5, False, gathered=True)


# ---- 3. TrainStep on the two-level detector ---------------------------------------------------------------------------------------------------
def _cfg(root, k=2, hook=False, **kw):
    oc = dict(type=HOOK, cumulative_iters=k, grad_clip=dict(CLIP)) if k is not None else dict(grad_clip=dict(CLIP))
    over = dict(custom_hooks=[dict(type='EMAHook', momentum=0.5, warm_up=0)]) if hook else {}
    return make_cfg(root / 'data', log_config=dict(interval=1), checkpoint_config=dict(interval=1, max_keep_ckpts=4), optimizer_config=oc,
                    **over, **kw)


def _loader(cfg, dev):
    from fcaf3d_amd import data as DT
    ds = DT.build_dataset(cfg.data.train)
    return DT.DeviceLoader(DT.ResidentScenes(ds, dev), ds.pipeline, 2, seed=SEED)


def _pass(tr, model, batch, backward=True):
    """open / passing around one forward (+ backward) pass -> the loss"""
    images = tr.open()
    with tr.passing(images):
        loss = R.parse_losses(model(return_loss=True, **batch))
        if backward:
            loss.backward()
    tr.averager.finish()
    return images, loss.detach()


def test_train_step_accumulating_equals_a_twin_that_sums_with_torch_ops(tmp_path):
    dev = torch.device(DEV)
    cfg, plain_cfg = _cfg(tmp_path), _cfg(tmp_path, k=None)
    ld = _loader(cfg, dev)
    batches = ld.batches(0) + ld.batches(1)
    assert len(batches) >= 5
    model, twin = _fresh(dev), _fresh(dev)
    tr = R.TrainStep.from_config(model, cfg)
    tw = R.TrainStep.from_config(twin, plain_cfg)
    assert tr.cumulative_iters == 2 and tr.max_iters is None and isinstance(tr.optimizer, R.FlatAdamW) and tr.optimizer.acc is None
    from fcaf3d_amd import executor
    assert executor.program_for(model, True) is not None                       # the executor path
    norms, twin_norms = [], []
    for j, b in enumerate(batches[:4]):
        before = tr.flat.data.clone()
        tr.set_iter(j)
        tr(b)
        norms.append(tr.last_grad_norm)
        if j % 2 == 0:
            assert tr.last_grad_norm is None and tr.acc_iters == 1 and torch.equal(tr.flat.data, before)      # the weights did not move
        else:
            assert tr.acc_iters == 0 and not torch.equal(tr.flat.data, before)
        _pass(tw, twin, b)
        if not getattr(tw.flat, 'complete', False):
            tw.flat.gather()
        scaled = torch.mul(tw.flat.grad, 0.5)
        if j % 2 == 0:
            total = scaled
            continue
        tw.flat.grad.copy_(torch.add(total, scaled))
        twin_norms.append(tw.optimizer.step(10.0, gathered=True))
        tw.invalidate_images()                                                 # the next pass rebuilds the twin's images
    torch.cuda.synchronize()
    assert tr.optimizer.steps == tw.optimizer.steps == 2
    assert all(torch.equal(x, y) for x, y in zip(_params(model), _params(twin)))      # parameters and BatchNorm running statistics
    assert torch.equal(norms[1], twin_norms[0]) and torch.equal(norms[3], twin_norms[1])
    live = torch.zeros(tr.flat.n, dtype=torch.bool, device=dev)
    for p, o in zip(tr.flat.params, tr.flat.offsets):
        live[o:o + p.numel()] = True
    assert not tr.optimizer.acc[~live].any() and tr.optimizer.acc[live].any()                 # the padding stays zero
    # the pre-split weight images are current: a pass of both models over a fifth batch gives equal losses.  For the accumulating
    # loop it opens a group outside fit: flush steps it, and the state carries it until then
    tr.set_iter(4)
    la = tr(batches[4])[0].detach()
    lb = _pass(tw, twin, batches[4])[1]
    assert torch.isfinite(la) and torch.equal(la, lb)
    sd = tr.state_dict()
    assert tr.acc_iters == 1 and sd['grad_accum']['iters'] == 1 and len(sd['grad_accum']['grads']) == len(tr.flat.params)
    for v, p, o in zip(sd['grad_accum']['grads'], tr.flat.params, tr.flat.offsets):
        assert torch.equal(v, tr.optimizer.acc[o:o + p.numel()].view(p.shape))
    before = tr.flat.data.clone()
    assert tr.flush() is True and tr.acc_iters == 0 and tr.optimizer.steps == 3 and not torch.equal(tr.flat.data, before)
    assert 'grad_accum' not in tr.state_dict() and tr.flush() is False


# ---- 4. fit -----------------------------------------------------------------------------------------------------------------------------------
def test_fit_resumed_inside_a_group_equals_the_straight_run(tmp_path):
    from fcaf3d_amd import fit
    dev = torch.device(DEV)
    straight = _fresh(dev)
    rec = fit(straight, _cfg(tmp_path, hook=True, max_epochs=4), str(tmp_path / 'straight'), seed=SEED)      # T = 12
    train = [r for r in rec if r['mode'] == 'train']
    assert len(train) == 12 and ['grad_norm' in r for r in train] == [False, True] * 6
    work = tmp_path / 'resumed'
    fit(_fresh(dev), _cfg(tmp_path, hook=True, max_epochs=2), str(work), seed=SEED)                          # T = 6
    ck1 = torch.load(work / 'epoch_1.pth', map_location='cpu', weights_only=False)
    assert ck1['grad_accum']['iters'] == 1 and ck1['meta']['iter'] == 3
    assert 'grad_accum' not in torch.load(work / 'epoch_2.pth', map_location='cpu', weights_only=False)
    for start in ('epoch_2.pth', 'epoch_1.pth'):                               # at a group's edge, and inside a group
        model = _fresh(dev)
        rec = fit(model, _cfg(tmp_path, hook=True, max_epochs=4), str(tmp_path / ('from_' + start)), seed=SEED, resume_from=str(work / start))
        torch.cuda.synchronize()
        assert all(r['mode'] == 'train' for r in rec)
        assert all(torch.equal(x, y) for x, y in zip(_params(model), _params(straight))), start
        a = torch.load(tmp_path / ('from_' + start) / 'epoch_4.pth', map_location='cpu', weights_only=False)['state_dict']
        b = torch.load(tmp_path / 'straight' / 'epoch_4.pth', map_location='cpu', weights_only=False)['state_dict']
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a), start      # the averages and the raw `ema_*` weights too


# ---- 5. the default is untouched ----------------------------------------------------------------------------------------------------------------
def test_a_config_without_the_hook_makes_the_plain_launches(tmp_path, monkeypatch):
    dev = torch.device(DEV)
    cfg = _cfg(tmp_path, k=None)
    batches = _loader(cfg, dev).batches(0)
    model, twin = _fresh(dev), _fresh(dev)
    tr = R.TrainStep.from_config(model, cfg)
    tw = R.TrainStep.from_config(twin, cfg)
    calls, real = [], L.call

    def spy(name, *args):
        if name.startswith(('fc_grad', 'fc_adamw', 'fc_swap')):
            calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, 'call', spy)
    for b in batches[:3]:
        tr(b)
    assert calls == ['fc_grad_norm', 'fc_adamw_step'] * 3
    assert getattr(tr.optimizer, 'acc', None) is None and tr.optimizer.steps == 3
    del calls[:]
    for b in batches[:3]:                            # the call sequence of a step before accumulation existed, by hand
        images, _ = _pass(tw, twin, b)
        tw.last_grad_norm = tw.optimizer.step(tw.max_norm, gathered=bool(tw.averager.buckets))
        tw.it += 1
        tw.invalidate_images()
        if images is not None:
            images.rebuild_after_step(torch.cuda.current_stream(), R.Fn.wgrad_stream(tw.flat.data.device))
    torch.cuda.synchronize()
    assert calls == ['fc_grad_norm', 'fc_adamw_step'] * 3
    assert all(torch.equal(x, y) for x, y in zip(_params(model), _params(twin)))
    assert torch.equal(tr.last_grad_norm, tw.last_grad_norm)
