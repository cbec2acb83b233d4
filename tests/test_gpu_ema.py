"""GPU: the weight average of mmcv's EMAHook — fc_adamw_ema_step / fc_swap_f32 on the sizes and run tables of
tests/test_ema_cpu.py against fc_adamw_step / fc_adamw_step_groups and numpy, bit for bit; runner.FlatAdamW with the average against
one without; and runner.fit with the hook on the two-level model of tests/test_gpu_fit.py: the swaps and the pre-split weight
images, the checkpoint's raw weights against the un-hooked run, resume."""
import pickle

import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from fcaf3d_amd import runner as R
from fcaf3d_amd.flat import FlatParams

from tests.test_ema_cpu import CLIPS, HYPER, MUS, SIZES, TABLES, bits, draw, ema_numpy, packed_table, table_of
from tests.test_fit_cpu import make_cfg
from tests.test_gpu_fit import SEED, _fresh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HOOK = dict(type='EMAHook', momentum=0.5, warm_up=0)
f32 = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).to(DEV)


def _hyper(step=HYPER['step']):
    h = HYPER
    return (h['lr'], h['b1'], h['b2'], h['eps'], h['wd'], 1.0 - h['b1'] ** step, 1.0 - h['b2'] ** step)


# ---- 4. the entry points --------------------------------------------------------------------------------------------------------------------
def _one_case(n, kind, clip, mu):
    p, g, m, v, e = draw(n, 5 + n)
    table = table_of(kind)
    clip_t = _dev(clip) if clip is not None else None
    tab_t, R_ = (None, 0)
    if table is not None:
        tab_t, R_ = torch.from_numpy(packed_table(*table, n).copy()).to(DEV), len(table[0])
    a = [_dev(x) for x in (p, g, m, v, e)]           # the fused launch
    b = [_dev(x) for x in (p, g, m, v)]              # the launch it must equal in p, m, v
    L.call('fc_adamw_ema_step', *(L.ptr(t) for t in a[:4]), L.ptr(a[4]), n, *_hyper(), L.ptr(clip_t), L.ptr(tab_t), R_,
           float(f32(mu)), float(f32(1.0 - mu)), L.stream())
    if table is None:
        L.call('fc_adamw_step', *(L.ptr(t) for t in b), n, *_hyper(), L.ptr(clip_t), L.stream())
    else:
        L.call('fc_adamw_step_groups', *(L.ptr(t) for t in b), n, *_hyper(), L.ptr(clip_t), L.ptr(tab_t), R_, L.stream())
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in a]
    want = [t.cpu().numpy() for t in b]
    for k, name in ((0, 'p'), (2, 'm'), (3, 'v')):
        assert np.array_equal(bits(got[k]), bits(want[k])), (n, kind, clip, mu, name)
    assert np.array_equal(bits(got[1]), bits(g)) and not np.array_equal(got[0], p)                  # the gradient is read only
    assert np.array_equal(bits(got[4]), bits(ema_numpy(e, got[0], mu))), (n, kind, clip, mu, 'ema')


def test_fused_launch_equals_the_plain_launches_and_numpy():
    k = 0
    for n in SIZES:
        for kind in TABLES:
            for clip in CLIPS:
                _one_case(n, kind, clip, MUS[k % 3])
                k += 1
    for clip in CLIPS:
        _one_case(65536, 'cap', clip, 0.01)


def test_swap_exchanges_every_bit_and_two_swaps_restore():
    for n in SIZES + (65536,):
        a, b = draw(n, 23 + n)[:2]
        a[0], b[-1] = np.float32('nan'), -0.0
        ta, tb = _dev(a), _dev(b)
        L.call('fc_swap_f32', L.ptr(ta), L.ptr(tb), n, L.stream())
        assert np.array_equal(bits(ta.cpu().numpy()), bits(b)) and np.array_equal(bits(tb.cpu().numpy()), bits(a)), n
        L.call('fc_swap_f32', L.ptr(ta), L.ptr(tb), n, L.stream())
        assert np.array_equal(bits(ta.cpu().numpy()), bits(a)) and np.array_equal(bits(tb.cpu().numpy()), bits(b)), n


def test_refused_arguments_launch_nothing():
    n = 1024
    arrays = draw(n, 1)
    t = [_dev(x) for x in arrays]
    big = torch.cat([_dev(arrays[0]), _dev(arrays[1])])
    l = L.lib()
    tab = torch.from_numpy(packed_table([0], [1.0], [1.0], n).copy()).to(DEV)
    P = [L.ptr(x) for x in t]

    def ema(n_=n, ema_ptr=P[4], hyper=_hyper(), table=None, R_=0, mu=0.5, keep=0.5):
        return l.fc_adamw_ema_step(P[0], P[1], P[2], P[3], ema_ptr, n_, *hyper, None, table, R_, mu, keep, L.stream())
    assert ema(n_=n - 2) == -1 and ema(ema_ptr=None) == -1
    assert ema(hyper=_hyper()[:5] + (0.0, 0.001)) == -1 and ema(hyper=_hyper()[:5] + (0.1, -1.0)) == -1
    assert ema(R_=1) == -1 and ema(table=L.ptr(tab), R_=0) == -1 and ema(table=L.ptr(tab), R_=R.MAX_RUNS + 1) == -1
    for bad in (-0.1, 1.5, float('nan'), float('inf')):
        assert ema(mu=bad) == -1 and ema(keep=bad) == -1
    assert l.fc_swap_f32(P[0], P[0], n, L.stream()) == -1 and l.fc_swap_f32(P[0], P[1], n - 2, L.stream()) == -1
    assert l.fc_swap_f32(big.data_ptr(), big.data_ptr() + 4 * (n - 4), n, L.stream()) == -1      # the ranges share 16 bytes
    assert l.fc_swap_f32(P[0], None, n, L.stream()) == -1
    torch.cuda.synchronize()
    assert all(np.array_equal(bits(x.cpu().numpy()), bits(y)) for x, y in zip(t, arrays))
    assert np.array_equal(bits(big.cpu().numpy()), bits(np.concatenate(arrays[:2])))
    assert l.fc_swap_f32(P[0], P[1], 0, L.stream()) == 0 and ema(n_=0) == 0                  # nothing to do: nothing launched
    torch.cuda.synchronize()
    assert all(np.array_equal(bits(x.cpu().numpy()), bits(y)) for x, y in zip(t, arrays))


# ---- 5. FlatAdamW with the average ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mults', [[(1.0, 1.0), (0.1, 1.0), (0.1, 0.0)], None], ids=['multipliers', 'plain'])
def test_flat_adamw_with_the_average_steps_as_without_and_follows_the_rule(mults):
    def make():
        torch.manual_seed(3)
        ps = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in ((60,), (7, 9), (130,))]
        flat = FlatParams(ps)
        return flat, R.FlatAdamW(flat, lr=1e-2, weight_decay=1e-2, multipliers=mults)
    (fa_, a), (fb, b) = make(), make()
    assert fa_.n == 320 and fa_.offsets == [0, 64, 128] and (a.table is not None) == (mults is not None)
    assert a.ema is None
    avg = a.enable_ema()
    assert a.enable_ema() is avg and torch.equal(avg, fa_.data) and avg.data_ptr() != fa_.data.data_ptr()
    sched = R.WeightEma(momentum=0.5, interval=2, warm_up=0)
    e = avg.cpu().numpy().copy()
    gen = torch.Generator(device='cpu').manual_seed(9)
    live = torch.zeros(320, dtype=torch.bool)
    for p, o in zip(fa_.params, fa_.offsets):
        live[o:o + p.numel()] = True
    for s in range(6):
        g = (torch.randn(320, generator=gen) * live).to(DEV)                # padding zero, as a step leaves it
        fa_.grad.copy_(g)
        fb.grad.copy_(g)
        c = sched.coeffs(s)
        na = a.step(10.0, gathered=True, ema=c)
        nb = b.step(10.0, gathered=True)
        assert torch.equal(fa_.data, fb.data) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq), s
        assert torch.equal(na, nb)
        got = avg.cpu().numpy()
        if s % 2:
            assert c is None and np.array_equal(bits(got), bits(e)), s      # not due: the average does not move
        else:
            assert c == (0.25, 0.75)
            e = ema_numpy(e, fa_.data.cpu().numpy(), 0.25)
            assert np.array_equal(bits(got), bits(e)), s
        assert (got[~live.numpy()] == 0).all()
    assert b.ema is None
    with pytest.raises(RuntimeError, match='enable_ema'):
        b.step(10.0, gathered=True, ema=(0.25, 0.75))


# ---- 6. / 7. fit ------------------------------------------------------------------------------------------------------------------------------
def _cfg(root, hook=True, **kw):
    over = dict(custom_hooks=[dict(HOOK)]) if hook else {}
    return make_cfg(root / 'data', log_config=dict(interval=1), checkpoint_config=dict(interval=1, max_keep_ckpts=2), **over, **kw)


@pytest.fixture(scope='module')
def hooked(tmp_path_factory):
    """two epochs of three steps with the hook and validation after every epoch; the TrainStep kept for the hand-called swap"""
    from fcaf3d_amd import fit
    from fcaf3d_amd.runner import TrainStep
    root = tmp_path_factory.mktemp('ema_gpu')
    dev = torch.device(DEV)
    cfg = _cfg(root, val=True)
    model = _fresh(dev)
    tr = TrainStep.from_config(model, cfg)
    assert tr.ema is not None and tr.ema.buf is not None and tr.images is not None
    rec = fit(model, cfg, str(root / 'work'), seed=SEED, step=tr)
    torch.cuda.synchronize()
    return dict(root=root, cfg=cfg, rec=rec, model=model, tr=tr, dev=dev)


def _val_loader(cfg, dev):
    from fcaf3d_amd import data as DT
    vs = DT.build_dataset(cfg.data.val)
    return DT.DeviceLoader(DT.ResidentScenes(vs, dev), vs.pipeline, 2, seed=SEED)


def _heads(model, batch):
    """eval-mode head outputs of every level before decoding -> (locations, class scores | box regressions), levels concatenated"""
    if model.training:
        model.eval()                                         # (eval() itself drops the executor's images: once, not per call)
    with torch.no_grad():
        x = model.extract_feat(batch['points'], batch['img_metas'])
        rows = torch.cat([lvl.full for lvl in x[3]]).clone()
        out = torch.cat([torch.cat([c.full, b.full], dim=1) for c, b in zip(x[2], x[1])]).clone()
    torch.cuda.synchronize()
    return rows, out


def _raw_state(sd, model):
    """the file's raw weights: every parameter's `ema_*` entry under the parameter's name, buffers as the file holds them"""
    names = {n: R.WeightEma.name_of(n) for n, _ in model.named_parameters()}
    assert sum(k.startswith('ema_') for k in sd) == len(names) and all(e in sd for e in names.values())
    out = {k: v for k, v in sd.items() if k not in set(names.values())}
    out.update({n: sd[e] for n, e in names.items()})
    return out


def test_swapped_weights_are_never_read_under_stale_images(hooked):
    from fcaf3d_amd import load_checkpoint
    dev, model, tr = hooked['dev'], hooked['model'], hooked['tr']
    path = str(hooked['root'] / 'work' / 'epoch_2.pth')
    batch = _val_loader(hooked['cfg'], dev).batches(0)[0]
    ref_a = _fresh(dev)
    rep = load_checkpoint(ref_a, path, map_location=dev, strict=False)['load_report']
    assert len(rep['unexpected']) == len(list(ref_a.parameters())) and not rep['missing'] and not rep['mismatched']
    sd = torch.load(path, map_location=dev, weights_only=False)['state_dict']
    ref_b = _fresh(dev)
    ref_b.load_state_dict(_raw_state(sd, ref_b), strict=True)
    rows_a, a = _heads(ref_a, batch)
    rows_b, b = _heads(ref_b, batch)
    assert tr.ema.swapped                                    # nothing swapped back after the last epoch
    model.static_weights = True                              # inference that trusts its images: only an invalidation rebuilds them
    try:
        rows, out = _heads(model, batch)
        assert torch.equal(rows, rows_a) and torch.equal(rows, rows_b)
        gap = float((a - b).abs().max())
        d_a = float((out - a).abs().max())
        print(f'after fit: |out - A| = {d_a:.3e}, |A - B| = {gap:.3e}')
        assert gap > 0 and d_a <= 1e-3 * gap
        tr.ema.swap()                                        # by hand: the model holds the raw weights again
        assert not tr.ema.swapped
        rows2, out2 = _heads(model, batch)
        d_b = float((out2 - b).abs().max())
        print(f'after swap(): |out - B| = {d_b:.3e}, |out - A| = {float((out2 - a).abs().max()):.3e}')
        assert torch.equal(rows2, rows_b) and d_b <= 1e-3 * gap
        tr.ema.swap()
        rows3, out3 = _heads(model, batch)
        assert float((out3 - a).abs().max()) <= 1e-3 * gap
    finally:
        model.static_weights = False
        model.train()


def test_val_records_equal_evaluate_on_the_saved_averaged_weights(hooked):
    from fcaf3d_amd import load_checkpoint
    from fcaf3d_amd.runner import evaluate
    cfg, dev = hooked['cfg'], hooked['dev']
    val = [r for r in hooked['rec'] if r['mode'] == 'val']
    assert [r['epoch'] for r in val] == [1, 2]
    infos = pickle.load(open(cfg.data.val['ann_file'], 'rb'))
    annos = [i['annos'] for i in infos]
    ld = _val_loader(cfg, dev)
    for r in val:
        model = _fresh(dev)
        load_checkpoint(model, str(hooked['root'] / 'work' / f'epoch_{r["epoch"]}.pth'), map_location=dev, strict=False)
        res = evaluate(model, ((b['points'], b['img_metas']) for b in ld.batches(0)), annos, metric=(0.25, 0.5), scene_ids=list(range(7)))
        got = {k: v for k, v in r.items() if k not in ('mode', 'epoch', 'iter', 'lr')}
        assert set(got) == set(res)
        np.testing.assert_equal(got, {k: float(v) for k, v in res.items()})


def test_raw_weights_equal_the_unhooked_run_and_resume_is_bitwise(hooked, tmp_path):
    from fcaf3d_amd import fit
    dev, root = hooked['dev'], hooked['root']
    plain = _fresh(dev)
    fit(plain, _cfg(root, hook=False), str(tmp_path / 'plain'), seed=SEED)
    torch.cuda.synchronize()
    sd = torch.load(root / 'work' / 'epoch_2.pth', map_location='cpu', weights_only=False)['state_dict']
    for n, p in plain.named_parameters():
        assert torch.equal(sd[R.WeightEma.name_of(n)], p.detach().cpu()), n      # the average rides along: training is not perturbed
    assert any(not torch.equal(sd[n], sd[R.WeightEma.name_of(n)]) for n, _ in plain.named_parameters())
    for n, b in plain.named_buffers():
        assert torch.equal(sd[n], b.detach().cpu()), n
    work = tmp_path / 'resumed'
    fit(_fresh(dev), _cfg(root, max_epochs=1), str(work), seed=SEED)
    model = _fresh(dev)
    fit(model, _cfg(root, max_epochs=2), str(work), seed=SEED, resume_from=str(work / 'latest.pth'))
    torch.cuda.synchronize()
    sd2 = torch.load(work / 'epoch_2.pth', map_location='cpu', weights_only=False)['state_dict']
    assert list(sd2) == list(sd)
    for k in sd:
        assert torch.equal(sd2[k], sd[k]), k
    for n, p in model.named_parameters():
        assert torch.equal(p.detach().cpu(), sd[n]), n                           # the model ends on the averaged weights
