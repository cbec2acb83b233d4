"""-m gpu: AdamW with per-parameter rate / decay multipliers on the flat buffers (csrc_post/optim_groups.hip, runner.FlatAdamW)
against torch.optim.AdamW with one group per tensor on the CPU — the optimizer mmcv's DefaultOptimizerConstructor builds from a
paramwise_cfg — with the shapes, gradient scales and bound of tests/test_gpu_model.py::test_flat_adamw_equals_torch_adamw_with_clip."""
import pytest
import torch

from fcaf3d_amd import _lib as L
from fcaf3d_amd.flat import ALIGN, FlatParams
from fcaf3d_amd.runner import FlatAdamW

pytestmark = pytest.mark.gpu

SHAPES = [(27, 64, 64), (128,), (1, 18), (), (8, 256, 128), (3,), (27, 3, 64)]
MULTS = [(0.1, 1.0), (0.1, 0.0), (2.0, 0.5), (1.0, 1.0), (0.0, 1.0), (0.5, 3.0), (1.0, 0.0)]      # one lr_mult = 0, decay_mult = 0 twice
SCALES = (40.0, 0.01, 3.0, 25.0, 0.5)                      # global norm above and below max_norm = 10


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _rel(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / max(1e-3, float(b.abs().max()))


def _padding_is_zero(flat, *bufs):
    for p, o in zip(flat.params, flat.offsets):
        end = o + -(-p.numel() // ALIGN) * ALIGN
        for b in bufs:
            if end > o + p.numel() and bool((b[o + p.numel():end] != 0).any()):
                return False
    return True


def _params(dev, seed=11):
    g = torch.Generator().manual_seed(seed)
    ref = [torch.nn.Parameter(torch.randn(s, generator=g) * 0.1) for s in SHAPES]
    mine = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ref]
    return g, ref, mine


def _set_grads(g, ref, mine, scale, dev):
    grads = [torch.randn(s, generator=g) * scale for s in SHAPES]
    for p, q, gr in zip(ref, mine, grads):
        p.grad = gr.clone()
        q.grad = gr.to(dev)


def test_grouped_adamw_equals_torch_adamw_with_one_group_per_tensor():
    dev = _dev()
    g, ref, mine = _params(dev)
    flat = FlatParams(mine)
    opt_r = torch.optim.AdamW([dict(params=[p], lr=1e-3 * a, weight_decay=1e-4 * b) for p, (a, b) in zip(ref, MULTS)], lr=1e-3, weight_decay=1e-4)
    opt_m = FlatAdamW(flat, lr=1e-3, weight_decay=1e-4, multipliers=MULTS)
    assert opt_m.table is not None and len(opt_m.runs[0]) == len(SHAPES) and len(opt_m.param_groups) == 1
    frozen0 = mine[4].detach().clone()
    calls = []
    orig = L.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    L.call = spy
    try:
        for step in range(5):
            _set_grads(g, ref, mine, SCALES[step], dev)
            norm_r = torch.nn.utils.clip_grad_norm_(ref, 10.0)
            opt_r.step()
            norm_m = opt_m.step(max_norm=10.0)
            assert abs(float(norm_m) - float(norm_r)) <= 1e-5 * float(norm_r), (float(norm_m), float(norm_r))
            errs = [_rel(q, p) for p, q in zip(ref, mine)]
            print(f'step {step}: clip {min(1.0, 10.0 / float(norm_r)):.3f}, worst parameter difference {max(errs):.2e}')
            assert max(errs) < 2e-6, (step, errs)
    finally:
        L.call = orig
    assert calls.count('fc_adamw_step_groups') == 5 and 'fc_adamw_step' not in calls
    sd, sd_r = opt_m.state_dict(), opt_r.state_dict()
    for i, st in sd_r['state'].items():
        assert _rel(sd['state'][i]['exp_avg'], st['exp_avg']) < 2e-6 and _rel(sd['state'][i]['exp_avg_sq'], st['exp_avg_sq']) < 2e-6, i
    assert torch.equal(mine[4].detach(), frozen0)                                     # lr_mult = 0: bit-unchanged ...
    assert float(sd['state'][4]['exp_avg'].abs().max()) > 0                           # ... while its moments advanced
    assert _padding_is_zero(flat, flat.data, opt_m.exp_avg, opt_m.exp_avg_sq)
    # torch's layout: one group per parameter with the effective rates, as the reference optimizer's own state_dict has them
    assert [gr['params'] for gr in sd['param_groups']] == [[i] for i in range(len(SHAPES))]
    for gr, gr_r in zip(sd['param_groups'], sd_r['param_groups']):
        assert gr['lr'] == gr_r['lr'] and gr['weight_decay'] == gr_r['weight_decay'] and tuple(gr['betas']) == tuple(gr_r['betas'])


def test_all_ones_take_the_plain_entry_and_the_grouped_entry_agrees_with_it():
    dev = _dev()
    g, ref, mine = _params(dev, 12)
    flat = FlatParams(mine)
    opt = FlatAdamW(flat, lr=1e-3, weight_decay=1e-4, multipliers=[(1.0, 1.0)] * len(SHAPES))
    assert opt.table is None
    calls = []
    orig = L.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    L.call = spy
    try:
        _set_grads(g, ref, mine, 40.0, dev)
        opt.step(max_norm=10.0)
    finally:
        L.call = orig
    assert 'fc_adamw_step' in calls and 'fc_adamw_step_groups' not in calls
    # the grouped entry called directly with all ones, on copies of the same state: one run, and one run per tensor
    from fcaf3d_amd.runner import pack_runs
    torch.manual_seed(3)
    n = flat.n
    state = [flat.data.clone(), torch.randn(n, device=dev) * 3, torch.randn(n, device=dev) * 0.1, torch.rand(n, device=dev) * 0.01]
    clip = torch.tensor([25.0, 0.4], device=dev)
    args = (n, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1.0 - 0.9 ** 3, 1.0 - 0.999 ** 3, L.ptr(clip))
    a = [t.clone() for t in state]
    L.call('fc_adamw_step', *(L.ptr(t) for t in a), *args, L.stream())
    for begin in ([0], list(flat.offsets)):
        R_ = len(begin)
        table = torch.from_numpy(pack_runs(begin, [1.0] * R_, [1.0] * R_, n)).to(dev)
        b = [t.clone() for t in state]
        L.call('fc_adamw_step_groups', *(L.ptr(t) for t in b), *args, L.ptr(table), R_, L.stream())
        torch.cuda.synchronize()
        # measured on the MI355X: the two kernels are bit-equal here (same operands, same operations, same contraction), so
        # equality is what is asserted, not the 2e-6 of the comparison with torch
        for x, y, name in zip(a, b, ('p', 'g', 'm', 'v')):
            assert torch.equal(x, y), (R_, name, _rel(y, x))


def test_state_round_trip_and_contradicting_groups():
    dev = _dev()
    g, ref, mine = _params(dev, 13)
    flat = FlatParams(mine)
    opt = FlatAdamW(flat, lr=1e-3, weight_decay=1e-4, multipliers=MULTS)
    for step in range(2):
        _set_grads(g, ref, mine, SCALES[step], dev)
        opt.step(max_norm=10.0)
    sd = opt.state_dict()
    mine2 = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    flat2 = FlatParams(mine2)
    opt2 = FlatAdamW(flat2, lr=5e-2, weight_decay=0.3, multipliers=MULTS)              # other base rates: the loaded ones win
    opt2.load_state_dict(sd)
    assert opt2.steps == 2 and opt2.param_groups[0]['lr'] == 1e-3 and opt2.param_groups[0]['weight_decay'] == 1e-4
    grads = [torch.randn(s, generator=g) * 3.0 for s in SHAPES]
    for q, q2, gr in zip(mine, mine2, grads):
        q.grad, q2.grad = gr.to(dev), gr.to(dev)
    opt.step(max_norm=10.0)
    opt2.step(max_norm=10.0)
    torch.cuda.synchronize()
    assert torch.equal(flat.data, flat2.data) and torch.equal(opt.exp_avg, opt2.exp_avg) and torch.equal(opt.exp_avg_sq, opt2.exp_avg_sq)
    # one group over all parameters (a checkpoint written without multipliers) loads too: its rates are the base rates
    plain = FlatAdamW(FlatParams([torch.nn.Parameter(p.detach().clone()) for p in mine]), lr=1e-3, weight_decay=1e-4)
    opt3 = FlatAdamW(FlatParams([torch.nn.Parameter(p.detach().clone()) for p in mine]), lr=1e-3, weight_decay=1e-4, multipliers=MULTS)
    opt3.load_state_dict(plain.state_dict())
    assert opt3.param_groups[0]['lr'] == 1e-3
    # groups written under other multipliers contradict the configured ones
    other = list(MULTS)
    other[2] = (1.0, 0.5)
    wrong = FlatAdamW(FlatParams([torch.nn.Parameter(p.detach().clone()) for p in mine]), lr=1e-3, weight_decay=1e-4, multipliers=other)
    with pytest.raises(ValueError, match='paramwise_cfg'):
        wrong.load_state_dict(sd)
    with pytest.raises(ValueError, match='paramwise_cfg'):
        plain.load_state_dict(sd)                                                    # configured all ones, loaded per-parameter rates
    bad = dict(sd, param_groups=sd['param_groups'][:3])
    with pytest.raises(ValueError, match='groups'):
        opt3.load_state_dict(bad)
