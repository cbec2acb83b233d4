"""What gradient accumulation (mmcv's GradientCumulativeOptimizerHook) costs on the chip (tools/, not product), on
bench.py's primary shape (8 scenes of 100 k points), in ONE process:

  * the launches, by HIP events, on the flat buffers of the benchmark's detector (about 70.5 M floats), in alternating windows:
    fc_adamw_step (twice per round: the distance between its two medians is the spread a difference has to exceed; its bandwidth is the
    yardstick of the byte bounds), fc_grad_norm, then fc_grad_accum first / later / later with the average and the fc_grad_accum_norm
    pair, each beside its unfused alternative in torch ops (torch.mul / torch.add, the three ops of the average's rule, fc_grad_norm
    on the materialised sum);
  * ms per micro-iteration of a TrainStep at cumulative_iters 1 (twice per round, for the spread), 2 and 4.

    python tools/accumbench.py [--rounds 4] [--window 20] [--window-warmup 4] [--opt-reps 20]  (+ bench.py's arguments)
window and window-warmup are rounded up to multiples of 4, so that every window holds whole groups.  Prints one JSON line."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                    # noqa: E402
import fcaf3d_amd.functional as Fn                              # noqa: E402
from fcaf3d_amd import _lib as L                                # noqa: E402
from fcaf3d_amd import runner as R                              # noqa: E402

CLIP = dict(max_norm=10, norm_type=2)


def pop(flag, default):
    if flag in sys.argv:
        i = sys.argv.index(flag)
        v = int(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return v
    return default


def build(args, dev, k):
    import fcaf3d_amd as fa
    cfg = fa.get_config(bench.CONFIG_OF[args.workload], voxel_size=args.voxel_size)
    m = cfg.model
    torch.manual_seed(0)
    model = fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg')).to(dev).train()
    model.async_maps = True
    model.inputs_resident = True
    oc = dict(grad_clip=dict(CLIP)) if k == 1 else dict(type='GradientCumulativeOptimizerHook', cumulative_iters=k, grad_clip=dict(CLIP))
    return model, R.TrainStep(model, cfg.optimizer, oc, cfg.get('lr_config'))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    rounds, window, wwarm, opt_reps = pop('--rounds', 4), pop('--window', 20), pop('--window-warmup', 4), pop('--opt-reps', 20)
    window, wwarm = -(-window // 4) * 4, -(-wwarm // 4) * 4
    args = bench.parse()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    Fn.WGRAD_ASYNC = True
    batches = bench.make_batches(args, 0, dev)
    R.reserve_device_memory(args.reserve_gb, dev)
    variants = [('k=1', 1), ('k=1 again', 1), ('k=2', 2), ('k=4', 4)]
    runs = {}
    for name, k in variants:
        model, tr = build(args, dev, k)
        runs[name] = dict(model=model, tr=tr, ms=[], i=0)

    def steps(r, n):
        for _ in range(n):
            r['tr'](batches[r['i'] % len(batches)], next_batch=batches[(r['i'] + 1) % len(batches)])
            r['i'] += 1

    for _ in range(rounds):
        for name, _k in variants:
            r = runs[name]
            steps(r, wwarm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(r, window)
            torch.cuda.synchronize()
            r['ms'].append((time.perf_counter() - t0) / window * 1e3)
    out = dict(what='tools/accumbench.py', workload=args.workload, scenes_per_micro_iteration=args.batch, rounds=rounds, window=window,
               source_hash=__import__('fcaf3d_amd.build', fromlist=['x']).source_hash(), step={})
    for name, _k in variants:
        r = runs[name]
        assert r['tr'].acc_iters == 0 and r['tr'].optimizer.steps * r['tr'].cumulative_iters == r['i']
        out['step'][name] = dict(ms_per_micro_iteration=[round(x, 3) for x in r['ms']], median_ms=round(median(r['ms']), 3))
    st = out['step']
    out['step_spread_ms'] = round(abs(st['k=1']['median_ms'] - st['k=1 again']['median_ms']), 3)
    base = min(st['k=1']['median_ms'], st['k=1 again']['median_ms'])
    out['step_minus_k1_ms'] = {k: round(st[k]['median_ms'] - base, 3) for k in ('k=2', 'k=4')}

    # ---- the launches alone, on one detector's flat buffers
    tr = runs['k=2']['tr']
    flat, opt = tr.flat, tr.optimizer
    n, g, acc = flat.n, flat.grad, opt.acc
    avg = flat.data.clone()
    torch.manual_seed(1)
    g.normal_()                      # (the padding floats are zero in a step; here they only have to be finite)
    acc.normal_()
    hyper = (n, 1e-5, 0.9, 0.999, 1e-8, 1e-4, 1.0 - 0.9 ** 50, 1.0 - 0.999 ** 50, L.ptr(opt.norm_clip))
    bufs = (L.ptr(flat.data), L.ptr(g), L.ptr(opt.exp_avg), L.ptr(opt.exp_avg_sq))
    ws = L.workspace(L.query('fc_grad_accum_norm_ws_bytes', n), dev)
    out2 = torch.zeros(2, device=dev)
    s, mu, keep = 0.5, 0.0002, 1.0 - 0.0002
    tmp = torch.empty_like(g)

    def adamw():
        L.call('fc_adamw_step', *bufs, *hyper, L.stream())

    def norm():
        L.call('fc_grad_norm', L.ptr(g), n, 10.0, L.ptr(out2), L.ptr(ws), ws.numel(), L.stream())

    def accum(first, ema):
        L.call('fc_grad_accum', L.ptr(acc), L.ptr(g), n, s, first, L.ptr(avg) if ema else None, L.ptr(flat.data) if ema else None,
               mu if ema else 0.0, keep if ema else 0.0, L.stream())

    def accum_norm():
        L.call('fc_grad_accum_norm', L.ptr(g), L.ptr(acc), n, s, 10.0, L.ptr(out2), L.ptr(ws), ws.numel(), L.stream())

    def torch_first():
        torch.mul(g, s, out=acc)

    def torch_later():
        torch.mul(g, s, out=tmp)
        acc.add_(tmp)

    def torch_later_avg():
        torch_later()
        avg.mul_(keep)
        torch.mul(flat.data, mu, out=tmp)
        avg.add_(tmp)

    def torch_norm():
        torch.mul(g, s, out=tmp)
        torch.add(acc, tmp, out=g)
        norm()
    kinds = [('fc_adamw_step', adamw), ('fc_adamw_step again', adamw), ('fc_grad_norm', norm),
             ('fc_grad_accum first', lambda: accum(1, False)), ('torch.mul', torch_first),
             ('fc_grad_accum later', lambda: accum(0, False)), ('torch.mul + add_', torch_later),
             ('fc_grad_accum later + average', lambda: accum(0, True)), ('torch.mul + add_ + 3 ops of the average', torch_later_avg),
             ('fc_grad_accum_norm', accum_norm), ('torch.mul + torch.add + fc_grad_norm', torch_norm)]
    times = {k: [] for k, _ in kinds}
    with torch.no_grad():
        for _ in range(rounds):
            for k, fn in kinds:
                for _ in range(3):
                    fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(opt_reps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                times[k].append(a.elapsed_time(b) / opt_reps * 1e3)
    med = {k: round(median(v), 1) for k, v in times.items()}
    spread = round(abs(med['fc_adamw_step'] - med['fc_adamw_step again']), 1)
    bw = 28 * n / (min(med['fc_adamw_step'], med['fc_adamw_step again']) * 1e-6)      # bytes per second fc_adamw_step reaches in this run
    pairs = [('fc_grad_accum first', 8, 'torch.mul'), ('fc_grad_accum later', 12, 'torch.mul + add_'),
             ('fc_grad_accum later + average', 24, 'torch.mul + add_ + 3 ops of the average'),
             ('fc_grad_accum_norm', 12, 'torch.mul + torch.add + fc_grad_norm')]
    out['launch'] = dict(floats=int(n), us={k: [round(x, 1) for x in v] for k, v in times.items()}, median_us=med, spread_us=spread,
                         adamw_tb_per_s=round(bw / 1e12, 2), fused={})
    for name, nbytes, other in pairs:
        bound = nbytes * n / bw * 1e6
        out['launch']['fused'][name] = dict(
            bytes_per_float=nbytes, median_us=med[name], byte_bound_us=round(bound, 1), over_byte_bound=round(med[name] / bound, 3),
            tb_per_s=round(nbytes * n / (med[name] * 1e-6) / 1e12, 2), unfused=other, unfused_median_us=med[other],
            unfused_minus_fused_us=round(med[other] - med[name], 1),
            fused_faster_than_unfused_by_more_than_the_spread=bool(med[other] - med[name] > spread))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
