"""What the weight average of mmcv's EMAHook costs on the chip (tools/, not product), on bench.py's primary
shape (8 scenes of 100 k points), in ONE process:

  * the launch, by HIP events, on the flat buffers of the benchmark's detector (about 70.5 M floats), in alternating windows:
    fc_adamw_step (twice per round: the distance between its two medians is the spread a difference has to exceed),
    fc_adamw_ema_step (the fused launch, 36 B per float), and fc_adamw_step followed by the three torch ops of the rule on the flat
    buffer (e.mul_(keep); t = p * mu; e.add_(t) — the unfused alternative);
  * ms per training step of a TrainStep with and without the hook (momentum 0.0002, interval 1: every step's update is due), the
    variant without it twice per round for the spread.

    python tools/emabench.py [--rounds 4] [--window 20] [--window-warmup 5] [--opt-reps 20]  (+ bench.py's arguments)
Prints one JSON line."""
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

HOOK = dict(type='EMAHook', momentum=0.0002, interval=1, warm_up=100)


def pop(flag, default):
    if flag in sys.argv:
        i = sys.argv.index(flag)
        v = int(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return v
    return default


def build(args, dev, hook):
    import fcaf3d_amd as fa
    cfg = fa.get_config(bench.CONFIG_OF[args.workload], voxel_size=args.voxel_size)
    m = cfg.model
    torch.manual_seed(0)
    model = fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg')).to(dev).train()
    model.async_maps = True
    model.inputs_resident = True
    return model, R.TrainStep.from_config(model, cfg, ema=dict(HOOK) if hook else None)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    rounds, window, wwarm, opt_reps = pop('--rounds', 4), pop('--window', 20), pop('--window-warmup', 5), pop('--opt-reps', 20)
    args = bench.parse()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    Fn.WGRAD_ASYNC = True
    batches = bench.make_batches(args, 0, dev)
    R.reserve_device_memory(args.reserve_gb, dev)
    variants = [('plain', False), ('plain again', False), ('EMAHook', True)]
    runs = {}
    for name, hook in variants:
        model, tr = build(args, dev, hook)
        runs[name] = dict(model=model, tr=tr, ms=[], i=0)

    def steps(r, n):
        for _ in range(n):
            r['tr'](batches[r['i'] % len(batches)], next_batch=batches[(r['i'] + 1) % len(batches)])
            r['i'] += 1

    for _ in range(rounds):
        for name, _h in variants:
            r = runs[name]
            steps(r, wwarm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(r, window)
            torch.cuda.synchronize()
            r['ms'].append((time.perf_counter() - t0) / window * 1e3)
    out = dict(what='tools/emabench.py', workload=args.workload, scenes_per_step=args.batch, rounds=rounds, window=window, hook=HOOK,
               source_hash=__import__('fcaf3d_amd.build', fromlist=['x']).source_hash(), step={})
    for name, _h in variants:
        r = runs[name]
        out['step'][name] = dict(ms_per_step=[round(x, 3) for x in r['ms']], median_ms=round(median(r['ms']), 3))
    st = out['step']
    out['step_spread_ms'] = round(abs(st['plain']['median_ms'] - st['plain again']['median_ms']), 3)
    out['step_added_ms'] = round(st['EMAHook']['median_ms'] - min(st['plain']['median_ms'], st['plain again']['median_ms']), 3)

    # ---- the launch alone, on the hooked detector's flat buffers
    tr = runs['EMAHook']['tr']
    flat, opt = tr.flat, tr.optimizer
    avg = opt.ema
    torch.manual_seed(1)
    flat.grad.normal_()
    # the padding floats of the gradient buffer are zero in a step; here they only have to be finite
    hyper = (flat.n, 1e-5, 0.9, 0.999, 1e-8, 1e-4, 1.0 - 0.9 ** 50, 1.0 - 0.999 ** 50, L.ptr(opt.norm_clip))
    bufs = (L.ptr(flat.data), L.ptr(flat.grad), L.ptr(opt.exp_avg), L.ptr(opt.exp_avg_sq))
    opt.norm_clip.copy_(torch.tensor([1.0, 1.0]))
    mu, keep = tr.ema.coeffs(10 ** 6)

    def plain():
        L.call('fc_adamw_step', *bufs, *hyper, L.stream())

    def fused():
        L.call('fc_adamw_ema_step', *bufs, L.ptr(avg), *hyper, None, 0, mu, keep, L.stream())

    def unfused():
        plain()
        with torch.no_grad():
            avg.mul_(keep)
            t = flat.data * mu
            avg.add_(t)
    kinds = [('fc_adamw_step', plain), ('fc_adamw_step again', plain), ('fc_adamw_ema_step', fused), ('fc_adamw_step + 3 torch ops', unfused)]
    times = {k: [] for k, _ in kinds}
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
    tb = lambda nbytes, us: round(nbytes * flat.n / (us * 1e-6) / 1e12, 2)
    out['launch'] = dict(floats=int(flat.n), us={k: [round(x, 1) for x in v] for k, v in times.items()}, median_us=med, spread_us=spread,
                         bytes_per_float={'fc_adamw_step': 28, 'fc_adamw_ema_step': 36},
                         tb_per_s={'fc_adamw_step': tb(28, med['fc_adamw_step']), 'fc_adamw_step again': tb(28, med['fc_adamw_step again']),
                                   'fc_adamw_ema_step': tb(36, med['fc_adamw_ema_step'])},
                         fused_over_plain=round(med['fc_adamw_ema_step'] / med['fc_adamw_step'], 3), bytes_ratio=round(36 / 28, 3),
                         unfused_minus_fused_us=round(med['fc_adamw_step + 3 torch ops'] - med['fc_adamw_ema_step'], 1),
                         fused_faster_than_unfused_by_more_than_the_spread=bool(
                             med['fc_adamw_step + 3 torch ops'] - med['fc_adamw_ema_step'] > spread))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
