"""What fine-tuning costs on the chip (tools/, not product; DESIGN.md sections 18, 19), on bench.py's primary shape, in ONE process:

  * ms per training step and the number of backward operator rows for backbone.frozen_stages = -1, 0, 1, 2, 4: alternating
    windows (one variant after the other, `--rounds` times), each window behind its own warm-up steps, and the -1 variant TWICE per
    round — the distance between its two windows is the spread a difference has to exceed;
  * in the same window scheme (section 19): `norm_eval` on the backbone, `norm_eval` on backbone and neck, and
    frozen_stages = 4 with `frozen_neck` (head only) — with the launches of their backward lists by operator;
  * the optimizer pass alone, by HIP events, on the flat buffers of the benchmark's detector (70 M floats): fc_adamw_step against
    fc_adamw_step_groups with all-ones multipliers (one run) and with the README's recipe (custom_keys backbone lr_mult 0.1,
    norm_decay_mult 0), the plain entry twice per round for its own spread.

    python tools/finetunebench.py [--rounds 4] [--window 20] [--window-warmup 5] [--opt-reps 20]  (+ bench.py's arguments)
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
from fcaf3d_amd import executor as EX                           # noqa: E402
from fcaf3d_amd import runner as R                              # noqa: E402

README_PARAMWISE = dict(custom_keys={'backbone': dict(lr_mult=0.1)}, norm_decay_mult=0.)


def pop(flag, default):
    if flag in sys.argv:
        i = sys.argv.index(flag)
        v = int(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return v
    return default


def build(args, dev, frozen, norm_eval=(False, False), frozen_neck=False):
    import fcaf3d_amd as fa
    cfg = fa.get_config(bench.CONFIG_OF[args.workload], voxel_size=args.voxel_size)
    m = cfg.model
    if frozen >= 0:
        m.backbone['frozen_stages'] = frozen
    if norm_eval[0]:
        m.backbone.update(norm_eval=True)
    if norm_eval[1]:
        m.neck_with_head.update(norm_eval=True)
    if frozen_neck:
        m.neck_with_head.update(frozen_neck=True)
    torch.manual_seed(0)
    model = fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg')).to(dev).train()
    model.async_maps = True
    model.inputs_resident = True
    return model, R.TrainStep.from_config(model, cfg)


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
    variants = [('-1', -1), ('-1 again', -1), ('0', 0), ('1', 1), ('2', 2), ('4', 4),
                ('norm_eval backbone', (-1, (True, False), False)), ('norm_eval backbone + neck', (-1, (True, True), False)),
                ('4 + frozen_neck (head only)', (4, (False, False), True))]
    runs = {}
    for name, k in variants:
        model, tr = build(args, dev, *(k if isinstance(k, tuple) else (k,)))
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
    out = dict(what='tools/finetunebench.py', workload=args.workload, scenes_per_step=args.batch, rounds=rounds, window=window,
               source_hash=__import__('fcaf3d_amd.build', fromlist=['x']).source_hash(), frozen_stages={}, norm_eval={})
    for name, k in variants:
        r = runs[name]
        prog = EX.program_for(r['model'], True)
        ops = {n[3:].lower(): int((prog.ops_b[:, EX.ROW_OP] == v).sum()) for n, v in vars(EX).items() if n.startswith('OP_') and isinstance(v, int)}
        out['frozen_stages' if not isinstance(k, tuple) else 'norm_eval'][name] = dict(
            ms_per_step=[round(x, 3) for x in r['ms']], median_ms=round(median(r['ms']), 3), rows_backward=int(len(prog.ops_b)),
            rows_forward=int(len(prog.ops_f)), trainable_floats=int(r['tr'].flat.n), backward_launches={n: c for n, c in ops.items() if c})
    base = out['frozen_stages']
    out['spread_ms'] = round(abs(base['-1']['median_ms'] - base['-1 again']['median_ms']), 3)

    # ---- the optimizer pass alone, on the unfrozen detector's flat buffers
    tr = runs['-1']['tr']
    flat, opt = tr.flat, tr.optimizer
    names = {id(p): n for n, p in runs['-1']['model'].named_parameters()}
    pm = R.param_multipliers(runs['-1']['model'], README_PARAMWISE)
    recipe = R.group_runs(flat.offsets, [pm[names[id(p)]] for p in flat.params])
    tables = dict(ones=([0], [1.0], [1.0]), recipe=recipe)
    dev_tables = {k: (torch.from_numpy(R.pack_runs(*v, flat.n)).to(dev), len(v[0])) for k, v in tables.items()}
    torch.manual_seed(1)
    flat.grad.normal_()
    # the padding floats of the gradient buffer are zero in a step; here they only have to be finite
    args_ = (L.ptr(flat.data), L.ptr(flat.grad), L.ptr(opt.exp_avg), L.ptr(opt.exp_avg_sq), flat.n, 1e-5, 0.9, 0.999, 1e-8, 1e-4,
             1.0 - 0.9 ** 50, 1.0 - 0.999 ** 50, L.ptr(opt.norm_clip))
    opt.norm_clip.copy_(torch.tensor([1.0, 1.0]))

    def plain():
        L.call('fc_adamw_step', *args_, L.stream())

    def grouped(which):
        t, n = dev_tables[which]
        return lambda: L.call('fc_adamw_step_groups', *args_, L.ptr(t), n, L.stream())
    kinds = [('fc_adamw_step', plain), ('fc_adamw_step again', plain), ('groups all ones', grouped('ones')), ('groups README recipe', grouped('recipe'))]
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
    out['optimizer'] = dict(floats=int(flat.n), runs_recipe=len(recipe[0]), bytes_per_float=28,
                            us={k: [round(x, 1) for x in v] for k, v in times.items()},
                            median_us={k: round(median(v), 1) for k, v in times.items()})
    mu = out['optimizer']['median_us']
    out['optimizer']['tb_per_s'] = {k: round(28 * flat.n / (v * 1e-6) / 1e12, 2) for k, v in mu.items()}
    out['optimizer']['spread_us'] = round(abs(mu['fc_adamw_step'] - mu['fc_adamw_step again']), 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
