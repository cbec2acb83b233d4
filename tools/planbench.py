"""Stage 1 of the coordinate plan alone on the chip (tools/, not product): fc_plan_levels over the benchmark's 8 synthetic scenes
(fcaf3d_amd.synthetic, workload scannet-100k, 2 cm voxels, 4 levels) — no fc_plan_maps, no network.  Prints the median and the
minimum of --reps calls between two HIP events (the call ends with its own read-back of the counts), then, from calls with the
probe on (cfg[C_PROBE]: an event pair around every launch), the median time of every launch of the chain.
    python tools/planbench.py [--reps 30] [--batch 8]        (FC_LIB=<other build of the same ABI> for an A/B)
Knock-out libraries of k_plan_finalize (csrc/plan_chain.h FC_KO_PF_*) make WRONG plans: this tool is the only thing to run them
with.  `--ko DIR` builds them: DIR/<flag>/libfcaf3d_hip.so = the product library with plan.hip compiled under -D<flag>."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KO_FLAGS = ('FC_KO_PF_NOCOUNT', 'FC_KO_PF_NOINSERT', 'FC_KO_PF_NOVALS')


def build_knockouts(out_dir):
    from fcaf3d_amd import build as B
    B.build(verbose=False)
    objs = [os.path.join(d, s[:-4] + '.o') for d, s in B._sources()]
    plan_o = os.path.join(B.CSRC, 'plan.o')
    for flag in KO_FLAGS:
        d = os.path.join(out_dir, flag)
        os.makedirs(d, exist_ok=True)
        ko = os.path.join(d, 'plan.o')
        subprocess.check_call([B.HIPCC] + B.FLAGS + ['-D' + flag, '-c', os.path.join(B.CSRC, 'plan.hip'), '-o', ko])
        subprocess.check_call([B.HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', os.path.join(d, 'libfcaf3d_hip.so'), ko] +
                              [o for o in objs if o != plan_o])
        print(os.path.join(d, 'libfcaf3d_hip.so'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--probe-reps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--levels', type=int, default=4)
    ap.add_argument('--voxel-size', type=float, default=0.02)
    ap.add_argument('--ko', metavar='DIR', help='build the knock-out libraries under DIR and exit (no GPU needed)')
    args = ap.parse_args()
    if args.ko:
        return build_knockouts(args.ko)
    import fcaf3d_amd._lib as L
    from fcaf3d_amd import plan as PL
    from fcaf3d_amd.synthetic import WORKLOADS, make_scene
    dev = torch.device('cuda:0')
    pts = [torch.from_numpy(make_scene(i, **WORKLOADS['scannet-100k']['scene'])[0]).to(dev) for i in range(args.batch)]
    B, nl, nfeat = len(pts), args.levels, pts[0].shape[1] - 3
    total = sum(p.shape[0] for p in pts)
    lib = L.lib()
    cfg = np.zeros(lib.fc_plan_cfg_words(), dtype=np.int64)
    cfg[PL.C_B], cfg[PL.C_NL], cfg[PL.C_NFEAT], cfg[PL.C_TOTAL] = B, nl, nfeat, total
    cfg[PL.C_VS], cfg[PL.C_FEATDIV], cfg[PL.C_PT_STRIDE] = PL._f64_bits(args.voxel_size), PL._f64_bits(255.0), pts[0].shape[1]
    scenes = np.array([[p.data_ptr(), p.shape[0], p.shape[1]] for p in pts], dtype=np.int64)
    out = np.zeros(lib.fc_plan_out_words(B, nl), dtype=np.int64)
    counts = torch.zeros(PL.pinned_words(B, nl)[0], dtype=torch.int32).pin_memory()
    arena = torch.empty(L.query('fc_plan_stage1_bytes', total, B, nl, nfeat), dtype=torch.uint8, device=dev)

    def levels():
        rc = lib.fc_plan_levels(cfg.ctypes.data, scenes.ctypes.data, arena.data_ptr(), arena.numel(), out.ctypes.data, counts.data_ptr(), L.stream())
        assert rc == 0, rc

    for _ in range(3):
        levels()
    torch.cuda.synchronize()
    S = 3 + nl
    rows = [int(counts[PL.METAW * s + PL.META_ROWS]) for s in range(S)]
    print(f'lib {os.environ.get("FC_LIB", "in-tree")}: {B} scenes, {total} points, rows per set {rows}')
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        levels()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    print(f'fc_plan_levels, {args.reps} calls: median {ts[len(ts) // 2]:7.1f} us, min {ts[0]:7.1f} us')
    cfg[PL.C_PROBE] = 1
    PL.probe_read()
    per = []
    for _ in range(args.probe_reps):
        levels()
        torch.cuda.synchronize()
        per.append(PL.probe_read())
    med = [(per[0][k][0], float(np.median([p[k][2] for p in per]) * 1e3)) for k in range(len(per[0]))]
    for kind in ('flags_scan', 'finalize_insert'):
        t = [v for k, v in med if k == kind]
        print(f'  {kind:16s} per set (us, median of {args.probe_reps}): ' + ' '.join(f'{v:6.1f}' for v in t) + f'   sum {sum(t):7.1f}')
    for kind in ('tables_init', 'collate_insert'):
        print(f'  {kind:16s} {sum(v for k, v in med if k == kind):6.1f} us')
    print(f'  all launches     {sum(v for _, v in med):6.1f} us')


if __name__ == '__main__':
    main()
