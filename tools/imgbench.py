"""The batched weight-image build alone on the chip (tools/, not product): fc_x6_weight_images over every convolution kernel of the
benchmark's detector (what TrainStep rebuilds after each optimizer step), HIP-event timed — the whole build, and the zero, amax and
image pass each alone (fc_x6_weight_images_passes), an event pair around each.  Two descriptor sets: `plain`, the kernels as the
modules hold them (runner.TrainStep's own set), and `exec`, the executor's `_Weights` (the packed head kernel and the generative
convolutions' GEMM form in place of those modules' kernels: what the benchmark's step rebuilds).
    python tools/imgbench.py [--reps 30]        (FC_LIB=<other build of the same ABI> for an A/B)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                    # noqa: E402
import fcaf3d_amd._lib as L                                     # noqa: E402
import fcaf3d_amd.functional as Fn                              # noqa: E402
from fcaf3d_amd import executor                                 # noqa: E402
from fcaf3d_amd.nn import MinkowskiConvolution                  # noqa: E402


def timed(fn, reps):
    """-> (median, min) us of `fn` between two events, after three untimed calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    reps = 30
    if '--reps' in sys.argv:
        i = sys.argv.index('--reps')
        reps = int(sys.argv[i + 1])
        del sys.argv[i:i + 2]
    args = bench.parse()
    dev = torch.device('cuda:0')
    model, _ = bench.build_model(args)
    model = model.to(dev).train()
    ws = [m.kernel for m in model.modules() if isinstance(m, MinkowskiConvolution) and m.kernel.requires_grad]
    holder = executor._Weights(model, dev, executor.NetProgram.signature(model))
    holder.prepare()
    print(f'lib {os.environ.get("FC_LIB", "in-tree")}, {reps} builds each; units per amax block: {L.query("fc_x6_amax_units")}')
    for name, im in (('plain', Fn.WeightImages(ws)), ('exec', holder.images)):
        d = im.desc.cpu().view(-1, 8)
        n_w = int((d[:, 2] * d[:, 3] * d[:, 4])[d[:, 7] == 0].sum())             # weights of the entries that own a slot: the amax pass's reads
        n_all = int((d[:, 2] * d[:, 3] * d[:, 4]).sum())                          # ... of every entry: the image pass reads 4 and writes 4 bytes of each
        print(f'{name}: {im.n} images, {n_w / 1e6:.1f} M weights, {im.blocks} units, {im.amax_blocks} amax blocks')
        med, lo = timed(im.build, reps)
        print(f'  build       median {med:7.1f} us, min {lo:7.1f} us')
        for label, bit, nbytes in (('zero pass', 1, 0), ('amax pass', 2, 4 * n_w), ('image pass', 4, 8 * n_all)):
            med, lo = timed(lambda: L.call('fc_x6_weight_images_passes', L.ptr(im.desc), im.n, im.blocks, L.ptr(im.amax_chunks), im.amax_blocks,
                                           bit, L.stream()), reps)
            rate = f', {nbytes / med / 1e6:5.2f} TB/s at the median' if nbytes else ''
            print(f'  {label:11s} median {med:7.1f} us, min {lo:7.1f} us{rate}')


if __name__ == '__main__':
    main()
