"""Per-launch time of fc_bn_eval_bwd (with and without sums) against fc_bn_train_bwd (no producer table) on given BatchNorm shapes
(tools/, not product): ten launches of each form per shape, every form in a run of its own, for a kernel trace.

    rocprofv3 --kernel-trace --stats -- python tools/evalbwd_trace.py 436736x128 853x512
(the largest and the deepest BatchNorm of bench.py's primary step; profiles/norm_eval_kernel_stats.csv is the trace's stats table)"""
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fcaf3d_amd import _lib as L

dev = torch.device('cuda:0')
shapes = [tuple(int(v) for v in a.split('x')) for a in sys.argv[1:]]
for n, C in shapes:
    g = torch.Generator(device='cpu').manual_seed(n)
    x, gy = (torch.randn(n, C, generator=g).to(dev) for _ in range(2))
    mean, var = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    cnt = torch.full((1,), float(n), device=dev)
    gx, sums = torch.empty_like(x), torch.empty(2, C, device=dev)
    ws = torch.empty(max(L.query('fc_bn_train_ws_bytes', n, C), L.query('fc_bn_eval_bwd_ws_bytes', n, C, 1), 16), dtype=torch.uint8, device=dev)
    st = L.stream()
    # every form in a run of its own: each launch behind launches of the same form, so that what the caches hold is the same for all
    for rep in range(10):
        L.call('fc_bn_eval_bwd', L.ptr(x), None, L.ptr(gy), None, n, C, L.ptr(mean), L.ptr(var), 1e-5, L.ptr(gamma), L.ptr(beta), 1, L.ptr(gx), None,
               L.ptr(sums), None, L.ptr(ws), ws.numel(), st)
    for rep in range(10):
        L.call('fc_bn_eval_bwd', L.ptr(x), None, L.ptr(gy), None, n, C, L.ptr(mean), L.ptr(var), 1e-5, L.ptr(gamma), L.ptr(beta), 1, L.ptr(gx), None,
               None, None, L.ptr(ws), ws.numel(), st)
    for rep in range(10):
        L.call('fc_bn_train_bwd', L.ptr(x), None, L.ptr(gy), None, n, C, L.ptr(mean), L.ptr(var), L.ptr(cnt), 1e-5, L.ptr(gamma), L.ptr(beta), 1,
               L.ptr(gx), None, L.ptr(sums), None, 0, 1024 * 1024, L.ptr(ws), ws.numel(), st)
    torch.cuda.synchronize()
print('done', shapes)
