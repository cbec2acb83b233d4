"""torch.autograd wrappers over the C ABI (libfcaf3d_hip.so).  fp32 only; every forward/backward is
HIP — there is no eager/CPU fallback (tensors on the CPU raise)."""
import os

import torch

from . import _lib as L
from .weight_images import ImageSet, WeightImages  # noqa: F401  (WeightImages: its home; importable from here as before)

# bits of the convolution `flags` word: the one Python mirror of include/fcaf3d_hip.h FC_CONV_* (tests/test_cabi.py compares them)
CONV_FMA = 1 << 0                        # the generic FMA kernels (parity cross-check)
CONV_BM_SHIFT, CONV_BN_SHIFT, CONV_TILE_MASK = 4, 6, 3      # tuning fields: tile rows / columns (1 = 64, 2 = 128, 3 = 256 rows)
CONV_S_SHIFT, CONV_S_MASK = 8, 255       # ... and the number of partial sums
CONV_WGRAD_PIPE_OFF = 1 << 16            # kernel variants (tools/nbench, tools/convbench.py, tests/test_gpu_ops.py)
CONV_PIPE_OFF = 1 << 17
CONV_PIPE_ON = 1 << 18
CONV_WGRAD_DEEP = 1 << 19
CONV_WGRAD_PIPE_ON = 1 << 20
CONV_GLDS = 1 << 21
CONV_GLDS_OFF = 1 << 22
CONV_WT = 1 << 23                        # W[k] is stored (Cout, Cin): the backward-data pass on the layer's own kernel
CONV_SPLIT = 1 << 24                     # split-bf16 / fp16 kernels (csrc/conv_x6.h, csrc/wgrad_x6.h)
CONV_IMAGE = 1 << 26                     # with CONV_SPLIT: W is a pre-split weight image
CONV_FLAT = 1 << 27                      # with CONV_SPLIT: flat 64-bit addresses instead of buffer descriptors
CONV_WGRAD_MULTI_OFF = 1 << 29
CONV_WGRAD_MULTI_FIRST = 1 << 30

FLAGS = int(os.environ.get('FC_FLAGS', '0'), 0)   # kernel-variant bits of every convolution launch (CONV_* above)

# Weight-gradient kernels are leaves of the backward graph: with WGRAD_ASYNC they are enqueued on a second HIP
# stream and overlap the backward-data chain on the main stream (the many small layers of the backbone do not
# fill 256 CUs on their own).  The main stream re-joins at the end of the backward pass (engine callback) and
# before any gradient is consumed earlier (dist.GradientAverager).
WGRAD_ASYNC = False
_wg_streams = {}
_join_queued = False


def wgrad_stream(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _wg_streams:
        _wg_streams[idx] = torch.cuda.Stream(device=idx, priority=0)
    return _wg_streams[idx]


def join_wgrad_stream():
    """Make the current stream wait for every weight-gradient kernel enqueued so far."""
    global _join_queued
    _join_queued = False
    for s in _wg_streams.values():
        torch.cuda.current_stream(s.device).wait_stream(s)


_flat_handed = set()          # ids of the leaf kernels whose flat gradient slice this backward pass has handed out
_flat_cb_queued = False


def _flat_pass_done():
    global _flat_cb_queued
    _flat_cb_queued = False
    _flat_handed.clear()


def _chk(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('fcaf3d_amd ops run on the GPU only (HIP); got a CPU tensor')


# ---- rows ------------------------------------------------------------------------------------------
def _gather(src, idx, n_out=None):
    n = idx.numel()
    out = torch.empty((n, src.shape[1]), dtype=src.dtype, device=src.device)
    L.call('fc_gather_rows', L.ptr(src), L.ptr(idx), n, src.shape[1], L.ptr(out), L.stream())
    return out


def _scatter_add(dst, idx, src):
    L.call('fc_scatter_rows_add', L.ptr(src), L.ptr(idx), idx.numel(), src.shape[1], L.ptr(dst), L.stream())


class _GatherRows(torch.autograd.Function):
    """dst[i] = src[idx[i]] with unique idx (pruning / per-scene split / first-occurrence pick)."""

    @staticmethod
    def forward(ctx, src, idx):
        _chk(src, idx)
        ctx.save_for_backward(idx)
        ctx.n_src = src.shape[0]
        return _gather(src.contiguous(), idx)

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        g = g.contiguous()
        out = torch.zeros((ctx.n_src, g.shape[1]), dtype=g.dtype, device=g.device)
        _scatter_add(out, idx, g)
        return out, None


def gather_rows(src, idx):
    return _GatherRows.apply(src, idx.to(torch.int32).contiguous())


# ---- convolution -----------------------------------------------------------------------------------
def _mfma_shape(Cin, Cout):
    return not (FLAGS & CONV_FMA) and Cin % 32 == 0 and Cout % 64 == 0


def _pair_conv(kmap, n_rows, Cin, Cout):
    """run this convolution per offset over the exact pair lists? (small, sparsely occupied 27-offset maps)"""
    from . import sparse as SP
    return (kmap is not None and kmap.use_pairs and n_rows <= SP.PAIR_CONV_ROWS and not (FLAGS & CONV_FMA)
            and Cin % 32 == 0 and Cout % 64 == 0)


STEM_COL = os.environ.get('FC_STEM_COL', '1') != '0'      # stem: save the gathered inputs in forward, stream them in the weight gradient
DGRAD_WT = os.environ.get('FC_DGRAD_TRANSPOSE', '0') != '1'      # backward-data reads the layer's own kernel (no transpose launch)


# fp32 convolutions on the bf16 matrix pipe by exact three-way operand splitting (csrc/conv_x6.h): forward and backward-data
# of every MFMA-shaped layer.  The kernel reads the weights as a pre-split image, rebuilt when the weights change.
X6 = os.environ.get('FC_X6', '1') != '0'
CONV_X6 = CONV_SPLIT | CONV_IMAGE        # forward / backward-data: split-bf16 kernel, weights as a pre-split image
WGRAD_X6 = CONV_SPLIT                    # weight gradient: split-bf16 kernels


def split_mode():
    """how the matrix-pipe convolutions cut an fp32 operand right now (csrc/conv.hip fc_get_split_mode): 2 = two fp16 pieces, three
    products (r6 default), 0 = three bf16 pieces, six products (r3-r5; also while the bf16 fast mode is on)"""
    return int(L.lib().fc_get_split_mode())


def set_split_mode(mode):
    """switch the operand split (0 / 2).  Weight images are mode-dependent: the mode is part of the key a `weight_images.ImageSet`
    was built under, so prebuilt ones are rebuilt before the next pass; the per-call images of the module path follow by themselves."""
    L.call('fc_set_split_mode', int(mode))


def set_bf16_fast(on):
    """the flagged NON-PARITY bf16 fast mode (csrc/conv.hip fc_set_bf16_fast); it reads six-product images: `split_mode()` reads 0
    while it is on, so the key of a `weight_images.ImageSet` built in the other mode no longer matches"""
    L.call('fc_set_bf16_fast', 1 if on else 0)


def _x6_image(weight, transposed):
    """pre-split image of a (K, Cin, Cout) kernel for the forward launch (transposed=False: reduction Cin, columns Cout) or
    for the backward-data launch on the same kernel (transposed=True: reduction Cout, columns Cin).  Built at every call:
    a cache across calls would have to know when the weights changed, and torch's fused optimizers update parameters
    without touching their version counters (measured: torch.optim.AdamW(fused=True) leaves `_version` at 0).  A training
    loop that owns the optimizer step hands over its own for one step: the set whose `ImageSet.lease()` is held is asked first."""
    pre = ImageSet.held.lookup(weight, transposed) if ImageSet.held is not None else None
    if pre is not None:
        return pre
    K, Cin, Cout = weight.shape
    R, C = (Cout, Cin) if transposed else (Cin, Cout)
    img = torch.empty(L.query('fc_x6_weight_image_bytes', K, R, C), dtype=torch.uint8, device=weight.device)
    L.call('fc_x6_weight_image', L.ptr(weight), L.ptr(img), K, R, C, 1 if transposed else 0, L.stream())
    return img


def _stats_table(n_out, K, Cin, Cout, flags, pairs, device):
    """(table, row blocks) for the statistics epilogue of this launch (fc_conv_stats_blocks), or (None, 0) if it has none"""
    nb = L.query('fc_conv_stats_blocks', n_out, K, Cin, Cout, flags, 1 if pairs else 0)
    if nb <= 0:
        return None, 0
    return torch.empty((nb, 2, Cout), dtype=torch.float32, device=device), nb


def _conv_pairs(x, w, lists, out, n_in, n_out, K, Cin, Cout, live_tiles=0, flags=None, stats=None):
    pi, _, pos, cnt = lists
    flags = FLAGS if flags is None else flags
    ws = L.workspace(L.query('fc_conv_fwd_pairs_ws_bytes', n_out, K, Cout), x.device)
    if stats is not None:
        L.call('fc_conv_fwd_pairs_tiles_stats', L.ptr(x), L.ptr(w), L.ptr(pi), L.ptr(cnt), L.ptr(pos), L.ptr(out), n_in, n_out, K,
               Cin, Cout, live_tiles, flags, L.ptr(ws), ws.numel(), L.ptr(stats), L.stream())
        return
    L.call('fc_conv_fwd_pairs_tiles', L.ptr(x), L.ptr(w), L.ptr(pi), L.ptr(cnt), L.ptr(pos), L.ptr(out), n_in, n_out, K, Cin,
           Cout, live_tiles, flags, L.ptr(ws), ws.numel(), L.stream())


def _conv_fwd(x, w, nbr, out, n_in, n_out, K, Cin, Cout, out_index=None, flags=None, stats=None):
    flags = FLAGS if flags is None else flags
    wsb = L.query('fc_conv_fwd_ws_bytes', n_out, K, Cin, Cout, flags)
    ws = L.workspace(wsb, x.device) if wsb else None
    if stats is not None:
        L.call('fc_conv_fwd_stats', L.ptr(x), L.ptr(w), L.ptr(nbr), L.ptr(out_index), L.ptr(out), n_in, n_out, K, Cin, Cout, flags,
               L.ptr(ws), ws.numel() if ws is not None else 0, L.ptr(stats), L.stream())
        return
    L.call('fc_conv_fwd', L.ptr(x), L.ptr(w), L.ptr(nbr), L.ptr(out_index), L.ptr(out), n_in, n_out, K, Cin, Cout, flags,
           L.ptr(ws), ws.numel() if ws is not None else 0, L.stream())


class _SparseConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, weight, kmap, n_out, training=True, want_stats=False):
        """feats (n_in,Cin), weight (K,Cin,Cout), kmap KernelMap or None (identity, K==1).  training: the caller is in
        training mode with gradients enabled (only then does the stem keep its gathered inputs for the weight gradient).
        want_stats (r5): a training-mode BatchNorm follows — also return the statistics table the launch's epilogue leaves
        ((nb, 2, Cout): column sums of the result and of its square per row block; None where the launch has no such epilogue):
        -> (out, table)"""
        _chk(feats, weight)
        feats = feats.contiguous()
        # only a LEAF kernel's gradient goes straight to AccumulateGrad (no kernel reads it before the join)
        ctx.w_leaf = weight.is_leaf and weight.is_contiguous()
        # a leaf kernel that lives in flat buffers (flat.FlatParams): its gradient is written straight into its slice
        ctx.flat = getattr(weight, '_fc_flat', None) if ctx.w_leaf else None
        weight = weight.contiguous()
        K, Cin, Cout = weight.shape
        n_in = feats.shape[0]
        out = torch.empty((n_out, Cout), dtype=torch.float32, device=feats.device)
        col = stats = None
        if (STEM_COL and training and kmap is not None and Cin == 3 and Cout == 64 and K <= 27 and not (FLAGS & CONV_FMA)
                and ctx.needs_input_grad[1]):
            # stem in training: keep the gathered inputs (n_out, 84) for the weight gradient (conv.hip: k_stem_fwd / k_stem_wgrad_col)
            col = torch.empty((n_out, 84), dtype=torch.float32, device=feats.device)
            L.call('fc_stem_conv_fwd', L.ptr(feats), L.ptr(weight), L.ptr(kmap.nbr), L.ptr(out), L.ptr(col), n_in, n_out, K,
                   L.stream())
        else:
            x6 = X6 and _mfma_shape(Cin, Cout)
            w, fl = (_x6_image(weight, False), FLAGS | CONV_X6) if x6 else (weight, FLAGS)
            pairs = _pair_conv(kmap, n_out, Cin, Cout)
            stats = _stats_table(n_out, K, Cin, Cout, fl, pairs, feats.device)[0] if (want_stats and BN_FUSE and x6) else None
            if pairs:
                _conv_pairs(feats, w, kmap.pairs(), out, n_in, n_out, K, Cin, Cout, kmap.pair_tiles(), flags=fl, stats=stats)
            else:
                nbr, oidx = ((kmap.sorted_fwd() if _mfma_shape(Cin, Cout) else (kmap.nbr, None))
                             if kmap is not None else (None, None))
                _conv_fwd(feats, w, nbr, out, n_in, n_out, K, Cin, Cout, oidx, flags=fl, stats=stats)
        ctx.has_col = col is not None
        ctx.save_for_backward(*((feats, weight, col) if col is not None else (feats, weight)))
        ctx.kmap = kmap
        if want_stats:
            if stats is not None:
                ctx.mark_non_differentiable(stats)
            ctx.set_materialize_grads(False)
            return out, stats
        return out

    @staticmethod
    def backward(ctx, gout, _gstats=None):
        feats, weight = ctx.saved_tensors[:2]
        kmap = ctx.kmap
        gout = gout.contiguous()
        K, Cin, Cout = weight.shape
        n_in, n_out = feats.shape[0], gout.shape[0]
        dev = feats.device
        gin = gw = None
        if ctx.needs_input_grad[0]:
            # the (Cout -> Cin) operator of the backward-data pass: the kernels read the layer's own (K, Cin, Cout) kernel as
            # its transpose (flags CONV_WT; r2: 50 transpose launches and 0.34 ms per step gone); identity maps (dense GEMMs)
            # still take a transposed copy
            if X6 and _mfma_shape(Cout, Cin):
                wt, fl = _x6_image(weight, True), FLAGS | CONV_X6
            elif DGRAD_WT and kmap is not None:
                wt, fl = weight, FLAGS | CONV_WT
            else:
                wt, fl = torch.empty((K, Cout, Cin), dtype=torch.float32, device=dev), FLAGS
                L.call('fc_transpose_weight', L.ptr(weight), L.ptr(wt), K, Cin, Cout, L.stream())
            gin = torch.empty((n_in, Cin), dtype=torch.float32, device=dev)
            if _pair_conv(kmap, n_in, Cout, Cin):
                _conv_pairs(gout, wt, kmap.pairs_t(), gin, n_out, n_in, K, Cout, Cin, kmap.pair_tiles(transposed=True), flags=fl)
            else:
                nbr_t, tidx = ((kmap.sorted_bwd() if _mfma_shape(Cout, Cin) else (kmap.nbr_t, None))
                               if kmap is not None else (None, None))
                _conv_fwd(gout, wt, nbr_t, gin, n_out, n_in, K, Cout, Cin, tidx, flags=fl)
        if ctx.needs_input_grad[1]:
            nbr, ridx = (kmap.nbr if kmap is not None else None), None      # wgrad walks rows in natural order (see conv.hip)

            col = ctx.saved_tensors[2] if ctx.has_col else None
            # a kernel used by TWO convolutions of one graph (shared weights) gets its slice only once per backward pass: the
            # second node would overwrite it and hand autograd an aliasing view (g2 + g2 instead of g1 + g2)
            flat = ctx.flat if (ctx.flat is not None and weight.grad is None and id(weight) not in _flat_handed) else None
            if flat is not None:
                global _flat_cb_queued
                _flat_handed.add(id(weight))
                if not _flat_cb_queued:
                    _flat_cb_queued = True
                    torch.autograd.Variable._execution_engine.queue_callback(_flat_pass_done)

            def launch():
                # flat storage: a FRESH view of the parameter's slice of the flat gradient buffer — autograd adopts it as
                # .grad without a copy because nothing else references the tensor object (an accumulating .grad takes a copy)
                g = flat[0].grad_view(weight) if flat is not None else torch.empty_like(weight)
                if col is not None:
                    ws = L.workspace(L.query('fc_stem_conv_wgrad_ws_bytes', n_out, K), dev)
                    L.call('fc_stem_conv_wgrad', L.ptr(col), L.ptr(gout), L.ptr(g), n_out, K, L.ptr(ws), ws.numel(), L.stream())
                    return g
                fl = FLAGS | WGRAD_X6 if X6 else FLAGS      # split-bf16 where the library has a kernel for the shape (wgrad_x6.h)
                wsb = L.query('fc_conv_wgrad_ws_bytes', n_out, K, Cin, Cout, fl)
                ws = L.workspace(wsb, dev)
                if kmap is not None and kmap.use_pairs and not (FLAGS & CONV_FMA) and Cin % 64 == 0 and Cout % 64 == 0:
                    pi, po, _, cnt = kmap.pairs()
                    L.call('fc_conv_wgrad_pairs', L.ptr(feats), L.ptr(gout), L.ptr(pi), L.ptr(po), L.ptr(cnt), L.ptr(g), n_in,
                           n_out, K, Cin, Cout, fl, L.ptr(ws), ws.numel(), L.stream())
                else:
                    L.call('fc_conv_wgrad', L.ptr(feats), L.ptr(gout), L.ptr(nbr), L.ptr(ridx), L.ptr(g), n_in, n_out, K, Cin,
                           Cout, fl, L.ptr(ws), ws.numel(), L.stream())
                return g
            if WGRAD_ASYNC and ctx.w_leaf:
                global _join_queued
                main = torch.cuda.current_stream()
                side = wgrad_stream(dev)
                side.wait_stream(main)                      # gout / activations are ready on the main stream
                with torch.cuda.stream(side):
                    gw = launch()
                for t in (feats, gout, nbr, col):
                    if t is not None:
                        t.record_stream(side)              # keep their memory until the side stream has read it
                # no second reference to gw may be kept here: AccumulateGrad only STEALS a gradient it holds the sole
                # reference to — otherwise it clones it on the spot, on the main stream, before the side stream has written it
                gw.record_stream(main)
                if not _join_queued:
                    _join_queued = True
                    torch.autograd.Variable._execution_engine.queue_callback(join_wgrad_stream)
            else:
                gw = launch()
        return gin, gw, None, None, None, None


def sparse_conv(feats, weight, kmap, n_out, training=True, want_stats=False):
    """want_stats: -> (out, statistics table | None), see _SparseConv.forward"""
    if want_stats:
        return _SparseConv.apply(feats, weight, kmap, n_out, training, True)
    return _SparseConv.apply(feats, weight, kmap, n_out, training)


# ---- normalisation + activation ---------------------------------------------------------------------
ACT = {None: 0, 'none': 0, 'relu': 1, 'elu': 2}


def col_stats(x, seg, nseg):
    """mean, biased var (nseg,C), count (nseg)."""
    n, C = x.shape
    dev = x.device
    mean = torch.empty((nseg, C), dtype=torch.float32, device=dev)
    var = torch.empty((nseg, C), dtype=torch.float32, device=dev)
    cnt = torch.empty(nseg, dtype=torch.float32, device=dev)
    ws = L.workspace(L.query('fc_col_stats_ws_bytes', n, C, nseg), dev)
    L.call('fc_col_stats', L.ptr(x), L.ptr(seg), 4 if seg is not None else 0, n, C, nseg, L.ptr(mean), L.ptr(var),
           L.ptr(cnt), L.ptr(ws), ws.numel(), L.stream())
    return mean, var, cnt


def seg_col_sums(x, seg, nseg):
    """(nseg,C) per-segment column sums of x (N,C), C % 4 == 0; seg int32 (N,) — deterministic."""
    n, C = x.shape
    out = torch.empty((nseg, C), dtype=torch.float32, device=x.device)
    ws = L.workspace(L.query('fc_col_stats_ws_bytes', n, C, nseg), x.device)
    L.call('fc_seg_col_sums', L.ptr(x.contiguous()), L.ptr(seg.contiguous()), 1, n, C, nseg, L.ptr(out), L.ptr(ws),
           ws.numel(), L.stream())
    return out


class _NormAct(torch.autograd.Function):
    """y = act(norm(x)*gamma + beta (+ residual)); statistics over segments (1 = batch norm, B = instance norm).
    In eval mode the caller passes fixed mean/var (stats_const=True) and the backward treats them as constants."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, seg, nseg, eps, act, mean, var, cnt, stats_const):
        _chk(x, gamma, beta, residual)
        x = x.contiguous()
        n, C = x.shape
        y = torch.empty_like(x)
        res = residual.contiguous() if residual is not None else None
        g = gamma.reshape(-1).contiguous() if gamma is not None else None
        b = beta.reshape(-1).contiguous() if beta is not None else None
        L.call('fc_norm_act_fwd', L.ptr(x), L.ptr(seg), 4 if seg is not None else 0, n, C, L.ptr(mean), L.ptr(var),
               float(eps), L.ptr(g), L.ptr(b), L.ptr(res), act, L.ptr(y), L.stream())
        # without a residual the backward pass recomputes act'(.) from x, gamma, beta (norm.hip bn_pre): y is not read there
        ctx.save_for_backward(x, y if res is not None else None, g, mean, var, cnt, seg, b)
        ctx.cfg = (nseg, float(eps), act, residual is not None, stats_const,
                   gamma.shape if gamma is not None else None, beta.shape if beta is not None else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, g, mean, var, cnt, seg, b = ctx.saved_tensors
        nseg, eps, act, has_res, stats_const, gshape, bshape = ctx.cfg
        if stats_const and nseg != 1:      # (before any launch; the model has no such layer)
            raise RuntimeError('backward through eval-mode normalisation over segments is not supported')
        gy = gy.contiguous()
        n, C = x.shape
        dev = x.device
        gx = torch.empty_like(x)
        gres = torch.empty_like(x) if has_res else None
        if stats_const:
            # constant statistics (an eval-mode BatchNorm whose layer trains): one pass, gx needs no sum (csrc/norm_eval.h); the sums
            # only where gamma or beta takes a gradient
            want = (gshape is not None and ctx.needs_input_grad[1]) or (bshape is not None and ctx.needs_input_grad[2])
            sums = torch.empty((2, C), dtype=torch.float32, device=dev) if want else None
            ws = L.workspace(L.query('fc_bn_eval_bwd_ws_bytes', n, C, int(want)), dev)
            L.call('fc_bn_eval_bwd', L.ptr(x), L.ptr(y), L.ptr(gy), None, n, C, L.ptr(mean), L.ptr(var), eps, L.ptr(g), L.ptr(b), act,
                   L.ptr(gx), L.ptr(gres), L.ptr(sums), None, L.ptr(ws), ws.numel(), L.stream())
            ggamma = sums[1].reshape(gshape) if want and gshape is not None and ctx.needs_input_grad[1] else None
            gbeta = sums[0].reshape(bshape) if want and bshape is not None and ctx.needs_input_grad[2] else None
            return gx, ggamma, gbeta, gres, None, None, None, None, None, None, None, None
        sums = torch.empty((nseg, 2, C), dtype=torch.float32, device=dev)
        ws = L.workspace(L.query('fc_norm_act_bwd_ws_bytes', n, C, nseg), dev)
        L.call('fc_norm_act_bwd', L.ptr(x), L.ptr(y), L.ptr(gy), L.ptr(seg), 4 if seg is not None else 0, n, C, nseg,
               L.ptr(mean), L.ptr(var), L.ptr(cnt), eps, L.ptr(g), L.ptr(b), act, L.ptr(gx), L.ptr(gres), L.ptr(sums),
               L.ptr(ws), ws.numel(), L.stream())
        if nseg == 1:
            ggamma = sums[0, 1].reshape(gshape) if gshape is not None else None
            gbeta = sums[0, 0].reshape(bshape) if bshape is not None else None
        else:
            ggamma = sums[:, 1].sum(0).reshape(gshape) if gshape is not None else None
            gbeta = sums[:, 0].sum(0).reshape(bshape) if bshape is not None else None
        return gx, ggamma, gbeta, gres, None, None, None, None, None, None, None, None


import os as _os
# r5: BatchNorm statistics from the producing convolution's epilogue, and the add of a two-consumer tensor's gradients inside the
# BatchNorm backward kernels (csrc/norm.hip fc_bn_train_fwd / fc_bn_train_bwd); 0: the r4 kernels (A/B switch)
BN_FUSE = _os.environ.get('FC_BN_FUSE', '1') != '0'
# matrices up to this size take the two-launch BatchNorm path (the `small_elems` of csrc/norm_route.h, where the r1 measurement stands)
BN_SMALL_ELEMS = 1024 * 1024


class _BNTrain(torch.autograd.Function):
    """Training-mode BatchNorm (+act, +residual) of an (N,C) matrix through one entry point per direction, with the statistics,
    the running-buffer update and the apply fused (csrc/norm.hip, routes: csrc/norm_route.h).
    part is None: a small matrix, fc_bn_act_train_fwd / fc_bn_act_train_bwd — 2 launches forward, 2 backward (k_bn1_*).
    part (nb, 2, groups * C): the statistics table of the convolution that produced x, fc_bn_train_fwd — the route the native
    executor takes, so that the two paths stay bit for bit equal in the forward pass; the backward pass is the r4 one
    (fc_bn_train_bwd without a table)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, eps, act, momentum, rmean, rvar, nbt, part, groups):
        _chk(x, gamma, beta, residual, part)
        x = x.contiguous()
        n, C = x.shape
        dev = x.device
        y = torch.empty_like(x)
        stats = torch.empty((2, C), dtype=torch.float32, device=dev)       # [mean, var]
        cnt = torch.empty(1, dtype=torch.float32, device=dev)
        res = residual.contiguous() if residual is not None else None
        g = gamma.reshape(-1).contiguous()
        b = beta.reshape(-1).contiguous()
        head = (L.ptr(x), n, C, float(eps), L.ptr(g), L.ptr(b), L.ptr(res), act, float(momentum), L.ptr(y), L.ptr(stats[0]),
                L.ptr(stats[1]), L.ptr(cnt), L.ptr(rmean), L.ptr(rvar), L.ptr(nbt))
        if part is None:
            ws = L.workspace(L.query('fc_bn_small_ws_bytes', C), dev)
            L.call('fc_bn_act_train_fwd', *head, L.ptr(ws), ws.numel(), L.stream())
        else:
            ws = L.workspace(L.query('fc_bn_train_ws_bytes', n, C), dev)
            L.call('fc_bn_train_fwd', *head, L.ptr(part), part.shape[0], groups, BN_SMALL_ELEMS, L.ptr(ws), ws.numel(), L.stream())
        ctx.save_for_backward(x, y if res is not None else None, g, stats, b, cnt)
        ctx.cfg = (float(eps), act, residual is not None, gamma.shape, beta.shape, part is None)
        ctx.mark_non_differentiable(stats, cnt)
        ctx.set_materialize_grads(False)           # no zero-filled grads for the two statistics outputs
        return y, stats, cnt

    @staticmethod
    def backward(ctx, gy, _gs, _gc):
        x, y, g, stats, b, cnt = ctx.saved_tensors
        eps, act, has_res, gshape, bshape, small = ctx.cfg
        gy = gy.contiguous()
        n, C = x.shape
        dev = x.device
        gx = torch.empty_like(x)
        gres = torch.empty_like(x) if has_res else None
        sums = torch.empty((2, C), dtype=torch.float32, device=dev)
        tail = (eps, L.ptr(g), L.ptr(b), act, L.ptr(gx), L.ptr(gres), L.ptr(sums))
        if small:
            ws = L.workspace(L.query('fc_bn_small_ws_bytes', C), dev)
            L.call('fc_bn_act_train_bwd', L.ptr(x), L.ptr(y), L.ptr(gy), n, C, L.ptr(stats[0]), L.ptr(stats[1]), *tail, L.ptr(ws),
                   ws.numel(), L.stream())
        else:
            ws = L.workspace(L.query('fc_bn_train_ws_bytes', n, C), dev)
            L.call('fc_bn_train_bwd', L.ptr(x), L.ptr(y), L.ptr(gy), None, n, C, L.ptr(stats[0]), L.ptr(stats[1]), L.ptr(cnt), *tail,
                   None, 0, BN_SMALL_ELEMS, L.ptr(ws), ws.numel(), L.stream())
        return gx, sums[1].reshape(gshape), sums[0].reshape(bshape), gres, None, None, None, None, None, None, None, None


class _BNTrainSmall(_BNTrain):
    """_BNTrain without a statistics table (a class of its own: oracle/record.py hooks `forward` per path)"""


class _BNTrainFused(_BNTrain):
    """_BNTrain behind a convolution's statistics table"""


def bn_train(x, gamma, beta, residual, eps, act, momentum, rmean, rvar, nbt, part=None, groups=1):
    """BatchNorm in training mode with buffer update; picks the two-launch path for small matrices.
    Returns y (and leaves mean/var/count of the batch on the device for inspection).
    part (r5): the statistics table of the convolution that produced x (sparse_conv(want_stats=True))."""
    n, C = x.shape
    if part is not None and n > 0 and gamma is not None and beta is not None:
        y, stats, cnt = _BNTrainFused.apply(x, gamma, beta, residual, eps, ACT[act], momentum, rmean, rvar, nbt, part, groups)
        return y, (stats[0:1], stats[1:2], cnt)
    if 0 < n * C <= BN_SMALL_ELEMS and gamma is not None and beta is not None:
        y, stats, cnt = _BNTrainSmall.apply(x, gamma, beta, residual, eps, ACT[act], momentum, rmean, rvar, nbt, None, 1)
        return y, (stats[0:1], stats[1:2], cnt)
    # general size: one statistics pass (shifted sums) + finalise/buffer update + apply = 3 launches
    xc = x.detach().contiguous()
    dev = x.device
    mean = torch.empty((1, C), dtype=torch.float32, device=dev)
    var = torch.empty((1, C), dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.float32, device=dev)
    ws = L.workspace(L.query('fc_bn_stats_ws_bytes', n, C), dev)
    L.call('fc_bn_stats_train', L.ptr(xc), n, C, float(momentum), L.ptr(mean), L.ptr(var), L.ptr(cnt), L.ptr(rmean),
           L.ptr(rvar), L.ptr(nbt), L.ptr(ws), ws.numel(), L.stream())
    y = _NormAct.apply(x, gamma, beta, residual, None, 1, eps, ACT[act], mean, var, cnt, False)
    return y, (mean, var, cnt)


def norm_act(x, gamma, beta, residual=None, seg=None, nseg=1, eps=1e-5, act=None, stats=None):
    """stats=None: batch statistics (training); stats=(mean,var,cnt): fixed statistics."""
    const = stats is not None
    if stats is None:
        stats = col_stats(x.detach().contiguous(), seg, nseg)
    mean, var, cnt = stats
    y = _NormAct.apply(x, gamma, beta, residual, seg, nseg, eps, ACT[act], mean, var, cnt, const)
    return y, stats


# ---- pooling ---------------------------------------------------------------------------------------
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, kmap):
        _chk(feats)
        feats = feats.contiguous()
        C = feats.shape[1]
        out = torch.empty((kmap.n_out, C), dtype=torch.float32, device=feats.device)
        arg = torch.empty((kmap.n_out, C), dtype=torch.int32, device=feats.device)
        L.call('fc_maxpool_fwd', L.ptr(feats), L.ptr(kmap.nbr), kmap.n_out, kmap.K, C, L.ptr(out), L.ptr(arg), L.stream())
        ctx.save_for_backward(arg)
        ctx.n_in = feats.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        arg, = ctx.saved_tensors
        g = g.contiguous()
        gin = torch.zeros((ctx.n_in, g.shape[1]), dtype=torch.float32, device=g.device)
        L.call('fc_maxpool_bwd', L.ptr(g), L.ptr(arg), g.shape[0], g.shape[1], L.ptr(gin), L.stream())
        return gin, None


def max_pool(feats, kmap):
    return _MaxPool.apply(feats, kmap)


# ---- union add -------------------------------------------------------------------------------------
class _UnionAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fa, fb, row_b, n_union):
        _chk(fa, fb)
        fa = fa.contiguous()
        fb = fb.contiguous()
        out = torch.zeros((n_union, fa.shape[1]), dtype=torch.float32, device=fa.device)
        out[:fa.shape[0]] = fa
        _scatter_add(out, row_b, fb)
        ctx.save_for_backward(row_b)
        ctx.n_a = fa.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        row_b, = ctx.saved_tensors
        g = g.contiguous()
        return g[:ctx.n_a], _gather(g, row_b), None, None


def union_add(a, b):
    """SparseTensor a + b (fcaf3d_neck_with_head.py:101)."""
    from .sparse import SparseTensor
    if a.cmap is b.cmap:
        return SparseTensor(a.F + b.F, coordinate_map_key=a.cmap)
    cm, rows, swapped = a.cmap.union(b.cmap)
    if swapped:          # a's voxels all lie in b: result on b's map = b.F with a.F added at a's rows
        return SparseTensor(_UnionAdd.apply(b.F, a.F, rows, cm.n), coordinate_map_key=cm)
    return SparseTensor(_UnionAdd.apply(a.F, b.F, rows, cm.n), coordinate_map_key=cm)


# ---- head epilogue ------------------------------------------------------------------------------------
class _HeadSplit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, bias, scale, n_reg, n_cls):
        """y (N, ld) = fused 1x1 head GEMM output -> centerness (N,1), bbox_pred (N,n_reg), cls_score (N,n_cls),
        cls_max (N,1, no gradient)  (fcaf3d_neck_with_head.py:256-279)."""
        _chk(y, bias, scale)
        y = y.contiguous()
        n, ld = y.shape
        dev = y.device
        b = bias.reshape(-1).contiguous()
        sc = scale.reshape(1).contiguous()
        cent = torch.empty((n, 1), dtype=torch.float32, device=dev)
        bbox = torch.empty((n, n_reg), dtype=torch.float32, device=dev)
        cls = torch.empty((n, n_cls), dtype=torch.float32, device=dev)
        cmax = torch.empty((n, 1), dtype=torch.float32, device=dev)
        L.call('fc_head_split_fwd', L.ptr(y), ld, L.ptr(b), L.ptr(sc), n, n_reg, n_cls, L.ptr(cent), L.ptr(bbox), L.ptr(cls),
               L.ptr(cmax), L.stream())
        ctx.save_for_backward(y, sc, bbox)
        ctx.dims = (n_reg, n_cls, bias.shape, scale.shape)
        ctx.mark_non_differentiable(cmax)
        return cent, bbox, cls, cmax

    @staticmethod
    def backward(ctx, g_cent, g_bbox, g_cls, _g_max):
        y, sc, bbox = ctx.saved_tensors
        n_reg, n_cls, bias_shape, scale_shape = ctx.dims
        n, ld = y.shape
        g_cent = g_cent.contiguous() if g_cent is not None else None
        g_bbox = g_bbox.contiguous() if g_bbox is not None else None
        g_cls = g_cls.contiguous() if g_cls is not None else None
        gy = torch.empty_like(y)
        gs_row = torch.empty(n, dtype=torch.float32, device=y.device)
        L.call('fc_head_split_bwd', L.ptr(y), ld, L.ptr(sc), L.ptr(bbox), L.ptr(g_cent), L.ptr(g_bbox), L.ptr(g_cls), n, n_reg,
               n_cls, L.ptr(gy), L.ptr(gs_row), L.stream())
        gbias = g_cls.sum(0).reshape(bias_shape) if g_cls is not None and ctx.needs_input_grad[1] else None
        gscale = gs_row.sum().reshape(scale_shape) if ctx.needs_input_grad[2] else None
        return gy, gbias, gscale, None, None


def head_split(y, bias, scale, n_reg, n_cls):
    return _HeadSplit.apply(y, bias, scale, n_reg, n_cls)
