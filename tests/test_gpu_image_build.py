"""-m gpu: the batched weight-image build (fc_x6_weight_images: zero pass, streaming amax pass over the entries that own a slot, image
pass) against the single-image entry point fc_x6_weight_image, which keeps its own kernels — amax slots by bit pattern, planes 0 and 1
of every unit `torch.equal` — on descriptor sets whose entries are 1, U - 1, U, U + 1 and 2 U + 1 units long (U = fc_x6_amax_units,
the units one block of the amax pass folds), with and without a backward-data sibling; and one executor case: three TrainStep calls
give the same bits whoever waits for the images (executor.IMAGE_WAIT) and wherever they were built."""
import contextlib
import functools

import pytest
import torch

import fcaf3d_amd._lib as L
import fcaf3d_amd.functional as Fn
from fcaf3d_amd import executor as E
from fcaf3d_amd.weight_images import WeightImages

pytestmark = pytest.mark.gpu
UNIT = 2048                                   # weights per image unit (32 rows x 64 columns)
AMAX_WORD, SUB, STRIDE = 2048, 32, 16         # csrc/conv_x6.h X6_IMG_AMAX_WORD; csrc/fc_common.h FC_AMAX_SUB, FC_AMAX_STRIDE
PLANTS = ('first', 'last', 'chunk_end', 'next_chunk', 'tail')


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _shapes():
    """(K, Cin, Cout) of a set: a unit is 2 048 weights, an entry has K (R / 32) (C / 64) of them"""
    U = L.query('fc_x6_amax_units')
    assert U >= 4 and U % 2 == 0
    lone = [(n, 32, 64) for n in (1, U - 1, U, U + 1, 2 * U + 1)]            # forward only: (64, 32) has no image
    lone_t = [(3, 64, 32), (U + 1, 64, 32)]                                     # backward-data only, with a slot of its own
    paired = [(U // 2, 64, 64), (U // 2 + 1, 64, 64), (27, 64, 64), (1, 64, 128), (27, 128, 64), (1, 128, 64)]      # U, U + 2, 54, 4, 108, 4 units each way
    return U, [lone[0], paired[0], lone[1], lone_t[0], paired[1], lone[2], paired[2], lone[3], paired[3], lone_t[1], lone[4], paired[4], paired[5]]


def _plant_at(kind, n, U):
    """the flat index of the planted element in a kernel of n weights (None: this kernel has no such place)"""
    chunk = U * UNIT
    if kind == 'first':
        return 0
    if kind == 'last':
        return n - 1
    if kind == 'chunk_end':
        return chunk - 1 if n >= chunk else None
    if kind == 'next_chunk':
        return chunk if n > chunk else None
    full = n // chunk * chunk                    # 'tail': inside the short last chunk
    return full + (n - full) // 2 if n > full else None


def _weights(kind, offset, dev):
    """the kernels of a set, each a contiguous view `offset` floats into a buffer of its own (torch allocates at 512-byte boundaries)"""
    U, shapes = _shapes()
    g = torch.Generator().manual_seed(1234)
    ws = []
    for i, (K, R, C) in enumerate(shapes):
        n = K * R * C
        x = torch.rand(n, generator=g) * 2 - 1
        if kind == 'zeros':
            x.zero_()
        else:
            at = _plant_at(kind if kind in PLANTS else PLANTS[i % len(PLANTS)], n, U)
            if at is not None:
                x[at] = 3.0 if i % 2 else -3.0
            if kind == 'nonfinite':
                x[(7 * i + 1) % n], x[(n // 2 + 3) % n], x[n - 2] = float('inf'), float('nan'), float('-inf')
        buf = torch.empty(n + 4, dtype=torch.float32, device=dev)
        w = buf[offset:offset + n].view(K, R, C)
        w.copy_(x.view(K, R, C))
        assert w.is_contiguous() and w.data_ptr() % 16 == 4 * offset
        ws.append(w)
    return ws


def _slot(img):
    return img.view(torch.int32)[AMAX_WORD:AMAX_WORD + SUB * STRIDE:STRIDE]


def _planes01(img):
    return img.view(-1, 3, 4096)[:, :2]          # per (k, slab, group) block: three planes of 64 rows x 64 bytes


def _host_amax_bits(w):
    a = w.detach().abs().flatten()
    a = a[torch.isfinite(a)]
    return int(a.max().view(torch.int32)) if a.numel() else 0


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'element_path'])
@pytest.mark.parametrize('kind', PLANTS + ('nonfinite', 'zeros'))
def test_batched_build_equals_the_single_image_entry_point(kind, offset):
    dev = _dev()
    assert L.lib().fc_get_split_mode() == 2
    ws = _weights(kind, offset, dev)
    im = WeightImages(ws)
    U = im.amax_units
    n_fwd = sum(1 for w in ws if im.table[(w.data_ptr(), *w.shape)][0] is not None)
    n_sib = sum(1 for w in ws if None not in im.table[(w.data_ptr(), *w.shape)])
    assert n_fwd == 11 and n_sib == 6 and im.n == len(ws) + n_sib
    # the amax grid: one block per chunk of U units of every entry that owns its slot, none for an entry with a sibling
    # (every kernel here has exactly one such entry: its forward image, or its backward-data image where there is no forward one)
    assert im.amax_blocks == sum(-(-(w.numel() // UNIT) // U) for w in ws)
    im.buf.fill_(0x5a)                            # stale bytes everywhere, the slots included
    im.build()
    torch.cuda.synchronize()
    for w in ws:
        K, R, C = w.shape
        fwd, bwd = im.table[(w.data_ptr(), K, R, C)]
        want = _host_amax_bits(w)
        if kind == 'zeros':
            assert want == 0
        elif kind != 'nonfinite' and _plant_at(kind, w.numel(), U) is not None:
            assert want == 0x40400000            # 3.0
        owner = fwd if fwd is not None else bwd
        assert int(_slot(owner).max()) == want, (K, R, C, hex(int(_slot(owner).max())), hex(want))
        if fwd is not None and bwd is not None:
            assert int(_slot(bwd)[0]) == want, 'a backward-data image carries its sibling\'s amax in sub-word 0'
        for tr, img, (r, c) in ((0, fwd, (R, C)), (1, bwd, (C, R))):
            if img is None:
                continue
            ref = torch.full_like(img, 0xa5)
            L.call('fc_x6_weight_image', L.ptr(w), L.ptr(ref), K, r, c, tr, L.stream())
            torch.cuda.synchronize()
            assert int(_slot(ref).max()) == want
            assert torch.equal(_planes01(img), _planes01(ref)), (kind, offset, K, R, C, tr)


# ---- the executor: who waits for the images, and where they were built ----------------------------------------------------------
@contextlib.contextmanager
def _streams_of_builds(dev):
    log, orig, side = [], L.call, Fn.wgrad_stream(dev).cuda_stream

    def logging_call(name, *a):
        if name == 'fc_x6_weight_images':
            log.append('side' if a[-1] == side else 'main')
        return orig(name, *a)
    L.call = logging_call
    try:
        yield log
    finally:
        L.call = orig


@functools.lru_cache(None)
def _three_steps(image_wait, build_on_main):
    """losses and parameters after three TrainStep calls on the smallest training case of tests/test_gpu_exec.py (two levels, one
    scene of 30 000 points, weight gradients on their stream), from one seed"""
    from fcaf3d_amd.runner import TrainStep
    from tests.test_gpu_exec import _batch, _build
    dev = _dev()
    batch = _batch((81,), dev)
    old = E.IMAGE_WAIT, E.ENABLED, Fn.WGRAD_ASYNC
    E.IMAGE_WAIT, E.ENABLED, Fn.WGRAD_ASYNC = image_wait, True, True
    try:
        model, cfg = _build(levels=2)
        model = model.to(dev).train()
        model.async_maps = True
        tr = TrainStep.from_config(model, cfg)
        losses = []
        with _streams_of_builds(dev) as log:
            for _ in range(3):
                if build_on_main:
                    torch.cuda.synchronize()      # (the build of the last step's close has ended: two builds never write the buffer at once)
                    tr.invalidate_images()        # nobody may believe the images: this step's `ensure` builds them, on the main stream
                losses.append(float(tr(batch)[0]))
        torch.cuda.synchronize()
        prog = E.program_for(model, True)
        assert prog is not None and prog.img_pair == (image_wait == 'first_reader')
        return losses, {k: p.detach().clone() for k, p in model.named_parameters()}, tuple(log)
    finally:
        E.IMAGE_WAIT, E.ENABLED, Fn.WGRAD_ASYNC = old


def test_three_steps_give_the_same_bits_whoever_waits_for_the_images():
    first, entry, on_main = _three_steps('first_reader', False), _three_steps('entry', False), _three_steps('first_reader', True)
    print('losses', first[0], entry[0], on_main[0])
    # the first step builds on the main stream (nothing was built yet), every step's close on the weight-gradient stream
    assert first[2] == entry[2] == ('main', 'side', 'side', 'side')
    assert on_main[2] == ('main', 'side') * 3
    for other in (entry, on_main):
        assert other[0] == first[0]
        assert other[1].keys() == first[1].keys()
        for k, v in first[1].items():
            assert torch.equal(other[1][k], v), k
