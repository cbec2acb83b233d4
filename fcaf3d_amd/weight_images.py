"""The pre-split weight images of the matrix-pipe convolutions (csrc/conv_x6.h): the buffer (`WeightImages`) and its one owner
(`ImageSet`), the only place that knows when images may be read without a rebuild."""
import contextlib

import torch

from . import _lib as L


class WeightImages:
    """Pre-split images (csrc/conv_x6.h) of every convolution kernel of a model, forward and backward-data, built by ONE
    launch — for a training loop that knows when the weights change (runner.TrainStep builds them right after the optimizer
    step, on the weight-gradient stream, and hands them to the next step under `ImageSet.lease`).  Kernels that reach
    `sparse_conv` as a fresh tensor (the transposed convolution's permuted copy) are not covered and build their own."""

    def __init__(self, weights):
        ents, off = [], 0
        self.table = {}
        dev = None
        for w in weights:
            if w.dim() == 2:                       # 1 x 1 convolution: (Cin, Cout), used as (1, Cin, Cout)
                K, (Cin, Cout) = 1, w.shape
            else:
                K, Cin, Cout = w.shape
            dev = w.device
            pair = [None, None]
            for tr, (R, C) in ((0, (Cin, Cout)), (1, (Cout, Cin))):
                if R % 32 or C % 64 or not w.is_contiguous():
                    continue
                nbytes = L.query('fc_x6_weight_image_bytes', K, R, C)
                pair[tr] = (off, nbytes, K, R, C)
                off += (nbytes + 255) // 256 * 256
            if pair[0] or pair[1]:
                ents.append((w, pair))
        self.n = 0
        self.event = None
        if not ents:
            return
        self.buf = torch.empty(off, dtype=torch.uint8, device=dev)
        desc, blk = [], 0
        for w, pair in ents:
            views = []
            for tr in (0, 1):
                if pair[tr] is None:
                    views.append(None)
                    continue
                o, nb, K, R, C = pair[tr]
                v = self.buf[o:o + nb]
                views.append(v)
                # word 7 (h3 split): a backward-data image shares the amax slot of its forward image (the same weights): no second pass
                desc += [w.data_ptr(), v.data_ptr(), K, R, C, tr, blk, views[0].data_ptr() if (tr == 1 and views[0] is not None) else 0]
                blk += K * (R // 32) * (C // 64)
            K = 1 if w.dim() == 2 else w.shape[0]
            self.table[(w.data_ptr(), K, w.shape[-2], w.shape[-1])] = tuple(views)
        self.n = len(desc) // 8
        self.blocks = blk
        self.desc = torch.tensor(desc, dtype=torch.int64).to(dev)
        # the amax pass's own grid (csrc/conv_x6.h k_x6_weight_amax): one block per chunk of U units of every entry that owns its slot
        # (word 7 == 0), as entry << 32 | chunk; made once, here
        self.amax_units = U = L.query('fc_x6_amax_units')
        chunks = [e << 32 | c for e in range(self.n) if desc[8 * e + 7] == 0
                  for c in range(-(-(desc[8 * e + 2] * (desc[8 * e + 3] // 32) * (desc[8 * e + 4] // 64)) // U))]
        self.amax_blocks = len(chunks)
        self.amax_chunks = torch.tensor(chunks, dtype=torch.int64).to(dev)

    def build(self):
        """enqueue the build on the CURRENT stream; records the event consumers on other streams wait for"""
        if self.n:
            L.call('fc_x6_weight_images', L.ptr(self.desc), self.n, self.blocks, L.ptr(self.amax_chunks), self.amax_blocks, L.stream())
            self.event = torch.cuda.Event()
            self.event.record()


class ImageSet:
    """A `WeightImages` buffer, the parameters it is made from, and whether it is still good.
    THE RULE.  The images are used without a rebuild iff `built` equals the current key AND the caller holds the lease, or the
    detector is in eval mode with `static_weights`; otherwise they are rebuilt on the current stream before use.
    `built` is all the freshness state there is: None, or the key the images were built under — (sum of the sources' `_version`,
    functional.split_mode()).  A write through a torch op moves the sum, a switch of the operand split the mode; `invalidate()` is
    for a write through `.data` or a raw pointer, which moves no `_version` (the blind spot: torch's fused optimizers write that way
    too).  Hence the lease: only the loop that makes every such write itself (runner.TrainStep: its optimizer step, then
    `rebuild_after_step`) takes it, for one forward + backward pass; anybody else's pass rebuilds.  weights (default: the sources):
    the tensors the images are cut from, where `prepare()` packs copies of the sources."""
    held = None                     # the set whose lease is held now: at most one per process

    def __init__(self, sources, weights=None):
        self.sources = list(sources)
        self.images = WeightImages(self.sources if weights is None else weights)
        self.built = None
        self._built_on = None       # the raw stream of the last build
        self._first = False         # under a lease: no per-operator consumer has waited for the build yet

    def key(self):
        from . import functional as Fn             # (functional imports this module)
        return sum(p._version for p in self.sources), Fn.split_mode()

    def prepare(self):
        """what a build enqueues before the launch (the executor packs its copies here)"""

    def _launch(self):
        """everything a build enqueues, on the current stream (the one place: a test counts builds by replacing it)"""
        self.prepare()
        self.images.build()
        self._built_on = L.stream()

    def invalidate(self):
        self.built = None

    def ensure(self, trusted):
        """build on the current stream unless the images are current and the caller may believe it -> whether it built"""
        key = self.key()
        if trusted and self.built == key:
            return False
        self._launch()
        self.built = key
        return True

    def rebuild_after_step(self, main, side):
        """after an optimizer step enqueued on `main` (as every reader of the old images is): build on `side`"""
        side.wait_stream(main)
        with torch.cuda.stream(side):
            self._launch()
        self.built = self.key()

    def wait(self):
        """the current stream waits for the last build, if that was enqueued on another one"""
        if self.images.event is not None and self._built_on != L.stream():
            torch.cuda.current_stream().wait_event(self.images.event)

    def lookup(self, weight, transposed):
        """-> the image of a (K, Cin, Cout) kernel or None, for `_x6_image` under this set's lease; the first consumer waits"""
        pre = self.images.table.get((weight.data_ptr(), *weight.shape))
        if pre is None or pre[transposed] is None:
            return None
        if self._first:
            self._first = False
            self.wait()
        return pre[transposed]

    @contextlib.contextmanager
    def lease(self):
        """for the block this set is the one NetProgram.forward trusts and `_x6_image` consults; an exception withdraws it too"""
        assert ImageSet.held is None, 'a weight-image lease is already held: one step at a time'
        ImageSet.held, self._first = self, True
        try:
            yield self
        finally:
            ImageSet.held = None
