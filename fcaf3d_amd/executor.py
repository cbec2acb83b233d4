"""The network body (MEResNet3D backbone + Fcaf3DNeckWithHead.forward) as a STATIC operator list walked by the native executor
(csrc/exec.hip: one C-ABI call per direction) instead of ~1 000 Python-dispatched launches per step.

r4 (profiles/r4_hostprof.txt): the training step was host-bound at every batch size (16.7 ms of Python per step at 2 scenes per
GPU, 20.3 ms at 8).  The operator sequence of `SingleStageSparse3DDetector.extract_feat` (single_stage_sparse.py:43-50;
me_resnet.py:43-50; fcaf3d_neck_with_head.py:94-108, :256-279) is fixed by the module graph; only row counts and addresses change
from step to step.  `NetProgram` walks the module graph ONCE and emits

  * forward operators  — the entry points `nn.py` / `functional.py` would call, in the same order, with the same arguments;
  * backward operators — what torch.autograd would replay over them (backward-data, weight gradients on their own stream,
    normalisation backward, gradient accumulation where a tensor has two consumers), gradients written straight into the flat
    gradient buffer (flat.FlatParams) or a buffer of the same layout;

as rows of int64 (the fields of every operator, by name: csrc/exec_ops.h).  Operands are indices into three host tables refreshed per step with
a few vectorised numpy operations: `addr` (device addresses: arena tensors = base + aligned prefix sum of rows x bytes per row;
parameters, buffers, weight images: static), `dims` (row counts) and `maps` (KernelMap.desc()).

Parameter gradients are delivered by `backward()` into `p.grad` (views of the gradient buffer; accumulated into if gradients
are already there); `torch.autograd.grad(loss, parameters)` does not see the parameters behind the single autograd node of the
body — use the module path (FC_EXEC=0) for that.

The module path stays the general route (and the cross-check of the tests: forward bit for bit, gradients to rounding): the
program covers BasicBlock backbones (depth 14 / 18 / 34) with the FCAF3D neck when no pruning bites (`plan_maps` succeeded), the
split-bf16 convolution route (FC_X6=1) and heads of at most 64 fused columns; anything else falls back.
"""
import operator
import os
import struct

import numpy as np
import torch

from . import _lib as L
from . import functional as Fn
from . import nn as MEnn
from .weight_images import ImageSet

ENABLED = os.environ.get('FC_EXEC', '1') != '0'
# bench.py's live roofline measurement: a list -> every step bound while it is set has its convolution operators bracketed by
# HIP events inside fc_exec (csrc/exec.hip, cfg[2]) and appends {pairs per kernel map (device scalars), operators per direction}
PROBE = None
# tests: keep the bound state of the last forward pass on the detector (`det._last_exec = (program, state)`) so that the recorded
# activations can be inspected (NetProgram.decisions).  A program built while it is set also stores the stem's normalised output,
# which a plain step never materialises (r7): part of the program cache key
KEEP_STATE = False


def _layouts():
    """csrc/exec_ops.h -> ({OP_*, OPW, MAPW, ROW_OP, ROW_STREAM: value}, {opcode: {field: (word, stored as index + 1)}}): operator OP_X's fields are the
    enum X_<FIELD> ... X_END, a field's name here is <field> in lower case without the _P1 that marks the index + 1 coding"""
    names, fields = {}, {}
    for block in L.parse_enums():
        names.update(block)
        *members, end = block
        op = names.get('OP_' + end[:-len('_END')]) if end.endswith('_END') else None
        if op is not None:
            fields[op] = {n[len(end) - 3:].lower().removesuffix('_p1'): (block[n], n.endswith('_P1')) for n in members}
    return {k: v for k, v in names.items() if k.startswith('OP_') or k in ('OPW', 'MAPW', 'ROW_OP', 'ROW_STREAM')}, fields


_NAMES, FIELDS = _layouts()
globals().update(_NAMES)         # OP_STEM_FWD ... OP_INV_ROWS, OPW, MAPW, ROW_OP, ROW_STREAM


def word(op, field):
    """the column of `field` in the rows of operator `op` (program build, tests; nothing per step looks a name up)"""
    return FIELDS[op][field][0]


ALIGN = 256
S_MAIN, S_HEAD, S_WGRAD = 0, 1, 2
EV_FORK, EV_HEAD_DONE, EV_W0, EV_W1, EV_WEND, EV_BWD0, EV_IMG, EV_HB = 0, 8, 9, 10, 11, 12, 13, 16       # EV_FORK + level, EV_HB + level
# Who waits for the weight images that runner.TrainStep builds on the weight-gradient stream after the optimizer step (DESIGN.md
# section 6a): 'first_reader' — a training program with `wgrad_async` carries a record on S_WGRAD / wait on S_MAIN of EV_IMG behind the
# stem's operators, which read no image, and NetProgram.forward leaves the host-side wait out; 'entry' — the main stream waits
# before the program's first operator (every other program does, whatever this says).  Part of the program cache key.
# FC_IMAGE_WAIT=entry: the A/B run of the benchmark.
IMAGE_WAIT = os.environ.get('FC_IMAGE_WAIT', 'first_reader')


def _f(x):
    """a float immediate: the bit pattern of a double in an int64 word"""
    return struct.unpack('<q', struct.pack('<d', float(x)))[0]


def supported(det):
    bb, nh = det.backbone, det.neck_with_head
    if not (ENABLED and Fn.X6 and not (Fn.FLAGS & Fn.CONV_FMA) and Fn.STEM_COL and Fn.DGRAD_WT):
        return False
    if getattr(bb.BLOCK, 'expansion', 1) != 1 or det.spatial_sort:
        return False
    if 1 + nh.n_reg_outs + nh.n_classes > 64 or bb.conv1[0].in_channels != 3:
        return False
    return type(nh).forward_single is _FORWARD_SINGLE and type(nh).forward is _NECK_FORWARD


_FORWARD_SINGLE = _NECK_FORWARD = None       # set by fcaf3d_neck_with_head at import: a subclass that overrides them falls back


class NetProgram:
    def __init__(self, det, training, wgrad_async, head_overlap, tail0=False, keep_state=None, frozen=-1, plan=None, image_wait='entry'):
        """frozen: the backbone's frozen prefix of a training program (`frontier`: -1 none, 0 the stem, k the stem and layer1 .. layerk).
        plan: the verdict of `freeze_plan` this program was asked for (None: `frozen`).  Either only NAMES the program: what a layer
        emits is read from its own flags as they are now (its kernel's requires_grad, its BatchNorm's mode), which the caller has checked
        against the verdict.
        keep_state (default: the module's KEEP_STATE now): the stem's normalised output is stored for `decisions`.
        tail0: the finest neck level is PRUNED this step (`pts_threshold` bites there, fcaf3d_neck_with_head.py:110-126): the
        program ends at that level's union — `x0`, exported as a fourth differentiable output — and `_prune` + out_block_0 +
        forward_single of level 0 run on the per-operator path, attached by autograd (single_stage_sparse._exec_forward)"""
        self.det = det
        self.tail0 = tail0
        self.keep_state = bool(KEEP_STATE if keep_state is None else keep_state)
        self.training = training
        self.frozen = int(frozen) if training else -1
        self.plan = plan if training else None
        self.wgrad_async = wgrad_async and training
        # image_wait: who waits for a weight-image build on stream 2 (IMAGE_WAIT above; `program_for` hands the switch in, a program
        # built directly is the 'entry' one unless asked)
        assert image_wait in ('first_reader', 'entry')
        self.image_wait = image_wait if self.wgrad_async else 'entry'
        self.img_pair = False       # ops_f carries the EV_IMG pair: the program itself waits for a build on its stream 2
        bb, nh = det.backbone, det.neck_with_head
        self.nl = min(bb.n_outs, 4)
        self.head_overlap = head_overlap and self.nl > 1
        self.dev = next(det.parameters()).device
        self.ops_f, self.ops_b = [], []
        self.n_addr = 0
        self.static = []            # (addr index, address)
        self.arena = {'f': [], 'b': []}     # (addr index, dims index of the row count, bytes per row, extra bytes)
        self.alias = []             # (addr index, parent addr index, dims index of the row offset, bytes per row)
        self.dyn = {}               # name -> addr index
        self.dim_names = {}
        self.map_names = {}
        self.grad_refs = []         # (addr index, float offset into the gradient buffer)
        self.keep = []              # tensors that must outlive the program build (persistent buffers)
        # what the walk records for the runtime, each a (tensor, rows dim, C) unless said otherwise
        self.relu_outs = []         # every fused norm + ReLU output, forward order (decisions)
        self.pool_arg = None        # the stem pool's arg-max rows (decisions)
        self.out_idx = None         # (cent_all, bbox_all, cls_all, cmax_all): the tensors of all head locations
        self.gout_idx = self.x0_idx = ()        # training: the dyn indices of the three loss gradients; tail0: the finest level's union
        self.in_sums = None         # training: the stem instance norm's (B, 2 x 64) d beta / d gamma sums (backward arena)
        self.small = []             # normalisation layers in BACKWARD emission order: (sums address | None, nseg dim | None, C, weight, bias)
        self._pready = {}           # id(parameter) -> number of backward operators after which its gradient is final
        self._params = [p for p in det.parameters() if p.requires_grad]
        self._goff, off = {}, 0
        flat = getattr(self._params[0], '_fc_flat', None)
        self.flat = flat[0] if flat is not None else None
        for p in self._params:
            if self.flat is not None:
                assert p._fc_flat[0] is self.flat
                self._goff[id(p)] = p._fc_flat[1]
            else:
                self._goff[id(p)] = off
                off += -(-p.numel() // 64) * 64
        self._gtotal = self.flat.n if self.flat is not None else off
        self._sig = self.signature(det)
        self._build_weights()
        self._build(_Emitter(self))
        self._finalise()

    @staticmethod
    def signature(det):
        """what the program's static address table depends on: cheap to compare per step (parameters are re-pointed only by
        flat.FlatParams and by nn.Module._apply, which drops the detector's programs)"""
        from .flat import GENERATION
        return GENERATION[0]

    # ---- tables ------------------------------------------------------------------------------------------------------
    def _new(self):
        self.n_addr += 1
        return self.n_addr - 1

    def D(self, name):
        if name not in self.dim_names:
            self.dim_names[name] = len(self.dim_names)
        return self.dim_names[name]

    def M(self, name):
        if name not in self.map_names:
            self.map_names[name] = len(self.map_names)
        return self.map_names[name]

    def T(self, rows, cols, arena='f', elem=4, extra=0):
        i = self._new()
        self.arena[arena].append((i, self.D(rows), cols * elem, extra))
        return i

    def S(self, tensor):
        """a static address: parameter data, module buffer, persistent scratch"""
        i = self._new()
        self.static.append((i, tensor.data_ptr()))
        self.keep.append(tensor)
        return i

    def SA(self, address):
        i = self._new()
        self.static.append((i, int(address)))
        return i

    def DY(self, name):
        if name not in self.dyn:
            self.dyn[name] = self._new()
        return self.dyn[name]

    def AL(self, parent, off_dim, cols, elem=4):
        i = self._new()
        self.alias.append((i, parent, self.D(off_dim), cols * elem))
        return i

    def G(self, p):
        i = self._new()
        self.grad_refs.append((i, self._goff[id(p)]))
        return i

    def emit(self, lst, op, stream, **fields):
        """append a row of operator `op`: its fields by name (csrc/exec_ops.h), the others 0"""
        row = [0] * OPW
        row[ROW_OP], row[ROW_STREAM] = op, stream
        self.patch(row, **fields)
        lst.append(row)

    @staticmethod
    def patch(row, **fields):
        """set fields of an emitted row.  A field the header declares ..._P1 takes the plain index (-1: none) and is stored + 1"""
        layout = FIELDS[row[ROW_OP]]
        for k, v in fields.items():
            if k not in layout:
                raise KeyError(f'operator {row[ROW_OP]} has no field {k!r}')
            w, p1 = layout[k]
            row[w] = v + 1 if p1 else v

    # ---- weights: pre-split images of every kernel, incl. the packed head kernel and the generative convolutions' GEMM form; ONE
    # set per detector, shared by its programs (training / inference, stream configurations, pruned-tail variant)
    def _build_weights(self):
        holder = self.det.__dict__.get('_exec_weights')
        if holder is None or holder.sig != self._sig:
            holder = self.det.__dict__['_exec_weights'] = _Weights(self.det, self.dev, self._sig)
        self.w = holder
        self.packed, self.gent_w, self.gents, self.ncol = holder.packed, holder.gent_w, holder.gents, holder.ncol

    def IMG(self, w, transposed):
        v = self.w.images.table.get((w.data_ptr(), 1 if w.dim() == 2 else w.shape[0], w.shape[-2], w.shape[-1]))
        assert v is not None and v[1 if transposed else 0] is not None, 'no split-bf16 image for this kernel shape'
        return self.S(v[1 if transposed else 0])

    # ---- program ---------------------------------------------------------------------------------------------------------
    def _build(self, em):
        """the network as `extract_feat` runs it (me_resnet.py:14-50; fcaf3d_neck_with_head.py:94-108, :256-279): stem, backbone
        levels, then neck level i and the head of level i from the coarsest down; last the backward schedule"""
        bb, nh = self.det.backbone, self.det.neck_with_head
        x = em.stem(bb.conv1[0], bb.conv1[1])
        if self.image_wait == 'first_reader':
            # the stem's three operators read the fp32 kernel and no image: the main stream joins the build (enqueued on stream 2 by
            # ImageSet.rebuild_after_step) here, in front of the first operator with an image word
            em.sync(self.ops_f, S_WGRAD, S_MAIN, EV_IMG)
            self.img_pair = True
        levels = []
        for li in range(1, self.nl + 1):
            x = em.level(li, getattr(bb, f'layer{li}'), x)
            levels.append(x)
        self.out_idx = (self.T('Nall', 1), self.T('Nall', nh.n_reg_outs), self.T('Nall', nh.n_classes), self.T('Nall', 1))
        if self.training:
            em.tape.append(lambda: em.flush_small(S_MAIN))               # reversed walk: reached after the whole neck's backward
            self.gout_idx = (self.DY('g_cent'), self.DY('g_bbox'), self.DY('g_cls'))
        for i in range(self.nl - 1, -1, -1):
            if i < self.nl - 1:
                x = em.up(i, getattr(nh, f'up_block_{i + 1}'), x, levels[i])
            if i == 0 and self.tail0:
                self.x0_idx = x                             # the pruned level's tail runs outside the program
                if self.training and x[0] in em.needs:
                    em.grads.arrive(x[0], self.DY('g_x0'), *x[1:], S_MAIN)       # ... and hands back d loss / d x0
            else:
                em.head(i, getattr(nh, f'out_block_{i}'), x)
        if self.head_overlap:
            em.sync(self.ops_f, S_HEAD, S_MAIN, EV_HEAD_DONE)
        em.backward()

    # ---- per-step tables ---------------------------------------------------------------------------------------------------
    def _finalise(self):
        self.ops_f = np.ascontiguousarray(np.asarray(self.ops_f, dtype=np.int64).reshape(-1, OPW))
        self.ops_b = np.ascontiguousarray(np.asarray(self.ops_b, dtype=np.int64).reshape(-1, OPW)) if self.ops_b else np.zeros((0, OPW), np.int64)
        self.addr0 = np.zeros(self.n_addr, dtype=np.int64)
        for i, a in self.static:
            self.addr0[i] = a

        def columns(table, width):
            return tuple(np.ascontiguousarray(np.array(table, dtype=np.int64).reshape(-1, width).T))
        self._ar = {k: columns(a, 4) for k, a in self.arena.items()}
        self._al = columns(self.alias, 4)
        self._gr = columns([(i, 4 * off) for i, off in self.grad_refs], 2)
        self.n_dims, self.n_maps = len(self.dim_names), len(self.map_names)
        self._ws = [None, None, None]
        self._need = np.zeros(3, dtype=np.int64)
        self._cfg = np.array([Fn.BN_SMALL_ELEMS, Fn.FLAGS, 0, 0], dtype=np.int64)
        self.n_conv_f = int((self.ops_f[:, ROW_OP] == OP_CONV).sum())
        self.n_conv_b = int((self.ops_b[:, ROW_OP] == OP_CONV).sum()) if len(self.ops_b) else 0
        self.n_amax = int((self.ops_f[:, ROW_OP] == OP_AMAX).sum()) + (int((self.ops_b[:, ROW_OP] == OP_AMAX).sum()) if len(self.ops_b) else 0)
        self._anchor = torch.zeros(1, device=self.dev, requires_grad=True)
        if self.training:
            # small-gradient descriptor template: (src, dst, C, nseg, stride, 0, 0, 0) per (bias, weight) of every normalisation layer
            n = len(self.small)
            self._small = np.zeros((2 * n, 8), dtype=np.int64)
            self._small_goff = np.zeros(2 * n, dtype=np.int64)
            self._small_in = None
            for k, (src, nseg, C, w, b) in enumerate(self.small):
                for h, p in ((0, b), (1, w)):          # sums[0] = d beta, sums[1] = d gamma
                    r = 2 * k + h
                    self._small[r, 2], self._small[r, 3], self._small[r, 4] = C, 1, 2 * C
                    self._small_goff[r] = self._goff[id(p)] * 4
                    if src is not None:
                        self._small[r, 0] = src + 4 * C * h
                    else:
                        self._small_in = (2 * k, C)

    def _fill_arena(self, addr, dims, which, base):
        idx, di, bpr, ext = self._ar[which]
        if len(idx) == 0:
            return
        sizes = (dims[di] * bpr + ext + (ALIGN - 1)) // ALIGN * ALIGN
        offs = np.cumsum(sizes) - sizes
        addr[idx] = base + offs

    def _arena_bytes(self, dims, which):
        idx, di, bpr, ext = self._ar[which]
        return int(((dims[di] * bpr + ext + (ALIGN - 1)) // ALIGN * ALIGN).sum()) + ALIGN

    def bind(self, x, batch_size, backward):
        """per-step tables from the input SparseTensor's coordinate maps (all cached lookups after plan_maps); None if this
        step's maps do not fit the program (a union that is not the generated set)"""
        nl = self.nl
        cm0 = x.cmap
        dims = np.zeros(self.n_dims, dtype=np.int64)
        maps = np.zeros((self.n_maps, MAPW), dtype=np.int64)
        dn, mn, N = self.dim_names, self.map_names, _Names

        def setd(k, v):
            if k in dn:
                dims[dn[k]] = v
        m1 = cm0.strided(2)
        m2 = m1.strided(2)
        maps[mn['stem']] = cm0.kernel_map(m1, 3).desc(conv=False)
        maps[mn['pool']] = m1.kernel_map(m2, 2).desc(conv=False)
        kms = {}
        setd('n0', cm0.n); setd('n1', m1.n); setd('n1w', 2 * m1.n); setd('n2', m2.n); setd('B', batch_size); setd('one', 1)
        prev, lv = m2, []
        for li in range(1, nl + 1):
            mi = prev.strided(2)
            kms[N.down(li)], kms[N.ds(li)], kms[N.same(li)] = prev.kernel_map(mi, 3), prev.kernel_map(mi, 1), mi.kernel_map(mi, 3)
            for k in (N.down(li), N.ds(li), N.same(li)):
                maps[mn[k]] = kms[k].desc(True, backward)
            setd(N.rows(li), mi.n)
            lv.append(mi)
            prev = mi
        xm = lv[-1]
        head_maps = [xm]
        dyn = {}
        for i in range(nl - 2, -1, -1):
            g = xm.generate()
            u, rows, swapped = lv[i].union(g)
            if not swapped or u is not g:
                return None
            kms[N.gsame(i)] = g.kernel_map(g, 3)
            maps[mn[N.gsame(i)]] = kms[N.gsame(i)].desc(True, backward)
            setd(N.gen(i), g.n)
            dyn[N.union(i)] = rows
            xm = g
            head_maps.append(g)
        head_maps = head_maps[::-1]                       # finest first
        off = 0
        for i, cm in enumerate(head_maps):
            if i == 0 and self.tail0:
                continue                                  # (its head outputs come from the per-operator tail)
            setd(N.off(i), off)
            off += cm.n
        setd('Nall', off)
        st = dict(dims=dims, maps=maps, dyn=dyn, head_maps=head_maps, x=x, seg1=m1.coords, n_all=off)
        if PROBE is not None:
            # valid (input, output) pairs of every map, as device scalars (read back after the timed region): the FLOPs of a launch
            from .sparse import _rec
            st['pairs'] = {mn[k]: _rec(km._pairs[3].sum() if km._pairs is not None else (km.nbr >= 0).sum()) for k, km in kms.items()}
            PROBE.append(dict(pairs=st['pairs'], nf=self.n_conv_f, nb=self.n_conv_b, na=self.n_amax))
        return st

    def _streams(self):
        dev = self.dev
        nh = self.det.neck_with_head
        main = L.stream()
        head = nh._head_stream(dev).cuda_stream if self.head_overlap else main
        wg = Fn.wgrad_stream(dev).cuda_stream if self.wgrad_async else main
        return np.array([main, head, wg], dtype=np.int64)

    def _run(self, ops, addr, st, begin=0, end=None, size_only=False):
        """size_only: the sizing pass alone (cfg[3]) — grows the scratch buffers to what [begin, end) needs and launches nothing.
        The segmented data-parallel backward sizes its WHOLE list first: a buffer replaced between two segments would go back to
        the caching allocator while kernels of an earlier segment on the head / weight-gradient stream still use it"""
        streams = self._streams()
        self._cfg[2] = 1 if 'pairs' in st else 0
        self._cfg[3] = 1 if size_only else 0
        end = len(ops) if end is None else end
        while True:
            ws = np.array([w.data_ptr() if w is not None else 0 for w in self._ws], dtype=np.int64)
            wsb = np.array([w.numel() if w is not None else 0 for w in self._ws], dtype=np.int64)
            rc = L.lib().fc_exec(ops.ctypes.data, begin, end, addr.ctypes.data, st['dims'].ctypes.data, st['maps'].ctypes.data,
                                 streams.ctypes.data, ws.ctypes.data, wsb.ctypes.data, self._need.ctypes.data, self._cfg.ctypes.data)
            if rc == -2:                                  # nothing was launched: grow the scratch buffers and go again
                for i in range(3):
                    if self._need[i] > wsb[i]:
                        self._ws[i] = torch.empty(int(self._need[i] * 5 // 4) + (1 << 20), dtype=torch.uint8, device=self.dev)
                continue
            if rc != 0:
                raise RuntimeError(f'fc_exec failed: {"invalid argument" if rc == -1 else "hipError %d" % rc}')
            return

    def decisions(self, st):
        """(ReLU sign patterns in forward order, max-pool arg-max rows) of the forward pass bound in `st` — what
        oracle.DecisionTape replays (test infrastructure reads it; needs KEEP_STATE)"""
        assert self.keep_state, 'this program does not store the stem\'s normalised output: build it under executor.KEEP_STATE'
        relu = [(self._view(st, *t) > 0).cpu() for t in self.relu_outs]
        return relu, self._view(st, *self.pool_arg, torch.int32).cpu()

    def _view(self, st, idx, rows, C, dtype=torch.float32):
        """the (rows, C) view of forward-arena tensor `idx` in this step's state"""
        fa, n = st['fa'], int(st['dims'][self.dim_names[rows]])
        o = int(st['addr'][idx] - fa.data_ptr())
        return fa[o:o + n * C * 4].view(dtype).view(n, C)

    def forward(self, st):
        """-> (cent_all, bbox_all, cls_all, cmax_all) for all head locations (levels finest first), autograd-connected in training"""
        # the previous call's images are believed only under runner.TrainStep's lease or, in eval mode, a detector's `static_weights`
        self.w.ensure(trusted=ImageSet.held is self.w or (not self.training and getattr(self.det, 'static_weights', False)))
        # they may have been built on another stream (runner: after the optimizer step).  A build on the weight-gradient stream is waited
        # for by the program's own EV_IMG pair, behind the stem (IMAGE_WAIT); any other build by the main stream, here
        if not (self.img_pair and self.w._built_on == Fn.wgrad_stream(self.dev).cuda_stream):
            self.w.wait()
        if self.training:
            return _NetFn.apply(self._anchor, self, st)
        return self._forward(st)

    def _forward(self, st):
        dims = st['dims']
        fa = torch.empty(self._arena_bytes(dims, 'f'), dtype=torch.uint8, device=self.dev)
        addr = self.addr0.copy()
        base = (fa.data_ptr() + ALIGN - 1) // ALIGN * ALIGN
        self._fill_arena(addr, dims, 'f', base)
        addr[self.dyn['x0']] = st['x'].F.data_ptr()
        addr[self.dyn['seg1']] = st['seg1'].data_ptr()
        for k, t in st['dyn'].items():
            addr[self.dyn[k]] = t.data_ptr()
        ai, ap, ad, ab = self._al
        fwd_alias = addr[ap] != 0                         # aliases of forward tensors (the backward ones are resolved later)
        addr[ai[fwd_alias]] = addr[ap[fwd_alias]] + dims[ad[fwd_alias]] * ab[fwd_alias]
        st['fa'], st['addr'] = fa, addr
        self._run(self.ops_f, addr, st)
        nh = self.det.neck_with_head
        outs = [self._view(st, idx, 'Nall', c) for idx, c in zip(self.out_idx, (1, nh.n_reg_outs, nh.n_classes, 1))]
        if self.tail0:
            outs.append(self._view(st, *self.x0_idx))
        return tuple(outs)

    def _backward(self, st, g_cent, g_bbox, g_cls, g_x0=None):
        dims, addr = st['dims'], st['addr']
        n = st['n_all']
        nh = self.det.neck_with_head
        gs = []
        for g, c in zip((g_cent, g_bbox, g_cls), (1, nh.n_reg_outs, nh.n_classes)):
            gs.append(g.contiguous() if g is not None else torch.zeros((n, c), dtype=torch.float32, device=self.dev))
        if self.tail0:
            t, rows, C = self.x0_idx
            n0 = int(dims[self.dim_names[rows]])
            g_x0 = g_x0.contiguous() if g_x0 is not None else torch.zeros((n0, C), dtype=torch.float32, device=self.dev)
            gs.append(g_x0)                                 # (kept alive until the operators have been enqueued)
        ba = torch.empty(self._arena_bytes(dims, 'b'), dtype=torch.uint8, device=self.dev)
        base = (ba.data_ptr() + ALIGN - 1) // ALIGN * ALIGN
        self._fill_arena(addr, dims, 'b', base)
        for k, g in zip(('g_cent', 'g_bbox', 'g_cls', 'g_x0'), gs):
            if k in self.dyn:                               # (g_x0: only where the union behind the pruned tail needs a gradient)
                addr[self.dyn[k]] = g.data_ptr()
        ai, ap, ad, ab = self._al
        addr[ai] = addr[ap] + dims[ad] * ab
        own = self._own_params()
        # Parameters that already hold a gradient when this pass starts: (a) a few, in tensors of their own — the pruned level's
        # per-operator tail has delivered the head kernels' share before this node ran: the program writes its share into the
        # buffer as always and the earlier one is added there afterwards; (b) views of the very buffer this pass writes (a second
        # backward without zero_grad): then, and without flat storage, the pass writes into a buffer of its own and is added on top
        pre = [(p, p.grad) for p in own if p.grad is not None]
        aliased = self.flat is not None and any(g.data_ptr() == self.flat.grad_view(p).data_ptr() for p, g in pre)
        accum = bool(pre) and (self.flat is None or aliased or len(pre) > 16)
        if self.flat is not None and not accum:
            gbuf = self.flat.grad
        else:
            gbuf = torch.zeros(self._gtotal, dtype=torch.float32, device=self.dev)
        gi, go = self._gr
        addr[gi] = gbuf.data_ptr() + go
        desc = self._small.copy()
        desc[:, 1] = gbuf.data_ptr() + self._small_goff
        if self._small_in is not None:                      # (a frozen stem has no rows in the descriptor)
            r, C = self._small_in
            B = int(dims[self.dim_names['B']])
            desc[r, 0], desc[r + 1, 0] = addr[self.in_sums], addr[self.in_sums] + 4 * C
            desc[r:r + 2, 3] = B
        if 'small_desc' in self.dyn:                         # (a head-only program has no normalisation layer in its backward list)
            desc_dev = L.upload(desc, self.dev)
            addr[self.dyn['small_desc']] = desc_dev.data_ptr()
        gv = self._grad_views(gbuf)
        if not accum:
            for p in own:                                   # before the operators run: a data-parallel bucket may leave mid-way
                p.grad = gv[id(p)]
        from . import dist as D
        av = D.ACTIVE
        if av is not None and av.buckets and av.flat is self.flat and self.flat is not None and not accum and not self.tail0:
            # data parallel: every gradient bucket leaves (all-reduce on the weight-gradient stream) as soon as the operators that
            # write its parameters are enqueued — what the autograd hooks of the per-operator path do
            pos = 0
            self._run(self.ops_b, addr, st, size_only=True)
            for upto in self._bucket_ready(av):
                if upto > pos:
                    self._run(self.ops_b, addr, st, pos, upto)
                    pos = upto
                av.launch_next()
            if pos < len(self.ops_b):
                self._run(self.ops_b, addr, st, pos, len(self.ops_b))
        else:
            self._run(self.ops_b, addr, st)
        if accum:
            for p in own:
                if p.grad is None:
                    p.grad = gv[id(p)]
                else:
                    p.grad.add_(gv[id(p)])
        else:
            for p, g0 in pre:                               # (a): the share that was there first
                gv[id(p)].add_(g0)
            if self.flat is not None and not self.tail0:
                self.flat.complete = True
        st['ba'] = ba                                       # until the caller drops the step state

    def _own_params(self):
        """the parameters whose gradients this program writes (all of them, unless the pruned level's tail runs outside it)"""
        c = getattr(self, '_own', None)
        if c is None:
            c = self._own = [p for p in self._params if id(p) in self._pready]
        return c

    def _bucket_ready(self, av):
        """per bucket of the averager (in launch order): the number of backward operators after which all of its gradients are
        written (non-decreasing: buckets leave strictly in order)"""
        key = id(av)
        c = getattr(self, '_br', None)
        if c is None or c[0] != key:
            out, run = [], 0
            for b in av.buckets:
                run = max(run, max(self._pready[id(p)] for p in b))
                out.append(run)
            c = self._br = (key, out)
        return c[1]

    def _grad_views(self, gbuf):
        key = gbuf.data_ptr()
        cache = getattr(self, '_gv', None)
        if cache is None or cache[0] != key:
            views = {id(p): gbuf[self._goff[id(p)]:self._goff[id(p)] + p.numel()].view(p.shape) for p in self._params}
            cache = self._gv = (key, views, gbuf)
        return cache[1]


class _Names:
    """the names under which the walk registers the per-level row counts (`dim_names`), kernel maps (`map_names`) and bound
    tensors (`dyn`), and under which `bind` fills them in.  li = 1 ..: backbone level, i = 0 ..: neck level (finest first)"""
    rows, down, ds, same = 'L{}'.format, 'down{}'.format, 'ds{}'.format, 'same{}'.format
    gen, gsame, off, union = 'g{}'.format, 'gsame{}'.format, 'off{}'.format, 'rows{}'.format


class _Grads:
    """the gradient ledger of the backward walk: forward tensor -> its gradient (a tensor of the backward arena), from the first
    contribution that arrives to the consumer that takes the sum"""

    def __init__(self, em):
        self.em = em
        self.full = {}                   # forward tensor -> gradient tensor
        self.second = {}                 # forward tensor -> (second contribution, rows, cols, stream), not yet added
        self.behind = {}                 # forward tensor -> (gradient from its head branch on the head stream, level)
        self.src = {}                    # gradient tensor -> (index in ops_b of the backward-data OP_CONV that wrote it, rows, cols, stream)

    def _add(self, t, g, rows, cols, stream):
        em, dst = self.em, self.full[t]
        em.p.emit(em.Bk, OP_ADD, stream, dst=dst, src=g, n=em.p.D(rows), c=cols)
        self.src.pop(dst, None)          # added to in place: no longer the plain result of the convolution that wrote it
        em.amax_of.pop(dst, None)        # ... nor bounded by its producer's amax word

    def arrive(self, t, g, rows, cols, stream):
        """gradient `g` (a backward tensor) arrives for forward tensor t.  The SECOND contribution is kept aside: if the
        consumer of the sum is a BatchNorm backward it adds the two on the fly (norm.hip gy2) and no add pass runs; a third
        arrival, or any other consumer, adds the first two as before (same operands, same order: same bits)"""
        if t not in self.full:
            self.full[t] = g
        elif Fn.BN_FUSE and t not in self.second:
            self.second[t] = (g, rows, cols, stream)
        else:
            self.own(t)                  # (a contribution kept aside goes in first)
            self._add(t, g, rows, cols, stream)

    def take(self, t, rows, cols, pair=False):
        """the complete gradient of forward tensor t, for the emitter of the operator that produced t (main stream); pair:
        the caller adds a second contribution itself -> (gradient, second contribution | None)"""
        if t in self.behind:
            g, lvl = self.behind.pop(t)
            self.em.join(lvl)
            self.arrive(t, g, rows, cols, S_MAIN)
        if pair:
            return self.full[t], (self.second.pop(t)[0] if t in self.second else None)
        return self.own(t)

    def own(self, t):
        """the gradient of t for a consumer on the tensor's own (head) stream"""
        if t in self.second:
            self._add(t, *self.second.pop(t))
        return self.full[t]

    def deliver(self, t, lvl):
        """the head branch of level `lvl` has left its gradient of neck tensor t behind event EV_HB + lvl: `take` joins it"""
        self.behind[t] = (self.own(t), lvl)
        del self.full[t]


class _Emitter:
    """The walk over the module graph that fills a NetProgram's operator lists and tables; it lives for the program build only.
    Every layer emits its forward operators as the walk passes and leaves an emitter of its backward operators on the current
    tape; `backward` replays the tapes in reverse."""

    # ---- r6: amax words of the convolutions' operands (csrc/conv_x6.h "h3": the scale of the two-piece fp16 split) ------------
    # One fc_amax pass per operand TENSOR and stream instead of one per consuming launch: a forward activation's word serves its
    # forward convolution(s) and, a pass later, their weight gradients; a gradient's word serves the backward-data convolution and the
    # weight gradient of its layer.  Slots are 2 KB of one persistent buffer (32 sub-words, fc_common.h; fc_amax returns its scratch words to zero).
    AMAX_SLOTS = 1024
    AMAX_SLOT_BYTES = 2048           # include/fcaf3d_hip.h FC_AMAX_SLOT_BYTES: 32 sub-words at a 64-byte stride

    def __init__(self, p):
        self.p, self.F, self.Bk, self.tr = p, p.ops_f, p.ops_b, p.training
        nh = p.det.neck_with_head
        self.grads = _Grads(self)
        self.main = []                   # backward emitters of the main chain, in forward order
        self.branches = {}               # forked neck level -> (its neck tensor, backward emitters of its head branch (S_HEAD), in forward order)
        self.tape = self.main            # where the layer being walked leaves its backward emitter
        self.branch = None               # the neck level whose head branch's backward is being emitted, None: main chain
        self.branch_params = {}          # level -> parameters whose gradient is written on S_HEAD by that branch
        self.flushed = 0                 # rows of p.small that an OP_SMALL_GRADS covers already
        self.producer = {}               # forward tensor -> (index of the OP_CONV that wrote it, rows, columns)
        # a fine-tuning program (DESIGN.md sections 18, 19), layer by layer: a forward tensor NEEDS a gradient only if a trainable layer lies
        # upstream; a layer with nothing to train and an input nobody needs emits the rows an inference program emits for it and leaves
        # nothing on the tape; a frozen layer on the gradient path emits its backward-data half alone
        self.needs = set()
        self.unjoined = []               # head branches whose neck tensor needs no gradient: nothing to deliver, joined at the end
        self.n_reg, self.n_cls, self.Cn = nh.n_reg_outs, nh.n_classes, nh.centerness_conv.in_channels
        self.n_heads = p.nl - (1 if p.tail0 else 0)
        self.head_partials = 0           # levels whose partial of the packed head kernel's gradient has been emitted
        if self.tr:
            self.head_part = torch.zeros((p.nl, self.Cn, 64), dtype=torch.float32, device=p.dev)
            # per level: the column sums of d loss / d cls_score (the class-bias gradient's share), left by OP_HEAD_BWD
            self.bias_part = torch.zeros((p.nl, self.n_cls), dtype=torch.float32, device=p.dev)
            p.keep += [self.head_part, self.bias_part]
        self.amax = Fn.X6 and Fn.split_mode() == 2       # the convolutions scale their operands by their amax words (csrc/conv_x6.h h3)
        self.amax_f = {}                 # (forward tensor, stream) -> address index of its amax word
        self.amax_of = {}                # tensor -> address index of the amax word its PRODUCER folds into (fc_amax_out_hint)
        self.amax_used = 0
        if self.amax:
            self.amax_buf = torch.zeros(self.AMAX_SLOTS * self.AMAX_SLOT_BYTES // 4, dtype=torch.int32, device=p.dev)
            p.keep.append(self.amax_buf)
            # the words the producers fold into start every pass at zero: one fill per direction, its size patched in by `backward`
            self.amax_slot()             # (slot 0 doubles as the buffer's base address)
            p.emit(self.F, OP_CLEAR, S_MAIN, dst=p.SA(self.amax_buf.data_ptr()), bytes=0)

    def amax_slot(self):
        assert self.amax_used < self.AMAX_SLOTS
        self.amax_used += 1
        return self.p.SA(self.amax_buf.data_ptr() + self.AMAX_SLOT_BYTES * (self.amax_used - 1))

    def amax_op(self, lst, stream, x, rows, cols):
        """emit the amax pass of tensor x ((rows, cols) floats) on `stream` -> address index of its word"""
        slot = self.amax_slot()
        self.p.emit(lst, OP_AMAX, stream, x=x, n=self.p.D(rows), c=cols, slot=slot)
        return slot

    def amax_fwd(self, x, rows, cols, stream):
        if not self.amax:
            return -1
        if x in self.amax_of:
            return self.amax_of[x]
        if (x, stream) not in self.amax_f:
            self.amax_f[(x, stream)] = self.amax_op(self.F, stream, x, rows, cols)
        return self.amax_f[(x, stream)]

    def folded(self, t):
        """-> the amax word that the producer of tensor t folds max |t| into (-1: the convolutions take no amax words)"""
        if self.amax:
            self.amax_of[t] = self.amax_slot()
        return self.amax_of.get(t, -1)

    # ---- streams and gradient readiness ----------------------------------------------------------------------------------------
    def sync(self, lst, src, dst, event):
        """stream `dst` goes on behind what stream `src` holds now"""
        self.p.emit(lst, OP_RECORD, src, event=event)
        self.p.emit(lst, OP_WAIT, dst, event=event)

    def wgrad(self, cur, op, **fields):
        """a weight-gradient operator of a layer on stream `cur`: on the weight-gradient stream, behind `cur`, where there is one"""
        if self.p.wgrad_async:
            self.sync(self.Bk, cur, S_WGRAD, EV_W0 if cur == S_MAIN else EV_W1)
        self.p.emit(self.Bk, op, S_WGRAD if self.p.wgrad_async else cur, **fields)

    def wrote(self, *params):
        for prm in params:
            self.p._pready[id(prm)] = len(self.Bk)
        if self.branch is not None:
            # written on the head stream (or behind it): final for a data-parallel bucket only once the MAIN stream has
            # joined this branch (join: OP_WAIT EV_HB + level) — GradientAverager.launch_next orders the collective behind
            # the main and the weight-gradient stream, not behind S_HEAD
            self.branch_params.setdefault(self.branch, []).extend(params)

    def join(self, lvl):
        self.p.emit(self.Bk, OP_WAIT, S_MAIN, event=EV_HB + lvl)           # the head branch of this level has delivered
        for prm in self.branch_params.pop(lvl, ()):
            self.p._pready[id(prm)] = max(self.p._pready[id(prm)], len(self.Bk))

    def flush_small(self, stream):
        """the d gamma / d beta sums of the normalisation layers whose backward has been emitted since the last flush -> their
        gradient slices (one launch); called where a group of layers ends, so that a data-parallel bucket is complete early"""
        p, n = self.p, len(self.p.small) - self.flushed
        if n:
            p.emit(self.Bk, OP_SMALL_GRADS, stream, desc=p.DY('small_desc'), first=2 * self.flushed, count=2 * n)
            for _, _, _, w_, b_ in p.small[self.flushed:]:
                self.wrote(w_, b_)
            self.flushed = len(p.small)

    def head_wfin(self, stream):
        p, nh, lo = self.p, self.p.det.neck_with_head, self.p.nl - self.n_heads
        p.emit(self.Bk, OP_HEAD_WFIN, stream, part=p.SA(self.head_part[lo].data_ptr()), nl=self.n_heads, r=self.Cn, ld=64, n_reg=self.n_reg,
               n_cls=self.n_cls, g_cent=p.G(nh.centerness_conv.kernel), g_reg=p.G(nh.reg_conv.kernel), g_cls=p.G(nh.cls_conv.kernel),
               bias_part=p.SA(self.bias_part[lo].data_ptr()), g_bias=p.G(nh.cls_conv.bias))
        self.wrote(nh.centerness_conv.kernel, nh.reg_conv.kernel, nh.cls_conv.kernel, nh.cls_conv.bias)

    # ---- layers ------------------------------------------------------------------------------------------------------------
    def conv(self, x, rows_in, rows_out, mod=None, mname=None, dense=None, stream=S_MAIN, trainable=None):
        """one convolution launch and its backward.  Either MinkowskiConvolution `mod` on kernel map `mname`
        (functional._SparseConv), or dense = (weights, address index their gradient goes to): the GEMM (n, Cin) x (Cin, Cout) of
        the generative transposed convolution and of the fused 1x1 heads.  trainable (default: the kernel's requires_grad; the packed
        head GEMM always): the weight gradient is emitted iff it holds, the backward-data launch iff the input needs a gradient"""
        p, F, Bk, G = self.p, self.F, self.Bk, self.grads
        if dense is None:
            w, gw, Cin, Cout, m, n = mod.kernel, None, mod.in_channels, mod.out_channels, p.M(mname), -1
        else:
            (w, gw), m, n = dense, -1, p.D(rows_in)
            Cin, Cout = w.shape[-2:]
        y = p.T(rows_out, Cout)
        ax = self.amax_fwd(x, rows_in, Cin, stream)
        p.emit(F, OP_CONV, stream, x=x, img=p.IMG(w, False), map=m, dir=0, out=y, n=n, cin=Cin, cout=Cout, amax_x=ax)
        self.producer[y] = (len(F) - 1, rows_out, Cout)
        need_in = x in self.needs
        if trainable is None:
            trainable = mod.kernel.requires_grad if dense is None else True
        if not (self.tr and (trainable or need_in)):
            return y

        def bwd():
            gy = G.take(y, rows_out, Cout) if stream == S_MAIN else G.own(y)
            ag = (self.amax_of[gy] if gy in self.amax_of else self.amax_op(Bk, stream, gy, rows_out, Cout)) if self.amax else -1
            if need_in:                  # (an input nobody upstream needs: the weight gradient alone)
                gx = p.T(rows_in, Cin, 'b')
                p.emit(Bk, OP_CONV, stream, x=gy, img=p.IMG(w, True), map=m, dir=1, out=gx, n=n, cin=Cout, cout=Cin, amax_x=ag)
                G.src[gx] = (len(Bk) - 1, rows_in, Cin, stream)
            if trainable:                # (a frozen kernel on the gradient path: the backward-data launch alone)
                self.wgrad(stream, OP_WGRAD, x=x, gout=gy, map=m, gw=p.G(w) if gw is None else gw, n=n, cin=Cin, cout=Cout, amax_x=ax, amax_gout=ag)
                if gw is None:
                    self.wrote(w)
            if need_in:
                G.arrive(x, gx, rows_in, Cin, stream)
        self.tape.append(bwd)
        self.needs.add(y)
        return y

    def bn(self, x, mod, act, rows, res=None, stream=S_MAIN, add=None):
        """MinkowskiBatchNorm (+ residual) + activation (functional.bn_train / norm_act); add = (inverse row map, tensor): the
        apply kernel also adds tensor[inverse[r]] to row r behind the activation (the neck's sparse sum) — y IS the sum then"""
        # ... which is legal because the layer's backward never reads y: without a residual act' is recomputed from x (y = -1 below)
        assert add is None or res is None
        p, F, Bk, G = self.p, self.F, self.Bk, self.grads
        tr = self.tr and mod.training     # a layer in eval mode: the running statistics are the statistics, as in an inference program
        b, C = mod.bn, mod.bn.num_features
        affine = b.weight.requires_grad
        assert affine == b.bias.requires_grad and (affine or not tr), 'gamma and beta train together, and always in training mode'
        y = p.T(rows, C)
        mean, var, cnt = (p.T('one', C), p.T('one', C), p.T('one', 1)) if tr else (-1, -1, -1)
        if act == Fn.ACT['relu']:
            p.relu_outs.append((y, rows, C))
        prod, groups = -1, 1
        if tr and Fn.BN_FUSE and x in self.producer:
            # the convolution that wrote x leaves the column sums of x and x^2 per row block in its epilogue (conv_x6.h /
            # k_sum_*_stats) and this BatchNorm takes its batch statistics from them: no statistics pass over x
            prod, prows, pcols = self.producer[x]
            groups = pcols // C
            assert pcols == groups * C and groups in (1, 8)
            # table: [blocks][2][pcols] floats, blocks <= rows / 16 + 1 (conv.hip fc_stat_rb)
            p.patch(F[prod], stats=p.T(prows, pcols // 8, extra=8 * pcols + 256))
        ay = self.folded(y)              # the apply kernel folds max |y| into this word: a convolution gathering y needs no amax pass
        add_inv, add_src = add if add is not None else (-1, -1)
        p.emit(F, OP_BN_FWD, stream, x=x, n=p.D(rows), c=C, eps=_f(b.eps), gamma=p.S(b.weight), beta=p.S(b.bias),
               res=-1 if res is None else res, act=act, momentum=_f(b.momentum), y=y, mean=mean, var=var, cnt=cnt,
               rmean=p.S(b.running_mean), rvar=p.S(b.running_var), nbt=p.S(b.num_batches_tracked), train=1 if tr else 0,
               producer=prod, groups=groups, amax_y=ay, add_inv=add_inv, add_src=add_src)
        need_x, need_res = x in self.needs, res is not None and res in self.needs
        if not self.tr or not (tr or affine or need_x or need_res):
            return y
        sums = torch.zeros((2, C), dtype=torch.float32, device=p.dev) if affine else None
        si = p.S(sums) if affine else -1

        def bwd_eval():
            # eval mode in a layer on the gradient path (`norm_eval`, a frozen neck in front of a trainable backbone): the statistics are
            # constants, gx needs no sum — one pass (csrc/norm_eval.h), no table from the backward-data convolution that wrote gy, and
            # sums only where gamma / beta train
            if affine:
                p.small.append((sums.data_ptr(), None, C, b.weight, b.bias))
            gy, gy2 = G.take(y, rows, C, pair=True) if stream == S_MAIN else (G.own(y), None)
            gx = p.T(rows, C, 'b')
            gres = p.T(rows, C, 'b') if res is not None else -1
            agx = self.folded(gx) if need_x else -1
            p.emit(Bk, OP_BN_EVAL_BWD, stream, x=x, y=y if res is not None else -1, gy=gy, n=p.D(rows), c=C, rmean=p.S(b.running_mean),
                   rvar=p.S(b.running_var), eps=_f(b.eps), gamma=p.S(b.weight), beta=p.S(b.bias), act=act, gx=gx, gres=gres, sums=si,
                   gy2=-1 if gy2 is None else gy2, amax_gx=agx)
            if need_x:
                G.arrive(x, gx, rows, C, stream)
            if need_res:
                G.arrive(res, gres, rows, C, stream)
        if not tr:
            self.tape.append(bwd_eval)
            self.needs.add(y)
            return y

        def bwd():
            p.small.append((sums.data_ptr(), None, C, b.weight, b.bias))
            gy, gy2 = G.take(y, rows, C, pair=True) if stream == S_MAIN else (G.own(y), None)
            gx = p.T(rows, C, 'b')
            gres = p.T(rows, C, 'b') if res is not None else -1
            prod = -1
            # the LAST contribution to gy is the result of a backward-data convolution (and at most one other contribution
            # arrived before it): that launch leaves this layer's two reductions (sum g', sum g' xhat) in its epilogue
            # (fc_conv_fwd_bn_bwd_stats; `add` = the earlier contribution, bn_y = this layer's output where act' needs it)
            # — no reduction pass over x, gy (, y)
            last, first = (gy, None) if gy2 is None else (gy2, gy)
            src = G.src.get(last)
            if Fn.BN_FUSE and src is not None and src[3] == stream and src[1:3] == (rows, C):
                prod = src[0]
                p.patch(Bk[prod], stats=p.T(rows, C // 8, 'b', extra=8 * C + 256), bn_x=x, bn_mean=mean, bn_var=var,
                        bn_gamma=p.S(b.weight), bn_beta=p.S(b.bias), bn_eps=_f(b.eps), bn_act=act,
                        bn_add=-1 if first is None else first, bn_y=-1 if res is None else y)
            agx = self.folded(gx)
            p.emit(Bk, OP_BN_BWD, stream, x=x, y=y if res is not None else -1, gy=gy, n=p.D(rows), c=C, mean=mean, var=var,
                   cnt=cnt, eps=_f(b.eps), gamma=p.S(b.weight), beta=p.S(b.bias), act=act, gx=gx, gres=gres, sums=si,
                   gy2=-1 if gy2 is None else gy2, producer=prod, amax_gx=agx)
            G.arrive(x, gx, rows, C, stream)
            if res is not None:
                G.arrive(res, gres, rows, C, stream)
        assert x in self.needs and (res is None or res in self.needs)
        self.tape.append(bwd)
        self.needs.add(y)
        return y

    def stem(self, stem, inorm):
        """me_resnet.py conv1: the 3-channel convolution, instance norm + ReLU, max pool -> (tensor, rows, channels)"""
        p, F, relu = self.p, self.F, Fn.ACT['relu']
        tr = self.tr and stem.kernel.requires_grad       # a frozen stem emits an inference program's rows: no col buffer, the arg-max rows, no mask
        assert not self.tr or inorm.weight.requires_grad == inorm.bias.requires_grad == stem.kernel.requires_grad
        x0, seg1 = p.DY('x0'), p.DY('seg1')
        t_stem = p.T('n1', 64)
        col = p.T('n1', 84) if tr else -1
        p.emit(F, OP_STEM_FWD, S_MAIN, x=x0, w=p.S(stem.kernel), map=p.M('stem'), out=t_stem, col=col)
        mean_in, var_in, cnt_in = p.T('B', 64), p.T('B', 64), p.T('B', 1)
        p.emit(F, OP_COL_STATS, S_MAIN, x=t_stem, seg=seg1, n=p.D('n1'), c=64, nseg=p.D('B'), mean=mean_in, var=var_in, cnt=cnt_in)
        # instance norm + ReLU + max pool in ONE pass (norm.hip k_norm_act_maxpool8_fwd, bit for bit the two operators): the
        # normalised tensor's only consumer is the pool, and the backward pass recomputes act' from t_stem — it is stored only for
        # `decisions` (keep_state)
        t_in = p.T('n1', 64) if p.keep_state else -1
        if p.keep_state:
            p.relu_outs.append((t_in, 'n1', 64))
        # the arg-max rows (n2 x 64 ints): what an inference program's kernel stores, and what `decisions` reads (keep_state).  A training
        # program's backward pass reads a per-child mask instead — one 64-bit word per n1 row, bit c set where arg[parent[r]][c] == r,
        # written by the same forward kernel (norm.hip fc_norm_act_maxpool8_mask_fwd): two 4-byte words per row, the dimension 'n1w'
        t_pool = p.T('n2', 64)
        arg = p.T('n2', 64) if (p.keep_state or not tr) else -1
        p.pool_arg = (arg, 'n2', 64)
        ap = self.folded(t_pool)
        pool_parent = p.T('n1', 1) if tr else -1          # child row -> pooled row (4 bytes per row), for the backward pass
        pool_mask = p.T('n1w', 1) if tr else -1
        p.emit(F, OP_NORM_POOL_FWD, S_MAIN, x=t_stem, seg=seg1, c=64, mean=mean_in, var=var_in, eps=_f(inorm.eps), gamma=p.S(inorm.weight),
               beta=p.S(inorm.bias), act=relu, map=p.M('pool'), out=t_pool, arg=arg, y=t_in, amax_out=ap, parent=pool_parent, mask=pool_mask)
        if tr:
            p.in_sums = p.T('B', 2 * 64, 'b')

            def bwd():
                p.small.append((None, 'B', 64, inorm.weight, inorm.bias))
                g_pool = self.grads.take(t_pool, 'n2', 64)
                g_stem = p.T('n1', 64, 'b')
                # pool backward + instance-norm backward without the scattered gradient in between: the normalisation backward's
                # kernels read row r's gradient as g_pool[parent[r]] where the mask's bit is set (arg[parent[r]] == r), else 0 (norm.hip
                # pool_parent) — the sums in the order of OP_NORM_BWD, the same bits; y is not read (bn_pre recomputes act' from t_stem)
                p.emit(self.Bk, OP_POOL_NORM_BWD, S_MAIN, x=t_stem, g_pool=g_pool, arg=arg, parent=pool_parent, seg=seg1, n=p.D('n1'), c=64,
                       nseg=p.D('B'), mean=mean_in, var=var_in, cnt=cnt_in, eps=_f(inorm.eps), gamma=p.S(inorm.weight),
                       beta=p.S(inorm.bias), act=relu, gx=g_stem, sums=p.in_sums, mask=pool_mask)
                self.wgrad(S_MAIN, OP_STEM_WGRAD, col=col, gout=g_stem, map=p.M('stem'), gw=p.G(stem.kernel))
                self.wrote(stem.kernel)
            self.tape.append(bwd)
            self.needs.add(t_pool)
        return t_pool, 'n2', 64

    def level(self, li, layer, x):
        """backbone level li (me_resnet.py BasicBlock: the first one strided, with a 1x1 downsample branch) -> (tensor, rows, channels)"""
        relu, none, N = Fn.ACT['relu'], Fn.ACT['none'], _Names
        (cur, cur_rows, _), rows = x, N.rows(li)
        if self.tr:
            self.tape.append(lambda: self.flush_small(S_MAIN))           # reversed walk: reached after this level's backward
        for j, blk in enumerate(layer):
            if j == 0:
                assert blk.downsample is not None and blk.conv1.stride == 2
                t_ds = self.conv(cur, cur_rows, rows, blk.downsample[0], N.ds(li))
                res = self.bn(t_ds, blk.downsample[1], none, rows)
                t1 = self.conv(cur, cur_rows, rows, blk.conv1, N.down(li))
            else:
                assert blk.downsample is None
                res = cur
                t1 = self.conv(cur, rows, rows, blk.conv1, N.same(li))
            t1 = self.bn(t1, blk.norm1, relu, rows)
            t2 = self.conv(t1, rows, rows, blk.conv2, N.same(li))
            cur = self.bn(t2, blk.norm2, relu, rows, res=res)
        return cur, rows, blk.conv1.out_channels

    def up(self, i, up, x, fb):
        """neck level i < nl - 1: up_block_{i + 1} on the coarser level's tensor x, joined with the backbone's `fb` -> (tensor, rows, channels)"""
        p, F, Bk, G, tr, elu = self.p, self.F, self.Bk, self.grads, self.tr, Fn.ACT['elu']
        (x, x_rows, x_C), (fb, fb_rows, _) = x, fb
        g_rows, Ci = _Names.gen(i), up[0].out_channels
        # generative transposed convolution: one dense GEMM (n, Cin) x (Cin, 8 Cout) whose (n, 8 Cout) output IS the
        # (8 n, Cout) children matrix (row 8 i + k); its weight gradient comes out in the GEMM's layout and is permuted
        # into the layer's (8, Cin, Cout) kernel gradient afterwards
        gw_tmp = torch.zeros((x_C, 8 * Ci), dtype=torch.float32, device=p.dev)
        gw_i = p.S(gw_tmp)

        def bwd_perm():
            if up[0].kernel.requires_grad:
                p.emit(Bk, OP_PERMUTE_GENT, S_WGRAD if p.wgrad_async else S_MAIN, src=gw_i, dst=p.G(up[0].kernel), cin=x_C, cout=Ci)
                self.wrote(up[0].kernel)
            self.flush_small(S_MAIN)                     # ... and after every neck level's up-block
        if tr:
            self.tape.append(bwd_perm)                   # forward order: BEFORE the GEMM, so the reversed walk reaches it after
        t = self.conv(x, x_rows, x_rows, dense=(p.gent_w[p.gents.index(up[0])], gw_i), trainable=up[0].kernel.requires_grad)
        t = self.bn(t, up[1], elu, g_rows)
        t = self.conv(t, g_rows, g_rows, up[3], _Names.gsame(i))
        # x = inputs[i] + t: every backbone voxel lies in the generated set -> the union IS the generated set (sparse.CoordMap.union)
        # and the up block's last normalisation writes it (r7): its apply kernel adds the backbone row behind the activation
        # through the inverse of rows{i} and folds the amax word of the SUM, complete when that kernel ends — before the head
        # branch forks.  (The map is made here, two small launches, not by fc_plan_maps: the plan's outputs and interface stay.)
        rows_i = p.DY(_Names.union(i))
        inv_i = p.T(g_rows, 1)
        p.emit(F, OP_INV_ROWS, S_MAIN, rows=rows_i, n=p.D(fb_rows), n_inv=p.D(g_rows), inv=inv_i)
        u = self.bn(t, up[4], elu, g_rows, add=(inv_i, fb))

        def bwd_union():
            # d u / d (normalisation output) = identity on all rows (n_a == n_union): the layer's backward, next in the
            # reversed walk, takes the gradient of u as its own
            gu = G.take(u, g_rows, Ci)
            gfb = p.T(fb_rows, Ci, 'b')
            p.emit(Bk, OP_GATHER, S_MAIN, src=gu, idx=rows_i, n=p.D(fb_rows), c=Ci, dst=gfb)
            G.arrive(fb, gfb, fb_rows, Ci, S_MAIN)
        if tr and fb in self.needs and u in self.needs:  # (a backbone tensor behind the frontier takes no share of the union's gradient; a union nobody needs has none)
            self.tape.append(bwd_union)
        return u, g_rows, Ci

    def head(self, i, ob, x):
        """out_block_i + forward_single of neck level i on its tensor x: on the head stream for i > 0"""
        p, F, Bk, tr = self.p, self.F, self.Bk, self.tr
        nh, n_reg, n_cls = p.det.neck_with_head, self.n_reg, self.n_cls
        x, rows, _ = x
        hs = S_HEAD if (p.head_overlap and i > 0) else S_MAIN
        if hs == S_HEAD:
            assert p.img_pair or p.image_wait == 'entry', 'a head branch (it reads the packed head image) forked in front of the image wait'
            self.sync(F, S_MAIN, S_HEAD, EV_FORK + i)
            self.tape = []
            self.branches[i] = (x, self.tape)
        o = self.conv(x, rows, rows, ob[0], _Names.same(p.nl) if i == p.nl - 1 else _Names.gsame(i), stream=hs)
        o = self.bn(o, ob[1], Fn.ACT['elu'], rows, stream=hs)
        gw_head = p.SA(self.head_part[i].data_ptr()) if tr else -1

        def partial_done():
            self.head_partials += 1
            if self.head_partials == self.n_heads and p.wgrad_async:
                # every level's partial of the packed head kernel is on its way, all on the weight-gradient stream:
                # sum them there right away (the head's parameters sit in the first gradient bucket to leave)
                self.head_wfin(S_WGRAD)
        if tr:
            self.tape.append(partial_done)               # forward order: BEFORE the GEMM, so the reversed walk reaches it right after
        y = self.conv(o, rows, rows, dense=(p.packed, gw_head), stream=hs)
        off = _Names.off(i)
        outs = [p.AL(t, off, c) for t, c in zip(p.out_idx, (1, n_reg, n_cls, 1))]
        p.emit(F, OP_HEAD_FWD, hs, y=y, ld=64, bias=p.S(nh.cls_conv.bias), scale=p.S(nh.scales[i].scale), n=p.D(rows), n_reg=n_reg,
               n_cls=n_cls, cent=outs[0], bbox=outs[1], cls=outs[2], cmax=outs[3])

        def bwd():
            gy = p.T(rows, 64, 'b')
            gin = [p.AL(g, off, c) for g, c in zip(p.gout_idx, (1, n_reg, n_cls))]
            # ... with d loss / d scale of this level and this level's share of the class-bias gradient (column sums of
            # d loss / d cls_score; summed over the levels by OP_HEAD_WFIN) out of the same pass (r5: they were single-block
            # reductions over every location, k_col_sum: 0.35 ms per step on the dependent chain)
            agy = self.folded(gy)        # the kernel folds max |gy| for the backward-data GEMM behind it
            p.emit(Bk, OP_HEAD_BWD, hs, y=y, ld=64, scale=p.S(nh.scales[i].scale), bbox=outs[1], g_cent=gin[0], g_bbox=gin[1],
                   g_cls=gin[2], n=p.D(rows), n_reg=n_reg, n_cls=n_cls, gy=gy, gs_row=-1, g_scale=p.G(nh.scales[i].scale),
                   bias_part=p.SA(self.bias_part[i].data_ptr()), amax_gy=agy)
            self.wrote(nh.scales[i].scale)
            self.grads.arrive(y, gy, rows, 64, hs)
        if tr:
            self.tape.append(bwd)
        self.tape = self.main

    # ---- backward program --------------------------------------------------------------------------------------------------
    def backward(self):
        p, Bk, tr = self.p, self.Bk, self.tr
        if self.amax:
            n_fwd_slots = self.amax_used
            p.patch(self.F[0], bytes=self.AMAX_SLOT_BYTES * n_fwd_slots)     # the forward pass clears its own words; they stay valid through the backward pass
            if tr:
                p.emit(Bk, OP_CLEAR, S_MAIN, dst=p.SA(self.amax_buf.data_ptr() + self.AMAX_SLOT_BYTES * n_fwd_slots), bytes=0)
        if not tr:
            return
        if p.head_overlap:
            # the head branches depend on the loss gradients only: their backward is enqueued first, on the head stream, finest
            # forked level first (the main chain needs that one first); each leaves the gradient of its neck tensor behind an event
            self.sync(Bk, S_MAIN, S_HEAD, EV_BWD0)       # the loss gradients are ready on the caller's stream
            for lvl in sorted(self.branches):
                xt, tape = self.branches[lvl]
                assert xt not in self.grads.full
                self.branch = lvl
                for e in reversed(tape):
                    e()
                self.flush_small(S_HEAD)                 # this branch's normalisation layer
                self.branch = None
                p.emit(Bk, OP_RECORD, S_HEAD, event=EV_HB + lvl)
                if xt in self.needs:
                    self.grads.deliver(xt, lvl)
                else:
                    self.unjoined.append(lvl)
        for e in reversed(self.main):
            e()
        for lvl in self.unjoined:                        # (its parameters' gradients are final once the main stream has joined it)
            self.join(lvl)
        assert not self.grads.behind and not self.branch_params, 'a head branch was never joined'
        if not p.wgrad_async:
            # without the weight-gradient stream the partials were written on the streams of their levels (main, head): the
            # main stream has joined every head branch by now
            self.head_wfin(S_MAIN)
        self.flush_small(S_MAIN)                         # what is left: the stem's instance norm
        assert self.head_partials == self.n_heads
        missing = [n for n, prm in p.det.named_parameters() if prm.requires_grad and id(prm) not in p._pready]
        if p.tail0:                                      # out_block_0 and scales.0 get their gradients on the per-operator path
            missing = [n for n in missing if not (n.startswith('neck_with_head.out_block_0.') or n == 'neck_with_head.scales.0.scale')]
        assert not missing, missing
        if p.wgrad_async:
            self.sync(Bk, S_WGRAD, S_MAIN, EV_WEND)
        if self.amax:
            p.patch(Bk[0], bytes=self.AMAX_SLOT_BYTES * (self.amax_used - n_fwd_slots))


class _Weights(ImageSet):
    """the executor's view of a detector's weights: pre-split images of every convolution kernel (weight_images.ImageSet), the
    three 1x1 head kernels packed side by side (zero-padded to 64 columns), the generative transposed convolutions' kernels in
    their GEMM form (Cin, 8 Cout) — persistent buffers, rebuilt with the images (5-6 launches on the current stream)"""

    def __init__(self, det, dev, sig):
        nh = det.neck_with_head
        self.det, self.sig = det, sig
        head = (nh.centerness_conv, nh.reg_conv, nh.cls_conv)
        convs = [m for m in det.modules() if isinstance(m, MEnn.MinkowskiConvolution) and m not in head]
        self.gents = [m for m in det.modules() if isinstance(m, MEnn.MinkowskiGenerativeConvolutionTranspose)]
        C = nh.centerness_conv.in_channels
        self.ncol = 1 + nh.n_reg_outs + nh.n_classes
        self.packed = torch.zeros((1, C, 64), dtype=torch.float32, device=dev)       # [centerness | reg | cls | 0...]
        self.gent_w = [torch.empty((1, m.in_channels, 8 * m.out_channels), dtype=torch.float32, device=dev) for m in self.gents]
        ws = [m.kernel for m in convs] + [self.packed] + self.gent_w
        super().__init__([m.kernel for m in convs + list(head) + self.gents], weights=ws)

    def lookup(self, weight, transposed):
        return None                 # programs read these images natively; a per-operator convolution of such a step builds its own

    @torch.no_grad()
    def prepare(self):
        nh = self.det.neck_with_head
        torch.cat((nh.centerness_conv.kernel, nh.reg_conv.kernel, nh.cls_conv.kernel), dim=1, out=self.packed[0][:, :self.ncol])
        for m, w in zip(self.gents, self.gent_w):
            w.view(m.in_channels, 8, m.out_channels).copy_(m.kernel.permute(1, 0, 2))


class _NetFn(torch.autograd.Function):
    """The whole network body as one autograd node: forward = one fc_exec call, backward = one fc_exec call that leaves every
    parameter gradient in the (flat) gradient buffer."""

    @staticmethod
    def forward(ctx, anchor, prog, st):
        ctx.prog, ctx.st = prog, st
        outs = prog._forward(st)
        ctx.mark_non_differentiable(outs[3])
        return outs

    @staticmethod
    def backward(ctx, g_cent, g_bbox, g_cls, _g_max, g_x0=None):
        ctx.prog._backward(ctx.st, g_cent, g_bbox, g_cls, g_x0)    # (the state is released with the graph; retain_graph keeps it)
        return None, None, None


def program_for(det, training, tail0=False):
    """the cached NetProgram of this detector for the current mode / stream configuration (None: not covered -> module path)"""
    if not supported(det):
        return None
    nh = det.neck_with_head
    if tail0 and min(det.backbone.n_outs, 4) < 2:
        return None
    front = freeze_plan(det) if training else -1
    if front is None:
        return None
    by_plan = not isinstance(front, int)       # a per-layer plan: the program is named by it, `frozen` then says the declared prefix
    key = (bool(training), bool(Fn.WGRAD_ASYNC), bool(nh.head_overlap), bool(tail0))
    keep = bool(KEEP_STATE)                    # the recorder flips it at run time: a program built without the stem's normalised output
                                               # must never be handed to `decisions`
    fuse = bool(Fn.BN_FUSE)                    # changes the emitted program (statistics tables, producer words): part of the cache key
    # ... and so does the operand split (r6): the three-product route's program carries amax slots, hint words and clear operators
    # (the weight images, shared by the programs, carry the mode in their own key)
    mode = Fn.split_mode() if Fn.X6 else -1
    cache = det.__dict__.setdefault('_programs', {})
    sig = NetProgram.signature(det)
    key += (IMAGE_WAIT,)                       # ... and who waits for the weight images (a training program with wgrad_async carries the pair or not)
    prog = cache.get(key + (fuse, mode, keep, front))
    if prog is None or prog._sig != sig:
        if by_plan:
            prog = NetProgram(det, *key[:4], keep_state=keep, frozen=getattr(det.backbone, 'frozen_stages', -1), plan=front, image_wait=IMAGE_WAIT)
        else:
            prog = NetProgram(det, *key[:4], keep_state=keep, frozen=front, image_wait=IMAGE_WAIT)
        cache[key + (fuse, mode, keep, front)] = prog
    return prog


_FLAGS = (operator.attrgetter('requires_grad'), operator.attrgetter('training'))


def frontier(det):
    """the frozen prefix of the backbone that a TRAINING program of this detector stops its backward pass at, read from the
    parameters' requires_grad and the modules' training flags as they are NOW (part of the program cache key: freezing a stage or
    calling train() / eval() on it never meets a stale program):

      -1   nothing is frozen (every parameter requires a gradient, every BatchNorm is in training mode): today's program
       0   the stem is frozen (conv1.0's kernel, conv1.1's weight and bias)
       k   the stem and layer1 .. layerk are frozen: none of their parameters requires a gradient and their BatchNorm are in eval mode
     None  anything else — a frozen parameter behind a trainable one, an eval-mode BatchNorm in a trainable stage (`norm_eval`), a
           frozen neck or head layer: no frozen PREFIX.  `freeze_plan` then decides whether the pattern is one the model declared
           (and the executor compiles) or the module path takes the step (autograd handles any pattern)

    What is read per call is two tuples of flags; the verdict per pair of tuples is cached on the detector."""
    lists = det.__dict__.get('_frontier_lists')
    if lists is None:
        bb = det.backbone
        stages = [bb.conv1] + [getattr(bb, f'layer{i}') for i in range(1, min(bb.n_outs, 4) + 1)]
        rest = [m for n, m in det.named_children() if m is not bb]
        params = [list(s.parameters()) for s in stages] + [[q for m in rest for q in m.parameters()]]
        norms = [[m for m in s.modules() if isinstance(m, MEnn.MinkowskiBatchNorm)] for s in stages] + \
                [[m for r in rest for m in r.modules() if isinstance(m, MEnn.MinkowskiBatchNorm)]]
        lists = det.__dict__['_frontier_lists'] = (params, norms, [q for g in params for q in g], [m for g in norms for m in g], {})
    params, norms, all_p, all_n, verdicts = lists
    flags = (tuple(map(_FLAGS[0], all_p)), tuple(map(_FLAGS[1], all_n)))
    if flags in verdicts:
        return verdicts[flags]
    k = -1
    while k + 1 < len(params) - 1 and not any(q.requires_grad for q in params[k + 1]) and not any(m.training for m in norms[k + 1]):
        k += 1
    ok = all(q.requires_grad for g in params[k + 1:] for q in g) and all(m.training for g in norms[k + 1:] for m in g)
    v = verdicts[flags] = k if ok else None
    return v


def _declared_flags(det, lists):
    """the flag tuples (`frontier`'s two) that the constructors' declarations imply after train(): backbone.frozen_stages / norm_eval,
    neck_with_head.norm_eval / frozen_neck"""
    params, norms, _, _, _ = lists
    bb, nh = det.backbone, det.neck_with_head
    k, ne_b = getattr(bb, 'frozen_stages', -1), bool(getattr(bb, 'norm_eval', False))
    ne_n, fn = bool(getattr(nh, 'norm_eval', False)), bool(getattr(nh, 'frozen_neck', False))
    neck = {id(q) for m in (nh.neck_blocks() if hasattr(nh, 'neck_blocks') else ()) for q in m.parameters()}
    neck_norms = {id(m) for b in (nh.neck_blocks() if hasattr(nh, 'neck_blocks') else ()) for m in b.modules()}
    rg = tuple(s > k for s, g in enumerate(params[:-1]) for _ in g) + tuple(not (fn and id(q) in neck) for q in params[-1])
    tm = tuple(s > k and not ne_b for s, g in enumerate(norms[:-1]) for _ in g) + \
        tuple(not ((fn or ne_n) and id(m) in neck_norms) for m in norms[-1])
    return rg, tm


def freeze_plan(det):
    """what a TRAINING program of this detector is compiled for, or None (the module path takes the step):

      an int     `frontier(det)` wherever that is not None: nothing frozen, or a frozen prefix of the backbone
      a tuple    the current flag tuples (every parameter's requires_grad, every BatchNorm's mode — a per-layer plan, hashable, part of
                 the program cache key) when they are exactly what the constructors' declarations imply after train():
                 MEResNet3D(frozen_stages, norm_eval) and Fcaf3DNeckWithHead(norm_eval, frozen_neck) in any combination.  The emitter
                 then reads each layer's own flags: an eval-mode BatchNorm on the gradient path runs OP_BN_EVAL_BWD (with sums only
                 where gamma / beta train), a frozen convolution on it its backward-data launch alone, a layer behind which nothing
                 trains an inference program's rows
      None       anything set by hand that no declaration implies (a lone layer2.eval(), one frozen neck kernel), frozen head
                 kernels or scales, a training-mode BatchNorm with frozen gamma / beta, a stem whose convolution and norm differ,
                 Bottleneck depths: autograd on the module path handles any of these

    Verdicts are cached per pair of tuples and declaration, as `frontier` caches its own."""
    front = frontier(det)
    if front is not None:
        return front
    lists = det.__dict__['_frontier_lists']
    _, _, all_p, all_n, _ = lists
    bb, nh = det.backbone, det.neck_with_head
    flags = (tuple(map(_FLAGS[0], all_p)), tuple(map(_FLAGS[1], all_n)))
    decl = (getattr(bb, 'frozen_stages', -1), getattr(bb, 'norm_eval', False), getattr(nh, 'norm_eval', False), getattr(nh, 'frozen_neck', False))
    verdicts = det.__dict__.setdefault('_plan_verdicts', {})
    if (flags, decl) not in verdicts:
        ok = getattr(bb.BLOCK, 'expansion', 1) == 1 and _declared_flags(det, lists) == flags
        verdicts[(flags, decl)] = flags if ok else None
    return verdicts[(flags, decl)]
