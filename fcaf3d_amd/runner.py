"""Optimizer / LR-schedule / step driver with the reference's training recipe:

    optimizer        = dict(type='AdamW', lr=0.001, weight_decay=0.0001)      configs/fcaf3d/fcaf3d.py:30
    optimizer_config = dict(grad_clip=dict(max_norm=10, norm_type=2))         :31   (mmcv OptimizerHook: clip_grad_norm_)
    lr_config        = dict(policy='step', warmup=None, step=[8, 11])         :32   (mmcv StepLrUpdaterHook, gamma 0.1)
    runner           = dict(type='EpochBasedRunner', max_epochs=12)           :33

`TrainStep` is what mmcv's `EpochBasedRunner.run_iter` + `OptimizerHook.after_train_iter` do for one batch:
zero_grad -> model(return_loss=True, **batch) -> sum of the `loss*` entries (mmdet `_parse_losses`) -> backward ->
(data parallel: gradient averaging, overlapped with backward) -> clip_grad_norm_ -> optimizer.step; `epoch_end()` is the
LR hook's per-epoch update.  On the GPU the parameters, gradients and AdamW moments live in flat buffers (flat.FlatParams)
and clip + AdamW are three launches of csrc/optim.hip (`FlatAdamW`); CPU parameters (the host-logic tests) take
torch.optim.AdamW + clip_grad_norm_, the calls the reference makes.
"""
import contextlib
import os
import time

import numpy as np
import torch

from . import _lib as L
from . import dist as D
from . import executor
from . import functional as Fn
from .flat import FlatParams
from .weight_images import ImageSet


class FlatAdamW:
    """torch.optim.AdamW (betas 0.9 / 0.999, eps 1e-8, decoupled weight decay, no amsgrad) + clip_grad_norm_ over the flat
    buffers of a `FlatParams`: `step(max_norm)` = fc_grad_norm (global 2-norm and clip coefficient, on the device) +
    fc_adamw_step (one pass; the coefficient is applied while the gradient is read).  One difference to torch.optim.AdamW:
    a parameter that received NO gradient in a step has its slice zeroed by `FlatParams.gather` and is stepped with a zero
    gradient (weight decay and moment decay apply) where torch skips it — every parameter of the FCAF3D detector receives a
    gradient in every step.  Keeps the slice of torch's optimizer
    interface the runner and the LR hook use: `param_groups`, `defaults`, `zero_grad`, `state_dict` / `load_state_dict` in
    torch's own layout (per-parameter `step`, `exp_avg`, `exp_avg_sq`), so mmcv-style checkpoints round-trip."""

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, multipliers=None):
        """multipliers: one (lr_mult, decay_mult) per parameter of `flat`, in its order (param_multipliers); None: all 1"""
        self.flat = flat
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False)
        self.param_groups = [dict(self.defaults, params=flat.params)]      # ONE schedule group: the LR hook scales every parameter alike
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)
        self.norm_clip = torch.zeros(2, dtype=torch.float32, device=flat.data.device)      # [global grad norm, clip coefficient]
        self.steps = 0
        self.multipliers = [(float(a), float(b)) for a, b in multipliers] if multipliers is not None else [(1.0, 1.0)] * len(flat.params)
        assert len(self.multipliers) == len(flat.params)
        self.runs, self.table = None, None       # all ones: fc_adamw_step, as without multipliers
        if any(mm != (1.0, 1.0) for mm in self.multipliers):
            self.runs = group_runs(flat.offsets, self.multipliers)
            self.table = torch.from_numpy(pack_runs(*self.runs, flat.n)).to(flat.data.device)      # uploaded once
        self.ema = None                          # the weight average (enable_ema): flat.n floats laid out like flat.data
        self.acc = None                          # an open accumulation group's gradient sum (accumulate): flat.n floats, allocated on first use

    def enable_ema(self):
        """-> the buffer of the parameters' moving average (WeightEma owns its schedule), a copy of flat.data: padding zero, and zero
        it stays under e * keep + mu * 0"""
        if self.ema is None:
            self.ema = self.flat.data.clone()
        return self.ema

    def zero_grad(self, set_to_none=True):
        for p in self.flat.params:
            p.grad = None                        # the flat gradient buffer is overwritten, not accumulated into
        self.flat.complete = False

    def accumulate(self, scale, first, gathered=False, ema=None):
        """a micro-iteration that does not step (mmcv GradientCumulativeOptimizerHook): acc = g * scale (`first` of its group) or
        acc = acc + g * scale, ONE fc_grad_accum over the flat buffers; the gradient buffer is left as it is.  scale: 1 / factor, rounded
        to fp32 by the call.  ema: (mu, keep) of an average update that is due on this iteration (WeightEma.coeffs): the average moves
        towards the unchanged parameters in the same launch"""
        f = self.flat
        if not f.data.is_cuda:
            raise RuntimeError('FlatAdamW runs on the GPU only (HIP); CPU parameters take torch.optim.AdamW')
        if not gathered and not getattr(f, 'complete', False):
            f.gather()
        if self.acc is None:
            if not first:
                raise RuntimeError('FlatAdamW.accumulate(first=False) without an open group')
            self.acc = torch.zeros_like(f.grad)
        if ema is not None and self.ema is None:
            raise RuntimeError('FlatAdamW.accumulate(ema=...) without an average: call enable_ema() first')
        mu, keep = (float(ema[0]), float(ema[1])) if ema is not None else (0.0, 0.0)
        L.call('fc_grad_accum', L.ptr(self.acc), L.ptr(f.grad), f.n, float(scale), 1 if first else 0,
               L.ptr(self.ema) if ema is not None else None, L.ptr(f.data) if ema is not None else None, mu, keep, L.stream())

    def step(self, max_norm=None, gathered=False, ema=None, accum_scale=None):
        """-> the global gradient norm (0-d device tensor) when max_norm is given.  ema: (mu, keep) of a step whose average update
        is due (WeightEma.coeffs): the step is then ONE fc_adamw_ema_step, which updates the average of every vector it has just
        stepped; None: exactly the call made without an average.  accum_scale: the stepping iteration of an open group (accumulate):
        fc_grad_accum_norm writes acc + g * accum_scale over the gradient and takes its norm in the same pass, in place of fc_grad_norm;
        None: exactly the calls made without accumulation"""
        f = self.flat
        if not f.data.is_cuda:
            raise RuntimeError('FlatAdamW runs on the GPU only (HIP); CPU parameters take torch.optim.AdamW')
        if not gathered and not getattr(f, 'complete', False):      # complete: the executor's backward left every gradient in place
            f.gather()
        g = self.param_groups[0]
        self.steps += 1
        b1, b2 = g['betas']
        clip = None
        if accum_scale is not None:
            if self.acc is None:
                raise RuntimeError('FlatAdamW.step(accum_scale=...) without an open group: call accumulate() first')
            ws = L.workspace(L.query('fc_grad_accum_norm_ws_bytes', f.n), f.data.device)
            clip = self.norm_clip if max_norm is not None else None
            L.call('fc_grad_accum_norm', L.ptr(f.grad), L.ptr(self.acc), f.n, float(accum_scale), float(max_norm) if clip is not None else 0.0,
                   L.ptr(clip), L.ptr(ws), ws.numel(), L.stream())
        elif max_norm is not None:
            ws = L.workspace(L.query('fc_grad_norm_ws_bytes', f.n), f.data.device)
            L.call('fc_grad_norm', L.ptr(f.grad), f.n, float(max_norm), L.ptr(self.norm_clip), L.ptr(ws), ws.numel(), L.stream())
            clip = self.norm_clip
        if ema is not None:
            if self.ema is None:
                raise RuntimeError('FlatAdamW.step(ema=...) without an average: call enable_ema() first')
            L.call('fc_adamw_ema_step', L.ptr(f.data), L.ptr(f.grad), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), L.ptr(self.ema), f.n,
                   float(g['lr']), float(b1), float(b2), float(g['eps']), float(g['weight_decay']), 1.0 - b1 ** self.steps,
                   1.0 - b2 ** self.steps, L.ptr(clip), L.ptr(self.table), len(self.runs[0]) if self.table is not None else 0,
                   float(ema[0]), float(ema[1]), L.stream())
        elif self.table is None:
            L.call('fc_adamw_step', L.ptr(f.data), L.ptr(f.grad), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), f.n, float(g['lr']),
                   float(b1), float(b2), float(g['eps']), float(g['weight_decay']), 1.0 - b1 ** self.steps, 1.0 - b2 ** self.steps,
                   L.ptr(clip), L.stream())
        else:
            L.call('fc_adamw_step_groups', L.ptr(f.data), L.ptr(f.grad), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), f.n, float(g['lr']),
                   float(b1), float(b2), float(g['eps']), float(g['weight_decay']), 1.0 - b1 ** self.steps, 1.0 - b2 ** self.steps,
                   L.ptr(clip), L.ptr(self.table), len(self.runs[0]), L.stream())
        return self.norm_clip[0].clone() if clip is not None else None      # a copy: norm_clip is rewritten by the next step

    def _views(self, buf):
        return [buf[o:o + p.numel()].view(p.shape) for p, o in zip(self.flat.params, self.flat.offsets)]

    def state_dict(self):
        """torch's layout.  Without multipliers: one group over all parameters.  With them: one group per parameter carrying its
        EFFECTIVE lr / weight_decay (what mmcv's constructor hands torch.optim.AdamW), so the file reads as the reference's would"""
        m, v = self._views(self.exp_avg), self._views(self.exp_avg_sq)
        state = {i: dict(step=torch.tensor(float(self.steps)), exp_avg=m[i].clone(), exp_avg_sq=v[i].clone())
                 for i in range(len(m))} if self.steps else {}
        group = {k: val for k, val in self.param_groups[0].items() if k != 'params'}
        if self.table is None:
            return dict(state=state, param_groups=[dict(group, params=list(range(len(self.flat.params))))])
        groups = [dict(group, lr=group['lr'] * a, weight_decay=group['weight_decay'] * b, params=[i])
                  for i, (a, b) in enumerate(self.multipliers)]
        return dict(state=state, param_groups=groups)

    def load_state_dict(self, sd):
        """accepts one group over all parameters or one group per parameter; per-parameter rates that are not ONE base rate
        times the configured multipliers raise (the checkpoint was written under another paramwise_cfg)"""
        groups = sd['param_groups']
        if len(groups) == 1:
            base = dict(groups[0])
        else:
            if len(groups) != len(self.multipliers) or any(list(gr['params']) != [i] for i, gr in enumerate(groups)):
                raise ValueError(f'optimizer state holds {len(groups)} parameter groups: expected 1, or one per parameter ({len(self.multipliers)})')
            base = dict(groups[0])
            for key, col in (('lr', 0), ('weight_decay', 1)):
                pairs = list(zip(groups, self.multipliers))      # the base rate: a parameter with multiplier 1 holds it exactly
                ref = next((gr[key] for gr, mm in pairs if mm[col] == 1.0),
                           next((gr[key] / mm[col] for gr, mm in pairs if mm[col] > 0), self.param_groups[0][key]))
                for i, (gr, mm) in enumerate(zip(groups, self.multipliers)):
                    if abs(gr[key] - ref * mm[col]) > 1e-6 * max(abs(ref * mm[col]), abs(gr[key])):
                        raise ValueError(f"optimizer state: parameter {i} has {key} {gr[key]!r}, the configured multipliers give "
                                         f"{ref!r} x {mm[col]!r}: it was written under another paramwise_cfg")
                base[key] = ref
        m, v = self._views(self.exp_avg), self._views(self.exp_avg_sq)
        steps = 0
        with torch.no_grad():
            self.exp_avg.zero_()                  # entries the loaded state does not hold start from zero moments, as a
            self.exp_avg_sq.zero_()               # fresh torch.optim.AdamW state would
            for i, st in sd['state'].items():
                m[int(i)].copy_(st['exp_avg'])
                v[int(i)].copy_(st['exp_avg_sq'])
                steps = int(st['step'])
        self.steps = steps
        for k, val in base.items():
            if k != 'params':
                self.param_groups[0][k] = tuple(val) if k == 'betas' else val


def group_runs(offsets, multipliers):
    """-> (begin, lr_mult, decay_mult): the maximal stretches of consecutive parameters with equal multipliers, each by the float
    offset of its first parameter in the flat buffers"""
    begin, lr, dec = [], [], []
    for o, (a, b) in zip(offsets, multipliers):
        if not begin or (a, b) != (lr[-1], dec[-1]):
            begin.append(int(o)); lr.append(float(a)); dec.append(float(b))
    return begin, lr, dec


def pack_runs(begin, lr_mult, decay_mult, n):
    """fc_adamw_groups_pack (csrc_post/optim_groups.hip, a pure host function): the validated run table as the kernel reads it
    -> uint8 array.  ValueError on what the library refuses (include/fcaf3d_hip.h lists it)"""
    import ctypes
    R = len(begin)
    b = np.ascontiguousarray(begin, dtype=np.int64)
    a = np.ascontiguousarray(lr_mult, dtype=np.float32)
    d = np.ascontiguousarray(decay_mult, dtype=np.float32)
    out = np.zeros(max(int(L.lib().fc_adamw_groups_table_bytes(R)), 1), dtype=np.uint8)
    rc = L.lib().fc_adamw_groups_pack(b.ctypes.data_as(ctypes.c_void_p), a.ctypes.data_as(ctypes.c_void_p), d.ctypes.data_as(ctypes.c_void_p),
                                      R, int(n), out.ctypes.data_as(ctypes.c_void_p), out.nbytes if R else 0)
    if rc != 0:
        raise ValueError(f'fc_adamw_groups_pack refused the run table (status {rc}): {R} runs over {n} floats, at most {MAX_RUNS} runs')
    return out


MAX_RUNS = 1024        # include/fcaf3d_hip.h FC_ADAMW_MAX_RUNS
_PARAMWISE_KEYS = ('custom_keys', 'bias_lr_mult', 'bias_decay_mult', 'norm_decay_mult')


def param_multipliers(model, paramwise_cfg):
    """-> {parameter name: (lr_mult, decay_mult)} for every parameter of `model`: mmcv's DefaultOptimizerConstructor.add_params
    (third party, not in the reference tree; the configs of configs/fcaf3d/ pass no paramwise_cfg).  The rule, restated:

      custom_keys = {key: dict(lr_mult=1, decay_mult=1)}: of the keys that are SUBSTRINGS of the parameter's full name the longest
          wins, ties broken alphabetically; its lr_mult / decay_mult (default 1) are the parameter's multipliers.
      Only when no custom key matches:
          bias_lr_mult      the learning rate of parameters named `bias` outside normalisation layers
          norm_decay_mult   the weight decay of every parameter of a normalisation layer
          bias_decay_mult   the weight decay of parameters named `bias` outside normalisation layers

    A normalisation layer is what mmcv tests for: torch's _BatchNorm / _InstanceNorm / GroupNorm / LayerNorm — here the
    nn.BatchNorm1d inside a MinkowskiBatchNorm.  MinkowskiInstanceNorm is a plain nn.Module to that test (as ME's is to mmcv), so
    the stem's instance-norm `bias` takes the BIAS multipliers and its `weight` none.  Any other key of mmcv's constructor
    (dwconv_decay_mult, dcn_offset_lr_mult, bypass_duplicate, ...) raises KeyError: no FCAF3D layer is of those kinds."""
    cfg = dict(paramwise_cfg or {})
    for k in cfg:
        if k not in _PARAMWISE_KEYS:
            raise KeyError(f'paramwise_cfg key {k!r} is not implemented ({", ".join(_PARAMWISE_KEYS)})')
    custom = cfg.get('custom_keys') or {}
    for k, val in custom.items():
        for kk in val:
            if kk not in ('lr_mult', 'decay_mult'):
                raise KeyError(f'paramwise_cfg custom_keys[{k!r}] key {kk!r} is not implemented (lr_mult, decay_mult)')
    keys = sorted(sorted(custom), key=len, reverse=True)
    norms = (torch.nn.modules.batchnorm._BatchNorm, torch.nn.modules.instancenorm._InstanceNorm, torch.nn.GroupNorm, torch.nn.LayerNorm)
    out = {}
    for prefix, mod in model.named_modules():
        is_norm = isinstance(mod, norms)
        for name, _ in mod.named_parameters(recurse=False):
            full = f'{prefix}.{name}' if prefix else name
            if full in out:
                continue
            key = next((k for k in keys if k in full), None)
            if key is not None:
                out[full] = (float(custom[key].get('lr_mult', 1.0)), float(custom[key].get('decay_mult', 1.0)))
                continue
            lr_mult = decay_mult = 1.0
            if name == 'bias' and not is_norm and cfg.get('bias_lr_mult') is not None:
                lr_mult = float(cfg['bias_lr_mult'])
            if is_norm:
                if cfg.get('norm_decay_mult') is not None:
                    decay_mult = float(cfg['norm_decay_mult'])
            elif name == 'bias' and cfg.get('bias_decay_mult') is not None:
                decay_mult = float(cfg['bias_decay_mult'])
            out[full] = (lr_mult, decay_mult)
    return out


def build_optimizer(model, cfg, flat=None):
    """cfg: the `optimizer` dict of a config (type AdamW / Adam / SGD, mmcv's constructor keys; `paramwise_cfg`: per-parameter
    multipliers, param_multipliers).  `flat`: the model's FlatParams (GPU): AdamW then runs on the flat buffers (FlatAdamW, which
    keeps one schedule group and applies the multipliers in its kernel); the torch optimizers get one group per parameter with
    lr = base * lr_mult and weight_decay = base * decay_mult, as mmcv builds them."""
    cfg = dict(cfg)
    kind = cfg.pop('type')
    paramwise = cfg.pop('paramwise_cfg', None)
    if kind not in ('AdamW', 'Adam', 'SGD'):
        raise KeyError(f'optimizer type {kind!r} is not used by any FCAF3D config')
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    params = [p for _, p in named]
    mults = None
    if paramwise:
        by_name = param_multipliers(model, paramwise)
        mults = {id(p): by_name[n] for n, p in named}
    fused = all(p.is_cuda for p in params)
    if kind == 'AdamW' and flat is not None:
        return FlatAdamW(flat, multipliers=[mults[id(p)] for p in flat.params] if mults else None, **cfg)
    if mults:
        base_wd = cfg.get('weight_decay')
        groups = []
        for p in params:
            a, b = mults[id(p)]
            gr = dict(params=[p], lr=cfg['lr'] * a)
            if base_wd is not None:
                gr['weight_decay'] = base_wd * b
            groups.append(gr)
        params = groups
    if kind == 'AdamW':
        return torch.optim.AdamW(params, fused=fused, **cfg)
    if kind == 'Adam':
        return torch.optim.Adam(params, fused=fused, **cfg)
    return torch.optim.SGD(params, **cfg)


_EMA_KEYS = ('type', 'momentum', 'interval', 'warm_up', 'resume_from')


def ema_hook_of(custom_hooks):
    """-> the EMAHook dict among `cfg.custom_hooks`, or None.  EMAHook is the one custom hook implemented: any other type raises
    KeyError naming it, and so does a key of the hook's dict that mmcv 1.3.x's EMAHook does not take"""
    found = None
    for hook in (custom_hooks or []):
        kind = hook.get('type')
        if kind != 'EMAHook':
            raise KeyError(f'custom hook type {kind!r} is not implemented (EMAHook)')
        for k in hook:
            if k not in _EMA_KEYS:
                raise KeyError(f'EMAHook key {k!r} is not implemented ({", ".join(_EMA_KEYS[1:])})')
        if found is not None:
            raise ValueError('custom_hooks holds more than one EMAHook')
        found = dict(hook)
    return found


class WeightEma:
    """mmcv 1.3.x EMAHook(momentum=0.0002, interval=1, warm_up=100, resume_from=None) (third party, not in the reference tree),
    restated:

      stored momentum   M = momentum ** interval                                  (0 < momentum < 1, interval an int >= 1)
      start             every parameter gets an average e, a copy of the parameter (`attach` / `reset`)
      step s (0-based)  s % interval != 0: nothing.  Otherwise mu = min(M, (1 + s) / (warm_up + s)) in Python floats (a zero
                        denominator, warm_up = 0 at s = 0, counts as no bound) and, with p the parameter AFTER the optimizer step,
                        e <- fl32( fl32(e * fl32(1 - mu)) + fl32(fl32(mu) * p) ): three fp32 roundings, no fused multiply-add
      swap()            parameters <-> averages: `fit` swaps after every training epoch (checkpoint and validation see the
                        average) and swaps back before the next; after the last epoch the model keeps the averaged weights

    Parameters only (named_parameters): BatchNorm's running statistics are not averaged.  The average is NOT a module buffer:
    model.state_dict(), the broadcast list and the executor's address tables stay as they are; `state_dict()` names the averages as
    mmcv's buffers are named, 'ema_' + name.replace('.', '_'), for the checkpoint.
    With a FlatAdamW the averages are ONE buffer laid out like flat.data and the update rides in the optimizer's launch
    (fc_adamw_ema_step, `coeffs`); parameters outside a flat buffer (CPU, flat=False, other optimizers) keep a tensor each and take
    three torch ops (`update`).  A frozen parameter's average is the parameter itself."""

    def __init__(self, momentum=0.0002, interval=1, warm_up=100, resume_from=None):
        if not (isinstance(interval, int) and not isinstance(interval, bool) and interval >= 1):
            raise ValueError(f'EMAHook interval {interval!r}: an int >= 1')
        if not 0.0 < float(momentum) < 1.0:
            raise ValueError(f'EMAHook momentum {momentum!r}: 0 < momentum < 1')
        if warm_up < 0:
            raise ValueError(f'EMAHook warm_up {warm_up!r}: >= 0')
        self.momentum = float(momentum) ** interval           # mmcv stores the power
        self.interval, self.warm_up, self.resume_from = interval, warm_up, resume_from
        self.swapped = False
        self.step = None                                       # the TrainStep whose parameters are averaged (attach)
        self.buf = None                                        # flat path: the optimizer's average buffer
        self.named, self.tensors = [], {}                      # [(name, parameter)]; id(parameter) -> its own average tensor

    @classmethod
    def from_config(cls, hook):
        """hook: an EMAHook dict (ema_hook_of), a WeightEma (returned as it is) or None"""
        if hook is None or isinstance(hook, cls):
            return hook
        hook = ema_hook_of([hook])
        return cls(**{k: v for k, v in hook.items() if k != 'type'})

    def momentum_at(self, s):
        """-> mu of 0-based step s, or None when no update is due"""
        if s % self.interval:
            return None
        den = self.warm_up + s
        return min(self.momentum, (1 + s) / den) if den else self.momentum

    def coeffs(self, s):
        """-> (fl32(mu), fl32(1 - mu)) as Python floats, or None when no update is due"""
        mu = self.momentum_at(s)
        return None if mu is None else (float(np.float32(mu)), float(np.float32(1.0 - mu)))

    @staticmethod
    def name_of(param_name):
        return 'ema_' + param_name.replace('.', '_')

    def names(self):
        return [self.name_of(n) for n, _ in self.named]

    def attach(self, step):
        """take the averages of `step`'s model as copies of its parameters (they are final: after load_from and the broadcast)"""
        self.step = step
        self.named = list(step.model.named_parameters())
        seen = {}
        for n, _ in self.named:
            e = self.name_of(n)
            if e in seen:
                raise ValueError(f'parameters {seen[e]!r} and {n!r} both map to the EMA buffer name {e!r}')
            seen[e] = n
        own = set(step.model.state_dict())
        clash = [e for e in seen if e in own]
        if clash:
            raise ValueError(f'EMA buffer name {clash[0]!r} is an entry of the model itself')
        self.reset()

    def on_flat(self):
        return self.step.flat is not None and isinstance(self.step.optimizer, FlatAdamW)

    @torch.no_grad()
    def reset(self):
        """every average <- its parameter; not swapped"""
        self.swapped, self.buf, self.tensors = False, None, {}
        if self.on_flat():
            opt = self.step.optimizer
            self.buf = opt.enable_ema()
            self.buf.copy_(opt.flat.data)
        else:
            self.tensors = {id(p): p.detach().clone() for _, p in self.named if p.requires_grad}

    def _avg(self, p):
        """the average of parameter p: a view of the flat buffer, its own tensor, or (frozen) the parameter itself"""
        if p.requires_grad and self.buf is not None:
            o = p._fc_flat[1]
            return self.buf[o:o + p.numel()].view(p.shape)
        return self.tensors.get(id(p), p.detach())

    @torch.no_grad()
    def update(self, s):
        """the per-tensor path, after the optimizer step of iteration s: three torch ops, three roundings (add_(p, alpha=mu) may fuse)"""
        c = self.coeffs(s)
        if c is None or not self.tensors:
            return
        mu, keep = c
        for _, p in self.named:
            e = self.tensors.get(id(p))
            if e is not None:
                e.mul_(keep)
                t = p.detach() * mu
                e.add_(t)

    @torch.no_grad()
    def swap(self):
        """parameters <-> averages.  The weights change behind every version counter: the image sets are invalidated, so the next
        forward pass, training or inference, rebuilds the weight images before it reads them"""
        tr = self.step
        if self.buf is not None:
            for s in (tr.images, getattr(tr.model, '_exec_weights', None)):
                if s is not None:
                    s.wait()                  # a build of the stepped weights' images on the side stream still reads them
            f = tr.flat
            L.call('fc_swap_f32', L.ptr(f.data), L.ptr(self.buf), f.n, L.stream())
        for _, p in self.named:
            e = self.tensors.get(id(p))
            if e is not None:
                t = p.detach().clone()
                p.data.copy_(e)
                e.copy_(t)
        self.swapped = not self.swapped
        tr.invalidate_images()

    def state_dict(self):
        """{mmcv's buffer name: the average} of every parameter, as copies (what the `ema_*` slots hold now: the raw weights while
        swapped)"""
        from collections import OrderedDict
        return OrderedDict((self.name_of(n), self._avg(p).detach().clone()) for n, p in self.named)

    @torch.no_grad()
    def load_state_dict(self, sd, swapped=True):
        """the `ema_*` entries of a checkpoint `fit` wrote after an epoch: they hold the raw weights, the model's own entries the
        averages, so the state is `swapped`"""
        missing = [k for k in self.names() if k not in sd]
        if missing:
            raise KeyError(f'EMA state lacks {len(missing)} of {len(self.named)} entries, the first: {missing[0]!r}')
        for n, p in self.named:
            if p.requires_grad:
                self._avg(p).copy_(sd[self.name_of(n)])
        self.swapped = bool(swapped)


class StepLrUpdater:
    """mmcv StepLrUpdaterHook with by_epoch=True: lr = base_lr * gamma ** (number of `step` entries <= epoch).
    warmup='linear' (mmcv LrUpdaterHook, warmup_by_epoch=False): before iteration `it` < warmup_iters (global, counted from 0) the
    rate is regular_lr * (1 - (1 - it / warmup_iters) * (1 - warmup_ratio)); from warmup_iters on, the epoch's regular rate.  The
    caller hands the iteration over with `set_iter` before every step (runner.fit does)."""

    def __init__(self, optimizer, step, gamma=0.1, min_lr=None, warmup=None, warmup_iters=0, warmup_ratio=0.1, warmup_by_epoch=False,
                 **_ignored):
        if warmup not in (None, 'linear'):
            raise KeyError(f"lr warmup {warmup!r} is not implemented (None or 'linear')")
        assert not warmup_by_epoch, 'warm-up is counted in iterations'
        if warmup is not None:
            assert warmup_iters > 0 and 0 < warmup_ratio <= 1.0
        self.warmup, self.warmup_iters, self.warmup_ratio = warmup, int(warmup_iters), float(warmup_ratio)
        self.optimizer = optimizer
        self.steps = [step] if isinstance(step, int) else sorted(step)
        self.gamma, self.min_lr = gamma, min_lr
        self.base_lrs = [g['lr'] for g in optimizer.param_groups]
        self.epoch = 0

    def lr_at(self, base_lr, epoch, it=None):
        exp = sum(1 for s in self.steps if epoch >= s)
        lr = base_lr * self.gamma ** exp
        lr = max(lr, self.min_lr) if self.min_lr is not None else lr
        if self.warmup is not None and it is not None and it < self.warmup_iters:
            lr = lr * (1 - (1 - it / self.warmup_iters) * (1 - self.warmup_ratio))
        return lr

    def set_epoch(self, epoch):
        self.epoch = epoch
        for g, base in zip(self.optimizer.param_groups, self.base_lrs):
            g['lr'] = self.lr_at(base, epoch)

    def set_iter(self, it):
        """before global iteration `it`: the warm-up rate while it lasts (mmcv before_train_iter); a no-op without warm-up"""
        if self.warmup is None or it > self.warmup_iters:
            return
        for g, base in zip(self.optimizer.param_groups, self.base_lrs):
            g['lr'] = self.lr_at(base, self.epoch, it)

    def epoch_end(self):
        self.set_epoch(self.epoch + 1)


def build_lr_updater(optimizer, cfg):
    cfg = dict(cfg)
    policy = cfg.pop('policy')
    if policy != 'step':
        raise KeyError(f'lr policy {policy!r} is not used by any FCAF3D config')
    return StepLrUpdater(optimizer, **cfg)


def parse_losses(losses):
    """mmdet BaseDetector._parse_losses: every entry is reduced to a scalar (a tensor by its mean, a list of tensors by
    the sum of their means) and the training loss is the sum of the entries whose key contains 'loss'."""
    def mean(t):                     # the mean of a 0-dim tensor is the tensor: no reduction launch, none in its backward
        return t if t.dim() == 0 else t.mean()
    total = None
    for k, v in losses.items():
        if 'loss' in k:
            v = mean(v) if torch.is_tensor(v) else sum(mean(x) for x in v)
            total = v if total is None else total + v
    return total


def reserve_device_memory(gigabytes, device=None, streams=None, chunk_gb=8):
    """Take `gigabytes` of device memory into torch's caching allocator up front (as chunk_gb blocks, released to the cache at once:
    later requests are carved out of them).  A training step asks the allocator for its arenas (the coordinate phase's tables, the
    executor's activations and workspaces) every step; which cached block fits depends on how far the host runs ahead of the GPU, and a
    step that finds none goes to the driver — a device allocation of a few hundred MB takes 20-120 ms on this stack, inside the step
    (profiles/r6_notes.md section 14: every "slow first process" of r5 / r6 was one to five such calls inside the 20 timed steps).  On a
    288 GB device holding back a few tens of GB removes them.
    The allocator keeps one pool PER STREAM: `streams` = [(stream, share)] splits the reserve over the streams the step allocates under
    (default: the current stream 1/2, the coordinate stream 1/4, the weight-gradient stream 1/4).  Returns the bytes reserved (at most
    a quarter of what is free)."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if streams is None:
        from . import sparse as SP
        streams = [(torch.cuda.current_stream(dev), 0.5), (SP.map_stream(dev), 0.25), (Fn.wgrad_stream(dev), 0.25)]
    free, _ = torch.cuda.mem_get_info(dev)
    budget = min(float(gigabytes), free / 4 / 2 ** 30)
    tot = sum(w for _, w in streams) or 1.0
    got = 0
    for st, w in streams:
        n = int(budget * w / tot // chunk_gb)
        with torch.cuda.stream(st):
            blocks = []
            try:
                for _ in range(max(n, 0)):
                    blocks.append(torch.empty(chunk_gb << 30, dtype=torch.uint8, device=dev))
            except torch.OutOfMemoryError:         # somebody else took the memory meanwhile (several processes on one device): keep what there is
                pass
            got += sum(b.numel() for b in blocks)
            del blocks
    return got


_OPTIMIZER_HOOKS = (None, 'OptimizerHook', 'GradientCumulativeOptimizerHook')
_OPTIMIZER_CONFIG_KEYS = ('type', 'grad_clip', 'cumulative_iters')


def cumulative_iters_of(optimizer_config):
    """-> k of `optimizer_config` (mmcv: OptimizerHook, the default type, or GradientCumulativeOptimizerHook(cumulative_iters=k)); 1
    without accumulation.  Any other hook type raises KeyError naming it, and so does any key beside grad_clip and cumulative_iters;
    a k that is not an int >= 1 raises ValueError"""
    cfg = optimizer_config or {}
    kind = cfg.get('type')
    if kind not in _OPTIMIZER_HOOKS:
        raise KeyError(f'optimizer hook type {kind!r} is not implemented ({", ".join(_OPTIMIZER_HOOKS[1:])})')
    for key in cfg:
        if key not in _OPTIMIZER_CONFIG_KEYS:
            raise KeyError(f'optimizer_config key {key!r} is not implemented ({", ".join(_OPTIMIZER_CONFIG_KEYS[1:])})')
    if 'cumulative_iters' not in cfg:
        return 1
    k = cfg['cumulative_iters']
    if not (isinstance(k, int) and not isinstance(k, bool) and k >= 1):
        raise ValueError(f'cumulative_iters {k!r}: an int >= 1')
    if kind != 'GradientCumulativeOptimizerHook' and k != 1:
        raise KeyError(f"cumulative_iters={k} needs optimizer_config type 'GradientCumulativeOptimizerHook', not {kind!r}")
    return k


def accum_factor(it, k, max_iters=None):
    """mmcv GradientCumulativeOptimizerHook: what the gradients of 0-based global iteration `it` are divided by: k, or in the run's
    last, shorter group (max_iters % k iterations) that group's length.  max_iters None: k throughout"""
    if max_iters is None:
        return k
    r = max_iters % k
    return k if it < max_iters - r else r


def accum_steps(it, k, max_iters=None):
    """whether the optimizer steps after 0-based global iteration `it`: every k-th, and the run's last"""
    return (it + 1) % k == 0 or (max_iters is not None and it == max_iters - 1)


class TrainStep:
    """One optimisation step of the reference's recipe on this process's GPU (one process per GPU; gradients are averaged
    over the process group, if any, by fcaf3d_amd.dist.GradientAverager while backward is still running).

    Gradient accumulation (optimizer_config type 'GradientCumulativeOptimizerHook', cumulative_iters=k > 1): a
    call is then a MICRO-iteration.  Its gradients, divided by accum_factor(it), are added to the open group's sum, and the optimizer
    steps on the iterations accum_steps(it) names — groups are counted on the global iteration `it` (set_iter) and may straddle an epoch.
    On the flat path the sum is FlatAdamW.acc and the division happens after the backward pass (fc_grad_accum / fc_grad_accum_norm);
    on the per-tensor path it is mmcv's `loss / factor` with the sum left in `p.grad`.  `acc_iters` is the open group's length so far."""

    def __init__(self, model, optimizer_cfg, optimizer_config=None, lr_config=None, bucket_mb=64, flat=None, ema=None, max_iters=None):
        """ema: an EMAHook dict (cfg.custom_hooks' entry) or a WeightEma: the parameters' moving average is updated with every step
        (`self.ema`; on the flat path inside the optimizer's launch).  The average starts as a copy of the weights the model holds NOW.
        max_iters: the run's total of iterations (fit passes max_epochs x iterations per epoch), for the factor of the last, shorter
        accumulation group; None: every group counts cumulative_iters (`flush` steps an open one)"""
        self.model = model
        self.cumulative_iters = cumulative_iters_of(optimizer_config)
        self.max_iters = None if max_iters is None else int(max_iters)
        self.acc_iters = 0                           # micro-iterations in the open accumulation group
        self.params = [p for p in model.parameters() if p.requires_grad]
        clip = (optimizer_config or {}).get('grad_clip')
        self.max_norm = clip['max_norm'] if clip else None
        self.norm_type = clip.get('norm_type', 2) if clip else 2
        # GPU: parameters and gradients move into flat buffers (flat.FlatParams re-points every p.data; call after
        # model.to(device) and do not move the model afterwards); `flat=False` keeps the per-tensor torch path
        on_gpu = all(p.is_cuda for p in self.params)
        use_flat = (on_gpu and optimizer_cfg.get('type') == 'AdamW' and self.norm_type == 2) if flat is None else flat
        self.flat = FlatParams(self.params) if use_flat else None
        self.optimizer = build_optimizer(model, optimizer_cfg, flat=self.flat)
        self.lr = build_lr_updater(self.optimizer, lr_config) if lr_config else None
        self.averager = D.GradientAverager(self.params, bucket_mb=bucket_mb, flat=self.flat)
        self.last_grad_norm = None
        # host seconds per phase, accumulated over the calls: [run-ahead bound + prefetch submit + zero_grad, forward_train enqueue, backward enqueue,
        # averager + clip + AdamW + weight images] (bench.py config.host.phases_ms: which phase grows when the host is slow)
        self.phase_s = [0.0, 0.0, 0.0, 0.0]
        # split-bf16 convolutions read pre-split weight images (weight_images.ImageSet): with the flat optimizer this loop is the only
        # writer of the weights, so it builds them all in one launch right after its step (weight-gradient stream, under the next step's
        # voxelisation and stem) instead of ~100 per-layer launches there, and leases them to its own pass.  This set serves the module path.
        self.images = None
        if self.flat is not None and Fn.X6:
            from .nn import MinkowskiConvolution
            self.images = ImageSet(m.kernel for m in model.modules() if isinstance(m, MinkowskiConvolution) and m.kernel.requires_grad)
        self._step_events = []
        self.it = 0                                  # the 0-based index of the next step (set_iter; counted here otherwise)
        self.ema = WeightEma.from_config(ema)
        if self.ema is not None:
            self.ema.attach(self)

    @classmethod
    def from_config(cls, model, cfg, **kw):
        """kw: bucket_mb, flat, ema, max_iters of the constructor"""
        if kw.get('ema') is None:
            kw['ema'] = ema_hook_of(cfg.get('custom_hooks'))
        return cls(model, cfg.optimizer, cfg.get('optimizer_config'), cfg.get('lr_config'), **kw)

    def set_iter(self, it):
        """before global iteration `it` (counted from 0): the LR updater's warm-up rate and the step index of the weight average"""
        self.it = int(it)
        if self.lr is not None:
            self.lr.set_iter(it)

    def invalidate_images(self):
        """Call after writing the weights in a way that does not move their version counters (`p.data.copy_`,
        `dist.broadcast(p.data)`, EMA / weight surgery through `.data`): the next step rebuilds the pre-split weight images
        (the module path's and the native executor's) before it uses them.  Writes through torch ops on the parameters
        themselves (load_state_dict, `with no_grad(): p.copy_()`) are detected by the version counters."""
        for s in (self.images, getattr(self.model, '_exec_weights', None)):
            if s is not None:
                s.invalidate()

    def __call__(self, batch, next_batch=None):
        """next_batch: the batch of the FOLLOWING call, if the caller has it (a data loader's prefetched item): its coordinate
        phase starts now on a worker thread (SingleStageSparse3DDetector.prefetch) and overlaps this step"""
        t0 = time.perf_counter()
        images = self.open(next_batch)
        t1 = time.perf_counter()
        with self.passing(images):
            losses = self.model(return_loss=True, **batch)
            loss = parse_losses(losses)
            t2 = time.perf_counter()
            if self.cumulative_iters > 1 and not isinstance(self.optimizer, FlatAdamW):
                (loss / self.factor()).backward()    # the per-tensor path follows mmcv literally; the flat path scales the gradient
            else:
                loss.backward()
            t3 = time.perf_counter()
        self.averager.finish()
        self.close(images)
        for k, dt in enumerate((t1 - t0, t2 - t1, t3 - t2, time.perf_counter() - t3)):
            self.phase_s[k] += dt
        return loss, losses

    def open(self, next_batch=None):      # open / passing / close: the pieces of a step (tools/hostprof.py puts its marks between them)
        """before the pass: bound the run-ahead, start the next batch's coordinate phase, drop the gradients -> the image set this
        step runs under: the executor's if it will go through a program (executor.py), else this loop's own (or None)"""
        self._bound_run_ahead()
        if next_batch is not None and hasattr(self.model, 'prefetch'):
            self.model.prefetch(next_batch['points'], gt=True)
        if self.acc_iters == 0 or isinstance(self.optimizer, FlatAdamW):      # (an open group's sum sits in p.grad on the per-tensor path)
            self.optimizer.zero_grad(set_to_none=True)
        Fn._flat_pass_done()                         # a backward pass that raised never ran its final callback: start clean
        if self.flat is not None and hasattr(self.model, 'backbone') and self.model.training:
            prog = executor.program_for(self.model, True)
            if prog is not None:
                return prog.w
        return self.images

    @contextlib.contextmanager
    def passing(self, images):
        """the forward + backward pass runs inside, under the lease of this step's images (rebuilt first unless they are current)"""
        with images.lease() if images is not None else contextlib.nullcontext():
            if images is not None:
                images.ensure(trusted=True)
            yield

    def close(self, images):
        """after the pass and the averager: clip + optimizer step, then the images of the stepped weights (weight-gradient stream);
        under gradient accumulation, on the iterations that do not step: the accumulation alone"""
        ema = self.ema
        if self.cumulative_iters > 1:
            if not self._close_accumulating():
                return                               # no step: the weights did not move, the images stay current
        elif isinstance(self.optimizer, FlatAdamW):    # (after finish() under data parallelism the averaged gradients sit in the flat buffer)
            if ema is None:
                self.last_grad_norm = self.optimizer.step(self.max_norm, gathered=bool(self.averager.buckets))
            else:                                    # a step whose average update is due takes it in the optimizer's launch
                self.last_grad_norm = self.optimizer.step(self.max_norm, gathered=bool(self.averager.buckets), ema=ema.coeffs(self.it))
        else:
            if self.max_norm is not None:
                self.last_grad_norm = torch.nn.utils.clip_grad_norm_(self.params, self.max_norm, norm_type=self.norm_type)
            self.optimizer.step()
        if ema is not None:
            ema.update(self.it)                      # parameters outside a flat buffer: three torch ops each
        self.it += 1
        self._after_step(images)

    def factor(self):
        """what the gradients of the iteration at hand are divided by (accum_factor)"""
        return accum_factor(self.it, self.cumulative_iters, self.max_iters)

    def _close_accumulating(self):
        """`close` with cumulative_iters > 1, up to the optimizer step -> whether the optimizer stepped.  The average keeps mmcv's
        cadence: its update is due by the iteration, stepped or not"""
        ema, opt = self.ema, self.optimizer
        f, stepping = self.factor(), accum_steps(self.it, self.cumulative_iters, self.max_iters)
        on_flat = isinstance(opt, FlatAdamW)
        coeffs = ema.coeffs(self.it) if ema is not None and on_flat else None
        if on_flat:
            gathered = bool(self.averager.buckets)
            if not stepping:
                opt.accumulate(1.0 / f, self.acc_iters == 0, gathered=gathered, ema=coeffs)
            elif self.acc_iters == 0 and f == 1:     # a group of one (the run's last iteration alone): the plain step, no extra pass
                self.last_grad_norm = opt.step(self.max_norm, gathered=gathered, ema=coeffs)
            else:
                if self.acc_iters == 0:              # a group that lost its earlier iterations (resumed without them): sum from zero
                    if opt.acc is None:
                        opt.acc = torch.zeros_like(opt.flat.grad)
                    opt.acc.zero_()
                self.last_grad_norm = opt.step(self.max_norm, gathered=gathered, ema=coeffs, accum_scale=1.0 / f)
        elif stepping:
            self._torch_step()
        if not stepping:
            self.last_grad_norm = None
            self.acc_iters += 1
            if ema is not None:
                ema.update(self.it)
            self.it += 1
            return False
        self.acc_iters = 0
        return True

    def _torch_step(self):
        if self.max_norm is not None:
            self.last_grad_norm = torch.nn.utils.clip_grad_norm_(self.params, self.max_norm, norm_type=self.norm_type)
        self.optimizer.step()

    def flush(self):
        """step an open accumulation group at once, with the sum it holds (a loop outside `fit` that ends inside a group); nothing
        without one.  Not an iteration: `it` and the weight average stay as they are.  -> whether the optimizer stepped"""
        if self.acc_iters == 0:
            return False
        opt = self.optimizer
        if isinstance(opt, FlatAdamW):
            opt.flat.grad.copy_(opt.acc)             # the sum as the gradient; the plain step's launches follow
            self.last_grad_norm = opt.step(self.max_norm, gathered=True)
        else:
            self._torch_step()
        self.acc_iters = 0
        self.invalidate_images()                     # the next pass rebuilds the weight images before it reads them
        return True

    def _after_step(self, images):
        self.invalidate_images()                     # the step wrote through raw pointers (torch's fused ones too): no version counter moved
        if images is not None:
            images.rebuild_after_step(torch.cuda.current_stream(), Fn.wgrad_stream(self.flat.data.device))

    def _bound_run_ahead(self, depth=int(os.environ.get('FC_RUN_AHEAD', '2'))):
        """the host may enqueue at most `depth` steps ahead of the GPU: with the coordinate phase off the main thread nothing else
        in a step waits for the device, and every step in flight holds its arenas"""
        if not self.params or not self.params[0].is_cuda:
            return
        evs = self._step_events
        if len(evs) >= depth:
            e0 = evs.pop(0)
            if not e0.query():
                t0 = time.perf_counter()
                e0.synchronize()
                L.HOST_WAIT[0] += time.perf_counter() - t0
        e = torch.cuda.Event()
        e.record()
        evs.append(e)

    def epoch_end(self):
        if self.lr is not None:
            self.lr.epoch_end()

    def state_dict(self):
        """while an accumulation group is open also `grad_accum` = dict(iters=its length so far, grads=[the sum per parameter, in
        optimizer order]): mmcv loses the partial sum when it resumes, this keeps it"""
        sd = dict(optimizer=self.optimizer.state_dict(), epoch=self.lr.epoch if self.lr else 0)
        ga = self.grad_accum_state()
        if ga is not None:
            sd['grad_accum'] = ga
        return sd

    def grad_accum_state(self):
        """-> dict(iters, grads) of the open accumulation group (copies), or None"""
        if not self.acc_iters:
            return None
        if isinstance(self.optimizer, FlatAdamW):
            grads = [v.clone() for v in self.optimizer._views(self.optimizer.acc)]
        else:
            grads = [p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p) for p in self.params]
        return dict(iters=self.acc_iters, grads=grads)

    def load_state_dict(self, sd):
        self.invalidate_images()
        self.optimizer.load_state_dict(sd['optimizer'])
        if self.lr is not None:
            self.lr.set_epoch(sd.get('epoch', 0))
        ga = sd.get('grad_accum')
        self.acc_iters = 0
        if ga is not None and self.cumulative_iters > 1:
            opt = self.optimizer
            params = opt.flat.params if isinstance(opt, FlatAdamW) else self.params
            if len(ga['grads']) != len(params):
                raise ValueError(f"grad_accum holds {len(ga['grads'])} gradients for {len(params)} parameters")
            with torch.no_grad():
                if isinstance(opt, FlatAdamW):
                    if opt.acc is None:
                        opt.acc = torch.zeros_like(opt.flat.grad)
                    for v, t in zip(opt._views(opt.acc), ga['grads']):
                        v.copy_(t)
                else:
                    for p, t in zip(params, ga['grads']):
                        p.grad = t.detach().to(p.device).clone()
            self.acc_iters = int(ga['iters'])


def evaluate(model, batches, gt_annos, metric=(0.25, 0.5), label2cat=None, in_flight=2, scene_ids=None, group=None):
    """What the reference's tools/test.py:184-190 does with mmdet3d/apis/test.py:10 (single_gpu_test / multi_gpu_test) and the
    dataset's indoor_eval: run `model` over a validation set and return the mAP / mAR dict.  `batches` yields (points, img_metas)
    in `gt_annos` order.  `in_flight` batches stay enqueued as in simple_test_async (extract_feat, then get_bboxes(defer=True); the
    next batch's coordinate phase runs on the host while the GPU works on this one); the results stay on the device and go to
    evaluation.indoor_eval_device ONCE, after the last batch.  More than one rank: each passes its own batches, gt_annos and
    global scene_ids (default rank + world_size * i); the ranks' tables are gathered over `group`, every rank returns the same
    dict.  Runs in eval mode under no_grad and leaves the model in the mode it found it in.  label2cat=None names a class by its
    number.
    Test-time augmentation: a batch whose img_metas is nested (img_metas[a][b], points[a][b] as aug_test takes them; a
    data.AugDeviceLoader batch carries all copies as `points.flat`) goes through extract_feat on the flat batch and
    get_bboxes_aug, whose merge runs on the device; its two read-backs are not deferred, so before they are waited for the NEXT
    batch's coordinate phase is started on the planner's worker thread (model.prefetch on its `.flat`)."""
    from .evaluation import indoor_eval_device
    modes = [(m, m.training) for m in model.modules()]                 # every module's own flag: frozen parts stay frozen
    if any(t for _, t in modes):
        model.eval()
    pending, dets = [], []

    def nested(item):
        return len(item[1]) > 0 and isinstance(item[1][0], (list, tuple))

    def flat_of(points):
        return points.flat if hasattr(points, 'flat') else [p for pa in points for p in pa]
    try:
        with torch.no_grad():
            it = iter(batches)
            cur = next(it, None)
            while cur is not None:
                nxt = next(it, None)                                   # one item ahead: the batch after this one
                points, img_metas = cur
                cur = nxt
                if nested((points, img_metas)):
                    x = model.extract_feat(flat_of(points), [m for ma in img_metas for m in ma])
                    if nxt is not None and nested(nxt) and hasattr(nxt[0], 'flat') and hasattr(model, 'prefetch'):
                        model.prefetch(nxt[0].flat, gt=False)
                    while pending:                                     # results stay in batch order
                        dets.extend(pending.pop(0)())
                    dets.extend(model.neck_with_head.get_bboxes_aug(*x, img_metas))
                    continue
                x = model.extract_feat(points, img_metas)
                pending.append(model.neck_with_head.get_bboxes(*x, img_metas, defer=True))
                if len(pending) >= max(int(in_flight), 1):
                    dets.extend(pending.pop(0)())
            while pending:
                dets.extend(pending.pop(0)())
            assert len(dets) == len(gt_annos), f'{len(dets)} scenes of detections for {len(gt_annos)} scenes of ground truth'
            # a deferred batch builds its results on a read-back stream of its device: everything enqueued there must be done
            # before the matching reads the results on the current stream (one wait per device, at the end of the set)
            for dev in {d[1].device for d in dets if d[1].is_cuda}:
                torch.cuda.synchronize(dev)
            return indoor_eval_device(gt_annos, dets, tuple(metric), label2cat, scene_ids=scene_ids, group=group)
    finally:
        if any(m.training != t for m, t in modes):
            for m, t in modes:
                m.training = t
            model.invalidate_images()                          # what the detector's own train() does besides the flags


# ---- the EpochBasedRunner recipe of the configs ---------------------------------------------------------------------------------------------
def _rank():
    return torch.distributed.get_rank() if D.is_dist() else 0


class _Log:
    """mmcv's TextLoggerHook JSON lines: the losses and the gradient norm are summed ON THE DEVICE step by step and read back once per
    `interval` steps (one copy: the host never waits for a step it has just enqueued, so the run-ahead bound keeps working)."""

    def __init__(self, path, interval):
        self.path, self.interval = path, max(int(interval), 1)
        self.records, self.acc, self.keys, self.n, self.t_step, self.t_data = [], None, None, 0, 0.0, 0.0
        self.gn, self.gn_n = None, 0                     # the gradient norm has a count of its own: under accumulation only the stepping iterations bring one

    def add(self, loss, losses, grad_norm, t_step, t_data):
        items = [(k, v.detach()) for k, v in losses.items() if torch.is_tensor(v) and v.dim() == 0] + [('loss', loss.detach())]
        keys, vals = [k for k, _ in items], [v.to(loss.device) for _, v in items]
        row = torch.stack([v.float().reshape(()) for v in vals])
        self.acc = row if self.acc is None else self.acc + row
        if grad_norm is not None:
            gn = (grad_norm.detach() if torch.is_tensor(grad_norm) else torch.as_tensor(float(grad_norm))).to(loss.device).float().reshape(1)
            self.gn, self.gn_n = gn if self.gn is None else self.gn + gn, self.gn_n + 1
        self.keys, self.n, self.t_step, self.t_data = keys, self.n + 1, self.t_step + t_step, self.t_data + t_data

    def flush(self, mode, epoch, it, lr):
        if not self.n:
            return None
        keys, mean = list(self.keys), self.acc / self.n
        if self.gn_n:                                    # averaged over the iterations that stepped; no key if none did
            keys, mean = keys + ['grad_norm'], torch.cat([mean, self.gn / self.gn_n])
        vals = mean.tolist()                             # the interval's ONE read-back
        rec = dict(mode=mode, epoch=epoch, iter=it, lr=lr)
        rec.update({k: float(v) for k, v in zip(keys, vals)})
        rec.update(time=self.t_step / self.n, data_time=self.t_data / self.n)
        self.acc, self.n, self.t_step, self.t_data = None, 0, 0.0, 0.0
        self.gn, self.gn_n = None, 0
        return self.write(rec)

    def write(self, rec):
        import json
        self.records.append(rec)
        if self.path is not None:
            with open(self.path, 'a') as f:
                f.write(json.dumps(rec) + '\n')
        return rec


def _save(model, tr, work_dir, epoch, it, seed, cfg_ck):
    """mmcv CheckpointHook: epoch_{n}.pth (meta: epoch, iter, seed; optimizer state), latest.pth, and at most max_keep_ckpts files"""
    import shutil
    from .checkpoint import save_checkpoint
    path = os.path.join(work_dir, f'epoch_{epoch}.pth')
    # with an EMAHook the file is written while swapped: the model's entries hold the averages, the `ema_*` entries the raw weights
    # an accumulation group open at the epoch's end: its sum goes into the file as the top-level key `grad_accum` (other readers ignore it)
    save_checkpoint(model, path, optimizer=tr.optimizer, meta=dict(epoch=epoch, iter=it, seed=seed),
                    extra_state=tr.ema.state_dict() if tr.ema is not None else None, grad_accum=tr.grad_accum_state())
    shutil.copyfile(path, os.path.join(work_dir, 'latest.pth'))
    keep, interval = cfg_ck.get('max_keep_ckpts', -1), max(int(cfg_ck.get('interval', 1)), 1)
    if keep and keep > 0:
        for e in range(epoch - keep * interval, 0, -interval):
            old = os.path.join(work_dir, f'epoch_{e}.pth')
            if not os.path.exists(old):
                break
            os.remove(old)
    return path


def fit(model, cfg, work_dir, train_loader=None, val_loader=None, resume_from=None, seed=0, device=None, max_gb=64.0, on_batch=None,
        step=None, load_from=None):
    """What the reference's tools/train.py does through mmdet3d/apis/train.py train_model: mmcv's EpochBasedRunner with its
    optimizer, LR, checkpoint, evaluation and text-logger hooks, for `cfg.runner.max_epochs` epochs.

      epoch e:  lr.set_epoch(e) -> every batch of the loader through TrainStep(batch, next_batch) -> epoch_end()
      checkpoint_config  dict(interval=1, max_keep_ckpts=-1): work_dir/epoch_{n}.pth + latest.pth, older files removed
      evaluation         dict(interval=n): runner.evaluate over the validation loader (fixed draws per scene), logged as mode 'val'
      log_config         dict(interval=n): one JSON line per n steps in work_dir/<time>.log.json (mode, epoch, iter, lr, losses,
                         grad_norm, time, data_time), read back from the device once per line
      resume_from        a checkpoint written here: model, optimizer, epoch and iteration continue where it stopped; the batches of
                         the remaining epochs are the straight run's (data.DeviceLoader draws by (seed, epoch, index))
      load_from          (default cfg.load_from, configs/fcaf3d/fcaf3d.py:46) a checkpoint to FINE-TUNE from, as mmdet's
                         train_detector treats it: resume_from wins when both are given; otherwise the weights alone are loaded
                         with strict=False (a head of another n_classes is reported as mismatched and keeps its initialisation)
                         BEFORE the TrainStep builds its flat buffers, the run starts at epoch 1, iteration 0 with a fresh
                         optimizer, and the load report is written once to the log as a record with mode 'load'
      custom_hooks       [dict(type='EMAHook', momentum=0.0002, interval=1, warm_up=100)] (mmcv's, the one hook implemented): a moving
                         average of the parameters (WeightEma).  Per epoch: swap back if swapped -> train -> epoch_end -> swap ->
                         checkpoint -> validation, so both see the averaged weights; the file holds the raw ones as `ema_*` entries,
                         which resume_from puts back (a file without them: the average starts from the loaded weights, one record
                         with mode 'ema').  After the last epoch the model keeps the averaged weights

      optimizer_config   dict(type='GradientCumulativeOptimizerHook', cumulative_iters=k, grad_clip=...) (mmcv's): the gradients of k
                         iterations, each divided by k, make one optimizer step (TrainStep; the run's last max_iters % k iterations are
                         divided by their number).  grad_norm enters a log line from the stepping iterations only.  A group open at an
                         epoch's end goes into the checkpoint (`grad_accum`) and resume_from puts it back (a file without it, inside
                         a group: the group starts empty, one record with mode 'accum')

    train_loader / val_loader: data.DeviceLoader (default: built from cfg.data.train / cfg.data.val, resident on `device`; a validation
    pipeline that asks for test-time augmentation, MultiScaleFlipAug3D(flip=True), gets a data.AugDeviceLoader: build_val_loader).  Under
    torch.distributed every rank calls fit: the loaders shard, rank 0 alone writes files, evaluate gathers over the group.
    on_batch(epoch, iteration, batch): called before every step (tests, progress bars).  step: a TrainStep to reuse (default:
    TrainStep.from_config(model, cfg)).  Returns the log records (dicts, train and val, in order)."""
    from . import data as DT
    rank, world = _rank(), D.world_size()
    if device is None:
        device = next(model.parameters()).device
    if train_loader is None:
        ds = DT.build_dataset(cfg.data.train)
        train_loader = DT.DeviceLoader(DT.ResidentScenes(ds, device, max_gb), ds.pipeline, cfg.data.get('samples_per_gpu', 1), seed, rank, world)
    ev = cfg.get('evaluation') or {}
    ev_interval = int(ev.get('interval', 0) or 0)
    if val_loader is None and ev_interval > 0 and cfg.get('data', {}).get('val') is not None:
        vs = DT.build_dataset(cfg.data.val)
        val_loader = build_val_loader(DT.ResidentScenes(vs, device, max_gb), vs.pipeline, cfg.data.get('samples_per_gpu', 1), seed, rank, world)
    if load_from is None:
        load_from = cfg.get('load_from')
    # the weight average (custom_hooks' EMAHook, or the one of the TrainStep handed in); its own `resume_from` key is `fit`'s
    hook = step.ema if step is not None else WeightEma.from_config(ema_hook_of(cfg.get('custom_hooks')))
    if hook is not None and hook.resume_from is not None:
        if resume_from is not None and str(resume_from) != str(hook.resume_from):
            raise ValueError(f"EMAHook resume_from {hook.resume_from!r} differs from fit's resume_from {resume_from!r}")
        resume_from = hook.resume_from
    load_report = None
    if load_from is not None and resume_from is None:
        from .checkpoint import load_checkpoint
        load_report = load_checkpoint(model, load_from, map_location=device, strict=False)['load_report']
        if step is not None:
            step.invalidate_images()
    if world > 1:
        for t in list(model.parameters()) + list(model.buffers()):
            torch.distributed.broadcast(t.data, 0)            # every rank starts from rank 0's weights, as DDP's constructor does
    max_epochs = int(cfg.runner['max_epochs'])
    max_iters = None                                          # the run's total of iterations: asked for under gradient accumulation only
    if (step.cumulative_iters if step is not None else cumulative_iters_of(cfg.get('optimizer_config'))) > 1:
        max_iters = max_epochs * len(train_loader)
    tr = step if step is not None else TrainStep.from_config(model, cfg, ema=hook, max_iters=max_iters)
    if step is not None and max_iters is not None:
        tr.max_iters = max_iters
    if world > 1 and step is not None:
        tr.invalidate_images()                                # the broadcast wrote the weights through .data behind an existing TrainStep
    ema = tr.ema
    if ema is not None and step is not None:
        ema.reset()                                           # the weights are final only now (load_from, the broadcast)
    start_epoch, it = 0, 0
    ema_note = accum_note = None
    if resume_from is not None:
        from .checkpoint import load_checkpoint
        ck = load_checkpoint(model, resume_from, map_location=device, strict=True, extra_keys=ema.names() if ema is not None else None)
        start_epoch, it = int(ck['meta']['epoch']), int(ck['meta']['iter'])
        tr.load_state_dict(dict(optimizer=ck['optimizer'], epoch=start_epoch, grad_accum=ck.get('grad_accum')))
        if tr.cumulative_iters > 1 and ck.get('grad_accum') is None and it % tr.cumulative_iters:
            accum_note = dict(mode='accum', resume_from=str(resume_from),
                              note=f'the checkpoint holds no grad_accum entry at iteration {it}, inside a group of {tr.cumulative_iters}: '
                                   'the group starts empty')
        if ema is not None:
            if ck['extra_state']:
                ema.load_state_dict(ck['extra_state'], swapped=True)      # the file's own entries are the averages, these the raw weights
            else:
                ema.reset()
                ema_note = dict(mode='ema', resume_from=str(resume_from),
                                note='the checkpoint holds no ema_* entries: the average starts from the loaded weights')
    log_path = None
    if rank == 0:
        os.makedirs(work_dir, exist_ok=True)
        log_path = os.path.join(work_dir, time.strftime('%Y%m%d_%H%M%S') + '.log.json')
    log = _Log(log_path, (cfg.get('log_config') or {}).get('interval', 50))
    if load_report is not None:
        log.write(dict(mode='load', load_from=str(load_from), unexpected=list(load_report['unexpected']), missing=list(load_report['missing']),
                       mismatched=[[k, list(a), list(b)] for k, a, b in load_report['mismatched']]))
    if ema_note is not None:
        log.write(ema_note)
    if accum_note is not None:
        log.write(accum_note)
    ck_cfg = cfg.get('checkpoint_config') or {}
    model.train()
    for epoch in range(start_epoch, max_epochs):
        if ema is not None and ema.swapped:
            ema.swap()                                        # back to the raw weights (mmcv EMAHook.before_train_epoch)
        if tr.lr is not None:
            tr.lr.set_epoch(epoch)
        train_loader.set_epoch(epoch)
        t_data0 = time.perf_counter()
        batches = train_loader.batches(epoch)
        t_data = (time.perf_counter() - t_data0) / max(len(batches), 1)
        for k, batch in enumerate(batches):
            tr.set_iter(it)
            if on_batch is not None:
                on_batch(epoch, it, batch)
            t0 = time.perf_counter()
            loss, losses = tr(batch, batches[k + 1] if k + 1 < len(batches) else None)
            it += 1
            log.add(loss, losses, tr.last_grad_norm, time.perf_counter() - t0, t_data)
            if (k + 1) % log.interval == 0:
                log.flush('train', epoch + 1, k + 1, tr.optimizer.param_groups[0]['lr'])
        log.flush('train', epoch + 1, len(batches), tr.optimizer.param_groups[0]['lr'])
        tr.epoch_end()
        if ema is not None:
            ema.swap()                                        # the checkpoint and the validation see the averaged weights (after_train_epoch)
        if rank == 0 and ck_cfg.get('interval', 1) > 0 and (epoch + 1) % int(ck_cfg.get('interval', 1)) == 0:
            _save(model, tr, work_dir, epoch + 1, it, seed, ck_cfg)
        if val_loader is not None and ev_interval > 0 and (epoch + 1) % ev_interval == 0:
            res = validate(model, val_loader, metric=tuple(ev.get('iou_thr', (0.25, 0.5))))
            res = {k: float(v) if isinstance(v, (int, float, np.generic)) else v for k, v in res.items()}
            log.write(dict(mode='val', epoch=epoch + 1, iter=len(batches), lr=tr.optimizer.param_groups[0]['lr'], **res))
    return log.records


def build_val_loader(resident, pipeline_cfg, samples_per_gpu, seed=0, rank=0, world_size=1):
    """the validation loader of `fit`: data.AugDeviceLoader when the pipeline's MultiScaleFlipAug3D asks for more than one augmentation
    (test-time augmentation: flip=True, several pts_scale_ratio), data.DeviceLoader otherwise"""
    from . import data as DT
    _, augs = DT.parse_aug_pipeline(pipeline_cfg)
    cls = DT.AugDeviceLoader if len(augs) > 1 else DT.DeviceLoader
    return cls(resident, pipeline_cfg, samples_per_gpu, seed, rank, world_size)


def validate(model, val_loader, metric=(0.25, 0.5), label2cat=None):
    """runner.evaluate over a validation data.DeviceLoader: this rank's scenes (rank r: [r::world_size]), the ranks' tables gathered"""
    rs = val_loader.resident
    idx = val_loader.indices(0)
    annos = rs.dataset.gt_annos() if hasattr(rs.dataset, 'gt_annos') else None
    assert annos is not None, 'validation needs a plain dataset (ScanNetDataset / SUNRGBDDataset / S3DISDataset)'
    group = torch.distributed.group.WORLD if D.world_size() > 1 else None
    return evaluate(model, ((b['points'], b['img_metas']) for b in val_loader.batches(0)), [annos[int(i)] for i in idx], metric=metric,
                    label2cat=label2cat, scene_ids=[int(i) for i in idx], group=group)
