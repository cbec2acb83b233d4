"""CPU: the stem's tail in the executor's programs (fcaf3d_amd/executor.py) — a training program carries the per-child arg-max mask from
the forward operator to the backward one and no arg-max rows; a program built under KEEP_STATE carries both (`decisions` reads the rows); an
inference program has neither mask nor parent map and stores the rows, as before (the numerics: tests/test_gpu_pool_mask.py)."""
import functools

import torch

import fcaf3d_amd as fa
from fcaf3d_amd import executor as E

OP = E.ROW_OP


def _model():
    torch.manual_seed(0)
    cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=0.02)
    m = cfg.model
    return fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg'))


def _tail_rows(p):
    f, b = p.ops_f, p.ops_b
    fwd = f[list(f[:, OP]).index(E.OP_NORM_POOL_FWD)]
    bwd = b[list(b[:, OP]).index(E.OP_POOL_NORM_BWD)] if len(b) and E.OP_POOL_NORM_BWD in list(b[:, OP]) else None
    return fwd, bwd


def _arena(p, which, dim):
    """bytes per row of the arena tensors of dimension `dim`"""
    return sorted(bpr for _, d, bpr, _ in p.arena[which] if d == p.dim_names.get(dim, -1))


def test_training_program_carries_the_mask_and_no_argmax_rows():
    p = E.NetProgram(_model(), True, True, True, keep_state=False)
    NP, PB = functools.partial(E.word, E.OP_NORM_POOL_FWD), functools.partial(E.word, E.OP_POOL_NORM_BWD)
    fwd, bwd = _tail_rows(p)
    assert fwd[NP('mask')] > 0 and bwd[PB('mask')] == fwd[NP('mask')], 'the mask goes from the forward operator to the backward one'
    assert fwd[NP('arg')] == -1 and bwd[PB('arg')] == -1, 'no arg-max rows in a plain training program'
    assert fwd[NP('parent')] >= 0 and bwd[PB('parent')] == fwd[NP('parent')]
    # the mask: 8 bytes per n1 row as two 4-byte words ('n1w' = 2 n1 rows); of n2 rows only the pooled tensor is left in the stem
    assert _arena(p, 'f', 'n1w') == [4]
    assert p.pool_arg[0] == -1


def test_keep_state_program_carries_both():
    p = E.NetProgram(_model(), True, True, True, keep_state=True)
    NP, PB = functools.partial(E.word, E.OP_NORM_POOL_FWD), functools.partial(E.word, E.OP_POOL_NORM_BWD)
    fwd, bwd = _tail_rows(p)
    assert fwd[NP('mask')] > 0 and bwd[PB('mask')] == fwd[NP('mask')]
    assert fwd[NP('arg')] >= 0 and fwd[NP('arg')] == p.pool_arg[0], '`decisions` reads the arg-max rows'
    assert fwd[NP('y')] >= 0
    plain = E.NetProgram(_model(), True, True, True, keep_state=False)
    assert len(_arena(p, 'f', 'n2')) == len(_arena(plain, 'f', 'n2')) + 1, 'one n2-row tensor more: the arg-max rows'


def test_inference_program_has_neither_mask_nor_parent_map():
    p = E.NetProgram(_model().eval(), False, False, True, keep_state=False)
    NP = functools.partial(E.word, E.OP_NORM_POOL_FWD)
    fwd, bwd = _tail_rows(p)
    assert bwd is None
    assert fwd[NP('mask')] == 0 and fwd[NP('parent')] == -1 and fwd[NP('arg')] >= 0 and fwd[NP('y')] == -1
    assert 'n1w' not in p.dim_names
    # the words this change added are the last of the operator's row and 0: the row is what it was
    assert NP('mask') == E.FIELDS[E.OP_NORM_POOL_FWD]['parent'][0] + 1 and not fwd[NP('mask'):].any()
