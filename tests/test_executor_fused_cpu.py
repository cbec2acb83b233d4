"""CPU: the r7 rewiring of the executor's program (fcaf3d_amd/executor.py) for the benchmark configuration — the stem's tail is one
operator per direction, the neck's unions are written by the up blocks' last normalisation, and the tensors in between are not in
the arena (the numerics: tests/test_gpu_fused_glue.py, tests/test_gpu_exec.py)."""
import functools

import numpy as np
import torch

import fcaf3d_amd as fa
from fcaf3d_amd import executor as E

OP = E.ROW_OP                  # columns of an operator row: the opcode, then E.word(operator, field) (csrc/exec_ops.h)


def _model():
    torch.manual_seed(0)
    cfg = fa.get_config('fcaf3d_scannet-3d-18class', voxel_size=0.02)         # bench.py's detector: 4 levels
    m = cfg.model
    return fa.build_detector(m, train_cfg=m.get('train_cfg'), test_cfg=m.get('test_cfg'))


def _arena_rows(p, which):
    """dimension names of the arena tensors of one direction"""
    names = {v: k for k, v in p.dim_names.items()}
    return [names[d] for _, d, _, _ in p.arena[which]]


def test_training_program_has_no_stem_or_union_intermediates():
    det = _model()
    assert E.supported(det)
    p = E.NetProgram(det, True, True, True, keep_state=False)
    f, b = p.ops_f, p.ops_b
    kinds_f, kinds_b = list(f[:, OP]), list(b[:, OP])
    for gone in (E.OP_UNION_FWD, E.OP_NORM_FWD, E.OP_MAXPOOL_FWD):
        assert gone not in kinds_f
    for gone in (E.OP_MAXPOOL_BWD, E.OP_NORM_BWD):
        assert gone not in kinds_b
    # one operator for the stem's tail per direction, the forward one right behind the statistics
    assert kinds_f.count(E.OP_NORM_POOL_FWD) == 1 and kinds_b.count(E.OP_POOL_NORM_BWD) == 1
    assert kinds_f[kinds_f.index(E.OP_NORM_POOL_FWD) - 1] == E.OP_COL_STATS
    NP, BF = functools.partial(E.word, E.OP_NORM_POOL_FWD), functools.partial(E.word, E.OP_BN_FWD)
    tail = f[kinds_f.index(E.OP_NORM_POOL_FWD)]
    assert tail[NP('y')] == -1, 'a plain step does not store the normalised tensor'
    back = b[kinds_b.index(E.OP_POOL_NORM_BWD)]
    assert tail[NP('parent')] >= 0 and back[E.word(E.OP_POOL_NORM_BWD, 'parent')] == tail[NP('parent')], \
        'the child -> parent map goes from the forward operator to the backward one'
    # the unions: three normalisation operators carry an inverse map and a backbone tensor in their trailing words
    bn = f[f[:, OP] == E.OP_BN_FWD]
    un = bn[bn[:, BF('add_inv')] > 0]
    assert len(un) == p.nl - 1 == 3 and (un[:, BF('add_src')] > 0).all() and (un[:, BF('res')] == -1).all(), \
        'no residual on a layer that writes a union'
    inv_ops = f[f[:, OP] == E.OP_INV_ROWS]
    assert sorted(inv_ops[:, E.word(E.OP_INV_ROWS, 'inv')]) == sorted(un[:, BF('add_inv')] - 1)
    union_tensors = set(un[:, BF('y')])
    # ... whose amax word the apply kernel folds: no stand-alone pass over a union
    assert (un[:, BF('amax_y')] > 0).all()
    assert not [r for r in f[f[:, OP] == E.OP_AMAX] if r[E.word(E.OP_AMAX, 'x')] in union_tensors]
    # their backward does not read y
    ys = set(b[b[:, OP] == E.OP_BN_BWD][:, E.word(E.OP_BN_BWD, 'y')])
    assert not (ys & union_tensors)
    # arena: forward n1-row tensors are the stem's output, its column matrix and the 4-byte parent map; backward: the stem's gradient only
    n1 = p.dim_names['n1']
    assert sorted(bpr for _, d, bpr, _ in p.arena['f'] if d == n1) == [4, 64 * 4, 84 * 4] and _arena_rows(p, 'b').count('n1') == 1
    for i in range(3):
        sizes = sorted(bpr for _, d, bpr, _ in p.arena['f'] if d == p.dim_names[f'g{i}'])
        assert sizes[0] == 4, 'the inverse row map'
    # every operand index is in range, every operator fits its words
    assert f.shape[1] == E.OPW == b.shape[1]
    assert int(max(f[:, OP].max(), b[:, OP].max())) <= E.OP_INV_ROWS


def test_inference_program_is_rewired_too():
    det = _model().eval()
    p = E.NetProgram(det, False, False, True, keep_state=False)
    kinds = list(p.ops_f[:, OP])
    assert E.OP_UNION_FWD not in kinds and E.OP_NORM_FWD not in kinds and kinds.count(E.OP_NORM_POOL_FWD) == 1
    assert _arena_rows(p, 'f').count('n1') == 1


def test_keep_state_program_exposes_the_stem_activation_to_decisions():
    det = _model()
    old = E.KEEP_STATE
    try:
        E.KEEP_STATE = False
        plain = E.program_for(det, True)
        E.KEEP_STATE = True
        kept = E.program_for(det, True)
        assert kept is not plain and kept.keep_state and not plain.keep_state
        assert E.program_for(det, True) is kept
        E.KEEP_STATE = False
        assert E.program_for(det, True) is plain
    finally:
        E.KEEP_STATE = old
    f = kept.ops_f
    tail = f[list(f[:, OP]).index(E.OP_NORM_POOL_FWD)]
    t_in = int(tail[E.word(E.OP_NORM_POOL_FWD, 'y')])
    assert t_in >= 0 and kept.relu_outs[0] == (t_in, 'n1', 64)
    assert len(kept.relu_outs) == len(plain.relu_outs) + 1
    assert _arena_rows(kept, 'f').count('n1') == 4
    # decisions() views it in a bound state (a fake arena on the CPU: the views only), and refuses a program built without it
    dims = np.zeros(kept.n_dims, dtype=np.int64)
    for k, v in kept.dim_names.items():
        dims[v] = 8
    fa_ = torch.zeros(kept._arena_bytes(dims, 'f'), dtype=torch.uint8)
    addr = kept.addr0.copy()
    kept._fill_arena(addr, dims, 'f', fa_.data_ptr())
    relu, pool = kept.decisions(dict(fa=fa_, addr=addr, dims=dims))
    assert relu[0].shape == (8, 64) and pool.shape == (8, 64)
    try:
        plain.decisions(dict(fa=fa_, addr=addr, dims=dims))
    except AssertionError:
        pass
    else:
        raise AssertionError('a program without the stem activation answered decisions()')
