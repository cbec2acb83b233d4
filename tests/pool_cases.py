"""Inputs shared by tests/test_gpu_norm_partial_forms.py and tests/test_gpu_pool_mask.py: a k2s2-like pooling table built without a Python
loop over its rows, and the per-child arg-max mask of csrc/norm_rows.h (POOL_MASK) computed from the arg-max rows."""
import numpy as np
import torch


def pool_table(n_out, nseg, seed, single_child_row=None):
    """-> dict(nbr (8, n_out) int32, parent (n_in,) int64, seg_out (n_out,), seg_in (n_in,), kcount (n_out,), n_in).  Every input row is the
    child of exactly one pooled row; a pooled row has 0..8 children in random offset slots (so children are absent in the middle of the
    offset order), the children of a pooled row lie in one scene, pooled rows are scene-contiguous, the first `nseg` pooled rows (as far as
    there are rows) have at least two children, and row `single_child_row` (if given) has exactly one."""
    rng = np.random.default_rng(seed)
    kcount = rng.integers(0, 9, n_out)
    kcount[:min(nseg, n_out)] = np.maximum(kcount[:min(nseg, n_out)], 2)
    if single_child_row is not None:
        kcount[single_child_row] = 1
    if n_out > 3 * nseg:
        kcount[-1] = 0                                                # a pooled row without any child: 0 / -1
    seg_out = np.sort(rng.integers(0, nseg, n_out))
    seg_out[:min(nseg, n_out)] = np.arange(min(nseg, n_out))          # every scene is there (as far as there are rows)
    seg_out = np.sort(seg_out)
    n_in = int(kcount.sum())
    rank = np.argsort(rng.random((n_out, 8)), axis=1)                 # rank[o, j]: the offset slot of pooled row o's j-th child
    present = np.arange(8)[None, :] < kcount[:, None]
    child_ids = rng.permutation(n_in)
    nbr = np.full((8, n_out), -1, dtype=np.int32)
    o_idx = np.repeat(np.arange(n_out), 8).reshape(n_out, 8)
    nbr[rank[present], o_idx[present]] = child_ids                    # row-major over (o, j): the children of one pooled row are consecutive ids
    parent = np.empty(n_in, dtype=np.int64)
    parent[child_ids] = o_idx[present]
    return dict(nbr=nbr, parent=parent, seg_out=seg_out, seg_in=seg_out[parent], kcount=kcount, n_in=n_in)


def mask_from_argrow(argrow, parent):
    """int64 (n_in,): bit c of word r set exactly where argrow[parent[r]][c] == r (torch tensors on one device; C == 64)"""
    n_in = parent.shape[0]
    rows = torch.arange(n_in, device=parent.device, dtype=torch.int64)
    won = argrow.long()[parent.long()] == rows[:, None]              # (n_in, 64)
    bit = torch.ones(64, dtype=torch.int64, device=parent.device) << torch.arange(64, device=parent.device)     # 1 << 63 wraps to the sign bit
    return (won.long() * bit).sum(1)
