"""The amax slot of fc_amax_out_hint as the exact tests read it (tests/test_gpu_norm_exact.py, tests/test_gpu_head_split_exact.py)."""
import torch


def _new_slot():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.zeros(512, dtype=torch.int32, device=torch.device('cuda:0'))


def _amax_word(slot):
    """the amax as its consumers read it: the maximum of the slot's 32 sub-words (fc_common.h fc_amax_read)"""
    return int(slot.view(32, 16)[:, 0].max())


def _amax_bits(t):
    t = t[torch.isfinite(t)]
    return int(t.abs().max().reshape(1).view(torch.int32)) if t.numel() else 0
