"""-m gpu: the target assignment (csrc/assign.hip: k_best, k_kth, k_final; k_count has tests/test_gpu_assign_counts.py) against the
float64 restatement of Fcaf3DAssigner.assign in tests/head_cases.py, on cases that are decidable alike in fp32 and float64 (the
conditions are checked on the CPU by tests/test_head_cases_cpu.py): the level rule at limit - 1 / limit, a starved level 0, a rich level
after a starved one; the candidate list exactly full (8192), one over, and the rescan path (9216); ties straddling rank topk + 1;
exhausted candidates (kth = -1); scenes of fewer than topk + 1 locations; a best-level segment without rows; segments of 255 .. 1027
rows with the most central candidates in the tail; equal volumes (first wins), nested boxes (smaller wins), best levels that differ,
a scene without boxes in the middle of the batch; rotated boxes in general position.

Every launch goes through the C ABI (fc_assign_targets), finds ct / bt at NaN, the labels at -7, the workspace at 0x5a bytes and the
padded box slots at NaN / label -99; `best` and `kth` are read back from the workspace (fc_assign_targets: counts, best, kth, trig).
Labels, box targets, best levels and the positive set are compared exactly, ct at atol 1e-6 on positives (the bar of
test_hip_assigner_vs_reference_goldens) and == 0 elsewhere, kth == -1.0 exactly where the reference pads.  Each case runs with the
identity `order` and with the scenes interleaved inside every level; the two must agree row for row, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from fcaf3d_amd import _lib as L
from tests import head_cases as HC

pytestmark = pytest.mark.gpu
CASES = HC.assigner_cases()


@functools.lru_cache(maxsize=None)
def _reference(name):
    return HC.assign_reference(next(c for c in CASES if c.name == name))


def _stop_after_a_gpu_fault(e):
    """a HIP error leaves the process without a usable device: nothing more is launched from this session"""
    text = str(e)
    if 'hipError' in text or 'HIP error' in text or 'illegal memory access' in text:
        pytest.exit(f'GPU fault, no further launches: {text[:300]}', returncode=3)


def _launch(case, interleave):
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    dev = torch.device('cuda:0')
    lay = HC.layout(case, interleave)
    boxes, labels, count = case.padded()
    B, M, Lv, N = case.B, case.M, case.L, len(lay['pts'])

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = {k: up(lay[k]) for k in ('pts', 'scene', 'level', 'order', 'seg_start')}
    d_boxes, d_labels, d_count = up(boxes), up(labels), up(count)
    assert d['pts'].dtype == torch.float32 and d['order'].dtype == torch.int32 and d_labels.dtype == torch.int64
    assert int(lay['order'].max()) < N and int(lay['seg_start'][-1]) == N and len(lay['seg_start']) == Lv * B + 1
    ct = torch.full((N,), float('nan'), device=dev)
    bt = torch.full((N, 7), float('nan'), device=dev)
    lab = torch.full((N,), -7, dtype=torch.int64, device=dev)
    ws = torch.full((L.query('fc_assign_ws_bytes', B, M, Lv),), 0x5a, dtype=torch.uint8, device=dev)
    L.call('fc_assign_targets', L.ptr(d['pts']), L.ptr(d['scene']), L.ptr(d['level']), N, L.ptr(d_boxes), L.ptr(d_labels), L.ptr(d_count), B, M, Lv,
           L.ptr(d['order']), L.ptr(d['seg_start']), HC.LIMIT, HC.TOPK, L.ptr(ct), L.ptr(bt), L.ptr(lab), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    nb = B * M
    words = ws[:nb * (Lv + 2) * 4].view(torch.int32).cpu()
    out = dict(counts=words[:nb * Lv].view(B, M, Lv).numpy(), best=words[nb * Lv:nb * (Lv + 1)].view(B, M).numpy(),
               kth=words[nb * (Lv + 1):nb * (Lv + 2)].view(torch.float32).view(B, M).numpy())
    canon = lay['canon']
    for key, t in (('ct', ct), ('bt', bt), ('labels', lab)):
        a = t.cpu().numpy()
        full = np.empty_like(a)
        full[canon] = a                                  # back to the canonical rows
        out[key] = full
    return out


def _findings(case, got, ref):
    f = []
    real = np.zeros((case.B, case.M), dtype=bool)
    for s in range(case.B):
        real[s, :len(case.boxes[s])] = True
    if np.isnan(got['ct']).any() or np.isnan(got['bt']).any() or (got['labels'] == -7).any():
        f.append('an output row was not written, or holds a NaN')
    if (got['labels'] == -99).any():
        f.append('a padded box slot reached the labels')
    if not np.array_equal(got['counts'][real], ref['counts'][real]):
        f.append(f"counts {got['counts'][real].tolist()} != {ref['counts'][real].tolist()}")
    if not np.array_equal(got['best'][real], ref['best'][real]):
        f.append(f"best {got['best'][real].tolist()} != {ref['best'][real].tolist()}")
    kg, kr = got['kth'][real].astype(np.float64), ref['kth'][real]
    if not np.array_equal(kg == -1.0, kr == -1.0):
        f.append(f'kth == -1 at {(kg == -1.0).tolist()}, the reference pads at {(kr == -1.0).tolist()}')
    elif not np.all(np.abs(kg - kr)[kr != -1.0] <= 1e-6):
        f.append(f'kth {kg.tolist()} != {kr.tolist()}')
    if not np.array_equal(got['labels'], ref['labels']):
        bad = np.nonzero(got['labels'] != ref['labels'])[0]
        f.append(f"labels differ on {len(bad)} rows (first {bad[:6].tolist()}: {got['labels'][bad[:6]].tolist()} != {ref['labels'][bad[:6]].tolist()}); "
                 f"positives {int((got['labels'] >= 0).sum())} against {int((ref['labels'] >= 0).sum())}")
    if not np.array_equal(got['bt'], ref['bt']):
        f.append(f"box targets differ on {int((got['bt'] != ref['bt']).any(1).sum())} rows")
    pos = ref['labels'] >= 0
    if not np.array_equal(got['ct'] > 0, pos):
        f.append('the positive set of ct differs')
    if pos.any():
        err = float(np.abs(got['ct'][pos].astype(np.float64) - ref['ct'][pos]).max())
        print(f"{case}: {int(pos.sum())} positives, max |ct - reference| {err:.2e}")
        if not err <= 1e-6:
            f.append(f'ct misses the reference by {err:.2e} on positives')
    if not np.all(got['ct'][~pos] == 0.0):
        f.append('ct is not exactly 0 on background rows')
    return f


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_assignment_equals_the_float64_reference_in_both_row_orders(case):
    ref = _reference(case.name)
    HC.check_expectations(case, ref)
    try:
        plain = _launch(case, False)
        mixed = _launch(case, True)
    except RuntimeError as e:
        _stop_after_a_gpu_fault(e)
        raise
    fails = [f'identity order: {m}' for m in _findings(case, plain, ref)] + [f'interleaved: {m}' for m in _findings(case, mixed, ref)]
    real = np.zeros((case.B, case.M), dtype=bool)
    for s in range(case.B):
        real[s, :len(case.boxes[s])] = True
    for key in ('ct', 'bt', 'labels'):
        if not np.array_equal(plain[key].view(np.int32 if plain[key].dtype == np.float32 else np.int64),
                              mixed[key].view(np.int32 if mixed[key].dtype == np.float32 else np.int64)):
            fails.append(f'{key} differs between the two row orders')
    for key in ('best', 'kth'):
        if not np.array_equal(plain[key][real], mixed[key][real]):
            fails.append(f'{key} differs between the two row orders')
    assert not fails, f'{case}: ' + '\n'.join(fails)
