"""CPU: the host half of the device-side evaluation (fcaf3d_amd/evaluation.py: match_table_host, merge_tables, gather_tables,
finish_table) against indoor_eval on the committed goldens, sharded and through two gloo ranks; the tie rule; the argument checks
of fc_eval_match (which return before any launch)."""
import os
import socket

import numpy as np
import torch
import torch.multiprocessing as mp

METRIC = (0.25, 0.5)


def _cases():
    """(name, gt_annos, dt_annos, label2cat, want or None): both cases of tests/golden/indoor_eval.npz and both vectors of the
    reference's own test"""
    from tests.test_oracle_golden import _indoor_eval_case, _ref_indoor_eval_vectors
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'indoor_eval.npz'))
    out = []
    for case in (0, 1):
        gt, dt, l2c, want = _indoor_eval_case(d, case)
        out.append((f'golden{case}', gt, dt, l2c, want))
    for i, (gt, dt, l2c) in enumerate(_ref_indoor_eval_vectors()):
        out.append((f'vector{i}', gt, dt, l2c, None))
    return out


def _same(a, b):
    """same keys in the same order, bit-equal values"""
    assert list(a) == list(b)
    for k in a:
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() or (np.isnan(a[k]) and np.isnan(b[k])), (k, a[k], b[k])


def test_host_producer_and_finisher_equal_indoor_eval_on_the_goldens():
    from fcaf3d_amd.evaluation import finish_table, indoor_eval, match_table_host
    from tests.test_oracle_golden import _oracle_iou3d
    for name, gt, dt, l2c, want in _cases():
        ref = indoor_eval(gt, dt, METRIC, l2c, iou_fn=_oracle_iou3d)
        table = match_table_host(gt, dt, METRIC, _oracle_iou3d)
        assert len(table) == sum(len(d['scores_3d']) for d in dt)
        got = finish_table(table, METRIC, l2c)
        _same(got, ref)
        if want is not None:
            assert sorted(got) == sorted(want)
            for k in want:
                assert abs(got[k] - want[k]) < 1e-4, (name, k, got[k], want[k])


def test_the_fixtures_have_no_equal_scores_no_ties_and_clear_thresholds():
    """what makes the bit-equality above meaningful.  Within a class no two scores are equal, so the reference's unstable argsort
    cannot reorder anything and the one designed difference (the order of equal scores) does not show; no best IoU (oracle) lies
    within 6.9e-3 of a threshold and no positive best IoU is tied with another box of the class, so rounding cannot move a match."""
    from fcaf3d_amd.evaluation import _gravity7
    from tests.test_oracle_golden import _oracle_iou3d
    for name, gt, dt, l2c, want in _cases():
        labels = np.concatenate([np.asarray(d['labels_3d']) for d in dt])
        scores = np.concatenate([np.asarray(d['scores_3d']) for d in dt])
        for c in np.unique(labels):
            s = scores[labels == c]
            assert len(np.unique(s)) == len(s), (name, c)
        near, gap = np.inf, np.inf
        for g, d in zip(gt, dt):
            if g['gt_num'] == 0 or len(d['scores_3d']) == 0:
                continue
            dl, gl = np.asarray(d['labels_3d']), np.asarray(g['class'])
            iou = np.asarray(_oracle_iou3d(_gravity7(d['boxes_3d']), _gravity7(g['gt_boxes_upright_depth'])), np.float64)
            m = np.where(dl[:, None] == gl[None, :], iou, -np.inf)
            top = np.sort(m, 1)[:, ::-1]
            best = top[:, 0]
            fin = np.isfinite(best)
            near = min([near] + [np.abs(best[fin] - t).min() for t in METRIC if fin.any()])
            if m.shape[1] > 1:
                pos = best > 0
                gap = min([gap] + list(best[pos] - top[pos, 1]))
        print(f'{name}: nearest best IoU to a threshold {near:.3e}, smallest lead of a positive best IoU {gap:.3e}')
        assert near >= 6.9e-3 and gap > 0, (name, near, gap)


def test_two_shards_merge_to_the_unsharded_result():
    from fcaf3d_amd.evaluation import finish_table, match_table_host, merge_tables
    from tests.test_oracle_golden import _oracle_iou3d
    for name, gt, dt, l2c, want in _cases()[:2]:
        whole = finish_table(match_table_host(gt, dt, METRIC, _oracle_iou3d), METRIC, l2c)
        ids = np.arange(len(gt))
        shards = [match_table_host([gt[i] for i in ids[r::2]], [dt[i] for i in ids[r::2]], METRIC, _oracle_iou3d, scene_ids=ids[r::2])
                  for r in (0, 1)]
        assert len(shards[0]) and len(shards[1])
        _same(finish_table(merge_tables(shards), METRIC, l2c), whole)
        _same(finish_table(merge_tables(shards[::-1]), METRIC, l2c), whole)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from fcaf3d_amd import dist as D
    from fcaf3d_amd.evaluation import default_scene_ids, finish_table, gather_tables, match_table_host
    from tests.test_oracle_golden import _oracle_iou3d
    D.init_dist(backend='gloo')
    res = []
    for name, gt, dt, l2c, want in _cases()[:2]:
        mine = list(range(rank, len(gt), world))
        ids = default_scene_ids(len(mine))
        assert list(ids) == mine
        table = match_table_host([gt[i] for i in mine], [dt[i] for i in mine], METRIC, _oracle_iou3d, scene_ids=ids)
        res.append(finish_table(gather_tables(table), METRIC, l2c))
    out.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_return_the_unsharded_result():
    from fcaf3d_amd.evaluation import finish_table, match_table_host
    from tests.test_oracle_golden import _oracle_iou3d
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for k, (name, gt, dt, l2c, want) in enumerate(_cases()[:2]):
        whole = finish_table(match_table_host(gt, dt, METRIC, _oracle_iou3d), METRIC, l2c)
        _same(got[0][k], whole)
        _same(got[1][k], whole)


def test_equal_scores_go_to_the_smallest_scene_id_and_position():
    """two scenes with one box each; scene 0 holds a miss and two hits, scene 1 three hits, all six of score 0.5.  Per box the
    true positive is the claimant at the lowest position; the class's rows are ordered (scene id, position) whatever order the
    shards are merged in: FP TP FP | TP FP FP -> recall .0 .5 .5 1 1 1, precision 0 1/2 1/3 1/2 2/5 1/3 -> AP 0.5 (with scene 1
    first it would be 0.7)"""
    from fcaf3d_amd.evaluation import finish_table, match_table_host, merge_tables
    from tests.test_oracle_golden import _oracle_iou3d
    box = np.array([[0., 0., 0., 1., 1., 1., 0.]], np.float32)
    far = np.array([[9., 9., 0., 1., 1., 1., 0.]], np.float32)
    gt = [{'gt_num': 1, 'gt_boxes_upright_depth': box.copy(), 'class': np.array([0])} for _ in range(2)]
    det = lambda b: dict(boxes_3d=b, scores_3d=torch.full((3,), 0.5), labels_3d=torch.zeros(3, dtype=torch.long))
    dt = [det(np.concatenate([far, box, box])), det(np.concatenate([box, box, box]))]
    l2c = {0: 'thing'}
    whole = match_table_host(gt, dt, METRIC, _oracle_iou3d)
    assert whole.tp_bits.tolist() == [0, 3, 0, 3, 0, 0]
    shards = [match_table_host(gt[i:i + 1], dt[i:i + 1], METRIC, _oracle_iou3d, scene_ids=[i]) for i in (0, 1)]
    for tables in ([whole], shards, shards[::-1]):
        r = finish_table(merge_tables(tables), METRIC, l2c)
        assert r['thing_AP_0.25'] == r['thing_AP_0.50'] == 0.5 and r['thing_rec_0.25'] == 1.0, r
    # the same scenes under swapped ids: scene "1" (three hits) now comes second no more
    swapped = [match_table_host(gt[i:i + 1], dt[i:i + 1], METRIC, _oracle_iou3d, scene_ids=[1 - i]) for i in (0, 1)]
    r = finish_table(merge_tables(swapped), METRIC, l2c)
    assert r['thing_AP_0.25'] == float(np.float32(0.7)), r           # (average_precision returns fp32)


def test_size_query_and_argument_checks_need_no_gpu():
    from fcaf3d_amd import _lib as L
    assert L.query('fc_eval_match_ws_bytes', 1000, 100, 2) >= 100 * 2 * 8
    assert L.query('fc_eval_match_ws_bytes', 1000, 0, 2) == 0
    assert L.query('fc_eval_match_ws_bytes', 1000, 100, 8) >= 100 * 8 * 8
    fn = L.lib().fc_eval_match
    p = 0x1000                       # never dereferenced: every call below is refused before a launch

    def call(det_dim=7, n_thr=2, n_det=10, n_gt=10, ws_bytes=1 << 20, flags=0):
        return fn(p, det_dim, p, p, p, p, p, 1, n_det, n_gt, p, n_thr, flags, p, p, p, p, ws_bytes, None)
    assert call(det_dim=5) == -1 and call(det_dim=8) == -1
    assert call(n_thr=9) == -1 and call(n_thr=0) == -1
    assert call(n_det=-1) == -1 and call(n_gt=-1) == -1 and call(flags=2) == -1
    assert call(ws_bytes=8) == -2 and call(ws_bytes=10 * 2 * 8 - 1) == -2
    assert call(n_det=0, ws_bytes=0) == 0                              # nothing to do: nothing launched


# ---- the kernels' text on the host (tools/eval_host_emu.cpp) -----------------------------------------------------------------------

def _build_emulator(tmp):
    """csrc_post/eval.hip from its EVAL_* constants to the end of its anonymous namespace (constants, grid helpers, kernels), behind
    fc_common.h's own FC_EMPTY_KEY line, compiled for the host with AddressSanitizer and UBSan: the emulator restates none of them"""
    import shutil
    import subprocess
    from fcaf3d_amd import build as B
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(B.CSRC_POST, 'eval.hip')).read()
    end = '}  // namespace'
    body = src[src.index('#define EVAL_THREADS'):src.index(end) + len(end)]
    assert '#include' not in body and all(f'#define {n} ' in body for n in ('EVAL_GT_CHUNK', 'EVAL_MAX_GY')), 'eval.hip was reordered'
    empty_key = [ln for ln in open(os.path.join(B.CSRC, 'fc_common.h')).read().splitlines() if ln.startswith('#define FC_EMPTY_KEY ')]
    assert len(empty_key) == 1
    (tmp / 'kernels.inc').write_text(empty_key[0] + '\n' + body)
    (tmp / 'hip').mkdir()
    (tmp / 'hip' / 'hip_runtime.h').write_text('#pragma once\n#include <cmath>\n')
    cxx = os.path.join(os.path.dirname(os.path.dirname(B.HIPCC)), 'llvm', 'bin', 'clang++')
    cxx = cxx if os.path.exists(cxx) else shutil.which('clang++')
    exe = str(tmp / 'eval_host_emu')
    subprocess.check_call([cxx, '-std=c++20', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-pthread', f'-I{tmp}', f'-I{B.CSRC_POST}',
                           f"-I{os.path.join(root, 'include')}", os.path.join(root, 'tools', 'eval_host_emu.cpp'), '-o', exe])
    return exe


def _emulate(exe, tmp, gt, dt, metric):
    """the arrays match_table_device hands to fc_eval_match, through the emulator -> best_iou, best_gt, tp_bits"""
    import subprocess
    from fcaf3d_amd import evaluation as E
    ids = np.arange(len(gt))
    gb, gl, gc, _, _ = E._gt_arrays(gt, ids)
    boxes, scores, labels, dc, flags = E._det_tensors(dt, torch.device('cpu'))
    seg = np.stack([np.cumsum(dc) - dc, dc, np.cumsum(gc) - gc, gc], 1).astype(np.int64)
    n = len(scores)
    with open(tmp / 'in.bin', 'wb') as f:
        np.array([n, boxes.shape[1], len(gl), len(ids), len(metric), flags], np.int64).tofile(f)
        boxes.numpy().astype(np.float32).tofile(f); scores.numpy().tofile(f); labels.numpy().tofile(f)
        gb.tofile(f); gl.tofile(f); seg.tofile(f); np.asarray(metric, np.float64).tofile(f)
    r = subprocess.run([exe, str(tmp / 'in.bin'), str(tmp / 'out.bin')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    raw = open(tmp / 'out.bin', 'rb').read()
    return (np.frombuffer(raw[:4 * n], np.float32), np.frombuffer(raw[4 * n:8 * n], np.int32).astype(np.int64),
            np.frombuffer(raw[8 * n:], np.uint8), flags, boxes.shape[1])


def test_kernel_text_on_the_host_equals_the_host_producer(tmp_path):
    """the kernels of csrc_post/eval.hip, compiled for the host under AddressSanitizer and UBSan (a thread per GPU thread, a
    barrier for __syncthreads): on the four fixtures (bottom-centre box objects), with 8 thresholds, and on the GPU test's crafted
    set (scene sizes around the 256-detection tile and the 64-box LDS chunk, 7 and 6 columns) best_gt and tp_bits equal the host
    producer's and no access leaves its array.  The fixtures' and the crafted set's margins (see above, and tests/test_gpu_eval.py)
    are far larger than the host-libm against oracle difference of the IoU (1e-5 allowed here)."""
    from fcaf3d_amd.evaluation import match_table_host
    from tests.test_gpu_eval import DET_COUNTS, GT_COUNTS, _scene
    from tests.test_oracle_golden import _oracle_iou3d
    exe = _build_emulator(tmp_path)
    sets = [(name, gt, dt, METRIC) for name, gt, dt, _, _ in _cases()]
    sets.append(('golden1, 8 thresholds', sets[1][1], sets[1][2], (.1, .2, .3, .4, .5, .6, .7, .8)))
    for yaw in (True, False):
        rng = np.random.default_rng(3 if yaw else 4)
        scenes = [_scene(rng, nd, ng, yaw) for nd, ng in zip(DET_COUNTS, GT_COUNTS)]
        n = sum(DET_COUNTS)
        scores, o = (rng.permutation(n) + 1).astype(np.float32) / np.float32(n), 0
        gt, dt = [], []
        for gb, gl, db, dl in scenes:
            gt.append({'gt_num': len(gb), 'gt_boxes_upright_depth': gb, 'class': gl})
            dt.append(dict(boxes_3d=torch.from_numpy(np.ascontiguousarray(db if yaw else db[:, :6])),
                           scores_3d=torch.from_numpy(scores[o:o + len(dl)]), labels_3d=torch.from_numpy(dl)))
            o += len(dl)
        sets.append((f'crafted, yaw={yaw}', gt, dt, METRIC))
    for name, gt, dt, metric in sets:
        host, h_iou, h_gt = match_table_host(gt, dt, metric, _oracle_iou3d, return_match=True)
        e_iou, e_gt, e_bits, flags, dim = _emulate(exe, tmp_path, gt, dt, metric)
        assert flags == (0 if name.startswith('crafted') else 1) and dim == (6 if name.endswith('False') else 7), name
        fin = np.isfinite(h_iou)
        assert np.array_equal(np.isfinite(e_iou), fin) and (e_iou[~fin] == -np.inf).all(), name
        assert np.abs(e_iou[fin] - h_iou[fin]).max() < 1e-5, name
        assert np.array_equal(e_gt, h_gt) and np.array_equal(e_bits, host.tp_bits) and e_bits.any(), name
