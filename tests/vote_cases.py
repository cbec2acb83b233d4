"""The segment sets tests/test_gpu_vote.py runs the voting kernel on (csrc_post/vote.hip) and tests/test_vote_cpu.py runs its host
emulation on: tables in the layout of the merge NMS (boxes (nseg, stride, 7), scores, counts, keep, keep counts) with stride > count,
every padding row NaN and every padding keep entry out of range, and the per-segment statement of the rule they are checked against."""
import numpy as np
import torch

TILE = 128                # csrc_post/vote.hip VOTE_TILE
WAVES = 4                 # VOTE_WAVES: kept boxes a workgroup votes for at once
KEPT_PER_BLOCK = 32       # VOTE_KEPT_PER_BLOCK: sizes the grid
BAD_KEEP = 0x7fffffff     # padding of the keep table: never a position
PI = float(np.float32(np.pi))
# the seeds of the random sets: drawn so that no pair's IoU lies within 1e-5 of the threshold (assert_clear_of_threshold)
GENERAL_SEEDS = (11, 12, 13)
CRAFTED_SEED = 7
THR = 0.55


def constants_of_the_kernel():
    """(VOTE_TILE, VOTE_WAVES, VOTE_KEPT_PER_BLOCK) as csrc_post/vote.hip defines them"""
    import os
    import re
    from fcaf3d_amd import build as B
    txt = open(os.path.join(B.CSRC_POST, 'vote.hip')).read()
    d = {k: int(v) for k, v in re.findall(r'^#define (VOTE_\w+) (\d+)\b', txt, flags=re.M)}
    return d['VOTE_TILE'], d['VOTE_THREADS'] // d['VOTE_WAVE'], d['VOTE_KEPT_PER_BLOCK']


def random_boxes(rng, n, with_yaw):
    """n boxes in clusters of near-duplicates (the candidates of one object seen under several flips), rows in descending score
    order; with yaws, about a third of the boxes are the same rectangle written with its sides exchanged (yaw + pi/2) and a fifth
    written half a turn on (yaw + pi)"""
    ncl = max(1, n // 4)
    gx = int(np.ceil(np.sqrt(ncl)))
    cl = rng.integers(0, ncl, size=n)
    cx, cy = (cl % gx) * 2.5, (cl // gx) * 2.5
    base = rng.uniform(0.7, 1.3, size=(ncl, 3)) * np.array([1.2, 0.8, 0.6])
    cyaw = rng.uniform(-3.0, 3.0, size=ncl)
    b = np.zeros((n, 7))
    b[:, 0], b[:, 1] = cx + rng.normal(0, 0.05, n), cy + rng.normal(0, 0.05, n)
    b[:, 2] = rng.normal(0, 0.3, n)
    b[:, 3:6] = base[cl] * rng.uniform(0.92, 1.08, size=(n, 3))
    if with_yaw:
        b[:, 6] = cyaw[cl] + rng.normal(0, 0.04, n)
        u = rng.random(n)
        quarter, half = u < 0.33, (u >= 0.33) & (u < 0.53)
        b[quarter, 3], b[quarter, 4] = b[quarter, 4].copy(), b[quarter, 3].copy()
        b[quarter, 6] += np.pi / 2
        b[half, 6] += np.pi
    s = np.sort(rng.uniform(0.05, 1.0, n))[::-1]
    return b.astype(np.float32), np.ascontiguousarray(s).astype(np.float32)


def pack(segments, stride=None, keep_stride=None):
    """[(boxes (n, 7), scores (n,), keep positions)] -> dict of the kernel's tables (numpy), padding poisoned"""
    nseg = len(segments)
    stride = stride or max([len(s[1]) for s in segments] + [0]) + 3
    keep_stride = keep_stride or stride
    T = dict(boxes=np.full((nseg, stride, 7), np.nan, np.float32), scores=np.full((nseg, stride), np.nan, np.float32),
             counts=np.zeros(nseg, np.int32), keep=np.full((nseg, keep_stride), BAD_KEEP, np.int32), kcounts=np.zeros(nseg, np.int32))
    for k, (b, s, kp) in enumerate(segments):
        n = len(s)
        T['boxes'][k, :n], T['scores'][k, :n], T['counts'][k] = b, s, n
        T['keep'][k, :len(kp)], T['kcounts'][k] = kp, len(kp)
    return T


def crafted(with_yaw):
    """segment lengths 0, 1, T-1, T, T+1, 2T+1; kept counts 0, 1, every row, one more than a workgroup votes for at once, one more
    than the grid votes for in one round; empty segments between full ones"""
    rng = np.random.default_rng(CRAFTED_SEED + (100 if with_yaw else 0))
    T, W, K = TILE, WAVES, KEPT_PER_BLOCK
    stride = 2 * T + 1 + 3
    per_pass = -(-stride // K) * W                  # kept boxes the whole grid votes for in one round
    plan = [(T + 1, 'all'), (0, 0), (1, 1), (0, 0), (T - 1, 'all'), (T, W + 1), (2 * T + 1, 'all'), (1, 0), (T + 1, 0),
            (2 * T + 1, per_pass + 1), (T, 1), (0, 0)]
    segs = []
    for n, kc in plan:
        b, s = random_boxes(rng, n, with_yaw)
        kc = n if kc == 'all' else kc
        segs.append((b, s, np.sort(rng.choice(n, size=kc, replace=False)) if kc else np.zeros(0, np.int64)))
    return pack(segs, stride=stride)


def general(seed, with_yaw):
    """a set of 6 segments of about 60 random boxes, about half of them kept"""
    rng = np.random.default_rng(seed + (100 if with_yaw else 0))
    segs = []
    for _ in range(6):
        n = int(rng.integers(50, 71))
        b, s = random_boxes(rng, n, with_yaw)
        segs.append((b, s, np.sort(rng.choice(n, size=n // 2, replace=False))))
    return pack(segs)


def exact():
    """axis-aligned boxes on a grid of binary fractions, every footprint written 1 to 4 times with other heights, power-of-two
    scores: at vote_thr = 1.0 exactly the duplicates of a footprint vote (their IoU is 1.0: equality must vote) and every sum
    is exact, so the output is determined to the bit"""
    rng = np.random.default_rng(5)
    segs = []
    for n_foot in (1, 9, 40):
        rows = []
        for f in range(n_foot):
            x, y = (f % 7) * 0.75, (f // 7) * 0.75                       # footprints overlap their neighbours, IoU < 1
            dx, dy = rng.integers(4, 9) / 8.0, rng.integers(4, 9) / 8.0
            for _ in range(int(rng.integers(1, 5))):
                rows.append([x, y, rng.integers(-8, 9) / 16.0, dx, dy, rng.integers(2, 17) / 8.0, 0.0])
        b = np.array(rows, np.float32)[rng.permutation(len(rows))]
        s = np.sort(2.0 ** -rng.integers(0, 6, size=len(b)).astype(np.float64))[::-1].astype(np.float32)
        segs.append((b, np.ascontiguousarray(s), np.sort(rng.choice(len(b), size=(len(b) + 1) // 2, replace=False))))
    return pack(segs)


def assert_clear_of_threshold(T, thr, rotated, margin=1e-5):
    """no pair (kept box, candidate) of the set has an IoU within `margin` of the threshold, by the C oracle's BEV IoU (host code,
    independent of the kernels): what the kernel, nms.boxes_iou_bev and the oracle compute may differ in the last bits without
    moving a member.  Returns the oracle's IoUs per segment."""
    from oracle import bev
    ious, near = [], np.inf
    for k in range(len(T['counts'])):
        n, kc = int(T['counts'][k]), int(T['kcounts'][k])
        b, kp = T['boxes'][k, :n], T['keep'][k, :kc]
        iou = bev.iou_matrix(b[kp], b, rotated=rotated) if kc else np.zeros((0, n), np.float32)
        off = np.abs(iou.astype(np.float64) - thr)
        off[np.arange(kc), kp] = np.inf                                  # a box is its own member by definition
        if off.size:
            near = min(near, off.min())
        ious.append(iou)
    assert near > margin, f'an IoU lies {near:.3e} from vote_thr={thr}: draw another seed'
    return ious


def expected(T, thr, rotated, with_yaw, ious=None, device='cpu'):
    """merge_augs.vote_boxes per segment -> [(out (n, 7), members (kc,), member mask (kc, n))]; ious: per segment (kc, n) fp32, or
    None to take them from nms.boxes_iou_bev on `device`"""
    from fcaf3d_amd.merge_augs import vote_boxes
    from fcaf3d_amd.nms import boxes_iou_bev
    res = []
    for k in range(len(T['counts'])):
        n, kc = int(T['counts'][k]), int(T['kcounts'][k])
        b = torch.from_numpy(T['boxes'][k, :n]).to(device)
        s = torch.from_numpy(T['scores'][k, :n]).to(device)
        kp = torch.from_numpy(T['keep'][k, :kc].astype(np.int64)).to(device)
        if ious is not None:
            iou = torch.from_numpy(ious[k]).to(device)
        else:
            iou = boxes_iou_bev(b[kp], b, rotated=rotated) if kc and n else torch.zeros((kc, n), device=device)
        out, cnt = vote_boxes(b, s, kp, thr, rotated, with_yaw, iou=iou, return_members=True)
        mem = iou >= torch.tensor(thr, dtype=torch.float32, device=device)
        mem[torch.arange(kc, device=device), kp] = True
        res.append((out.cpu(), cnt.cpu(), mem.cpu()))
    return res


def check(T, got_boxes, got_members, init, want, exact_bits=False):
    """the kernel's output against `expected`: kept rows within 2^-23 * max_{j in M} |box_j[k]| per column (bit-equal with
    exact_bits), member counts equal, yaw column and every row that is not kept bit-equal to the input, rows at or past the count
    and member entries past the kept count as they were before the launch (`init`, -1), no NaN below the count"""
    worst = 0.0
    for k, (out, cnt, mem) in enumerate(want):
        n, kc = int(T['counts'][k]), int(T['kcounts'][k])
        g = torch.from_numpy(np.array(got_boxes[k]))
        assert torch.equal(g[n:].view(torch.int32), torch.from_numpy(np.ascontiguousarray(init[k, n:])).view(torch.int32)), f'segment {k}: a padding row was written'
        assert not torch.isnan(g[:n]).any(), f'segment {k}: NaN in the output: the padding was read'
        b = torch.from_numpy(T['boxes'][k, :n])
        kp = torch.from_numpy(T['keep'][k, :kc].astype(np.int64))
        rest = torch.ones(n, dtype=torch.bool)
        rest[kp] = False
        assert torch.equal(g[:n][rest], b[rest]), f'segment {k}: a row that is not kept changed'
        assert torch.equal(g[:n, 6], b[:, 6]), f'segment {k}: the yaw column changed'
        assert np.array_equal(got_members[k, :kc], cnt.numpy()), (k, got_members[k, :kc], cnt)
        assert (got_members[k, kc:] == -1).all(), f'segment {k}: a member entry past the kept count was written'
        if kc == 0:
            continue
        if exact_bits:
            assert torch.equal(g[:n][kp], out[kp]), (k, (g[:n][kp] - out[kp]).abs().max())
            continue
        scale = torch.where(mem[:, :, None], b[None, :, :6].abs().double(), torch.zeros((), dtype=torch.float64)).amax(1)    # (kc, 6)
        err = (g[:n][kp][:, :6].double() - out[kp][:, :6].double()).abs()
        bound = scale * 2.0 ** -23
        assert (err <= bound).all(), (k, float((err - bound).max()))
        worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
    return worst
