"""Case builders and float64 references of the exact head tests (tests/test_head_cases_cpu.py, tests/test_gpu_assign_exact.py,
tests/test_gpu_head_split_exact.py, tests/test_gpu_head_loss_exact.py).  Pure numpy, no GPU import.

Three parts.

ASSIGNER (csrc/assign.hip).  A case is a batch: per scene its boxes [cx,cy,cz,w,l,h,yaw] (gravity centre) and labels, per (level, scene)
its locations.  `assign_reference` follows Fcaf3DAssigner.assign in float64; `assigner_violations` lists where a case breaks the
conditions under which the fp32 kernel and the float64 reference cannot decide differently:
  * tie cases: yaw 0, every coordinate and size a multiple of 1/16 below 2^10 (face distances exact in both precisions);
  * no location within 1e-3 of a face of a box of its scene;
  * per box, v its kth value: no candidate with 0 < |c - v| <= 1e-4 v; candidates with c == v are mirror images (equal |offset| per axis);
  * no two boxes claiming one location have volumes closer than 1e-4 relative unless sizes are bit-equal.
`assigner_branches` states, per case, which branches of k_best / k_kth / k_final the case takes (asserted by the builder).

HEAD SPLIT (csrc/head.hip).  Small integers stored as fp32: every sum and product is an integer (or a half) below 2^24, so everything but
exp() is compared bit for bit.

LOSS (csrc/loss.hip).  `loss_reference` evaluates the fused loss and its three gradients in float64 in the kernels' own operation order
through `E`, a value with a rigorous bound on what the fp32 evaluation of the same operation sequence may differ by (running error
analysis: every operation passes its operands' bounds on — products and quotients with their second-order parts — and adds one rounding,
u = 2^-24 of the computed magnitude; expf / logf / log1pf add one ulp = 2 u).  Saturated rows take the oracle's fp32 restatement
(`focal_fp32`) as their reference instead: at |x| >= 30, 1 - p is exactly 0 or 1 in fp32 and mmcv's clamp at FLT_MIN defines the value.
"""
import numpy as np

U32 = 2.0 ** -24                     # unit roundoff of fp32
EPS32 = 2.0 ** -23
FLT_MIN = float(np.finfo(np.float32).tiny)
LIMIT, TOPK, KTH_CAP = 27, 18, 8192
FACE_MARGIN, KTH_GAP, VOL_GAP = 1e-3, 1e-4, 1e-4
FLOAT_MAX_VOL = 1e8


# =====================================================================================================================================
# assigner
# =====================================================================================================================================
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def grid(centre, counts, step):
    """counts[a] points of step `step` per axis, centred on `centre` (an even count puts the offsets at odd multiples of step / 2)"""
    axes = [c + step * (np.arange(n) - (n - 1) / 2) for c, n in zip(centre, counts)]
    return _f32(np.stack(np.meshgrid(*axes, indexing='ij'), -1).reshape(-1, 3))


def line(n, start, step, axis=0):
    p = np.tile(np.asarray(start, dtype=np.float64), (n, 1))
    p[:, axis] += step * np.arange(n)
    return _f32(p)


def far(n, k=0):
    """n locations inside no box of any case"""
    return line(n, (40.0 + k, 40.0, 40.0), 1 / 4, axis=1)


EMPTY = np.zeros((0, 3), dtype=np.float32)
BOX_A = (3, 5, 1, 5, 6, 2, 0)               # the issue's design: three different sizes
BOX_S = (3, 5, 1, 3, 2, 1, 0)


class AssignCase:
    def __init__(self, name, L, boxes, labels, segs, tie, expect):
        """boxes / labels: per scene; segs: {(level, scene): (n, 3) locations}; expect: facts the builder asserts (assigner_branches)"""
        self.name, self.L, self.B, self.tie, self.expect = name, L, len(boxes), tie, expect
        self.boxes = [_f32(np.asarray(b, dtype=np.float64).reshape(-1, 7)) for b in boxes]
        self.labels = [np.asarray(l, dtype=np.int64).reshape(-1) for l in labels]
        self.M = max(len(b) for b in self.boxes) + 1                    # every scene keeps at least one padded slot
        self.segs = {(l, s): _f32(segs.get((l, s), EMPTY)).reshape(-1, 3) for l in range(L) for s in range(self.B)}

    def __repr__(self):
        return self.name

    # canonical rows: grouped by (level, scene), as the head's location arrays are
    def rows(self):
        pts, scene, level = [], [], []
        for l in range(self.L):
            for s in range(self.B):
                p = self.segs[(l, s)]
                pts.append(p); scene += [s] * len(p); level += [l] * len(p)
        return np.concatenate(pts), np.array(scene, dtype=np.int32), np.array(level, dtype=np.int32)

    def padded(self):
        """(boxes (B, M, 7), labels (B, M), box_count (B)): slots past a scene's count hold NaN / -99 and must never reach an output"""
        boxes = np.full((self.B, self.M, 7), np.nan, dtype=np.float32)
        labels = np.full((self.B, self.M), -99, dtype=np.int64)
        for s in range(self.B):
            boxes[s, :len(self.boxes[s])] = self.boxes[s]
            labels[s, :len(self.boxes[s])] = self.labels[s]
        return boxes, labels, np.array([len(b) for b in self.boxes], dtype=np.int32)


def layout(case, interleave, seed=7):
    """the launch's row arrays.  interleave False: canonical rows, identity `order`.  True: inside each level the rows of all scenes are
    permuted (seeded) and `order` lists every segment's rows.  canon[i] = canonical row of launch row i."""
    pts, scene, level = case.rows()
    N = len(pts)
    seg_start = [0]
    for l in range(case.L):
        for s in range(case.B):
            seg_start.append(seg_start[-1] + len(case.segs[(l, s)]))
    canon = np.arange(N)
    if interleave:
        rng = np.random.default_rng(seed)
        for l in range(case.L):
            r0, r1 = seg_start[l * case.B], seg_start[(l + 1) * case.B]
            canon[r0:r1] = r0 + rng.permutation(r1 - r0)
        order = np.empty(N, dtype=np.int32)
        where = np.empty(N, dtype=np.int64)
        where[canon] = np.arange(N)                                       # launch row of every canonical row
        for q in range(case.L * case.B):
            order[seg_start[q]:seg_start[q + 1]] = rng.permutation(where[seg_start[q]:seg_start[q + 1]])
    else:
        order = np.arange(N, dtype=np.int32)
    return dict(pts=pts[canon], scene=scene[canon], level=level[canon], order=order, seg_start=np.array(seg_start, dtype=np.int32), canon=canon)


def face_distances(pts, b):
    """(n, 6) distances to the faces and (n, 3) offsets in the box frame, float64 (Fcaf3DAssigner.assign; rotation by -yaw about z)"""
    pts, b = pts.astype(np.float64), b.astype(np.float64)
    sh = pts - b[:3]
    c, s = np.cos(-b[6]), np.sin(-b[6])
    off = np.stack([sh[:, 0] * c + sh[:, 1] * s, -sh[:, 0] * s + sh[:, 1] * c, sh[:, 2]], 1)
    ctr, half = b[:3] + off, b[3:6] / 2
    lo, hi = ctr - b[:3] + half, b[:3] + half - ctr
    return np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1], lo[:, 2], hi[:, 2]], 1), off


def centerness(d):
    d = d.reshape(-1, 3, 2)
    lo, hi = d.min(2), d.max(2)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.sqrt(lo[:, 0] / hi[:, 0] * lo[:, 1] / hi[:, 1] * lo[:, 2] / hi[:, 2])


def assign_reference(case, limit=LIMIT, topk=TOPK):
    """float64 restatement of Fcaf3DAssigner.assign per scene, on canonical rows.  labels / owner / ct / bt per row (ct 0 and owner 0 on
    background, bt 0 in a scene without boxes); counts (B, M, L), best (B, M), kth (B, M) (-1: the rank-th value is the padding;
    NaN in padded slots), ncand / rank / mult (candidates equal to kth) / above (candidates over kth) per box."""
    pts, scene, level = case.rows()
    N, B, M, L = len(pts), case.B, case.M, case.L
    out = dict(labels=np.full(N, -1, dtype=np.int64), owner=np.zeros(N, dtype=np.int64), ct=np.zeros(N), bt=np.zeros((N, 7), dtype=np.float32),
               counts=np.zeros((B, M, L), dtype=np.int64), best=np.zeros((B, M), dtype=np.int64), kth=np.full((B, M), np.nan),
               ncand=np.zeros((B, M), dtype=np.int64), rank=np.zeros((B, M), dtype=np.int64), mult=np.zeros((B, M), dtype=np.int64),
               above=np.zeros((B, M), dtype=np.int64), claims=[[] for _ in range(N)], min_face=np.inf)
    for s in range(B):
        rows = np.nonzero(scene == s)[0]
        n, boxes = len(rows), case.boxes[s]
        if len(boxes) == 0 or n == 0:
            continue
        best_vol = np.full(n, FLOAT_MAX_VOL)
        owner, cn_own = np.zeros(n, dtype=np.int64), np.zeros(n)
        for j, b in enumerate(boxes):
            d, _ = face_distances(pts[rows], b)
            out['min_face'] = min(out['min_face'], float(np.abs(d).min()))
            inside = d.min(1) > 0
            counts = np.array([int((inside & (level[rows] == l)).sum()) for l in range(L)])
            starved = counts < limit
            best = L - 1 if not starved.any() else max(int(np.argmax(starved)) - 1, 0)
            cand = inside & (level[rows] == best)
            cn = np.where(cand, centerness(d), -1.0)
            rank = min(topk + 1, n)
            kth = np.sort(cn)[::-1][rank - 1]
            good = cand & (cn > kth)
            vol = float(b[3]) * float(b[4]) * float(b[5])
            take = good & (vol < best_vol)                                # strict: the first of equal volumes keeps the location
            best_vol[take], owner[take], cn_own[take] = vol, j, cn[take]
            for r in rows[good]:
                out['claims'][r].append(j)
            out['counts'][s, j], out['best'][s, j], out['kth'][s, j] = counts, best, kth
            out['ncand'][s, j], out['rank'][s, j] = int(cand.sum()), rank
            out['mult'][s, j], out['above'][s, j] = int((cand & (cn == kth)).sum()), int(good.sum())
        pos = best_vol != FLOAT_MAX_VOL
        out['owner'][rows] = owner
        out['labels'][rows] = np.where(pos, case.labels[s][owner], -1)
        out['ct'][rows] = np.where(pos, cn_own, 0.0)
        out['bt'][rows] = boxes[owner]
    return out


def assigner_violations(case, ref=None, limit=LIMIT, topk=TOPK):
    """the stated conditions, as a list of what breaks them (empty: the case is decidable alike in fp32 and float64)"""
    ref = ref or assign_reference(case, limit, topk)
    pts, scene, level = case.rows()
    bad = []
    if case.tie:
        for what, a in [('location', pts)] + [(f'box of scene {s}', b[:, :6]) for s, b in enumerate(case.boxes)]:
            a = a.astype(np.float64)
            if a.size and (np.any(a * 16 != np.round(a * 16)) or np.abs(a).max() >= 1024):
                bad.append(f'{case}: a {what} is no multiple of 1/16 below 2^10')
        if any(np.any(b[:, 6] != 0) for b in case.boxes):
            bad.append(f'{case}: a tie case holds a rotated box')
    for s in range(case.B):
        rows = np.nonzero(scene == s)[0]
        if not len(rows):
            continue
        for j, b in enumerate(case.boxes[s]):
            d, off = face_distances(pts[rows], b)
            if np.abs(d).min() <= FACE_MARGIN:
                bad.append(f'{case}: scene {s} box {j}: a location lies {np.abs(d).min():.2e} from a face')
            v = ref['kth'][s, j]
            if not v > 0:
                continue
            cand = (d.min(1) > 0) & (level[rows] == ref['best'][s, j])
            cn = centerness(d)[cand]
            gap = np.abs(cn - v)
            if np.any((gap > 0) & (gap <= KTH_GAP * v)):
                bad.append(f'{case}: scene {s} box {j}: a candidate lies {gap[gap > 0].min() / v:.2e} (relative) from the kth value')
            tied = np.abs(off[cand][cn == v])
            if len(tied) and np.any(tied != tied[0]):
                bad.append(f'{case}: scene {s} box {j}: {len(tied)} candidates equal the kth value without being mirror images')
    for r, js in enumerate(ref['claims']):
        bx = case.boxes[scene[r]]
        for a in range(len(js)):
            for c in range(a + 1, len(js)):
                sa, sc = bx[js[a], 3:6], bx[js[c], 3:6]
                va, vc = np.prod(sa.astype(np.float64)), np.prod(sc.astype(np.float64))
                same = sa[0] * sa[1] * sa[2] == sc[0] * sc[1] * sc[2] and va == vc               # fp32 product, then float64
                if not same and abs(va - vc) <= VOL_GAP * max(va, vc):
                    bad.append(f'{case}: row {r}: boxes {js[a]} and {js[c]} claim it with volumes {va} and {vc}')
    return bad


def assigner_branches(case, ref=None, limit=LIMIT, topk=TOPK):
    """the set of kernel branches the case takes, by name (see BRANCHES)"""
    ref = ref or assign_reference(case, limit, topk)
    pts, scene, level = case.rows()
    got = set()
    for s in range(case.B):
        n_scene = int((scene == s).sum())
        if len(case.boxes[s]) == 0:
            got.add('scene without boxes' + (' inside a batch' if 0 < s < case.B - 1 else ''))
        for j in range(len(case.boxes[s])):
            cnt, best, kth = ref['counts'][s, j], int(ref['best'][s, j]), ref['kth'][s, j]
            nc, mult, above, rank = (int(ref[k][s, j]) for k in ('ncand', 'mult', 'above', 'rank'))
            if n_scene == 0:
                continue
            got.add('ncand == KTH_CAP' if nc == KTH_CAP else 'ncand == KTH_CAP + 1' if nc == KTH_CAP + 1 else 'rescan' if nc > KTH_CAP else 'lds list')
            if kth > 0 and mult > 1 and above < rank - 1 < above + mult:
                got.add('ties straddle the rank')
            if kth > 0 and mult > 1:
                got.add('tie at kth')
            if rank < topk + 1:
                got.add('rank below topk + 1')
            if kth == -1:
                got.add('candidates exhausted')
            if limit - 1 in cnt:
                got.add('count == limit - 1')
            if limit in cnt:
                got.add('count == limit')
            if cnt[0] < limit:
                got.add('level 0 starved')
            first = int(np.argmax(cnt < limit)) if (cnt < limit).any() else case.L
            if (cnt[first + 1:] >= limit).any():
                got.add('rich level after a starved one')
            if not (cnt < limit).any():
                got.add('no level starved')
            r0 = len(case.segs[(best, s)])
            if r0 % 1024 and (r0 % 1024) % 256:
                got.add('partial tail of the four-row loop')
            if r0 % 1024 and r0 % 1024 <= 768:
                got.add('four-row loop with whole slots past the segment')
            if r0 == 0:
                got.add('best-level segment without rows')
    for r, js in enumerate(ref['claims']):
        bx = case.boxes[scene[r]]
        vols = [float(np.prod(bx[j, 3:6].astype(np.float64))) for j in js]
        if len(js) > 1 and len(set(vols)) < len(vols) and min(vols) == vols[0]:
            got.add('equal-volume pair, first wins')
        if len(js) > 1 and int(np.argmin(vols)) > 0:
            got.add('later smaller box wins')
    if any(len(case.segs[q]) == 0 for q in case.segs):
        got.add('segment without rows')
    if any(len(b) < case.M for b in case.boxes):
        got.add('padded box slots')
    if len({int(b) for s in range(case.B) for b in ref['best'][s, :len(case.boxes[s])]}) > 1:
        got.add('best levels differ')
    return got


BRANCHES = ('lds list', 'ncand == KTH_CAP', 'ncand == KTH_CAP + 1', 'rescan', 'tie at kth', 'ties straddle the rank', 'rank below topk + 1',
            'candidates exhausted', 'count == limit - 1', 'count == limit', 'level 0 starved', 'rich level after a starved one', 'no level starved',
            'partial tail of the four-row loop', 'four-row loop with whole slots past the segment', 'best-level segment without rows',
            'equal-volume pair, first wins', 'later smaller box wins', 'scene without boxes inside a batch', 'segment without rows', 'padded box slots',
            'best levels differ')


def _level_scene(counts, y0):
    """one BOX_A and, per level, counts[l] locations on a line inside it (one side of the centre: all centerness values differ) plus 25 outside"""
    return {l: np.concatenate([line(c, (3 + 1 / 16, y0 + l / 8, 1 + 1 / 16), 1 / 32), far(25, l)]) for l, c in enumerate(counts)}


def _tail_segment(n):
    """n rows of which the first 10 and the last 20 lie inside BOX_A (on one line, most central last): a dropped tail row changes the answer"""
    inside = line(30, (3 + 1 / 16, 5 + 1 / 16, 1 + 1 / 16), 1 / 16)[::-1]
    return np.concatenate([inside[:10], far(n - 30), inside[10:]])


def _general_scene(seed):
    rng = np.random.default_rng(seed)
    pts = [np.round(rng.uniform(-1.5, 1.5, (n, 3)) * 4096) / 4096 for n in (700, 300)]
    boxes = [(0.125, -0.0625, 0.03125, 2.0, 1.625, 1.25, 0.4), (-0.25, 0.1875, -0.0625, 1.75, 2.25, 1.5, -1.1), (0.5, 0.5, 0.25, 1.0, 0.75, 0.875, 2.0)]
    for b in boxes:                                              # general position: no location within twice the margin of a face
        pts = [p[np.abs(face_distances(_f32(p), _f32(b))[0]).min(1) > 2 * FACE_MARGIN] for p in pts]
    return boxes, pts


def assigner_cases():
    c = []
    A, S = BOX_A, BOX_S
    s0, s1, s2 = _level_scene((26, 40), 5), _level_scene((27, 26), 5), _level_scene((0, 0), 5)
    c.append(AssignCase('levels_L2', 2, [[A], [A], [A]], [[1], [2], [3]],
                        {(l, s): sc[l] for s, sc in enumerate((s0, s1, s2)) for l in range(2)}, False,
                        dict(best=[[0], [0], [0]], branches={'count == limit - 1', 'count == limit', 'level 0 starved', 'rich level after a starved one',
                                                            'candidates exhausted'})))
    s0, s1 = _level_scene((27, 27, 27), 5), _level_scene((30, 5, 60), 5)
    c.append(AssignCase('levels_L3', 3, [[A], [A]], [[4], [5]], {(l, s): sc[l] for s, sc in enumerate((s0, s1)) for l in range(3)}, False,
                        dict(best=[[2], [0]], branches={'no level starved', 'count == limit', 'rich level after a starved one'})))
    g8, g9 = grid(A[:3], (32, 32, 8), 1 / 8), grid(A[:3], (32, 32, 9), 1 / 8)
    off_centre = _f32([[3 + 2 + 5 / 16, 5 + 2 + 13 / 16, 1 + 13 / 16]])
    c.append(AssignCase('cap_8192', 2, [[A]], [[6]], {(0, 0): g8, (1, 0): far(3)}, True,
                        dict(ncand=8192, mult=8, above=16, branches={'ncand == KTH_CAP', 'tie at kth', 'ties straddle the rank'})))
    c.append(AssignCase('cap_8193', 2, [[A]], [[6]], {(0, 0): np.concatenate([g8, off_centre]), (1, 0): far(3)}, True,
                        dict(ncand=8193, mult=8, above=16, branches={'ncand == KTH_CAP + 1', 'tie at kth'})))
    c.append(AssignCase('cap_9216', 2, [[A]], [[6]], {(0, 0): g9, (1, 0): far(3)}, True,
                        dict(ncand=9216, mult=4, above=16, branches={'rescan', 'tie at kth', 'ties straddle the rank'})))
    g48 = grid(S[:3], (6, 4, 2), 1 / 2)
    c.append(AssignCase('ties_rank19', 2, [[S]], [[7]], {(0, 0): g48, (1, 0): far(2)}, True,
                        dict(ncand=48, mult=8, above=16, branches={'ties straddle the rank', 'lds list'})))
    ten = line(10, (3 + 1 / 16, 5 + 1 / 16, 1 + 1 / 16), 1 / 8)
    five = line(5, (3 + 1 / 16, 5 + 1 / 16, 1 + 1 / 16), 1 / 4)
    three = np.concatenate([five[:3], far(2)])
    # scene 3: every location on level 1, so the best level (0, by the clamp) is a segment without rows
    c.append(AssignCase('small_scenes', 2, [[A], [A], [A], [A]], [[8], [9], [10], [11]],
                        {(0, 0): np.concatenate([ten, far(20)]), (1, 0): far(4), (0, 1): five, (0, 2): three, (1, 3): np.concatenate([ten, far(12)])}, True,
                        dict(above=[[10], [4], [3], [0]], branches={'candidates exhausted', 'rank below topk + 1', 'segment without rows', 'level 0 starved',
                                                                    'best-level segment without rows'})))
    sizes = (255, 256, 257, 1023, 1024, 1025, 1027)
    c.append(AssignCase('tails', 1, [[A]] * len(sizes), [[11 + i] for i in range(len(sizes))], {(0, s): _tail_segment(n) for s, n in enumerate(sizes)},
                        True, dict(above=[[18]] * len(sizes), branches={'partial tail of the four-row loop', 'four-row loop with whole slots past the segment'})))
    elsewhere = (20, 20, 1, 2, 3, 1, 0)
    big_inside = np.concatenate([g48, line(12, (0.5 + 1 / 16, 5 + 1 / 16, 1 + 1 / 16), 1 / 16)])
    c.append(AssignCase('owners', 2, [[elsewhere, S, S], [], [A, S]], [[1, 3, 7], [], [2, 5]],
                        {(0, 0): g48, (1, 0): far(3), (0, 1): far(30), (1, 1): far(5), (0, 2): big_inside, (1, 2): far(3)}, True,
                        dict(branches={'equal-volume pair, first wins', 'later smaller box wins', 'scene without boxes inside a batch', 'padded box slots'})))
    P = (5, 5, 1, 3, 2, 1, 0)                                        # overlaps BOX_A in 3.5 < x < 5.5
    shared = line(30, (3.5 + 1 / 16, 5 + 1 / 16, 1 + 1 / 16), 1 / 16)
    own = line(30, (5.5 + 1 / 32, 5 + 1 / 16, 1 + 1 / 16), 1 / 32)
    c.append(AssignCase('best_levels_differ', 2, [[P, A]], [[3, 4]], {(0, 0): shared, (1, 0): own}, False,
                        dict(best=[[1, 0]], branches={'best levels differ'})))
    boxes, pts = _general_scene(11)
    c.append(AssignCase('general_rotated', 2, [boxes, boxes[:2]], [[0, 1, 2], [5, 6]],
                        {(0, 0): pts[0], (1, 0): pts[1], (0, 1): pts[0][::2], (1, 1): pts[1][::3]}, False, dict(branches=set())))
    return c


def check_expectations(case, ref):
    """what the builder promises about a case (raises AssertionError): the table of the issue and the branches the case is there for"""
    e = case.expect
    for key in ('ncand', 'mult', 'above', 'best'):
        if key in e:
            want = e[key] if isinstance(e[key], list) else [[e[key]] * len(case.boxes[s]) for s in range(case.B)]
            got = [[int(ref[key][s, j]) for j in range(len(case.boxes[s]))] for s in range(case.B)]
            assert got == want, f'{case}: {key} {got}, promised {want}'
    missing = e['branches'] - assigner_branches(case, ref)
    assert not missing, f'{case}: does not take {sorted(missing)}'


# =====================================================================================================================================
# head split
# =====================================================================================================================================
HEAD_ROWS = (1, 3, 4, 5, 63, 64, 65, 127, 129)
HEAD_SHAPES = ((64, 6, 18), (32, 6, 18), (25, 6, 18), (64, 8, 10), (64, 6, 57))
HEAD_GUARD = 64


def head_case(n, ld, n_reg, n_cls, scale, seed=0):
    """integer operands (fp32 holds them exactly) and the float64 reference of forward and backward"""
    rng = np.random.default_rng(seed * 1000003 + n * 131 + ld * 7 + n_reg + n_cls)
    y = rng.integers(-3, 4, (n, ld)).astype(np.float64)
    used = 1 + n_reg + n_cls
    y[:, used:] = rng.choice([-3, -2, -1, 1, 2, 3], (n, ld - used))          # pad columns: never zero, never to be read
    d = dict(n=n, ld=ld, n_reg=n_reg, n_cls=n_cls, scale=float(scale), y=y, bias=rng.integers(-4, 5, n_cls).astype(np.float64),
             g_cent=rng.integers(-4, 5, n).astype(np.float64), g_bbox=rng.integers(-4, 5, (n, n_reg)).astype(np.float64),
             g_cls=rng.integers(-4, 5, (n, n_cls)).astype(np.float64), bbox_pred=rng.integers(-4, 5, (n, n_reg)).astype(np.float64))
    reg = y[:, 1:1 + n_reg]
    cls = y[:, 1 + n_reg:used] + d['bias']
    d['fwd'] = dict(centerness=y[:, 0].copy(), bbox_exp=np.exp(reg[:, :6] * scale), bbox_rest=reg[:, 6:].copy(), cls=cls, cls_max=cls.max(1))
    d['bwd'] = head_backward(d, True, True, True)
    return d


def head_backward(d, with_cent, with_bbox, with_cls):
    """gy (n, ld), gscale_row (n), gbias (n_cls), gscale: a missing incoming gradient counts as zeros"""
    n, ld, n_reg, n_cls = d['n'], d['ld'], d['n_reg'], d['n_cls']
    gc = d['g_cent'] if with_cent else np.zeros(n)
    gb = d['g_bbox'] if with_bbox else np.zeros((n, n_reg))
    gk = d['g_cls'] if with_cls else np.zeros((n, n_cls))
    gy = np.zeros((n, ld))
    e = gb[:, :6] * d['bbox_pred'][:, :6]
    gy[:, 0] = gc
    gy[:, 1:7] = e * d['scale']
    gy[:, 7:1 + n_reg] = gb[:, 6:]
    gy[:, 1 + n_reg:1 + n_reg + n_cls] = gk
    row = (e * d['y'][:, 1:7]).sum(1)
    out = dict(gy=gy, gscale_row=row, gbias=gk.sum(0), gscale=np.array([row.sum()]))
    assert all(np.abs(v).max() < 2 ** 24 and np.all(v * 2 == np.round(v * 2)) for v in out.values())
    return out


# =====================================================================================================================================
# losses: values with rigorous fp32 error bounds
# =====================================================================================================================================
class E:
    """v: the float64 value; e: a bound on |what fp32 computes by the same operations - v|"""
    TINY = 2.0 ** -149

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape).copy()

    @staticmethod
    def lift(x):
        return x if isinstance(x, E) else E(x)

    def rnd(self, ulps=0.5):
        return E(self.v, self.e + 2 * ulps * U32 * (np.abs(self.v) + self.e) + E.TINY)

    def __add__(a, b):
        b = E.lift(b)
        return E(a.v + b.v, a.e + b.e).rnd()

    __radd__ = __add__

    def __sub__(a, b):
        b = E.lift(b)
        return E(a.v - b.v, a.e + b.e).rnd()

    def __rsub__(a, b):
        return E.lift(b) - a

    def __mul__(a, b):
        b = E.lift(b)
        return E(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e).rnd()

    __rmul__ = __mul__

    def __truediv__(a, b):
        b = E.lift(b)
        den = np.abs(b.v) - b.e
        assert np.all(den > 0)
        q = a.v / b.v
        return E(q, (a.e + np.abs(q) * b.e) / den).rnd()

    def __rtruediv__(a, b):
        return E.lift(b) / a

    def __neg__(a):
        return E(-a.v, a.e)

    def half(a):
        return E(a.v / 2, a.e / 2)                      # exact (no operand of these tests is denormal)

    def abs(a):
        return E(np.abs(a.v), a.e)

    def exp(a):
        return E(np.exp(a.v), np.exp(a.v) * np.expm1(a.e)).rnd(1.0)

    def log(a):
        rel = a.e / np.abs(a.v)
        assert np.all(rel < 1)
        return E(np.log(a.v), -np.log1p(-rel)).rnd(1.0)

    def log1p(a):
        assert np.all(1 + a.v - a.e > 0)
        return E(np.log1p(a.v), a.e / (1 + a.v - a.e)).rnd(1.0)

    def __getitem__(a, k):
        return E(a.v[k], a.e[k])


def where(c, a, b):
    a, b = E.lift(a), E.lift(b)
    return E(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


GAMMA, ALPHA = 2.0, 0.25
IOU_EPS = float(np.float32(1e-6))
DECIDE = 1e-5                          # general rows: every comparison of the IoU is decided by more than this


def sigmoid_e(x):
    return 1.0 / (1.0 + (-E.lift(x)).exp())


def focal_elem_e(x, is_pos):
    """focal_elem of csrc/loss.hip, gamma = 2 (the plain product)"""
    p = sigmoid_e(x)
    q = 1.0 - p
    pos = (E(-ALPHA) * (q * q)) * where(p.v > FLT_MIN, p, FLT_MIN).log()
    neg = (E(-(1 - ALPHA)) * (p * p)) * where(q.v > FLT_MIN, q, FLT_MIN).log()
    return where(is_pos, pos, neg)


def focal_grad_e(x, is_pos):
    p = sigmoid_e(x)
    q = 1.0 - p
    pos = (E(-ALPHA) * (q * q)) * (q - (E(GAMMA) * p) * where(p.v > FLT_MIN, p, FLT_MIN).log())
    neg = (E(-(1 - ALPHA)) * (p * p)) * ((E(GAMMA) * q) * where(q.v > FLT_MIN, q, FLT_MIN).log() - p)
    return where(is_pos, pos, neg)


def bce_e(x, t):
    x = E.lift(x)
    return (where(x.v > 0, x, 0.0) - x * t) + (-x.abs()).exp().log1p()


def aiou_e(p, t, eps=IOU_EPS, want_grad=True):
    """aiou3d_eval of csrc/loss.hip: p, t lists of six E ([cx,cy,cz,w,l,h]); returns (IoU, [d IoU / d p] * 6), torch's tie rules: max / min
    split 1/2 : 1/2 on equal operands, clamp(min=0) passes at 0"""
    wh, dc, ds, sp = [], [], [], []
    a1 = a2 = ov = E(np.ones_like(p[0].v))
    for a in range(3):
        p1, p2 = p[a] - p[3 + a].half(), p[a] + p[3 + a].half()
        t1, t2 = t[a] - t[3 + a].half(), t[a] + t[3 + a].half()
        lt, wl = where(p1.v > t1.v, p1, t1), np.where(p1.v > t1.v, 1.0, np.where(p1.v == t1.v, 0.5, 0.0))
        rb, wr = where(p2.v < t2.v, p2, t2), np.where(p2.v < t2.v, 1.0, np.where(p2.v == t2.v, 0.5, 0.0))
        d = rb - lt
        passes = np.where(d.v >= 0, 1.0, 0.0)
        wh.append(where(d.v > 0, d, 0.0))
        dc.append(passes * (wr - wl)); ds.append(passes * 0.5 * (wr + wl))             # exact: {0, +-1/2, +-1}
        sp.append(p2 - p1)
        a1, a2, ov = a1 * sp[a], a2 * (t2 - t1), ov * wh[a]
    un = (a1 + a2) - ov
    upass = np.where(un.v > eps, 1.0, 0.0)
    U = where(un.v > eps, un, E(np.full_like(un.v, eps)))
    grads = [None] * 6
    if want_grad:
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            dov = wh[b] * wh[c]
            dov_dc, dov_ds = dov * dc[a], dov * ds[a]
            dU_dc, dU_ds = E(upass) * (-dov_dc), E(upass) * (sp[b] * sp[c] - dov_ds)
            grads[a] = (dov_dc * U - ov * dU_dc) / (U * U)
            grads[3 + a] = (dov_ds * U - ov * dU_ds) / (U * U)
    decided = dict(un=un)
    return ov / U, grads, decided


def iou_margin(pred, target, eps=IOU_EPS):
    """per row, the smallest |difference| any comparison of the IoU decides on (0: an exact tie), float64: faces against faces, the overlap
    extent against 0, the union against eps"""
    pred, target = pred.astype(np.float64), target.astype(np.float64)
    m = np.full(len(pred), np.inf)
    ov, a1, a2 = 1.0, 1.0, 1.0
    for a in range(3):
        p1, p2 = pred[:, a] - pred[:, 3 + a] / 2, pred[:, a] + pred[:, 3 + a] / 2
        t1, t2 = target[:, a] - target[:, 3 + a] / 2, target[:, a] + target[:, 3 + a] / 2
        d = np.minimum(p2, t2) - np.maximum(p1, t1)
        m = np.minimum(m, np.minimum(np.minimum(np.abs(p1 - t1), np.abs(p2 - t2)), np.abs(d)))
        ov, a1, a2 = ov * np.maximum(d, 0), a1 * (p2 - p1), a2 * (t2 - t1)
    return np.minimum(m, np.abs(a1 + a2 - ov - eps))


def decode_e(points, d):
    """decode6: box = [pt + (d1 - d0) / 2, ..., d0 + d1, ...]"""
    pt = [E(points[:, a]) for a in range(3)]
    d = [E(d[:, k]) for k in range(6)]
    return [pt[a] + (d[2 * a + 1] - d[2 * a]).half() for a in range(3)] + [d[2 * a] + d[2 * a + 1] for a in range(3)]


def focal_fp32(x, is_pos, grad):
    """the oracle's fp32 restatement of mmcv's sigmoid focal loss (value or its own backward formula), elementwise, as float64 numbers"""
    with np.errstate(over='ignore', under='ignore'):
        x = x.astype(np.float32)
        one, tiny = np.float32(1), np.float32(FLT_MIN)
        a, g = np.float32(ALPHA), np.float32(GAMMA)
        p = one / (one + np.exp(-x))
        q = one - p
        lp, lq = np.log(np.maximum(p, tiny)), np.log(np.maximum(q, tiny))
        if grad:
            out = np.where(is_pos, -a * (q * q) * (q - g * p * lp), -(one - a) * (p * p) * (g * q * lq - p))
        else:
            out = np.where(is_pos, -a * (q * q) * lp, -(one - a) * (p * p) * lq)
    return out.astype(np.float64)


SAT_LOGITS = (30.0, -30.0, 80.0, -80.0, 100.0, -100.0, 200.0, -200.0)
ROW_GENERAL, ROW_EDGE, ROW_SAT = 0, 1, 2
EDGE_KINDS = ('identical', 'one shared face', 'two shared faces', 'three shared faces', 'touching', 'disjoint', 'pred inside target',
              'target inside pred', 'below eps')
LW = (1.0, 0.5, 2.0)                    # loss weights (exact in fp32)
G_IN = (0.75, 1.5, -0.5)                # incoming scalar gradients g0, g1, g2


def _edge_faces(kind):
    """(pred lo, pred hi, target lo, target hi), dyadic"""
    t_lo, t_hi = np.array([1.0, -2.0, 0.5]), np.array([3.0, 1.0, 2.0])
    p_lo, p_hi = t_lo + np.array([0.5, -0.25, 0.25]), t_hi + np.array([0.75, -0.5, 0.5])        # partial overlap, no shared face
    if kind == 'identical':
        p_lo, p_hi = t_lo.copy(), t_hi.copy()
    elif kind.endswith('shared face') or kind.endswith('shared faces'):
        k = {'one': 1, 'two': 2, 'three': 3}[kind.split()[0]]
        p_lo[0] = t_lo[0]
        if k > 1:
            p_hi[1] = t_hi[1]
        if k > 2:
            p_lo[2] = t_lo[2]
    elif kind == 'touching':
        p_lo[0], p_hi[0] = t_lo[0] - 1.5, t_lo[0]
    elif kind == 'disjoint':
        p_lo[0], p_hi[0] = t_lo[0] - 2.0, t_lo[0] - 0.5
    elif kind == 'pred inside target':
        p_lo, p_hi = t_lo + 0.25, t_hi - 0.5
    elif kind == 'target inside pred':
        p_lo, p_hi = t_lo - 0.5, t_hi + 0.25
    elif kind == 'below eps':
        t_lo = np.array([1.0, -2.0, 0.5]); t_hi = t_lo + 2.0 ** -7
        p_lo = t_lo + 2.0 ** -8; p_hi = p_lo + 2.0 ** -7
    return p_lo, p_hi, t_lo, t_hi


def _general_row(rng):
    while True:
        tc, ts = rng.uniform(-2, 2, 3), rng.uniform(0.5, 2.0, 3)
        pt = tc + rng.uniform(-0.2, 0.2, 3)
        d = np.repeat(ts / 2, 2) * rng.uniform(0.6, 1.4, 6)
        pt, d, bt = _f32(pt), _f32(d), _f32(np.concatenate([tc, ts, [0.5]]))
        box = np.array([[float(pt[a]) + (float(d[2 * a + 1]) - float(d[2 * a])) / 2 for a in range(3)] + [float(d[2 * a]) + float(d[2 * a + 1]) for a in range(3)]])
        if iou_margin(box, bt[None, :6])[0] > 10 * DECIDE:
            return pt, d, bt


class LossCase:
    pass


def loss_case(N, C, seed=0, only=None):
    """one launch of N rows: every row class in it (N >= 255), or the single class `only` = (row class, edge kind index)"""
    rng = np.random.default_rng(seed * 7919 + N * 37 + C)
    c = LossCase()
    c.N, c.C, c.B = N, C, 3
    kinds = np.full(N, ROW_GENERAL)
    edge = np.full(N, -1)
    if only is None:
        assert N >= 64
        where_ = rng.permutation(N)
        kinds[where_[:2 * len(EDGE_KINDS)]] = ROW_EDGE
        edge[where_[:2 * len(EDGE_KINDS)]] = np.arange(2 * len(EDGE_KINDS)) % len(EDGE_KINDS)
        kinds[where_[2 * len(EDGE_KINDS):2 * len(EDGE_KINDS) + 24]] = ROW_SAT
        sat_rows = where_[2 * len(EDGE_KINDS):2 * len(EDGE_KINDS) + 24]
    else:
        kinds[:] = only[0]
        edge[:] = only[1] if only[0] == ROW_EDGE else -1
        sat_rows = np.nonzero(kinds == ROW_SAT)[0]
    c.kind, c.edge = kinds, edge
    c.scene = rng.integers(0, 3, N).astype(np.int32)
    if only is not None:
        c.scene[:] = 0
    special = np.nonzero(kinds != ROW_GENERAL)[0]
    c.scene[special] = np.where(np.arange(len(special)) % 2 == 0, 0, 2) if only is None else 0       # scene 1 has no positive: none of these
    c.points, c.bbox_pred, c.bt = np.zeros((N, 3), np.float32), np.zeros((N, 6), np.float32), np.zeros((N, 7), np.float32)
    for r in range(N):
        if kinds[r] == ROW_EDGE:
            p_lo, p_hi, t_lo, t_hi = _edge_faces(EDGE_KINDS[edge[r]])
            pt = p_lo + (p_hi - p_lo) / 4
            c.points[r], c.bbox_pred[r, 0::2], c.bbox_pred[r, 1::2] = pt, pt - p_lo, p_hi - pt
            c.bt[r] = np.concatenate([(t_lo + t_hi) / 2, t_hi - t_lo, [0.5]])
        else:
            c.points[r], c.bbox_pred[r], c.bt[r] = _general_row(rng)
    c.cls = _f32(rng.uniform(-12, 12, (N, C)))
    c.centerness = _f32(rng.uniform(-12, 12, N))
    c.labels = rng.choice([-1, 0, C - 1], N).astype(np.int64)
    for k, r in enumerate(sat_rows):
        c.cls[r] = [SAT_LOGITS[(k + col) % 8] for col in range(C)]
        c.labels[r] = (-1, 0, C - 1)[k % 3]
    if only is not None and only[0] == ROW_SAT:
        c.cls[0] = [SAT_LOGITS[(only[1] + col) % 8] for col in range(C)]
        c.labels[0] = (-1, 0, C - 1)[only[1] % 3]
    edge_rows = kinds == ROW_EDGE
    if only is not None and only[0] == ROW_GENERAL:
        c.labels[:] = 0
    c.labels[edge_rows] = np.where(c.labels[edge_rows] < 0, 0, c.labels[edge_rows])            # edge rows carry weight: their gradients are the point
    c.labels[c.scene == 1] = -1                                                               # scene 1 has no positive
    c.ct = _f32(np.where(c.labels >= 0, rng.integers(1, 65, N) / 64, 0.0))
    plain = np.nonzero((c.labels >= 0) & ~edge_rows)[0]
    c.ct[plain[3::8]] = 0.0                                                                    # positives of weight 0
    npos = np.array([max(int(((c.scene == s) & (c.labels >= 0)).sum()), 1) for s in range(3)], dtype=np.float64)
    den = np.array([max(float(c.ct[c.scene == s].astype(np.float64).sum()), 1e-6) for s in range(3)])
    c.inv_pos, c.inv_den = _f32(1.0 / (3 * npos)), _f32(1.0 / (3 * den))
    c.sat_rows = np.nonzero(kinds == ROW_SAT)[0]
    return c


def loss_items(N, C):
    """the launches of one (N, C) item: one with every row class, or — a single row cannot hold them — one per row class"""
    if N >= 64:
        return [loss_case(N, C)]
    return ([loss_case(N, C, only=(ROW_GENERAL, -1))] + [loss_case(N, C, seed=k, only=(ROW_EDGE, k)) for k in range(len(EDGE_KINDS))]
            + [loss_case(N, C, seed=k, only=(ROW_SAT, k)) for k in range(24)])


def loss_violations(c):
    bad = []
    box = np.stack([e.v for e in decode_e(c.points.astype(np.float64), c.bbox_pred.astype(np.float64))], 1)
    m = iou_margin(box, c.bt[:, :6])
    gen, edge = c.kind != ROW_EDGE, c.kind == ROW_EDGE
    if np.any(m[gen] <= DECIDE):
        bad.append(f'a general row decides a comparison by {m[gen].min():.2e}')
    vals = np.concatenate([c.points[edge].ravel(), c.bbox_pred[edge].ravel(), c.bt[edge, :6].ravel()]).astype(np.float64)
    if np.any(vals * 512 != np.round(vals * 512)) or (vals.size and np.abs(vals).max() >= 16):
        bad.append('an edge row is not dyadic (multiples of 2^-9 below 16)')
    if np.abs(c.cls[c.kind != ROW_SAT]).max(initial=0) > 12 or np.abs(c.centerness).max() > 12:
        bad.append('a general logit leaves [-12, 12]')
    if np.any((c.labels >= 0) & (c.scene == 1)) or np.any(c.ct[c.labels < 0] != 0):
        bad.append('scene 1 holds a positive, or a background row a weight')
    if c.N >= 64:
        w = c.ct > 0
        if {int(k) for k in c.edge[edge & w]} != set(range(len(EDGE_KINDS))):
            bad.append('an edge kind is missing among the rows of weight')
        is_pos = c.labels[:, None] == np.arange(c.C)[None, :]
        sat = c.kind == ROW_SAT
        if {(float(v), bool(q)) for v, q in zip(c.cls[sat].ravel(), is_pos[sat].ravel())} != {(v, q) for v in SAT_LOGITS for q in (True, False)}:
            bad.append('a saturated logit is missing for a positive or a negative label')
        if not (np.any((c.labels >= 0) & (c.ct == 0)) and np.any(c.labels < 0) and np.any(c.scene == 1)):
            bad.append('no positive of weight 0, no background row or no row of scene 1')
    return bad


def loss_reference(c, g=G_IN, lw=LW):
    """the three losses and the three gradients as E (value, fp32 bound), in the kernels' operation order.  g[i] None: that loss is not
    part of the objective.  Saturated rows: class terms and class gradients from focal_fp32, bound 1e-6 |value| + FLT_MIN.
    Sums: per-row values as the kernel forms them (class terms added in column order), then summed; the bound of a sum is the sum of the
    rows' bounds + (6 + 2) u sum |row| for the wave and block trees + 2 u |sum| for the cast from double and the loss weight."""
    N, C = c.N, c.C
    f64 = lambda a: a.astype(np.float64)
    s = c.scene
    wp, wd = E(f64(c.inv_pos)[s]), E(f64(c.inv_den)[s])
    is_pos = c.labels[:, None] == np.arange(C)[None, :]
    sat = (c.kind == ROW_SAT)[:, None] & np.ones((1, C), bool)
    x = f64(c.cls)

    def with_sat(e, grad):
        v32 = focal_fp32(c.cls, is_pos, grad)
        return where(sat, E(v32, 1e-6 * np.abs(v32) + FLT_MIN), e)
    terms = with_sat(focal_elem_e(np.where(sat, 0.0, x), is_pos), False)
    acc = E(np.zeros(N))
    for col in range(C):
        acc = acc + terms[:, col]
    v0 = acc * wp
    ct = E(f64(c.ct))
    v1 = where(c.labels >= 0, bce_e(f64(c.centerness), ct) * wp, 0.0)
    w = ct * wd
    box = decode_e(f64(c.points), f64(c.bbox_pred))
    tgt = [E(f64(c.bt[:, k])) for k in range(6)]
    iou, dp, _ = aiou_e(box, tgt)
    v2 = where(w.v > 0, (1.0 - iou) * w, 0.0)

    def total(v, lwj):
        sm = float(v.v.sum())
        return E(np.array(lwj * sm), abs(lwj) * (float(v.e.sum()) + 8 * U32 * float(np.abs(v.v).sum() + v.e.sum()) + 2 * U32 * abs(sm)) + E.TINY)
    out = dict(loss_cls=total(v0, lw[0]), loss_cent=total(v1, lw[1]), loss_bbox=total(v2, lw[2]), rows=(v0, v1, v2), iou=iou, w=w)
    zero = E(np.zeros(N))
    if g[0] is None:
        out['gcls'] = E(np.zeros((N, C)))
    else:
        s0 = (E(g[0]) * lw[0]) * wp
        ge = with_sat(focal_grad_e(np.where(sat, 0.0, x), is_pos), True)
        out['gcls'] = ge * E(s0.v[:, None], s0.e[:, None])
    if g[1] is None:
        out['gcent'] = zero
    else:
        out['gcent'] = where(c.labels >= 0, (sigmoid_e(f64(c.centerness)) - ct) * ((E(g[1]) * lw[1]) * wp), 0.0)
    gb = [zero] * 6
    if g[2] is not None:
        sc = -((E(g[2]) * lw[2]) * w)
        for a in range(3):
            gb[2 * a] = where(w.v > 0, sc * (dp[3 + a] - dp[a].half()), 0.0)
            gb[2 * a + 1] = where(w.v > 0, sc * (dp[3 + a] + dp[a].half()), 0.0)
    out['gbbox'] = E(np.stack([e.v for e in gb], 1), np.stack([e.e for e in gb], 1))
    return out


# rotated IoU, where it is well-posed: yaw 0 on both, partial overlap or containment without a shared face; disjoint pairs; weight-0 rows
def riou_cases():
    rng = np.random.default_rng(5)
    pred, tgt, kind = [], [], []
    for k in range(40):
        tc, ts = rng.uniform(-2, 2, 3), rng.uniform(1.0, 2.0, 3)
        if k % 4 == 0:                                               # pred inside target
            pc, ps = tc + rng.uniform(-0.1, 0.1, 3), ts * rng.uniform(0.4, 0.6, 3)
        elif k % 4 == 1:                                             # target inside pred
            pc, ps = tc + rng.uniform(-0.1, 0.1, 3), ts * rng.uniform(1.5, 1.8, 3)
        elif k % 4 == 2:                                             # partial overlap on every axis
            pc, ps = tc + ts * rng.choice([-1, 1], 3) * rng.uniform(0.3, 0.5, 3), ts * rng.uniform(0.8, 1.2, 3)
        else:                                                        # disjoint in x
            pc, ps = tc + np.array([ts[0] * 2.5, 0.3, -0.3]), ts * rng.uniform(0.8, 1.2, 3)
        pred.append(np.concatenate([pc, ps, [0.0]])); tgt.append(np.concatenate([tc, ts, [0.0]])); kind.append(k % 4)
    pred, tgt, kind = _f32(pred), _f32(tgt), np.array(kind)
    iou, dp, _ = aiou_e([E(pred[:, k].astype(np.float64)) for k in range(6)], [E(tgt[:, k].astype(np.float64)) for k in range(6)])
    margin = iou_margin(pred[:, :6], tgt[:, :6])
    assert margin.min() > 1e-2                                       # no shared face, no touching pair
    return dict(pred=pred, target=tgt, kind=kind, iou=iou.v, grad=np.stack([e.v for e in dp], 1))


def focal_reference(c, gscale):
    """the standalone focal kernels on (cls, labels, row weight inv_pos[scene]): loss_rows = acc * w; gx = (g * gscale) * w"""
    f64 = lambda a: a.astype(np.float64)
    w = E(f64(c.inv_pos)[c.scene])
    is_pos = c.labels[:, None] == np.arange(c.C)[None, :]
    sat = (c.kind == ROW_SAT)[:, None] & np.ones((1, c.C), bool)
    x = np.where(sat, 0.0, f64(c.cls))

    def with_sat(e, grad):
        v32 = focal_fp32(c.cls, is_pos, grad)
        return where(sat, E(v32, 1e-6 * np.abs(v32) + FLT_MIN), e)
    terms = with_sat(focal_elem_e(x, is_pos), False)
    acc = E(np.zeros(c.N))
    for col in range(c.C):
        acc = acc + terms[:, col]
    grad = (with_sat(focal_grad_e(x, is_pos), True) * gscale) * E(w.v[:, None], w.e[:, None])
    return acc * w, grad


def aiou_reference(pred, target):
    """fc_aiou3d_fwd_bwd on fp32 boxes taken as they are: (IoU, d IoU / d pred (n, 6)) as E"""
    iou, dp, _ = aiou_e([E(pred[:, k].astype(np.float64)) for k in range(6)], [E(target[:, k].astype(np.float64)) for k in range(6)])
    return iou, E(np.stack([e.v for e in dp], 1), np.stack([e.e for e in dp], 1))


def decoded_boxes(c):
    """the decoded prediction of every row, rounded to fp32 (exact on the edge rows)"""
    return _f32(np.stack([e.v for e in decode_e(c.points.astype(np.float64), c.bbox_pred.astype(np.float64))], 1))
