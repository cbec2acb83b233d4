"""Cases and numpy references of the exact coordinate tests (tests/test_coord_cases_cpu.py, tests/test_gpu_coords_exact.py,
tests/test_gpu_plan_exact.py).  Nothing here touches a GPU.

Both coordinate phases — the per-operator entry points (csrc/coords.hip) and the native plan (csrc/plan.hip with plan_chain.h,
plan_maps.h, plan_radix.h) — share the rules of csrc/coord_rules.h and csrc/fc_common.h, so comparing one with the other cannot see a
mistake in a shared rule.  This module
  * restates those rules on plain integers: `fc_pack`, `fc_mix`, the capacity rule, a linear-probing insert / lookup, the quantiser,
    the range predicate, the candidate arithmetic of the strided maps, the block arithmetic of the winners' positions, of the pair
    lists and of the -1 prefill — each with the one-token MUTATIONS a case is there to reject (keyword arguments; the CPU test shows
    that the expected tables change under them, nothing mutated is ever built or run on a GPU);
  * states the references: sets (`unique_first`, `chain`), kernel maps, nbr_t, pair lists, live tiles, row masks, the mask-sorted
    table, generated sets with their maps, child / union rows, the head arrays — on keys of 18 bits per axis (`wide_keys`), so a
    16-bit alias of the device keys shows as a false neighbour; oracle/me_oracle.py is the second opinion the CPU test holds them to;
  * builds the cases (`cases()`, `raw_cases()`): rows (b, x, y, z) int32, the batch size, the pyramid depth the plan runs them with, and the branch
    facts each case claims (recomputed and asserted by the CPU test).
"""
import functools
from collections import namedtuple

import numpy as np

LIMIT = 32639                                    # FC_COORD_LIMIT
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)            # FC_EMPTY_KEY
VAL_INIT = 0x7fffffff
SENT = -7                                        # what a test pre-fills its own integer output buffers with


# ---- restatements of the shared rules -------------------------------------------------------------------------------------------
def fc_pack(c):
    """(n, 4) int (b, x, y, z) -> uint64 keys: 16 bits of batch index, 16 bits per axis with a 2^15 bias (fc_common.h)"""
    c = np.asarray(c).astype(np.int64).reshape(-1, 4)
    f = [(c[:, 0] & 0xFFFFFFFF).astype(np.uint64)] + [((c[:, a] + 32768) & 0xFFFFFFFF).astype(np.uint64) for a in (1, 2, 3)]
    return (f[0] << np.uint64(48)) | (f[1] << np.uint64(32)) | (f[2] << np.uint64(16)) | f[3]


def fc_mix(k):
    k = np.atleast_1d(np.asarray(k, dtype=np.uint64)).copy()
    s = np.uint64(33)
    k ^= k >> s
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> s
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> s
    return k


def capacity(n_in):
    """slots of the table of a set whose INPUT has n_in rows: next_pow2(2 n_in), at least 2 (plan_chain.h table_mask,
    sparse.CoordMap.from_coords)"""
    cap = 2
    while cap < 2 * n_in:
        cap *= 2
    return cap


def home(c, cap):
    return (fc_mix(fc_pack(c)) & np.uint64(cap - 1)).astype(np.int64)


def table_insert(c, cap, last_wins=False):
    """rows in order into an open-addressing table -> (keys uint64 (cap,), vals (cap,), slot of every row).  The value is the smallest
    row of the key (fc_hash_insert: atomicMin).  WHICH key of a probe chain sits in which slot depends on the order of insertion —
    on the device: on timing —, the SET of occupied slots does not (linear probing), and that set is what a test may predict."""
    keys = np.full(cap, EMPTY, dtype=np.uint64)
    vals = np.full(cap, VAL_INIT, dtype=np.int64)
    pk, hm = fc_pack(c), home(c, cap)
    slot = np.empty(len(pk), dtype=np.int64)
    for i in range(len(pk)):
        h = int(hm[i])
        while keys[h] != EMPTY and keys[h] != pk[i]:
            h = (h + 1) & (cap - 1)
        keys[h] = pk[i]
        vals[h] = i if last_wins else min(int(vals[h]), i)
        slot[i] = h
    return keys, vals, slot


def table_lookup(keys, vals, q, stop_at_first=False, no_wrap=False):
    """fc_lookup of every row of q -> value | -1.  Mutations: give up at the first slot that holds another key; walk off the end of
    the table instead of wrapping to slot 0 (stated as a miss)"""
    cap = len(keys)
    pk, hm = fc_pack(q), home(q, cap)
    out = np.full(len(pk), -1, dtype=np.int64)
    for i in range(len(pk)):
        h = int(hm[i])
        while True:
            if keys[h] == pk[i]:
                out[i] = vals[h]
                break
            if keys[h] == EMPTY or stop_at_first:
                break
            h += 1
            if h == cap:
                if no_wrap:
                    break
                h = 0
    return out


def probe_path_ok(keys):
    """every key of a table sits on the probe path from its home slot with no empty slot before it"""
    cap = len(keys)
    for h in np.nonzero(keys != EMPTY)[0]:
        g = int(fc_mix(keys[h])[0] & np.uint64(cap - 1))
        while g != h:
            if keys[g] == EMPTY:
                return False
            g = (g + 1) & (cap - 1)
    return True


def quantize(c, q, trunc=False):
    """every axis rounded DOWN to a multiple of q (fc_quantize).  Mutation: C's truncating division"""
    c = np.asarray(c).astype(np.int64).copy()
    if q > 1:
        x = c[:, 1:]
        c[:, 1:] = (np.trunc(x / q).astype(np.int64) if trunc else np.floor_divide(x, q)) * q
    return c


def out_of_range(c, limit=LIMIT):
    """fc_coord_out_of_range, row by row"""
    c = np.asarray(c).astype(np.int64).reshape(-1, 4)
    return (c[:, 0] < 0) | (c[:, 0] > 32767) | (np.abs(c[:, 1:]) > limit).any(axis=1)


# ---- references -------------------------------------------------------------------------------------------------------------------
def wide_keys(c):
    """injective int64 keys with 18 bits per axis (|c| < 2^17) and 9 bits of batch index: no alias where the device's 16-bit fields
    could have one"""
    c = np.asarray(c).astype(np.int64).reshape(-1, 4)
    assert len(c) == 0 or (c[:, 0].min() >= 0 and c[:, 0].max() < 512 and np.abs(c[:, 1:]).max() < (1 << 17))
    o = 1 << 17
    return (c[:, 0] << 54) | ((c[:, 1] + o) << 36) | ((c[:, 2] + o) << 18) | (c[:, 3] + o)


def unique_first(c, last_wins=False):
    """unique rows in order of first occurrence -> (rows, first-occurrence row of each (ascending), inverse).  Mutation: the LAST
    occurrence names the row (and its place)"""
    c = np.asarray(c)
    k = wide_keys(c)
    if last_wins:
        _, f, inv = np.unique(k[::-1], return_index=True, return_inverse=True)
        f, inv = len(k) - 1 - f, inv[::-1]
    else:
        _, f, inv = np.unique(k, return_index=True, return_inverse=True)
    order = np.argsort(f, kind='stable')
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return c[f[order]], f[order].astype(np.int64), rank[inv.reshape(-1)].astype(np.int64)


Set = namedtuple('Set', 'coords first inverse stride n_in')


def _memo_key(rows, *a):
    rows = np.ascontiguousarray(rows)
    return (rows.shape, rows.dtype.str, hash(rows.tobytes())) + a


_chains = {}


def chain(rows, n_sets, trunc=False, last_wins=False):
    """memoised `_chain` (the million-row case is asked for by several tests)"""
    k = _memo_key(rows, n_sets, trunc, last_wins)
    if k not in _chains:
        _chains[k] = _chain(rows, n_sets, trunc, last_wins)
    return _chains[k]


def _chain(rows, n_sets, trunc=False, last_wins=False):
    """the pyramid of sets: set 0 = unique rows, set s = unique rows of floor(set s-1 / 2^s) * 2^s; `first` / `inverse` refer to the
    rows of the set's INPUT (all rows for set 0, the previous set's rows after it)"""
    sets, cur = [], np.asarray(rows, dtype=np.int32)
    for s in range(n_sets):
        uc, f, inv = unique_first(quantize(cur, 1 << s, trunc).astype(np.int32), last_wins)
        sets.append(Set(uc, f, inv, 1 << s, len(cur)))
        cur = uc
    return sets


def offsets(ks, stride):
    """(K, 3) kernel offsets, x fastest; centred for odd kernels, {0 .. k-1} for even"""
    r = (np.arange(ks) - ks // 2 if ks % 2 else np.arange(ks)) * stride
    return np.array([(dx, dy, dz) for dz in r for dy in r for dx in r], dtype=np.int64)


def kernel_map(cin, cout, ks, stride):
    """nbr (K, n_out): row of the input voxel at out + offset_k, or -1"""
    offs = offsets(ks, stride)
    nbr = np.full((len(offs), len(cout)), -1, dtype=np.int32)
    if len(cin) == 0 or len(cout) == 0:
        return nbr
    ik = wide_keys(cin)
    order = np.argsort(ik, kind='stable')
    sk = ik[order]
    for k, d in enumerate(offs):
        q = np.asarray(cout).astype(np.int64).copy()
        q[:, 1:] += d
        qk = wide_keys(q)
        pos = np.minimum(np.searchsorted(sk, qk), len(sk) - 1)
        hit = sk[pos] == qk
        nbr[k, hit] = order[pos[hit]]
    return nbr


def strided_map_from_input(cin, cout, ks, s, trunc=False, prefill_tail=True):
    """the table of a map stride s -> 2 s as k_plan_strided_maps builds it: pre-filled with -1, then every input row writes itself
    at its candidate output voxels (per axis q = floor(p / 2s) * 2s, r = p - q: ks = 2 -> offset r / s at q; ks = 3 -> r = 0:
    offset 0 at q, r = s: offset +s at q and offset -s at q + 2s).  Mutations: truncating division for q; a prefill that leaves the
    last K n mod 4 entries as they were (SENT)"""
    K, n_out, s2 = ks ** 3, len(cout), 2 * s
    flat = np.full(K * n_out, -1, dtype=np.int32)
    if not prefill_tail and (K * n_out) % 4:
        flat[-((K * n_out) % 4):] = SENT
    nbr = flat.reshape(K, n_out)
    row_of = {int(k): i for i, k in enumerate(wide_keys(cout))}
    for i, p in enumerate(np.asarray(cin).astype(np.int64)):
        cand = []
        for d in range(3):
            x = int(p[1 + d])
            q = (int(np.trunc(x / s2)) if trunc else x // s2) * s2
            r = x - q
            if ks == 2:
                cand.append([(q, r // s)])
            elif r == 0:
                cand.append([(q, 1)])
            else:
                cand.append([(q, 2), (q + s2, 0)])
        for cx, kx in cand[0]:
            for cy, ky in cand[1]:
                for cz, kz in cand[2]:
                    if max(abs(cx), abs(cy), abs(cz)) >= (1 << 17):
                        continue
                    o = row_of.get(int(wide_keys([[p[0], cx, cy, cz]])[0]))
                    if o is not None and 0 <= kx + ks * ky + ks * ks * kz < K:
                        nbr[kx + ks * ky + ks * ks * kz, o] = i
    return nbr


def transpose(nbr, n_in):
    """nbr_t[k][i] = o  iff  nbr[k][o] == i"""
    t = np.full((nbr.shape[0], n_in), -1, dtype=np.int32)
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        t[k, nbr[k, o]] = o
    return t


PAIR_BLOCK = 1024


def pair_lists(nbr, max_prefix_blocks=None):
    """(pair_in, pair_out, pos, cnt) of a (K, n) table: per offset the pairs in ascending output row; entries behind a list are SENT.
    Stated as the kernels count: a list position = pairs of the 1 024-row blocks in front + the rank inside the block.  Mutation:
    the prefix adds up at most `max_prefix_blocks` block counts"""
    K, n = nbr.shape
    pi, po = np.full((K, n), SENT, dtype=np.int32), np.full((K, n), SENT, dtype=np.int32)
    pos = np.full((K, n), -1, dtype=np.int32)
    cnt = np.zeros(K, dtype=np.int32)
    nblk = max((n + PAIR_BLOCK - 1) // PAIR_BLOCK, 1)
    for k in range(K):
        present = nbr[k] >= 0
        blk_cnt = np.add.reduceat(present.astype(np.int64), np.arange(0, max(n, 1), PAIR_BLOCK))[:nblk] if n else np.zeros(1, np.int64)
        base = np.zeros(nblk, dtype=np.int64)
        for b in range(nblk):
            base[b] = blk_cnt[:b if max_prefix_blocks is None else min(b, max_prefix_blocks)].sum()
        o = np.nonzero(present)[0]
        within = np.cumsum(present) - 1 - np.repeat(np.cumsum(blk_cnt) - blk_cnt, PAIR_BLOCK)[:n]
        j = (base[o // PAIR_BLOCK] + within[o]).astype(np.int64)
        pi[k, j], po[k, j], pos[k, o] = nbr[k, o], o, j
        cnt[k] = base[-1] + blk_cnt[-1] if n else 0
    return pi, po, pos, cnt


def live_tiles(cnt):
    return int(((np.asarray(cnt).astype(np.int64) + 127) // 128).sum())


def row_masks(nbr):
    m = np.zeros(nbr.shape[1], dtype=np.int64)
    for k in range(nbr.shape[0]):
        m |= (nbr[k] >= 0).astype(np.int64) << k
    return m.astype(np.int32)


def mask_sorted(nbr):
    """(table in mask order, order): a STABLE argsort of the row masks"""
    order = np.argsort(row_masks(nbr), kind='stable').astype(np.int32)
    return nbr[:, order], order


def winner_positions(flags, max_coarse=None):
    """k_plan_finalize: output row of every winner = winners of the 1 024-row blocks in front (the `coarse` counts) + its rank
    inside the block; -> (positions of the winners, rows of the set).  Mutation: at most `max_coarse` coarse counts are added"""
    flags = np.asarray(flags).astype(np.int64)
    n = len(flags)
    coarse = np.add.reduceat(flags, np.arange(0, n, 1024)) if n else np.zeros(0, np.int64)
    lim = len(coarse) if max_coarse is None else max_coarse
    before = np.array([coarse[:min(b, lim)].sum() for b in range(len(coarse))], dtype=np.int64)
    within = np.cumsum(flags) - flags - np.repeat(np.cumsum(coarse) - coarse, 1024)[:n]
    w = np.nonzero(flags)[0]
    return before[w // 1024] + within[w], int(coarse[:lim].sum())


def gen_coords(coarse, stride):
    """children set of a set of stride `stride`: row 8 i + k at coarse_i + bits(k) * stride / 2"""
    h = stride // 2
    bits = np.array([[k & 1, (k >> 1) & 1, (k >> 2) & 1] for k in range(8)], dtype=np.int64) * h
    c = np.repeat(np.asarray(coarse).astype(np.int64), 8, axis=0)
    c[:, 1:] += np.tile(bits, (len(coarse), 1))
    return c.astype(np.int32)


def rows_in(cset, q):
    """row of every voxel of q in cset, or -1"""
    if len(cset) == 0:
        return np.full(len(q), -1, dtype=np.int32)
    ck = wide_keys(cset)
    order = np.argsort(ck, kind='stable')
    qk = wide_keys(q)
    pos = np.minimum(np.searchsorted(ck[order], qk), len(ck) - 1)
    return np.where(ck[order][pos] == qk, order[pos], -1).astype(np.int32)


def child_rows(q, parent, child_stride, trunc=False):
    """fc_child_rows / k_plan_gen_rows by their own arithmetic: 8 * (row of the parent cell) + child bits, or -1"""
    T, P = child_stride, 2 * child_stride
    q = np.asarray(q).astype(np.int64)
    cell = quantize(q, P, trunc)
    r = rows_in(parent, cell).astype(np.int64)
    d = (q[:, 1:] - cell[:, 1:]) // T
    return np.where(r < 0, -1, 8 * r + (d[:, 0] | (d[:, 1] << 1) | (d[:, 2] << 2))).astype(np.int32)


def head_arrays(level_sets, B, vs):
    """the head's location arrays over the levels, finest first: pts = float32(c) * float32(vs), scene, level, order, and the
    (level, scene) segment starts (rows of every set are grouped by scene)"""
    c = np.concatenate(level_sets)
    pts = c[:, 1:].astype(np.float32) * np.float32(vs)
    level = np.concatenate([np.full(len(s), l, dtype=np.int32) for l, s in enumerate(level_sets)])
    seg = np.concatenate([[0], np.cumsum(np.concatenate([np.bincount(s[:, 0], minlength=B)[:B] for s in level_sets]))]).astype(np.int32)
    return dict(pts=pts, scene=c[:, 0].astype(np.int32), level=level, order=np.arange(len(c), dtype=np.int32), seg_start=seg)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
Case = namedtuple('Case', 'rows B nl facts kind')       # kind: 'graph' | 'hash' | 'chain_big' | 'map_big' | 'refuse' | 'raw'


def _rows(b, xyz):
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([np.full((len(xyz), 1), b, np.int64), xyz], axis=1).astype(np.int32)


def _cube(lo, hi, step=1):
    r = np.arange(lo, hi, step)
    return np.array([(x, y, z) for z in r for y in r for x in r], dtype=np.int64)


def _shuffle(rows, seed):
    return rows[np.random.default_rng(seed).permutation(len(rows))]


def _two_level(n_out, n_in, s, seed, B=1):
    """n_in voxels of stride s inside exactly n_out cells of stride 2 s, in a box around the origin a third full"""
    rng = np.random.default_rng(seed)
    side = max(int(np.ceil((3.0 * n_out) ** (1 / 3))), 2)
    cells = _cube(-(side // 2), side - side // 2)
    cells = cells[rng.permutation(len(cells))[:n_out]]
    assert len(cells) == n_out and n_out <= n_in <= 8 * n_out
    # the last three cells have no child 6 / 7: the last entries of the (27, n_out) table — offsets 25, 26 of the last rows, what a
    # prefill in groups of four leaves to its tail — are true -1 entries that no input row writes
    allowed = [list(range(8 if i < n_out - 3 else 6)) for i in range(n_out)]
    kids = [[int(rng.choice(allowed[i]))] for i in range(n_out)]
    extra = n_in - n_out
    while extra:
        i = int(rng.integers(n_out))
        k = int(rng.choice(allowed[i]))
        if k not in kids[i]:
            kids[i].append(k)
            extra -= 1
    xyz = np.array([cells[i] * 2 * s + np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1]) * s for i in range(n_out) for k in kids[i]])
    b = np.repeat(np.sort(rng.integers(0, B, size=n_out)), [len(k) for k in kids])          # a cell belongs to one scene; rows grouped by scene
    return np.concatenate([b[:, None], xyz], axis=1).astype(np.int32)


def _lattice_with_homes(cap, step=1, b=0, side=24):
    """{home slot: [rows]} of a small lattice at capacity cap"""
    r = _rows(b, _cube(-(side // 2) * step, (side - side // 2) * step, step))
    hm = home(r, cap)
    return {h: r[hm == h] for h in range(cap)}


def _hash_case(step, stride2):
    """24 distinct voxels made for a table of 64 slots: 9 keys whose home is slot 61 (they fill 61, 62, 63, 0 .. 5: the probe wraps
    through slot 0), 5 keys at home in slots 1 .. 5, pushed behind the chain into 6 .. 10, 10 keys alone in their home slots
    12, 14 .. 30; slot 11 stays empty.  Then duplicates of chain keys (the smallest row must win).
    stride2: the voxels are even, three odd rows fall onto chain keys at stride 2 (duplicates of THAT insert) and more duplicates
    give the level-0 table 128 slots: the chain forms in the stride-2 table only.
    -> rows, absent keys (homes 61: first slot of the run, 2: middle, 10: last, 11: an empty slot, 40), predicted occupied slots"""
    by = _lattice_with_homes(64, step)
    chain_rows = by[61][:9]
    pushed = np.concatenate([by[h][:1] for h in (1, 2, 3, 4, 5)])
    alone = np.concatenate([by[h][:1] for h in range(12, 32, 2)])
    uniq = np.concatenate([chain_rows[:4], alone[:5], chain_rows[4:], pushed, alone[5:]])
    dups = np.concatenate([chain_rows[8:9]] * 3 + [chain_rows[0:1], pushed[4:5]])
    rows = np.concatenate([uniq[:15], dups[:2], uniq[15:], dups[2:]])
    if stride2:
        odd = np.concatenate([chain_rows[8:9], chain_rows[3:4], pushed[0:1]])
        odd[:, 1:] += 1
        rows = np.concatenate([rows, odd, uniq[::-1][:8]])
    absent = np.concatenate([by[61][9:10], by[2][1:2], by[10][:1], by[11][:1], by[40][:1]])
    occupied = sorted([61, 62, 63] + list(range(0, 11)) + list(range(12, 32, 2)))
    return rows, absent, occupied


def _range_rows():
    L_ = LIMIT
    pts = [(sx * L_, sy * L_, sz * L_) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    for a in range(3):
        for sg in (-1, 1):
            p = [0, 0, 0]
            p[a] = sg * L_
            pts.append(tuple(p))
            p2 = [5, -7, 11]
            p2[a] = sg * (L_ - 64)                                  # the neighbour one coarsest voxel inside
            pts.append(tuple(p2))
    pts = np.array(pts)
    return np.concatenate([_rows(0, pts), _rows(1, pts[::-1]), _rows(2, pts[:3])])


@functools.lru_cache(maxsize=None)
def cases():
    cs = {}

    def add(name, rows, B, nl=2, kind='graph', **facts):
        assert name not in cs
        cs[name] = Case(np.ascontiguousarray(rows, dtype=np.int32), B, nl, facts, kind)
    # -- sign and parity
    for s in (1, 2, 4):
        blk = _cube(-s, s + 1, s)
        add(f'block3_s{s}', _rows(0, blk), 1, sign='both')
        add(f'block3_s{s}_negative_odd', _rows(0, blk - (s + 1 if s % 2 == 0 else s + 2)), 1, sign='negative', odd=s % 2 == 0)
        add(f'isolated_s{s}', np.concatenate([_rows(0, [(-1, -1, -1), (-2 * s, -2 * s, -2 * s), (-2 * s - 1, -2 * s - 1, -2 * s - 1)]),
                                              _rows(1, [(-2 * s - 1, -1, -2 * s), (-1, -2 * s, -2 * s - 1)])]), 2, sign='negative')
    rng = np.random.default_rng(7)
    half = rng.integers(0, 20, size=(700, 3))
    sym = np.concatenate([half, -half])
    add('symmetric_cloud', np.concatenate([_rows(0, sym), _rows(1, sym[::-1][:900])]), 2, sign='both', both_r=True)
    add('negative_cloud', np.concatenate([_rows(0, -1 - rng.integers(0, 24, size=(900, 3))), _rows(1, -1 - rng.integers(0, 9, size=(500, 3)))]),
        2, sign='negative', both_r=True)
    # -- range
    add('range_limit', _range_rows(), 3, nl=4, limit=True)
    for a in range(3):
        for sg in (-1, 1):
            for v, kind in ((LIMIT, 'graph'), (LIMIT + 1, 'refuse')):
                p = [3, -4, 5]
                p[a] = sg * v
                rows = np.concatenate([_rows(0, _cube(-2, 2)), _rows(1, [p]), _rows(1, _cube(-1, 1))])
                add(f'edge_{"xyz"[a]}_{"neg" if sg < 0 else "pos"}_{v}', rows, 2, nl=4 if kind == 'graph' else 2, kind=kind, axis=a, value=sg * v)
    bad = np.concatenate([_rows(0, _cube(-2, 2)), np.array([[-1, 1, 2, 3]], dtype=np.int32)])
    add('edge_batch_minus_one', bad, 1, kind='refuse', axis=-1, value=-1)
    # -- hash
    for name, step, pad in (('hash_chain_level0', 1, False), ('hash_chain_stride2', 2, True)):
        rows, absent, occupied = _hash_case(step, pad)
        add(name, rows, 1, kind='hash', absent=absent, table=1 if pad else 0, chain_home=61, chain_len=9, occupied=occupied)
    # -- block edges of the chain
    big = _rows(0, np.array([(x, y, z) for z in range(-32, 32) for y in range(-64, 64) for x in range(-64, 64)]))
    new = _rows(0, [(200 + 3 * i, -200 - 5 * i, 7 * i) for i in range(40)])
    tail = np.concatenate([big[:730], new[:20], big[5000:5274], big[100:500], new[15:40], big[1000:1051]])
    assert len(tail) == 1500
    add('chain_1m', np.concatenate([big, tail]), 1, nl=4, kind='chain_big')
    # -- map sizes (the set of stride 8 has n rows: the maps the plan derives tables for), strided-map input rows
    for n in (1, 2, 3, 5, 255, 256, 257, 1023, 1024, 1025, 2049):
        add(f'map_rows_{n}', _two_level(n, min(2 * n + 1, 8 * n), 4, n, B=1 if n < 5 else 2), 1 if n < 5 else 2, n_out=n)
    for n in (31, 32, 33):
        add(f'strided_map_in_{n}', _two_level(12, n, 4, 100 + n), 1, n_in=n)
    for nb in (64, 65):
        g = np.array([(x, y, z) for z in range(-20, 21) for y in range(-20, 21) for x in range(-20, 21)])[:nb * 1024 + 1]
        add(f'same_map_{nb}_blocks_plus_1', _rows(0, g * 8), 1, nl=1, kind='map_big', blocks=nb + 1)      # stride 8: `same1` of the plan
    # -- sparsity of offsets (stride 8, where the plan's convolution maps begin)
    s = 8
    add('offsets_centre_only', _rows(0, _cube(-4, 4) * 3 * s), 1, present=[13])
    add('offsets_line_x', np.concatenate([_rows(0, [(i * s, -s, 2 * s) for i in range(-9, 9)]), _rows(1, [(i * s, 0, 0) for i in range(-3, 4)])]), 2,
        present=[12, 13, 14])
    iso = _cube(-3, 3) * 4 * s
    add('offsets_single_pair_last_row', _rows(0, np.concatenate([iso, iso[:1] + [[s, 0, 0]]])), 1, present=[12, 13, 14], single=(14, 12))
    add('offsets_full_cube', _rows(0, _cube(-3, 3) * s - 1), 1, present=list(range(27)))
    return cs


# raw-points cases (the plan's collate): per scene the voxel rows; points = voxel + 0.5 at voxel size 1.0, feature = global row
@functools.lru_cache(maxsize=None)
def raw_cases():
    def tiny(b, seed):
        r = np.random.default_rng(1000 + seed)
        return _rows(b, r.integers(-3, 3, size=(int(r.integers(2, 9)), 3)))
    cs = {}
    for B in (32, 33, 65):
        cs[f'raw_{B}_scenes'] = (B, [tiny(b, b) for b in range(B)])
    cs['raw_empty_first_middle_last'] = (5, [_rows(0, []), tiny(1, 1), _rows(2, []), tiny(3, 3), _rows(4, [])])
    cs['raw_scene_of_one_point'] = (3, [tiny(0, 5), _rows(1, [(-1, -1, -1)]), tiny(2, 6)])
    return cs


def mask_patterns(n):
    """row masks for the argsort: all equal, ascending, descending, two values alternating"""
    i = np.arange(n, dtype=np.int64)
    return {'equal': np.full(n, 0x2000, np.int32), 'ascending': (i * 7).astype(np.int32), 'descending': ((n - i) * 5 + (1 << 26)).astype(np.int32),
            'alternating': np.where(i % 2 == 0, (1 << 27) - 1, 1).astype(np.int32)}


ARGSORT_SIZES = (1, 64, 4096, 4097)


# ---- the expected object graph of a case ----------------------------------------------------------------------------------------------
def case_of(name):
    if name in cases():
        return cases()[name]
    B, scenes = raw_cases()[name]
    return Case(np.concatenate(scenes), B, 2, {}, 'raw')


@functools.lru_cache(maxsize=None)
def expected(name):
    """every table of a case, as both coordinate phases must produce it: the chain of 3 + nl sets, the stem / pool / down / ds /
    same maps, the generated sets under the coarsest level with their maps and the union rows of the backbone levels inside them"""
    c = case_of(name)
    nl, S0 = c.nl, 3 + c.nl
    sets = chain(c.rows, S0)
    ex = dict(sets=sets, caps=[capacity(s.n_in) for s in sets], maps={}, gen=[], rows_per_scene=[np.bincount(s.coords[:, 0], minlength=c.B) for s in sets])
    co = [s.coords for s in sets]
    ex['maps']['stem'] = (0, 1, 3, kernel_map(co[0], co[1], 3, 1))
    ex['maps']['pool'] = (1, 2, 2, kernel_map(co[1], co[2], 2, 2))
    for li in range(1, nl + 1):
        p, m = 1 + li, 2 + li
        down = kernel_map(co[p], co[m], 3, 1 << p)
        ex['maps'][f'down{li}'] = (p, m, 3, down)
        ex['maps'][f'ds{li}'] = (p, m, 1, kernel_map(co[p], co[m], 1, 1 << p))
        assert np.array_equal(ex['maps'][f'ds{li}'][3][0], down[13])
        ex['maps'][f'same{li}'] = (m, m, 3, kernel_map(co[m], co[m], 3, 1 << m))
    par, stride = co[-1], 1 << (S0 - 1)
    for i in range(nl - 2, -1, -1):
        g = gen_coords(par, stride)
        stride //= 2
        ex['gen'].append(dict(coords=g, stride=stride, nbr=kernel_map(g, g, 3, stride), level=3 + i, rows=rows_in(g, co[3 + i])))
        assert np.array_equal(ex['gen'][-1]['rows'], child_rows(co[3 + i], par, stride))
        par = g
    return ex
