"""Case generator of the exact-integer normalisation tests (tests/test_norm_routes_cpu.py, tests/test_gpu_norm_exact.py) — the
normalisation twin of tests/conv_cases.py.

csrc/norm_route.h turns a training-mode normalisation call into one of about a dozen launch shapes; inside the kernels the block
geometry picks further branches (row lanes, a half-filled last wave, a short last row block, the unrolled loops of the finalise
kernels, the L1 bypass of the prologue reduction).  This module
  * reduces the answer of the route query (fc_bn_train_fwd_route / fc_bn_train_bwd_route, pure host functions) together with those
    facts — recomputed here from the route's blocks, rows per block, threads and channel window — to a hashable CLASS; the segment
    statistics (fc_col_stats, fc_seg_col_sums) compute their launch without a route, so it is restated from `row_blocks` /
    `stats_geometry` and classified the same way,
  * sweeps the query over a fixed grid (`sweep`) and keeps per class its smallest representative,
  * derives the GPU case list from the representatives (`row_counts`, `cases`): row counts at the row-block edges and at the
    four-rows-in-flight edges, each confirmed by the route query to stay in the class, times the crossed options,
  * makes the integer operands, the marker rows, the crafted segment tables and the float64 references.

Operands: integers in [-8, 8] stored as fp32 (x with a per-column offset so that no column mean is tiny).  MARKER rows — the first
and the last row of every row block of every kernel of the launch, row n - 1, the first row of every segment — carry +-64 in x (and
in gy): exactly the rows a wrong bound would lose or double.  Behind a table of sums (a producer's statistics epilogue) the unit a
kernel can lose is an ENTRY of the table: the test cuts the rows into as many uneven, non-empty ranges as the table has entries,
each starting on a marker row, and a table call exists from 2 x entries - 1 rows on — so no entry is all zero.
k_bn1_partial shifts every column by its row 0 (documented there: a sample of the column, |mean - shift| ~ sigma): a 64 in row 0 of
a column whose sigma is 7 is no such sample and costs the fp32 variance its last digits, and a marker row EQUAL to row 0 would add
nothing to the shifted sums — so row 0 carries 16 to 48 (`first_marker`), never what another marker row carries.
Forward: the shifted sums are integers below 2^24; where n is a power of two (column sums then rounded to a multiple of n / 16, so
that the square of the shifted mean is exact too) mean, var and running_mean equal float64 bit for bit.  Backward: the statistics are
inputs — integer means, var in {1, 0.25}, eps = 0, gamma in {1, 2, 0.5}, integer beta — so g', xhat and both column sums are
integers: the sums are exact for every n, gx / gres where n (every segment's count) is a power of two.
ReLU: act'(0) = 0, from y and from the recomputed pre-activation alike (norm.hip: y > 0, p > 0); the data has exact zeros there.
"""
import ctypes
import functools
import zlib
from collections import namedtuple

import numpy as np

from fcaf3d_amd import _lib as L

E = L.header_enums()
FWD, BWD, STATS = 'fwd', 'bwd', 'stats'
DIRECTIONS = (FWD, BWD, STATS)
INT64_MAX = (1 << 63) - 1
NONE, RELU, ELU = 0, 1, 2

# ---- norm_route.h restated (the CPU test holds these against the route query) -------------------------------------------------------------
MAXBLOCKS, BN1_MAXB, AP_MAXB, FIN_SL, MAXSEG = 1024, 64, 256, 64, 64


def cdiv(a, b):
    return -(-a // b)


def row_blocks(n, cap):
    """(blocks, rows per block) of n rows over at most `cap` blocks of at least 64 rows"""
    m = max(n, 1)
    g = min(cdiv(m, 64), cap)
    rpb = cdiv(m, g)
    return cdiv(m, rpb), rpb


def stats_geometry(C):
    """(threads, row lanes) of a row-blocked kernel over C channels"""
    c4n = C // 4
    nrl = min(max(256 // c4n, 1), 16)
    return nrl * c4n, nrl


# ---- the sweep's grid ---------------------------------------------------------------------------------------------------------------
MAX_ROWS, MAX_ELEMS = 16641, 4161 * 1024          # no launch of these tests is larger than 16 641 x 64 or 4 161 x 1024
C_LIST = (4, 8, 60, 64, 68, 128, 192, 256, 512, 1020, 1024)
NB_PART = (0, 1, 16, 17, 48, 49, 64, 65, 192, 193, 257)          # 0: no table
GROUPS = (1, 3, 64)
SMALL_ELEMS = (-1, 0, 1 << 20, INT64_MAX)
NSEG = (1, 2, 64)
# every row count up to 520, then the neighbours of every multiple of 64 (row_blocks, ap_window and the caps only move there)
N_LIST = tuple(sorted(set(range(1, 521)) | {v for k in range(64, MAX_ROWS + 64, 64) for v in (k - 1, k, k + 1) if v <= MAX_ROWS}
                      | {4161, MAX_ROWS}))

# entry: 'fwd' fc_bn_train_fwd (fc_bn_train_add_fwd with a sparse sum); 'train' / 'small' / 'seg': the backward forms; 'col_stats' /
# 'seg_col_sums'.  fin: the finalise kernel; nrl: row lanes 1, 2..15 ('mid'), 16; wave: the last wave full; last: the last row block
# 'full' / 'short' ('-': no row-blocked kernel); table: the finalise kernel's table against its slices and its unrolled loop —
# 'single' (at most one entry per slice), 'tail' (the tail loop only), 'unrolled' (both); past_l1: bn1_reduce_parts' switch
NormClass = namedtuple('NormClass', 'entry sums apply amax launches windowed fin nrl wave last table past_l1 grouped segs')
# a call of the sweep's grid (nb_part 0: no table; nseg: the backward SEG form and the segment statistics)
Rep = namedtuple('Rep', 'entry n C nb_part groups small_elems nseg')
# one GPU launch: rep's call at another row count with a set of options ('res', 'add', 'run', 'gy2', 'y', 'gres', 'relu', 'elu') and,
# for the segment forms, a crafted segment table and the stride of its ids
Case = namedtuple('Case', 'n opts table stride')

_FORM = {'train': E['FC_NFORM_TRAIN'], 'small': E['FC_NFORM_SMALL'], 'seg': E['FC_NFORM_SEG']}
_SUMS_F = {E[k]: k[len('FC_NSTATS_'):].lower() for k in E if k.startswith('FC_NSTATS_')}
_SUMS_B = {E[k]: k[len('FC_NRED_'):].lower() for k in E if k.startswith('FC_NRED_')}
_APPLY_F = {E[k]: k[len('FC_NAPPLY_'):].lower() for k in E if k.startswith('FC_NAPPLY_')}
_APPLY_B = {E[k]: k[len('FC_NBAPPLY_'):].lower() for k in E if k.startswith('FC_NBAPPLY_')}
_AMAX = {E[k]: k[len('FC_NAMAX_'):].lower() for k in E if k.startswith('FC_NAMAX_')}
_I = {k[len('FC_NROUTE_'):].lower(): v for k, v in E.items() if k.startswith('FC_NROUTE_')}


def class_id(c):
    """the class as a test id"""
    return (f'{c.entry}-{c.sums}-{c.apply}-amax_{c.amax}-{c.launches}l-{"win" if c.windowed else "all"}-{c.fin}-nrl{c.nrl}-'
            f'{"anywave" if c.wave is None else "wave" if c.wave else "halfwave"}-{c.last}-{c.table}-{"l1byp" if c.past_l1 else "l1" if c.past_l1 is not None else "nol1"}'
            f'-{"grouped" if c.grouped else "g1"}-{"segs" if c.segs else "oneseg"}')


def _bucket(total, slices, unrolled_from):
    return 'single' if total <= slices else 'tail' if total <= unrolled_from else 'unrolled'


def _nrl_bucket(nrl):
    return '1' if nrl == 1 else '16' if nrl == 16 else 'mid'


def _blocked(n, blocks, rpb, threads, C, table='none'):
    """(nrl bucket, last wave full, last row block) of a row-blocked kernel.  Behind a table too long for one entry per slice (1 025 rows
    and more, 4 097 for most) the geometry is not told apart ('any', None): the finalise kernel is a launch of its own whose code does
    not read it, and every geometry branch is reached at short tables — so the long-table classes are represented at 4 channels"""
    last = 'full' if blocks * rpb == n else 'short'
    if table in ('tail', 'unrolled'):
        return 'any', None, last
    return _nrl_bucket(threads // (C // 4)), threads % 64 == 0, last


def layouts(rep, n, o=None):
    """the row blockings [(blocks, rows per block, row lanes)] of every row-blocked kernel of rep's call at n rows: the partial-sum
    kernel and the prologue-reducing apply kernel (one entry where they share a blocking)"""
    if rep.entry in ('col_stats', 'seg_col_sums'):
        return [row_blocks(n, MAXBLOCKS) + (stats_geometry(rep.C)[1],)]
    o = _query(rep, n) if o is None else o
    assert o is not None, (rep, n)
    out = []
    if o[_I['nb']]:
        out.append((o[_I['nb']], o[_I['rpb']], o[_I['threads']] // (o[_I['cg']] // 4)))
    has_red = (rep.entry == 'fwd' and not rep.nb_part) or (rep.entry != 'fwd' and not (rep.entry == 'train' and rep.nb_part))
    if has_red:
        small = (rep.entry == 'small' or (rep.entry in ('fwd', 'train') and n * rep.C <= rep.small_elems))
        b = row_blocks(n, BN1_MAXB if small else MAXBLOCKS) + (stats_geometry(rep.C)[1],)
        if b not in out:
            out.append(b)
    return out


# ---- the route query ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fns():
    l = L.lib()
    return l.fc_bn_train_fwd_route, l.fc_bn_train_bwd_route, (ctypes.c_int * 16)()


def _query(rep, n):
    """the raw out[] of the route query for rep's call at n rows, or None where the entry point would answer FC_EINVAL"""
    f, b, out = _fns()
    if rep.entry == 'fwd':
        rc = f(n, rep.C, 1 if rep.nb_part else 0, rep.nb_part, rep.groups, rep.small_elems, out)
    else:
        rc = b(n, rep.C, rep.nseg, 1 if rep.nb_part else 0, rep.nb_part, rep.small_elems, _FORM[rep.entry], out)
    return out if rc == 0 else None


def _reduce(rep, n, o):
    C = rep.C
    sums, apply, np_, nb, rpb, cg, thr = (o[_I[k]] for k in ('sums', 'apply', 'np', 'nb', 'rpb', 'cg', 'threads'))
    launches, windowed = o[_I['launches']], cg < C
    red_thr = stats_geometry(C)[0]
    if rep.entry == 'fwd':
        s, a = _SUMS_F[sums], _APPLY_F[apply]
        fin = {'partial': 'bn_finalize', 'table': 'bn2_finalize'}.get(s, 'none')
        table = _bucket(np_, 16, 48) if s == 'partial' else _bucket(np_ * rep.groups, FIN_SL, 3 * FIN_SL) if s == 'table' else 'none'
        if a in ('bn1', 'bn2'):
            geo = _blocked(n, nb, rpb, thr, cg)
        elif s == 'partial':
            geo = _blocked(n, *row_blocks(n, MAXBLOCKS), red_thr, C, table)
        else:
            geo = ('-', True, '-')
        past = (np_ * C * 8 <= 32768) if a == 'bn1' else None
        return NormClass('fwd', s, a, _AMAX[o[_I['amax']]], launches, windowed, fin, *geo, table, past, bool(rep.nb_part) and rep.groups > 1, False)
    s, a = _SUMS_B[sums], _APPLY_B[apply]
    if a == 'prologue':
        fin, table, geo, past = 'none', 'none', _blocked(n, nb, rpb, thr, cg), np_ * C * 8 <= 32768
    else:
        fin, table, past = 'stats_final', _bucket(np_, FIN_SL, 3 * FIN_SL), None
        geo = _blocked(n, *row_blocks(n, MAXBLOCKS), red_thr, C, table) if s == 'partial' else ('-', True, '-')
    return NormClass(rep.entry, s, a, _AMAX[o[_I['amax']]], launches, windowed, fin, *geo, table, past, False, rep.nseg > 1)


def route_class(rep, n=None):
    """the class of rep's call (at n rows), or None where the entry point answers FC_EINVAL or the call has no rows"""
    n = rep.n if n is None else n
    if rep.entry in ('col_stats', 'seg_col_sums'):
        if n < 1 or rep.C < 4 or rep.C % 4 or rep.C > 1024:
            return None
        nb, rpb = row_blocks(n, MAXBLOCKS)
        fin = 'seg_meanvar_final' if rep.entry == 'col_stats' else 'stats_final'
        table = _bucket(nb, FIN_SL, 3 * FIN_SL if rep.entry == 'seg_col_sums' else 1 << 30)
        return NormClass(rep.entry, 'partial', 'none', 'none', 2, False, fin, *_blocked(n, nb, rpb, stats_geometry(rep.C)[0], rep.C, table), table,
                         None, False, rep.nseg > 1)
    if n < 1 or n < 2 * table_entries(rep) - 1:
        return None
    o = _query(rep, n)
    return None if o is None else _reduce(rep, n, o)


def table_entries(rep):
    """entries of the table of sums a call is handed (0: none).  The cases give every entry at least one row and two on average — an
    entry without rows is all zero, and a kernel that loses it goes unseen — so a table call exists from 2 x entries - 1 rows on (one entry: from one row)"""
    return rep.nb_part * (rep.groups if rep.entry == 'fwd' else 1)


def route_fields(rep, n=None):
    """(status, {field: value}) of the route query proper (L.route) for rep's call"""
    n = rep.n if n is None else n
    if rep.entry == 'fwd':
        return L.route('fc_bn_train_fwd_route', n, rep.C, 1 if rep.nb_part else 0, rep.nb_part, rep.groups, rep.small_elems)
    return L.route('fc_bn_train_bwd_route', n, rep.C, rep.nseg, 1 if rep.nb_part else 0, rep.nb_part, rep.small_elems, _FORM[rep.entry])


def direction_of(entry):
    return FWD if entry == 'fwd' else STATS if entry in ('col_stats', 'seg_col_sums') else BWD


def _calls(C):
    """the sweep's calls over C channels, in list order, without the row count"""
    for small in SMALL_ELEMS:
        yield Rep('fwd', 0, C, 0, 1, small, 1)
    for nbp in NB_PART[1:]:
        for G in GROUPS:
            yield Rep('fwd', 0, C, nbp, G, 1 << 20, 1)
    for small in SMALL_ELEMS:
        yield Rep('train', 0, C, 0, 1, small, 1)
    for nbp in NB_PART[1:]:
        yield Rep('train', 0, C, nbp, 1, 1 << 20, 1)
    yield Rep('small', 0, C, 0, 1, 0, 1)
    for nseg in NSEG:
        yield Rep('seg', 0, C, 0, 1, 0, nseg)
    for entry in ('col_stats', 'seg_col_sums'):
        for nseg in NSEG:
            yield Rep(entry, 0, C, 0, 1, 0, nseg)


@functools.lru_cache(maxsize=None)
def sweep():
    """-> {FWD: {class: Rep}, BWD: ..., STATS: ...}: every class the grid reaches with its representative — the smallest row count, then
    the first channel count and call in list order"""
    best = {d: {} for d in DIRECTIONS}
    for n in N_LIST:
        for C in C_LIST:
            if n * C > MAX_ELEMS:
                continue
            for call in _calls(C):
                cls = route_class(call, n)
                d = best[direction_of(call.entry)]
                if cls is not None and cls not in d:
                    d[cls] = call._replace(n=n)
    return {d: dict(sorted(best[d].items(), key=lambda kv: class_id(kv[0]))) for d in DIRECTIONS}


# ---- row counts and cases of a class --------------------------------------------------------------------------------------------------
SEARCH = 700          # how far from a target (and from the representative) a row count of the class is looked for


def _n_max(rep):
    return min(MAX_ROWS, MAX_ELEMS // rep.C)


def row_counts(cls, rep):
    """the representative's n, then the row counts of the class nearest to rpb - 1, rpb, rpb + 1, 2 rpb + 1 (rpb: rows per block of
    the representative's row-blocked kernel) and to 1, then the first row counts of the class from the representative's on whose LAST
    row block holds r rows with r mod (4 nrl) in {0, 1, nrl, nrl + 1, 4 nrl - 1}: the four-rows-in-flight loop ends on a full
    batch, one row, one full lane set, one more, all but one.  A class without a row-blocked kernel keeps n, n + 1 and 2 n + 1."""
    assert route_class(rep) == cls, (cls, rep)
    hi = _n_max(rep)
    inside = functools.lru_cache(maxsize=None)(lambda n: 1 <= n <= hi and route_class(rep, n) == cls)
    lay = layouts(rep, rep.n)
    targets = [1, rep.n + 1, 2 * rep.n + 1]
    for _, rpb, _ in lay:
        targets += [rpb - 1, rpb, rpb + 1, 2 * rpb + 1]
    out = [rep.n]
    for t in targets:
        t = min(max(t, 1), hi)
        for d in range(SEARCH):
            hit = next((v for v in (t - d, t + d) if inside(v)), None)
            if hit is not None:
                if hit not in out:
                    out.append(hit)
                break
    want = {}
    for n in range(rep.n, min(hi, rep.n + SEARCH) + 1):
        if not inside(n):
            continue
        for nb, rpb, nrl in layouts(rep, n):
            r = (n - (nb - 1) * rpb) % (4 * nrl)
            for k, v in (('full', 0), ('one', 1), ('lanes', nrl % (4 * nrl)), ('lanes1', (nrl + 1) % (4 * nrl)), ('short', 4 * nrl - 1)):
                if r == v:
                    want.setdefault((k, nrl), n)
    for n in want.values():
        if n not in out:
            out.append(n)
    return out


FWD_OPTS = (('run',), ('res', 'add', 'relu'), ('add', 'run', 'relu'), ('res', 'run'), ('elu',), ('res', 'add', 'run', 'elu'))
BWD_OPTS = (('gres',), ('gy2', 'y', 'gres', 'relu'), ('gy2', 'relu'), ('y', 'relu'), ('elu',), ('gy2', 'y', 'gres', 'elu'))
SEG_TABLES = ('contig', 'straddle', 'unsorted')
BIG_ELEMS = 1 << 19          # a class whose representative is larger runs two option sets there and two further row counts


def cases(cls, rep):
    """the GPU launches of a class: at the representative's row count every option set (so every apply kernel sees a residual, the
    sparse sum, a second gradient, y given and absent, running buffers present and absent, ReLU, ELU and no activation on every class,
    windowed or not), at the other row counts of `row_counts` the option sets in turn (BIG_ELEMS: fewer); the segment forms also cycle through the
    crafted tables and the two strides"""
    seg = cls.segs
    out, k = [], 0

    def add(n, opts):
        nonlocal k
        out.append(Case(n, tuple(opts), SEG_TABLES[k % 3] if seg else 'one', (1, 4)[k % 2] if seg else 0))
        k += 1
    d = direction_of(rep.entry)
    if d == STATS:
        for n in row_counts(cls, rep):
            add(n, ())
        if seg:
            add(rep.n, ())
            add(rep.n, ())          # (the representative's row count on all three tables)
        return out
    opt_list = FWD_OPTS if d == FWD else BWD_OPTS
    if rep.entry in ('seg', 'small'):          # fc_norm_act_bwd / fc_bn_act_train_bwd take no second gradient
        opt_list = tuple(tuple(o for o in opts if o != 'gy2') for opts in opt_list)
    big = rep.n * rep.C > BIG_ELEMS
    for opts in (opt_list[1], opt_list[0]) if big else opt_list:
        add(rep.n, opts)
    for i, n in enumerate(row_counts(cls, rep)[1:3 if big else None]):
        add(n, opt_list[(i + 2) % 4])
    return out


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode())


def is_pow2(n):
    return n >= 1 and n & (n - 1) == 0


def marker_rows(n, lay, seg=None, edges=None):
    """sorted rows that carry a marker: the first and last row of every block of every blocking of `lay`, row n - 1, the first row of
    every segment (the first rows of the blocks are also the rows a padding lane re-reads)"""
    rows = {0, n - 1}
    for nb, rpb, _ in lay:
        for b in range(nb):
            rows.add(b * rpb)
            rows.add(min((b + 1) * rpb, n) - 1)
    if edges is not None:
        rows.update(int(e) for e in edges[:-1])          # the first row of every row range of a table: no entry is all zero
    if seg is not None:
        ids = np.asarray(seg)
        for s in np.unique(ids):
            rows.add(int(np.nonzero(ids == s)[0][0]))
    return sorted(rows)


@functools.lru_cache(maxsize=32)
def int_matrix(shape, seed, amp=8, zero_frac=1.0 / 3.0):
    """integers in [-amp, amp] as float64, `zero_frac` of them zero (read-only: the option sets of a row count share it)"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-amp, amp + 1, shape).astype(np.float64)
    v[rng.random(shape) < zero_frac] = 0.0
    v.setflags(write=False)
    return v


def _put_markers(a, rows, first, flip):
    """+-64 into the marker rows (row 0: `first`), the sign alternating along the rows (in pairs where `flip`) and the channels"""
    C = a.shape[1]
    col = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    for k, r in enumerate(rows):
        sign = -1.0 if ((k // 2 if flip else k) % 2) else 1.0
        a[r] = sign * col * (first if r == 0 else 64.0)


def _round_column_sums(x, frozen, q):
    """x's column sums to multiples of q by +-1 on rows outside `frozen`, every entry kept in [-8, 8]"""
    free = np.ones(len(x), bool)
    free[frozen] = False
    s = x.sum(0)
    t = np.rint(s / q) * q - s
    for c in np.nonzero(t)[0]:
        sg, k = (1.0 if t[c] > 0 else -1.0), int(abs(t[c]))
        ok = np.nonzero(free & (x[:, c] * sg < 8))[0][:k]
        assert len(ok) == k
        x[ok, c] += sg


def first_marker(n):
    """|x[0]| of the forward input.  k_bn1_partial shifts every column by its row 0: at a power-of-two n (exact comparison) the sum of
    the shifted squares, about n (|x[0]|^2 + 50), has to stay below 2^24; elsewhere (1e-5 of the tensor's scale) 32 keeps the fp32
    variance's cancellation error, about 2.4e-7 |x[0]|^2, under a fifth of the bound and the row still 100 bounds heavy at 16 641 rows"""
    return (48.0 if n <= 2048 else 32.0 if n <= 8192 else 16.0) if is_pow2(n) else 32.0


def fwd_x(n, C, rows, seed):
    return _fwd_x(n, C, tuple(rows), seed)


@functools.lru_cache(maxsize=16)
def _fwd_x(n, C, rows, seed):
    """the forward input: integers in [-8, 8], column c offset by c mod 3 - 1, markers (module docstring), at a power-of-two n the
    column sums multiples of n / 16"""
    x = np.clip(int_matrix((n, C), seed) + (np.arange(C) % 3 - 1.0), -8, 8)
    _put_markers(x, rows, first_marker(n), False)
    if is_pow2(n) and n >= 32:
        _round_column_sums(x, list(rows), n // 16)
    x.setflags(write=False)
    return x


def affine(C):
    """gamma in {1, 2, 0.5}, integer beta in [-2, 2]"""
    return np.array([1.0, 2.0, 0.5])[np.arange(C) % 3], (np.arange(C) % 5 - 2.0)[::-1].copy()


def given_stats(nseg, C):
    """the statistics a backward call is given: integer means in [-2, 2], var in {1, 0.25} (eps = 0: 1 / sqrt is 1 or 2)"""
    s, c = np.arange(nseg)[:, None], np.arange(C)[None, :]
    return ((c + s) % 5 - 2.0), np.where((c + s) % 2 == 0, 1.0, 0.25)


def add_rows(n):
    """(rows of add_src, add_inv (n,) int32): two thirds of the rows take a row of add_src, row 0 — block 0's stand-in row — among them"""
    m = n // 2 + 1
    r = np.arange(n)
    return m, np.where(r % 3 != 1, (r * 7) % m, -1).astype(np.int32)


def table_edges(n, t, seed):
    """(t + 1,) row edges of t uneven, NON-EMPTY row ranges over n >= t rows: one row each, the other n - t rows dealt out at random"""
    assert n >= t >= 1
    rng = np.random.default_rng(seed)
    w = rng.random(t) ** 2 + 1e-3
    size = 1 + rng.multinomial(n - t, w / w.sum())
    return np.concatenate([[0], np.cumsum(size)]).astype(np.int64)


def part_table(a, b, edges, nb_part, groups):
    """[nb_part][2][groups * C]: the column sums of a and of b (n, C) over the nb_part * groups row ranges of `edges`, range t = blk * groups
    + g in block blk, group g — what a producer's statistics epilogue leaves (float64: the entries are integers below 2^24)"""
    C = a.shape[1]
    c1 = np.concatenate([np.zeros((1, C)), np.cumsum(a, 0)])
    c2 = np.concatenate([np.zeros((1, C)), np.cumsum(b, 0)])
    s1 = (c1[edges[1:]] - c1[edges[:-1]]).reshape(nb_part, groups * C)
    s2 = (c2[edges[1:]] - c2[edges[:-1]]).reshape(nb_part, groups * C)
    return np.stack([s1, s2], 1)


# ---- crafted segment tables -------------------------------------------------------------------------------------------------------------
def seg_table(kind, n, nseg, rpb):
    """(n,) int32 ids in [0, nseg).  nseg = 1: zeros.  Else
    'contig'   sorted ids, uneven counts; from four segments on segment nseg // 2 and segment nseg - 1 are empty,
    'straddle' the first block of rpb rows holds three segments (two where nseg = 2) in sorted runs, every later block lies in one segment,
    'pow2'     see pow2_rows,
    'unsorted' 'contig' with the ids of its first block of rpb rows shuffled (a block whose min / max range holds segments it has no row of
               at every position)"""
    if nseg == 1:
        return np.zeros(n, np.int32)
    if kind == 'pow2':
        assert n == pow2_rows(nseg)
        return np.repeat(np.arange(nseg, dtype=np.int32), _pow2_counts(nseg))
    rng = np.random.default_rng(_seed('seg', n, nseg, rpb))
    if kind == 'straddle':
        k, head, nblk = min(3, nseg), min(rpb, n), cdiv(n, rpb)
        r = np.arange(n)
        b = r // rpb
        later = np.minimum(k - 1 + (b - 1) * (nseg - k + 1) // max(nblk - 1, 1), nseg - 1)
        return np.where(b == 0, np.minimum(r * k // head, k - 1), later).astype(np.int32)
    live = [s for s in range(nseg) if nseg < 4 or s not in (nseg // 2, nseg - 1)]
    w = rng.random(len(live)) + 0.2
    cnt = np.floor(w / w.sum() * n).astype(np.int64)
    cnt[0] += n - cnt.sum()
    ids = np.repeat(np.array(live, np.int32), cnt)
    if kind == 'unsorted':
        head = min(rpb, n)
        ids[:head] = rng.permutation(ids[:head])
    elif kind != 'contig':
        raise KeyError(kind)
    return ids


def _pow2_counts(nseg):
    c = np.array([(32, 64, 16, 128)[s % 4] for s in range(nseg)])
    if nseg >= 4:
        c[[nseg // 2, nseg - 1]] = 0
    return c


def pow2_rows(nseg):
    """the row count of the 'pow2' table: sorted ids, every segment's count a power of two (32, 64, 16, 128 in turn) or, from four
    segments on, zero in segment nseg // 2 and segment nseg - 1 — the table on which gx is exact"""
    return int(_pow2_counts(nseg).sum())


def strided(ids, stride):
    """the ids as the entry points read them: column 0 of an (n, stride) int32 matrix whose other columns hold junk"""
    if stride == 1:
        return np.ascontiguousarray(ids, np.int32)
    m = np.full((len(ids), stride), 12345, np.int32)
    m[:, 0] = ids
    return m


# ---- references (float64 numpy) ---------------------------------------------------------------------------------------------------------
EXACT = float(2 ** 24)


def act_fwd(p, act):
    return np.maximum(p, 0.0) if act == RELU else np.where(p > 0, p, np.expm1(np.minimum(p, 0.0))) if act == ELU else p


def act_grad(p, act):
    """from the pre-activation (equally from y): ReLU 0 at 0"""
    return (p > 0).astype(np.float64) if act == RELU else np.where(p > 0, 1.0, np.exp(np.minimum(p, 0.0))) if act == ELU else np.ones_like(p)


def ref_fwd_stats(x, w=None, momentum=0.25, rmean=None, rvar=None):
    """mean, biased var of n rows in float64 — w (n,): how often each row enters the sums (the sensitivity test drops and doubles
    rows; the divisor stays n, as it does in a kernel that loses a row) — and the running buffers after one update"""
    n = len(x)
    w = np.ones(n) if w is None else w
    s1, s2 = (w[:, None] * x).sum(0), (w[:, None] * x * x).sum(0)
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, 0.0)
    out = {'mean': mean, 'var': var}
    if rmean is not None:
        out['rmean'] = (1 - momentum) * rmean + momentum * mean
        out['rvar'] = (1 - momentum) * rvar + momentum * var * (n / max(n - 1.0, 1.0))
    return out


def ref_fwd_y(x, mean, var, eps, gamma, beta, act, res=None, add_inv=None, add_src=None):
    y = (x - mean) / np.sqrt(var + eps) * gamma + beta
    if res is not None:
        y = y + res
    y = act_fwd(y, act)
    if add_inv is not None:
        y = y + np.where(add_inv[:, None] >= 0, add_src[np.maximum(add_inv, 0)], 0.0)
    return y


def ref_bwd(x, g, mean, var, gamma, beta, act, seg, nseg, cnt, res=None, w=None):
    """g (n, C): the incoming gradient (gy + gy2, or the pooled gradient scattered).  -> g' (gres), sums (nseg, 2, C), gx — with eps = 0
    and the given per-segment statistics; w: see ref_fwd_stats (the sums lose / double a row, every row is still applied to)"""
    n = len(x)
    w = np.ones(n) if w is None else w
    is_ = 1.0 / np.sqrt(var)[seg]
    xh = (x - mean[seg]) * is_
    pre = xh * gamma + beta + (0.0 if res is None else res)
    gp = g * act_grad(pre, act)
    sums = np.zeros((nseg, 2, x.shape[1]))
    np.add.at(sums[:, 0], seg, w[:, None] * gp)
    np.add.at(sums[:, 1], seg, w[:, None] * gp * xh)
    cn = np.asarray(cnt, np.float64)[seg][:, None]
    gx = gamma * is_ * (gp - sums[seg, 0] / cn - xh * sums[seg, 1] / cn)
    return {'gres': gp, 'sums': sums, 'gx': gx, 'pre': pre, 'xh': xh}


def ref_seg_stats(x, seg, nseg):
    """per-segment mean, biased var, count (an empty segment: zeros) and the column sums"""
    C = x.shape[1]
    s1, s2, cnt = np.zeros((nseg, C)), np.zeros((nseg, C)), np.zeros(nseg)
    np.add.at(s1, seg, x)
    np.add.at(s2, seg, x * x)
    np.add.at(cnt, seg, 1.0)
    d = np.maximum(cnt, 1.0)[:, None]
    mean = np.where(cnt[:, None] > 0, s1 / d, 0.0)
    var = np.where(cnt[:, None] > 0, np.maximum(s2 / d - mean * mean, 0.0), 0.0)
    return {'mean': mean, 'var': var, 'cnt': cnt, 'sums': s1}


# ---- one case's inputs and expected outputs ------------------------------------------------------------------------------------------------
REL_STATS, REL_SCALE = 1e-5, 1e-4          # the project's bounds: batch statistics (tests/test_gpu_ops.py), everything else


def case_seg(rep, case):
    """(ids (n,), rows per block of the segment kernels) of a case"""
    rpb = row_blocks(case.n, MAXBLOCKS)[1]
    return seg_table(case.table, case.n, rep.nseg, rpb), rpb


@functools.lru_cache(maxsize=8)
def build(rep, case):
    """-> (inputs, expected, bounds, markers): float64 / int32 numpy arrays by name; bounds[name] is 0 (torch.equal) or the fraction of
    the expected tensor's max-abs the output may be off by"""
    n, C = case.n, rep.C
    d = direction_of(rep.entry)
    o = set(case.opts)
    act = RELU if 'relu' in o else ELU if 'elu' in o else NONE
    key = (rep.entry, n, C, rep.nb_part, rep.groups)
    gamma, beta = affine(C)
    seg = case_seg(rep, case)[0] if (d == STATS or rep.entry == 'seg') else np.zeros(n, np.int32)
    edges = table_edges(n, table_entries(rep), _seed('edges', key)) if table_entries(rep) else None
    rows = marker_rows(n, layouts(rep, n), seg if rep.nseg > 1 else None, edges)
    inp = {'gamma': gamma, 'beta': beta, 'seg': seg, 'act': act}
    exp, bnd = {}, {}
    if d == STATS:
        x = fwd_x(n, C, rows, _seed('x', key))
        inp['x'] = x
        r = ref_seg_stats(x, seg, rep.nseg)
        assert np.abs(x).sum(0).max() < EXACT and (x * x).sum(0).max() < EXACT
        if rep.entry == 'seg_col_sums':
            exp['sums'], bnd['sums'] = r['sums'], 0
        else:
            exp.update(mean=r['mean'], var=r['var'], cnt=r['cnt'])
            exact = all(c == 0 or is_pow2(int(c)) for c in r['cnt'])
            bnd.update(mean=0 if exact else REL_STATS, var=0 if exact else REL_STATS, cnt=0)
        return inp, exp, bnd, rows
    if d == FWD:
        x = fwd_x(n, C, rows, _seed('x', key))
        inp['x'] = x
        sh = x - x[0]
        assert np.abs(sh).max() <= 128
        if rep.nb_part:          # (the table routes add the entries in fp64: only the entries have to be exact)
            inp['part'] = part_table(x, x * x, edges, rep.nb_part, rep.groups)
            assert np.abs(inp['part']).max() < EXACT and inp['part'][:, 1].reshape(-1, C).any(1).all()
        else:
            assert not is_pow2(n) or max(np.abs(sh).sum(0).max(), (sh * sh).sum(0).max()) < EXACT
        if 'run' in o:
            inp['rmean'], inp['rvar'] = np.arange(C) % 7 - 3.0, np.arange(C) % 4 + 1.0
        if 'res' in o:
            inp['res'] = int_matrix((n, C), _seed('res', key))
        if 'add' in o:
            m, inp['add_inv'] = add_rows(n)
            inp['add_src'] = int_matrix((m, C), _seed('add', key))
        st = ref_fwd_stats(x, None, 0.25, inp.get('rmean'), inp.get('rvar'))
        exact = is_pow2(n)
        exp.update(mean=st['mean'], var=st['var'], cnt=np.array([float(n)]))
        bnd.update(mean=0 if exact else REL_STATS, var=0 if exact else REL_STATS, cnt=0)
        if 'run' in o:
            exp.update(rmean=st['rmean'], rvar=st['rvar'])
            bnd.update(rmean=0 if exact else REL_STATS, rvar=REL_STATS)
        # y from the fp32 statistics the kernel is held to (a structural error in them is the statistics' finding, not y's)
        m32, v32 = st['mean'].astype(np.float32).astype(np.float64), st['var'].astype(np.float32).astype(np.float64)
        exp['y'], bnd['y'] = ref_fwd_y(x, m32, v32, EPS_FWD, gamma, beta, act, inp.get('res'), inp.get('add_inv'), inp.get('add_src')), REL_SCALE
        return inp, exp, bnd, rows
    # backward
    x = int_matrix((n, C), _seed('bx', key)).copy()
    gy = int_matrix((n, C), _seed('gy', key)).copy()
    _put_markers(x, rows, 64.0, False)
    _put_markers(gy, rows, 64.0, True)
    mean, var = given_stats(rep.nseg, C)
    cnt = np.bincount(seg, minlength=rep.nseg).astype(np.float64)
    inp.update(x=x, gy=gy, mean=mean, var=var, cnt=cnt)
    g = gy
    if 'gy2' in o:
        inp['gy2'] = int_matrix((n, C), _seed('gy2', key))
        g = gy + inp['gy2']
    res = int_matrix((n, C), _seed('res', key)) if 'y' in o else None          # y given: the forward had a residual
    r = ref_bwd(x, g, mean, var, gamma, beta, act, seg, rep.nseg, cnt, res)
    inp.update(ref_gres=r['gres'], ref_xh=r['xh'], ref_pre=r['pre'], ref_res=res)          # (for the CPU test's premise; no launch reads them)
    if 'y' in o:
        inp['y'] = act_fwd(r['pre'], act)
    if rep.entry == 'train' and rep.nb_part:          # gy's producer's table: column sums of g' and g' xhat over uneven row ranges
        inp['part'] = part_table(r['gres'], r['gres'] * r['xh'], edges, rep.nb_part, 1)
    int_act = act != ELU
    if int_act:
        assert np.abs(r['gres']).sum(0).max() < EXACT and np.abs(r['gres'] * r['xh']).sum(0).max() < EXACT
    exact_gx = int_act and all(c == 0 or is_pow2(int(c)) for c in cnt) and gx_premise(r, seg, cnt)
    exp.update(sums=r['sums'], gx=r['gx'])
    bnd.update(sums=0 if int_act else REL_SCALE, gx=0 if exact_gx else REL_SCALE)
    if 'gres' in o:
        exp['gres'], bnd['gres'] = r['gres'], 0 if int_act else REL_SCALE
    return inp, exp, bnd, rows


EPS_FWD = 1e-5


def gx_premise(r, seg, cnt):
    """every term of gx = gamma is (g' - S1 / n - xhat S2 / n) is a multiple of 1 / n below 2^24 / n, and xhat S2 itself below 2^24: fp32
    evaluates the bracket without rounding in any order (n a power of two per segment)"""
    cn = np.asarray(cnt, np.float64)[seg][:, None]
    s1, s2 = np.abs(r['sums'][seg, 0]), np.abs(r['sums'][seg, 1])
    xs = np.abs(r['xh']) * s2
    return bool(xs.max() < EXACT and ((np.abs(r['gres']) * cn + s1 + xs).max() < EXACT))


def differs(got, want, bound, factor=1.0):
    """does `got` miss `want` by more than factor x its bound (bound 0: is it unequal after the cast to fp32)"""
    if bound == 0:
        return not np.array_equal(got.astype(np.float32), want.astype(np.float32))
    return bool(np.abs(got - want).max() > factor * bound * np.abs(want).max())


# ---- the fused max-pool forms -----------------------------------------------------------------------------------------------------------
POOL_SIZES = (8, 3, 1, 5, 8, 2, 0)


def pool_table(seg, seed):
    """a k2s2-like table over the input rows of a segment table: -> (nbr (8, n_out) int32, parent (n_in,) int32).  Consecutive input
    rows of one segment are the children of one pooled row, 8, 3, 1, 5, 8, 2 of them in turn (fewer where the segment ends), in
    shuffled offset slots; every seventh pooled row has no child"""
    n_in, rng = len(seg), np.random.default_rng(seed)
    groups, r, k = [], 0, 0
    while r < n_in:
        sz = POOL_SIZES[k % len(POOL_SIZES)]
        k += 1
        e = r
        while e < n_in and e - r < sz and seg[e] == seg[r]:
            e += 1
        groups.append((r, e))
        r = e
    nbr = np.full((8, len(groups)), -1, np.int32)
    parent = np.full(n_in, -1, np.int32)
    for o, (a, b) in enumerate(groups):
        nbr[rng.permutation(8)[:b - a], o] = np.arange(a, b)
        parent[a:b] = o
    return nbr, parent


def ref_pool(y, nbr):
    """(out (n_out, C), argrow (n_out, C) int32): the maximum over the present children, the first in offset order at a tie; 0 / -1 for a
    pooled row without children"""
    valid = nbr >= 0
    v = np.where(valid[:, :, None], y[np.maximum(nbr, 0)], -np.inf)
    k = v.argmax(0)
    some = valid.any(0)[:, None]
    arg = nbr[k, np.arange(nbr.shape[1])[:, None]]
    return np.where(some, v.max(0), 0.0), np.where(some, arg, -1).astype(np.int32)


def pooled_gradient(g_pool, argrow, parent):
    """what fc_maxpool_bwd scatters into a zeroed matrix: row r takes g_pool[parent[r]][c] where it won channel c"""
    r = np.arange(len(parent))[:, None]
    return np.where(argrow[parent] == r, g_pool[parent], 0.0)
