"""Case generator of the exact-integer convolution tests (tests/test_conv_routes_cpu.py, tests/test_gpu_conv_exact.py).

csrc/conv_route.h turns a convolution call into one of about a dozen kernel families times tile, offset split, weight source,
arithmetic, addressing, statistics epilogue and grid shape.  This module
  * reduces the answer of the route query (fc_conv_fwd_route / fc_conv_wgrad_route, pure host functions) to a hashable CLASS,
  * sweeps the query over a fixed grid (`sweep`: the one place where the lists live) and keeps, per class, its representative —
    the smallest row count, then the first shape in list order, that reaches the class,
  * derives the GPU case list from the representatives (`row_counts`, `cases`): row counts at the tile and row-range edges, each
    confirmed by the route query to stay in the class, times crafted neighbour tables,
  * makes the tables, the integer operands and the exact float64 references,
  * makes, for the classes with a statistics epilogue, the inputs, the option combinations and the float64 reference of that
    epilogue's backward form, with the one-token mutations of the reference the CPU test holds the cases against (last section).

Operands are small integers stored as fp32 (x, gout in [-8, 8], w in [-4, 4], a third of them zero): every arithmetic mode of the
library is exact on them (fp32: integers below 2^24; six-product / bf16-fast: the first bf16 piece holds the value; h3: the
power-of-two scale keeps fp16(s x) exact and the low piece zero), so results are compared with torch.equal.

Classes.  Forward: (family, bm, bn, S > 1, wsrc, mode, buf, epi, linear grid); weight gradient: (family, bm, bn, ko, mode, S > 1,
wbuf, table, bkr) — bkr (rows per chunk) is appended because FC_CONV_WGRAD_DEEP selects another template on it alone.  The untiled
families (stem, FMA) carry bm = bn = 0 and S > 1 = False: the route fills those fields but the kernels do not read them; the stem
also reads its fp32 kernel under every flag, so its wsrc counts as fp32.
FC_TABLE_STATS never changes a class (it only makes calls off the split route invalid), so the sweep leaves it out and the CPU test
checks that on every representative; the process-global switches are swept on the split flags only (the others do not read them).
Out of scope: the 2 GB / 2^24-row conditions of `buf` / `wbuf` cannot turn false at these sizes (a 4 100 x 256 operand is 4 MB), so
buf = 0 / wbuf = 0 are reached through FC_CONV_FLAT and the image-less routes only.
"""
import ctypes
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

import fcaf3d_amd.functional as Fn
from fcaf3d_amd import _lib as L

E = L.header_enums()
FWD, WGRAD = 'fwd', 'wgrad'
ENV_DEFAULT = (2, 0, 1)                          # fc_set_split_mode, fc_set_bf16_fast, fc_debug_set_h3r
N_MAX = 4100                                     # no launch of these tests has more rows

# ---- the sweep's grid ---------------------------------------------------------------------------------------------------------------
N_LIST = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 513, 1000, 1023, 1024, 1025, 2049, 4095, 4096, 4097)
CHANNELS = ((64, 64), (64, 128), (128, 128), (128, 64), (32, 64), (256, 256), (3, 64), (16, 24))
KS = (27, 8, 1)
KINDS = ('none', 'dense', 'sorted', 'pairs', 'pairs_linear')          # pairs: the 3-D grid (live_tiles = 0), pairs_linear: the live-tile list
WGRAD_KINDS = ('none', 'dense', 'pairs')
ENVS = tuple((m, b, h) for m in (2, 0) for b in (0, 1) for h in (0, 1, 2))
_S1, _BM256 = 1 << Fn.CONV_S_SHIFT, 3 << Fn.CONV_BM_SHIFT
_SPLIT, _IMAGE, _FLAT = Fn.CONV_SPLIT, Fn.CONV_IMAGE, Fn.CONV_FLAT


def _fwd_flags():
    bases = (0, _SPLIT, _SPLIT | _IMAGE, _SPLIT | _FLAT, _SPLIT | _IMAGE | _FLAT, Fn.CONV_WT, _SPLIT | Fn.CONV_WT, Fn.CONV_FMA,
             Fn.CONV_FMA | Fn.CONV_WT)
    out = [b | o for o in (0, _S1, _BM256, _S1 | _BM256) for b in bases]
    for v in (Fn.CONV_PIPE_ON, Fn.CONV_PIPE_OFF, Fn.CONV_GLDS, Fn.CONV_GLDS_OFF):      # the flag-selected fp32 variants
        out += [v | b | o for o in (0, _BM256) for b in (0, Fn.CONV_WT)]
    return tuple(out)


def _wgrad_flags():
    bases = (0, _SPLIT, _SPLIT | _FLAT, Fn.CONV_FMA)
    out = [b | o for o in (0, _S1) for b in bases]
    for v in (Fn.CONV_WGRAD_PIPE_ON, Fn.CONV_WGRAD_PIPE_OFF, Fn.CONV_WGRAD_MULTI_OFF, Fn.CONV_WGRAD_MULTI_FIRST, Fn.CONV_WGRAD_DEEP,
              Fn.CONV_WGRAD_PIPE_OFF | Fn.CONV_WGRAD_MULTI_OFF):
        out += [v | b for b in (0, _SPLIT)]
    return tuple(out)


FWD_FLAGS, WGRAD_FLAGS = _fwd_flags(), _wgrad_flags()

FwdClass = namedtuple('FwdClass', 'family bm bn split wsrc mode buf epi linear')
WgradClass = namedtuple('WgradClass', 'family bm bn ko mode split wbuf table bkr')
# a call of the sweep's grid: square (n_in = n_out = n); kind: KINDS / WGRAD_KINDS; env: the process-global switches it needs
Rep = namedtuple('Rep', 'n Cin Cout K kind flags env')
# one GPU launch: rep's shape at other row counts, on a crafted table, with one operand variant ('int', 'zero': x all zero,
# 'stats': the statistics entry point on 0 / 1 operands, 'bn<i>': the BACKWARD form of that epilogue on the same operands with the
# option combination BN_COMBOS[i])
Case = namedtuple('Case', 'n_in n_out table variant')

_NAMES = {}
for _k, _v in E.items():
    for _p in ('FC_FAM_', 'FC_WFAM_', 'FC_WSRC_', 'FC_MODE_', 'FC_EPI_', 'FC_TABLE_'):
        if _k.startswith(_p):
            _NAMES[(_p, _v)] = _k[len(_p):].lower()


def class_id(direction, c):
    """the class as a test id"""
    n = lambda p, v: _NAMES[(p, v)]
    if direction == FWD:
        return (f'{n("FC_FAM_", c.family)}-{c.bm}x{c.bn}-{"split" if c.split else "whole"}-{n("FC_WSRC_", c.wsrc)}-{n("FC_MODE_", c.mode)}'
                f'-{"buf" if c.buf else "flat"}-epi_{n("FC_EPI_", c.epi)}-{"linear" if c.linear else "grid3d"}')
    return (f'{n("FC_WFAM_", c.family)}-{c.bm}x{c.bn}-ko{c.ko}-{n("FC_MODE_", c.mode)}-{"split" if c.split else "whole"}'
            f'-{"wbuf" if c.wbuf else "flat"}-{n("FC_TABLE_", c.table)}-bkr{c.bkr}')


# ---- the route query ----------------------------------------------------------------------------------------------------------------
def set_env(env):
    """the process-global switches (the route query and the launches read them); callers restore ENV_DEFAULT in `finally`"""
    l = L.lib()
    assert l.fc_set_split_mode(env[0]) == 0 and l.fc_set_bf16_fast(env[1]) == 0 and l.fc_debug_set_h3r(env[2]) == 0


def table_kind(kind, stats=False):
    t = {'none': E['FC_TABLE_NONE'], 'dense': E['FC_TABLE_DENSE'], 'sorted': E['FC_TABLE_SORTED'], 'pairs': E['FC_TABLE_PAIRS'],
         'pairs_linear': E['FC_TABLE_PAIRS']}[kind]
    return t | (E['FC_TABLE_STATS'] if stats else 0)


def full_live_tiles(n_out, K):
    """live_tiles of a pair list with every entry valid"""
    return K * ((n_out + 127) // 128)


_UNTILED_F = (E['FC_FAM_STEM'], E['FC_FAM_FMA'])
_UNTILED_W = (E['FC_WFAM_STEM'], E['FC_WFAM_FMA'])


def _untiled_wsrc(family, wsrc):
    """k_stem_fwd reads the fp32 kernel whatever FC_CONV_IMAGE says (no image exists for 3 input channels)"""
    return E['FC_WSRC_FP32'] if family == E['FC_FAM_STEM'] else wsrc


def _reduce(direction, r, linear):
    """route fields (dict by the header's lower-case names) -> class"""
    if direction == FWD:
        if r['family'] in _UNTILED_F:
            return FwdClass(r['family'], 0, 0, False, _untiled_wsrc(r['family'], r['wsrc']), r['mode'], r['buf'], r['epi'], False)
        return FwdClass(r['family'], r['bm'], r['bn'], r['s'] > 1, r['wsrc'], r['mode'], r['buf'], r['epi'], bool(linear))
    if r['family'] in _UNTILED_W:
        return WgradClass(r['family'], 0, 0, r['ko'], r['mode'], False, r['wbuf'], r['table'], r['bkr'])
    return WgradClass(r['family'], r['bm'], r['bn'], r['ko'], r['mode'], r['s'] > 1, r['wbuf'], r['table'], r['bkr'])


def route_fields(direction, n_in, n_out, K, Cin, Cout, flags, kind, live_tiles=0, stats=False):
    """(status, fields) of the route query for one call, under the CURRENT process-global switches"""
    if direction == FWD:
        return L.route('fc_conv_fwd_route', n_in, n_out, K, Cin, Cout, flags, table_kind(kind, stats), live_tiles)
    return L.route('fc_conv_wgrad_route', n_in, n_out, K, Cin, Cout, flags, table_kind(kind))


def route_class(direction, n_in, n_out, K, Cin, Cout, flags, kind, live_tiles=0, stats=False):
    """the class of one call under the CURRENT switches, or None where the entry point would return FC_EINVAL"""
    rc, r = route_fields(direction, n_in, n_out, K, Cin, Cout, flags, kind, live_tiles, stats)
    return None if rc != 0 else _reduce(direction, r, kind == 'pairs_linear' and live_tiles > 0)


class _Fast:
    """route_class without the dictionary (the sweep makes ~10^6 queries): the same reduction on the raw out[] by FC_ROUTE_* index"""

    def __init__(self):
        l = L.lib()
        self.f, self.w, self.out = l.fc_conv_fwd_route, l.fc_conv_wgrad_route, (ctypes.c_int * 16)()
        self.fi = {k[len('FC_ROUTE_'):].lower(): v for k, v in E.items() if k.startswith('FC_ROUTE_')}
        self.wi = {k[len('FC_WROUTE_'):].lower(): v for k, v in E.items() if k.startswith('FC_WROUTE_')}

    def fwd(self, n, K, Cin, Cout, flags, tk, live, n_in=None):
        if self.f(n if n_in is None else n_in, n, K, Cin, Cout, flags, tk, live, self.out) != 0:
            return None
        o, i = self.out, self.fi
        if o[i['family']] in _UNTILED_F:
            return FwdClass(o[i['family']], 0, 0, False, _untiled_wsrc(o[i['family']], o[i['wsrc']]), o[i['mode']], o[i['buf']], o[i['epi']], False)
        return FwdClass(o[i['family']], o[i['bm']], o[i['bn']], o[i['s']] > 1, o[i['wsrc']], o[i['mode']], o[i['buf']], o[i['epi']], live > 0)

    def wgrad(self, n, K, Cin, Cout, flags, tk, n_in=None):
        if self.w(n if n_in is None else n_in, n, K, Cin, Cout, flags, tk, self.out) != 0:
            return None
        o, i = self.out, self.wi
        if o[i['family']] in _UNTILED_W:
            return WgradClass(o[i['family']], 0, 0, o[i['ko']], o[i['mode']], False, o[i['wbuf']], o[i['table']], o[i['bkr']])
        return WgradClass(o[i['family']], o[i['bm']], o[i['bn']], o[i['ko']], o[i['mode']], o[i['s']] > 1, o[i['wbuf']], o[i['table']], o[i['bkr']])


@functools.lru_cache(maxsize=None)
def _fast():
    return _Fast()


def fast_class(direction, n_in, n_out, K, Cin, Cout, flags, kind, live_tiles=0, stats=False):
    """route_class by the short way (tests/test_conv_routes_cpu.py holds the two equal)"""
    live = live_tiles if kind == 'pairs_linear' else 0
    if direction == FWD:
        return _fast().fwd(n_out, K, Cin, Cout, flags, table_kind(kind, stats), live, n_in)
    return _fast().wgrad(n_out, K, Cin, Cout, flags, table_kind(kind), n_in)


@functools.lru_cache(maxsize=None)
def sweep():
    """-> {FWD: {class: Rep}, WGRAD: {class: Rep}}: every class the grid above reaches, with its representative (the smallest n,
    then the first channel pair, K, table kind, flags word and switch setting in list order)"""
    fast = _fast()
    best = {FWD: {}, WGRAD: {}}

    def keep(direction, cls, key):
        if cls is not None and (cls not in best[direction] or key < best[direction][cls]):
            best[direction][cls] = key
    try:
        seen_env = set()
        for ie, env in enumerate(ENVS):
            # what the routes read of the switches: split mode 0 while bf16-fast is on, h3r in split mode 2 only — the later
            # settings that read the same repeat an earlier one's classes
            eff = (0 if env[1] else env[0], env[1], env[2] if (env[0] == 2 and not env[1]) else -1)
            if eff in seen_env:
                continue
            seen_env.add(eff)
            set_env(env)
            for direction, flag_list, kinds in ((FWD, FWD_FLAGS, KINDS), (WGRAD, WGRAD_FLAGS, WGRAD_KINDS)):
                flag_ids = [i for i, f in enumerate(flag_list) if (f & _SPLIT) or env == ENV_DEFAULT]
                for i_n, n in enumerate(N_LIST):
                    for ic, (Cin, Cout) in enumerate(CHANNELS):
                        for ik, K in enumerate(KS):
                            for it, kind in enumerate(kinds):
                                tk = table_kind(kind)
                                live = full_live_tiles(n, K) if kind == 'pairs_linear' else 0
                                for i_f in flag_ids:
                                    cls = (fast.fwd(n, K, Cin, Cout, flag_list[i_f], tk, live) if direction == FWD else
                                           fast.wgrad(n, K, Cin, Cout, flag_list[i_f], tk))
                                    keep(direction, cls, (i_n, ic, ik, it, i_f, ie))
    finally:
        set_env(ENV_DEFAULT)
    out = {}
    for direction, flag_list, kinds in ((FWD, FWD_FLAGS, KINDS), (WGRAD, WGRAD_FLAGS, WGRAD_KINDS)):
        out[direction] = {cls: Rep(N_LIST[i_n], *CHANNELS[ic], KS[ik], kinds[it], flag_list[i_f], ENVS[ie])
                          for cls, (i_n, ic, ik, it, i_f, ie) in sorted(best[direction].items())}
    return out


# ---- row counts and cases of a class ---------------------------------------------------------------------------------------------------
def _square_class(direction, rep, n, live=None):
    live = (full_live_tiles(n, rep.K) if live is None else live) if rep.kind == 'pairs_linear' else 0
    return fast_class(direction, n, n, rep.K, rep.Cin, rep.Cout, rep.flags, rep.kind, live)


def tile_of(direction, rep):
    """(tile rows, S) the crafted tables of a class are shaped on, from the representative's route: the forward tile and offset
    split; for a weight gradient the rows of one range (the rows per chunk where there is one range) and max(S, 2)"""
    rc, r = route_fields(direction, rep.n, rep.n, rep.K, rep.Cin, rep.Cout, rep.flags, rep.kind,
                         full_live_tiles(rep.n, rep.K) if rep.kind == 'pairs_linear' else 0)
    assert rc == 0
    if direction == FWD:
        return (r['bm'] or 64), max(r['s'], 1)
    return (min(r['rps'], 1024) if r['s'] > 1 else r['bkr']), max(r['s'], 1)


def row_counts(direction, cls, rep):
    """the representative's n, then the row counts nearest to the tile edges {bm - 1, bm, bm + 1, 2 bm + 1} (weight gradients: bkr for
    bm, and rps - 1, rps, rps + 1, S rps - 63, (S - 1) rps + 1 with the representative's rps and S, then — rps follows n — the first
    row counts of the class whose last row range is one row, full, or one row short), and n + 1 (from BIG_ROWS rows: and N_MAX),
    at which the route query still answers `cls`.  A class that exists from some size on (or in a band) keeps the reachable values: the nearest
    one is then the edge of its own rule.  Call under rep.env."""
    rc, r = route_fields(direction, rep.n, rep.n, rep.K, rep.Cin, rep.Cout, rep.flags, rep.kind,
                         full_live_tiles(rep.n, rep.K) if rep.kind == 'pairs_linear' else 0)
    assert rc == 0 and _square_class(direction, rep, rep.n) == cls, (cls, rep)
    if direction == FWD:
        bm = r['bm'] or 64
        targets = [bm - 1, bm, bm + 1, 2 * bm + 1]
    else:
        b, rps, S = r['bkr'], r['rps'], r['s']
        targets = [b - 1, b, b + 1, 2 * b + 1, rps - 1, rps, rps + 1, S * rps - 63, (S - 1) * rps + 1]
        if S > 1:
            # rps follows n: the first row counts of the class whose LAST row range holds one row / is full / lacks one row
            f, tk = _fast(), table_kind(rep.kind)
            want = {1: None, 0: None, -1: None}
            for n in range(rep.n, min(N_MAX, rep.n + 2048) + 1):
                if f.wgrad(n, rep.K, rep.Cin, rep.Cout, rep.flags, tk) != cls:
                    continue
                last = n - (f.out[f.wi['s']] - 1) * f.out[f.wi['rps']]
                for k in want:
                    if want[k] is None and last == (f.out[f.wi['rps']] + k if k < 1 else k):
                        want[k] = n
            targets += [n for n in want.values() if n is not None]
    targets += [rep.n + 1] + ([N_MAX] if rep.n >= BIG_ROWS else [])
    inside = functools.lru_cache(maxsize=None)(lambda n: 1 <= n <= N_MAX and _square_class(direction, rep, n) == cls)
    out = [rep.n]
    for t in targets:
        t = min(max(t, 1), N_MAX)
        for d in range(N_MAX):
            hit = next((v for v in (t - d, t + d) if inside(v)), None)
            if hit is not None:
                if hit not in out:
                    out.append(hit)
                break
    return out


BIG_ROWS = 4096                                  # from here on a row count takes the `full` and `offset_holes` tables only
EDGE_TABLES = ('full', 'empty', 'last_only', 'tile_holes', 'offset_holes')
BIG_TABLES = ('full', 'offset_holes')
EXTRA_TABLES = ('first_only', 'offset_holes_b', 'fan_in', 'perm')          # at the representative's row count only


def live_tiles_of(nbr):
    return int(((np.count_nonzero(nbr >= 0, axis=1) + 127) // 128).sum())


def has_stats(direction, cls):
    return direction == FWD and cls.epi != E['FC_EPI_NONE']


def cases(direction, cls, rep):
    """the GPU launches of a class: every row count of `row_counts` x EDGE_TABLES (BIG_TABLES from BIG_ROWS rows), at the
    representative's row count also EXTRA_TABLES, an all-zero x, and `perm` tables over n_in = 2 n + 3 and n // 8 + 1 input rows (the
    strided and the generative shape); classes with a statistics epilogue run every edge table through the statistics entry point
    as well, and a third time through its BACKWARD form ('bn<i>', the option combinations BN_COMBOS in turn) — that form also on
    the two `perm` shapes, on `fan_in` and `first_only`, and, where a sum kernel writes the table, at RB_ROWS; every such class sees
    every combination, and `empty` only combinations that pass `add` (both asserted here).  Table-free classes (K = 1, the row itself is the index) have the row counts and the all-zero x only.  Each case is
    confirmed by the route query: for the linear pair-list launch the class depends on the table's own live-tile count, and a
    table without any pair (live_tiles = 0) IS the 3-D launch, so those cases belong to the sibling class and are left to it.
    Call under rep.env."""
    tile, S = tile_of(direction, rep)
    out = []
    epi = has_stats(direction, cls)
    turn = [0]                                   # the next option combination of the backward epilogue

    def add(n_in, n_out, table, variant):
        live = 0
        if rep.kind == 'pairs_linear':
            live = live_tiles_of(make_table(table, rep.K, n_in, n_out, tile, S))
        stats = variant == 'stats' or is_bn(variant)
        if fast_class(direction, n_in, n_out, rep.K, rep.Cin, rep.Cout, rep.flags, rep.kind, live, stats) == cls:
            out.append(Case(n_in, n_out, table, variant))
            return True
        return False

    def add_bn(n_in, n_out, table):
        """the backward-epilogue twin of a statistics case, the option combinations in turn; without any pair the result is zero and
        every sum with it unless `add` is passed, so `empty` takes the next combination that passes one"""
        i = turn[0]
        while table == 'empty' and not BN_COMBOS[i % len(BN_COMBOS)].add:
            i += 1
        if add(n_in, n_out, table, bn_variant(i % len(BN_COMBOS))):
            turn[0] = i + 1
    for n in row_counts(direction, cls, rep):
        if rep.kind == 'none':
            add(n, n, 'identity', 'int')
            if epi:
                add(n, n, 'identity', 'stats')
                add_bn(n, n, 'identity')
            continue
        for t in (EDGE_TABLES if n < BIG_ROWS else BIG_TABLES):
            add(n, n, t, 'int')
            if epi:
                add(n, n, t, 'stats')
                add_bn(n, n, t)
    n = rep.n
    if rep.kind == 'none':
        add(n, n, 'identity', 'zero')
    else:
        for t in EXTRA_TABLES:
            add(n, n, t, 'int')
        add(n, n, 'full', 'zero')
        for n_in in (2 * n + 3, n // 8 + 1):
            add(n_in, n, 'perm', 'int')
    if epi:
        base = 'identity' if rep.kind == 'none' else 'full'
        if rep.kind != 'none':
            # the strided and the generative shape of a real backward-data pass (bn_x has n_out rows, x has not), and the two tables
            # that leave most rows (fan_in: some rows) without any neighbour
            for n_in in (2 * n + 3, n // 8 + 1):
                add_bn(n_in, n, 'perm')
            for t in ('fan_in', 'first_only'):
                add_bn(n, n, t)
        if cls.epi == E['FC_EPI_SUM']:
            # the sum kernels' row blocks follow the row count (conv.hip fc_stat_rb: 16 rows up to 1 024, 64 up to 4 096, then 32): both
            # steps, and the row counts whose last block ends k_sum_pairs_stats' two-rows-per-pass loop on a partial pass
            for m, t in RB_ROWS:
                add_bn(m, m, base if rep.kind == 'none' else t)
        seen = {c.variant for c in out if is_bn(c.variant)}
        for i in range(len(BN_COMBOS)):          # a short case list (table-free classes) did not get through the cycle
            if bn_variant(i) not in seen:
                add(n, n, base, bn_variant(i))
        seen = {c.variant for c in out if is_bn(c.variant)}
        assert seen == {bn_variant(i) for i in range(len(BN_COMBOS))}, (cls, rep, sorted(seen))
        assert all(bn_combo(c.variant).add for c in out if is_bn(c.variant) and c.table == 'empty'), (cls, rep)
    return out


def required_tables(direction, rep):
    """the tables every class must keep after the route filter"""
    if rep.kind == 'none':
        return {'identity'}
    if rep.kind == 'pairs_linear':               # (tables without a pair are the 3-D launch; the sparse ones may leave a live-tile band)
        return {'full', 'offset_holes' if rep.K > 1 else 'offset_holes_b'}          # (K = 1: variant a has no pair)
    return set(EDGE_TABLES if rep.n < BIG_ROWS else BIG_TABLES)


# ---- crafted neighbour tables -------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode())


OFFSET_HOLE_COUNTS = lambda bm: (0, 1, bm - 1, bm, bm + 1)


def offset_hole_counts(K, n_out, bm, S, variant_b=False):
    """rows per offset of the `offset_holes` tables: none at k = 1 (mod max(S, 2)); the others cycle through {0, 1, bm - 1, bm, bm + 1}
    (clipped to n_out), the cycle placed so that offset K - 1 is empty (variant a) or the fullest (variant b)"""
    m = max(S, 2)
    live = [k for k in range(K) if k % m != 1]
    cyc = OFFSET_HOLE_COUNTS(bm)
    shift = ((4 if variant_b else 0) - (len(live) - 1)) % 5          # position in the cycle of the LAST live offset
    cnt = [0] * K
    for j, k in enumerate(live):
        cnt[k] = min(cyc[(j + shift) % 5], n_out)
    return cnt


@functools.lru_cache(maxsize=256)
def make_table(name, K, n_in, n_out, tile, S):
    """(K, n_out) int32 over n_in input rows, every entry in [-1, n_in) — the tables of the issue's list; tile / S: `tile_of`"""
    rng = np.random.default_rng(_seed(name, K, n_in, n_out, tile, S))
    nbr = np.full((K, n_out), -1, np.int32)
    if name == 'full':
        nbr[:] = rng.integers(0, n_in, (K, n_out))
    elif name == 'empty':
        pass
    elif name == 'last_only':
        nbr[K - 1, n_out - 1] = n_in - 1
    elif name == 'first_only':
        nbr[0, 0] = 0
    elif name == 'fan_in':
        nbr[rng.random((K, n_out)) < 0.6] = n_in - 1
    elif name == 'tile_holes':                   # odd tiles: nothing; even tile t: offset t / 2 (mod K) only, every row
        for t in range(0, (n_out + tile - 1) // tile, 2):
            lo, hi = t * tile, min((t + 1) * tile, n_out)
            nbr[(t // 2) % K, lo:hi] = rng.integers(0, n_in, hi - lo)
    elif name in ('offset_holes', 'offset_holes_b'):
        for k, c in enumerate(offset_hole_counts(K, n_out, tile, S, name.endswith('_b'))):
            rows = (k * 37 + np.arange(c)) % n_out          # a run of rows that starts inside a tile and may wrap
            nbr[k, rows] = rng.integers(0, n_in, c)
    elif name == 'perm':                         # per offset an injective partial map: ~60 % of the rows, fewer where n_in runs out
        c = min(int(round(0.6 * n_out)), n_in)
        for k in range(K):
            nbr[k, rng.permutation(n_out)[:c]] = rng.permutation(n_in)[:c]
    else:
        raise KeyError(name)
    nbr.setflags(write=False)
    return nbr


# ---- operands and exact references ----------------------------------------------------------------------------------------------------
def int_operand(shape, amp, seed, zero_frac=1.0 / 3.0, lo=None):
    """fp32 integers in [lo, amp] (lo = -amp by default), `zero_frac` of them zero"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-amp if lo is None else lo, amp + 1, shape).astype(np.float32)
    v[rng.random(shape) < zero_frac] = 0.0
    return v


def operands(n_in, n_out, K, Cin, Cout, variant):
    """(x (n_in, Cin), w (K, Cin, Cout), gout (n_out, Cout)) as read-only float32 arrays.  'int': x, gout in [-8, 8], w in [-4, 4];
    'zero': x all zero; 'stats' (and the backward epilogue's 'bn<i>'): x in {0, 1} (two thirds zero), w in {-1, 0, 1}"""
    return _operands(n_in, n_out, K, Cin, Cout, operand_variant(variant))


@functools.lru_cache(maxsize=64)
def _operands(n_in, n_out, K, Cin, Cout, variant):
    key = (n_in, n_out, K, Cin, Cout)
    if variant == 'stats':
        x = int_operand((n_in, Cin), 1, _seed('x', key), 2.0 / 3.0, lo=0)
        w = int_operand((K, Cin, Cout), 1, _seed('w', key))
    else:
        x = int_operand((n_in, Cin), 8, _seed('x', key))
        w = int_operand((K, Cin, Cout), 4, _seed('w', key))
        if variant == 'zero':
            x = np.zeros_like(x)
    go = int_operand((n_out, Cout), 8, _seed('g', key))
    for a in (x, w, go):
        a.setflags(write=False)
    return x, w, go


EXACT = float(2 ** 24)


def _exact32(ref64, what):
    assert ref64.numel() == 0 or float(ref64.abs().max()) < EXACT, f'{what}: reference leaves the exact fp32 integers'
    return ref64.to(torch.float32)


def _t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def ref_fwd(x, w, nbr):
    """y[o] = sum_k x[nbr[k][o]] @ w[k] in float64 (exact on these integers) -> float32 tensor; nbr None: y = x @ w[0]"""
    x64, w64 = _t64(x), _t64(w)
    if nbr is None:
        return _exact32(x64 @ w64[0], 'y')
    y = torch.zeros((nbr.shape[1], w64.shape[2]), dtype=torch.float64)
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        if len(o):
            y[torch.from_numpy(o)] += x64[torch.from_numpy(nbr[k, o].astype(np.int64))] @ w64[k]
    return _exact32(y, 'y')


def ref_wgrad(x, go, nbr, K):
    """gW[k] = sum_o x[nbr[k][o]]^T (x) gout[o] in float64 -> float32 tensor (K, Cin, Cout)"""
    x64, g64 = _t64(x), _t64(go)
    if nbr is None:
        return _exact32((x64.t() @ g64)[None], 'gW')
    gw = torch.zeros((K, x64.shape[1], g64.shape[1]), dtype=torch.float64)
    for k in range(K):
        o = np.nonzero(nbr[k] >= 0)[0]
        if len(o):
            gw[k] = x64[torch.from_numpy(nbr[k, o].astype(np.int64))].t() @ g64[torch.from_numpy(o)]
    return _exact32(gw, 'gW')


def ref_dgrad(go, w, nbr, n_in):
    """gx[i] = sum over the pairs (k, o) with nbr[k][o] = i of gout[o] @ w[k]^T in float64 -> float32 tensor (n_in, Cin)"""
    g64, w64 = _t64(go), _t64(w)
    if nbr is None:
        return _exact32(g64 @ w64[0].t(), 'gx')
    gx = torch.zeros((n_in, w64.shape[1]), dtype=torch.float64)
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        if len(o):
            gx.index_add_(0, torch.from_numpy(nbr[k, o].astype(np.int64)), g64[torch.from_numpy(o)] @ w64[k].t())
    return _exact32(gx, 'gx')


def ref_stem_col(x, nbr):
    """(n_out, 84) gathered stem inputs: col[o][3 k + c] = x[nbr[k][o]][c], zero where absent and past 3 K"""
    K, n_out = nbr.shape
    col = np.zeros((n_out, 84), np.float32)
    for k in range(K):
        o = np.nonzero(nbr[k] >= 0)[0]
        col[o, 3 * k:3 * k + 3] = np.asarray(x)[nbr[k, o]]
    return torch.from_numpy(col)


# ---- the backward form of the statistics epilogue -----------------------------------------------------------------------------------------
# fc_conv_fwd_bn_bwd_stats / fc_conv_fwd_pairs_tiles_bn_bwd_stats: the launch's result g is the gradient arriving at a BatchNorm (+ ReLU /
# ELU) layer with input bn_x; its epilogue leaves, per row block, the column sums of g' = (g + add) act'(.) and of g' xhat.  The inputs
# are designed as tests/norm_cases.py designs its backward inputs — bn_x integers in [-8, 8], integer mean, var in {1, 0.25} with
# eps = 0 (1 / sqrtf(var) is exactly 1 or 2), gamma in {1, 2, 0.5}, integer beta, add integers in [-8, 8] — so xhat = (bn_x - mean) is
# is an integer, pre = fmaf(xhat, gamma, beta) a multiple of 1/2, and both are exact in fp32.  act' is
#   * 1 without an activation (a bn_y passed all the same — NaN throughout — must not be read into the sums),
#   * ReLU: pre > 0, or bn_y > 0 where the layer's output is given: bn_y = relu(pre + res) with an integer residual, so that its sign
#     disagrees with pre's on a visible share of the elements, exact zeros (res = -pre) among them; pre == 0 is planted in every
#     64-column block (it tells ReLU's act' = 0 from ELU's expf(0) = 1 and from `pre >= 0`),
#   * ELU from bn_y: bn_y + 1 where bn_y <= 0; the outputs are positive integers, 0, -0.5 and -0.75, so act' is 1, 0.5 or 0.25,
#   * ELU recomputed from bn_x — the one place a transcendental enters: expf(pre) where pre <= 0.  Kept exact by construction: every
#     element whose pre would be negative gets bn_x = mean - 2 (130 + k), k in 0..6, so that pre = -2 (130 + k) is gamma + beta <= -128
#     (is gamma >= 1/2, beta <= 2) and pre takes only values > 0, == 0 or <= -128.  exp(-128) = 2^-184.7 lies below half the
#     smallest fp32 denormal, 2^-150: ANY expf that is within the whole denormal range of the true value returns +0 there, and
#     expf(0) = 1.  So act' is 1 or 0 exactly and no tolerance is needed.  Where `add` is passed, half of those elements also carry
#     add = -g (the reference result): v = g + add = 0 exactly there, whatever act' is.
# Every term is then a multiple of 1/4.  The cap, a condition on the REFERENCE as in the forward form: 4 sum_rows |g'| and
# 4 sum_rows |g' xhat| stay below 2^24 per column — then every partial sum in any order is a multiple of 1/4 below 2^22, exact in
# fp32, and the table's column totals equal the float64 reference bit for bit.
NONE, RELU, ELU = 0, 1, 2
# act; `add` passed; y: None (act' recomputed from bn_x), 'y' (the layer's output), 'nan' (an output that must be ignored); gamma / beta given
BnCombo = namedtuple('BnCombo', 'act add y affine')
BN_COMBOS = (BnCombo(NONE, False, None, False), BnCombo(NONE, True, 'nan', True), BnCombo(RELU, False, None, True),
             BnCombo(RELU, True, 'y', True), BnCombo(RELU, False, 'y', True), BnCombo(ELU, False, None, True),
             BnCombo(ELU, True, None, True), BnCombo(ELU, True, 'y', True), BnCombo(RELU, True, None, True))
# fc_stat_rb's steps; 1 047 = 16 x 64 + 23 and 4 095 = 63 x 64 + 63 end on a partial pass (on `full`: its rows all have a result)
RB_ROWS = ((1024, 'full'), (1025, 'offset_holes'), (1047, 'full'), (4095, 'full'), (4096, 'offset_holes'), (4097, 'full'))
BnCase = namedtuple('BnCase', 'combo g x mean var gamma beta add y res')


def is_bn(variant):
    return variant.startswith('bn')


def bn_variant(i):
    return f'bn{i}'


def bn_combo(variant):
    return BN_COMBOS[int(variant[2:])] if is_bn(variant) else None


def operand_variant(variant):
    """the convolution operands of a case: the backward epilogue runs on the statistics variant's (the `int` operands push
    sum |g' xhat| past 2^24 at 4 097 rows x 256 channels)"""
    return 'stats' if is_bn(variant) else variant


def stat_rb(n):
    """conv.hip fc_stat_rb: rows per block of k_sum_parts_stats / k_sum_pairs_stats"""
    return 16 if n <= 1024 else 64 if n <= 4096 else 32


def sorted_order(n_out):
    """out_index of the `sorted` launches: a seeded permutation of the rows"""
    return np.random.default_rng(n_out).permutation(n_out).astype(np.int32)


@functools.lru_cache(maxsize=64)
def stats_result(n_in, n_out, K, Cin, Cout, table, tile, S):
    """g: the exact result of the launch on the statistics variant's operands, float64 (n_out, Cout), read-only"""
    x, w, _ = operands(n_in, n_out, K, Cin, Cout, 'stats')
    nbr = None if table == 'identity' else make_table(table, K, n_in, n_out, tile, S)
    g = ref_fwd(x, w, nbr).double().numpy()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=16)
def _bn_base(n_out, C):
    """what the option combinations share at one shape: (bn_x, add, res, mean, var, gamma, beta) float64"""
    from tests import norm_cases as NC
    key = (n_out, C)
    gamma, beta = NC.affine(C)
    mean, var = (a[0] for a in NC.given_stats(1, C))
    is_ = 1.0 / np.sqrt(var)
    rng = np.random.default_rng(_seed('bn', key))
    x = int_operand((n_out, C), 8, _seed('bn_x', key)).astype(np.float64)
    # pre == 0: bn_x = mean - beta / (is gamma) in the columns where that is an integer (beta = 0: every fifth column) — a tenth of
    # their elements, and column c's row c mod n_out
    x0 = mean - beta / (is_ * gamma)
    ok = (x0 == np.rint(x0)) & (np.abs(x0) <= 8)
    assert C % 64 == 0 and ok.reshape(-1, 64).any(1).all()
    plant = rng.random((n_out, C)) < 0.1
    plant[np.arange(C) % n_out, np.arange(C)] = True
    x = np.where(plant & ok, x0, x)
    add = int_operand((n_out, C), 8, _seed('bn_add', key)).astype(np.float64)
    res = int_operand((n_out, C), 8, _seed('bn_res', key)).astype(np.float64)
    pre = (x - mean) * is_ * gamma + beta
    res = np.where((rng.random((n_out, C)) < 0.05) & (pre == np.rint(pre)), 0.0 - pre, res)          # exact zeros of the layer's output
    for a in (x, add, res, mean, var, gamma, beta):
        a.setflags(write=False)
    return x, add, res, mean, var, gamma, beta


@functools.lru_cache(maxsize=8)
def bn_case(n_in, n_out, K, Cin, Cout, table, tile, S, variant):
    """the epilogue inputs of one backward-epilogue case (float64, read-only; add / y None where the combination passes none; gamma /
    beta hold what the kernel uses for NULL where the combination passes none) with the reference result g"""
    combo = bn_combo(variant)
    g = stats_result(n_in, n_out, K, Cin, Cout, table, tile, S)
    x, add, res, mean, var, gamma, beta = _bn_base(n_out, Cout)
    if not combo.affine:
        gamma, beta = np.ones(Cout), np.zeros(Cout)
    add = add if combo.add else None
    is_ = 1.0 / np.sqrt(var)
    r, c = np.ogrid[:n_out, :Cout]
    if combo.act == ELU and combo.y is None:
        neg = (x - mean) * is_ * gamma + beta < 0
        x = np.where(neg, mean - 2.0 * (130 + (r + c) % 7), x)
        if combo.add:
            add = np.where(neg & ((r + c) % 2 == 0), 0.0 - g, add)
    pre = (x - mean) * is_ * gamma + beta
    y = None
    if combo.y == 'nan':
        y = np.full((n_out, Cout), np.nan)
    elif combo.y == 'y':
        t = pre + res
        f = np.floor(t)
        y = np.maximum(t, 0.0) if combo.act == RELU else np.where(f > 0, f, np.where(f == 0, 0.0, np.where(f % 2 == 0, -0.5, -0.75)))
    for a in (x, add, y):
        if a is not None:
            a.setflags(write=False)
    return BnCase(combo, g, x, mean, var, gamma, beta, add, y, res)


# one-token mutations of the reference (tests/test_conv_routes_cpu.py: each changes a column total wherever its branch is live)
MUTATIONS = ('act_ignored', 'add_dropped', 'pre_for_y', 'y_for_act0', 'pre_ge0', 'skip_no_neighbour', 'launch_row', 'last_row_dropped',
             'o16_dropped')


def bn_terms(bc, mut=None, order=None):
    """(g', g' xhat) in float64, (n_out, C) each: g' = (g + add) act'(.), xhat = (bn_x - mean) / sqrt(var)"""
    act = bc.combo.act
    xh = (bc.x - bc.mean) / np.sqrt(bc.var)
    pre = xh * bc.gamma + bc.beta
    g = bc.g[order] if mut == 'launch_row' else bc.g          # launch row r holds the result of row out_index[r], reads bn_x / add / bn_y at r
    add = 0.0 if (bc.add is None or mut == 'add_dropped') else bc.add
    from_y = bc.y is not None and act != NONE
    if mut == 'pre_for_y':
        from_y = False
    if mut == 'y_for_act0' and bc.y is not None and act == NONE:
        from_y, act = True, RELU
    if mut == 'act_ignored':
        act = NONE
    pos = pre >= 0 if mut == 'pre_ge0' else pre > 0
    if act == NONE:
        d = np.ones_like(pre)
    elif from_y:
        d = (bc.y > 0).astype(np.float64) if act == RELU else np.where(bc.y > 0, 1.0, bc.y + 1.0)
    elif act == RELU:
        d = pos.astype(np.float64)
    else:
        assert mut == 'pre_for_y' or ((pre > 0) | (pre == 0) | (pre <= -128)).all(), 'ELU recomputed: a pre-activation whose expf is not exact'
        d = np.where(pos, 1.0, np.exp(np.minimum(pre, 0.0)).astype(np.float32).astype(np.float64))          # fp32: 1 at 0, +0 from -128 down
    gp = (g + add) * d
    return gp, gp * xh


def o16_rows(n):
    """rows o + 16 of the LAST pass of k_sum_pairs_stats over a row block whose rows leave that pass partial: lanes with a row o but
    no row o + 16 beside lanes with both (the `two` guard) — the short last block of fc_stat_rb(n) >= 32 rows only"""
    rb = stat_rb(n)
    r0 = (n - 1) // rb * rb
    last = (n - r0 - 1) // 32 * 32
    m = n - r0 - last                              # rows of the last pass
    return np.arange(r0 + last + 16, n) if 16 < m < 32 else np.arange(0)


def bn_sums(bc, mut=None, nbr=None, order=None):
    """(2, C) float64: the column totals of g' and of g' xhat — the reference of both planes of the table (mut: one of MUTATIONS)"""
    gp, gx = bn_terms(bc, mut, order)
    w = np.ones(len(gp))
    if mut == 'skip_no_neighbour' and nbr is not None:
        w = (nbr >= 0).any(0).astype(np.float64)
    elif mut == 'last_row_dropped':
        w[-1] = 0.0
    elif mut == 'o16_dropped':
        w[o16_rows(len(gp))] = 0.0
    return np.stack([(w[:, None] * gp).sum(0), (w[:, None] * gx).sum(0)])


def bn_cap(bc):
    """the exactness cap as a fraction of 2^24 (the factor 4: the quarter-valued ELU derivatives)"""
    gp, gx = bn_terms(bc)
    return 4.0 * max(float(np.abs(gp).sum(0).max()), float(np.abs(gx).sum(0).max())) / EXACT


def mutation_live(mut, bc, nbr, kinds, order):
    """is the branch a mutation changes reached by this case — from the option combination and the table's structure alone.  kinds:
    the launch kinds the class runs the case through; nbr None: table-free"""
    combo, n = bc.combo, len(bc.g)
    covered = np.ones(n, bool) if nbr is None else (nbr >= 0).any(0)          # rows with a neighbour: g is not zero there
    some = combo.add or bool(covered.any())
    if mut == 'act_ignored':
        return combo.act != NONE and some
    if mut == 'add_dropped':
        return combo.add
    if mut == 'pre_for_y':
        return combo.y == 'y' and some
    if mut == 'y_for_act0':
        return combo.y == 'nan' and some
    if mut == 'pre_ge0':                           # ReLU recomputed (ELU: expf(0) = 1 either way); a pre == 0 sits in one row in ten
        return combo.act == RELU and combo.y is None and (combo.add or int(covered.sum()) >= min(n, 16))
    if mut == 'skip_no_neighbour':
        return combo.add and not covered.all()
    if mut == 'launch_row':                        # a row with a result that the order moves
        return 'sorted' in kinds and bool((covered[order] & (order != np.arange(n))).any())
    if mut == 'last_row_dropped':
        return combo.add or bool(covered[-1])
    if mut == 'o16_dropped':
        rows = o16_rows(n)
        return any(k.startswith('pairs') for k in kinds) and len(rows) > 0 and (combo.add or bool(covered[rows].any()))
    raise KeyError(mut)


def bn_facts(bc, nbr):
    """the branch facts a combination claims, recomputed from the inputs"""
    xh = (bc.x - bc.mean) / np.sqrt(bc.var)
    pre = xh * bc.gamma + bc.beta
    covered = np.ones(len(bc.g), bool) if nbr is None else (nbr >= 0).any(0)
    f = {'pre_zero_blocks': bool((pre == 0).any(0).reshape(-1, 64).any(1).all()), 'big_negative': int((pre <= -128).sum()),
         'small_negative': int(((pre < 0) & (pre > -128)).sum()), 'lonely_rows': int((~covered).sum()),
         'add_cancels': 0 if bc.add is None else int(((bc.g + bc.add == 0) & (pre <= -128) & (bc.g != 0)).sum())}
    if bc.combo.y == 'y':
        f['y_disagrees'] = float((((bc.y > 0) != (pre > 0))).mean())
        f['y_zero'] = int((bc.y == 0).sum())
        f['y_values'] = set(np.unique(bc.y[bc.y <= 0]).tolist())
    return f
