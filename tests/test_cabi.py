"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/fcaf3d_hip.h declares."""
import ctypes
import os

from fcaf3d_amd import _lib as L


def test_library_exports_every_declared_symbol():
    from fcaf3d_amd.build import build
    path = build(verbose=False)
    assert os.path.exists(path)
    protos = L.parse_header()
    assert len(protos) >= 20
    lib = ctypes.CDLL(path)
    missing = [n for n in protos if not hasattr(lib, n)]
    assert not missing, missing


def test_abi_version_matches_the_header_and_the_host():
    import re
    from fcaf3d_amd._lib import HEADER
    v = int(re.search(r'#define FC_ABI_VERSION (\d+)', open(HEADER).read()).group(1))
    assert L.lib().fc_abi_version() == v == L.ABI_VERSION


def test_size_queries_run_without_gpu():
    assert L.query('fc_hash_unique_ws_bytes', 1000) > 0
    assert L.query('fc_conv_wgrad_ws_bytes', 100000, 27, 64, 64, 0) >= 27 * 64 * 64 * 4
    assert L.query('fc_col_stats_ws_bytes', 1000, 64, 1) > 0


def test_every_prototype_cites_its_reference_interface():
    """include/fcaf3d_hip.h: the comment above each declaration names the reference file:line it replaces (or says that
    there is no reference counterpart)"""
    import re
    from fcaf3d_amd._lib import HEADER
    txt = open(HEADER).read()
    last, missing = '', []
    for block in re.split(r'(/\*.*?\*/)', txt, flags=re.S):
        if block.startswith('/*'):
            last = block
            continue
        for m in re.finditer(r'\b(?:int64_t|int)\s+(fc_\w+)\s*\(', block):
            if not re.search(r'\.(py|cu|cpp|cuh)\s*:\s*\d+|No reference counterpart', last):
                missing.append(m.group(1))
    assert not missing, missing


def test_conv_flag_constants_mirror_the_header():
    """every FC_CONV_* bit / field of the convolution `flags` word in include/fcaf3d_hip.h has its Python twin in
    fcaf3d_amd.functional (CONV_*), with the same value"""
    import re
    import fcaf3d_amd.functional as Fn
    from fcaf3d_amd._lib import HEADER
    hdr = {}
    for m in re.finditer(r'^#define FC_(CONV_\w+) \(?(\d+)(?: << (\d+))?\)?$', open(HEADER).read(), flags=re.M):
        hdr[m.group(1)] = int(m.group(2)) << int(m.group(3) or 0)
    assert len(hdr) == 19, hdr
    assert (hdr['CONV_FMA'], hdr['CONV_WT'], hdr['CONV_SPLIT'], hdr['CONV_IMAGE'], hdr['CONV_FLAT']) == (1, 1 << 23, 1 << 24, 1 << 26, 1 << 27)
    py = {k: v for k, v in vars(Fn).items() if re.fullmatch(r'CONV_[A-Z0-9_]+', k) and k not in ('CONV_X6',)}
    assert py == hdr


def test_statistics_table_sizes_fit_the_executors_arena_bound():
    """fc_conv_stats_blocks (pure host function) against the bound fcaf3d_amd/executor.py allocates a statistics table with:
    rows * (C / 8) * 4 + 8 * C + 256 bytes must hold blocks * 2 * C floats for every route and size (r5)."""
    from fcaf3d_amd.functional import CONV_X6 as X6
    for C in (64, 128, 256, 512):
        for n in (1, 15, 16, 17, 100, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 16384, 50000, 437248):
            for K, pairs in ((27, 0), (27, 1), (1, 0)):
                nb = L.query('fc_conv_stats_blocks', n, K, C, C, X6, pairs)
                assert nb > 0, (n, K, C, pairs)
                assert nb * 2 * C * 4 <= n * (C // 8) * 4 + 8 * C + 256, (n, K, C, pairs, nb)
                if n <= 4096:
                    assert nb <= 64, (n, nb)      # up to 4 096 rows: at most 64 row blocks -> the BatchNorm behind it is ONE launch
    assert L.query('fc_conv_stats_blocks', 1000, 27, 64, 64, 0, 0) == 0                # fp32 route: no statistics epilogue
    assert L.query('fc_conv_stats_blocks', 1000, 27, 3, 64, X6, 0) == 0                # stem shape: not an MFMA launch


# ---- the route queries (fc_conv_fwd_route / fc_conv_wgrad_route, csrc/conv_route.h) -------------------------------------------------

def _route_grid():
    """the shapes and flag words the size queries were compared on against the parent of the route refactor (profiles/r7_notes.md)"""
    import itertools
    import fcaf3d_amd.functional as Fn
    X6 = Fn.CONV_SPLIT | Fn.CONV_IMAGE
    n_out = (1, 50, 64, 65, 511, 512, 862, 3500, 4095, 4096, 6900, 14900, 32767, 32768, 55000, 64000, 98304, 262144, 441000, 580000)
    chans = ((3, 64), (64, 64), (64, 128), (128, 64), (128, 128), (256, 256), (512, 128), (48, 64), (64, 96))
    flags = (0, Fn.CONV_SPLIT, X6, Fn.CONV_FMA, X6 | Fn.CONV_FLAT, Fn.CONV_PIPE_ON, Fn.CONV_PIPE_OFF, Fn.CONV_GLDS, Fn.CONV_GLDS_OFF,
             Fn.CONV_WGRAD_MULTI_OFF, Fn.CONV_WGRAD_MULTI_FIRST, Fn.CONV_SPLIT | Fn.CONV_WGRAD_MULTI_OFF,
             1 << Fn.CONV_BM_SHIFT, 2 << Fn.CONV_BM_SHIFT, 3 << Fn.CONV_BM_SHIFT, 1 << Fn.CONV_BN_SHIFT, 2 << Fn.CONV_BN_SHIFT,
             5 << Fn.CONV_S_SHIFT)
    return itertools.product(n_out, (1, 8, 27), chans, flags)


def test_size_queries_agree_with_the_route_queries():
    """fc_conv_fwd_ws_bytes, fc_conv_stats_blocks and fc_conv_wgrad_ws_bytes are read off the route the launch will take: over the
    whole grid, in both split modes, they equal what fc_conv_fwd_route / fc_conv_wgrad_route report"""
    E = L.header_enums()
    l = L.lib()
    try:
        for mode in (0, 2):
            assert l.fc_set_split_mode(mode) == 0
            for n, K, (ci, co), f in _route_grid():
                _, r = L.route('fc_conv_fwd_route', n, n, K, ci, co, f, E['FC_TABLE_DENSE'], 0)
                assert l.fc_conv_fwd_ws_bytes(n, K, ci, co, f) == (r['s'] * n * co * 4 if r['s'] > 1 else 0), (mode, n, K, ci, co, f, r)
                assert (l.fc_conv_stats_blocks(n, K, ci, co, f, 0) > 0) == (r['epi'] != E['FC_EPI_NONE']), (mode, n, K, ci, co, f, r)
                _, rp = L.route('fc_conv_fwd_route', n, n, K, ci, co, f, E['FC_TABLE_PAIRS'], 0)
                assert (l.fc_conv_stats_blocks(n, K, ci, co, f, 1) > 0) == (rp['epi'] != E['FC_EPI_NONE']), (mode, n, K, ci, co, f, rp)
                splits = [w['s'] for rc, w in (L.route('fc_conv_wgrad_route', n, n, K, ci, co, f, E[t])
                                               for t in ('FC_TABLE_NONE', 'FC_TABLE_DENSE', 'FC_TABLE_PAIRS')) if rc == 0]
                assert l.fc_conv_wgrad_ws_bytes(n, K, ci, co, f) == max(splits) * K * ci * co * 4, (mode, n, K, ci, co, f, splits)
    finally:
        l.fc_set_split_mode(2)


def test_route_queries_refuse_what_the_launch_refuses():
    """fc_conv_fwd_route / fc_conv_wgrad_route return -1 exactly for the calls the entry points answer with -1"""
    import fcaf3d_amd.functional as Fn
    E = L.header_enums()
    X6 = Fn.CONV_SPLIT | Fn.CONV_IMAGE
    NONE, DENSE, SORTED, PAIRS, STATS = (E['FC_TABLE_' + k] for k in ('NONE', 'DENSE', 'SORTED', 'PAIRS', 'STATS'))
    fwd = lambda *a: L.route('fc_conv_fwd_route', *a)[0]
    wgrad = lambda *a: L.route('fc_conv_wgrad_route', *a)[0]
    n = 1000
    # transposed weights need a table
    assert fwd(n, n, 1, 64, 64, Fn.CONV_WT, NONE, 0) == -1 and fwd(n, n, 1, 64, 64, 0, NONE, 0) == 0
    assert fwd(n, n, 27, 64, 64, Fn.CONV_WT, DENSE, 0) == 0
    # a table-free launch is the identity map
    assert fwd(n, n, 27, 64, 64, 0, NONE, 0) == -1 and fwd(n + 1, n, 1, 64, 64, 0, NONE, 0) == -1
    assert wgrad(n, n, 27, 64, 64, 0, NONE) == -1 and wgrad(n, n, 1, 64, 64, 0, NONE) == 0
    # sorted-row tables and weight images are MFMA-path features
    for ci, f in ((48, 0), (64, Fn.CONV_FMA)):
        assert fwd(n, n, 27, ci, 64, f, DENSE, 0) == 0
        assert fwd(n, n, 27, ci, 64, f, SORTED, 0) == -1
        assert fwd(n, n, 27, ci, 64, f | X6, DENSE, 0) == -1
    assert fwd(n, n, 27, 64, 64, X6, SORTED, 0) == 0
    # statistics: the split route only
    assert fwd(n, n, 27, 64, 64, 0, DENSE | STATS, 0) == -1 and fwd(n, n, 27, 64, 64, 0, PAIRS | STATS, 0) == -1
    assert fwd(n, n, 27, 48, 64, X6, DENSE | STATS, 0) == -1 and fwd(n, n, 27, 3, 64, X6, DENSE | STATS, 0) == -1
    assert fwd(n, n, 27, 64, 64, X6, DENSE | STATS, 0) == 0 and fwd(n, n, 27, 64, 64, X6, PAIRS | STATS, 37) == 0
    # pair lists: MFMA shapes only
    assert fwd(n, n, 27, 48, 64, 0, PAIRS, 0) == -1 and fwd(n, n, 27, 64, 96, 0, PAIRS, 0) == -1 and fwd(n, n, 27, 32, 64, 0, PAIRS, 0) == 0
    assert wgrad(n, n, 27, 48, 64, 0, PAIRS) == -1 and wgrad(n, n, 27, 64, 64, Fn.CONV_FMA, PAIRS) == -1 and wgrad(n, n, 27, 64, 64, 0, PAIRS) == 0
    assert wgrad(n, n, 27, 64, 64, 0, SORTED) == -1          # (row_index of fc_conv_wgrad is reserved)
    assert L.route('fc_conv_fwd_route', n, n, 27, 48, 64, 0, PAIRS, 0)[1]['family'] == E['FC_FAM_INVALID']


# ---- the normalisation route queries (fc_bn_train_fwd_route / fc_bn_train_bwd_route, csrc/norm_route.h) ---------------------------------

NORM_N = (0, 1, 63, 64, 65, 872, 3500, 4096, 4097, 16383, 65536, 65537, 441000, 3000000)
NORM_C = (4, 8, 64, 128, 192, 256, 512, 1024)
NORM_NSEG = (1, 8, 64)


def test_norm_size_queries_agree_with_the_route_queries():
    """the grid the six norm size queries were compared on against the parent of the route refactor (profiles/r7_notes.md section 9):
    every route fc_bn_train_fwd / fc_bn_train_bwd can take of (n, C) fits fc_bn_train_ws_bytes(n, C), and each specific size query
    equals the workspace bytes of its entry point's route"""
    import itertools
    E = L.header_enums()
    TRAIN, SMALL, SEG = (E['FC_NFORM_' + k] for k in ('TRAIN', 'SMALL', 'SEG'))
    ALWAYS, NEVER = (1 << 63) - 1, -1                    # small_elems of fc_bn_act_train_fwd / of fc_bn_stats_train's statistics step
    fwd = lambda *a: L.route('fc_bn_train_fwd_route', *a)
    bwd = lambda *a: L.route('fc_bn_train_bwd_route', *a)
    l = L.lib()
    for n, C in itertools.product(NORM_N, NORM_C):
        bound = l.fc_bn_train_ws_bytes(n, C)
        assert bound == max(l.fc_bn_stats_ws_bytes(n, C), l.fc_norm_act_bwd_ws_bytes(n, C, 1), l.fc_bn_small_ws_bytes(C))
        for has_part, nb_part, small in itertools.product((0, 1), (1, 64, 65, 200), (0, 1 << 20)):
            for rc, r in (fwd(n, C, has_part, nb_part, 1, small), bwd(n, C, 1, has_part, nb_part, small, TRAIN)):
                assert rc == (0 if n >= 1 else -1), (n, C, has_part, nb_part, small)
                assert 0 <= r['ws_bytes'] <= bound, (n, C, has_part, nb_part, small, r, bound)
                assert (r['ws_bytes'] == 0) == (has_part == 1 or n < 1), (n, C, has_part, r)
        if n >= 1:
            # without a table: the small or the general route's bytes, which fc_bn_act_train_* / fc_bn_stats_train ask for by themselves
            assert fwd(n, C, 0, 0, 1, ALWAYS)[1]['ws_bytes'] == bwd(n, C, 1, 0, 0, ALWAYS, TRAIN)[1]['ws_bytes'] == l.fc_bn_small_ws_bytes(C)
            assert bwd(n, C, 1, 0, 0, 0, SMALL)[1]['ws_bytes'] == l.fc_bn_small_ws_bytes(C)
            assert fwd(n, C, 0, 0, 1, NEVER)[1]['ws_bytes'] == bwd(n, C, 1, 0, 0, 0, TRAIN)[1]['ws_bytes'] == l.fc_bn_stats_ws_bytes(n, C)
        for nseg in NORM_NSEG:
            rc, r = bwd(n, C, nseg, 0, 0, 0, SEG)
            assert rc == 0 and r['ws_bytes'] == l.fc_norm_act_bwd_ws_bytes(n, C, nseg) == l.fc_maxpool8_norm_act_bwd_ws_bytes(n, C, nseg), (n, C, nseg, r)
            # fc_col_stats: the same row blocks (cap 1024), 2 C sums + a count per block and segment
            assert l.fc_col_stats_ws_bytes(n, C, nseg) * 2 * C == l.fc_norm_act_bwd_ws_bytes(n, C, nseg) * (2 * C + 1)


def test_norm_route_queries_refuse_what_the_launch_refuses():
    """fc_bn_train_fwd_route / fc_bn_train_bwd_route return -1 exactly for the sizes the entry point answers with -1"""
    E = L.header_enums()
    TRAIN, SMALL, SEG = (E['FC_NFORM_' + k] for k in ('TRAIN', 'SMALL', 'SEG'))
    fwd = lambda *a: L.route('fc_bn_train_fwd_route', *a)[0]
    bwd = lambda *a: L.route('fc_bn_train_bwd_route', *a)[0]
    n = 1000
    for C, rc in ((0, -1), (3, -1), (4, 0), (6, -1), (66, -1), (1024, 0), (1028, -1), (2048, -1)):      # C < 4, C % 4, C > 1024
        for small in (0, 1 << 20):
            assert fwd(n, C, 0, 0, 1, small) == rc and fwd(n, C, 1, 10, 1, small) == rc, (C, small)
        for form in (TRAIN, SMALL, SEG):
            assert bwd(n, C, 1, 0, 0, 0, form) == rc, (form, C)
    assert fwd(0, 64, 0, 0, 1, 0) == -1 and fwd(-1, 64, 0, 0, 1, 0) == -1 and fwd(1, 64, 0, 0, 1, 0) == 0      # n < 1
    assert bwd(0, 64, 1, 0, 0, 0, TRAIN) == -1 and bwd(0, 64, 1, 0, 0, 0, SMALL) == -1 and bwd(1, 64, 1, 0, 0, 0, TRAIN) == 0
    # per-segment statistics (fc_norm_act_bwd, fc_maxpool8_norm_act_bwd): no rows is a call, 1..64 segments
    assert bwd(0, 64, 1, 0, 0, 0, SEG) == 0 and bwd(-1, 64, 1, 0, 0, 0, SEG) == -1
    assert bwd(n, 64, 0, 0, 0, 0, SEG) == -1 and bwd(n, 64, 64, 0, 0, 0, SEG) == 0 and bwd(n, 64, 65, 0, 0, 0, SEG) == -1
    assert bwd(n, 64, 2, 0, 0, 0, TRAIN) == -1                      # (one segment there)
    # a table: groups 1..64 (forward), at least one block
    for groups, rc in ((0, -1), (1, 0), (8, 0), (64, 0), (65, -1)):
        assert fwd(n, 64, 1, 10, groups, 0) == rc, groups
    assert fwd(n, 64, 0, 0, 0, 0) == 0                              # (no table: groups is not looked at)
    for nb_part, rc in ((-1, -1), (0, -1), (1, 0), (64, 0), (65, 0)):
        assert fwd(n, 64, 1, nb_part, 1, 0) == rc and bwd(n, 64, 1, 1, nb_part, 0, TRAIN) == rc, nb_part
    assert fwd(n, 64, 1, 0x7fffffff // 64 + 1, 1, 0) == -1
    assert bwd(n, 64, 1, 0, 0, 0, 3) == -1 and bwd(n, 64, 1, 0, 0, 0, -1) == -1                          # unknown forms
    assert L.route('fc_bn_train_fwd_route', n, 6, 0, 0, 1, 0)[1]['sums'] == E['FC_NSTATS_INVALID']
    assert L.route('fc_bn_train_bwd_route', n, 6, 1, 0, 0, 0, TRAIN)[1]['sums'] == E['FC_NRED_INVALID']
