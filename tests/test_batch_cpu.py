"""CPU: the sampler and the ragged indexing of csrc_post/batch.hip (fc_batch_augment_voxelize) without a GPU.

The sampler is restated here in numpy from the integer arithmetic documented at the head of batch.hip (32-bit wrapping words);
tools/batch_host_emu.cpp runs the kernel's own text on the host under AddressSanitizer and UBSan and must draw the same rows."""
import os

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
DESC_WORDS = 18


# ---- the documented arithmetic, in numpy (uint64 holding 32-bit words) -----------------------------------------------------------------
def mix(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13); x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x


def keys_of(seed):
    """seed: array of 64-bit seeds -> (4, len) round keys"""
    seed = np.atleast_1d(np.asarray(seed, np.uint64))
    lo, hi = seed & M32, seed >> np.uint64(32)
    return np.stack([mix(lo ^ mix((hi + np.uint64(((i + 1) * 0x9E3779B9) & 0xFFFFFFFF)) & M32)) for i in range(4)])


def half_bits(n):
    m = max(int(n - 1).bit_length(), 1)
    return (m + 1) // 2


def perm(j, n, key):
    """j: array of positions, key: (4,) or (4, len(j)) -> perm(j) in [0, n) (cycle walking); also the number of iterations"""
    h = np.uint64(half_bits(n))
    mask = (np.uint64(1) << h) - np.uint64(1)
    x = np.asarray(j, np.uint64).copy()
    key = np.asarray(key, np.uint64)
    key = key if key.ndim == 2 else np.repeat(key[:, None], len(x), 1)
    active = np.ones(len(x), bool)
    iters = 0
    while active.any():
        xa, ka = x[active], key[:, active]
        l, r = xa >> h, xa & mask
        for i in range(4):
            t = l ^ (mix(((r * np.uint64(0x9E3779B1)) & M32) + ka[i]) & mask)
            l, r = r, t
        x[active] = (l << h) | r
        iters += int(active.sum())
        active = x >= np.uint64(n)
    return x.astype(np.int64), iters


def draw(j, n, key):
    hsh = mix(mix(np.asarray(j, np.uint64) ^ key[0]) + key[1])
    return ((hsh * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def sample_rows(n_src, n_out, seed):
    """the rows scene (n_src, n_out, seed) reads, in output order"""
    key = keys_of(seed)[:, 0]
    j = np.arange(n_out)
    return perm(j, n_src, key)[0] if n_src >= n_out else draw(j, n_src, key)


# ---- the ragged batch both this file and tests/test_gpu_batch.py run ----------------------------------------------------------------------
N_SRC = (1, 255, 6000, 3000, 4097)
N_OUT = (1, 256, 4000, 4000, 4097)          # a one-row scene, with replacement (2), without, with replacement, an exact permutation
GAPS = (3, 0, 7, 1, 0, 5)                   # rows nobody writes: before scene 0, between the scenes, behind the last one


def xform(align=None, flip_h=False, flip_v=False, angle=0.0, scale=1.0, trans=(0.0, 0.0, 0.0)):
    x = np.zeros(24, np.float32)
    if align is not None:
        x[0:9], x[9:12], x[12] = np.asarray(align, np.float32)[:3, :3].reshape(-1), np.asarray(align, np.float32)[:3, 3], 1.0
    x[13], x[14] = float(flip_h), float(flip_v)
    x[15], x[16] = np.float32(np.cos(angle)), np.float32(np.sin(angle))
    x[17] = scale
    x[18:21] = trans
    return x


def make_batch(n_src=N_SRC, n_out=N_OUT, nfeat=3, gaps=GAPS, variant=0, seed=0):
    """-> dict(arena, desc (B,18) int64, xf (B,24), out_off, out_rows, total_out ...).  The four flip combinations are all present;
    `variant` swaps which scenes rotate, so the two variants together hold every flip / rotation combination; scene 2 is aligned."""
    rng = np.random.default_rng(100 + seed)
    B = len(n_src)
    arena = np.concatenate([np.concatenate([rng.uniform(-4, 4, (n, 3)), rng.integers(0, 256, (n, nfeat)).astype(np.float64)], 1)
                            for n in n_src]).astype(np.float32)
    a = 0.3
    align = np.array([[np.cos(a), -np.sin(a), 0, 0.5], [np.sin(a), np.cos(a), 0, -1.25], [0, 0, 1, 0.125], [0, 0, 0, 1]], np.float32)
    desc = np.zeros((B, DESC_WORDS), np.int64)
    xfs = np.zeros((B, 24), np.float32)
    src_off = np.cumsum((0,) + tuple(n_src))[:-1]
    out_off, o = [], gaps[0]
    for s in range(B):
        out_off.append(o)
        o += n_out[s] + gaps[min(s + 1, len(gaps) - 1)]
        rot = (s + variant) % 2 == 1
        xfs[s] = xform(align if s == 2 % B else None, flip_h=bool(s & 1), flip_v=bool(s & 2) or s == 4,
                       angle=(0.05 * (s + 1) if rot else 0.0), scale=0.9 + 0.04 * s, trans=rng.normal(0, 0.1, 3))
        desc[s, :6] = src_off[s], n_src[s], n_out[s], out_off[s], 0, 0
        desc[s, 4:5].view(np.uint64)[0] = (0x9E3779B97F4A7C15 * (s + 1) + seed) & 0xFFFFFFFFFFFFFFFF      # all 64 bits, sign bit too
        desc[s, 6:] = xfs[s].view(np.int64)
    return dict(arena=arena, desc=desc, xf=xfs, src_off=src_off, out_off=np.array(out_off), out_rows=o, total_out=sum(n_out),
                n_src=n_src, n_out=n_out, nfeat=nfeat, B=B)


def expected_rows(bt, sample_idx=None):
    """per scene, the source rows in output order"""
    if sample_idx is not None:
        return [sample_idx[int(bt['desc'][s, 5]):int(bt['desc'][s, 5]) + bt['n_out'][s]].astype(np.int64) for s in range(bt['B'])]
    return [sample_rows(bt['n_src'][s], bt['n_out'][s], bt['desc'][s, 4:5].view(np.uint64)[0]) for s in range(bt['B'])]


def restate(bt, rows, vs, feat_div):
    """k_augment_voxelize's arithmetic in numpy float32, one rounding per operation -> per scene (coords (n,4), feats, points)"""
    f = np.float32
    out = []
    for s in range(bt['B']):
        p = bt['arena'][bt['src_off'][s] + rows[s]]
        a = bt['xf'][s]
        x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
        if a[12] != 0:
            nx = (x * a[0] + y * a[1]) + z * a[2]
            ny = (x * a[3] + y * a[4]) + z * a[5]
            nz = (x * a[6] + y * a[7]) + z * a[8]
            x, y, z = nx + a[9], ny + a[10], nz + a[11]
        if a[13] != 0:
            x = -x
        if a[14] != 0:
            y = -y
        nx, ny = x * a[15] - y * a[16], x * a[16] + y * a[15]
        x, y, z = nx * a[17] + a[18], ny * a[17] + a[19], z * a[17] + a[20]
        assert x.dtype == np.float32
        cd = np.stack([np.full(len(x), s, np.int32)] + [np.floor(v / f(vs)).astype(np.int32) for v in (x, y, z)], 1)
        out.append((cd, p[:, 3:] / f(feat_div), np.concatenate([np.stack([x, y, z], 1), p[:, 3:]], 1)))
    return out


# ---- tests ---------------------------------------------------------------------------------------------------------------------------------
def test_permutation_is_a_bijection_and_the_walk_is_short():
    """n_out == n_src returns every row exactly once: powers of two, one above them (the longest walks: the domain is up to four
    times the set) and the degenerate sizes.  The mean number of Feistel evaluations per row stays under 4."""
    for n in (1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 4097, 100003):
        for seed in (0, 1, 0xDEADBEEFCAFEF00D):
            rows, iters = perm(np.arange(n), n, keys_of(seed)[:, 0])
            assert np.array_equal(np.sort(rows), np.arange(n)), (n, seed)
            assert iters < 4 * n + 8, (n, seed, iters / n)


def _subsets(n, k, S):
    """rows (S, k): the first k outputs for the seeds 0 .. S-1"""
    key = np.repeat(keys_of(np.arange(S, dtype=np.uint64)), k, 1)
    rows, _ = perm(np.tile(np.arange(k), S), n, key)
    return rows.reshape(S, k)


def test_sampling_without_replacement_is_uniform():
    """over seeds 0 .. S-1: every row is included equally often (chi-square over the rows, variance e (1 - k/n) of a
    hypergeometric inclusion count), neighbouring rows are not chosen together more or less often than independent subsets would,
    and the row in output position 0 is uniform.  The bounds catch a weak construction (three rounds: pair ratio 1.15)."""
    for n, k, S in ((1000, 100, 2000), (257, 64, 4000), (4097, 1000, 500)):
        rows = _subsets(n, k, S)
        assert all(len(set(r)) == k for r in rows[:50])
        cnt = np.bincount(rows.ravel(), minlength=n).astype(np.float64)
        e = S * k / n
        z_inc = (((cnt - e) ** 2).sum() / (e * (1 - k / n)) - (n - 1)) / np.sqrt(2 * (n - 1))
        chosen = np.zeros((S, n), bool)
        chosen[np.arange(S)[:, None], rows] = True
        pairs = (chosen[:, 1:] & chosen[:, :-1]).sum()
        ratio = pairs / (S * k * (k - 1) / n)
        c0 = np.bincount(rows[:, 0], minlength=n).astype(np.float64)
        e0 = S / n
        z_pos = (((c0 - e0) ** 2).sum() / e0 - (n - 1)) / np.sqrt(2 * (n - 1))
        print(f'n={n} k={k} S={S}: inclusion z {z_inc:+.2f}, adjacent-pair ratio {ratio:.4f}, position-0 z {z_pos:+.2f}')
        assert abs(z_inc) < 4, (n, k, S, z_inc)
        assert 0.95 < ratio < 1.05, (n, k, S, ratio)
        assert abs(z_pos) < 4, (n, k, S, z_pos)


def _build_emulator(tmp):
    """csrc_post/batch.hip from its BATCH_* constants to the end of its anonymous namespace, compiled for the host with
    AddressSanitizer and UBSan: the emulator restates nothing of the kernel"""
    import shutil
    import subprocess
    from fcaf3d_amd import build as B
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(B.CSRC_POST, 'batch.hip')).read()
    end = '}  // namespace'
    body = src[src.index('#define BATCH_THREADS'):src.index(end) + len(end)]
    assert '#include' not in body and '#define BATCH_DESC_WORDS 18' in body, 'batch.hip was reordered'
    (tmp / 'kernels.inc').write_text(body)
    cxx = os.path.join(os.path.dirname(os.path.dirname(B.HIPCC)), 'llvm', 'bin', 'clang++')
    cxx = cxx if os.path.exists(cxx) else shutil.which('clang++')
    exe = str(tmp / 'batch_host_emu')
    subprocess.check_call([cxx, '-std=c++20', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-pthread', f'-I{tmp}', os.path.join(root, 'tools', 'batch_host_emu.cpp'), '-o', exe])
    return exe


POISON_I, POISON_F = -77, np.float32(-12345.5)


def _emulate(exe, tmp, bt, vs, feat_div, sample_idx=None, total_out=None):
    import subprocess
    R, nf = bt['out_rows'], bt['nfeat']
    with open(tmp / 'in.bin', 'wb') as f:
        np.array([len(bt['arena']), 3 + nf, bt['B'], bt['total_out'] if total_out is None else total_out, R,
                  -1 if sample_idx is None else len(sample_idx), nf, 1], np.int64).tofile(f)
        np.array([vs, feat_div], np.float32).tofile(f)
        bt['arena'].tofile(f); bt['desc'].tofile(f)
        if sample_idx is not None:
            sample_idx.astype(np.int32).tofile(f)
        np.full(R * 4, POISON_I, np.int32).tofile(f); np.full(R * nf, POISON_F, np.float32).tofile(f)
        np.full(R, POISON_I, np.int32).tofile(f); np.full(R * (3 + nf), POISON_F, np.float32).tofile(f)
    r = subprocess.run([exe, str(tmp / 'in.bin'), str(tmp / 'out.bin')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    raw = np.fromfile(tmp / 'out.bin', np.int32)
    o = np.cumsum([0, R * 4, R * nf, R, R * (3 + nf)])
    return (raw[o[0]:o[1]].reshape(R, 4), raw[o[1]:o[2]].view(np.float32).reshape(R, nf), raw[o[2]:o[3]],
            raw[o[3]:o[4]].view(np.float32).reshape(R, 3 + nf))


def check_outputs(bt, rows, got, vs, feat_div, exact):
    """got = (coords, feats, sample_out, points_out) of all out_rows rows.  Rows outside every scene keep the poison; sample_out is
    `rows`; feats equal; coords equal the numpy restatement — exactly (`exact`), or but for rows within an ulp of a cell face, whose
    number is returned."""
    coords, feats, sample_out, points = got
    want = restate(bt, rows, vs, feat_div)
    live = np.zeros(bt['out_rows'], bool)
    near = 0
    for s in range(bt['B']):
        sl = slice(int(bt['out_off'][s]), int(bt['out_off'][s]) + bt['n_out'][s])
        live[sl] = True
        assert np.array_equal(sample_out[sl], rows[s]), s
        assert rows[s].min() >= 0 and rows[s].max() < bt['n_src'][s]
        assert np.array_equal(feats[sl].view(np.int32), want[s][1].view(np.int32)), s
        assert np.array_equal(coords[sl, 0], want[s][0][:, 0]), s
        bad = (coords[sl] != want[s][0]).any(1)
        if exact:
            assert not bad.any(), (s, int(bad.sum()))
            assert np.array_equal(points[sl].view(np.int32), want[s][2].view(np.int32)), s
        else:
            q = want[s][2][bad, :3].astype(np.float64) / vs
            assert (np.abs(q - np.round(q)) < 1e-4).all() and (np.abs(coords[sl][bad].astype(np.int64) - want[s][0][bad]) <= 1).all(), s
            near += int(bad.sum())
    assert (coords[~live] == POISON_I).all() and (sample_out[~live] == POISON_I).all()
    assert (feats[~live] == POISON_F).all() and (points[~live] == POISON_F).all()
    return near


def test_kernel_text_on_the_host_draws_the_documented_rows(tmp_path):
    """the kernel of csrc_post/batch.hip compiled for the host under AddressSanitizer and UBSan (a thread per GPU thread, a barrier
    for __syncthreads) on the ragged batch of the GPU test, both rotation variants, nfeat 0 with one scene, explicit indices, a
    host count smaller than the table's, and descriptors whose ranges leave the arrays (which must write nothing): no access leaves
    its array, the rows are the numpy sampler's, coords are the numpy restatement's but for rows within an ulp of a cell face."""
    exe = _build_emulator(tmp_path)
    vs, fd = 0.02, 255.0
    near = total = 0
    for variant in (0, 1):
        bt = make_batch(variant=variant)
        near += check_outputs(bt, expected_rows(bt), _emulate(exe, tmp_path, bt, vs, fd), vs, fd, exact=False)
        total += bt['total_out']
    one = make_batch(n_src=(700,), n_out=(300,), nfeat=0, gaps=(0, 2))
    near += check_outputs(one, expected_rows(one), _emulate(exe, tmp_path, one, vs, fd), vs, fd, exact=False)
    total += one['total_out']
    # explicit indices with per-scene offsets into one array (a gap in front of every scene's entries)
    bt = make_batch()
    rng = np.random.default_rng(5)
    idx, parts = 2, []
    for s in range(bt['B']):
        bt['desc'][s, 5] = idx
        parts.append((idx, rng.integers(0, bt['n_src'][s], bt['n_out'][s])))
        idx += bt['n_out'][s] + 3
    sample_idx = np.full(idx, 1 << 30, np.int32)
    for o, v in parts:
        sample_idx[o:o + len(v)] = v
    near += check_outputs(bt, expected_rows(bt, sample_idx), _emulate(exe, tmp_path, bt, vs, fd, sample_idx), vs, fd, exact=False)
    total += bt['total_out']
    print(f'rows within an ulp of a cell face (host libm / numpy): {near} of {total}')
    assert near < 1e-3 * total
    # descriptors that leave the arrays: the scene writes nothing, the others are as before (a small ragged batch)
    small = dict(n_src=(300, 40, 500, 9, 130), n_out=(200, 64, 500, 9, 130))
    ref = make_batch(**small)
    for word, value in ((0, len(ref['arena']) - 10), (3, ref['out_rows'] - 10), (1, 0), (2, -5), (0, -1), (1, 1 << 40)):
        bad = make_batch(**small)
        bad['desc'][2, word] = value
        coords, feats, sample_out, points = _emulate(exe, tmp_path, bad, vs, fd)
        sl = slice(int(ref['out_off'][2]), int(ref['out_off'][2]) + ref['n_out'][2])
        assert (coords[sl] == POISON_I).all() and (sample_out[sl] == POISON_I).all(), (word, value)
        for s in (0, 1, 3, 4):
            keep = slice(int(ref['out_off'][s]), int(ref['out_off'][s]) + ref['n_out'][s])
            assert np.array_equal(sample_out[keep], expected_rows(ref)[s]) and (coords[keep, 0] == s).all(), (word, value, s)


def test_einval_and_empty_batches_return_without_a_launch():
    """bad arguments are refused and empty batches accepted on the host, before any launch (no GPU needed: null pointers)"""
    from fcaf3d_amd import _lib as L
    fn = L.lib().fc_batch_augment_voxelize
    ok = dict(arena=16, arena_rows=10, pt_stride=6, desc=16, B=1, total_out=4, out_rows=4, sample_idx=None, n_idx=0, vs=0.02, fd=255.0,
              nfeat=3, coords=16, feats=16, sample_out=None, points_out=None, stream=None)

    def rc(**kw):
        a = dict(ok, **kw)
        return fn(*a.values())
    assert rc(B=0) == 0 and rc(total_out=0) == 0 and rc(B=0, arena=None, desc=None, coords=None, feats=None) == 0
    for kw in (dict(B=-1), dict(B=257), dict(total_out=-1), dict(total_out=5), dict(pt_stride=5), dict(nfeat=-1), dict(vs=0.0), dict(vs=-1.0),
               dict(arena=None), dict(desc=None), dict(coords=None), dict(feats=None), dict(sample_idx=16, n_idx=3), dict(arena_rows=-1),
               dict(out_rows=-1), dict(n_idx=-1)):
        assert rc(**kw) == -1, kw
