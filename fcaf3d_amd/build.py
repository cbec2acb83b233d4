"""Builds libfcaf3d_hip.so (gfx950) in-tree with hipcc.  No GPU needed (cross-compiles)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
# post-processing kernels that never run in the training step (test-time augmentation merge): compiled into the same library, kept
# out of csrc/ so that source_hash() — the hash every profile under profiles/ was taken on — does not cover them
CSRC_POST = os.path.join(HERE, 'csrc_post')
# the C ABI header: csrc/plan.hip returns its FC_ABI_VERSION, so every object depends on it (a stale object would report the old
# version and _lib.lib() would refuse the library)
ABI_HEADER = os.path.join(os.path.dirname(HERE), 'include', 'fcaf3d_hip.h')
LIB = os.path.join(HERE, 'libfcaf3d_hip.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['-O3', '-std=c++17', '--offload-arch=gfx950', '-fPIC', '-Wno-unused-result']
# r6: no SLP vectorisation in the MFMA kernels' files — the vectoriser packs the split arithmetic of adjacent channels into v_pk_mul_f32 /
# v_pk_fma_f32 / v_pk_add_f32, and beside MFMAs a packed fp32 instruction costs more than the two scalar ones it replaces
# (MI355X_MICROARCH.md "price of one filler beside MFMAs"): 454.9 / 453.8 -> 462.5 / 463.2 scenes/s (ABAB, one box), conv operator 93.2 -> 89.7 us
FILE_FLAGS = {'conv.hip': ['-fno-slp-vectorize'], 'norm.hip': ['-fno-slp-vectorize']}


def _sources():
    """(directory, file name) of every .hip the library is built from: csrc/ then csrc_post/, each in name order"""
    return [(d, f) for d in (CSRC, CSRC_POST) if os.path.isdir(d) for f in sorted(os.listdir(d)) if f.endswith('.hip')]


def _headers():
    return [os.path.join(d, f) for d in (CSRC, CSRC_POST) if os.path.isdir(d) for f in sorted(os.listdir(d)) if f.endswith('.h')] + [ABI_HEADER]


def source_hash():
    """sha256[:16] over the kernel sources (csrc/*.hip, csrc/*.h, in name order) — recorded with every profile under profiles/ and
    in bench.py's line, so that a committed kernel table can be told from one taken on other kernels
    (tests/test_host_logic.py::test_r5_profiles_were_taken_on_the_committed_kernels)"""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(('.hip', '.h')):
            h.update(f.encode())
            h.update(open(os.path.join(CSRC, f), 'rb').read())
    return h.hexdigest()[:16]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    hdrs = _headers()
    objs, jobs = [], []
    for d, s in _sources():
        src = os.path.join(d, s)
        obj = os.path.join(d, s[:-4] + '.o')
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            jobs.append([HIPCC] + FLAGS + FILE_FLAGS.get(s, []) + ['-c', src, '-o', obj])

    def run(cmd):
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs)
    return LIB


def build_tools(verbose=True):
    """tools/nbench (native conv micro-benchmark) and, with FC_TRACE kernels, tools/nbench_trace — diagnostics only."""
    root = os.path.dirname(HERE)
    tools = os.path.join(root, 'tools')
    inc = os.path.join(root, 'include')

    def run(cmd):
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)
    build(verbose=verbose)
    run([HIPCC, '-O2', '-std=c++17', '--offload-arch=gfx950', os.path.join(tools, 'nbench.cpp'), '-I' + inc, '-L' + HERE,
         '-lfcaf3d_hip', '-ldl', '-Wl,-rpath,$ORIGIN/../fcaf3d_amd', '-o', os.path.join(tools, 'nbench')])
    tdir = os.path.join(tools, 'trace')
    os.makedirs(tdir, exist_ok=True)
    objs = []
    for d, s in _sources():
        obj = os.path.join(tdir, s[:-4] + '.o')
        objs.append(obj)
        src = os.path.join(d, s)
        if _stale(obj, [src] + _headers()):
            run([HIPCC] + FLAGS + ['-DFC_TRACE', '-c', src, '-o', obj])
    tlib = os.path.join(tdir, 'libfcaf3d_hip.so')
    run([HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', tlib] + objs)
    run([HIPCC, '-O2', '-std=c++17', '--offload-arch=gfx950', os.path.join(tools, 'nbench.cpp'), '-I' + inc, '-L' + tdir, '-lfcaf3d_hip', '-ldl',
         '-Wl,-rpath,$ORIGIN/trace', '-o', os.path.join(tools, 'nbench_trace')])


if __name__ == '__main__':
    if '--tools' in sys.argv:
        build_tools()
    else:
        build(force='--force' in sys.argv)
    print(LIB)
