#!/usr/bin/env python3
"""Is the device code of two source trees the same?  The check behind tests/test_host_logic.py DEVICE_IDENTICAL_SOURCES
(profiles/r7_notes.md): a change of csrc/ that is meant to leave every kernel as it is — host code, names, comments, code moved
between files or into shared inline helpers — is proven by comparing the compiler's device assembly, symbol by symbol.

    python tools/device_asm_diff.py OLD_TREE NEW_TREE [--only conv.hip ...] [--keep DIR]

OLD_TREE / NEW_TREE: two checkouts of this repository (e.g. `git archive <parent> | tar -x -C /some/dir` and `.`).  Every
fcaf3d_amd/csrc/*.hip and csrc_post/*.hip of either tree is compiled with that tree's build.FLAGS + build.FILE_FLAGS +
`--offload-device-only -S` into a temporary directory outside both trees (at most 4 compiles at a time); no GPU is needed.

The text is normalised (`__hip_cuid_*` lines and assembler comments dropped, the function's position taken out of its local labels)
and split by symbol, because moving a function changes the order of emission and nothing else.  Reported: symbols added, removed,
different (with a unified diff of the first different body per file), and the same for the kernel descriptors (`.amdhsa_kernel`
blocks).  Exit status 0 only if every symbol and every descriptor of every file is equal.

It compares text; it knows nothing about any instruction.
"""
import argparse
import difflib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

_LOCAL = re.compile(r'\.L(BB|JTI|func_begin|func_end|tmp)(\d+)(_\d+)?')
_TYPE = re.compile(r'\s*\.type\s+([^\s,]+),@(function|object)')
_SIZE = re.compile(r'\s*\.size\s+([^\s,]+),')
_KD = re.compile(r'\s*\.amdhsa_kernel\s+(\S+)')
_STRING = re.compile(r'\s*\.(ascii|asciz|string)\b')


def load_build(tree):
    """the tree's own fcaf3d_amd/build.py (its flags are part of what is compared)"""
    path = os.path.join(tree, 'fcaf3d_amd', 'build.py')
    spec = importlib.util.spec_from_file_location('fc_build_' + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_jobs(tree, out_dir, only=None):
    """{file name: hipcc command that writes its device assembly, the output path last}"""
    b = load_build(tree)
    os.makedirs(out_dir, exist_ok=True)
    return {s: [b.HIPCC] + b.FLAGS + b.FILE_FLAGS.get(s, []) + ['--offload-device-only', '-S', os.path.join(d, s), '-o', os.path.join(out_dir, s[:-4] + '.s')]
            for d, s in b._sources() if not only or s in only}


def run(cmd):
    print(' '.join(cmd), file=sys.stderr, flush=True)
    subprocess.check_call(cmd)


def normalise(line):
    if '__hip_cuid_' in line:
        return None
    if not _STRING.match(line):
        line = line.split(';', 1)[0]
    line = line.rstrip()
    if not line.strip():
        return None
    # .LBB<function number>_<block>: the function number is the function's position in the file
    return _LOCAL.sub(lambda m: '.L' + m.group(1) + (m.group(3) or ''), line)


def split_symbols(path):
    """({symbol: [lines]}, {kernel: [descriptor lines]}) of one assembly file"""
    syms, kds = {}, {}
    typed, cur, cur_name, kd = set(), None, None, None
    for raw in open(path, errors='replace'):
        line = normalise(raw)
        if line is None:
            continue
        if kd is not None:
            kds[kd].append(line)
            if line.strip() == '.end_amdhsa_kernel':
                kd = None
            continue
        m = _KD.match(line)
        if m:
            kd = m.group(1)
            kds[kd] = [line]
            continue
        m = _TYPE.match(line)
        if m:
            typed.add(m.group(1))
            continue
        if cur is None:
            name = line[:-1] if line.endswith(':') else None
            if name in typed:
                cur_name, cur = name, []
            continue
        m = _SIZE.match(line)
        if m and m.group(1) == cur_name:
            syms[cur_name] = cur
            cur = cur_name = None
            continue
        cur.append(line)
    if cur is not None:
        syms[cur_name] = cur
    return syms, kds


def compare(what, a, b, report):
    """number of names of `a` / `b` that are not equal on both sides"""
    added, removed = sorted(set(b) - set(a)), sorted(set(a) - set(b))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    for title, names in (('added', added), ('removed', removed), ('different', differ)):
        if names:
            report.append(f'  {what} {title}: {len(names)}')
            report.extend(f'    {n}' for n in names)
    if differ:
        n = differ[0]
        report.extend('    | ' + l.rstrip('\n') for l in difflib.unified_diff(a[n], b[n], 'old ' + n, 'new ' + n, n=2, lineterm=''))
    return len(added) + len(removed) + len(differ)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('old_tree')
    ap.add_argument('new_tree')
    ap.add_argument('--only', nargs='+', help='file names (conv.hip ...) instead of every .hip')
    ap.add_argument('--keep', help='leave the assembly in this directory (must lie outside both trees)')
    args = ap.parse_args()
    trees = [os.path.realpath(args.old_tree), os.path.realpath(args.new_tree)]
    work = os.path.realpath(args.keep) if args.keep else tempfile.mkdtemp(prefix='device_asm_diff_')
    for t in trees:
        if os.path.commonpath([t, work]) == t:
            sys.exit(f'the assembly would be written into {t}: give --keep a directory outside both trees')
    try:
        outs, jobs = [], []
        for side, t in zip(('old', 'new'), trees):
            j = compile_jobs(t, os.path.join(work, side), args.only)
            outs.append({s: cmd[-1] for s, cmd in j.items()})
            jobs += j.values()
        with ThreadPoolExecutor(max_workers=4) as ex:
            list(ex.map(run, jobs))
        bad = total = 0
        for s in sorted(set(outs[0]) | set(outs[1])):
            if s not in outs[0] or s not in outs[1]:
                print(f'{s}: only in the {"new" if s in outs[1] else "old"} tree')
                bad += 1
                continue
            (sa, ka), (sb, kb) = split_symbols(outs[0][s]), split_symbols(outs[1][s])
            report = []
            n = compare('symbols', sa, sb, report) + compare('kernel descriptors', ka, kb, report)
            bad += n
            total += len(set(sa) | set(sb))
            print(f'{s}: {len(sb)} symbols ({len(kb)} kernels), {sum(map(len, sb.values()))} lines compared: '
                  + ('equal' if not n else f'{n} NOT EQUAL'))
            print('\n'.join(report), end='\n' if report else '')
        print(f'{total} symbols compared: ' + ('device code is identical' if not bad else f'{bad} differences'))
        return 1 if bad else 0
    finally:
        if not args.keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
