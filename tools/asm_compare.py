#!/usr/bin/env python3
"""Compare the gfx950 machine code of two source trees kernel by kernel.

  asm_compare.py dump CSRC_DIR OUT_DIR      compile every .hip of CSRC_DIR with the Makefile's FLAGS plus
                                            --cuda-device-only -S into OUT_DIR/<file>.s (no GPU needed)
  asm_compare.py compare DIR_A DIR_B        cut both dumps per kernel symbol and compare, by symbol across all files
                                            (kernels may change files), each kernel's instruction text and its
                                            .amdhsa_ resource lines; local label numbers are normalised

Plain text processing: the comparison knows nothing about the instructions.  Exit status 1 if a kernel exists on one
side only or differs."""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys


def makefile_flags(csrc):
    text = open(os.path.join(csrc, 'Makefile')).read()
    m = re.search(r'^FLAGS\s*:=\s*(.*)$', text, re.M)
    return m.group(1).replace('$(EXTRA)', '').split()


def dump(csrc, out, jobs=8):
    csrc, out = os.path.abspath(csrc), os.path.abspath(out)
    os.makedirs(out, exist_ok=True)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    flags = makefile_flags(csrc)

    def one(src):
        dst = os.path.join(out, os.path.basename(src)[:-4] + '.s')
        subprocess.run([hipcc] + flags + ['--cuda-device-only', '-S', '-o', dst, src], check=True, cwd=csrc)
        return dst
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        for dst in ex.map(one, sorted(glob.glob(os.path.join(csrc, '*.hip')))):
            print('wrote', dst)


_LABEL = re.compile(r'\.L(BB|func_end|func_begin|tmp|JTI)\d+(_\d+)?')


def _norm(line, labels):
    """Local labels renumbered in order of appearance within the kernel; trailing comments dropped."""
    line = line.split(';')[0].rstrip()

    def sub(m):
        return labels.setdefault(m.group(0), '.L%d' % len(labels))
    return _LABEL.sub(sub, line)


def kernels(path):
    """symbol -> (instruction lines, resource lines) of every kernel in one .s file."""
    lines = open(path).read().split('\n')
    label = {l.split(';')[0].rstrip()[:-1]: i for i, l in enumerate(lines) if l[:1] not in ('', '\t', ' ', '.', ';')
             and l.split(';')[0].rstrip().endswith(':')}
    out = {}
    for k, l in enumerate(lines):
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', l)
        if not m:
            continue
        name = m.group(1)
        body, labels = [], {}
        for j in range(label[name] + 1, len(lines)):
            if re.match(r'\.Lfunc_end\d+:', lines[j]):
                break
            n = _norm(lines[j], labels)
            if n.strip():
                body.append(n)
        res = []
        for j in range(k + 1, len(lines)):
            if '.end_amdhsa_kernel' in lines[j]:
                break
            res.append(lines[j].strip())
        out[name] = (body, res)
    return out


def load(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, '*.s'))):
        for name, k in kernels(path).items():
            assert name not in out, 'kernel %s defined twice' % name
            out[name] = (os.path.basename(path),) + k
    return out


def _res(res, key):
    for l in res:
        p = l.split()
        if p[0] == key:
            return p[1]
    return '-'


def compare(da, db):
    a, b = load(da), load(db)
    same, moved, bad = 0, 0, []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            bad.append('%s: only in %s' % (name, da if name in a else db))
            continue
        (fa, ia, ra), (fb, ib, rb) = a[name], b[name]
        if ia == ib and ra == rb:
            same += 1
            moved += fa != fb
            continue
        keys = ('.amdhsa_next_free_vgpr', '.amdhsa_next_free_sgpr', '.amdhsa_private_segment_fixed_size',
                '.amdhsa_group_segment_fixed_size')
        bad.append('%s (%s -> %s): instructions %s (%d -> %d lines), resources %s; vgpr %s -> %s, sgpr %s -> %s, '
                   'scratch %s -> %s, lds %s -> %s' % ((name, fa, fb, 'same' if ia == ib else 'DIFFER', len(ia), len(ib),
                                                         'same' if ra == rb else 'DIFFER') +
                                                        tuple(v for k in keys for v in (_res(ra, k), _res(rb, k)))))
    print('kernels compared: %d (A %d, B %d)' % (len(set(a) | set(b)), len(a), len(b)))
    print('identical: %d (of which in another file: %d)' % (same, moved))
    print('differing or missing: %d' % len(bad))
    for l in bad:
        print('  ' + l)
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == 'dump':
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
