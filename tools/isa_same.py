#!/usr/bin/env python3
"""Are the kernels of two gfx950 .s files (hipcc --cuda-device-only -S of one unit, before and after a refactor) the same code?
Per .amdhsa_kernel of either file: the instruction text (comments and __hip_cuid_* lines dropped, the function index of
.LBB<f>_<n> / .Lfunc_end<f> renumbered) and the register and segment sizes.  A DIFFERENT line ends with what decides whether the new code
may cost occupancy: the VGPR allocation (next_free_vgpr rounded up to the granule of 8) and the wavefronts per SIMD it allows,
min(8, 512 // allocation), old -> new, and `resources ok` unless scratch, static LDS or the allocation's wavefronts got worse.
Exit status 1 on any difference."""
import hashlib
import re
import sys

FIELDS = ('next_free_vgpr', 'next_free_sgpr', 'private_segment_fixed_size', 'group_segment_fixed_size')


def kernels(path):
    lines = open(path).read().split('\n')
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', l)
        if not m:
            continue
        name = m.group(1)
        desc = '\n'.join(lines[i:lines.index('\t.end_amdhsa_kernel', i)])
        nums = tuple(int(re.search(r'\.amdhsa_%s\s+(\d+)' % f, desc).group(1)) for f in FIELDS)
        start = next(j for j in range(i, -1, -1) if lines[j].startswith(name + ':'))
        text = []
        for l in lines[start + 1:i]:
            l = re.sub(r'\.(LBB|Lfunc_end)\d+', r'.\1#', l.split(';')[0]).strip()
            if l and '__hip_cuid_' not in l:
                text.append(' '.join(l.split()))
        nins = sum(1 for l in text if not l.startswith('.') and not l.endswith(':'))
        out[name] = (nins, nums, hashlib.sha256('\n'.join(text).encode()).hexdigest()[:12])
    return out


def show(k):
    return 'ins %d vgpr %d sgpr %d private %d lds %d %s' % ((k[0],) + k[1] + (k[2],)) if k else 'missing'


def waves(k):
    alloc = (k[1][0] + 7) // 8 * 8
    return alloc, min(8, 512 // alloc)


def resources(a, b):
    if not a or not b:
        return ''
    (aa, wa), (ab, wb) = waves(a), waves(b)
    ok = b[1][2] <= a[1][2] and b[1][3] <= a[1][3] and wb >= wa
    return '  alloc %d -> %d waves %d -> %d  %s' % (aa, ab, wa, wb, 'resources ok' if ok else 'RESOURCES WORSE')


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
names = sorted(set(old) | set(new))
for name in names:
    a, b = old.get(name), new.get(name)
    print('%-9s %s  %s' % ('same', name, show(b)) if a == b else 'DIFFERENT %s  old: %s  new: %s%s' % (name, show(a), show(b), resources(a, b)))
sys.exit(any(old.get(n) != new.get(n) for n in names))
