#!/usr/bin/env python3
"""Compares the kernels of two device-assembly listings instruction by instruction (comments, directives and label numbers
left out): the check that a change left the existing kernel instantiations as they were.  Needs no GPU.

    hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 --cuda-device-only -S rsik_lib.hip -o new.s   (in csrc/, each tree)
    python scripts/compare_kernel_asm.py parent.s new.s
"""
import re, sys, hashlib
def kernels(path):
    out = {}; name = None; buf = []
    for ln in open(path):
        m = re.match(r'^(_Z\w+):', ln)
        if m:
            name = m.group(1); buf = []; out[name] = buf; continue
        if name is None: continue
        if ln.startswith('.Lfunc_end') or ln.strip().startswith('.section') or ln.strip().startswith('.amdhsa'):
            name = None if ln.startswith('.Lfunc_end') or ln.strip().startswith('.section') else name
            continue
        s = ln.split(';')[0].strip()
        if not s or s.startswith('.') and not s.startswith('.LBB'): continue
        s = re.sub(r'\.LBB\d+_', '.LBB_', s)
        buf.append(s)
    return {k: hashlib.sha256('\n'.join(v).encode()).hexdigest()[:16] + f':{len(v)}' for k, v in out.items() if v}
a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
same = [k for k in a if k in b and a[k] == b[k]]
diff = [k for k in a if k in b and a[k] != b[k]]
print('parent kernels/functions', len(a), 'new', len(b), 'identical', len(same), 'different', len(diff), 'missing', [k for k in a if k not in b])
for k in diff: print('DIFF', k, a[k], b[k])
print('added', [k for k in b if k not in a])
