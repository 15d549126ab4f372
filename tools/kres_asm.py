#!/usr/bin/env python
"""VGPRs, SGPRs, scratch, LDS, code size and occupancy of every kernel of one csrc/*.hip file, read from the assembly the
compiler writes (no GPU needed):

    kres_asm.py <file.hip> [substring]            one line per kernel
    kres_asm.py --diff <parent.hip> <file.hip>    kernels of both, matched by (mangled) name

Flags: those of profiles/r10_isa_identity.txt.  --diff also matches a kernel whose name differs from a parent's kernel by
ONE added template argument `false` (mangled Lb0E) - of the kernel or of a type among its arguments - with that kernel:
a new compile-time switch in its off position.  The remaining kernels of <file.hip> are listed as new, each beside its
twin with the switch off (Lb1E -> Lb0E) and marked when it has scratch or fewer waves per SIMD than that twin."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from isa_check import per_file_flags  # noqa: E402

FLAGS = ['-O3', '-std=c++17', '--offload-arch=gfx950', '-fPIC', '-Wall', '-Wno-unused-function', '-ffp-contract=fast',
         '--offload-device-only', '-S']
KEYS = (('vgpr', r'; NumVgprs: (\d+)'), ('agpr', r'; NumAgprs: (\d+)'), ('sgpr', r'; TotalNumSgprs: (\d+)'),
        ('scratch', r'; ScratchSize: (\d+)'), ('lds', r'; LDSByteSize: (\d+)'), ('code', r'; codeLenInByte = (\d+)'),
        ('occ', r'; Occupancy: (\d+)'))


def pretty(name):
    """Demangled name without namespaces and the parameter list.  binutils' c++filt does not know DF16b (__bf16) and
    DF16_ (_Float16): they go through it as double / long double, which no kernel here uses."""
    sub = name.replace('DF16b', 'd').replace('DF16_', 'e')
    dn = subprocess.run(['c++filt', sub], capture_output=True, text=True).stdout.strip()
    dn = dn.replace('long double', 'f16').replace('double', 'bf16')
    dn = re.sub(r'\(anonymous namespace\)::|vah::', '', dn)
    dn = re.sub(r'^void ', '', dn)
    return dn[:dn.rindex('>(') + 1] if '>(' in dn else re.sub(r'\(.*$', '', dn)


def kernels(src):
    """{mangled name: {key: int}} of the kernels of one source file."""
    src = os.path.abspath(src)
    cmd = ['/opt/rocm/bin/hipcc'] + FLAGS + per_file_flags(src) + [src, '-o', '-']
    asm = subprocess.run(cmd, capture_output=True, text=True, check=True, cwd='/tmp').stdout
    out = {}
    for name in re.findall(r'^\s*\.amdhsa_kernel (\S+)', asm, flags=re.M):
        # the figures are comments behind the kernel descriptor, `; Occupancy:` last
        body = re.search(r'\.amdhsa_kernel %s\n.*?; Occupancy: \d+' % re.escape(name), asm, flags=re.S).group(0)
        out[name] = {k: int(re.search(p, body).group(1)) for k, p in KEYS}
    return out


def fmt(r):
    return 'vgpr %3d agpr %3d sgpr %3d scratch %3d lds %5d code %6d occ %d' % tuple(r[k] for k, _ in KEYS)


def parent_of(name, old):
    """The parent's kernel of `name`: itself, or the one name that `name` becomes when one Lb0E is taken out."""
    if name in old:
        return name
    cands = {name[:m.start()] + name[m.end():] for m in re.finditer('Lb0E', name)} & set(old)
    return cands.pop() if len(cands) == 1 else None


if __name__ == '__main__':
    if sys.argv[1] == '--diff':
        old, new = kernels(sys.argv[2]), kernels(sys.argv[3])
        seen, differ, fresh = set(), 0, []
        for name, r in new.items():
            pn = parent_of(name, old)
            if pn is None:
                fresh.append(name)
                continue
            seen.add(pn)
            same = old[pn] == r
            differ += not same
            print('%-4s %s\n     %s' % ('same' if same else 'DIFF', pretty(name), fmt(r)))
            if not same:
                print('     %s   (parent)' % fmt(old[pn]))
        worse = 0
        for name in fresh:          # a switch in its on position: held against its twin with the switch off
            twins = {name[:m.start()] + 'Lb0E' + name[m.end():] for m in re.finditer('Lb1E', name)} & set(new)
            tw = new[twins.pop()] if len(twins) == 1 else None
            bad = tw is not None and (new[name]['scratch'] > 0 or new[name]['occ'] < tw['occ'])
            worse += bad
            print('new  %s\n     %s%s' % (pretty(name), fmt(new[name]), '' if tw is None else
                                          '   twin: vgpr %d occ %d%s' % (tw['vgpr'], tw['occ'], '  FEWER WAVES OR SCRATCH' if bad else '')))
        for name in old:
            if name not in seen:
                print('GONE %s' % pretty(name))
        print('# %d kernels of the parent, %d matched, %d differ, %d new, %d of them with scratch or fewer waves per SIMD than their twin'
              % (len(old), len(seen), differ, len(fresh), worse))
    else:
        pat = sys.argv[2] if len(sys.argv) > 2 else ''
        for name, r in kernels(sys.argv[1]).items():
            if pat in pretty(name):
                print('%-120s %s' % (pretty(name), fmt(r)))
