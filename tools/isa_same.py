#!/usr/bin/env python
"""Is the gfx950 device code of every csrc/*.hip what it was at a git revision?  (no GPU needed)

    python tools/isa_same.py <git-rev>

Each file of the revision and of the working tree is compiled with the flags of vit-adapter_amd/build.py plus
--offload-device-only -S; the lines naming the source file (.file), the compiler (.ident) and the hash symbol of the
compilation unit (__hip_cuid_) are dropped and the two texts compared as a whole.  Exit status 1 if any file differs; a file
that only one side has is listed as such and counts as different.
"""
import concurrent.futures
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'vit-adapter_amd'))
from build import CSRC, FLAGS, HIPCC, PER_FILE_FLAGS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(CSRC))
EXTRA = ['--offload-device-only', '-S']


def asm_sha(src):
    if not os.path.exists(src):
        return '-' * 64                                  # a file only one side has (added or removed since the revision)
    cmd = [HIPCC] + FLAGS + PER_FILE_FLAGS.get(os.path.basename(src), []) + EXTRA + [os.path.basename(src), '-o', '-']
    text = subprocess.run(cmd, cwd=os.path.dirname(src), check=True, capture_output=True, text=True).stdout
    kept = [ln for ln in text.split('\n') if not ln.lstrip().startswith(('.file', '.ident')) and '__hip_cuid_' not in ln]
    return hashlib.sha256('\n'.join(kept).encode()).hexdigest()


def main():
    rev = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', sys.argv[1]], text=True).strip()
    rel = os.path.relpath(CSRC, ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'include', rel], check=True, capture_output=True)
        subprocess.run(['tar', '-x', '-C', tmp], input=tar.stdout, check=True)
        old = os.path.join(tmp, rel)
        names = sorted({f for d in (old, CSRC) for f in os.listdir(d) if f.endswith('.hip')})
        with concurrent.futures.ThreadPoolExecutor(8) as pool:
            shas = list(pool.map(asm_sha, [os.path.join(d, n) for n in names for d in (old, CSRC)]))
    print('# %s %s <file> -o -' % (os.path.basename(HIPCC), ' '.join(FLAGS + EXTRA)))
    print('# added per file: %s' % ', '.join('%s %s' % (f, ' '.join(PER_FILE_FLAGS[f])) for f in sorted(PER_FILE_FLAGS)))
    print('# file, SHA-256 of the filtered assembly at %s, SHA-256 of this tree\'s' % rev)
    for i, n in enumerate(names):
        one_side = '-' * 64 in shas[2 * i:2 * i + 2]
        print('%-18s %s %s %s' % (n, shas[2 * i], shas[2 * i + 1],
                                  'ONE SIDE ONLY' if one_side else 'same' if shas[2 * i] == shas[2 * i + 1] else 'DIFFERENT'))
    return int(any(shas[2 * i] != shas[2 * i + 1] for i in range(len(names))))


if __name__ == '__main__':
    sys.exit(main())
