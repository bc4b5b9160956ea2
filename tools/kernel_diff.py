#!/usr/bin/env python3
"""Did a change touch the compiled kernels?  Compares the gfx950 code of two builds, object file by object file: the kernels only in A, only in B,
and those in both whose disassembly differs once addresses and encodings are stripped.  Exit status 1 if any kernel differs or exists only in B.
Usage: python tools/kernel_diff.py A B     (two directories holding the .o files of a build, e.g. a copy of csrc/ of the parent and csrc/ itself)"""
import os
import re
import subprocess
import sys
import tempfile

import kernel_resources as KR


def disassembly(path):
    """{symbol: [instruction text, ...]} of every function in the gfx950 code objects of `path`"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for d in KR.code_objects(path, tmp):
            asm = subprocess.run([os.path.join(KR.LLVM, 'llvm-objdump'), '-d', d], check=True, capture_output=True, text=True).stdout
            cur = None
            for ln in asm.splitlines():
                m = re.match(r'^[0-9a-f]+ <(.+)>:$', ln)
                if m:
                    cur = out.setdefault(m.group(1), [])
                elif cur is not None and ln.startswith(('\t', ' ')):
                    text = ln.split('//')[0].strip()            # the comment holds the address and the encoding
                    if text:
                        cur.append(text)
    return out


def main(a_dir, b_dir):
    bad = 0
    for obj in sorted({f for d in (a_dir, b_dir) for f in os.listdir(d) if f.endswith('.o')}):
        pa, pb = os.path.join(a_dir, obj), os.path.join(b_dir, obj)
        if not (os.path.isfile(pa) and os.path.isfile(pb)):
            print(f'{obj}: only in {a_dir if os.path.isfile(pa) else b_dir}')
            bad += 1
            continue
        a, b = disassembly(pa), disassembly(pb)
        only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
        print(f'{obj}: {len(a)} kernels in A, {len(b)} in B, {len(only_a)} only in A, {len(only_b)} only in B, {len(differ)} differ')
        for tag, names in (('only in A', only_a), ('only in B', only_b), ('DIFFERS', differ)):
            for n in KR.demangle(names):
                print(f'    {tag}: {n[:200]}')
        bad += len(only_b) + len(differ)
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
