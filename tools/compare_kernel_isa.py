"""Are the kernels of two versions of a HIP source the same machine code?

Compiles both to gfx950 assembly (check_async_reads.compile_to_asm: the build's optimisation flags, device only), splits the assembly per
function, drops comments and assembler directives, renumbers the local labels (`.LBB<n>_<m>` carries the function's index, which shifts when
functions are added or removed) and compares function by function: the instructions and the `.amdhsa_*` lines of the kernel descriptor
(registers, LDS, scratch). For a refactor of host code, or one that removes kernels: every kept kernel must come out identical.
Usage: python tools/compare_kernel_isa.py OLD.hip|OLD.s [NEW.hip|NEW.s]     (NEW defaults to exorl_amd/csrc/gemm.hip; a .hip must sit next to
the headers it includes). Exit code 1 when a function present in both differs or one was added.
"""
import re
import sys
import tempfile
from pathlib import Path

from check_async_reads import ROOT, compile_to_asm, demangle

LABEL = re.compile(r'\.L(BB|tmp|func_begin|func_end)\d+')


def functions(path):
    """name -> (instruction and label lines, .amdhsa_* descriptor lines)"""
    body, desc, cur = {}, {}, None
    for line in open(path):
        t = line.split(';')[0].strip()
        m = re.match(r'^(_Z\w+):', t)
        if m:
            cur = body.setdefault(m.group(1), [])
        elif t.startswith('.Lfunc_end'):
            cur = None
        elif t.startswith('.amdhsa_kernel '):
            cur = desc.setdefault(t.split()[1], [])
        elif t == '.end_amdhsa_kernel':
            cur = None
        elif cur is not None and t and (not t.startswith('.') or t.endswith(':') or t.startswith('.amdhsa_')):
            cur.append(LABEL.sub(lambda m: '.L' + m.group(1), t))
    return {k: (v, desc.get(k, [])) for k, v in body.items()}


def assembly(arg, td, tag):
    p = Path(arg)
    if p.suffix == '.s':
        return p
    out = Path(td) / f'{tag}.s'
    compile_to_asm(p, out)
    return out


def main(old, new):
    with tempfile.TemporaryDirectory() as td:
        a, b = functions(assembly(old, td, 'old')), functions(assembly(new, td, 'new'))
    dm = demangle(sorted(set(a) | set(b)))
    gone, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    kept = [k for k in a if k in b]
    diff = [k for k in kept if a[k] != b[k]]
    print(f'{len(a)} functions in the old build, {len(b)} in the new')
    print(f'only in the old build: {len(gone)}')
    for k in gone:
        print('   ', dm[k])
    print(f'only in the new build: {len(added)}')
    for k in added:
        print('   ', dm[k])
    print(f'in both: {len(kept)} functions, {sum(len(a[k][0]) for k in kept)} instruction and label lines, '
          f'{sum(len(a[k][1]) for k in kept)} descriptor lines compared; different: {len(diff)}')
    for k in diff:
        print('   ', dm[k])
    return 1 if diff or added else 0


if __name__ == '__main__':
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ROOT / 'exorl_amd' / 'csrc' / 'gemm.hip'))
