"""Do two builds hold the same device code?  Compares the gfx950 code objects inside two objects / shared libraries kernel by
kernel - by symbol, not by file offset, so a changed instantiation order does not show: the set of kernel symbols, the resource
record of each (tools/kernel_meta.py) and its disassembled instructions (the ROCm llvm-objdump).

    python tools/kernel_diff.py before.o after.o        -> exit status 0 when nothing differs"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_meta  # noqa: E402

OBJDUMP = os.environ.get('LLVM_OBJDUMP', '/opt/rocm/lib/llvm/bin/llvm-objdump')
RESOURCES = ('vgpr_count', 'agpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
             'group_segment_fixed_size', 'max_flat_workgroup_size')


def functions(path):
    """symbol -> [instruction text + encoding, ...] of every function in the device ELFs of `path`"""
    out = {}
    for _, elf in kernel_meta._device_elfs(open(path, 'rb').read()):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(elf)
            f.flush()
            text = subprocess.run([OBJDUMP, '-d', f.name], capture_output=True, text=True, check=True).stdout
        name = None
        for line in text.splitlines():
            m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
            if m:
                name = m.group(1)
                out[name] = []
            elif name and line.strip():
                # "\tv_add ... // 000000001234: D1234567 ..." -> mnemonic + encoding words; the address goes
                out[name].append(re.sub(r'//\s*[0-9A-Fa-f]+:', '//', line.strip()))
    return out


def main(a, b):
    bad = 0
    ka, kb = ({k['name']: k for k in kernel_meta.kernels(p)} for p in (a, b))
    for name in sorted(set(ka) ^ set(kb)):
        print('only in %s: %s' % (a if name in ka else b, name))
        bad += 1
    fa, fb = functions(a), functions(b)
    for name in sorted(set(ka) & set(kb)):
        res = [(r, ka[name].get(r), kb[name].get(r)) for r in RESOURCES if ka[name].get(r) != kb[name].get(r)]
        if res or fa[name] != fb[name]:
            print('differs: %s %s%s' % (name, res, '' if fa[name] == fb[name] else ' instructions'))
            bad += 1
    print('%d / %d kernels, %d instructions compared, %d differ' % (len(ka), len(kb), sum(len(fa[n]) for n in ka if n in fa), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:3]))
