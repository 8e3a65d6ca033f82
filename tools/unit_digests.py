"""Digests of the code objects in a kernel cache: one line per unit and kernel, to compare two versions of the
kernel headers without a GPU.  A unit is named by the hash of its GENERATED source (which does not change with
the headers); the line gives sha256 prefixes of the .text section and of the constant data (every other
allocated section with contents; two fields of the kernel descriptors are masked: the kernarg size, reported on
its own, and the distance to the kernel's code, which moves with the length of the symbol the compiler derives
from the file's name), and each kernel's register counts, scratch and LDS bytes from the code object's notes.  Reads no
instruction.       usage: python tools/unit_digests.py [cache directory] > table.txt ; diff the two tables"""
import hashlib
import os
import struct
import sys


def elf_of(blob):
    """the gfx950 ELF inside a clang offload bundle (or the blob itself)"""
    if blob[:4] == b'\x7fELF':
        return blob
    assert blob[:24] == b'__CLANG_OFFLOAD_BUNDLE__', 'not a code object'
    n, at = struct.unpack_from('<Q', blob, 24)[0], 32
    for _ in range(n):
        off, size, tlen = struct.unpack_from('<QQQ', blob, at)
        triple = blob[at + 24:at + 24 + tlen]
        at += 24 + tlen
        if b'amdgcn' in triple:
            return blob[off:off + size]
    raise ValueError('no device image in the bundle')


def sections(elf):
    """[(name, type, flags, addr, offset, size, link, entsize)] of an ELF64 little-endian image"""
    shoff, = struct.unpack_from('<Q', elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from('<HHH', elf, 0x3A)
    raw = [struct.unpack_from('<IIQQQQIIQQ', elf, shoff + k * shentsize) for k in range(shnum)]
    names = elf[raw[shstrndx][4]:raw[shstrndx][4] + raw[shstrndx][5]]
    return [(names[r[0]:names.index(b'\0', r[0])].decode(), r[1], r[2], r[3], r[4], r[5], r[6], r[9]) for r in raw]


def unpack(b, i=0):
    """(value, next index) of the msgpack object at b[i] -- the subset the notes use"""
    t = b[i]
    if t <= 0x7f: return t, i + 1
    if t >= 0xe0: return t - 256, i + 1
    if 0xa0 <= t <= 0xbf: return b[i + 1:i + 1 + t - 0xa0].decode(), i + 1 + t - 0xa0
    if t in (0xc0, 0xc2, 0xc3): return {0xc0: None, 0xc2: False, 0xc3: True}[t], i + 1
    if t in (0xcc, 0xcd, 0xce, 0xcf):
        n = 1 << (t - 0xcc)
        return int.from_bytes(b[i + 1:i + 1 + n], 'big'), i + 1 + n
    if t in (0xd0, 0xd1, 0xd2, 0xd3):
        n = 1 << (t - 0xd0)
        return int.from_bytes(b[i + 1:i + 1 + n], 'big', signed=True), i + 1 + n
    if t in (0xd9, 0xda, 0xdb):
        n = 1 << (t - 0xd9)
        size = int.from_bytes(b[i + 1:i + 1 + n], 'big')
        return b[i + 1 + n:i + 1 + n + size].decode(), i + 1 + n + size
    if 0x90 <= t <= 0x9f or t in (0xdc, 0xdd) or 0x80 <= t <= 0x8f or t in (0xde, 0xdf):
        is_map = 0x80 <= t <= 0x8f or t in (0xde, 0xdf)
        if t in (0xdc, 0xde): count, i = int.from_bytes(b[i + 1:i + 3], 'big'), i + 3
        elif t in (0xdd, 0xdf): count, i = int.from_bytes(b[i + 1:i + 5], 'big'), i + 5
        else: count, i = t & 0x0f, i + 1
        items = []
        for _ in range(count * (2 if is_map else 1)):
            v, i = unpack(b, i)
            items.append(v)
        return (dict(zip(items[0::2], items[1::2])) if is_map else items), i
    raise ValueError('msgpack type 0x{:02x}'.format(t))


def digest_lines(path):
    with open(path, 'rb') as f:
        elf = elf_of(f.read())
    secs = sections(elf)
    body = {s[0]: bytearray(elf[s[4]:s[4] + s[5]]) for s in secs if s[1] == 1 and s[2] & 2}     # PROGBITS, allocated
    # kernel descriptors (<kernel>.kd, 64 bytes): bytes 8..11 are the kernarg size, 16..23 the offset of the code
    symtab = next(s for s in secs if s[1] == 2)
    strtab = secs[symtab[6]]
    names = elf[strtab[4]:strtab[4] + strtab[5]]
    for k in range(symtab[5] // symtab[7]):
        name, _, _, shndx, value, _ = struct.unpack_from('<IBBHQQ', elf, symtab[4] + k * symtab[7])
        if names[name:names.index(b'\0', name)].endswith(b'.kd'):
            sec = secs[shndx]
            at = value - sec[3]
            body[sec[0]][at + 8:at + 12] = bytes(4)
            body[sec[0]][at + 16:at + 24] = bytes(8)
    text = hashlib.sha256(bytes(body.pop('.text', b''))).hexdigest()[:16]
    const = hashlib.sha256(b''.join(n.encode() + bytes(body[n]) for n in sorted(body))).hexdigest()[:16]
    note = next(s for s in secs if s[1] == 7)
    namesz, descsz = struct.unpack_from('<II', elf, note[4])
    meta, _ = unpack(elf[note[4] + 12 + (namesz + 3) // 4 * 4:][:descsz])
    out = []
    for kern in sorted(meta['amdhsa.kernels'], key=lambda k: k['.name']):
        out.append('text {} const {} {} sgpr {} vgpr {} agpr {} scratch {} lds {} kernarg {}'.format(
            text, const, kern['.name'], kern['.sgpr_count'], kern['.vgpr_count'], kern.get('.agpr_count', 0),
            kern['.private_segment_fixed_size'], kern['.group_segment_fixed_size'], kern['.kernarg_segment_size']))
    return out


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    cache = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, '..', 'stodynprog_amd', '_kcache')
    rows = []
    for fn in sorted(os.listdir(cache)):
        if not fn.endswith('.hip') or not os.path.exists(os.path.join(cache, fn[:-4] + '.hsaco')):
            continue
        with open(os.path.join(cache, fn), 'rb') as f:
            unit = hashlib.sha256(f.read()).hexdigest()[:16]
        rows += ['unit {} {}'.format(unit, ln) for ln in digest_lines(os.path.join(cache, fn[:-4] + '.hsaco'))]
    print('\n'.join(sorted(rows)))
    print('# {} units, {} kernels'.format(len({r.split()[1] for r in rows}), len(rows)))


if __name__ == '__main__':
    main()
