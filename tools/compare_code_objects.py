"""Compares the gfx950 code objects of one translation unit from two builds kernel by kernel, for refactors of host code that reorder
template instantiations: the device code is the same, but the kernels sit in another order and the fat binaries differ.

    objcopy -O binary --only-section=.hip_fatbin UNIT.o UNIT.fatbin
    clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=UNIT.fatbin --output=UNIT.co --unbundle
    python tools/compare_code_objects.py PARENT/UNIT.co HEAD/UNIT.co

Per symbol name: the machine code of every function (the bytes of its symbol in .text) and the 64-byte kernel descriptor NAME.kd, which
holds the LDS and scratch sizes and the granulated VGPR / SGPR counts (compute_pgm_rsrc1..3); its kernel_code_entry_byte_offset (bytes
16..23) is the distance to the code and is left out.  Prints the counts and every symbol that differs; exit status 1 if any does.  Reads
the ELF files directly: needs no ROCm tool and no device."""
import struct
import sys


def symbols(path):
    """{name: bytes} of every function and object symbol with a size, the entry offset of kernel descriptors zeroed."""
    data = open(path, "rb").read()
    assert data[:6] == b"\x7fELF\x02\x01", f"{path}: not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]      # name, type, flags, addr, offset, size, link, ...
    out = {}
    for _, stype, _, _, off, size, link, _, _, entsize in sections:
        if stype != 2:      # SHT_SYMTAB
            continue
        stroff = sections[link][4]
        for k in range(size // entsize):
            name_off, info, _, shndx, value, ssize = struct.unpack_from("<IBBHQQ", data, off + k * entsize)
            if ssize == 0 or shndx == 0 or shndx >= shnum or (info & 15) not in (1, 2) or sections[shndx][1] == 8:      # OBJECT / FUNC with file bytes
                continue
            name = data[stroff + name_off:data.index(b"\0", stroff + name_off)].decode()
            start = sections[shndx][4] + value - sections[shndx][3]
            body = bytearray(data[start:start + ssize])
            if name.endswith(".kd") and ssize == 64:
                body[16:24] = bytes(8)
            out[name] = bytes(body)
    return out


def main():
    a, b = symbols(sys.argv[1]), symbols(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    kernels = sum(1 for n in a if n.endswith(".kd"))
    print(f"{len(a)} / {len(b)} symbols, {kernels} kernel descriptors, {sum(map(len, a.values()))} / {sum(map(len, b.values()))} bytes; "
          f"only in the first {len(only_a)}, only in the second {len(only_b)}, differing {len(differ)}")
    for n in only_a + only_b + differ:
        print("  ", n)
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main())
