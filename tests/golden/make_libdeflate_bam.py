"""Writes tests/golden/bamdec/libdeflate.{1,6,12}.bam: BAM files whose BGZF blocks were compressed by libdeflate (what current htslib / samtools builds use),
at three of its levels.  libdeflate emits what zlib never does - above all match distances up to 32,767 (zlib stops at 32,506) - so each file holds a long
record whose quality string repeats with a period of 32,700..32,767 bytes.  Needs libdeflate.so.0 (loaded through ctypes); run from the repository root:
    python tests/golden/make_libdeflate_bam.py
The committed files are decoded by both readers in tests/test_bamdec_streams_gpu.py."""
import ctypes
import os
import random
import struct
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import bamio  # noqa: E402
from test_bam_reader import NAMES, _records  # noqa: E402
from test_bamdec_gpu import _pattern_records  # noqa: E402


def main():
    lib = ctypes.CDLL("libdeflate.so.0")
    lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    lib.libdeflate_deflate_compress.restype = ctypes.c_size_t
    lib.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    out_dir = os.path.join(HERE, "bamdec")
    os.makedirs(out_dir, exist_ok=True)
    lens = [10_000_000] * len(NAMES)
    for k, level in enumerate((1, 6, 12)):
        rng = random.Random(100 + level)
        period = (32700, 32741, 32767)[k]
        unit = bytes(rng.randrange(42) for _ in range(period))
        n = 3 * period + 1000
        long = dict(qname=f"period{period}", flag=0, tid=0, pos=5000, mapq=60, cigar=[(20, 4), (n - 20, 0)], mtid=-1, mpos=-1, isize=0, seq="".join(rng.choice("ACGT") for _ in range(n)), qual=(unit * 4)[:n])
        recs = _records(900, 40 + level) + [long] + _pattern_records(500, 50 + level)
        text = "@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n_}\tLN:{l}\n" for n_, l in zip(NAMES, lens))
        raw = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(NAMES))
        for n_, l in zip(NAMES, lens):
            nb = n_.encode() + b"\0"
            raw += struct.pack("<i", len(nb)) + nb + struct.pack("<i", l)
        raw += b"".join(bamio.encode_record(r) for r in recs)
        comp = lib.libdeflate_alloc_compressor(level)
        buf = ctypes.create_string_buffer(70000)
        far = 0
        with open(os.path.join(out_dir, f"libdeflate.{level}.bam"), "wb") as f:
            for at in range(0, len(raw), 0xff00):
                data = raw[at:at + 0xff00]
                size = lib.libdeflate_deflate_compress(comp, data, len(data), buf, 65536 - 26)
                assert size, "the block did not fit"
                c = buf.raw[:size]
                assert zlib.decompressobj(-15).decompress(c) == data
                f.write(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, size + 25) + c + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))
            f.write(bamio.BGZF_EOF)
        lib.libdeflate_free_compressor(comp)
        print(f"libdeflate.{level}.bam: {os.path.getsize(os.path.join(out_dir, f'libdeflate.{level}.bam'))} bytes, period {period}")


if __name__ == "__main__":
    main()
