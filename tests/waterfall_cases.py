"""The cases of the record monitor (include/sgx.h: sgx_probe_waterfall), shared by tests/test_waterfall_host.py (the
contract against independent ground, sgx_waterfall_plan) and tests/test_waterfall_gpu.py (the kernels against the contract).
The smallest shapes at which the kernels can go wrong: the shortest and the longest segment, one in the middle and the one
below the LDS limit, each at no overlap, N/16, N/2 and N - 1; the three lengths between them (512, 2048, 4096) once each; slices of exactly one segment, of one segment and a tail that
counts in the moments only, a last slice that is partial but kept, a last piece that is dropped; more slices than the
statistics grid has workgroups (2048) and more segments than one scratch chunk holds (4096), with a slice cut by the chunk
boundary; odd offsets; extreme, constant and alternating contents.  Every record stays under 8 MB.  Test infrastructure."""
import collections
import zlib

import numpy as np

import waterfall_spec as spec

FS_MHZ = 38.192
Case = collections.namedtuple("Case", "name content offset n N noverlap S")

_OFFSETS = (0, 1, 3, 19)          # 19 = 3 mod 16


def _grid():
    out = []
    for a, N in enumerate((256, 1024, 8192, 16384)):
        for b, noverlap in enumerate((0, N // 16, N // 2, N - 1)):
            step = N - noverlap
            if b == 0:            # slices of exactly one segment; the last piece (N - 1 samples) is dropped
                S, n = N, 3 * N + N - 1
            elif b == 1:          # one segment and a tail; the last slice is partial, exactly one segment, and kept
                S = N + step - 1
                n = 2 * S + N
            else:                 # several segments and a tail; the last slice is partial with two segments and a tail
                S = N + 3 * step + 1
                n = 2 * S + N + step + (1 if step > 1 else 0)
            out.append(Case("grid-%d-%d" % (N, noverlap), "gauss", _OFFSETS[(a + b) % 4], n, N, noverlap, S))
    return out


CASES = _grid() + [
    # 16384 slices (the statistics grid has 2048 workgroups) and 16384 segments (a scratch chunk holds 4096)
    Case("many-slices", "gauss", 3, 4 * 1024 * 1024, 256, 0, 256),
    # 4 full slices of 1000 segments and a partial one of 200: the chunk boundary at segment 4096 cuts the last slice, and
    # a slice is several pieces of the statistics
    Case("chunk-cuts-slice", "gauss", 19, 4 * 256000 + 200 * 256 + 17, 256, 0, 256000),
    Case("all-min", "min", 1, 5000, 1024, 64, 2048),
    Case("all-max", "max", 0, 5000, 1024, 64, 2048),
    Case("constant", "const", 3, 5000, 1024, 512, 2048),
    Case("constant-16384", "const", 1, 2 * 16384 + 100, 16384, 1024, 16384 + 50),
    Case("alternating", "alt", 0, 5000, 1024, 0, 2048),
    Case("alternating-16384", "alt", 1, 2 * 16384, 16384, 1024, 16384),
    Case("late-tone", "tone", 0, 8 * 4096, 1024, 64, 4096),
] + [
    # the segment lengths the grid leaves out: 512 is the one pure radix-16 length below 8192 and runs with more lanes (64)
    # than radix-16 items (16), 2048 the one whose first step is the radix-4 step with no radix-2 step in front of it, 4096
    # the longest below the grid's 8192; each at noverlap = N / 16 with a tail and an odd offset.  Appended, so that the
    # cases above keep their names, offsets and seeds.
    Case("length-%d" % N, "gauss", offset, 2 * (2 * N - N // 16 + 7) + N + 5, N, N // 16, 2 * N - N // 16 + 7)
    for N, offset in ((512, 1), (2048, 3), (4096, 19))
]
BY_NAME = dict((c.name, c) for c in CASES)
TONE_BIN, TONE_AMPLITUDE = 100, 60
CONSTANT = 37

_RECORDS, _WANT = {}, {}


def record(c):
    """The int8 record of a case (read-only, made once): offset + n samples and 5 spare ones behind the window."""
    if c.name not in _RECORDS:
        total = c.offset + c.n + 5
        i = np.arange(total)
        if c.content == "gauss":
            rng = np.random.default_rng(zlib.crc32(c.name.encode()))
            x = np.clip(np.rint(rng.normal(0.0, 12.0, total)), -127, 127)
        elif c.content == "min":
            x = np.full(total, -128)
        elif c.content == "max":
            x = np.full(total, 127)
        elif c.content == "const":
            x = np.full(total, CONSTANT)
        elif c.content == "alt":
            x = np.where((i - c.offset) % 2 == 0, 127, -127)
        else:                     # a tone on a bin centre, in the second half of the window only
            x = np.where(i - c.offset >= c.n // 2, np.rint(TONE_AMPLITUDE * np.cos(2.0 * np.pi * TONE_BIN * i / c.N)), 0)
        _RECORDS[c.name] = x.astype(np.int8)
        _RECORDS[c.name].setflags(write=False)
    return _RECORDS[c.name]


def want(c):
    """The contract's answer for a case (computed once, read-only arrays)."""
    if c.name not in _WANT:
        w = spec.waterfall(record(c), c.offset, c.n, FS_MHZ, c.N, c.noverlap, c.S)
        for v in w.values():
            v.setflags(write=False)
        _WANT[c.name] = w
    return _WANT[c.name]
