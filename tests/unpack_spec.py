"""numpy restatement of the unpacker (include/sgx.h: sgx_unpack_table, sgx_if_unpack): the contract the host table code and
the HIP kernel (csrc/sgx_unpack.hip) are tested against, and a pack() inverse with which the tests build packed files.
Integers only.  Test infrastructure, not product code."""
import numpy as np

BITS = (1, 2, 4)
FRAMES = (1, 2, 4, 8, 16)
LSB_FIRST = 1
SIGN_MAGNITUDE, OFFSET_BINARY, TWOS_COMPLEMENT = 0, 1, 2
ENCODINGS = {"sign-magnitude": SIGN_MAGNITUDE, "offset-binary": OFFSET_BINARY, "twos-complement": TWOS_COMPLEMENT}
DEFAULT_PEAK = 48            # Settings.packedPeak


def check(bits, flags=0, frame=1, first=0, take=1, n_bytes=0):
    """The preconditions of unpack(); the library refuses what fails them with SGX_E_ARG."""
    if bits not in BITS:
        raise ValueError("bits must be 1, 2 or 4")
    if int(flags) & ~LSB_FIRST:
        raise ValueError("unknown flag bits")
    if frame not in FRAMES:
        raise ValueError("frame must be 1, 2, 4, 8 or 16")
    if take < 1 or first < 0 or first + take > frame:
        raise ValueError("first, take must select fields of the frame")
    if (8 * int(n_bytes) // bits) % frame:
        raise ValueError("the fields must fill whole frames")


def codes(b, bits, flags=0):
    """int64[8N / bits]: the code of every field of the bytes b, field j in byte j bits // 8 at position p = j mod
    (8 / bits): (B >> (8 - bits (p + 1))) & (2^bits - 1), or with LSB_FIRST (B >> (bits p)) & (2^bits - 1)."""
    B = np.ascontiguousarray(b).view(np.uint8).astype(np.int64)
    per = 8 // bits
    p = np.arange(per, dtype=np.int64)
    sh = bits * p if int(flags) & LSB_FIRST else 8 - bits * (p + 1)
    return ((B[:, None] >> sh[None, :]) & ((1 << bits) - 1)).reshape(-1)


def selected(n_fields, frame=1, first=0, take=1):
    """The fields the stage takes, in output order: q frame + first + t."""
    q = np.arange(n_fields // frame, dtype=np.int64)
    return (q[:, None] * frame + first + np.arange(take, dtype=np.int64)[None, :]).reshape(-1)


def selected_codes(b, bits, flags=0, frame=1, first=0, take=1):
    b = np.ascontiguousarray(b)
    check(bits, flags, frame, first, take, b.size)
    c = codes(b, bits, flags)
    return c[selected(c.size, frame, first, take)]


def unpack(b, bits, table, flags=0, frame=1, first=0, take=1):
    """N bytes -> int8[(8N / bits / frame) take]: out[q take + t] = table[code(q frame + first + t)]."""
    t = np.asarray(table)
    assert t.size == 1 << bits and t.min() >= -128 and t.max() <= 127
    return t.astype(np.int8)[selected_codes(b, bits, flags, frame, first, take)]


def code_counts(b, bits, flags=0, frame=1, first=0, take=1):
    """int64[16]: how often each code occurs among the selected fields; entries 2^bits and above are 0."""
    return np.bincount(selected_codes(b, bits, flags, frame, first, take), minlength=16).astype(np.int64)


def pack(c, bits, flags=0):
    """uint8[len(c) bits / 8]: the bytes whose fields carry the codes c, the inverse of codes()."""
    c = np.asarray(c, dtype=np.int64)
    per = 8 // bits
    assert bits in BITS and c.size % per == 0 and (c.size == 0 or (c.min() >= 0 and c.max() < 1 << bits))
    p = np.arange(per, dtype=np.int64)
    sh = bits * p if int(flags) & LSB_FIRST else 8 - bits * (p + 1)
    return (c.reshape(-1, per) << sh[None, :]).sum(axis=1).astype(np.uint8)


def levels(bits, encoding):
    """int64[2^bits]: the symmetric odd level of every code."""
    c = np.arange(1 << bits, dtype=np.int64)
    if encoding == SIGN_MAGNITUDE:
        s, mu = c >> (bits - 1), c & ((1 << (bits - 1)) - 1)
        return (1 - 2 * s) * (2 * mu + 1)
    if encoding == OFFSET_BINARY:
        return 2 * c - ((1 << bits) - 1)
    if encoding == TWOS_COMPLEMENT:
        return 2 * np.where(c >= 1 << (bits - 1), c - (1 << bits), c) + 1
    raise ValueError("unknown encoding")


def table(bits, encoding=SIGN_MAGNITUDE, peak=DEFAULT_PEAK):
    """int8[2^bits]: levels times peak // (2^bits - 1); peak in 2^bits - 1 .. 127."""
    if bits not in BITS:
        raise ValueError("bits must be 1, 2 or 4")
    lv = levels(bits, encoding)
    if not ((1 << bits) - 1 <= int(peak) <= 127):
        raise ValueError("peak must lie in 2^bits - 1 .. 127")
    return (lv * (int(peak) // ((1 << bits) - 1))).astype(np.int8)


def code_of_level(bits, encoding):
    """int64[2^bits]: entry (level + 2^bits - 1) / 2 is the code that carries that level - levels()'s inverse, for
    building files from quantised samples."""
    lv = levels(bits, encoding)
    inv = np.zeros(1 << bits, dtype=np.int64)
    inv[(lv + (1 << bits) - 1) // 2] = np.arange(1 << bits)
    return inv
