"""numpy restatement of the block-adaptive antenna combiner (include/sgx.h: sgx_array_block_stats, sgx_array_design_blocks,
sgx_if_combine_blocks), on top of tests/array_spec.py, whose record layout, lanes, A, K, flags, design steps and q() it
keeps: the statistics per block of B frames, the design of every block from the summed statistics of a window of blocks
with the hold rule for windows the design refuses, and the combiner whose OUTPUT frame f uses tap set f // B.  Integers
only where samples are touched; the design is array_spec.design itself.  Test infrastructure, not product code."""
import numpy as np

import array_spec as spec
from decim_spec import quantise

BLOCK_UNIT = 4096        # SGX_ARRAY_BLOCK_UNIT
MAX_BLOCKS = 1 << 20     # SGX_ARRAY_MAX_BLOCKS
MAX_WINDOW = 63          # SGX_ARRAY_MAX_WINDOW


def blocks_of(F, B):
    """n_blocks = ceil(F / B); ValueError for a B the library refuses, or more blocks than it takes."""
    B = int(B)
    if B < 1 or B % BLOCK_UNIT:
        raise ValueError("B must be a positive multiple of %d" % BLOCK_UNIT)
    n = -(-int(F) // B)
    if n > MAX_BLOCKS:
        raise ValueError("more than %d blocks" % MAX_BLOCKS)
    return n


def block_stats(b, lanes, A, K, B, flags=0):
    """int64 rho_blocks[n_blocks, A, A, K, lanes]: block j holds the terms of array_spec.stats whose x_b frame lies in
    [j B, min((j + 1) B, F)); the x_a[f + d] factor may lie in the next block, frames beyond F are zero."""
    b = np.ascontiguousarray(b)
    spec.check_shape(lanes, A, K, flags, b.size)
    x = spec.streams(b, lanes, A, flags)
    F = x.shape[0]
    nb = blocks_of(F, B)
    xp = np.concatenate([x, np.zeros((K, A, lanes), dtype=np.int64)])
    rho = np.zeros((nb, A, A, K, lanes), dtype=np.int64)
    for j in range(nb):
        f0, f1 = j * B, min((j + 1) * B, F)
        lag = xp[f0:f1]
        for d in range(K):
            lead = xp[f0 + d:f1 + d]
            if lanes == 1:
                rho[j, :, :, d, 0] = spec._dot(lead[:, :, 0], lag[:, :, 0])
            else:
                (ai, aq), (bi, bq) = (lead[:, :, 0], lead[:, :, 1]), (lag[:, :, 0], lag[:, :, 1])
                rho[j, :, :, d, 0] = spec._dot(ai, bi) + spec._dot(aq, bq)
                rho[j, :, :, d, 1] = spec._dot(aq, bi) - spec._dot(ai, bq)
    return rho


def window(j, n_blocks, W):
    """(lo, hi) of block j's window of W blocks."""
    h = (int(W) - 1) // 2
    return max(0, j - h), min(n_blocks, j + h + 1)


def design_blocks(rho_blocks, F, B, W, lanes, ref=0, loading=spec.DEFAULT_LOADING, target_rms=spec.DEFAULT_TARGET_RMS):
    """(taps int16[n_blocks, A, K] or [n_blocks, A, K, 2], shift, gain[n_blocks], suppression_db[n_blocks], weights
    [n_blocks, A, K], status uint8[n_blocks]).  Block j: array_spec.design of (the exact sum of the window's blocks,
    min(hi B, F) - lo B frames).  A window whose MATRIX the design refuses holds the nearest designed block before it, a
    leading one the first designed block, status 1; with no designed block at all, or any other refusal, ValueError."""
    rho_blocks = np.asarray(rho_blocks, dtype=np.int64)
    if rho_blocks.ndim != 5:
        raise ValueError("rho_blocks is [n_blocks, A, A, K, lanes]")
    nb = rho_blocks.shape[0]
    W, F, B = int(W), int(F), int(B)
    if not (1 <= W <= MAX_WINDOW and W % 2 == 1):
        raise ValueError("W must be odd, 1 .. %d" % MAX_WINDOW)
    if F < 1 or nb < 1 or blocks_of(F, B) != nb:
        raise ValueError("n_blocks must be ceil(F / B) >= 1")
    out = [None] * nb
    for j in range(nb):
        lo, hi = window(j, nb, W)
        rho = rho_blocks[lo:hi].sum(axis=0, dtype=np.int64)
        try:
            out[j] = spec.design(rho, min(hi * B, F) - lo * B, lanes, ref, loading, target_rms)
        except ValueError as e:
            if "positive definite" not in str(e):
                raise ValueError("block %d: %s" % (j, e))
    designed = [j for j in range(nb) if out[j] is not None]
    if not designed:
        raise ValueError("the covariance matrix is not positive definite")
    status = np.array([out[j] is None for j in range(nb)], dtype=np.uint8)
    src = designed[0]
    for j in range(nb):
        if out[j] is None:
            out[j] = out[src]
        else:
            src = j
    return (np.stack([o[0] for o in out]), spec.DESIGN_SHIFT, np.array([o[2] for o in out]), np.array([o[3] for o in out]),
            np.stack([o[4] for o in out]), status)


def check_blocks(taps, S, B, lanes, A, flags=0, n_bytes=0):
    """The preconditions of combine_blocks: array_spec.check for every block's taps, B, and one set per block."""
    taps = np.asarray(taps)
    if taps.ndim != (3 if int(lanes) == 1 else 4):
        raise ValueError("taps are [n_blocks, A, K] or, for I/Q, [n_blocks, A, K, 2]")
    spec.check_shape(lanes, A, taps.shape[2], flags, n_bytes)
    if blocks_of(int(n_bytes) // (int(A) * int(lanes)), B) != taps.shape[0]:
        raise ValueError("one set of taps per block")
    for j in range(taps.shape[0]):
        try:
            spec.check(taps[j], S, lanes, A, flags, n_bytes)
        except ValueError as e:
            raise ValueError("block %d: %s" % (j, e))


def block_sums(b, taps, B, lanes, A, flags=0, first=0, count=None):
    """The sums in front of the rounding of OUTPUT frames [first, first + count) (count None: to the end), int64 [count] or
    [count, 2]: frame f with tap set f // B, its inputs f + c - k wherever they lie, zero outside the record."""
    taps = np.asarray(taps)
    w = int(A) * int(lanes)
    F = np.asarray(b).size // w
    count = F - first if count is None else count
    c = (taps.shape[2] - 1) // 2
    parts = []
    j = first // B
    while j * B < first + count:
        f0, f1 = max(j * B, first), min((j + 1) * B, first + count)
        g0, g1 = max(f0 - c, 0), min(f1 + c, F)                    # the inputs the block's outputs reach
        s = spec.sums(b[g0 * w:g1 * w], taps[j], lanes, A, flags)
        parts.append(s[f0 - g0:f1 - g0])
        j += 1
    if not parts:
        return np.zeros((0,) if lanes == 1 else (0, 2), dtype=np.int64)
    return np.concatenate(parts)


def combine_blocks(b, taps, B, S, lanes, A, flags=0):
    """(int8 output bytes, clipped): array_spec.combine with tap set f // B for output frame f."""
    b = np.ascontiguousarray(b)
    taps = np.asarray(taps)
    assert b.dtype.itemsize == 1 and taps.dtype == np.int16
    check_blocks(taps, S, B, lanes, A, flags, b.size)
    y, over = quantise(block_sums(b, taps, B, lanes, A, flags), S)
    return y, int(np.count_nonzero(over))
