"""numpy restatement of the block-wise front-end conditioning stage (include/sgx.h: sgx_cond_block_stats, sgx_cond_plan,
sgx_if_condition): the contract the host plan code and the HIP kernels (csrc/sgx_cond.hip) are tested against.  A record
of n elements - int8 (w = 1), offset-binary bytes (uint8: element = byte - 128) or little-endian int16 (w = 2) - holds
F = n / L frames of L lanes (L = 2: interleaved I/Q); blocks of B frames get a DC per lane, a gain and a blanking threshold
each, and the record comes out as n int8 bytes.  Everything is an integer but the plan, which is double arithmetic in the
order written here.  float32 records have no byte-exact contract (their sums are not order-free) and are refused.  Test
infrastructure, not product code."""
import math

import numpy as np

INT8 = np.dtype("i1")
UINT8 = np.dtype("u1")
INT16 = np.dtype("<i2")
BLOCK_MIN, BLOCK_MAX = 256, 16384
GUARD_MAX = 64
MAX_MULT, MAX_SHIFT = 32767, 30
DC_MAX = 1 << 20                     # |dc| a plan entry may carry, 1/16 LSB
INT64_MAX = (1 << 63) - 1
STATS_DTYPE = np.dtype([(k, "<i8") for k in ("n", "kept", "dc0", "dc1", "p_kept", "p_all", "e_max", "reserved")])
PLAN_DTYPE = np.dtype([("dc0", "<i4"), ("dc1", "<i4"), ("mult", "<i4"), ("shift", "<i4"), ("theta", "<i8")])
assert STATS_DTYPE.itemsize == 64 and PLAN_DTYPE.itemsize == 24


def width(dtype, offset_binary=False):
    """(bytes per element, offset binary) of a sample type the stage reads; uint8 IS offset binary."""
    dt = np.dtype(dtype)
    if dt == UINT8:
        return 1, True
    if dt == INT8:
        return 1, bool(offset_binary)
    if dt == INT16:
        if offset_binary:
            raise ValueError("offset binary is an 8-bit format, not int16")
        return 2, False
    raise ValueError("the conditioning stage reads int8, uint8 and int16 records, not %r" % (dtype,))


def check_record(n_bytes, dtype, lanes, block, blank_q4=0, offset_binary=False):
    """The preconditions of block_stats() and condition(); the library refuses what fails them with SGX_E_ARG.  Returns
    (w, n elements, F frames, K blocks)."""
    w, _ = width(dtype, offset_binary)
    if lanes not in (1, 2):
        raise ValueError("lanes must be 1 or 2")
    if not (BLOCK_MIN <= int(block) <= BLOCK_MAX) or int(block) % 16:
        raise ValueError("block must be a multiple of 16 in 256 .. 16384 frames")
    if not (blank_q4 == 0 or 16 <= int(blank_q4) <= 4096):
        raise ValueError("blank_q4 must be 0 or 16 .. 4096")
    if n_bytes % w or (n_bytes // w) % lanes:
        raise ValueError("a record of %d bytes does not hold whole frames of %d %d-byte elements" % (n_bytes, lanes, w))
    n = n_bytes // w
    F = n // lanes
    return w, n, F, -(-F // int(block))


def check_guard(guard):
    if not 0 <= int(guard) <= GUARD_MAX:
        raise ValueError("guard must be 0 .. 64 frames")


def check_plan(plan, K):
    p = np.asarray(plan)
    if p.dtype != PLAN_DTYPE or p.shape != (K,):
        raise ValueError("the plan must hold one entry per block (%d)" % K)
    if K and (p["mult"].min() < 1 or p["mult"].max() > MAX_MULT or p["shift"].min() < 0 or p["shift"].max() > MAX_SHIFT
              or max(np.abs(p["dc0"].astype(np.int64)).max(), np.abs(p["dc1"].astype(np.int64)).max()) > DC_MAX
              or p["theta"].min() < 0):
        raise ValueError("a plan entry is out of range: mult 1 .. 32767, shift 0 .. 30, |dc| <= 2^20, theta >= 0")


def frames(b, dtype, lanes, offset_binary=False):
    """int64[F, L]: the record's bytes (any array, only its bytes count) as frames of elements."""
    raw = np.ascontiguousarray(b).view(np.uint8).ravel()
    w, ob = width(dtype, offset_binary)
    if raw.size % (w * lanes):
        raise ValueError("a record of %d bytes does not hold whole frames of %d %d-byte elements" % (raw.size, lanes, w))
    if w == 2:
        x = raw.view(INT16).astype(np.int64)
    elif ob:
        x = raw.astype(np.int64) - 128
    else:
        x = raw.view(INT8).astype(np.int64)
    return x.reshape(-1, lanes)


def block_stats(b, dtype, lanes, block, blank_q4, offset_binary=False):
    """STATS_DTYPE[K]: per block n, kept (m_2), dc0, dc1 (1/16 LSB), p_kept (P_2), p_all (P_0), e_max, 0.
    S_l = sum of lane l; dc_l = (16 S_l + (n >> 1)) // n (floor); d_l = 16 x - dc_l; e = sum_l d_l^2; P_0 = sum e, m_0 = n;
    two rounds r = 1, 2: theta_r = ((P_{r-1} // m_{r-1}) blank_q4) >> 4, the frames with e <= theta_r are kept (m_r of
    them, P_r their sum); blank_q4 = 0 skips the rounds."""
    raw = np.ascontiguousarray(b).view(np.uint8).ravel()
    w, n, F, K = check_record(raw.size, dtype, lanes, block, blank_q4, offset_binary)
    x = frames(raw, dtype, lanes, offset_binary)
    out = np.zeros(K, dtype=STATS_DTYPE)
    for k in range(K):
        xb = x[k * block:min(F, (k + 1) * block)]
        nk = xb.shape[0]
        dc = [(16 * int(xb[:, l].sum()) + (nk >> 1)) // nk for l in range(lanes)]
        d = 16 * xb - np.array(dc, dtype=np.int64)
        assert np.abs(d).max() < 1 << 21
        e = (d * d).sum(axis=1)
        P, m = int(e.sum()), nk
        p_all = P
        if blank_q4:
            for _ in range(2):
                theta = ((P // m) * int(blank_q4)) >> 4
                keep = e <= theta
                m, P = int(np.count_nonzero(keep)), int(e[keep].sum())
                assert m >= 1
        out[k] = (nk, m, dc[0], dc[1] if lanes == 2 else 0, P, p_all, int(e.max()), 0)
    return out


def mult_shift(g):
    """(mult, shift) of a gain g > 0 by the rule of requant_spec.gain: shift = the largest S in 0 .. 30 with
    rint(g 2^S) <= 32767 (half to even), mult = max(1, rint(g 2^S)); if even S = 0 gives more: (32767, 0)."""
    for S in range(MAX_SHIFT, -1, -1):
        r = np.rint(math.ldexp(g, S))
        if r <= MAX_MULT:
            return max(1, int(r)), S
    return MAX_MULT, 0


def check_plan_args(lanes, blank_q4, target_rms, agc_blocks):
    if lanes not in (1, 2):
        raise ValueError("lanes must be 1 or 2")
    if not (blank_q4 == 0 or 16 <= int(blank_q4) <= 4096):
        raise ValueError("blank_q4 must be 0 or 16 .. 4096")
    if not (0.0 < target_rms <= 127.0):
        raise ValueError("target_rms must lie in (0, 127]")
    if not (agc_blocks >= 1.0 and math.isfinite(agc_blocks)):
        raise ValueError("agc_blocks must be finite and at least 1")


def plan(stats, lanes, blank_q4, target_rms, agc_blocks):
    """PLAN_DTYPE[K] from STATS_DTYPE[K], in doubles and in this order:
    v_k = p_kept / (kept L 256.0), D_lk = dc_l; alpha = 1 / agc_blocks; a_0 = v_0, a_k = a_{k-1} + alpha (v_k - a_{k-1}),
    A_lk alike from D_lk; g_k = target_rms / sqrt(a_k) (1 where a_k is not > 0); (mult, shift) = mult_shift(g_k);
    dc_l = rint(A_lk); theta = floor(a_k (16 L blank_q4)), INT64_MAX for blank_q4 = 0."""
    check_plan_args(lanes, blank_q4, target_rms, agc_blocks)
    st = np.asarray(stats)
    out = np.zeros(st.shape[0], dtype=PLAN_DTYPE)
    alpha = 1.0 / float(agc_blocks)
    a = A0 = A1 = 0.0
    for k in range(st.shape[0]):
        kept = int(st["kept"][k])
        if kept < 1:
            raise ValueError("block %d keeps no frame" % k)
        v = float(int(st["p_kept"][k])) / (float(kept) * float(lanes) * 256.0)
        D0, D1 = float(int(st["dc0"][k])), float(int(st["dc1"][k]))
        if k == 0:
            a, A0, A1 = v, D0, D1
        else:
            a = a + alpha * (v - a)
            A0 = A0 + alpha * (D0 - A0)
            A1 = A1 + alpha * (D1 - A1)
        g = float(target_rms) / math.sqrt(a) if a > 0.0 else 1.0
        mult, shift = mult_shift(g)
        theta = int(math.floor(a * float(16 * lanes * int(blank_q4)))) if blank_q4 else INT64_MAX
        out[k] = (int(np.rint(A0)), int(np.rint(A1)), mult, shift, theta)
    return out


def condition(b, dtype, lanes, block, plan, guard, offset_binary=False):
    """(y int8[n], blanked_frames, clipped).  d_l = 16 x - dc_l of the frame's block; hit[f] = sum_l d_l^2 > theta; a frame
    is blanked (all its elements 0) if a frame within `guard` of it is hit - across block boundaries, cut only by the ends
    of the record; any other element is clip((d mult + (1 << (shift + 3))) >> (shift + 4), -127, 127), floor shift.
    clipped counts the elements on +-127."""
    raw = np.ascontiguousarray(b).view(np.uint8).ravel()
    w, n, F, K = check_record(raw.size, dtype, lanes, block, 0, offset_binary)
    check_guard(guard)
    check_plan(plan, K)
    if F == 0:
        return np.zeros(0, dtype=np.int8), 0, 0
    x = frames(raw, dtype, lanes, offset_binary)
    p = np.asarray(plan)
    k = np.arange(F) // int(block)
    dc = np.stack([p["dc0"][k], p["dc1"][k]], axis=1)[:, :lanes].astype(np.int64)
    d = 16 * x - dc
    assert np.abs(d).max() < 1 << 21
    hit = (d * d).sum(axis=1) > p["theta"][k]
    G = int(guard)
    c = np.concatenate([[0], np.cumsum(hit)])
    idx = np.arange(F)
    blank = (c[np.minimum(F, idx + G + 1)] - c[np.maximum(0, idx - G)]) > 0
    sh = p["shift"][k].astype(np.int64)[:, None]
    y = (d * p["mult"][k].astype(np.int64)[:, None] + (np.int64(1) << (sh + 3))) >> (sh + 4)
    y = np.clip(y, -127, 127)
    y[blank] = 0
    return y.astype(np.int8).ravel(), int(np.count_nonzero(blank)), int(np.count_nonzero(np.abs(y) == 127))


def block_frames(sampling_freq, block_us):
    """Settings.condBlockUs as frames: that many microseconds at sampling_freq, to the nearest multiple of 16, in
    [256, 16384]."""
    b = 16 * int(np.rint(float(block_us) * 1e-6 * float(sampling_freq) / 16.0))
    return min(BLOCK_MAX, max(BLOCK_MIN, b))


def blank_q4_of(factor):
    """Settings.condBlankFactor c as blank_q4 = rint(16 c^2); 0 turns blanking off."""
    return int(np.rint(16.0 * float(factor) * float(factor)))
