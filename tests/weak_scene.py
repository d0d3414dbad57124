"""int8 records of weak satellites in Gaussian noise, generated in numpy (test infrastructure for the coherent acquisition).

Each satellite is A code(t) bit(t) cos(2 pi (IF + doppler) t + phase0) with the code Doppler of its carrier Doppler and
random 20-ms navigation bits.  With noise sigma, a real carrier of amplitude A has C/N0 = A^2 fs / (4 sigma^2)."""
import numpy as np

from oracle import softgnss_oracle as orc

FS = 38192000.0
IF = 9548000.0
L1 = 1575.42e6
CHIP_RATE = 1.023e6
SIGMA = 30.0

# (PRN index, C/N0 dB-Hz, Doppler Hz, sample at which a code period starts at t = 0)
WEAK_SATS = ((1, 33.0, -2730.0, 6113), (6, 33.5, 1415.0, 30011), (11, 34.0, 2210.0, 17420),
             (16, 33.0, -880.0, 24990), (22, 33.5, 390.0, 11877), (28, 34.0, -1660.0, 35002))


def amplitude(cn0_dbhz, sigma=SIGMA, fs=FS):
    return np.sqrt(4.0 * sigma ** 2 * 10.0 ** (cn0_dbhz / 10.0) / fs)


def code_drift_samples(doppler, ms, fs=FS):
    """How far the code-period start moves over `ms` ms (samples; negative = earlier)."""
    return -doppler / L1 * ms * 1e-3 * fs


def generate(ms, sats=WEAK_SATS, seed=20261016, sigma=SIGMA, fs=FS, if_=IF, chunk=1 << 21, nav_bits=True):
    """`sats` rows may carry a fifth entry (first ms, last ms): the satellite is on from sample round(first ms) up to round(last ms) only (the
    random draws do not depend on it).  nav_bits=False: no data-bit flips (the draws are made all the same)."""
    n_total = int(round(ms * 1e-3 * fs))
    rng = np.random.default_rng(seed)
    on = {row[0]: row[4] for row in sats if len(row) > 4 and row[4] is not None}
    sats = tuple(tuple(row[:4]) for row in sats)
    codes = {p: orc.generate_ca_code(p).astype(np.float64) for p, _, _, _ in sats}
    bits = {p: rng.choice([-1.0, 1.0], size=int(ms) // 20 + 3) for p, _, _, _ in sats}
    if not nav_bits:
        bits = {p: np.ones_like(b) for p, b in bits.items()}
    bit_off = {p: rng.uniform(0.0, 20.0) for p, _, _, _ in sats}
    ph0 = {p: rng.uniform(0.0, 2 * np.pi) for p, _, _, _ in sats}
    out = np.empty(n_total, dtype=np.int8)
    for start in range(0, n_total, chunk):
        idx = np.arange(start, min(start + chunk, n_total), dtype=np.float64)
        t = idx / fs
        y = rng.standard_normal(idx.size) * sigma
        for p, cn0, dop, s0 in sats:
            fc = CHIP_RATE * (1.0 + dop / L1)
            chip = np.floor((idx - s0) / fs * fc).astype(np.int64) % 1023
            bit = bits[p][np.floor((t * 1e3 + bit_off[p]) / 20.0).astype(np.int64)]
            sig = amplitude(cn0, sigma, fs) * codes[p][chip] * bit * np.cos(2 * np.pi * (if_ + dop) * t + ph0[p])
            if p in on:
                sig *= (idx >= round(on[p][0] * 1e-3 * fs)) & (idx < round(on[p][1] * 1e-3 * fs))
            y += sig
        out[start:start + idx.size] = np.clip(np.round(y), -128, 127).astype(np.int8)
    return out
