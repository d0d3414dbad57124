"""The case table of the radix-pass tests (csrc/sgx_fft.hip: fft_pass_kernel<R, TPB, MODE>): code lengths chosen so that
every radix runs in every position a pass can take, and what tests/test_fft_cover_host.py and tests/test_fft_gpu.py share.
Nothing here restates the factoring rule or the workgroup widths: each case is what sgx_acquire_fft_passes reports for its
samplesPerCode (plan()).  Everything else is numpy from fixed seeds."""
import numpy as np

import any_rate
from conftest import pkg
from oracle import softgnss_oracle as orc

RADICES = [16, 8, 4, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31]

# samplesPerCode values that factor into 2..31.  Odd products put an odd radix first (15 015 = 3 5 7 11 13, 3 751 = 11^2 31,
# 4 199 = 13 17 19, 7 429 = 17 19 23, 12 673 = 19 23 29, 20 677 = 23 29 31, 26 071 = 29^2 31, 29 791 = 31^3); 8 008, 4 092
# and 10 230 put 8, 4 and 2 first; the powers of two and R 2^k put every radix last; 100 000, 98 304 and 131 072 need more
# than 64 workgroups in their last pass.
FACTORING = [15015, 5005, 17017, 3751, 4199, 7429, 12673, 20677, 26071, 29791, 8008, 4092, 10230,
             4096, 2048, 16384, 7168, 11264, 100000, 98304, 131072]
# samplesPerCode values with a prime factor above 31: the search runs on a padded length, one per last radix
# (48 257 -> 98 304 with 128 workgroups in the last pass, 50 177 -> 102 400 with 80)
PADDED = [2003, 15759, 7297, 3970, 48257, 50177, 3129, 4099, 3225, 2049, 2177, 2585, 3585, 3201]
LENGTHS = FACTORING + PADDED
MANY_BLOCKS = 64        # the partial maxima of a row once had this many slots

_PLANS = {}


class Case(object):
    """One samplesPerCode and the plan the library reports for it."""

    def __init__(self, n):
        p = pkg()._native.acquire_fft_passes(n)
        self.n = int(n)
        self.length = int(p["length"])
        self.radices = list(p["radices"])
        self.tpb = list(p["tpb"])
        self.blocks = int(p["last_pass_blocks"])
        self.padded = self.length != self.n
        self.first, self.last = self.radices[0], self.radices[-1]
        self.middle = self.radices[1:-1]
        self.ns_last = self.length // self.last          # stride of the last pass's outputs: thread j owns j + q ns_last
        self.tpb_last = self.tpb[-1]
        self.partial = self.ns_last % self.tpb_last != 0  # the last workgroup of the last pass has idle lanes

    def slots(self):
        """The last-pass output slots q = index // (length / R) that hold a code phase below n."""
        return list(range((self.n - 1) // self.ns_last + 1))


def plan(n):
    if n not in _PLANS:
        _PLANS[n] = Case(n)
    return _PLANS[n]


def coverage(lengths=None):
    """{position: set of radices} over the table: 'first', 'middle', 'last' (a length that factors: MODE 2) and
    'last_padded' (MODE 3)."""
    cov = dict(first=set(), middle=set(), last=set(), last_padded=set())
    for n in (LENGTHS if lengths is None else lengths):
        c = plan(n)
        cov["first"].add(c.first)
        cov["middle"].update(c.middle)
        cov["last_padded" if c.padded else "last"].add(c.last)
    return cov


# ---- reference transform: numpy's pocketfft on clongdouble (80-bit extended on x86: complex256) ----
def fft_long(x):
    return np.fft.fft(np.asarray(x, dtype=np.clongdouble), axis=-1)


def ifft_long(x):
    return np.fft.ifft(np.asarray(x, dtype=np.clongdouble), axis=-1)


def rel_err(got, want):
    """Normwise error per row: ||got - want||_2 / ||want||_2, in long double."""
    want = np.asarray(want, dtype=np.clongdouble)
    d = np.asarray(got, dtype=np.clongdouble) - want
    return np.asarray(np.sqrt(np.sum(np.abs(d) ** 2, axis=-1) / np.sum(np.abs(want) ** 2, axis=-1)), dtype=np.float64)


U = 2.0 ** -53
# one complex product (a real product pair and an FMA per part) and the rounding of a stored table entry, in units of u
_CMUL = 2.0 * np.sqrt(2.0)


def error_bound(radices, fused_first=False):
    """Worst-case normwise bound on the passes' rounding error, first order in u = 2^-53 (Higham, Accuracy and Stability
    of Numerical Algorithms, section 24.1, applied pass by pass: each pass is a unitary-scaled matrix product, so the
    relative errors of the passes add).  Per pass of radix R:
      * the butterfly: every output is an inner product of R terms whose coefficients are roots of unity rounded to
        double (1 u) - an R-term sum costs (R - 1) u, each coefficient product sqrt(8) u (odd radices: real FMAs on the
        folded halves, bounded by the same count; radix 16 / 8 / 4 / 2 by radix-4 / 2 butterflies with fewer roundings);
        together (R + 1 + sqrt(8)) u against sqrt(R) growth of the norm, i.e. at most that relative to the output norm;
      * the twiddle: the product of two table entries (each rounded: 1 u; their product sqrt(8) u), then the product
        with the data (sqrt(8) u): (2 + 2 sqrt(8)) u, absent in the first pass;
      * a fused first pass forms conj(X) F first: one more complex product, sqrt(8) u."""
    total = 0.0
    for i, r in enumerate(radices):
        total += r + 1.0 + _CMUL
        if i > 0:
            total += 2.0 + 2.0 * _CMUL
    if fused_first:
        total += _CMUL
    return total * U


# ---- plain-form inputs --------------------------------------------------------------------------------------------
def tail_lengths(c):
    """nonzero_len values of the zero-tailed rows: 1, around the first pass's stride n / R1, and n - 1."""
    m = c.length // c.first
    return [1, m - 1, m + 1, c.length - 1]


def plain_rows(c, seed):
    """(rows [k][length] complex128, nonzero_len) groups for the plain form: random rows; random rows under each zero tail
    (the hook takes the input as zero from nonzero_len on, so the rows passed keep garbage there and the reference
    zeroes it); a unit impulse in every residue class of the first radix; one pure tone per radix of the plan."""
    rng = np.random.default_rng(seed)
    L = c.length

    def rnd(k):
        return rng.standard_normal((k, L)) + 1j * rng.standard_normal((k, L))

    groups = [("random", rnd(3), L)]
    for t in tail_lengths(c):
        groups.append(("tail%d" % t, rnd(2), t))
    m = L // c.first
    imp = np.zeros((c.first, L), dtype=np.complex128)
    for q in range(c.first):
        imp[q, q * m + (7 * q + 3) % m] = 1.0 - 0.5j      # input j + q m: operand q of the first pass's butterfly
    groups.append(("impulse", imp, L))
    tones = []
    ns = 1
    for r in c.radices:
        # the bin that is 1 in this pass's output digit and 0 in every other: k = ns (Stockham: digit of weight ns)
        k = (ns * (r - 1)) % L
        tones.append(np.exp(2j * np.pi * ((k * np.arange(L, dtype=np.int64)) % L) / L))
        ns *= r
    groups.append(("tone", np.array(tones), L))
    return groups


# ---- fused-form inputs: rows built backwards from the wanted output ------------------------------------------------
def dominant_indices(c):
    """Output indices that take the maximum in turn, as (name, index, valid): every slot q of the last radix (in lanes
    and workgroups that vary with q), the first and last workgroup, lanes 0 and TPB - 1, the partial last workgroup
    and, on a padded length, n - 1; then those that must NOT win on a padded length."""
    ns, tpb, L, n = c.ns_last, c.tpb_last, c.length, c.n
    out = []
    for q in range(c.last):
        j = (q * 7919 + 13) % ns
        out.append(("slot%d" % q, q * ns + j))
    out.append(("first_wg_lane0", 0))
    out.append(("first_wg_last_lane", min(tpb, ns) - 1 + ns * (c.last // 2)))
    last_wg0 = ((ns - 1) // tpb) * tpb
    out.append(("last_wg_lane0", last_wg0 + ns * (c.last - 1)))
    out.append(("last_wg_last_live_lane", ns - 1))
    if c.padded:
        out.append(("n_valid-1", n - 1))
    return out


def backwards_rows(c, idx_list, seed, floor=0.25, also=()):
    """mul_x rows whose correlation with mul_f = 1 has its largest power at the given index: y = small random values
    plus 4 at the index (and 8 at the indices `also` gives for the same row: larger still, for places that must not be
    looked at); mul_x = conj(ifft(y)) in long double rounded to double, so that fft(conj(mul_x) * 1) = y."""
    rng = np.random.default_rng(seed)
    L = c.length
    y = floor * (rng.random((len(idx_list), L)) - 0.5 + 1j * (rng.random((len(idx_list), L)) - 0.5))
    for r, i in enumerate(idx_list):
        y[r, i] = 4.0 * np.exp(2j * np.pi * rng.random())
    for r, i in also:
        y[r, i] = 8.0 * np.exp(2j * np.pi * rng.random())
    x = np.conj(ifft_long(y)).astype(np.complex128)
    return x, y


def fused_reference(mul_x_rows, mul_f_rows, n_valid):
    """(max, arg, rows) of |fft(conj(X) F) / n|^2 over k < n_valid in long double, max rounded to double."""
    L = mul_x_rows.shape[-1]
    prod = np.conj(np.asarray(mul_x_rows, dtype=np.clongdouble)) * np.asarray(mul_f_rows, dtype=np.clongdouble)
    rows = fft_long(prod)
    pw = (np.abs(rows) / np.longdouble(L)) ** 2
    pw = pw[..., :n_valid]
    arg = np.argmax(pw, axis=-1)
    return np.max(pw, axis=-1).astype(np.float64), arg.astype(np.int64), rows


# ---- acquisition scenes: every slot of the last radix wins once ------------------------------------------------------
SATS_PER_SCENE = 8
GAP = any_rate.GAP
THRESHOLD_ROOM = any_rate.THRESHOLD_ROOM


def rate(n):
    """(samplingFreq, IF) of the front end with n samples per code: IF near a quarter of the rate, on the kHz grid."""
    return float(n) * 1000.0, float(round(n / 4.0)) * 1000.0


def slot_phase(c, q):
    """A code phase inside slot q of the last pass, below n, away from the slot's ends where it is wide enough."""
    spc = int(round(c.n * 1000.0 / 1.023e6))
    lo, hi = q * c.ns_last, min((q + 1) * c.ns_last, c.n)     # [lo, hi)
    pad = 2 * spc + 3
    if hi - lo <= 2 * pad + 1:
        return (lo + hi) // 2
    return lo + pad + (q * 7919 + 101) % (hi - lo - 2 * pad)


def scene_specs(c):
    """[(PRNs, Dopplers, code phases, amplitudes, seed)]: SATS_PER_SCENE satellites at most, one per slot."""
    slots = c.slots()
    out = []
    for i in range(0, len(slots), SATS_PER_SCENE):
        part = slots[i:i + SATS_PER_SCENE]
        prns = list(range(1, len(part) + 1))
        dop = [-3950.0 + 1100.0 * k + 35.0 * (i % 7) for k in range(len(part))]
        out.append((prns, dop, [slot_phase(c, q) for q in part], [8] * len(part), 0xFF7C0000 + c.n * 16 + i // SATS_PER_SCENE))
    return out


_SCENES = {}


def scene_records(n, ms=11):
    """[(prns, wanted code phases, record of `ms` code periods)] for samplesPerCode n."""
    if (n, ms) not in _SCENES:
        c = plan(n)
        synth = pkg("synth")
        fs, IF = rate(n)
        recs = []
        for prns, dop, phases, amps, seed in scene_specs(c):
            sc = synth.Scene.make(seed, fs, IF, prns, dop, [(p - 1) % n for p in phases], amps)
            recs.append((prns, phases, synth.generate(sc, ms * n)))
        _SCENES[(n, ms)] = recs
    return _SCENES[(n, ms)]


def oracle_settings(n, prns):
    fs, IF = rate(n)
    return orc.OracleSettings(samplingFreq=fs, IF=IF, acqSatelliteList=list(prns), numberOfChannels=2, msToProcess=11.0)


def settings(n, prns):
    fs, IF = rate(n)
    s = pkg().Settings()
    s.samplingFreq, s.IF = fs, IF
    s.acqSatelliteList = list(prns)
    s.numberOfChannels = 2
    s.msToProcess = 11.0
    return s


def winning_slots(c, ref, prns):
    """Slots of the last pass that hold a detection's code phase in oracle.acquire's result."""
    return {int(ref["codePhase"][p - 1]) // c.ns_last for p in prns if ref["carrFreq"][p - 1] > 0}


NONCOH_N = 100000      # the non-coherent route (acq_power_kernel) at a length with more than 64 last-pass workgroups
DEFERRED_N = 98304     # sgx_acquire_begin / sgx_acquire_end at one
