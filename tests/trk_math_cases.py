"""Operands and references for the arithmetic of the tracking chain (csrc/sgx_trk_math.h, csrc/sgx_trk_common.h), shared
by tests/test_trk_math_host.py (the host compilation, sgx_trk_math_eval_batch) and tests/test_trk_math_gpu.py (the device
compilation, sgx_trk_math_eval_device).  Everything here is numpy from fixed seeds: IEEE fp64 (correctly rounded /, sqrt,
ceil) for what must be EQUAL, np.longdouble to screen and mpmath at 50 digits to bound what may differ by a few ulp."""
import math

import numpy as np

# every sampling rate the suite tracks at (tests/any_rate.py: SMOOTH_IN_USE's rates and RATES), in Hz
FS = [38192000.0, 16367600.0, 5456000.0, 4092000.0, 61380000.0, 60000000.0, 26000000.0, 20460000.0, 12276000.0,
      53000000.0, 37000000.0, 5714000.0, 4099000.0]
SPACINGS = [0.25, 0.4, 0.5]
CODE_BASIS, CODE_LEN = 1.023e6, 1023.0
CF_DEV = 60.0                 # Hz: how far the code NCO is taken from the basis
LIM = 65536                   # the longest block any launch provides: n_units * unit = 16 * 4096 = 32 * 2048 samples
ATAN_SHORT_MAX = 0.25         # csrc/sgx_trk_math.h: SGX_ATAN_SHORT_MAX

# the ulp bounds of tests/test_cabi_and_host.py, by fn of include/sgx.h (sin / cos and the rotation: 2^-53 absolute)
BOUNDS = {"rcp": 1.0, "fast_div": 1.5, "fast_sqrt": 1.0, "atan_ratio": 2.5, "sincos_turns_short": 4.0, "div1": 1.5,
          "sqrt1": 1.0, "atan_ratio_k": 2.5, "rot_small": 2.0, "sqrt1_pos": 1.0, "sincos_turns": 4.0}
FN = {"rcp": 0, "fast_div": 1, "fast_sqrt": 2, "atan_ratio": 3, "sincos_turns_short": 4, "ceil_div": 5, "div1": 6,
      "sqrt1": 7, "atan_ratio_k": 8, "rot_small": 9, "block_length": 10, "sqrt1_pos": 11, "sgx_div_rn": 12,
      "block_length_inv": 13, "div_rn": 16, "sincos_turns": 17, "ramp_setup": 18, "prep_blk": 20, "prep_E": 21,
      "prep_P": 22, "prep_L": 23, "prep_inv": 24}


def n_code(fs):
    """samplesPerCode (initialize.py:185)"""
    return int(round(fs / (CODE_BASIS / CODE_LEN)))


def nb_base(fs):
    """csrc/sgx_trk.hip: trk_const - the first of the eight block lengths whose reciprocal the kernels keep"""
    return n_code(fs) - 3


def nudge(x, k):
    """x moved k representable numbers up (k < 0: down), elementwise"""
    x = np.array(x, dtype=np.float64)
    k = np.broadcast_to(np.asarray(k), x.shape)
    for _ in range(int(np.abs(k).max(initial=0))):
        up = np.nextafter(x, np.inf)
        dn = np.nextafter(x, -np.inf)
        x = np.where(k > 0, up, np.where(k < 0, dn, x))
        k = k - np.sign(k)
    return x


def bits_equal(a, b):
    """elementwise: the same bits, or both NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def first_mismatch(got, want, **operands):
    """None, or a text that names the first element where got and want differ in a bit, with its operands"""
    bad = np.flatnonzero(~bits_equal(got, want))
    if bad.size == 0:
        return None
    i = int(bad[0])
    ops = ", ".join("%s = %r" % (k, float(np.asarray(v)[i])) for k, v in operands.items())
    return "%d of %d differ; first at element %d: got %r, want %r (%s)" % (bad.size, np.size(got), i, float(np.asarray(got)[i]),
                                                                       float(np.asarray(want)[i]), ops)


# ---- the reference's block arithmetic restated elementwise (tracking.py:148-190, as oracle/softgnss_oracle.py: ramps(),
# step() have it; np.linspace(start, stop, blk, endpoint=False) is arange(blk) * ((stop - start) / blk) + start) ----
def prep_reference(cf, rem, fs, spacing):
    cf, rem = np.asarray(cf, dtype=np.float64), np.asarray(rem, dtype=np.float64)
    step = cf / fs
    blk = np.ceil((CODE_LEN - rem) / step)
    end = blk * step + rem
    out = {"step": step, "blk": blk}
    for arm, start, stop in (("E", rem - spacing, end - spacing), ("P", rem, end), ("L", rem + spacing, end + spacing)):
        out["start" + arm] = start
        out["d" + arm] = stop - start
        out["step" + arm] = (stop - start) / blk
    out["remCode"] = (((blk - 1.0) * out["stepP"] + rem) + step) - CODE_LEN
    return out


def prep_operands(fs, n, seed, wide=0.3):
    """(codeFreq, rem): blocks as tracking meets them - the NCO within CF_DEV of the basis, rem in [0, step) - and, for
    the share `wide`, rem up to 12 samples either way, which takes the block length out of the eight precomputed ones"""
    rng = np.random.default_rng(seed)
    cf = CODE_BASIS + rng.uniform(-CF_DEV, CF_DEV, n)
    step = cf / fs
    rem = rng.uniform(0.0, 1.0, n) * step
    w = rng.random(n) < wide
    rem = np.where(w, rng.uniform(-12.0, 12.0, n) * step, rem)
    cf[0], rem[0] = CODE_BASIS, 0.0     # block 0
    return cf, rem


# ---- div_rn: (a, b, y = RN(1 / b)) by divisor class --------------------------------------------------------------------
def div_rn_operands(per_divisor=1500, per_block_length=150, seed=7):
    """dict class -> (a, b): b = pi; b = every fs (a: code frequencies, and every block length within 60 of fs / 1000);
    b = each of the eight block lengths of every rate (a: 1023 +- 2e-3, and the spans dE, dP, dL prep_code forms)"""
    rng = np.random.default_rng(seed)
    out = {}
    a = rng.uniform(-0.25, 0.25, per_divisor) * rng.choice([1.0, 1e-3, 1e-7], per_divisor)
    out["pi"] = (a, np.full(per_divisor, math.pi))
    a_cf, b_cf, a_blk, b_blk, a_nb, b_nb, a_sp, b_sp = [], [], [], [], [], [], [], []
    for fs in FS:
        a_cf.append(CODE_BASIS + rng.uniform(-CF_DEV, CF_DEV, per_divisor))
        b_cf.append(np.full(per_divisor, fs))
        n = n_code(fs)
        a_blk.append(np.arange(n - 60, n + 61, dtype=np.float64))
        b_blk.append(np.full(121, fs))
        for nb in range(nb_base(fs), nb_base(fs) + 8):
            a_nb.append(CODE_LEN + rng.uniform(-2e-3, 2e-3, per_block_length))
            b_nb.append(np.full(per_block_length, float(nb)))
            # a block of exactly nb samples: (1023 - rem) / step = nb - u, 0 < u < 1
            m = per_block_length // 3
            rem = rng.uniform(0.0, 1.0, m) * (CODE_BASIS / fs)
            step = (CODE_LEN - rem) / (nb - rng.uniform(0.02, 0.98, m))
            for spc in SPACINGS:
                r = prep_reference(step * fs, rem, fs, spc)
                keep = r["blk"] == nb
                for arm in "EPL":
                    a_sp.append(r["d" + arm][keep])
                    b_sp.append(np.full(int(keep.sum()), float(nb)))
    out["code_freq_over_fs"] = (np.concatenate(a_cf), np.concatenate(b_cf))
    out["blk_over_fs"] = (np.concatenate(a_blk), np.concatenate(b_blk))
    out["1023_over_blk"] = (np.concatenate(a_nb), np.concatenate(b_nb))
    out["span_over_blk"] = (np.concatenate(a_sp), np.concatenate(b_sp))
    return out


# ---- block length ----------------------------------------------------------------------------------------------------------
def block_length_operands(per_rate, seed):
    """(a, codeFreq, fs) over every rate.  A quarter as tests/test_cabi_and_host.py builds its near-integer quotients
    (a = n step moved 0 .. 4 numbers either way, n within 200 of the nominal length); the code frequency up to CF_DEV from
    the basis (half uniform, half sigma = 5 Hz); block 0 of every rate first."""
    rng = np.random.default_rng(seed)
    aa, cc, ff = [], [], []
    for fs in FS:
        n = per_rate
        cf = CODE_BASIS + np.where(rng.random(n) < 0.5, rng.uniform(-CF_DEV, CF_DEV, n), rng.normal(0.0, 5.0, n))
        step = cf / fs
        a = CODE_LEN - rng.uniform(-0.05, 0.05, n)
        real = rng.random(n) < 0.5
        a = np.where(real, CODE_LEN - rng.uniform(0.0, 1.0, n) * step, a)       # rem in [0, step), as tracking has it
        q = n // 4 + 1
        k = rng.integers(n_code(fs) - 200, n_code(fs) + 201, q).astype(np.float64)
        a[:q] = nudge(k * step[:q], rng.integers(-4, 5, q))
        a[0], cf[0] = CODE_LEN, CODE_BASIS
        aa.append(a)
        cc.append(cf)
        ff.append(np.full(n, fs))
    return np.concatenate(aa), np.concatenate(cc), np.concatenate(ff)


# ---- ramp_setup ------------------------------------------------------------------------------------------------------------
def ramp_operands(per_ramp, seed):
    """(start, ramp step, code step, ilo, fs, near): the E / P / L ramps of prep_reference at every rate and spacing.  For `near`
    (at least a quarter) the start is moved so that one t(i*) = fl(fl(i* step) + start), i* in the chip
    that starts at ilo or the next, is an integer or within 4 ulp of one."""
    rng = np.random.default_rng(seed)
    S, T, C, I, F, NEAR = [], [], [], [], [], []
    for fs in FS:
        for spc in SPACINGS:
            cf, rem = prep_operands(fs, per_ramp, int(rng.integers(1 << 30)), wide=0.0)
            r = prep_reference(cf, rem, fs, spc)
            blk = r["blk"]
            per_chip = int(math.ceil(fs / CODE_BASIS))
            for arm in "EPL":
                start, step = r["start" + arm].copy(), r["step" + arm]
                ilo = np.floor(rng.random(per_ramp) * blk)
                edge = rng.random(per_ramp) < 0.05
                ilo = np.where(edge, np.where(rng.random(per_ramp) < 0.5, 0.0, blk - 1.0), ilo)
                near = rng.random(per_ramp) < 0.4
                i_star = np.minimum(ilo + rng.integers(0, per_chip + 2, per_ramp), blk + 2.0)
                p = i_star * step
                k = np.round(p + start)
                exact = k - p                                         # t(i*) == k with this start
                moved = exact + rng.integers(-4, 5, per_ramp) * np.spacing(k) * rng.choice([0.5, 1.0], per_ramp)
                start = np.where(near, moved, start)
                S.append(start)
                T.append(step)
                C.append(r["step"])
                I.append(ilo)
                F.append(np.full(per_ramp, fs))
                NEAR.append(near)
    return tuple(np.concatenate(x) for x in (S, T, C, I, F, NEAR))


def ramp_reference(start, step, ilo, fs):
    """(k1, isw) by brute force: t(i) = float64(i) * step + start (two roundings), k1 = ceil(t(ilo)), isw = the first i
    with t(i) > k1, searched sample by sample from ilo (t does not decrease) over a chip and four samples"""
    k1, isw = np.zeros(start.size), np.zeros(start.size)
    for f in np.unique(fs):
        m = fs == f
        window = int(math.ceil(f / CODE_BASIS)) + 4
        i = ilo[m][:, None] + np.arange(window, dtype=np.float64)[None, :]
        t = i * step[m][:, None] + start[m][:, None]
        k = np.ceil(t[:, 0]) + 0.0          # (+ 0.0: ceil of a t in (-1, 0) is -0.0, the kernels' k1 is an int)
        above = t > k[:, None]
        assert above.any(axis=1).all(), "the window holds every switch"
        k1[m], isw[m] = k, ilo[m] + np.argmax(above, axis=1)
    return k1, isw


# ---- ulp errors --------------------------------------------------------------------------------------------------------------
HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63
N_WORST, N_RANDOM, N_NO_SCREEN = 2000, 2000, 20000


def ulp_unit(exact):
    """2^(e - 53) for exact in [2^(e-1), 2^e): the unit tests/test_cabi_and_host.py measures in (numpy arrays of any float)"""
    return np.ldexp(1.0, np.frexp(np.asarray(exact, dtype=np.float64))[1] - 53)


def select(err_screen, rng):
    """indices to evaluate exactly: the N_WORST largest screened errors and N_RANDOM others - or, without a long double
    wider than fp64, N_NO_SCREEN random ones"""
    n = err_screen.size
    if not HAVE_LONGDOUBLE:
        return rng.choice(n, min(n, N_NO_SCREEN), replace=False)
    worst = np.argsort(np.nan_to_num(err_screen, nan=np.inf))[-N_WORST:]
    return np.unique(np.concatenate([worst, rng.choice(n, min(n, N_RANDOM), replace=False)]))


def worst_error(got, idx, exact_of, absolute=False):
    """(largest error over idx, its index): |got - exact| in ulps of exact (absolute: in units of 2^-53), exact_of(i) an
    mpmath number at 50 digits"""
    import mpmath as mp
    mp.mp.dps = 50
    worst, at = 0.0, -1
    for i in idx:
        i = int(i)
        ex = exact_of(i)
        e = abs(mp.mpf(float(got[i])) - ex)
        if absolute:
            u = e * 2 ** 53
        elif ex == 0:
            u = abs(float(got[i]))
        else:
            u = e / (mp.mpf(2) ** (math.frexp(float(ex))[1] - 53))
        u = float(u)
        if u != u:
            return math.inf, i   # a NaN where a number is due
        if u > worst or at < 0:
            worst, at = u, i
    return worst, at


def ld(x):
    return np.asarray(x, dtype=np.longdouble)


def ulp_operands(seed, n):
    """dict name -> operands (tuple of arrays): the distributions of tests/test_cabi_and_host.py, the operands the kernels
    see (envelope sums 1e2 .. 1e9, (E - L) / (E + L) with E ~ L), and quotients straddling SGX_ATAN_SHORT_MAX"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-3, 7, n)
    b = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 7, n)
    # envelopes: E, L = sqrt(I^2 + Q^2) of sums between 1e2 and 1e9; the DLL's quotient (E - L) / (E + L), E ~ L
    env = 10.0 ** rng.uniform(2, 9, n)
    e2 = np.where(rng.random(n) < 0.5, np.abs(a) ** 2, env * env * rng.uniform(0.5, 2.0, n))
    E = env
    L = env * (1.0 + rng.normal(0.0, 1.0, n) * 10.0 ** rng.uniform(-8, -0.5, n))
    kern = rng.random(n) < 0.5
    da = np.where(kern, E - L, a)
    db = np.where(kern, E + L, b)
    # atan(q / i): the host tests' (short and libm paths), a locked channel's (|q / i| small, sums 1e2 .. 1e9), and
    # |q / i| = 0.25 moved up to 4 numbers either way
    q = rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-2, 5, n)
    i = rng.choice([-1.0, 1.0], n) * np.abs(q) * 10.0 ** rng.uniform(-1, 3, n)
    lock = rng.random(n) < 0.3
    i = np.where(lock, rng.choice([-1.0, 1.0], n) * env, i)
    q = np.where(lock, i * rng.normal(0.0, 0.08, n), q)
    edge = rng.random(n) < 0.1
    i = np.where(edge, rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-5, 30, n), i)
    q = np.where(edge, nudge(rng.choice([-1.0, 1.0], n) * ATAN_SHORT_MAX * i, rng.integers(-4, 5, n)), q)
    u = rng.uniform(0, 2, n)
    ph = rng.uniform(-0.34, 0.34, n) * 10.0 ** -rng.integers(0, 5, n).astype(np.float64)
    return {"ab": (a, b), "b": (b,), "sqrt": (e2,), "div": (da, db), "atan": (q, i), "turns": (u,), "rot": (ph,)}


def atan_path(q, i):
    """+1: the short polynomial for certain (|q / i| below SGX_ATAN_SHORT_MAX by more than any quotient's error), -1: libm's
    atan for certain, 0: either (the computed quotient decides)"""
    z = np.abs(q / i)
    return np.where(z < ATAN_SHORT_MAX * (1 - 1e-14), 1, np.where(z > ATAN_SHORT_MAX * (1 + 1e-14), -1, 0))


_OPS = {}


def ulp_report(evaluate, names=None, seed=20261018, n=1 << 18):
    """Worst error of every function of the chain under `evaluate(fn name, *operands) -> (out0, out1)`, as
    {name: (worst, operands of the worst)}.  sin / cos / rotation: absolute, in units of 2^-53; the rest in ulps of the exact
    result.  The atan's are reported per path: '<name>/short', '<name>/libm'.  names: only these functions."""
    import mpmath as mp
    mp.mp.dps = 50
    if (seed, n) not in _OPS:
        _OPS[(seed, n)] = ulp_operands(seed, n)
    ops = _OPS[(seed, n)]
    rng = np.random.default_rng(seed + 1)
    rep = {}
    want = lambda name: names is None or name in names

    def one(name, out, operands, screen_ref, exact_of, absolute=False, subset=None, label=None):
        got = np.asarray(out, dtype=np.float64)
        if HAVE_LONGDOUBLE:
            ref = screen_ref()
            err = np.abs(ld(got) - ref) / (ld(2.0) ** -53 if absolute else ld(ulp_unit(ref)))
            err = np.asarray(err, dtype=np.float64)
        else:
            err = np.zeros(got.size)
        if subset is not None:
            err = np.where(subset, err, -1.0)
        idx = select(err, rng)
        if subset is not None:
            idx = idx[subset[idx]]
        w, at = worst_error(got, idx, exact_of, absolute)
        prev = rep.get(label or name, (0.0, None))
        if not w <= prev[0]:
            rep[label or name] = (w, tuple(float(x[at]) for x in operands))

    M = mp.mpf
    (b,) = ops["b"]
    if want("rcp"):
        one("rcp", evaluate("rcp", b)[0], (b,), lambda: 1 / ld(b), lambda k: 1 / M(float(b[k])))
    a2, b2 = ops["ab"]
    da, db = ops["div"]
    for name in filter(want, ("fast_div", "div1")):
        for x, y in ((a2, b2), (da, db)):
            one(name, evaluate(name, x, y)[0], (x, y), lambda: ld(x) / ld(y), lambda k: M(float(x[k])) / M(float(y[k])))
    (e2,) = ops["sqrt"]
    for name in filter(want, ("fast_sqrt", "sqrt1", "sqrt1_pos")):
        one(name, evaluate(name, e2)[0], (e2,), lambda: np.sqrt(ld(e2)), lambda k: mp.sqrt(M(float(e2[k]))))
    q, i = ops["atan"]
    path = atan_path(q, i)
    for name in filter(want, ("atan_ratio", "atan_ratio_k")):
        out = evaluate(name, q, i)[0]
        for label, sub in (("short", path >= 0), ("libm", path <= 0)):
            one(name, out, (q, i), lambda: np.arctan(ld(q) / ld(i)), lambda k: mp.atan(M(float(q[k])) / M(float(i[k]))),
                subset=sub, label=name + "/" + label)
    (u,) = ops["turns"]
    two_pi = 2 * ld(np.pi) + 2 * ld(1.2246467991473532e-16)     # pi to a long double
    for name in filter(want, ("sincos_turns_short", "sincos_turns")):
        try:
            sn, cs = evaluate(name, u)
        except NotImplementedError:      # (sincos_turns is a __device__ function: no host evaluation)
            continue
        one(name, sn, (u,), lambda: np.sin(two_pi * ld(u)), lambda k: mp.sin(2 * mp.pi * M(float(u[k]))), absolute=True)
        one(name, cs, (u,), lambda: np.cos(two_pi * ld(u)), lambda k: mp.cos(2 * mp.pi * M(float(u[k]))), absolute=True)
    (ph,) = ops["rot"]
    if not want("rot_small"):
        return rep
    sn, cs = evaluate("rot_small", ph)
    one("rot_small", sn, (ph,), lambda: np.sin(ld(ph)), lambda k: mp.sin(M(float(ph[k]))), absolute=True)
    one("rot_small", cs, (ph,), lambda: np.cos(ld(ph)), lambda k: mp.cos(M(float(ph[k]))), absolute=True)
    return rep


def bound_of(label):
    return BOUNDS[label.split("/")[0]]
