"""CPU-only checks of the boundary and the host logic: the C-ABI library loads and exports every
symbol include/sgx.h declares, the exact host helpers agree with the goldens captured from the
reference, device entry points fail loudly without a GPU, and the Python drop-in keeps the
reference's surface.  No compute kernels run here."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden, pkg


@pytest.fixture(scope="module")
def built():
    ge = importlib.import_module("__graft_entry__")
    ge.build()
    return pkg()


def header_symbols():
    text = open(os.path.join(ROOT, "include", "sgx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sgx_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(built):
    syms = header_symbols()
    assert len(syms) >= 20
    lib = ctypes.CDLL(built._native.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), "libsgx.so lacks %s declared in include/sgx.h" % s
    assert tuple(syms) == built._native.SYMBOLS, "ctypes prototypes and header disagree"
    assert b"gfx950" in built._native.lib().sgx_version()


def test_struct_layouts_match_header(built):
    n = built._native
    assert ctypes.sizeof(n.Settings) == 10 * 8 + 8 + 4 + 4
    assert ctypes.sizeof(n.ChanInit) == 24
    assert ctypes.sizeof(n.Sat) == 40
    assert ctypes.sizeof(n.Scene) == 16 + 16 * 40 + 512 + 16 * 256
    assert ctypes.sizeof(n.Timing) == 32


def test_host_helpers_match_reference_goldens(built):
    g = load_golden("codes.npz")
    s = built.Settings()
    assert s.samplesPerCode == int(g["samples_per_code"])
    codes = np.stack([s.generateCAcode(p) for p in range(32)])
    assert np.array_equal(codes.astype(np.int8), g["ca_codes"])
    t = s.makeCaTable()
    assert t.shape == (32, 38192)
    assert np.array_equal(np.packbits(t > 0, axis=1), g["ca_table_bits"])
    assert s.calcLoopCoef(2.0, 0.7, 1.0) == tuple(g["loop_dll"])
    assert s.calcLoopCoef(25.0, 0.7, 0.25) == tuple(g["loop_pll"])
    with pytest.raises(AssertionError):
        s.generateCAcode(32)                      # reference asserts prn in range(0, 32)
    out = np.empty(1023)
    rc = built._native.lib().sgx_generate_ca_code(40, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == built._native.SGX_E_ARG and "outside 0..31" in built._native.last_error()


def test_other_sampling_rate_table(built):
    """A second front-end (16.3676 Msps) exercises the exact index rule on another N."""
    from oracle import softgnss_oracle as orc
    s = built.Settings()
    s.samplingFreq = 16367600.0
    s.IF = 4130400.0
    o = orc.OracleSettings(samplingFreq=16367600.0, IF=4130400.0)
    assert s.samplesPerCode == o.samplesPerCode == 16368
    assert np.array_equal(s.makeCaTable(), orc.make_ca_table(o))


def test_settings_surface_matches_reference(built):
    s = built.Settings()
    want = dict(msToProcess=37000.0, numberOfChannels=8, skipNumberOfBytes=0, dataType='int8', IF=9548000.0,
                samplingFreq=38192000.0, codeFreqBasis=1023000.0, codeLength=1023, skipAcquisition=False,
                acqSearchBand=14.0, acqThreshold=2.5, dllDampingRatio=0.7, dllNoiseBandwidth=2.0,
                dllCorrelatorSpacing=0.5, pllDampingRatio=0.7, pllNoiseBandwidth=25.0, navSolPeriod=500.0,
                elevationMask=10.0, useTropCorr=True, plotTracking=True)
    for k, v in want.items():
        assert getattr(s, k) == v, k
    assert list(s.acqSatelliteList) == list(range(1, 33))
    assert s.c == 299792458.0 and s.startOffset == 68.802
    with pytest.raises(AttributeError):
        s.c = 1.0
    r = built.Result(s)
    with pytest.raises(AssertionError):
        r.results
    with pytest.raises(AssertionError):
        r.results = [1, 2, 3]
    # skipAcquisition=True makes the reference read acquisition results nothing assigned (NameError,
    # initialize.py:476-490); here: a clean error before any file is opened
    s.skipAcquisition = True
    with pytest.raises(ValueError, match="skipAcquisition"):
        s.postProcessing("/nonexistent/record.bin")


def test_no_gpu_means_loud_failure(built):
    if built._native.device_count() > 0:
        pytest.skip("a GPU is present")
    s = built.Settings()
    with pytest.raises(built._native.SgxError):
        built.engine.get_context(s, 0)
    a = built.AcquisitionResult(s)
    with pytest.raises(built._native.SgxError):
        a.acquire(np.zeros(11 * 38192, dtype=np.int8))


def test_product_never_imports_the_oracle():
    pdir = os.path.join(ROOT, "softgnss-python_amd")
    for dirpath, _, files in os.walk(pdir):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "softgnss_oracle" not in text and "from oracle" not in text, f


def test_prerun_matches_reference_golden(built):
    g = load_golden("acq_default.npz")
    s = built.Settings()
    a = built.AcquisitionResult(s)
    a.results = np.rec.fromarrays([g["carrFreq"], g["codePhase"], g["peakMetric"]],
                                  names='carrFreq,codePhase,peakMetric')
    a.preRun()
    assert np.array_equal(a.channels.PRN, g["ch_PRN"])
    assert np.array_equal(a.channels.acquiredFreq, g["ch_acquiredFreq"])
    assert np.array_equal(a.channels.codePhase, g["ch_codePhase"])
    assert [str(x) for x in a.channels.status] == [str(x) for x in g["ch_status"]]
    s.numberOfChannels = 3                         # fewer channels than detections: strongest three
    a.preRun()
    assert list(a.channels.PRN) == list(g["ch_PRN"][:3])
    a.showChannelStatus()


def test_dropin_module_names(built):
    import sys
    d = os.path.join(ROOT, "softgnss-python_amd", "dropin")
    sys.path.insert(0, d)
    try:
        for m in ("initialize", "acquisition", "tracking"):
            sys.modules.pop(m, None)
        import acquisition
        import initialize
        import tracking
        assert initialize.Settings is built.Settings
        assert acquisition.AcquisitionResult is built.AcquisitionResult
        assert tracking.TrackingResult is built.TrackingResult
    finally:
        sys.path.remove(d)
        for m in ("initialize", "acquisition", "tracking"):
            sys.modules.pop(m, None)


def test_synth_scene_is_integer_and_deterministic(built):
    sy = built.synth
    sc = sy.Scene.default()
    a = sy.generate(sc, 5000, offset=777)
    b = sy.generate(sc, 9000, offset=0)[777:777 + 5000]
    assert a.dtype == np.int8 and np.array_equal(a, b)
    assert np.abs(a).max() <= 127 and 15 < a.std() < 35
    for sat in sc.sats:
        assert all(isinstance(v, int) for v in sat.values())
    st = built._native.scene_struct(sc)
    assert st.n_sats == 8 and st.sats[0].prn == 1


def test_reciprocal_division_identity_used_by_the_kernels():
    """csrc/sgx_trk_common.h div_rn: a*y with two FMA corrections (y = RN(1/b)) equals IEEE a/b for the
    divisors on the tracking path (pi, fs, block lengths).  Emulated with exact rational arithmetic: the two rates and
    eight block lengths this test has always had, then every divisor class of tests/trk_math_cases.py at all thirteen
    rates of the suite - blk / fs, which the PLL waves of sgx_trk2.hip and sgx_trk3.hip form, among them.  (The same
    operands go through the COMPILED sgx_div_rn in tests/test_trk_math_host.py and, on the device, through both copies
    in tests/test_trk_math_gpu.py.)"""
    import math
    import random
    from fractions import Fraction as F
    import trk_math_cases as tm

    def rn(x):
        return float(x)          # Fraction -> nearest double, ties to even

    def fma(a, b, c):
        return rn(F(a) * F(b) + F(c))

    def div_rn(a, b, y):
        q0 = rn(F(a) * F(y))
        q1 = fma(fma(-q0, b, a), y, q0)
        return fma(fma(-q1, b, a), y, q1)

    random.seed(7)
    for b in (math.pi, 38192000.0, 16367600.0, 38189.0, 38191.0, 38192.0, 38193.0, 38196.0, 16368.0):
        y = rn(F(1) / F(b))
        for _ in range(1500):
            if b == math.pi:
                a = random.uniform(-0.25, 0.25) * random.choice([1.0, 1e-3, 1e-7])
            elif b > 1e6:
                a = 1023000.0 + random.uniform(-60.0, 60.0)
            else:
                a = 1023.0 + random.uniform(-2e-3, 2e-3)
            assert div_rn(a, b, y) == rn(F(a) / F(b))
    classes = tm.div_rn_operands(per_divisor=400, per_block_length=60, seed=11)
    assert set(np.unique(classes["blk_over_fs"][1])) == set(tm.FS) and classes["blk_over_fs"][0].size == 13 * 121
    for name, (aa, bb) in classes.items():
        recip = {}
        for a, b in zip(aa.tolist(), bb.tolist()):
            if b not in recip:
                recip[b] = rn(F(1) / F(b))
                assert recip[b] == 1.0 / b
            assert div_rn(a, b, recip[b]) == rn(F(a) / F(b)) == a / b, (name, a, b)


def test_nav_parity_check_matches_oracle():
    """sgx_nav_parity_check (host code, no GPU) vs the oracle's restatement of navPartyChk, incl. the in-place flip."""
    import oracle.softgnss_oracle as orc
    synth = pkg("synth")
    nav = pkg("postNavigation")
    bits = synth.subframe_bits(91, first_boundary=0, n_bits=1200).astype(np.float64) * 2 - 1
    rng = np.random.default_rng(5)
    for w in range(1, 38):
        for corrupt in (False, True):
            word = bits[30 * w - 2:30 * w + 30].copy()
            if corrupt:
                word[int(rng.integers(2, 32))] *= -1
            a, b = word.copy(), word.copy()
            assert nav.NavigationResult.navPartyChk(a) == orc.nav_party_chk(b)
            assert np.array_equal(a, b)
            if not corrupt:
                assert orc.nav_party_chk(word.copy()) != 0
    for _ in range(200):
        word = rng.choice([-1.0, 1.0], size=32)
        a, b = word.copy(), word.copy()
        assert nav.NavigationResult.navPartyChk(a) == orc.nav_party_chk(b)
        assert np.array_equal(a, b)


def test_navigation_result_surface():
    nav = pkg("postNavigation")
    for name in ("findPreambles", "navPartyChk", "postNavigate", "calculatePseudoranges", "plot"):
        assert hasattr(nav.NavigationResult, name)
    import importlib, sys
    sys.path.insert(0, os.path.join(ROOT, "softgnss-python_amd", "dropin"))
    try:
        m = importlib.import_module("postNavigation")
        assert m.NavigationResult is nav.NavigationResult
        e = importlib.import_module("ephemeris")
        assert e.ephemeris is pkg("ephemeris").ephemeris
        gfm = importlib.import_module("geoFunctions")
        for name in ("satpos", "leastSquarePos", "cart2geo", "findUtmZone", "cart2utm", "topocent", "togeod", "tropo",
                     "e_r_corr", "check_t"):
            assert getattr(gfm, name) is getattr(pkg("geoFunctions"), name)
    finally:
        sys.path.pop(0)
        sys.modules.pop("postNavigation", None)
        sys.modules.pop("ephemeris", None)
        sys.modules.pop("geoFunctions", None)


def test_nav_bits_matches_oracle_including_summation_order():
    """sgx_nav_bits (host code) vs the oracle: numpy's pairwise order decides the sign of near-cancelling sums."""
    import oracle.softgnss_oracle as orc
    native = pkg("_native")
    rng = np.random.default_rng(8)
    x = rng.normal(size=33000) * 10.0 ** rng.integers(-8, 8, size=33000)
    # columns that cancel to rounding noise: the sign then depends on the order of the additions
    for c in range(0, 32000, 40):
        x[c + 10:c + 20] = -x[c:c + 10]
    for start in (20, 37, 1999, 2980):
        assert np.array_equal(native.nav_bits(x, start), orc.nav_bits(x, start))
    assert len(native.nav_bits(x, 1999)) == 1501
    assert np.array_equal(native.nav_bits(x[:12000], 1980), orc.nav_bits(x[:12000], 1980))   # clipped, 20 | len
    with pytest.raises(ValueError):
        orc.nav_bits(x[:12000], 1999)
    with pytest.raises(ValueError):
        native.nav_bits(x[:12000], 1999)


def test_pseudoranges_match_reference():
    """sgx_pseudoranges (host code) and the oracle vs NavigationResult.calculatePseudoranges of the reference
    (fixture made from the reference tracker's absoluteSample series)."""
    import oracle.softgnss_oracle as orc
    g = load_golden("nav_preambles.npz")
    m = pkg()
    s = m.Settings()
    s.samplingFreq, s.IF, s.numberOfChannels = 16367600.0, 4130400.0, 2
    so = orc.OracleSettings(samplingFreq=16367600.0, IF=4130400.0, numberOfChannels=2)

    class Trk(object):
        pass

    t = Trk()
    t.settings, t.channels = s, None
    t.results = np.recarray((2,), dtype=[('status', 'S1'), ('absoluteSample', 'O'), ('PRN', 'i8')])
    for i in range(2):
        t.results[i].status, t.results[i].absoluteSample, t.results[i].PRN = b'T', g["absoluteSample"][i], (4, 10)[i]
    nav = m.NavigationResult(t)
    for k in range(4):
        want = g["pr_all"][k]
        assert np.array_equal(orc.calculate_pseudoranges(so, g["absoluteSample"], g["pr_ms"][k], g["activeChnList"]), want)
        assert np.array_equal(nav.calculatePseudoranges(g["pr_ms"][k], g["activeChnList"]), want)
    one = nav.calculatePseudoranges(g["pr_ms"][1], np.array([1]))
    assert np.array_equal(one, g["pr_one"]) and np.isinf(one[0])
    assert np.all(np.isnan(nav.calculatePseudoranges(g["pr_ms"][0], np.array([], dtype=int))))
    with pytest.raises(IndexError):
        nav.calculatePseudoranges(np.array([10000.0, 5.0]), [0])
    # negative measurement points index from the end, like numpy does
    neg = np.array([-1.0, -3.0])
    assert np.array_equal(nav.calculatePseudoranges(neg, [0, 1]),
                          orc.calculate_pseudoranges(so, g["absoluteSample"], neg, [0, 1]))


def _eph_case(synth, case):
    seed, fb, fid, tow0, inv = [int(v) for v in case]
    tab = synth.nav_message_bits(seed, fb, 2048, tow0, fid)
    if inv:
        tab = 1 - tab
    start = fb if fb > 0 else 300
    return [str(int(b)) for b in tab[start:start + 1500]], str(int(tab[start - 1])), tab, start


def test_ephemeris_decode_matches_reference():
    """sgx_ephemeris (host code) and the oracle vs the reference's ephemeris.ephemeris on the generator's frames."""
    import oracle.softgnss_oracle as orc
    g = load_golden("eph_cases.npz")
    synth = pkg("synth")
    eph_mod = pkg("ephemeris")
    for case, want in zip(g["cases"], g["eph_tow"]):
        bits, d30, tab, start = _eph_case(synth, case)
        for fn in (orc.ephemeris, eph_mod.ephemeris):
            eph, tow = fn(list(bits), d30)
            assert np.array_equal(np.array(list(eph) + [tow], dtype=np.float64), want), fn
            assert all(isinstance(eph[i], int) for i in g["int_fields"]) and isinstance(tow, int)
    bits, d30, tab, start = _eph_case(synth, g["cases"][0])
    with pytest.raises(TypeError):
        eph_mod.ephemeris(bits[:1499], d30)
    with pytest.raises(TypeError):
        orc.ephemeris(bits[:1499], d30)
    # five subframes that repeat IDs 4 and 5 only: the reference trips over an unassigned local
    four = [str(int(b)) for b in np.concatenate([tab[start + 900:start + 1500]] * 3)[:1500]]
    with pytest.raises(UnboundLocalError):
        orc.ephemeris(list(four), str(int(tab[start + 899])))
    with pytest.raises(UnboundLocalError):
        eph_mod.ephemeris(four, str(int(tab[start + 899])))


def test_ephemeris_round_trip_of_random_parameters():
    """Encode random clock / orbit parameters into subframes 1-3 (synth.encode_ephemeris + parity + random stream
    polarity), decode them with sgx_ephemeris and the oracle: both must return every field quantised to its
    message LSB - computed here independently of either decoder."""
    import random
    import oracle.softgnss_oracle as orc
    synth = pkg("synth")
    eph_mod = pkg("ephemeris")
    for seed in range(40):
        e = synth.make_ephemeris(9000 + seed, toe=16 * random.Random(seed).randrange(0, 37800))
        tab = synth.nav_message_bits(seed, 0, 2048, 50000 + seed, 1 + seed % 5, e)
        if seed % 2:
            tab = 1 - tab
        bits = [str(int(b)) for b in tab[300:1800]]
        d30 = str(int(tab[299]))
        got, tow = eph_mod.ephemeris(bits, d30)
        ref, tow2 = orc.ephemeris(list(bits), d30)
        assert got == ref and tow == tow2 == (50000 + seed + 1) * 6     # the stream starts one subframe in
        for sid, fields in synth.EPH_LAYOUT.items():
            for name, exp, times_pi, signed, slices in fields:
                v = e["IODE_sf2"] if name == "IODE_sf3" else e[name]
                v = v - 1024 if name == "weekNumber" else v
                q = int(round(v / (synth.GPS_PI if times_pi else 1.0) / 2.0 ** exp))
                want = q * 2.0 ** exp * (synth.GPS_PI if times_pi else 1.0) + (1024 if name == "weekNumber" else 0)
                have = got[eph_mod.FIELDS.index(name)]
                assert have == want or abs(have - want) <= 1e-15 * abs(want), (name, have, want)


def test_plot_methods_run_headless():
    """plot() of the three result classes draws with matplotlib when it is installed (Agg backend here) and
    returns quietly when it is not - a script written for the reference, which calls them, keeps running."""
    mpl = pytest.importorskip("matplotlib")
    mpl.use("Agg")
    m = pkg()
    s = m.Settings()
    s.numberOfChannels, s.msToProcess = 2, 50.0
    a = m.AcquisitionResult(s)
    cf = np.zeros(32)
    cf[[0, 6]] = 9.55e6
    a.results = np.rec.fromarrays([cf, np.zeros(32), np.linspace(1, 4, 32)], names='carrFreq,codePhase,peakMetric')
    a.plot()
    t = m.TrackingResult.__new__(m.TrackingResult)
    t._settings = s
    tr = pkg("tracking")
    t._results = np.recarray((2,), dtype=tr.RESULT_DTYPE)
    rng = np.random.default_rng(0)
    for i in range(2):
        for name in t._results.dtype.names[1:-1]:
            t._results[i][name] = rng.normal(size=50)
        t._results[i].status, t._results[i].PRN = b'T', 3 + i
    t.plot()
    g = load_golden("fix_scene.npz")
    nav = m.NavigationResult.__new__(m.NavigationResult)
    nav._settings = s
    channel = np.rec.array([(g["chPRN"], g["el"], g["az"], g["rawP"], g["correctedP"])], formats=['O'] * 5,
                           names='PRN,el,az,rawP,correctedP')
    nav._solutions = np.rec.array([(channel, g["DOP"], g["X"], g["Y"], g["Z"], g["dt"], g["latitude"], g["longitude"],
                                    g["height"], float(g["utmZone"]), g["E"], g["N"], g["U"])], formats=['O'] * 13,
                                  names='channel,DOP,X,Y,Z,dt,latitude,longitude,height,utmZone,E,N,U')
    nav.plot()
    import matplotlib.pyplot as plt
    assert len(plt.get_fignums()) >= 4
    plt.close('all')


def _math_eval(fn, a, b=0.0):
    import ctypes as C
    L = pkg()._native.lib()
    out = (C.c_double * 2)()
    assert L.sgx_trk_math_eval(fn, float(a), float(b), out) == 0
    return out[0], out[1]


def test_short_chain_loop_filter_arithmetic_ulp_bounds(built):
    """csrc/sgx_trk_math.h (the loop-filter waves' reciprocal-based division and square root, short atan, Estrin
    sincos, division-free ceil) against 50-digit arithmetic.  The host build starts its Newton iterations from a
    float-precision seed and calls glibc's atan; the device compilation (v_rcp_f64 / v_rsq_f64, ocml's atan) is held to the
    same bounds by tests/test_trk_math_gpu.py."""
    import math
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(20260102)

    def ulps(got, exact):
        if exact == 0:
            return abs(got)
        e = abs(mp.mpf(got) - exact)
        return float(e / (mp.mpf(2) ** (math.frexp(float(exact))[1] - 53)))

    worst = dict(rcp=0.0, div=0.0, sqrt=0.0, atan=0.0, sin=0.0, cos=0.0)
    for _ in range(4000):
        a = float(rng.uniform(-1, 1) * 10.0 ** rng.uniform(-3, 7))
        b = float(rng.choice([-1, 1]) * 10.0 ** rng.uniform(-3, 7))
        worst["rcp"] = max(worst["rcp"], ulps(_math_eval(0, b)[0], 1 / mp.mpf(b)))
        worst["div"] = max(worst["div"], ulps(_math_eval(1, a, b)[0], mp.mpf(a) / mp.mpf(b)))
        x = abs(a) ** 2
        worst["sqrt"] = max(worst["sqrt"], ulps(_math_eval(2, x)[0], mp.sqrt(mp.mpf(x))))
        # atan(q / i): both the short path (|q/i| <= 0.25) and the libm path; the argument itself is within 1 ulp
        q = float(rng.uniform(-1, 1) * 10.0 ** rng.uniform(-2, 5))
        i = float(rng.choice([-1, 1]) * abs(q) * 10.0 ** rng.uniform(-1, 3))
        worst["atan"] = max(worst["atan"], ulps(_math_eval(3, q, i)[0], mp.atan(mp.mpf(q) / mp.mpf(i))))
        u = float(rng.uniform(0, 2))
        sn, cs = _math_eval(4, u)
        ex_s, ex_c = mp.sin(2 * mp.pi * mp.mpf(u)), mp.cos(2 * mp.pi * mp.mpf(u))
        # absolute error in units of 2^-53 (the phasors have modulus 1; what matters is the phase error)
        worst["sin"] = max(worst["sin"], float(abs(mp.mpf(sn) - ex_s) * 2 ** 53))
        worst["cos"] = max(worst["cos"], float(abs(mp.mpf(cs) - ex_c) * 2 ** 53))
    assert worst["rcp"] <= 1.0 and worst["div"] <= 1.5 and worst["sqrt"] <= 1.0, worst
    assert worst["atan"] <= 2.5, worst
    assert worst["sin"] <= 4.0 and worst["cos"] <= 4.0, worst
    assert _math_eval(2, 0.0)[0] == 0.0
    assert _math_eval(3, 1.0, 0.0)[0] == math.atan(math.inf) and _math_eval(3, -1.0, 0.0)[0] == -math.atan(math.inf)
    assert math.isnan(_math_eval(3, 0.0, 0.0)[0])


def test_one_step_division_sqrt_atan_and_small_rotation_ulp_bounds(built):
    """Round 3's shorter chain arithmetic (csrc/sgx_trk_math.h): sgx_div1 / sgx_sqrt1 (one Newton step + one residual
    step), the atan with the quotient by sgx_div1, and the Taylor pair that turns a carrier-table entry by the rate
    step (|angle| <= 0.34 rad), against 50-digit arithmetic; host seeds are float precision (the device compilation:
    tests/test_trk_math_gpu.py)."""
    import math
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(20261002)

    def ulps(got, exact):
        e = abs(mp.mpf(got) - exact)
        return float(e / (mp.mpf(2) ** (math.frexp(float(exact))[1] - 53)))

    worst = dict(div=0.0, sqrt=0.0, atan=0.0, rot=0.0)
    for _ in range(4000):
        a = float(rng.uniform(-1, 1) * 10.0 ** rng.uniform(-3, 7))
        b = float(rng.choice([-1, 1]) * 10.0 ** rng.uniform(-3, 7))
        worst["div"] = max(worst["div"], ulps(_math_eval(6, a, b)[0], mp.mpf(a) / mp.mpf(b)))
        x = abs(a) ** 2
        worst["sqrt"] = max(worst["sqrt"], ulps(_math_eval(7, x)[0], mp.sqrt(mp.mpf(x))))
        q = float(rng.uniform(-1, 1) * 10.0 ** rng.uniform(-2, 5))
        i = float(rng.choice([-1, 1]) * abs(q) * 10.0 ** rng.uniform(-1, 3))
        worst["atan"] = max(worst["atan"], ulps(_math_eval(8, q, i)[0], mp.atan(mp.mpf(q) / mp.mpf(i))))
        ph = float(rng.uniform(-0.34, 0.34) * 10.0 ** -rng.integers(0, 5))
        sn, cs = _math_eval(9, ph)
        err = max(abs(mp.mpf(sn) - mp.sin(mp.mpf(ph))), abs(mp.mpf(cs) - mp.cos(mp.mpf(ph))))
        worst["rot"] = max(worst["rot"], float(err * 2 ** 53))     # phase error in units of 2^-53 rad
    assert worst["div"] <= 1.5 and worst["sqrt"] <= 1.0 and worst["atan"] <= 2.5 and worst["rot"] <= 2.0, worst
    assert _math_eval(7, 0.0)[0] == 0.0
    assert _math_eval(8, 1.0, 0.0)[0] == math.atan(math.inf) and math.isnan(_math_eval(8, 0.0, 0.0)[0])


def test_block_length_without_a_division_equals_the_reference(built):
    """sgx_block_length == ceil((1023 - rem) / (codeFreq / fs)) as numpy evaluates tracking.py:148-151 (two correctly
    rounded divisions), for code frequencies around the basis, including quotients that are integers or a few ulp off -
    at 38.192 MHz one call at a time, then at all thirteen rates of the suite through the batch entry's fs operand."""
    import math
    import trk_math_cases as tm
    rng = np.random.default_rng(77)
    fs = 38192000.0
    assert int(_math_eval(10, 1023.0, 1023000.0)[0]) == 38192          # block 0: the quotient IS an integer
    for k in range(20000):
        cf = 1.023e6 + rng.normal(0, 5)
        step = cf / fs
        if k % 4 == 0:
            n = int(rng.integers(38000, 38400))
            a = n * step
            for _ in range(int(rng.integers(0, 5))):
                a = float(np.nextafter(a, a + rng.choice([-1.0, 1.0])))
        else:
            a = 1023.0 - rng.uniform(-0.05, 0.05)
        got, step_a = _math_eval(10, a, cf)
        assert int(got) == math.ceil(a / step), (a, cf)
        assert abs(step_a - step) <= 3 * np.spacing(step)
    a, cf, fs = tm.block_length_operands(40000, 78)
    blk, step_a = pkg()._native.trk_math_eval(tm.FN["block_length"], a, cf, fs, 1.0 / fs)
    step = cf / fs
    assert not (msg := tm.first_mismatch(blk, np.ceil(a / step), a=a, codeFreq=cf, fs=fs)), msg
    bad = np.flatnonzero(~(np.abs(step_a - step) <= 3 * np.spacing(step)))
    assert bad.size == 0, (float(cf[bad[0]]), float(fs[bad[0]]), float(step_a[bad[0]]), float(step[bad[0]]))
    first = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]])              # block 0 of every rate
    assert np.all(a[first] == 1023.0) and np.all(cf[first] == 1.023e6) and first.size == 13
    # (26 MHz: RN(1023 / RN(1.023e6 / fs)) = 26000.000000000004, so the reference's first block there has 26 001 samples)
    assert np.array_equal(blk[first] - [tm.n_code(f) for f in tm.FS], [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0])


def test_division_free_ceil_equals_ieee_ceil(built):
    """sgx_ceil_div(a, b) == ceil(a / b) for the block-length computation blksize = ceil((1023 - rem) / step)
    (tracking.py:148-151), including quotients that are exact integers or within a few ulp of one - at 38.192 MHz one call
    at a time, then at all thirteen rates of the suite through the batch entry."""
    import math
    import trk_math_cases as tm
    rng = np.random.default_rng(7)
    fs = 38.192e6
    for k in range(20000):
        step = (1.023e6 + rng.normal(0, 5)) / fs
        if k % 4 == 0:
            # quotient at (or a few ulp next to) an integer
            n = int(rng.integers(38000, 38400))
            a = n * step
            a = float(np.nextafter(a, a + rng.choice([-1.0, 1.0]) * 1.0)) if k % 8 else a
            for _ in range(int(rng.integers(0, 4))):
                a = float(np.nextafter(a, a + 1.0))
        else:
            a = 1023.0 - rng.uniform(-0.05, 0.05)
        assert int(_math_eval(5, a, step)[0]) == math.ceil(a / step), (a, step)
    a, cf, fs = tm.block_length_operands(40000, 8)
    step = cf / fs
    got = pkg()._native.trk_math_eval(tm.FN["ceil_div"], a, step)[0]
    assert not (msg := tm.first_mismatch(got, np.ceil(a / step), a=a, step=step, fs=fs)), msg


def test_tracking_kernel_selection_table(built):
    """The host's one rule for which tracking kernel runs with how many workgroups per channel (csrc/sgx_trk.hip: trk_plan, the
    table in front of it; exported as sgx_track_plan, no GPU needed) - data type x channels x sampling rate x correlator
    spacing -> kernel, members.  kernel: 2 trk2_kernel, 3 trk_kernel_tp, 4 trk_kernel_multi, 5 trk3_kernel, 6 trk_kernel_any."""
    m = pkg()
    N = m._native
    DT = dict(int8=0, int16=1, uint8=2, float32=3, float64=4, uint16=5, float16=10)

    def plan(dt="int8", ch=8, fs=38.192e6, d=0.5, cus=256, fl=False):
        s = m.Settings()
        s.samplingFreq, s.dllCorrelatorSpacing = fs, d
        return N.track_plan(s, DT[dt], ch, cus, fl)

    table = [
        # the headline: 8 channels of the default front end -> the speculative kernel, 20 units of 128 groups
        (dict(), (5, 20)),
        (dict(dt="uint8"), (5, 20)),
        (dict(ch=12), (2, 10)),                   # 16 padded channels x 20 units do not fit 256 CUs: one workgroup per unit
        (dict(ch=4), (5, 20)),
        # other spacings, other rates: the round-3 kernel, one workgroup per unit and arm while 3 x units x ch8 CUs are free
        (dict(d=0.25), (2, 30)),
        (dict(d=0.4), (2, 30)),
        (dict(fs=60e6, d=0.32), (2, 15)),         # (the gap test alone would have let the speculative kernel in: ADVICE r4)
        (dict(fs=60e6, d=0.5), (5, 30)),
        (dict(fs=16.3676e6), (2, 15)),           # 16 samples per chip: 18 samples span more than half a chip
        # int16 and float records never run the speculative kernel
        (dict(dt="int16"), (2, 30)),
        (dict(dt="float32", fl=True), (2, 10)),
        (dict(dt="float64", fl=True), (2, 10)),
        (dict(dt="float32", fl=False), (6, 10)),  # out of range / not scanned: sample by sample
        (dict(dt="uint16"), (6, 10)),
        (dict(dt="float16"), (6, 10)),
        # many channels: members shrink with the CUs left, throughput mode beyond 128 channels
        (dict(ch=16), (2, 10)),
        (dict(ch=64), (2, 4)),
        (dict(ch=128), (2, 2)),
        (dict(ch=129), (3, 1)),
        (dict(ch=3072, dt="int16"), (3, 1)),
        (dict(ch=3072, dt="float32", fl=True), (2, 1)),
        # fewer than ~15.4 samples per chip: a group can hold several switches of one ramp
        (dict(fs=5.456e6), (4, 2)),
        (dict(fs=5.456e6, dt="uint8"), (6, 2)),
        (dict(fs=4.092e6, ch=200), (4, 1)),
        # a smaller device
        (dict(cus=64), (2, 8)),
        (dict(cus=8), (2, 1)),
    ]
    got = [plan(**kw) for kw, _ in table]
    bad = [(kw, g, want) for (kw, want), g in zip(table, got) if g != want]
    assert not bad, bad


def test_reserved_poll_registers_are_touched_by_nothing_else():
    """csrc/sgx_trk3.hip keeps poll loads in flight while the loop filter runs; the loads that land late write v[244:255],
    which therefore must appear in the speculative kernel's code ONLY inside the polls' asm statements.  The same gate runs
    inside build() and tools/build_variant.sh (softgnss-python_amd/build.py: check_trk3_registers)."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    ok, msg = pkg("build").check_trk3_registers((), hipcc)
    assert ok, msg
    ok, msg = pkg("build").check_trk3_registers(("-DT3_POLL2=0",), hipcc)   # (polls written in C++: no asm statements)
    assert not ok and "not found" in msg, msg       # the gate can fail


def test_throughput_kernel_spills_nothing_among_its_dot_products(tmp_path):
    """csrc/sgx_trk_tp.hip: the uint8 and int16 instances spill registers (5 and 44 at two workgroups per CU) - block-level
    values, stored once and reloaded once per block around the chip loop.  None of that may sit among the dot products
    (the chip loop's body): the compiled code of every instance has no scratch access between its first and last
    v_dot4_i32_i8."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "tp.s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
                        "-I", os.path.join(root, "include"), "-I", os.path.join(root, "softgnss-python_amd", "csrc"),
                        "-S", "--cuda-device-only", "-o", out, os.path.join(root, "softgnss-python_amd", "csrc", "sgx_trk_tp.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = open(out).read().splitlines()
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z13trk_kernel_tpILi\dEE", l)]
    assert len(starts) == 3
    for a, b in zip(starts, starts[1:] + [len(lines)]):
        body = lines[a:b]
        dots = [k for k, l in enumerate(body) if "v_dot4_i32_i8" in l]
        assert len(dots) >= 32
        inside = [body[k].strip() for k in range(min(dots), max(dots) + 1) if "scratch_" in body[k]]
        assert not inside, (lines[a][:30], inside[:3])


def test_acquisition_chunk_plan_covers_every_row_exactly_once():
    """sgx_acquire_plan (csrc/sgx_acq.hip: acq_plan) cuts the correlation batch into chunks of whole PRNs or - non-coherent
    sums - of one PRN's runs of Doppler bins, over one or two queues.  Whatever the sizes: every (PRN, bin) belongs to exactly
    one chunk, a chunk of bin runs holds ONE PRN (round 5: with two it wrote the second PRN's maxima to the first one's
    slots), a queue's chunk fits its share of the chunk size, and two queues are only used where there are two chunks."""
    m = pkg()
    default_rows, max_rows = m._native.acquire_plan_limits()     # (the library's own constants, not copies of them)
    assert 1 <= default_rows <= max_rows
    for n_prn in (1, 2, 4, 7, 32):
        for n_bins in (1, 2, 29, 57):
            for n_blocks, noncoh in ((1, False), (2, False), (10, True), (3, True), (1, True)):
                for chunk_rows in (0, 1, 29, 58, 120, 174, 200, 290, 348, 580, 1160, 4000):
                    for max_q in (1, 2):
                        prn_chunk, bin_runs, bins_per_run, queues = m._native.acquire_plan(n_prn, n_bins, n_blocks, noncoh,
                                                                                        chunk_rows, max_q)
                        what = (n_prn, n_bins, n_blocks, noncoh, chunk_rows, max_q, prn_chunk, bin_runs, bins_per_run, queues)
                        assert 1 <= prn_chunk <= n_prn and 1 <= bin_runs <= n_bins and 1 <= queues <= max_q, what
                        if bin_runs > 1:
                            assert noncoh and prn_chunk == 1 and queues == 2, what
                        seen = {}
                        chunks = 0
                        for p0 in range(0, n_prn, prn_chunk):
                            for b0 in range(0, n_bins, bins_per_run):
                                nb = n_bins if bin_runs == 1 else min(bins_per_run, n_bins - b0)
                                chunks += 1
                                for p in range(p0, min(p0 + prn_chunk, n_prn)):
                                    for b in range(b0, b0 + nb):
                                        seen[(p, b)] = seen.get((p, b), 0) + 1
                                rows = min(prn_chunk, n_prn - p0) * nb * n_blocks
                                limit = min(chunk_rows if chunk_rows > 0 else default_rows, max_rows)
                                if rows > n_bins * n_blocks or bin_runs > 1:       # (more than one PRN, or a part of one)
                                    assert rows <= max(limit // queues, 1) + (n_blocks * bins_per_run if bin_runs > 1 else 0), what
                        assert len(seen) == n_prn * n_bins and set(seen.values()) == {1}, what
                        if queues == 2:
                            assert chunks >= 2, what


def test_the_record_stages_share_one_binding_tail(monkeypatch):
    """Context._stage, which all seven record stage methods go through, against a stand-in library: the record pointer
    follows the stage's arguments, unpack's count array the record pointer, the int64 counters come last and become the
    record's attributes; a stage whose output length the host knows says so, the others ask sgx_if_length."""
    import weakref
    native = pkg("_native")
    calls = []

    class Lib(object):
        def __getattr__(self, name):
            def fn(*args):
                calls.append((name, args))
                if name == "sgx_if_length":
                    args[1]._obj.value = 4321
                counters = [a for a in args if isinstance(getattr(a, "_obj", None), ctypes.c_int64)]
                assert counters == list(args[len(args) - len(counters):])
                for k, a in enumerate(counters):
                    a._obj.value = 100 + k
                return native.SGX_OK
            return fn

    monkeypatch.setattr(native, "lib", lambda: Lib())
    ctx = native.Context.__new__(native.Context)
    ctx._h, ctx._records = native._P(), weakref.WeakSet()
    rec = native.Record(ctx, native._P(), 1000)
    taps = np.ones(3, dtype=np.int16)

    def stage_call():
        names = [name for name, _ in calls]
        args = calls[0][1]
        del calls[:]
        return names, args, [k for k, a in enumerate(args) if isinstance(getattr(a, "_obj", None), ctypes.c_void_p)]

    for run, fn, asks, counters in (
            (lambda: ctx.filter_record(rec, taps, 2), "sgx_if_filter", False, {}),
            (lambda: ctx.iq_to_if(rec, taps, 2), "sgx_if_from_iq", False, {}),
            (lambda: ctx.decimate(rec, 1, taps, 2, 4), "sgx_if_decimate", True, dict(clipped=100)),
            (lambda: ctx.resample(rec, taps, 2, 5, 3), "sgx_if_resample", True, dict(clipped=100))):
        out = run()
        names, args, records = stage_call()
        assert names == [fn] + ["sgx_if_length"] * asks and len(out) == (4321 if asks else 1000), fn
        assert records == [len(args) - 1 - len(counters)], fn            # &record: behind the arguments, before the counters
        assert dict((k, getattr(out, k)) for k in counters) == counters, fn
    out = ctx.requantize(rec, np.int16, mult=3, shift=1)
    assert stage_call()[0] == ["sgx_if_requantize"] and len(out) == 500 and out.clipped == 100
    out = ctx.condition(rec, np.int16, 1, 256, np.zeros(2, dtype=native.COND_PLAN_DTYPE), 8)
    assert stage_call()[0] == ["sgx_if_condition"] and len(out) == 500 and (out.blanked, out.clipped) == (100, 101)
    out = ctx.unpack(rec, 2, [-3, -1, 1, 3])
    names, args, records = stage_call()
    assert names == ["sgx_if_unpack", "sgx_if_length"] and len(out) == 4321 and records == [len(args) - 2]
    assert isinstance(args[-1], ctypes.c_void_p) and out.code_counts.shape == (4,) and out.code_counts.dtype == np.int64
