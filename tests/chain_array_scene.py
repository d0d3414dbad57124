"""The end-to-end scene of the multi-antenna chain tests: the I/Q scene of tests/array_cases.py - four antennas, four
satellites under a broadband jammer that no single antenna acquires through - read through antennas = 4, iqRecord and
resampleUp / resampleDown = 5 / 3: the combiner, the converter (8.184 Msps, IF 2.046 MHz) and the resampler behind it, a
real record at 13.64 Msps.  The file is a prefix of array_cases.record(SCENE_IQ); the composed contract of
tests/chain_cases.py prepares it.  Shared by tests/test_chain_array_host.py (CPU: the contracts plus the oracle alone) and
tests/test_chain_array_gpu.py."""
import array_cases
import chain_cases as cases
from oracle import softgnss_oracle as orc

SOURCE = array_cases.SCENE_IQ
MARGIN, ABSENT_MAX = array_cases.MARGIN, array_cases.ABSENT_MAX
PRNS = SOURCE.prns
TRK_MS = 100                            # code periods tracked end to end
SKIP_UNITS = 1237                       # the end-to-end skip, in the chain's smallest legal skipNumberOfBytes
CHAIN = cases.Chain(iq=True, resamp=(5, 3), fs=SOURCE.fs, f0=SOURCE.f0, iq_taps=array_cases.IQ_TAPS,
                    antennas=array_cases.ANTENNAS)
SKIP_BYTES = SKIP_UNITS * cases.skip_unit(CHAIN)        # whole frames of all antennas and whole groups of M samples
_CACHE = {}


def file_bytes(ms=TRK_MS + 4):
    """The first `ms` code periods of the scene's file."""
    return array_cases.head(SOURCE, ms * SOURCE.frames_per_ms)


def settings(m, **kw):
    return CHAIN.settings(m, numberOfChannels=len(PRNS), **kw)


def oracle_settings(**kw):
    p = cases.prepared_settings(CHAIN)
    return orc.OracleSettings(samplingFreq=p["samplingFreq"], IF=p["IF"], numberOfChannels=len(PRNS), **kw)


def need(skip_bytes):
    """The samples of the prepared record that postProcessing asks for with msToProcess = TRK_MS behind skip_bytes."""
    n = cases.prepared_settings(CHAIN)["samplesPerCode"]
    count = cases.prepared_skip(CHAIN, skip_bytes) + max(11 * n, TRK_MS * (n + 2) + 2 * n)
    return count + count % 2


def prepared(count, ms=TRK_MS + 4):
    """chain_cases.prepare of the first `count` samples of the prepared record of file_bytes(ms), as postProcessing prepares
    them (offset 0: a skip only picks the window that is searched)."""
    key = (int(count), int(ms))
    if key not in _CACHE:
        out = cases.prepare(file_bytes(ms), CHAIN, 0, count)
        out["record"].setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def contract_acquisition(skip_bytes=0):
    """oracle.acquire on 11 code periods of the composed contract's record of what postProcessing reads behind skip_bytes,
    from the sample that byte becomes."""
    o = oracle_settings()
    skip = cases.prepared_skip(CHAIN, skip_bytes)
    y = prepared(need(skip_bytes))["record"]
    window = y[skip:skip + 11 * o.samplesPerCode]
    assert window.size == 11 * o.samplesPerCode
    return orc.acquire(o, window)
