"""The table of small records for the swept-interference excision stage: every case is (name, int8 record, N, threshold,
passes), built in numpy from a fixed seed.  tests/test_excise_cases.py conditions them against the contract
(tests/excise_spec.py) alone - every decision at least spec.MARGIN from a rounding error - tests/test_excise_host.py runs
the host items on them and tests/test_excise_gpu.py the kernel.  A case that misses a margin gets another seed, never a
smaller margin.  The contract's result of a case is computed once per process (reference())."""
import importlib

import numpy as np

import excise_spec as spec

_native = importlib.import_module("softgnss-python_amd._native")


def tile_segments(N):
    """Segments one workgroup holds at segment length N, from the library's plan."""
    return _native.excise_plan(1, N)[1]


def tile_span(N, tiles):
    """A record length that is no multiple of the hop and spans `tiles` tiles and a little of the next: a tile owns the
    S - 1 hops between its segments."""
    return tiles * (tile_segments(N) - 1) * (N // 2) + N // 2 + 7


def noise(rng, n, sigma):
    return rng.normal(0.0, sigma, n)


def chirp(n, amp, f0, f1, period, start=0):
    """A sawtooth chirp: the frequency (cycles per sample) runs from f0 to f1 over `period` samples, then jumps back."""
    t = (np.arange(n, dtype=np.float64) + start) % period
    return amp * np.cos(2.0 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / period))


def to_int8(v):
    return np.clip(np.rint(v), -127, 127).astype(np.int8)


class Case(object):
    def __init__(self, name, N, build, threshold=8.0, passes=3, seed=1, expect=()):
        self.name, self.N, self.threshold, self.passes, self.seed = name, int(N), float(threshold), int(passes), seed
        self._build, self.expect = build, tuple(expect)
        self._x = self._ref = None

    @property
    def x(self):
        if self._x is None:
            self._x = self._build(np.random.default_rng(self.seed), self.N)
            assert self._x.dtype == np.int8
            self._x.setflags(write=False)
        return self._x

    def reference(self):
        """(y, info with margins) of the contract; once per process, never changed."""
        if self._ref is None:
            y, info = spec.excise(self.x, self.N, self.threshold, self.passes, margins=True)
            y.setflags(write=False)
            self._ref = (y, info)
        return self._ref


def _fixed(n, sigma=12.0):
    return lambda rng, N: to_int8(noise(rng, n(N) if callable(n) else n, sigma))


def _tiles(sigma, amp, tiles=3):
    # the chirp runs through the whole record, so through every tile cut and the segments on either side of it
    def build(rng, N):
        n = tile_span(N, tiles)
        return to_int8(noise(rng, n, sigma) + chirp(n, amp, 0.12, 0.12 + 0.04 * 64.0 / N, 3.0 * N))
    return build


def _rails(rng, N):
    # a strong line under noise that saturates: with the line cut, samples on a rail move beyond it by the line's amplitude
    n = 9000 + N // 2 + 3
    t = np.arange(n)
    return to_int8(80.0 * np.cos(2.0 * np.pi * 0.2031 * t) + noise(rng, n, 60.0))


def _cw(rng, N):
    n = 6001
    return to_int8(noise(rng, n, 10.0) + 40.0 * np.cos(2.0 * np.pi * 0.3117 * np.arange(n)))


def _chirp_alone(rng, N):
    n = 7013
    return to_int8(chirp(n, 90.0, 0.05, 0.05 + 0.1 * 64.0 / N, 2.5 * N) + noise(rng, n, 0.4))


def _chirp_noise(rng, N):
    n = 200000 + 11 if N == 256 else 20000 + 11
    return to_int8(noise(rng, n, 8.0) + chirp(n, 60.0, 0.20, 0.20 + 0.06 * 64.0 / N, 2.0 * N + 37))


def _constant(rng, N):
    return np.full(5 * N + 3, 37, dtype=np.int8)


def _alternating(rng, N):
    return (41 * (1 - 2 * (np.arange(4 * N + 5) & 1))).astype(np.int8)


CASES = []
for _N in (64, 256, 1024):
    _H = _N // 2
    for _tag, _n in (("1", 1), ("H-1", _H - 1), ("H", _H), ("H+1", _H + 1), ("N", _N)):
        CASES.append(Case("len_%s_N%d" % (_tag, _N), _N, _fixed(_n, 30.0), seed=10 + len(CASES)))
    CASES.append(Case("tiles3_N%d" % _N, _N, _tiles(6.0, 50.0), seed=40 + _N, expect=("tile_cuts",)))
    CASES.append(Case("noise_N%d" % _N, _N, _fixed(5003 + _N), seed=50 + _N))
    CASES.append(Case("cw_N%d" % _N, _N, _cw, seed=60 + _N, expect=("cut",)))
    CASES.append(Case("chirp_alone_N%d" % _N, _N, _chirp_alone, seed=70 + _N, expect=("cut",)))
    CASES.append(Case("chirp_noise_N%d" % _N, _N, _chirp_noise, seed=80 + _N, expect=("cut",)))
CASES += [
    Case("rails_N256", 256, _rails, seed=91, expect=("cut", "clipped")),
    Case("rails_N64", 64, _rails, seed=92, expect=("cut", "clipped")),
    Case("constant_N256", 256, _constant, seed=93),
    Case("alternating_N64", 64, _alternating, seed=94),
    Case("alternating_N1024", 1024, _alternating, seed=95),
    Case("passes1_N256", 256, _tiles(6.0, 50.0, 1), passes=1, seed=96, expect=("cut",)),
    Case("passes8_N256", 256, _tiles(6.0, 50.0, 1), passes=8, seed=97, expect=("cut",)),
    Case("passes8_N64", 64, _chirp_noise, passes=8, seed=98, expect=("cut",)),
    Case("threshold1_N256", 256, _fixed(4100), threshold=1.0, seed=99, expect=("cut",)),
    Case("threshold1_N1024", 1024, _fixed(4100), threshold=1.0, passes=8, seed=100, expect=("cut",)),
    Case("threshold_large_N256", 256, _tiles(6.0, 50.0, 2), threshold=1e6, seed=101, expect=("identity",)),
    Case("threshold_large_N64", 64, _rails, threshold=1e6, seed=102, expect=("identity",)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
