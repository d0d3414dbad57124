"""Dense scenes for the coherent acquisition: one strong satellite (no data-bit flips: these scenes are about indexing) per searched PRN, placed by Doppler BIN so that every
bin class of a search decides an assertion - both edge bins, every phi row of the shift path, both sides of every cut
between runs, a pair that shares one phi row with different circular shifts - and the table of searches
(tests/test_coherent_acq_cases.py conditions them in numpy, tests/test_coherent_acq_gpu.py runs them on the GPU).
Everything is numpy from fixed seeds; the numpy contract (tests/coherent_acq_spec.py) runs over PRNs in child processes
that import numpy only."""
import multiprocessing
import os

import numpy as np

import coherent_acq_spec as spec
import weak_scene
from oracle import softgnss_oracle as orc

CN0 = 50.0          # dB-Hz of every placed satellite
SIGMA = 8.0         # noise, LSB: 32 satellites of +-1.2 LSB each on top of it stay far from +-127
MAX_WORKERS = 16


def settings(fs=weak_scene.FS, if_=weak_scene.IF, band=14.0):
    return orc.OracleSettings(samplingFreq=fs, IF=if_, acqSearchBand=band)


def cut_bins(g):
    """Bins on either side of every cut between runs of bins (non-coherent sums cut in runs)."""
    if not (g["noncoh"] and g["bin_runs"] > 1):
        return []
    out = []
    for r in range(1, g["bin_runs"]):
        out += [r * g["per_run"] - 1, r * g["per_run"]]
    return out


def place(s, g, prns, seed, min_freq=None, phi_start=0, extra_bins=()):
    """One satellite per PRN index of `prns`, by bin.  Returns rows of dict(prn, bin, off (fraction of a step), doppler,
    phase, protected): edge bins, cut bins, one bin per phi row (from row phi_start on, as far as the PRNs reach), a
    second bin in the first covered phi row (another shift), then bins spread evenly over what is left.  Bins whose
    frequency is not above min_freq are left empty (a real signal ties bins f and -f)."""
    rng = np.random.default_rng(seed)
    nb, N = g["n_bins"], s.samplesPerCode
    ok = [k for k in range(nb) if min_freq is None or g["freqs"][k] > min_freq]
    chosen, protected = [], set()

    def take(k, prot):
        if k in ok and k not in chosen and len(chosen) < len(prns):
            chosen.append(k)
            if prot:
                protected.add(k)

    take(ok[0], ok[0] == 0)
    take(nb - 1, True)
    for k in list(extra_bins) + cut_bins(g):
        take(k, True)
    if g["path"] == "shift":
        room = len(prns) - len(chosen) - (1 if g["n_phi"] >= 2 else 0)
        for j in [(phi_start + i) % g["n_phi"] for i in range(g["n_phi"])]:
            if any(g["phi_index"][k] == j for k in chosen) or room <= 0:
                continue
            cand = [k for k in ok if g["phi_index"][k] == j and k not in chosen]
            if cand:
                take(cand[int(rng.integers(len(cand)))], False)
                room -= 1
        if g["n_phi"] >= 2:      # a pair in one phi row with different shifts
            pairs = [(a, b) for a in chosen for b in chosen if a < b and g["phi_index"][a] == g["phi_index"][b]
                     and g["shift"][a] != g["shift"][b]]
            if pairs:
                protected.update(pairs[0])
            else:
                a = chosen[-1]
                cand = [k for k in ok if k not in chosen and g["phi_index"][k] == g["phi_index"][a]
                        and g["shift"][k] != g["shift"][a]]
                take(cand[len(cand) // 2], True)
                protected.add(a)
    left = [k for k in ok if k not in chosen]
    need = len(prns) - len(chosen)
    if need <= len(left):
        for i in range(need):
            take(left[int(round((i + 0.5) * len(left) / need - 0.5))], False)
    else:                        # more PRNs than bins: every bin, then bins shared by two PRNs
        chosen += left + [ok[(5 * i + 2) % len(ok)] for i in range(need - len(left))]
    assert len(chosen) == len(prns), (len(chosen), len(prns))
    order = rng.permutation(len(prns))
    spc = int(round(s.samplingFreq / s.codeFreqBasis))
    lo, hi = spc + 2, N - spc - 2
    phases = np.linspace(lo + 40, hi - 40, len(prns)).astype(int) + rng.integers(-30, 31, len(prns))
    phases = phases[rng.permutation(len(prns))]
    rows = []
    for i, k in enumerate(chosen):
        on_bin = k in (0, nb - 1) or i % 2 == 1
        off = 0.0 if on_bin else float(rng.uniform(-0.3, 0.3))
        dop = float(g["freqs"][k] + off * g["step"] - s.IF)
        rows.append(dict(prn=int(prns[order[i]]), bin=int(k), off=off, doppler=dop, phase=int(phases[i]),
                         protected=k in protected))
    # two code phases within 3 samples of the ends of [spc + 2, N - spc - 2), the low one on the lowest Doppler (it drifts later, away from spc)
    free = [r for r in rows if not r["protected"]] or rows
    neg = min(free, key=lambda r: r["doppler"])
    pos = max(free, key=lambda r: r["doppler"])
    neg["phase"] = lo + 1
    pos["phase"] = hi - 2
    return sorted(rows, key=lambda r: r["prn"])


class Case(object):
    """One search of the table.  drop: {PRN index: gap seen} of PRNs whose bin, sample or fine arg-max is within 1e-6 of
    a tie in the numpy contract and so leave the exact-index assertions (at most 2, never a protected satellite).
    no_fine: the same for the fine index alone, for satellites that are on in one window only (gates)."""

    def __init__(self, name, T, M, noncoh=False, step=None, band=14.0, fs=weak_scene.FS, if_=weak_scene.IF, prns=None,
                 offset=0, f64=False, seed=1, min_freq=None, phi_start=0, gates=(), drop=None, no_fine=None, path="shift",
                 prn_chunk=None, bin_runs=1, slow=False, env=None):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        self.prns = list(range(32)) if prns is None else list(prns)
        self.drop = dict(drop or {})
        self.no_fine = dict(no_fine or {})
        self.s = settings(fs, if_, band)
        self.g = spec.grid(self.s, T, M, noncoh, step)
        self._cache = {}

    @property
    def n_samples(self):
        return (max(11, self.T * self.M) + 1) * self.s.samplesPerCode

    def sats(self):
        if "sats" not in self._cache:
            rows = place(self.s, self.g, self.prns, self.seed, self.min_freq, self.phi_start)
            free = [r for r in rows if not r["protected"] and abs(r["phase"] - self.s.samplesPerCode // 2) < 15000]
            for (first, last), r in zip(self.gates, free):     # satellites that are on in one window only
                r["on"] = (first, last)
                r["protected"] = True
            self._cache["sats"] = rows
        return self._cache["sats"]

    def record(self):
        """int8 record of offset + n_samples samples; the search reads it from `offset` on."""
        if "rec" not in self._cache:
            fs = self.s.samplingFreq
            rows = tuple((r["prn"], CN0, r["doppler"], r["phase"], r.get("on")) for r in self.sats())
            ms = self.n_samples / fs * 1e3
            x = weak_scene.generate(ms, sats=rows, seed=1000 + self.seed, sigma=SIGMA, fs=fs, if_=self.s.IF, nav_bits=False)
            assert x.size == self.n_samples
            if self.offset:
                pad = np.random.default_rng(self.seed).integers(-20, 21, self.offset).astype(np.int8)
                x = np.concatenate((pad, x))
            self._cache["rec"] = x
        return self._cache["rec"]

    def phase_range(self, row):
        """[lo, hi] of the samples at which this satellite's code period starts inside the 1-ms blocks it is on for: its
        placed phase, moved per block by the code Doppler (weak_scene.code_drift_samples) and by what the block length
        N differs from a nominal code period; plus 1, because sample i of the reference's local code holds the chip of
        time (i + 1) ts (acquisition.py's code table) while the scene's sample i holds the chip of time (i - phase) ts."""
        fs, N = self.s.samplingFreq, self.s.samplesPerCode
        slip = fs * 1e-3 / (1.0 + row["doppler"] / weak_scene.L1) - N
        first, last = row.get("on") or (0, self.T * self.M)
        ends = [row["phase"] + 1 + first * slip, row["phase"] + 1 + last * slip]
        return min(ends), max(ends)

    def signal(self):
        return self.record()[self.offset:]

    def reference(self):
        """spec.acquire(..., details=True) of this case, over PRNs in child processes; once per process."""
        if "ref" not in self._cache:
            self._cache["ref"] = parallel_spec(self.s, self.signal(), self.T, self.M, self.noncoh, self.step, self.prns)
        return self._cache["ref"]


def _spec_worker(args):
    kw, x, T, M, noncoh, step, prns = args
    return spec.acquire(orc.OracleSettings(**kw), x, T, M, noncoh, step, prn_indices=prns, details=True)


def parallel_spec(s, x, T, M, noncoh, step, prns, workers=None):
    """spec.acquire with details over `prns`, split over spawned children (each folds the record itself; they import
    numpy only, so a test process that has a GPU open may start them)."""
    g = spec.grid(s, T, M, noncoh, step)
    per_worker = 2 * 16 * g["M"] * g["n_bins"] * s.samplesPerCode          # the folded windows and their spectra
    if workers is None:
        workers = min(MAX_WORKERS, os.cpu_count() or 1, len(prns), max(1, int(16e9 // per_worker)))
    kw = dict(samplingFreq=s.samplingFreq, IF=s.IF, acqSearchBand=s.acqSearchBand, acqThreshold=s.acqThreshold)
    parts = [list(prns[i::workers]) for i in range(workers)]
    jobs = [(kw, x, T, M, noncoh, step, part) for part in parts]
    if workers == 1:
        outs = [_spec_worker(jobs[0])]
    else:
        with multiprocessing.get_context("spawn").Pool(workers) as pool:
            outs = pool.map(_spec_worker, jobs)
    merged = dict(carrFreq=np.zeros(32), codePhase=np.zeros(32), peakMetric=np.zeros(32),
                  freqBin=np.full(32, -1, dtype=np.int64), fineIdx=np.full(32, -1, dtype=np.int64), details={})
    for part, o in zip(parts, outs):
        for k in ("carrFreq", "codePhase", "peakMetric", "freqBin", "fineIdx"):
            merged[k][part] = o[k][part]
        merged["details"].update(o["details"])
    return merged


def index_error_case(direct):
    """(settings, record, search arguments, PRN index) of a search whose strongest peak lies at code phase spc exactly,
    where the reference raises IndexError (acquisition.py:152-162: its first exclusion list then reaches index N; any other
    phase <= spc, such as 10, gives a list that stays inside the row).  One 56 dB-Hz satellite at 0 Hz Doppler placed one
    sample before spc (phase_range's + 1); control=True places it at sample 10 instead."""
    fs, if_ = (RATE2["fs"], RATE2["if_"]) if direct else (weak_scene.FS, weak_scene.IF)
    s = settings(fs, if_, 2.0)
    return s, dict(coherent_ms=2, n_windows=2, noncoh=False, bin_step_hz=None), 4


def index_error_record(s, control=False):
    spc = int(round(s.samplingFreq / s.codeFreqBasis))
    n = 12 * s.samplesPerCode
    sats = ((4, 56.0, 0.0, 10 if control else spc - 1),)
    return weak_scene.generate(n / s.samplingFreq * 1e3, sats=sats, seed=77, sigma=SIGMA, fs=s.samplingFreq, if_=s.IF)


RATE2 = dict(fs=16367600.0, if_=4130400.0)
SHUFFLED_29 = [17, 3, 28, 9, 0, 22, 13, 31, 6, 25, 11, 1, 19, 27, 8, 15, 30, 4, 21, 12, 24, 2, 29, 10, 18, 7, 26, 14, 20]
ON_WINDOWS = ((30, 32), (32, 34), (30, 32), (32, 34), (0, 2), (38, 40))   # ms: windows 15, 16, 15, 16, 0, 19 of 2 ms

CASES = [
    Case("2x2_offset", 2, 2, step=250.0, offset=12345, seed=1, prn_chunk=3),
    Case("2x2_noncoh_f64_29", 2, 2, noncoh=True, step=250.0, f64=True, prns=SHUFFLED_29, seed=2, prn_chunk=3),
    Case("10x2_ref", 10, 2, seed=3, gates=((0, 10), (10, 20)), prn_chunk=1, bin_runs=2),
    Case("10x2_noncoh", 10, 2, noncoh=True, seed=4, phi_start=10, prn_chunk=1, bin_runs=2),
    Case("2x20_windows", 2, 20, band=5.0, seed=5, gates=ON_WINDOWS, prn_chunk=1, bin_runs=2),
    Case("20x2_a", 20, 2, step=25.0, band=10.0, seed=6, gates=((0, 20), (20, 40)), prn_chunk=1, bin_runs=2),
    Case("20x2_b", 20, 2, step=25.0, band=10.0, seed=7, phi_start=28, prn_chunk=1, bin_runs=2),
    Case("5x64_noncoh", 5, 64, noncoh=True, band=2.0, prns=range(16), seed=8, prn_chunk=1, bin_runs=5),
    Case("rate2_4x2_ref", 4, 2, band=6.0, seed=9, path="direct", prn_chunk=20, **RATE2),
    Case("rate2_4x2_noncoh", 4, 2, noncoh=True, band=6.0, seed=10, path="direct", prn_chunk=20, **RATE2),
    Case("fs5456_2x3", 2, 3, fs=5456000.0, if_=1364000.0, seed=11, path="direct", prn_chunk=11),
    Case("if3000_2x2", 2, 2, step=250.0, if_=3000.0, prns=range(0, 32, 2), seed=12, min_freq=4000.0, prn_chunk=3),
]
BY_NAME = {c.name: c for c in CASES}
