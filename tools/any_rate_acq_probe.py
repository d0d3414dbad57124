"""Time what a sampling rate that does not factor costs the acquisition (csrc/sgx_acq.hip, acquire_passes on a padded
length): the 32-PRN search at a rate whose samplesPerCode has a prime factor above 31 against the same search, same
build, at the nearest rate that factors into 2..31 and so runs on its own length.  Default pairs: 53 / 52.8 Msps and
5.714 / 5.456 Msps with the reference's 2 x 1 ms search, and 53 / 52.8 Msps with the 10 x 1 ms non-coherent sum.  The
record is the default synthetic scene's eight satellites at each rate (IF = fs / 4, code starts spread over the period).
Prints one JSON line per pair: transform lengths, device time per call (sgx_get_timing: HIP events on the context's
stream), min / median over --reps calls after one warm-up, and the ratio of the medians.

    python tools/any_rate_acq_probe.py [--reps 10]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = [(53000000.0, 52800000.0, 2, False), (5714000.0, 5456000.0, 2, False), (53000000.0, 52800000.0, 10, True)]


def scene(m, fs, n):
    """The default scene's satellites with code starts spread over the period, away from its ends (a peak at a code phase
    of exactly the samples per chip is the reference's IndexError, which the default starts meet at 5.714 Msps)."""
    prns = [1, 3, 7, 11, 14, 19, 22, 31]
    dop = [1250, -3100, 4800, -650, 2900, -4400, 350, -1900]
    starts = [(k + 1) * n // 9 + 17 for k in range(8)]
    return m.synth.Scene.make(0x5EED0001, fs, fs / 4.0, prns, dop, starts, [8, 7, 6, 7, 8, 6, 7, 6])


def time_search(m, fs, n_blocks, noncoh, reps):
    s = m.Settings()
    s.samplingFreq, s.IF = fs, fs / 4.0
    n = s.samplesPerCode
    ms = 10 + n_blocks
    ctx = m.engine.get_context(s, 0)
    rec = ctx.synth(scene(m, fs, n), m.synth.record_length(n, ms))
    dev = []
    r = None
    for i in range(reps + 1):
        r = ctx.acquire(rec, 0, ms * n, list(range(32)), n_blocks=n_blocks, noncoh=noncoh)
        if i:   # (the first call allocates and plans)
            dev.append(ctx.timing()["acquire_ms"])
    rec.free()
    return dict(fs=fs, n_code=n, fft_length=m._native.acquire_fft_length(n), device_ms_min=min(dev),
                device_ms_median=float(np.median(dev)), detected=[int(p) + 1 for p in np.flatnonzero(r["carrFreq"] > 0)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    importlib.import_module("__graft_entry__").build()
    m = importlib.import_module("softgnss-python_amd")
    for fs_pad, fs_own, n_blocks, noncoh in PAIRS:
        pad = time_search(m, fs_pad, n_blocks, noncoh, a.reps)
        own = time_search(m, fs_own, n_blocks, noncoh, a.reps)
        print(json.dumps(dict(kind="any_rate_acq", n_blocks=n_blocks, noncoh=noncoh, reps=a.reps, padded=pad, own_length=own,
                              ratio_median=pad["device_ms_median"] / own["device_ms_median"])), flush=True)


if __name__ == "__main__":
    main()
