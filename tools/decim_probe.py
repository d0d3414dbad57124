"""Times of the decimator's kernel (csrc/sgx_decim.hip: sgx_if_decimate) on one GPU beside its two yardsticks, and what a
decimated record saves the stages behind it:

    python tools/decim_probe.py [--ms 37000] [--calls 10] [--no-stage] [--no-gain]

The input is the default scene's record of --ms code periods (37 000: the 1.4 GB record of the benchmark), read as a real
record (lanes 1) and as interleaved I/Q (lanes 2).  One warm-up call, then --calls timed calls; HIP events on the context's
stream around the kernel.  Prints one JSON line with the read and copy rates sgx_stream_rates measures on the same GPU and,
per filter length, the tera-MAC/s sgx_if_filter reaches on the same record (N L MACs); then one line per
(lanes, D, L): min and median in ms, the time of bytes read + written at the copy rate, the time of the useful MACs
(N / D L for a real record, twice that for I/Q: four real MACs per complex one on half as many frames) at the notch's rate,
which of the two bounds the configuration, and the share of that bound the kernel reaches.

Then (unless --no-gain) the default record beside itself decimated by 5 (7.6384 Msps, IF 1.9096 MHz): the 32-PRN
acquisition, 8 channels tracked in latency mode per code period, and the many-channel throughput leg."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FACTORS = (2, 3, 4, 5, 8)
LENGTHS = (31, 127, 511)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", type=int, default=37000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--gain-ms", type=int, default=2000, help="code periods tracked in the comparison")
    ap.add_argument("--many-channels", type=int, default=3072)
    ap.add_argument("--no-stage", action="store_true")
    ap.add_argument("--no-gain", action="store_true")
    a = ap.parse_args()
    m = importlib.import_module("softgnss-python_amd")
    n = m._native
    s = m.Settings()
    ctx = m.engine.get_context(s, 0)
    scene = m.synth.Scene.default()
    rng = np.random.default_rng(7)
    if not a.no_stage:
        n_in = m.synth.record_length(s.samplesPerCode, a.ms)
        n_in -= n_in % 64
        rec = ctx.synth(scene, n_in)
        read_gbs, copy_gbs = ctx.stream_rates()
        notch = {}
        for L in LENGTHS:
            h = rng.integers(-1000, 1001, L).astype(np.int16)
            ms = []
            for i in range(a.calls + 1):
                ctx.filter_record(rec, h, 14).free()
                if i:
                    ms.append(ctx.filter_timing())
            notch[L] = n_in * L / min(ms) / 1e9                       # tera-MAC/s
        print(json.dumps(dict(in_bytes=n_in, read_GBps=round(read_gbs, 1), copy_GBps=round(copy_gbs, 1),
                              notch_TMACps={str(L): round(v, 1) for L, v in notch.items()})), flush=True)
        for lanes in (1, 2):
            for D in FACTORS:
                for L in LENGTHS:
                    h = rng.integers(-1000, 1001, lanes * L).astype(np.int16)
                    ms = []
                    for i in range(a.calls + 1):
                        out = ctx.decimate(rec, lanes, h, 14, D)
                        n_out = len(out)
                        out.free()
                        if i:
                            ms.append(ctx.decim_timing())
                    copy_ms = (n_in + n_out) / copy_gbs / 1e6
                    macs = n_in / float(D) * L * (2 if lanes == 2 else 1)
                    mac_ms = macs / notch[L] / 1e9
                    bound = "copy" if copy_ms >= mac_ms else "mac"
                    print(json.dumps(dict(kernel="decim_kernel", lanes=lanes, D=D, taps=L, calls=a.calls,
                                          kernel_ms_min=round(min(ms), 3), kernel_ms_median=round(float(np.median(ms)), 3),
                                          copy_ms=round(copy_ms, 3), mac_ms=round(mac_ms, 3), bound=bound,
                                          TMACps=round(macs / min(ms) / 1e9, 1),
                                          share_of_bound=round(max(copy_ms, mac_ms) / min(ms), 3))), flush=True)
        rec.free()
    if a.no_gain:
        return
    # what the stage buys: the default record beside itself at D = 5
    s5 = m.Settings()
    s5.decimation = 5
    real = s5._prepared_settings()
    ctx5 = m.engine.get_context(real, 0)
    n_rec = m.synth.record_length(s.samplesPerCode, a.gain_ms)
    n_rec -= n_rec % 320
    rec = ctx.synth(scene, n_rec)
    ctx.sync()
    taps, shift, info = s5._decim_design()
    dec = ctx5.decimate(rec, 1, taps, shift, 5)          # (the decimated record belongs to the context that reads it)
    print(json.dumps(dict(record="default at D = 5", fs_out=info["fs_out"], f_out=info["f_out"], inverted=info["inverted"],
                          clipped=dec.clipped / float(len(dec)), kernel_ms=round(ctx5.decim_timing(), 3))), flush=True)
    for name, c, st, r in (("default", ctx, s, rec), ("D = 5", ctx5, real, dec)):
        spc = st.samplesPerCode
        acq = m.AcquisitionResult(st, device=0)
        t_acq = []
        for i in range(4):
            acq = m.AcquisitionResult(st, device=0)
            acq.acquire(m.DeviceSignal(r, 0, 11 * spc))
            if i:
                t_acq.append(c.timing()["acquire_ms"])
        acq.preRun()
        ch8 = [(int(ch.PRN), float(ch.acquiredFreq), float(ch.codePhase)) for ch in acq.channels if int(ch.PRN)]
        ms = a.gain_ms - 20
        c.track(r, ch8, 50)
        c.track(r, ch8, ms)
        t8 = c.timing()["track_ms"]
        many = [ch8[i % len(ch8)] for i in range(a.many_channels)]
        many_ms = min(ms, 1000)
        c.track(r, many, 20)
        c.track(r, many, many_ms)
        tm = c.timing()["track_ms"]
        print(json.dumps(dict(record=name, samplingFreq=st.samplingFreq, satellites=len(ch8),
                              acquire_ms_min=round(min(t_acq), 3), acquire_ms_median=round(float(np.median(t_acq)), 3),
                              track8_us_per_code_period=round(1e3 * t8 / ms, 3),
                              many_channels=a.many_channels, many_ms=many_ms, many_track_ms=round(tm, 2),
                              many_kernel=int(c.timing()["track_kernel"]))), flush=True)
    dec.free()
    rec.free()


if __name__ == "__main__":
    main()
