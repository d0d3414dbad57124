"""Time of sgx_if_cancel's kernel (strong-signal cancellation, csrc/sgx_cancel.hip) on one GPU, and what cancelling the other
satellites gives a channel of the default scene:

    python tools/cancel_probe.py [--ms 37000] [--channels 2,8] [--calls 10] [--cno-channel 0]

The record is the default scene of --ms code periods (37 000: the 1.4 GB record of the benchmark), searched and tracked on the
GPU with 8 channels.  Per entry of --channels, that many rows are cancelled: one warm-up call, then --calls timed calls, HIP
events on the context's stream around the kernel.  Prints one JSON line each: min and median in ms next to
  copy_floor_ms   the record read and written once at the copy rate of sgx_stream_rates, measured in the same run,
and the samples clipped.  Then one line with the median C/N0 (sgx_track_quality, windows of cnoInterval ms) of channel
--cno-channel tracked alone on the raw record and on the record with the other seven cancelled: the self-interference that
DESIGN.md section 4.7 measures from the other side."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_cno(m, ctx, s, rec, chan, ms):
    series, done = ctx.track(rec, [chan], ms)
    cno = ctx.track_quality(series[:, 3], series[:, 7], m._native.lock_params(s))[0][0]
    cno = cno[np.isfinite(cno)]
    return float(np.median(cno)) if cno.size and int(done[0]) == ms else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", type=int, default=37000)
    ap.add_argument("--channels", default="2,8")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--cno-channel", type=int, default=0)
    a = ap.parse_args()
    m = importlib.import_module("softgnss-python_amd")
    s = m.Settings()
    s.msToProcess = float(a.ms)
    ctx = m.engine.get_context(s, 0)
    rec = ctx.synth(m.synth.Scene.default(), m.synth.record_length(s.samplesPerCode, a.ms))
    n = len(rec)
    acq = m.AcquisitionResult(s, device=0)
    acq.acquire(m.DeviceSignal(rec, 0, 11 * s.samplesPerCode))
    acq.preRun()
    trk = m.TrackingResult(acq, device=0)
    trk.track(m.DeviceFile(rec))
    chans = [(int(c.PRN), float(c.acquiredFreq), float(c.codePhase)) for c in acq.channels if c.PRN != 0]
    _, copy_gbs = ctx.stream_rates()
    state = m._native.replay_state(s, chans, trk.series, rec_bytes=n)
    amp = m._native.cancel_design(trk.series, state)
    for k in (int(x) for x in a.channels.split(",")):
        ker, clipped = [], 0
        for i in range(a.calls + 1):
            out = ctx.if_cancel(rec, chans[:k], trk.series[:k], amp[:k])
            clipped = out.clipped
            out.free()
            if i:
                ker.append(ctx.cancel_timing())
        print(json.dumps(dict(samples=n, ms=a.ms, channels=k, calls=a.calls, kernel_ms_min=round(min(ker), 3),
                              kernel_ms_median=round(float(np.median(ker)), 3),
                              gsamples_per_s=round(n / (min(ker) * 1e-3) / 1e9, 2),
                              ns_per_sample_channel=round(min(ker) * 1e6 / n / k, 5), copy_gbs=round(copy_gbs, 1),
                              copy_floor_ms=round(2.0 * n / (copy_gbs * 1e9) * 1e3, 3), clipped=clipped)), flush=True)
    j = a.cno_channel
    others = [i for i in range(len(chans)) if i != j]
    cleaned = trk.cancel(m.DeviceFile(rec), rows=others)
    print(json.dumps(dict(channel=j, prn=chans[j][0], ms=a.ms, cancelled_prn=cleaned.PRN,
                          median_cno_raw=round(median_cno(m, ctx, s, rec, chans[j], a.ms), 2),
                          median_cno_others_cancelled=round(median_cno(m, ctx, s, cleaned.record, chans[j], a.ms), 2),
                          cancel_kernel_ms=round(cleaned.kernel_ms, 3), clipped=cleaned.clipped)), flush=True)
    cleaned.record.free()
    rec.free()


if __name__ == "__main__":
    main()
