"""Child process of tests/test_trk3_cases_gpu.py: the cases of the speculative tracking kernel on the default scene, tracked
in a fresh process whose environment the parent chose (SGX_TRK3_GENERIC, SGX_TRK_PROFILE, SGX_TRK_TEST_SCATTER), every
series saved into one .npz.  argv: output path, then the names of the cases to run (default: all)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

MS = 60
CASES = ("int8", "uint8", "stream", "ch3", "ms1", "golden4", "short")


def run(m, names):
    """{case: series, case + '_done': ms_done, case + '_info': (kernel, members, streamed)} of the cases named."""
    from conftest import load_golden, scene_from_json
    g = load_golden("trk_default.npz")
    s = m.Settings()
    s.numberOfChannels = 8
    s.msToProcess = float(MS)
    n = s.samplesPerCode
    rec8 = m.synth.generate(scene_from_json(g["scene"]), m.synth.record_length(n, MS))
    ctx = m.engine.get_context(s, 0)
    rec = ctx.upload(rec8)
    acq = m.AcquisitionResult(s, device=0)
    acq.acquire(m.DeviceSignal(rec, 0, 11 * n))
    acq.preRun()
    ch = acq.channels
    assert int(np.sum(ch.PRN != 0)) == 8, ch.PRN
    chans = [(int(ch.PRN[i]), float(ch.acquiredFreq[i]), float(ch.codePhase[i])) for i in range(8)]
    out = {}

    def keep(name, series, done):
        t = ctx.timing()
        out[name], out[name + "_done"] = series, done
        out[name + "_info"] = np.array([t["track_kernel"], t["track_members"], t["track_streamed"]])

    for name in names:
        if name == "int8":
            keep(name, *ctx.track(rec, chans, MS))
        elif name == "ch3":      # (a launch padded to eight channels)
            keep(name, *ctx.track(rec, chans[:3], MS))
        elif name == "ms1":      # (block 0 alone: the direct path, no pass ever used)
            keep(name, *ctx.track(rec, chans, 1))
        elif name == "uint8":
            ru = ctx.upload_bytes((rec8.astype(np.int16) + 128).astype(np.uint8))
            keep(name, *ctx.track(ru, chans, MS, data_type=m._native.DT_UINT8))
            ru.free()
        elif name == "stream":
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "record.bin")
                rec8.tofile(path)
                r = ctx.open_file(path, 0, rec8.size)
                keep(name, *ctx.track(r, chans, MS))   # starts while the file is still being read
                r.wait()
                r.free()
        elif name == "golden4":  # the channel table of the reference's own run (tests/golden/trk_default.npz)
            gch = [(int(g["ch_PRN"][i]), float(g["ch_acquiredFreq"][i]), float(g["ch_codePhase"][i])) for i in range(4)]
            keep(name, *ctx.track(rec, gch, MS))
        elif name == "short":    # a record that ends inside the run (tests/golden/trk_short.npz): results stay unset
            gs = load_golden("trk_short.npz")
            s4 = m.Settings()
            s4.numberOfChannels = 4
            s4.msToProcess = float(int(g["ms"]))
            a4 = m.AcquisitionResult(s4, device=0)
            a4._channels = np.rec.fromarrays([g["ch_PRN"], g["ch_acquiredFreq"], g["ch_codePhase"], ['T'] * 4],
                                             names='PRN,acquiredFreq,codePhase,status')
            t4 = m.TrackingResult(a4, device=0)
            full = m.synth.generate(scene_from_json(g["scene"]), int(gs["n_samples"]))
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "short.bin")
                full.tofile(path)
                fid = open(path, "rb")
                ret = t4.track(fid)
                out["short"] = np.array([ret is None, t4._results is None, fid.closed])
        else:
            raise SystemExit("unknown case %r" % name)
    rec.free()
    return out


if __name__ == "__main__":
    import importlib
    np.savez(sys.argv[1], **run(importlib.import_module("softgnss-python_amd"), sys.argv[2:] or CASES))
