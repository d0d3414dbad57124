"""Child process of tests/test_trk3_moved_blocks_gpu.py: the scene of tests/trk3_moved_scene.py tracked in a fresh process
whose environment the parent chose (SGX_TRK3_GENERIC, SGX_TRK_V3), every series saved into one .npz.
argv: output path, then the cases to run: int8 (the record as generated), uint8 (its offset-binary copy)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import trk3_moved_scene as sc


def run(m, names):
    """{case: series [8, 13, MS], case + '_done': ms_done, case + '_info': (kernel, members, streamed)}"""
    s = m.Settings()
    s.numberOfChannels = 8
    s.msToProcess = float(sc.MS)
    assert float(s.samplingFreq) == sc.FS and float(s.IF) == sc.IF
    rec8 = sc.record(m.synth)
    ctx = m.engine.get_context(s, 0)
    out = {}
    for name in names:
        if name == "int8":
            rec = ctx.upload(rec8)
            series, done = ctx.track(rec, sc.channels(), sc.MS)
        elif name == "uint8":
            rec = ctx.upload_bytes((rec8.astype(np.int16) + 128).astype(np.uint8))
            series, done = ctx.track(rec, sc.channels(), sc.MS, data_type=m._native.DT_UINT8)
        else:
            raise SystemExit("unknown case %r" % name)
        t = ctx.timing()
        out[name], out[name + "_done"] = series, done
        out[name + "_info"] = np.array([t["track_kernel"], t["track_members"], t["track_streamed"]])
        rec.free()
    return out


if __name__ == "__main__":
    import importlib
    np.savez(sys.argv[1], **run(importlib.import_module("softgnss-python_amd"), sys.argv[2:] or ("int8", "uint8")))
