"""Times of the unpacker's kernel (csrc/sgx_unpack.hip: sgx_if_unpack) on one GPU, and what a packed file saves on the way
in:

    python tools/unpack_probe.py [--ms 37000] [--calls 10] [--dir DIR] [--no-files]

Every configuration makes the same int8 record, the default scene's length of --ms code periods (37 000: the 1.4 GB record
of the benchmark): 1-, 2- and 4-bit samples with frames of one field, and 2-bit samples in frames of four fields of which
one is kept (one of four interleaved streams).  The input is a synthesised record of the length the configuration needs,
its bytes read as packed fields (every bit pattern is a legal field).  One warm-up call, then --calls timed calls; HIP
events on the context's stream around the kernel.  Prints one JSON line with the read and copy rates sgx_stream_rates
measures on the same GPU, then one line per configuration: min and median in ms beside the floor - (bytes read + written) /
copy rate - and the share of the floor's rate the kernel reaches.

Then (unless --no-files) the same 2-bit record and the int8 record it unpacks to are written to DIR (default: the system's
temporary directory; 1.8 GB, removed afterwards) and loaded --calls times each after one warm-up: the wall clock of
upload_file + unpack of the packed file beside upload_file of the int8 file, min and median in ms."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", type=int, default=37000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--no-files", action="store_true")
    a = ap.parse_args()
    m = importlib.import_module("softgnss-python_amd")
    n = m._native
    s = m.Settings()
    ctx = m.engine.get_context(s, 0)
    n_out = m.synth.record_length(s.samplesPerCode, a.ms)
    n_out -= n_out % 64
    read_gbs, copy_gbs = ctx.stream_rates()
    print(json.dumps(dict(out_bytes=n_out, read_GBps=round(read_gbs, 1), copy_GBps=round(copy_gbs, 1))), flush=True)
    scene = m.synth.Scene.default()
    for bits, frame, take in ((1, 1, 1), (2, 1, 1), (4, 1, 1), (2, 4, 1)):
        n_in = n_out * bits * frame // (8 * take)
        rec = ctx.synth(scene, n_in)
        table = n.unpack_table(bits, "sign-magnitude", 48)
        ms = []
        for i in range(a.calls + 1):
            out = ctx.unpack(rec, bits, table, frame=frame, first=0, take=take)
            assert len(out) == n_out and int(out.code_counts.sum()) == n_out
            out.free()
            if i:
                ms.append(ctx.unpack_timing())
        floor = (n_in + n_out) / copy_gbs / 1e6
        print(json.dumps(dict(kernel="unpack_kernel", bits=bits, frame=frame, take=take, in_bytes=n_in, calls=a.calls,
                              kernel_ms_min=round(min(ms), 3), kernel_ms_median=round(float(np.median(ms)), 3),
                              floor_ms=round(floor, 3), share_of_floor_rate=round(floor / min(ms), 3))), flush=True)
        rec.free()
    if a.no_files:
        return
    d = tempfile.mkdtemp(prefix="unpack_probe_", dir=a.dir)
    packed, plain = os.path.join(d, "packed2.bin"), os.path.join(d, "int8.bin")
    try:
        table = n.unpack_table(2, "sign-magnitude", 48)
        rec = ctx.synth(scene, n_out // 4)
        out = ctx.unpack(rec, 2, table)
        rec.download().tofile(packed)
        out.download().tofile(plain)
        out.free()
        rec.free()
        t_packed, t_plain = [], []
        for i in range(a.calls + 1):
            t0 = time.perf_counter()
            r = ctx.upload_file(packed, 0, n_out // 4)
            o = ctx.unpack(r, 2, table)
            t1 = time.perf_counter()
            r.free()
            o.free()
            t2 = time.perf_counter()
            r = ctx.upload_file(plain, 0, n_out)
            t3 = time.perf_counter()
            r.free()
            if i:
                t_packed.append(1e3 * (t1 - t0))
                t_plain.append(1e3 * (t3 - t2))
        print(json.dumps(dict(load="upload_file + unpack, 2-bit file", file_bytes=n_out // 4, calls=a.calls,
                              wall_ms_min=round(min(t_packed), 2), wall_ms_median=round(float(np.median(t_packed)), 2))),
              flush=True)
        print(json.dumps(dict(load="upload_file, int8 file", file_bytes=n_out, calls=a.calls,
                              wall_ms_min=round(min(t_plain), 2), wall_ms_median=round(float(np.median(t_plain)), 2))),
              flush=True)
    finally:
        for p in (packed, plain):
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(d)


if __name__ == "__main__":
    main()
