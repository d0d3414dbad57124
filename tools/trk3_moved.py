"""(diagnosis) What a block costs the speculative tracking kernel when its final pass finds it somewhere else than its pass
had put it: runs the headline step (8 channels x 37 000 ms, default scene) with the -DT3_MOVED builds of csrc/sgx_trk3.hip
and prints, per channel, the moved blocks' share, their release-to-release period against the plain blocks', and the
ceiling of any change to the moved route, share x (moved period - plain period); with the -DT3_MOVED=2 build also the map
waves' release -> publish times by class.  Build first, where the compiler is:
    bash tools/build_variant.sh mv1 sgx_trk3.hip "-DT3_MOVED=1";  bash tools/build_variant.sh mv2 sgx_trk3.hip "-DT3_MOVED=2"
then on the GPU box:  python3 tools/trk3_moved.py [variant ...]   (default: mv1 mv2)
"""
import os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
per = re.compile(r"\[t3 moved\] ch (\d+) set (\d): plain (\d+) blocks, period ([\d.]+) \| moved (\d+) blocks, period ([\d.]+) \| other (\d+) blocks, period ([\d.]+)")
for name in sys.argv[1:] or ["mv1", "mv2"]:
    lib = os.path.join(ROOT, "softgnss-python_amd", "lib", "variants", "libsgx_%s.so" % name)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "step_profile.py"), "37000"], env=dict(os.environ, SGX_LIB=lib),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode(errors="replace")
    print("== variant %s: %s" % (name, next((l for l in out.splitlines() if l.startswith("step ")), "no step line")))
    rows = {}
    for m in per.finditer(out):
        rows[(int(m.group(1)), int(m.group(2)))] = [float(x) for x in m.groups()[2:]]
    lines = sorted(l for l in out.splitlines() if l.startswith("[t3 moved]"))
    print("\n".join(lines))
    worst = None
    for ch in sorted({k[0] for k in rows}):
        n = [sum(rows[(ch, s)][i] for s in (0, 1) if (ch, s) in rows) for i in (0, 2, 4)]
        t = [sum(rows[(ch, s)][i] * rows[(ch, s)][i + 1] for s in (0, 1) if (ch, s) in rows) / max(n[i // 2], 1.0) for i in (0, 2, 4)]
        share = n[1] / max(sum(n), 1.0)
        mean = sum(a * b for a, b in zip(n, t)) / max(sum(n), 1.0)
        print("ch %d: %5d moved blocks of %d (%.2f %%), period plain %.1f moved %.1f other %.1f (%d blocks) all %.1f cycles; ceiling "
              "%.1f cycles per block = %.2f %%" % (ch, n[1], sum(n), 100 * share, t[0], t[1], t[2], n[2], mean, share * (t[1] - t[0]),
                                                 100 * share * (t[1] - t[0]) / mean))
        if worst is None or n[1] > worst[1]:
            worst = (ch, n[1])
    if worst:
        print("the channel with the most moved blocks: %d (%d)" % worst)
