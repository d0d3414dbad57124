"""Telling a chip-boundary tie from a defect when a tracking kernel is compared with the oracle over a long record.

The correlator sums are piecewise constant in the code phase, so an implementation whose code phase differs from the
reference's by 1e-12 chips computes the same sums - until a sample lies that close to a chip boundary and falls on the other
side.  follow() steps the oracle (oracle.softgnss_oracle.TrackStepper) next to a kernel's series
and, at the first block that disagrees, accepts exactly one explanation: one or two samples of that block within D chips
of a boundary IN THE ORACLE'S OWN ARITHMETIC on the other side, which must reproduce every judged series of the block; it
then goes on from the flipped state.  Anything else is a defect.

Shared by tests/test_tie_follow_host.py, tests/test_tie_follow_gpu.py and the tools (which import from here: tests never
import from tools/)."""
import itertools
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np

from oracle import softgnss_oracle as orc   # checker only

# the ties measured so far lie 3.4e-13, 4.9e-12 and 6.8e-12 chips from their boundary
D_CHIPS = 1e-11
# the bar of test_full_config3_run_against_the_oracle for the sums (measured without a tie: 4.2e-11 at most), and its two
# bars for the rates
TIGHT = 1e-9
CODE_FREQ_TOL = 1e-8      # Hz
CARR_FREQ_TOL = 1e-7      # Hz
# a condition, not a measurement: a widened D or a sloppy match must not certify a broken kernel block by block
MAX_TIES = 2
MAX_TIES_SCENE = 4
CHECKPOINT_EVERY = 500    # blocks between the stepper states a plain run keeps
FS = 38.192e6


def random_scene(m, seed):
    """Eight satellites with random PRNs, Dopplers, code phases and amplitudes (scene seed != the default's)."""
    rng = np.random.default_rng(seed)
    prns = sorted(rng.choice(np.arange(1, 33), size=8, replace=False).tolist())
    return m.synth.Scene.make(0x50AC0000 + seed, 38192000.0, 9548000.0, prns,
                              [float(rng.uniform(-6500, 6500)) for _ in prns],
                              [int(rng.integers(0, 38192)) for _ in prns], [int(rng.integers(5, 10)) for _ in prns])


def rem_at(x, k_end, fs=FS):
    """remCodePhase at the start of block k_end and the code rate used in it, from a channel's recorded series x[13, ms]
    (absoluteSample, codeFreq), with the reference's own arithmetic."""
    pos = np.concatenate([[x[0, 0] - 38192.0], x[0]])
    rem, cf = 0.0, 1.023e6
    for k in range(k_end):
        blk = int(pos[k + 1] - pos[k])
        step = cf / fs
        stp = ((blk * step + rem) - rem) / blk
        rem = ((blk - 1) * stp + rem) + step - 1023.0
        cf = x[1, k]
    return rem, cf


def nearest_boundary(rem, cf, fs=FS):
    """min over samples and arms of the distance from a sample's code phase to an integer (a chip boundary of ceil)."""
    step = cf / fs
    blk = int(np.ceil((1023.0 - rem) / step))
    best = (1.0, None, None)
    for arm, off in (("E", -0.5), ("L", 0.5), ("P", 0.0)):
        t = np.linspace(rem + off, blk * step + rem + off, blk, endpoint=False)
        d = np.abs(t - np.round(t))
        i = int(np.argmin(d))
        if d[i] < best[0]:
            best = (float(d[i]), arm, i)
    return best


def stepper(record, channel, settings):
    """The oracle's stepper for channel = (PRN, acquiredFreq, codePhase) of a host record."""
    prn, freq, phase = channel
    return orc.TrackStepper(settings, prn, freq, phase, record)


def plain_run(record, channel, settings, ms, every=CHECKPOINT_EVERY):
    """The unforked oracle: -> (series [13, ms], {block: stepper state at its start} every `every` blocks)."""
    st = stepper(record, channel, settings)
    out = np.zeros((orc.NUM_SERIES, ms))
    marks = {}
    for k in range(ms):
        if k % every == 0:
            marks[k] = st.state()
        row = st.step()
        if row is None:
            raise ValueError("the record ends in block %d" % k)
        out[:, k] = row
    return out, marks


def plain_channel(args):
    """plain_run for a process pool: args = (host record, channel, ms[, settings])."""
    host, channel, ms = args[:3]
    so = args[3] if len(args) > 3 else orc.OracleSettings(numberOfChannels=1, msToProcess=float(ms))
    return plain_run(host, channel, so, ms)


def eligible_blocks(record, channel, settings, ms, dist=D_CHIPS):
    """[(block, arm, n, distance)] along the UNFORKED oracle trajectory: every sample within `dist` chips of a chip
    boundary (and not on it).  The count behind the caps of MAX_TIES."""
    st = stepper(record, channel, settings)
    out = []
    for k in range(ms):
        out += [(k, arm, n, d) for arm, n, d in st.eligible(dist)]
        if st.step() is None:
            raise ValueError("the record ends in block %d" % k)
    return out


def _scale(want):
    """max(1, RMS sqrt(I_P^2 + Q_P^2)) of the channel's oracle series: the project's measure (_trk_err)."""
    return max(1.0, float(np.sqrt(np.mean(want[3] ** 2 + want[7] ** 2))))


def _errors(got, want, scale):
    """Per block, for got / want of shape [13] or [13, blocks]: (absoluteSample equal, max |delta| of the six sums over
    scale, |delta codeFreq|, |delta carrFreq|, max |delta| of the four discriminator / filter series)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (got[0] == want[0], np.max(np.abs(got[3:9] - want[3:9]), axis=0) / scale, np.abs(got[1] - want[1]),
                np.abs(got[2] - want[2]), np.max(np.abs(got[9:13] - want[9:13]), axis=0))


def _within(e, tight):
    # (written so that a NaN is beyond every bar)
    return e[0] & (e[1] < tight) & (e[2] < CODE_FREQ_TOL) & (e[3] < CARR_FREQ_TOL)


class _Worst(object):
    """Largest errors seen over blocks that needed no flip."""
    def __init__(self):
        self.iq = self.code_freq = self.carr_freq = self.discr = 0.0

    def add(self, e):
        self.iq = max(self.iq, float(np.max(e[1], initial=0.0)))
        self.code_freq = max(self.code_freq, float(np.max(e[2], initial=0.0)))
        self.carr_freq = max(self.carr_freq, float(np.max(e[3], initial=0.0)))
        self.discr = max(self.discr, float(np.max(e[4], initial=0.0)))

    def as_dict(self):
        return dict(max_rel_err_IQ=self.iq, max_abs_err_codeFreq_Hz=self.code_freq, max_abs_err_carrFreq_Hz=self.carr_freq,
                    max_abs_err_discriminators=self.discr)


def follow(got, record, channel, settings, D=D_CHIPS, tight=TIGHT, max_ties=MAX_TIES, plain=None):
    """Judge one channel's kernel series got[13, ms] against the oracle, following chip-boundary ties.

    Every block: absoluteSample exactly, the six correlator sums within `tight` of max(1, RMS |P|) of the unforked oracle
    series, codeFreq within 1e-8 Hz, carrFreq within 1e-7 Hz; the discriminator / filter series are reported only.  A block
    beyond that is redone with each eligible sample (0 < distance to a chip boundary <= D in the oracle's own ramps) on
    the other side, and each pair if there are two or three; the first choice that brings ALL judged series of the block
    within the bars is adopted and the oracle goes on from the flipped state.  No such choice, no eligible sample, or more
    than max_ties adopted blocks (a tie is one block's adopted choice, as DESIGN.md section 2 counts them: the early and
    the late ramp lie exactly one chip apart, so a sample can be near a boundary in both and cross in both - one tie,
    listed once per arm): a defect.  absoluteSample gets no special case after a fork.

    plain   (series, marks) of plain_run() for this channel if the caller has it (it is the same for every kernel layout
            run on the record); made here otherwise.  Blocks before the first disagreement are judged against it in one
            vectorised pass; the stepper starts from the last mark before that block, so a channel is never re-run from
            block 0 more than once.
    -> report: verdict ('identical' | 'ties' | 'defect'), ties (block, arm, n, distance_chips, sample_value,
       step_in_sums, step_over_scale; one entry per flipped sample), tie_blocks (the number the cap counts), first_offending (block, kernel and oracle values, errors, eligible samples, why),
       blocks_checked, absoluteSample_identical, the largest errors over blocks that needed no flip (before / after the
       first fork).
    """
    got = np.asarray(got, dtype=np.float64)
    ms = got.shape[1]
    if plain is None:
        plain = plain_run(record, channel, settings, ms)
    want, marks = plain
    scale = _scale(want)
    report = dict(verdict="identical", channel=tuple(channel), ties=[], tie_blocks=0, first_offending=None, blocks_checked=ms,
                  absoluteSample_identical=True, scale=scale, D=D, tight=tight, max_ties=max_ties)
    before_fork, after_fork = _Worst(), _Worst()

    def done():
        report["unflipped"] = before_fork.as_dict()
        report["unflipped_after_first_tie"] = after_fork.as_dict() if report["ties"] else None
        return report

    e = _errors(got, want[:, :ms], scale)
    bad = np.nonzero(~_within(e, tight))[0]
    k0 = int(bad[0]) if bad.size else ms
    before_fork.add([x[:k0] for x in e])
    if k0 == ms:
        return done()

    st = stepper(record, channel, settings)
    b = max(k for k in marks if k <= k0)
    st.restore(marks[b])
    for _ in range(b, k0):
        st.step()
    for k in range(k0, ms):
        before = st.state()
        row = st.step()
        e = _errors(got[:, k], row, scale) if row is not None else None
        if e is not None and _within(e, tight):
            (after_fork if report["ties"] else before_fork).add(e)
            continue
        # a block beyond the bars: only a tie may explain it
        st.restore(before)
        elig = st.eligible(D)
        raw = st.samples(st.ramps()[1])
        cands = [(c,) for c in elig]
        if 2 <= len(elig) <= 3:
            cands += list(itertools.combinations(elig, 2))
        adopted = None
        for cand in cands:
            st.restore(before)
            try:
                flipped = st.step([(arm, n) for arm, n, _ in cand])
            except ValueError:
                continue
            if flipped is not None and _within(_errors(got[:, k], flipped, scale), tight):
                adopted = cand
                break
        why = None
        if not elig:
            why = "no sample of the block lies within D of a chip boundary"
        elif adopted is None:
            why = "no flip of an eligible sample explains the block"
        elif report["tie_blocks"] + 1 > max_ties:
            why = "more than max_ties ties in one channel"
        if why is not None:
            report.update(verdict="defect", blocks_checked=k, absoluteSample_identical=False,    # (not established)
                          first_offending=dict(block=k, why=why, kernel=[float(v) for v in got[:, k]],
                                               oracle=None if row is None else [float(v) for v in row],
                                               absoluteSample_equal=None if e is None else bool(e[0]),
                                               rel_err_IQ=None if e is None else float(e[1]),
                                               abs_err_codeFreq_Hz=None if e is None else float(e[2]),
                                               abs_err_carrFreq_Hz=None if e is None else float(e[3]),
                                               eligible=len(elig), nearest_eligible=elig[:6]))
            return done()
        step = float(np.max(np.abs(np.asarray(flipped[3:9]) - np.asarray(row[3:9]))))
        for arm, n, d in adopted:
            report["ties"].append(dict(block=k, arm=arm, n=n, distance_chips=d, sample_value=float(raw[n]),
                                       step_in_sums=step, step_over_scale=step / scale))
        report["verdict"] = "ties"
        report["tie_blocks"] += 1
        # (the stepper stands after the flipped block)
    return done()


def diverges(got, plain, tight=TIGHT):
    """Whether any block of got[13, ms] is beyond the bars of the channel's plain oracle series (then follow() has blocks
    to redo; otherwise it returns at once)."""
    want = plain[0]
    return not bool(np.all(_within(_errors(got, want[:, :np.shape(got)[1]], _scale(want)), tight)))


def _follow_job(args):
    got, host, channel, settings, D, tight, max_ties, plain = args
    return follow(got, host, channel, settings, D, tight, max_ties, plain)


def follow_scene(got, host, chans, settings, plains, D=D_CHIPS, tight=TIGHT, max_ties=MAX_TIES, workers=8):
    """follow() for every channel of a scene: got [channels, 13, ms], plains from plain_channel.  Channels that never leave
    the bars are judged here; the others go to a process pool of at most `workers` (each re-runs at most one stretch)."""
    reports = [None] * len(chans)
    todo = [c for c in range(len(chans)) if diverges(got[c], plains[c], tight)]
    for c in range(len(chans)):
        if c not in todo:
            reports[c] = follow(got[c], None, chans[c], settings, D, tight, max_ties, plains[c])
    if todo:
        with ProcessPoolExecutor(max_workers=max(1, min(workers, len(todo), os.cpu_count() or 1))) as ex:
            jobs = [(got[c], host, chans[c], settings, D, tight, max_ties, plains[c]) for c in todo]
            for c, r in zip(todo, ex.map(_follow_job, jobs)):
                reports[c] = r
    return reports


def describe(report):
    """A report as text (what a failed test prints)."""
    lines = ["channel %r: %s, %d blocks checked, scale %.6g, D %.3g, tight %.3g" % (
        report["channel"], report["verdict"], report["blocks_checked"], report["scale"], report["D"], report["tight"])]
    for t in report["ties"]:
        lines.append("  tie: block %(block)d arm %(arm)s sample %(n)d, %(distance_chips).3g chips from a boundary, x = %(sample_value)g, "
                     "sums step by %(step_in_sums).6g (%(step_over_scale).3g of scale)" % t)
    lines.append("  blocks without a flip: %r" % (report["unflipped"],))
    if report["unflipped_after_first_tie"] is not None:
        lines.append("  ... after the first tie: %r" % (report["unflipped_after_first_tie"],))
    f = report["first_offending"]
    if f is not None:
        lines.append("  first offending block %(block)d: %(why)s; absoluteSample equal %(absoluteSample_equal)r, I/Q %(rel_err_IQ)r, "
                     "codeFreq %(abs_err_codeFreq_Hz)r Hz, carrFreq %(abs_err_carrFreq_Hz)r Hz; %(eligible)d eligible, nearest %(nearest_eligible)r" % f)
        lines.append("    kernel %r" % (f["kernel"],))
        lines.append("    oracle %r" % (f["oracle"],))
    return "\n".join(lines)
