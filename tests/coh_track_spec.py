"""The numpy contract of bit-aligned coherent tracking (sgx_track_coherent, csrc/sgx_trk_coh.hip).

Every block is the reference's block (oracle.softgnss_oracle.TrackStepper: its own length from remCodePhase and codeFreq,
the three linspace ramps, a carrier that runs on through remCarrPhase, the six sums).  Only WHEN the loops are updated
changes: after a pull-in of P blocks with the reference's 1 ms updates the loops are handed a smoothed NCO value and then
updated once per group of T blocks, aligned with the navigation bit's edge, from the sums of the group.

    T       1, 2, 4, 5, 10 or 20 ms per group (1: never, the whole run is the reference's)
    P       pull-in length in blocks
    H       hand-over window, 1 .. 1000 blocks
    edge    per channel: -1 (find it during the pull-in) or 0 .. 19, the block number mod 20 at which a bit starts

track() returns, per channel of the table (off channels, PRN 0, keep the pre-fill): the 13 series of the reference with
the meaning stated in include/sgx.h, ms_done, the edge, k0 (-1 where the coherent phase has no start) and the 20 energies
of the bit synchronisation.
"""
import numpy as np

from oracle import softgnss_oracle as orc

COHERENT_MS = (1, 2, 4, 5, 10, 20)
_ZERO = ("absoluteSample", "I_P", "I_E", "I_L", "Q_E", "Q_P", "Q_L")


def first_group_start(P, edge):
    """k0: the smallest block k >= P with (k - edge) % 20 == 0."""
    return int(P) + (int(edge) - int(P)) % 20


class CohStepper(orc.TrackStepper):
    """One channel.  step() runs one block and returns its row of the 13 series, or None where the channel has ended
    (a short read, or the block behind an update whose six sums were all zero)."""

    def __init__(self, s, prn, acquired_freq, code_phase, record, T, P, H, edge, ms, coh_pll_bw, coh_dll_bw):
        orc.TrackStepper.__init__(self, s, prn, acquired_freq, code_phase, record)
        if T not in COHERENT_MS or not 1 <= H <= 1000 or not -1 <= edge <= 19:
            raise ValueError("T, H or edge outside the contract")
        self.T, self.P, self.H, self.ms = int(T), int(P), int(H), int(ms)
        self.edge = int(edge)
        self.find = self.edge == -1
        self.k0 = first_group_start(P, edge) if (self.edge >= 0 and T > 1) else -1
        self.t1cc, self.t2cc = orc.calc_loop_coef(coh_dll_bw, s.dllDampingRatio, 1.0)
        self.t1pc, self.t2pc = orc.calc_loop_coef(coh_pll_bw, s.pllDampingRatio, 0.25)
        self.acc = np.zeros(20, dtype=np.complex128)
        self.energy = np.zeros(20)
        self.carr_hist, self.code_hist = [], []
        self.group = np.zeros(6)          # I_P, I_E, I_L, Q_E, Q_P, Q_L of the group so far (SERIES order)
        self.shown = (np.inf,) * 4        # dllDiscr, dllDiscrFilt, pllDiscr, pllDiscrFilt of the latest update
        self.ended = False

    def _bit_sync(self, k, i_p, q_p):
        z = complex(i_p, q_p)
        for h in range(20):
            if k >= h:
                self.acc[h] += z
                if (k - h) % 20 == 19:
                    self.energy[h] += self.acc[h].real * self.acc[h].real + self.acc[h].imag * self.acc[h].imag
                    self.acc[h] = 0.0
        if k == self.P - 1:
            self.edge = int(np.argmax(self.energy))        # (the lowest h among equal maxima)
            if self.T > 1:
                self.k0 = first_group_start(self.P, self.edge)

    def _hand_over(self):
        """At the end of block k0 - 1, behind its own update: both filters restart from the mean of the last H' NCO
        values, added in ascending block order."""
        n = min(self.H, self.k0)
        for hist, nco, err in ((self.carr_hist, "old_carr_nco", "old_carr_err"), (self.code_hist, "old_code_nco", "old_code_err")):
            acc = 0.0
            for v in hist[-n:]:
                acc += v
            setattr(self, nco, acc / n)
            setattr(self, err, 0.0)
        self.carr_freq = self.carr_basis + self.old_carr_nco
        self.code_freq = self.s.codeFreqBasis - self.old_code_nco

    def _correlate(self):
        """The block of TrackStepper.step without its loop update: (position behind it, the six sums in SERIES order),
        or None on a short read."""
        s = self.s
        step, blk, t = self.ramps()
        raw = self.samples(blk)
        if raw is None:
            return None
        idx = {arm: np.ceil(t[arm]).astype(np.int64) for arm in orc.ARMS}
        self.pos += blk * self.dt.itemsize
        early, late, prompt = self.code[idx["E"]], self.code[idx["L"]], self.code[idx["P"]]
        self.rem_code = t["P"][blk - 1] + step - 1023.0
        tm = np.arange(0, blk + 1) / s.samplingFreq
        arg = self.carr_freq * 2.0 * np.pi * tm + self.rem_carr
        self.rem_carr = arg[blk] % (2 * np.pi)
        qbb = np.cos(arg[0:blk]) * raw
        ibb = np.sin(arg[0:blk]) * raw
        i_e, q_e = (early * ibb).sum(), (early * qbb).sum()
        i_p, q_p = (prompt * ibb).sum(), (prompt * qbb).sum()
        i_l, q_l = (late * ibb).sum(), (late * qbb).sum()
        self.block += 1
        return self.pos, np.array([i_p, i_e, i_l, q_e, q_p, q_l])

    def _update_group(self):
        """The reference's two discriminators of the group sums, both filters with PDI = T ms (tracking.py:223-251)."""
        pdi = self.T * 0.001
        i_p, i_e, i_l, q_e, q_p, q_l = self.group
        with np.errstate(divide="ignore", invalid="ignore"):
            carr_err = np.arctan(q_p / i_p) / 2.0 / np.pi
            carr_nco = self.old_carr_nco + self.t2pc / self.t1pc * (carr_err - self.old_carr_err) + carr_err * (pdi / self.t1pc)
            self.old_carr_nco, self.old_carr_err = carr_nco, carr_err
            self.carr_freq = self.carr_basis + carr_nco
            ee = np.sqrt(i_e * i_e + q_e * q_e)
            ll = np.sqrt(i_l * i_l + q_l * q_l)
            code_err = (ee - ll) / (ee + ll)
            code_nco = self.old_code_nco + self.t2cc / self.t1cc * (code_err - self.old_code_err) + code_err * (pdi / self.t1cc)
            self.old_code_nco, self.old_code_err = code_nco, code_err
            self.code_freq = self.s.codeFreqBasis - code_nco
        self.shown = (code_err, code_nco, carr_err, carr_nco)

    def step(self):
        if self.ended:
            return None
        k = self.block
        if self.k0 < 0 or k < self.k0:
            with np.errstate(divide="ignore", invalid="ignore"):
                row = orc.TrackStepper.step(self)
            if row is None:
                self.ended = True
                return None
            row = list(row)
            sums = row[3:9]
            self.shown = tuple(row[9:13])
            self.carr_hist.append(row[12])
            self.code_hist.append(row[10])
            if self.find and k < self.P:
                self._bit_sync(k, row[3], row[7])
            if all(v == 0.0 for v in sums):
                self.ended = True              # silence: this block is the channel's last row
            elif self.k0 == k + 1 and self.k0 < self.ms:
                self._hand_over()
                row[1], row[2] = self.code_freq, self.carr_freq
            return tuple(row)
        got = self._correlate()
        if got is None:
            self.ended = True
            return None
        pos, sums = got
        j = (k - self.k0) % self.T
        self.group = sums.copy() if j == 0 else self.group + sums
        if j == self.T - 1:
            self._update_group()
            if np.all(self.group == 0.0):
                self.ended = True
        return (pos, self.code_freq, self.carr_freq) + tuple(sums) + self.shown


def track(s, channels, record, ms, T, P, H, edges, coh_pll_bw=3.0, coh_dll_bw=1.0):
    """channels: sequence of (prn, acquiredFreq, codePhase), prn 0 = off.  -> dict(series float64[n_ch, 13, ms], ms_done,
    edge, k0 int32[n_ch], energy float64[n_ch, 20])."""
    n_ch, ms = len(channels), int(ms)
    series = np.empty((n_ch, orc.NUM_SERIES, ms))
    for j, name in enumerate(orc.SERIES):
        series[:, j, :] = 0.0 if name in _ZERO else np.inf
    done = np.zeros(n_ch, dtype=np.int32)
    edge = np.array(edges, dtype=np.int32).copy()
    k0 = np.full(n_ch, -1, dtype=np.int32)
    energy = np.zeros((n_ch, 20))
    for c, (prn, freq, phase) in enumerate(channels):
        if int(prn) == 0:
            continue
        st = CohStepper(s, prn, freq, phase, record, T, P, H, int(edges[c]), ms, coh_pll_bw, coh_dll_bw)
        for it in range(ms):
            row = st.step()
            if row is None:
                break
            series[c, :, it] = row
            done[c] = it + 1
        edge[c], k0[c], energy[c] = st.edge, st.k0, st.energy
    return dict(series=series, ms_done=done, edge=edge, k0=k0, energy=energy)
