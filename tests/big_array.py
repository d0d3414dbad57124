"""A multi-antenna record longer than 4 GiB for tests/test_array_gpu.py: tests/big_record.py's tiled record - a random block of
105 * 2^13 bytes over and over, a period that divides neither 2^31 nor 2^32 and holds whole frames of eight antennas - read as
8 real streams, with the combiner as a stage of that module (windows held to its wrap rule, the clip count of the whole from
the contract on two and three blocks) and the exact statistics the record's periodicity gives.  Test infrastructure; no GPU
code, no product import."""
import numpy as np

import array_spec as spec
import big_record as big

ANTENNAS = 8


class Combine(big.Stage):
    """sgx_if_combine on 8 real streams through K random taps each: one output byte per frame of 8 input bytes."""
    name = "combine"
    num, den, unit = 1, ANTENNAS, ANTENNAS

    def __init__(self, K=3, S=12, seed=9):
        self.h = big.taps_in_bound(np.random.default_rng(seed), ANTENNAS * K, S).reshape(ANTENNAS, K)
        self.S, self.halo = S, ANTENNAS * ((K - 1) // 2 + 1)

    def run(self, chunk, lo):
        y, clipped = spec.combine(chunk, self.h, self.S, 1, ANTENNAS)
        return y, dict(clipped=clipped)


def stats_of(rec):
    """int64 rho[8, 8, 1, 1] of the whole tiled record at K = 1, exact: the frames repeat with the block, no product
    reaches across a frame, so the record's sums are reps x the block's + those of the rest."""
    assert rec.P % ANTENNAS == 0 and rec.rest % ANTENNAS == 0
    block = spec.stats(rec.block, 1, ANTENNAS, 1)
    rest = spec.stats(rec.block[:rec.rest], 1, ANTENNAS, 1)
    return rec.reps * block + rest
