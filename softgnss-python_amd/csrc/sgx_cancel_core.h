// What the host twin (sgx_cancel.cpp, no HIP: it builds with a plain C++ compiler too) and the kernel (sgx_cancel.hip) of the
// strong-signal cancellation share: the limits, the argument checks, and the block table as the kernel reads it.
// tests/cancel_spec.py is the contract, DESIGN.md section 4.23 the account.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "sgx_check.h"

#define CN_MAX_CHANNELS 32
#define CN_MAX_SMOOTH 41
#define CN_TABLE 2048        // bytes of one channel's code laid out twice (2 x 1023 + 2), as the replay's

// One block of a cancelled channel as the kernel reads it: sgx_replay_state's block, the constants of its sample loop
// (replay_kernel's, formed once on the host) and its amplitude pair
struct CnBlock {
    long long pos;        // index in the RECORD of the block's first sample
    int blk;              // samples
    int pad;
    double start;         // rem_code: t_i = i lin + start
    double lin;           // (blk step + rem_code - rem_code) / blk, numpy's linspace step
    double cb;            // ceil(t_i) - cb indexes the doubled code table: ceil(start) - (ceil(start) - 1) mod 1023
    double w;             // carr_freq 2.0 pi
    double rem_carr;
    double rot_s, rot_c;  // (sin, cos)(w (1 / fs)): the turn of one sample
    double a_i, a_q;
    double pad2;
};
static_assert(sizeof(CnBlock) == 96, "six 16-byte loads per block");

struct CnChan {
    int done;             // blocks that are cancelled; 0 for a channel that is off
    int prn;              // 1-based, 0: off
};

// sgx_core.cpp
int sgx_host_ca_code(int prn0, int8_t* out /*1023*/);

// The checks sgx_if_cancel and sgx_cancel_host share, in this order: the pointers, n_ch, the data type, the amplitudes,
// then sgx_replay_state (whose codes come back unchanged) into state[n_ch * ms]
int cn_check(const sgx_settings* s, int64_t rec_file_offset, int64_t rec_bytes, const sgx_chan_init* ch, int32_t n_ch,
             int32_t ms, const int32_t* ms_done, const double* series, int32_t data_type, const double* amp,
             std::vector<sgx_replay_block>* state);
// The kernel's tables from the checked state: blocks[n_ch * ms], chan[n_ch]
void cn_tables(const sgx_settings* s, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch, int32_t ms,
               const int32_t* ms_done, const sgx_replay_block* state, const double* amp, CnBlock* blocks, CnChan* chan);
