// Ragged blocks of the offline batch handles (nutls_process_block_ragged, nutls_enhance_block_ragged): launchers of the stage-in /
// commit kernels (ragged.hip).  Kept apart from nutls_internal.hpp: the frame-step kernels include that header and have nothing to
// do with these.  (The block transforms take the same counts as an optional argument: launch_stft_block / launch_istft_block there.)
//
// `counts` is a DEVICE array [U] of int, read by the kernels: utterance u has counts[u] real leading frames in a block whose row
// stride is n (every kernel clamps it to 0 .. n).
#pragma once

#include <hip/hip_runtime.h>

namespace nutls {

// [U, n, 256] floats, 16-byte aligned: dst row (u, t) = src row (u, t) for t < counts[u], zeros behind.  src may BE dst (then only
// the rows behind the counts are written).
hipError_t launch_ragged_rows(const float* src, float* dst, const int* counts, int U, int n, hipStream_t s);
// Arena slot counts[u] of utterance u (slot_floats floats, a multiple of 4; utterance u's slots start at u * slots_per_utt) becomes
// its slot 0 -- the state carried into the next block.  counts[u] = 0: nothing moves.
hipError_t launch_ragged_state_gather(float* arena, long long slot_floats, int slots_per_utt, const int* counts, int U, int n, hipStream_t s);
// Time-attention history [U][12 stages][rows_per_stage][64] of the causal32 CTFA: rows counts[u] .. counts[u] + 30 of every stage
// become rows 0 .. 30 (in place; correct for counts below 31, where the two ranges overlap).
hipError_t launch_ragged_hist_roll(float* hist, int rows_per_stage, const int* counts, int U, int n, hipStream_t s);

}  // namespace nutls
