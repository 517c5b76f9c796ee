// Ragged blocks of the offline batch handles: per-utterance frame counts around an unchanged block (nutls_process_block_ragged).
//
// Every layer of the model is causal in time and utterances never mix, so frame t of utterance u depends on nothing behind t and on
// nothing of another utterance: a block in which utterance u has k_u real frames is computed as the uniform block of the row stride n,
// and only what goes in and what is kept differ.  Three small kernels do that, all on the caller's stream:
//   stage-in   rows behind the count are zeros in the library's input buffer (the caller's rows there may hold anything, NaN included);
//   stage-out  rows behind the count are zeros in the caller's output;
//   commit     the state carried to the next block is the arena slot of frame k_u (not n), the causal32 time-attention history the
//              31 rows in front of row 31 + k_u.  k_u = 0 holds the utterance: nothing of it moves.
// All of them are pure copies: 16-byte accesses, no arithmetic, no shared state between utterances.
#include <hip/hip_runtime.h>

#include "ragged.hpp"

namespace nutls {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRowVec = 256 / 4;        // 16-byte vectors per row of magnitudes
constexpr int kHistVec = 31 * 64 / 4;   // ... per 31-row history window
constexpr int kGatherBlocks = 64;       // workgroups per utterance of the state gather

__device__ __forceinline__ int clamped_count(const int* __restrict__ counts, int u, int n) { return min(max(counts[u], 0), n); }

// grid (ceil(n * 64 / 256), U), 256 threads: one 16-byte vector per thread
__global__ __launch_bounds__(256) void ragged_rows_kernel(const f32x4* src, f32x4* dst, const int* __restrict__ counts, int n) {
  const int u = blockIdx.y;
  const int i = static_cast<int>(blockIdx.x) * 256 + threadIdx.x;      // vector within the utterance's n rows
  if (i >= n * kRowVec) return;
  const bool real = i / kRowVec < clamped_count(counts, u, n);
  const size_t at = static_cast<size_t>(u) * n * kRowVec + i;
  if (real && src == dst) return;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (real) v = src[at];
  dst[at] = v;
}

// grid (kGatherBlocks, U), 256 threads.  Source (slot k >= 1) and destination (slot 0) never overlap; k = 0 copies nothing.
__global__ __launch_bounds__(256) void ragged_state_gather_kernel(float* __restrict__ arena, long long slot_floats, int slots_per_utt,
                                                                   const int* __restrict__ counts, int n) {
  const int u = blockIdx.y;
  const int k = clamped_count(counts, u, n);
  if (k == 0) return;
  f32x4* to = reinterpret_cast<f32x4*>(arena + static_cast<size_t>(u) * slots_per_utt * slot_floats);
  const f32x4* from = to + static_cast<size_t>(k) * (slot_floats / 4);
  const long long n4 = slot_floats / 4;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < n4; i += static_cast<long long>(kGatherBlocks) * 256)
    __builtin_nontemporal_store(__builtin_nontemporal_load(from + i), to + i);
}

// grid (12 stages, U), 512 threads: every value is read before any is written (the ranges overlap when k < 31)
__global__ __launch_bounds__(512) void ragged_hist_roll_kernel(float* __restrict__ hist, int rows_per_stage, const int* __restrict__ counts, int n) {
  const int u = blockIdx.y, tid = threadIdx.x;
  const int k = clamped_count(counts, u, n);
  if (k == 0) return;                                                          // (the whole workgroup: the count is per utterance)
  f32x4* rows = reinterpret_cast<f32x4*>(hist + (static_cast<size_t>(u) * 12 + blockIdx.x) * rows_per_stage * 64);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (tid < kHistVec) v = rows[static_cast<size_t>(k) * 16 + tid];
  __syncthreads();
  if (tid < kHistVec) rows[tid] = v;
}

}  // namespace

hipError_t launch_ragged_rows(const float* src, float* dst, const int* counts, int U, int n, hipStream_t s) {
  hipLaunchKernelGGL(ragged_rows_kernel, dim3((n * kRowVec + 255) / 256, U), dim3(256), 0, s, reinterpret_cast<const f32x4*>(src),
                     reinterpret_cast<f32x4*>(dst), counts, n);
  return hipGetLastError();
}

hipError_t launch_ragged_state_gather(float* arena, long long slot_floats, int slots_per_utt, const int* counts, int U, int n, hipStream_t s) {
  hipLaunchKernelGGL(ragged_state_gather_kernel, dim3(kGatherBlocks, U), dim3(256), 0, s, arena, slot_floats, slots_per_utt, counts, n);
  return hipGetLastError();
}

hipError_t launch_ragged_hist_roll(float* hist, int rows_per_stage, const int* counts, int U, int n, hipStream_t s) {
  hipLaunchKernelGGL(ragged_hist_roll_kernel, dim3(12, U), dim3(512), 0, s, hist, rows_per_stage, counts, n);
  return hipGetLastError();
}

}  // namespace nutls
