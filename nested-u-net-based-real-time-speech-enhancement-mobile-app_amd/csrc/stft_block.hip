// Waveform block mode of the offline handles: STFT analysis and inverse-STFT / overlap-add synthesis of a whole
// block (n_hops consecutive hops of each of U utterances) in one launch each.  Same function as stft.hip's per-hop
// kernels (interpreter_proposed.py:203-213, 352-365), written for real input:
//
//   * a 512-point real transform = ONE 256-point complex FFT of z[n] = x[2n] + i x[2n+1] plus the split pass
//       X[k] = (Z[k] + conj Z[256-k]) / 2  +  W512^k (Z[k] - conj Z[256-k]) / (2i),   k = 0..256
//     and its mirror in front of the inverse (Z[k] = E[k] + i O[k], E = Y[k] + conj Y[256-k],
//     O = (Y[k] - conj Y[256-k]) conj W512^k); the inverse complex FFT is the forward one with re / im swapped
//     on the way in and out, so both directions run the same code and the same twiddles.
//   * one wavefront owns one frame at a time: lane l holds z[l + 64 a], a = 0..3, and the FFT is four radix-4
//     decimation-in-frequency stages in registers (256 = 4^4) with three exchanges through the wave's own LDS
//     image between them and a fourth that leaves the result in natural order.  Only wave-level ordering
//     (LDS operations of a wave execute in order; wave_sync() keeps the compiler from moving them): no
//     __syncthreads anywhere in these kernels.
//   * a wave owns a run of kRun consecutive frames of one utterance, a workgroup kWaves such runs in a row.  The
//     wave keeps the hop it has just read (analysis) / the second half of the frame it has just transformed
//     (synthesis) in registers for the next frame, so inside a run every hop is read once and the overlap-add
//     needs neither atomics nor a second pass; the frame in front of a run is read (analysis: one hop, which the
//     neighbouring wave of the same workgroup reads at the same time) or transformed (synthesis: the one
//     redundant frame of the run) again -- or replaced by the carried tail / ola for the first run of a block.
//     Window, inverse window and all twiddles live in registers, loaded once per wave.
//   * every frame goes through the same loop body whatever its place in a run or block, so a result does not
//     depend on how the audio is cut into blocks, tiles or runs (tested bit for bit).
//
// LDS image of a wave: 320 float2.  All accesses are 8-byte (ds_write_b64: four groups of 16 consecutive lanes,
// bank = dword address mod 32 = float2 slot mod 16; ds_read_b64: two groups of 32 lanes, bank = dword address
// mod 64 = float2 slot mod 32).  Checked for every instruction of every exchange, by enumerating the slots of
// each lane group (tools/check_stft_block_lds.py does the same enumeration): all conflict-free.
//   exchange 1  lane l, register k0:        write [80 k0 + l]                    (16 consecutive slots)
//               lane m = 16 k0 + l0:        read  [80 k0 + l0 + 16 a]            (80 = 16 mod 32: the two k0 of a half-wave take the two halves of a bank row)
//   exchange 2  lane (k0, l0), register k1: write [80 k0 + 20 k1 + l0]
//               lane m = 16 k0 + 4 k1 + l00: read [80 k0 + 20 k1 + l00 + 4 a]     (20 k1 + 16 k0 mod 32 = eight distinct multiples of 4)
//   exchange 3  lane (k0, k1, l00), reg k2: write [80 k0 + 20 k1 + 4 l00 + (k2 ^ l00)]   (a 4 x 4 transpose per (k0, k1): the XOR keeps the
//               lane m = 16 k0 + 4 k1 + k2: read  [80 k0 + 20 k1 + 4 a + (k2 ^ a)]        four lanes that share (k1 + l00) mod 4 apart)
//   exchange 4  lane (k0, k1, k2), reg k3:  write [nat(k)], k = k0 + 4 k1 + 16 k2 + 64 k3, nat(k) = k ^ (bit 4 of k -> bit 1, bit 5 -> bit 0)
//               analysis, lane l:           read  [nat(k)], [nat(256 - k)], k = 2 l + e + 128 j   (32 lanes = the odd or the even k of a run of 64)
//               synthesis, lane l:          read  [nat(l + 64 a)]
//   synthesis, spectrum in front of the FFT:  write [spec(k)], k = 2 l + e + 128 j, spec(k) = k ^ (bit 4 of k -> bit 0), bin 256 at [256]
//                                             read  [spec(l + 64 a)], [spec(256 - l - 64 a)]
// The wave-level code itself (fft256, nat, spec, the per-frame analysis and synthesis bodies) is stft_wave.hpp, shared with the hop builds
// of the frame-step kernel.  Its index expressions, as written there (tools/check_stft_block_lds.py models exactly these):
//   nat(k):      return k ^ (((k >> 4) & 1) << 1) ^ ((k >> 5) & 1);
//   spec(k):     return k ^ ((k >> 4) & 1);
//   exchange 1:  buf[80 * q + lane]                             ->  buf[80 * k0 + l0 + 16 * a]
//   exchange 2:  buf[80 * k0 + 20 * q + l0]                     ->  buf[80 * k0 + 20 * k1 + l00 + 4 * a]
//   exchange 3:  buf[80 * k0 + 20 * k1 + 4 * l00 + (q ^ l00)]   ->  buf[80 * k0 + 20 * k1 + 4 * a + (l00 ^ a)]
#include <hip/hip_runtime.h>

#include <cmath>

#include "nutls_internal.hpp"
#include "stft_wave.hpp"

namespace nutls {

namespace {

using namespace stftw;      // the wave-level transform and the per-frame bodies: stft_wave.hpp

constexpr int H = NUTLS_FRAME_STEP;     // 256
constexpr int kWaves = 4;               // wavefronts per workgroup
constexpr int kRun = 4;                 // consecutive frames per wavefront: 16 frames per workgroup, 512 workgroups at 8 x 1024 frames
constexpr int kImage = 320;             // float2 per wave
static_assert(kImage == kWaveImage, "the LDS image of a wave is the one stft_wave.hpp addresses");

}  // namespace

// Both kernels: grid (tiles of kWaves * kRun frames, U), 256 threads.  RAGGED (nutls_stft_block_ragged / nutls_istft_block_ragged): hops [U],
// clamped to 0 .. n_hops -- utterance u has k = hops[u] real hops in a block whose row stride is n_hops.  A wave's run ends at hop k; the rows
// behind it are written with zeros and never read; the carry is written by the wave that owns hop k - 1 (k = 0: the carried-in hop / overlap
// tail is copied across, the two buffers alternate).  The counts change where a run ends and nothing else: every real hop goes through the one
// loop body below, so it has the bits of the uniform block (tests/test_gpu_ragged_enhance.py).  hops is null, and not read, without RAGGED.
template <bool RAGGED>
__global__ __launch_bounds__(64 * kWaves) void stft_block_kernel(const float* __restrict__ pcm, const float* __restrict__ tail_in,
                                                                 float* __restrict__ tail_out, const float* __restrict__ win,
                                                                 const float2* __restrict__ tw, float* __restrict__ mag,
                                                                 float2* __restrict__ ph, int n_hops, const int* __restrict__ hops) {
  __shared__ float2 image[kWaves][kImage];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, u = blockIdx.y;
  const int f0 = (static_cast<int>(blockIdx.x) * kWaves + wave) * kRun;
  if (f0 >= n_hops) return;
  int f1 = min(f0 + kRun, n_hops);
  const size_t row0 = static_cast<size_t>(u) * n_hops;
  int last = n_hops;                                                           // the carry is taken behind hop last - 1
  if constexpr (RAGGED) {
    last = min(max(hops[u], 0), n_hops);
    for (int f = max(f0, last); f < f1; ++f) {
      float2* mrow = reinterpret_cast<float2*>(mag + (row0 + f) * H);
      mrow[lane] = make_float2(0.f, 0.f);
      mrow[lane + 64] = make_float2(0.f, 0.f);
    }
    if (last == 0 && f0 == 0) {
      const float2* from = reinterpret_cast<const float2*>(tail_in + static_cast<size_t>(u) * H);
      float2* to = reinterpret_cast<float2*>(tail_out + static_cast<size_t>(u) * H);
      to[lane] = from[lane]; to[lane + 64] = from[lane + 64];
    }
    if (f0 >= last) return;
    f1 = min(f1, last);
  }
  float2* buf = image[wave];
  const Twiddles t = load_twiddles(tw, lane);
  float2 w[4], ws[4];
  load_analysis_regs(win, tw, lane, w, ws);
  const float2* prev = reinterpret_cast<const float2*>(f0 == 0 ? tail_in + static_cast<size_t>(u) * H : pcm + (row0 + f0 - 1) * H);
  float2 p0 = prev[lane], p1 = prev[lane + 64];
  const float2* cur = reinterpret_cast<const float2*>(pcm + (row0 + f0) * H);
  float2 c0 = cur[lane], c1 = cur[lane + 64];
#pragma unroll 1
  for (int f = f0; f < f1; ++f) {
    float2 n0 = c0, n1 = c1;
    if (f + 1 < f1) {                                                          // the next hop is on its way while this frame is transformed
      const float2* nxt = reinterpret_cast<const float2*>(pcm + (row0 + f + 1) * H);
      n0 = nxt[lane]; n1 = nxt[lane + 64];
    }
    float m[4];
    float2 rot[4], dc;
    analyse_frame(p0, p1, c0, c1, w, ws, t, buf, lane, m, rot, dc);
    const size_t row = row0 + f;
    float2* mrow = reinterpret_cast<float2*>(mag + row * H);
    mrow[lane] = make_float2(m[0], m[1]);
    mrow[lane + 64] = make_float2(m[2], m[3]);
    float2* prow = ph + row * (H + 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) prow[2 * lane + 1 + (i & 1) + 128 * (i >> 1)] = rot[i];
    if (lane == 0) prow[0] = dc;
    wave_sync();                                                               // (the reads above come before the next frame's writes)
    p0 = c0; p1 = c1;
    c0 = n0; c1 = n1;
  }
  if (f1 == last) {                                                            // the last hop of the block is the next block's previous hop
    float2* to = reinterpret_cast<float2*>(tail_out + static_cast<size_t>(u) * H);
    to[lane] = p0; to[lane + 64] = p1;
  }
}

// MIX, the attenuation limit (nutls_set_atten_limit / nutls_istft_block_mix): noisy [U][n_hops][256] the magnitudes of the same frames as the
// analysis wrote them, lim [U] = (l, c) of each utterance, loaded once per wave.  Every frame is synthesised from m' = fma(l, x, c * e)
// (synthesise_frame_mix); the noisy row of the redundant frame in front of a run is read again like its estimate, no row behind a count is read.
// noisy and lim are null, and not read, without MIX.
template <bool RAGGED, bool MIX>
__global__ __launch_bounds__(64 * kWaves) void istft_block_kernel(const float* __restrict__ est, const float2* __restrict__ ph,
                                                                  const float* __restrict__ inv_win, const float2* __restrict__ tw,
                                                                  const float* __restrict__ ola_in, float* __restrict__ ola_out,
                                                                  float* __restrict__ pcm_out, int dc_edge, int n_hops,
                                                                  const int* __restrict__ hops, const float* __restrict__ noisy,
                                                                  const float2* __restrict__ lim) {
  __shared__ float2 image[kWaves][kImage];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, u = blockIdx.y;
  const int o0 = (static_cast<int>(blockIdx.x) * kWaves + wave) * kRun;      // this wave produces output hops [o0, o1)
  if (o0 >= n_hops) return;
  int o1 = min(o0 + kRun, n_hops);
  const size_t row0 = static_cast<size_t>(u) * n_hops;
  int last = n_hops;                                                           // the carry is the second half of frame last - 1
  if constexpr (RAGGED) {
    last = min(max(hops[u], 0), n_hops);
    for (int f = max(o0, last); f < o1; ++f) {
      float2* orow = reinterpret_cast<float2*>(pcm_out + (row0 + f) * H);
      orow[lane] = make_float2(0.f, 0.f);
      orow[lane + 64] = make_float2(0.f, 0.f);
    }
    if (last == 0 && o0 == 0) {
      const float2* from = reinterpret_cast<const float2*>(ola_in + static_cast<size_t>(u) * H);
      float2* to = reinterpret_cast<float2*>(ola_out + static_cast<size_t>(u) * H);
      to[lane] = from[lane]; to[lane + 64] = from[lane + 64];
    }
    if (o0 >= last) return;
    o1 = min(o1, last);
  }
  float2* buf = image[wave];
  const Twiddles t = load_twiddles(tw, lane);
  float2 iw[4], ws[4];
  load_synthesis_regs(inv_win, tw, lane, iw, ws);
  float2 lc = make_float2(0.f, 1.f);
  if constexpr (MIX) lc = lim[u];
  float2 carry0 = make_float2(0.f, 0.f), carry1 = carry0;
  if (o0 == 0) {
    const float2* from = reinterpret_cast<const float2*>(ola_in + static_cast<size_t>(u) * H);
    carry0 = from[lane]; carry1 = from[lane + 64];
  }
  // frames o0 - 1 .. o1 - 1: the frame in front of the run only for its second half (the first run of a block has the carried one instead)
#pragma unroll 1
  for (int f = o0 > 0 ? o0 - 1 : 0; f < o1; ++f) {
    const size_t row = row0 + f;
    const float2* erow = reinterpret_cast<const float2*>(est + row * H);
    const float2* prow = ph + row * (H + 1);
    float2 v[4];
    if constexpr (MIX) synthesise_frame_mix(erow, reinterpret_cast<const float2*>(noisy + row * H), lc, prow, dc_edge, iw, ws, t, buf, lane, v);
    else synthesise_frame(erow, prow, dc_edge, iw, ws, t, buf, lane, v);
    if (f >= o0) {
      float2* orow = reinterpret_cast<float2*>(pcm_out + row * H);
      orow[lane] = make_float2(carry0.x + v[0].x, carry0.y + v[0].y);
      orow[lane + 64] = make_float2(carry1.x + v[1].x, carry1.y + v[1].y);
    }
    carry0 = v[2]; carry1 = v[3];
    wave_sync();
  }
  if (o1 == last) {
    float2* to = reinterpret_cast<float2*>(ola_out + static_cast<size_t>(u) * H);
    to[lane] = carry0; to[lane + 64] = carry1;
  }
}

std::vector<float> stft_block_twiddles() {
  std::vector<float> tw(static_cast<size_t>(2) * kTwEntries, 0.f);
  auto put = [&](int idx, double num, double den) {
    const double a = -2.0 * 3.14159265358979323846 * num / den;
    tw[2 * static_cast<size_t>(idx)] = static_cast<float>(std::cos(a));
    tw[2 * static_cast<size_t>(idx) + 1] = static_cast<float>(std::sin(a));
  };
  for (int q = 1; q < 4; ++q) {
    for (int l = 0; l < 64; ++l) put(kTwA + l * 3 + q - 1, l * q, 256.0);
    for (int l = 0; l < 16; ++l) put(kTwB + l * 3 + q - 1, l * q, 64.0);
    for (int l = 0; l < 4; ++l) put(kTwC + l * 3 + q - 1, l * q, 16.0);
  }
  for (int k = 0; k <= 256; ++k) put(kTwS + k, k, 512.0);
  return tw;
}

static dim3 block_grid(int U, int n_hops) { return dim3((n_hops + kWaves * kRun - 1) / (kWaves * kRun), U); }

// The instantiation follows from which of the optional pointers are given (nutls_internal.hpp).
hipError_t launch_stft_block(const float* pcm, const float* tail_in, float* tail_out, const float* win, const float* tw, float* mag, float* ph,
                             const int* hops, int U, int n_hops, hipStream_t s) {
  auto* kernel = hops ? stft_block_kernel<true> : stft_block_kernel<false>;
  hipLaunchKernelGGL(kernel, block_grid(U, n_hops), dim3(64 * kWaves), 0, s, pcm, tail_in, tail_out, win, reinterpret_cast<const float2*>(tw), mag,
                     reinterpret_cast<float2*>(ph), n_hops, hops);
  return hipGetLastError();
}

hipError_t launch_istft_block(const float* est, const float* noisy, const float* lim, const float* ph, const float* inv_win, const float* tw,
                              const float* ola_in, float* ola_out, float* pcm_out, int dc_edge, const int* hops, int U, int n_hops, hipStream_t s) {
  auto* kernel = noisy ? (hops ? istft_block_kernel<true, true> : istft_block_kernel<false, true>)
                       : (hops ? istft_block_kernel<true, false> : istft_block_kernel<false, false>);
  hipLaunchKernelGGL(kernel, block_grid(U, n_hops), dim3(64 * kWaves), 0, s, est, reinterpret_cast<const float2*>(ph), inv_win,
                     reinterpret_cast<const float2*>(tw), ola_in, ola_out, pcm_out, dc_edge, n_hops, hops, noisy, reinterpret_cast<const float2*>(lim));
  return hipGetLastError();
}

}  // namespace nutls
