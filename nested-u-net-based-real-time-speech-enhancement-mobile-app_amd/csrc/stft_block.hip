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
#include <hip/hip_runtime.h>

#include <cmath>

#include "nutls_internal.hpp"

namespace nutls {

namespace {

constexpr int H = NUTLS_FRAME_STEP;     // 256
constexpr int kWaves = 4;               // wavefronts per workgroup
constexpr int kRun = 4;                 // consecutive frames per wavefront: 16 frames per workgroup, 512 workgroups at 8 x 1024 frames
constexpr int kImage = 320;             // float2 per wave

// twiddle table (float2 entries; stft_block_twiddles): W256^(l q) [l][q - 1], W64^(l0 q) [l0][q - 1], W16^(l00 q) [l00][q - 1], W512^k k = 0..256
constexpr int kTwA = 0, kTwB = kTwA + 64 * 3, kTwC = kTwB + 16 * 3, kTwS = kTwC + 4 * 3, kTwEntries = 512;
static_assert(kTwS + 257 <= kTwEntries, "twiddle table");

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ int nat(int k) { return k ^ (((k >> 4) & 1) << 1) ^ ((k >> 5) & 1); }
__device__ __forceinline__ int spec(int k) { return k ^ ((k >> 4) & 1); }

// y[q] = sum_a x[a] (-i)^(a q)
__device__ __forceinline__ void bfly4(float2 (&x)[4]) {
  const float2 s02 = make_float2(x[0].x + x[2].x, x[0].y + x[2].y), d02 = make_float2(x[0].x - x[2].x, x[0].y - x[2].y);
  const float2 s13 = make_float2(x[1].x + x[3].x, x[1].y + x[3].y), d13 = make_float2(x[1].x - x[3].x, x[1].y - x[3].y);
  x[0] = make_float2(s02.x + s13.x, s02.y + s13.y);
  x[1] = make_float2(d02.x + d13.y, d02.y - d13.x);
  x[2] = make_float2(s02.x - s13.x, s02.y - s13.y);
  x[3] = make_float2(d02.x - d13.y, d02.y + d13.x);
}

struct Twiddles { float2 a[3], b[3], c[3]; };

__device__ __forceinline__ Twiddles load_twiddles(const float2* __restrict__ tw, int lane) {
  Twiddles t;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    t.a[q] = tw[kTwA + lane * 3 + q];
    t.b[q] = tw[kTwB + (lane & 15) * 3 + q];
    t.c[q] = tw[kTwC + (lane & 3) * 3 + q];
  }
  return t;
}

// Forward 256-point complex FFT of one wave.  In: lane l holds x[a] = z[l + 64 a].  Out: Z[k] at buf[nat(k)], visible to the whole wave.
__device__ __forceinline__ void fft256(float2 (&x)[4], float2* buf, const Twiddles& t, int lane) {
  const int k0 = lane >> 4, l0 = lane & 15, k1 = (lane >> 2) & 3, l00 = lane & 3;
  bfly4(x);
#pragma unroll
  for (int q = 1; q < 4; ++q) x[q] = cmul(x[q], t.a[q - 1]);
#pragma unroll
  for (int q = 0; q < 4; ++q) buf[80 * q + lane] = x[q];
  wave_sync();
#pragma unroll
  for (int a = 0; a < 4; ++a) x[a] = buf[80 * k0 + l0 + 16 * a];
  wave_sync();
  bfly4(x);
#pragma unroll
  for (int q = 1; q < 4; ++q) x[q] = cmul(x[q], t.b[q - 1]);
#pragma unroll
  for (int q = 0; q < 4; ++q) buf[80 * k0 + 20 * q + l0] = x[q];
  wave_sync();
#pragma unroll
  for (int a = 0; a < 4; ++a) x[a] = buf[80 * k0 + 20 * k1 + l00 + 4 * a];
  wave_sync();
  bfly4(x);
#pragma unroll
  for (int q = 1; q < 4; ++q) x[q] = cmul(x[q], t.c[q - 1]);
#pragma unroll
  for (int q = 0; q < 4; ++q) buf[80 * k0 + 20 * k1 + 4 * l00 + (q ^ l00)] = x[q];
  wave_sync();
#pragma unroll
  for (int a = 0; a < 4; ++a) x[a] = buf[80 * k0 + 20 * k1 + 4 * a + (l00 ^ a)];      // (this lane's k2 = lane & 3)
  wave_sync();
  bfly4(x);
  const int kb = k0 + 4 * k1 + 16 * l00;
#pragma unroll
  for (int q = 0; q < 4; ++q) buf[nat(kb + 64 * q)] = x[q];
  wave_sync();
}

}  // namespace

// grid (tiles of kWaves * kRun frames, U), 256 threads
__global__ __launch_bounds__(64 * kWaves) void stft_block_kernel(const float* __restrict__ pcm, const float* __restrict__ tail_in,
                                                                 float* __restrict__ tail_out, const float* __restrict__ win,
                                                                 const float2* __restrict__ tw, float* __restrict__ mag,
                                                                 float2* __restrict__ ph, int n_hops) {
  __shared__ float2 image[kWaves][kImage];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, u = blockIdx.y;
  const int f0 = (static_cast<int>(blockIdx.x) * kWaves + wave) * kRun;
  if (f0 >= n_hops) return;
  const int f1 = min(f0 + kRun, n_hops);
  float2* buf = image[wave];
  const Twiddles t = load_twiddles(tw, lane);
  float2 w[4], ws[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    w[a] = reinterpret_cast<const float2*>(win)[lane + 64 * a];              // taps 2 l + 128 a, + 1
    ws[a] = tw[kTwS + 2 * lane + 1 + (a & 1) + 128 * (a >> 1)];               // W512^k of this lane's four bins
  }
  const size_t row0 = static_cast<size_t>(u) * n_hops;
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
    float2 x[4];
    x[0] = make_float2(p0.x * w[0].x, p0.y * w[0].y);
    x[1] = make_float2(p1.x * w[1].x, p1.y * w[1].y);
    x[2] = make_float2(c0.x * w[2].x, c0.y * w[2].y);
    x[3] = make_float2(c1.x * w[3].x, c1.y * w[3].y);
    fft256(x, buf, t, lane);
    float m[4];
    float2 rot[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 2 * lane + 1 + (i & 1) + 128 * (i >> 1);                   // bins 1..256
      const float2 zk = buf[nat(k & 255)], zm = buf[nat(256 - k)];
      const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
      const float2 o = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
      const float2 wo = cmul(o, ws[i]);
      const float xr = e.x + wo.x, xi = e.y + wo.y;
      m[i] = sqrtf(xr * xr + xi * xi);
      rot[i] = m[i] > 0.f ? make_float2(xr / m[i], xi / m[i]) : make_float2(1.f, 0.f);
    }
    const float2 z0 = buf[0];
    const size_t row = row0 + f;
    float2* mrow = reinterpret_cast<float2*>(mag + row * H);
    mrow[lane] = make_float2(m[0], m[1]);
    mrow[lane + 64] = make_float2(m[2], m[3]);
    float2* prow = ph + row * (H + 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) prow[2 * lane + 1 + (i & 1) + 128 * (i >> 1)] = rot[i];
    if (lane == 0) {                                                           // bin 0 is real: X[0] = Re Z[0] + Im Z[0]
      const float x0 = z0.x + z0.y;
      prow[0] = make_float2(x0 < 0.f ? -1.f : 1.f, 0.f);
    }
    wave_sync();                                                               // (the reads above come before the next frame's writes)
    p0 = c0; p1 = c1;
    c0 = n0; c1 = n1;
  }
  if (f1 == n_hops) {                                                          // the last hop of the block is the next block's previous hop
    float2* to = reinterpret_cast<float2*>(tail_out + static_cast<size_t>(u) * H);
    to[lane] = p0; to[lane + 64] = p1;
  }
}

__global__ __launch_bounds__(64 * kWaves) void istft_block_kernel(const float* __restrict__ est, const float2* __restrict__ ph,
                                                                  const float* __restrict__ inv_win, const float2* __restrict__ tw,
                                                                  const float* __restrict__ ola_in, float* __restrict__ ola_out,
                                                                  float* __restrict__ pcm_out, int dc_edge, int n_hops) {
  __shared__ float2 image[kWaves][kImage];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, u = blockIdx.y;
  const int o0 = (static_cast<int>(blockIdx.x) * kWaves + wave) * kRun;      // this wave produces output hops [o0, o1)
  if (o0 >= n_hops) return;
  const int o1 = min(o0 + kRun, n_hops);
  float2* buf = image[wave];
  const Twiddles t = load_twiddles(tw, lane);
  float2 iw[4], ws[4];
  const float scale = 1.0f / static_cast<float>(NUTLS_FRAME_LEN);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    iw[a] = reinterpret_cast<const float2*>(inv_win)[lane + 64 * a];
    ws[a] = tw[kTwS + lane + 64 * a];                                          // W512^k, k = l + 64 a (used conjugated)
    ws[a].y = -ws[a].y;
  }
  const size_t row0 = static_cast<size_t>(u) * n_hops;
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
    const float2 e0 = erow[lane], e1 = erow[lane + 64];                        // bins 2 l + 1, 2 l + 2 (+ 128)
    const float es[4] = {e0.x, e0.y, e1.x, e1.y};
    // Hermitian spectrum: bins 0..256 given, the rest mirrored; the imaginary parts of bins 0 and 256 are ignored
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 2 * lane + 1 + (i & 1) + 128 * (i >> 1);
      const float2 r = prow[k];
      buf[k == 256 ? 256 : spec(k)] = make_float2(es[i] * r.x, k == 256 ? 0.f : es[i] * r.y);
    }
    if (lane == 0) buf[0] = make_float2(dc_edge ? e0.x * prow[0].x : 0.f, 0.f);
    wave_sync();
    float2 x[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int k = lane + 64 * a;
      const float2 yk = buf[spec(k)], ym = buf[k == 0 ? 256 : spec(256 - k)];
      const float2 e = make_float2(yk.x + ym.x, yk.y - ym.y);
      const float2 o = cmul(make_float2(yk.x - ym.x, yk.y + ym.y), ws[a]);
      x[a] = make_float2(e.y + o.x, e.x - o.y);                                // Z = E + i O, re / im swapped: the inverse transform
    }
    wave_sync();
    fft256(x, buf, t, lane);
    float2 v[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float2 z = buf[nat(lane + 64 * a)];                                // (swapped back: .y = sample 2 n, .x = sample 2 n + 1)
      v[a] = make_float2(z.y * scale * iw[a].x, z.x * scale * iw[a].y);
    }
    if (f >= o0) {
      float2* orow = reinterpret_cast<float2*>(pcm_out + row * H);
      orow[lane] = make_float2(carry0.x + v[0].x, carry0.y + v[0].y);
      orow[lane + 64] = make_float2(carry1.x + v[1].x, carry1.y + v[1].y);
    }
    carry0 = v[2]; carry1 = v[3];
    wave_sync();
  }
  if (o1 == n_hops) {
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

hipError_t launch_stft_block(const float* pcm, const float* tail_in, float* tail_out, const float* win, const float* tw, float* mag, float* ph,
                             int U, int n_hops, hipStream_t s) {
  hipLaunchKernelGGL(stft_block_kernel, block_grid(U, n_hops), dim3(64 * kWaves), 0, s, pcm, tail_in, tail_out, win,
                     reinterpret_cast<const float2*>(tw), mag, reinterpret_cast<float2*>(ph), n_hops);
  return hipGetLastError();
}

hipError_t launch_istft_block(const float* est, const float* ph, const float* inv_win, const float* tw, const float* ola_in, float* ola_out,
                              float* pcm_out, int dc_edge, int U, int n_hops, hipStream_t s) {
  hipLaunchKernelGGL(istft_block_kernel, block_grid(U, n_hops), dim3(64 * kWaves), 0, s, est, reinterpret_cast<const float2*>(ph), inv_win,
                     reinterpret_cast<const float2*>(tw), ola_in, ola_out, pcm_out, dc_edge, n_hops);
  return hipGetLastError();
}

}  // namespace nutls
