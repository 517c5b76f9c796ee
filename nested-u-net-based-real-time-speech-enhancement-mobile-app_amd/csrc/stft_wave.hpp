// Wave-level 512-point real transform shared by the waveform block mode (stft_block.hip) and the hop builds of the frame-step kernel
// (fused_step.hip, FZ_HOP): one wavefront owns one frame, a 256-point complex FFT in registers with four exchanges through the wave's own
// LDS image (kWaveImage float2), no workgroup barrier.  The scheme, the exchange patterns and their bank-conflict analysis are described at
// the top of stft_block.hip; this header is that file's wave-level code, moved here unchanged, plus the per-frame bodies of its analysis
// and synthesis loops as functions -- both users run the same arithmetic.
#pragma once

#include <hip/hip_runtime.h>

#include "nutls_internal.hpp"

namespace nutls {
namespace stftw {

constexpr int kWaveImage = 320;         // float2 per wave

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

// Analysis of one frame.  p0 / p1: this lane's float2 of the previous hop (samples 2 l, 2 l + 1 and + 128), c0 / c1: of the new hop; w: window
// taps 2 l + 128 a, + 1; ws: W512^k of this lane's four bins k = 2 l + 1 + (i & 1) + 128 (i >> 1).  Out: magnitudes m and unit phasors rot of
// those bins, dc = the phasor of bin 0 (real: the sign of X[0]; every lane gets it).  Leaves the image in use: wave_sync() before the next write.
__device__ __forceinline__ void analyse_frame(float2 p0, float2 p1, float2 c0, float2 c1, const float2 (&w)[4], const float2 (&ws)[4],
                                              const Twiddles& t, float2* buf, int lane, float (&m)[4], float2 (&rot)[4], float2& dc) {
  float2 x[4];
  x[0] = make_float2(p0.x * w[0].x, p0.y * w[0].y);
  x[1] = make_float2(p1.x * w[1].x, p1.y * w[1].y);
  x[2] = make_float2(c0.x * w[2].x, c0.y * w[2].y);
  x[3] = make_float2(c1.x * w[3].x, c1.y * w[3].y);
  fft256(x, buf, t, lane);
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
  const float x0 = z0.x + z0.y;                                              // bin 0 is real: X[0] = Re Z[0] + Im Z[0]
  dc = make_float2(x0 < 0.f ? -1.f : 1.f, 0.f);
}

// Synthesis of one frame from the four magnitudes es of the lane's bins 2 l + 1, 2 l + 2 (+ 128), whoever formed them.  prow: the 257 phasors of the
// frame; iw: inverse-window taps 2 l + 128 a, + 1; ws: conj W512^k, k = l + 64 a.  Out: v[a] = samples 2 l + 128 a, + 1 of the windowed inverse
// transform (v[0], v[1]: first half, added to the overlap tail; v[2], v[3]: second half, the next tail).  The DC rule takes the magnitude of bin 1.
// Leaves the image in use: wave_sync() before the next write.
__device__ __forceinline__ void synthesise_bins(const float (&es)[4], const float2* __restrict__ prow, int dc_edge, const float2 (&iw)[4],
                                                const float2 (&ws)[4], const Twiddles& t, float2* buf, int lane, float2 (&v)[4]) {
  const float scale = 1.0f / static_cast<float>(NUTLS_FRAME_LEN);
  // Hermitian spectrum: bins 0..256 given, the rest mirrored; the imaginary parts of bins 0 and 256 are ignored
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = 2 * lane + 1 + (i & 1) + 128 * (i >> 1);
    const float2 r = prow[k];
    buf[k == 256 ? 256 : spec(k)] = make_float2(es[i] * r.x, k == 256 ? 0.f : es[i] * r.y);
  }
  if (lane == 0) buf[0] = make_float2(dc_edge ? es[0] * prow[0].x : 0.f, 0.f);
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
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float2 z = buf[nat(lane + 64 * a)];                                // (swapped back: .y = sample 2 n, .x = sample 2 n + 1)
    v[a] = make_float2(z.y * scale * iw[a].x, z.x * scale * iw[a].y);
  }
}

// erow: the 256 estimates of the frame (bins 1..256), synthesised as they are.  (The hop builds of the step kernel call this one.)
__device__ __forceinline__ void synthesise_frame(const float2* __restrict__ erow, const float2* __restrict__ prow, int dc_edge, const float2 (&iw)[4],
                                                 const float2 (&ws)[4], const Twiddles& t, float2* buf, int lane, float2 (&v)[4]) {
  const float2 e0 = erow[lane], e1 = erow[lane + 64];                        // bins 2 l + 1, 2 l + 2 (+ 128)
  const float es[4] = {e0.x, e0.y, e1.x, e1.y};
  synthesise_bins(es, prow, dc_edge, iw, ws, t, buf, lane, v);
}

// With an attenuation limit (nutls_set_atten_limit): xrow the noisy magnitudes of the same frame, lc = (l, c) of its row with c = 1 - l formed
// on the host.  Every bin is synthesised from m' = fma(l, x, c * e), two separate roundings -- (1, 0) gives x and (0, 1) gives e bit for bit.
__device__ __forceinline__ void synthesise_frame_mix(const float2* __restrict__ erow, const float2* __restrict__ xrow, float2 lc,
                                                     const float2* __restrict__ prow, int dc_edge, const float2 (&iw)[4], const float2 (&ws)[4],
                                                     const Twiddles& t, float2* buf, int lane, float2 (&v)[4]) {
  const float2 e0 = erow[lane], e1 = erow[lane + 64];                        // bins 2 l + 1, 2 l + 2 (+ 128)
  const float2 x0 = xrow[lane], x1 = xrow[lane + 64];
  const float es[4] = {__fmaf_rn(lc.x, x0.x, __fmul_rn(lc.y, e0.x)), __fmaf_rn(lc.x, x0.y, __fmul_rn(lc.y, e0.y)),
                       __fmaf_rn(lc.x, x1.x, __fmul_rn(lc.y, e1.x)), __fmaf_rn(lc.x, x1.y, __fmul_rn(lc.y, e1.y))};
  synthesise_bins(es, prow, dc_edge, iw, ws, t, buf, lane, v);
}

// the window / split-pass registers of a wave (analysis: win and W512^k of the lane's four bins; synthesis: inverse window and conj W512^(l + 64 a))
__device__ __forceinline__ void load_analysis_regs(const float* __restrict__ win, const float2* __restrict__ tw, int lane, float2 (&w)[4], float2 (&ws)[4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    w[a] = reinterpret_cast<const float2*>(win)[lane + 64 * a];              // taps 2 l + 128 a, + 1
    ws[a] = tw[kTwS + 2 * lane + 1 + (a & 1) + 128 * (a >> 1)];               // W512^k of this lane's four bins
  }
}
__device__ __forceinline__ void load_synthesis_regs(const float* __restrict__ inv_win, const float2* __restrict__ tw, int lane, float2 (&iw)[4], float2 (&ws)[4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    iw[a] = reinterpret_cast<const float2*>(inv_win)[lane + 64 * a];
    ws[a] = tw[kTwS + lane + 64 * a];                                          // W512^k, k = l + 64 a (used conjugated)
    ws[a].y = -ws[a].y;
  }
}

}  // namespace stftw
}  // namespace nutls
