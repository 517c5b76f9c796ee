// PCM gateway: the callers' samples (float32 or int16 at 8 / 16 / 32 / 48 kHz) to and from the library's float32 at 16 kHz (nutls_set_pcm_format).
//
// One device body (pcm_hop) behind one kernel template (pcm_kernel), instantiated 36 times -- per half (decode, encode), rate, sample type and
// mode: launch_half, below, is the one place that says which exist and picks one.  A launch is one 256-thread workgroup per (row, hop) -- row =
// stream of a streaming handle, utterance of an offline one; the hop entries launch one hop per row, the block entries n_hops.  The body:
//   1. the prototype p[0 .. 2 K q] and the hop with its left context (the last 2 K q samples in front of it for a rate reduction, the last 2 K
//      for a rate increase) go to LDS as float32, 16 bytes per lane and load (8 int16 or 4 float32).  The context of a row's first hop comes
//      from the history the handle keeps, that of the later hops of a block straight from the row;
//   2. the workgroup of a row's last hop writes the new history: the last samples of what it has just staged;
//   3. every output sample is ONE chain of fp32 FMAs over the prototype's taps in ascending order, from 0 (pcm_fir: the zero-stuffed terms of a
//      rate increase are skipped by polyphase indexing, the rest keep their order).  The chain of an output sample does not depend on where
//      the sample lies in its hop, in its block or in which entry runs it: results are bit-exact across every cut of a stream;
//   4. the hop leaves through LDS in 16-byte stores (float32 -> int16: y * 32768 rounded to nearest even, clamped, NaN -> 0).
// A held row (active[row] == 0) returns before 1.: its history is neither read nor written, its output hop is zeros.
// Ragged blocks (counts[row] = k real hops of the row, clamped to 0 .. n_hops): the hops in front of k run 1. to 4. as they are, the workgroup
// of hop k - 1 writes the history, a hop behind k returns before 1. with a zero hop; k == 0 holds the row, and because a block call flips the
// history buffers of the whole handle, the workgroup of its hop 0 copies the row's history across.
// Cost: 256 * 145 FMAs per stream and hop at most (48 kHz decode); the launch, not the arithmetic, is what a hop pays for.
// Upper band (nutls_set_pcm_upper_band, 32 / 48 kHz): the band above 8 kHz goes around the model inside the same two launches, in the
// instantiations with UPPER (pcm_hop<..., UPPER>, see there) -- the ones without are what a gain of 0 runs.  Per caller sample n of a stream,
// each a fixed sequence of fp32 operations wherever the hop or block boundary falls:
//   d[m]   = the decode chain: taps ascending, one FMA each, from 0                                      (2 K q + 1 FMAs)
//   c[n]   = the encode chain over d: taps r, r + q, ... ascending, one FMA each, from 0, WITHOUT its product by q   (2 K + 1 FMAs at r = 0, else 2 K)
//   u[n]   = fmaf(-q, c[n], x[n - 2 K q])                                                                  (one FMA)
//   z[n]   = the encode chain over the model's output, times q: the sample a gain of 0 returns
//   out[n] = fmaf(gain, u[n - S], z[n])                                                                    (one FMA)
// The longest path of an output sample has 2 K q + 2 K + 4 roundings (d, c, u, out).  +49 FMAs per caller sample in the decode, and the 2 K
// decoded samples of context computed again by every hop of a block but its first (+19 % of the decode chains); the encode adds one FMA.
// Follow (nutls_set_pcm_upper_follow): the gain of out[n] follows the model, gamma_t[n] of nutls.h -- the instantiations with FOLLOW (pcm_hop<..., UPPER,
// FOLLOW>), in the same two launches; one energy code for both halves (pcm_e2), every g a function of 5 a and 5 b, so one workgroup per (row, hop).
// G.711 (NUTLS_PCM_ULAW / NUTLS_PCM_ALAW, 8 kHz only): two more sample types beside float32 and int16, one byte per sample (ulaw_t, alaw_t), so
// four instantiations -- the 8 kHz decode and encode of each law; no other rate and no other mode has them.  A lane loads or stores 16 codes in its 16 bytes.  On the way in a code is expanded to its int16 value and that times
// 2^-15 (exact): from there on the chain is the int16 format's.  On the way out the float is quantised by to_s16, the int16 format's rule,
// and that value is compressed.  Both directions are integer bit operations (g711_expand, g711_compress: the segment of a sample from the
// position of its leading bit, no table), exact, and agree with the host's statement of the rule (nutls_pcm_g711_expand / _compress, api_pcm.cpp)
// for all 256 codes and all 65 536 int16 values.  Where the other formats write a zero hop (a held row, a hop behind a count), these write the
// format's silence code -- 0xFF / 0xD5, what a zero hop compresses to: a zero BYTE is full-scale negative in mu-law and -5504 in A-law.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "pcm.hpp"

namespace nutls {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// One byte of G.711, mu-law or A-law: two distinct types, so that stage_in / stage_out / zero_out resolve by overload like float and short
struct ulaw_t { unsigned char code; };
struct alaw_t { unsigned char code; };

constexpr int kThreads = 256;

template <int Q>
struct Rate {
  static constexpr int k = Q == 1 ? 0 : kPcmK;      // 16 kHz: the single tap 1.0, no delay
  static constexpr int taps = 2 * k * Q + 1;
};

// ---- one output sample --------------------------------------------------------------------------------------------------------------------
// x: the staged samples in LDS, x[0] = the oldest sample of the left context (hist samples), x[hist] = the hop's first.
// DOWN (rate reduction by Q):  y[n] = sum_j p[j] x[Q n - j],                j = 0 .. 2 K Q
// UP   (rate increase by Q):   z[n] = Q sum_i p[r + Q i] x[m - i],  n = Q m + r,  i = 0 .. 2 K (r = 0) or 2 K - 1   (zero-stuffing, then Q p)
// pcm_up_chain: the chain of UP without its last step, the product by Q (the upper band folds that product into its subtraction).
template <int Q>
__device__ __forceinline__ float pcm_up_chain(const float* p, const float* x, int n) {
  constexpr int K = Rate<Q>::k;
  float acc = 0.f;
  const int m = n / Q, r = n - m * Q;
  const float* at = x + 2 * K + m;
  const float* pr = p + r;
#pragma unroll 8
  for (int i = 0; i < 2 * K; ++i) acc = fmaf(pr[Q * i], at[-i], acc);
  if (r == 0) acc = fmaf(p[2 * K * Q], at[-2 * K], acc);
  return acc;
}

template <int Q, bool UP>
__device__ __forceinline__ float pcm_fir(const float* p, const float* x, int n) {
  constexpr int K = Rate<Q>::k;
  if constexpr (!UP) {
    float acc = 0.f;
    const float* at = x + 2 * K * Q + Q * n;
#pragma unroll 8
    for (int j = 0; j <= 2 * K * Q; ++j) acc = fmaf(p[j], at[-j], acc);
    return acc;
  } else {
    return pcm_up_chain<Q>(p, x, n) * static_cast<float>(Q);
  }
}

// ---- samples <-> LDS floats, 16 bytes per lane ----------------------------------------------------------------------------------------------
// (src / dst 16-byte aligned, count a multiple of 8)
__device__ __forceinline__ void stage_in(const float* src, float* lds, int count, int tid) {
  for (int i = tid; i < count / 4; i += kThreads) reinterpret_cast<f32x4*>(lds)[i] = reinterpret_cast<const f32x4*>(src)[i];
}
__device__ __forceinline__ void stage_in(const short* src, float* lds, int count, int tid) {
  for (int i = tid; i < count / 8; i += kThreads) {
    const s16x8 v = reinterpret_cast<const s16x8*>(src)[i];
    f32x4 lo, hi;
    for (int k = 0; k < 4; ++k) {
      lo[k] = static_cast<float>(v[k]) * (1.f / 32768.f);      // exact
      hi[k] = static_cast<float>(v[4 + k]) * (1.f / 32768.f);
    }
    reinterpret_cast<f32x4*>(lds)[2 * i] = lo;
    reinterpret_cast<f32x4*>(lds)[2 * i + 1] = hi;
  }
}

__device__ __forceinline__ short to_s16(float y) {
  const float v = rintf(y * 32768.f);      // round to nearest even
  if (v != v) return 0;
  return static_cast<short>(static_cast<int>(fminf(fmaxf(v, -32768.f), 32767.f)));
}
__device__ __forceinline__ void stage_out(const float* lds, float* dst, int count, int tid) {
  for (int i = tid; i < count / 4; i += kThreads) reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(lds)[i];
}
__device__ __forceinline__ void stage_out(const float* lds, short* dst, int count, int tid) {
  for (int i = tid; i < count / 8; i += kThreads) {
    const f32x4 lo = reinterpret_cast<const f32x4*>(lds)[2 * i], hi = reinterpret_cast<const f32x4*>(lds)[2 * i + 1];
    s16x8 v;
    for (int k = 0; k < 4; ++k) {
      v[k] = to_s16(lo[k]);
      v[4 + k] = to_s16(hi[k]);
    }
    reinterpret_cast<s16x8*>(dst)[i] = v;
  }
}
__device__ __forceinline__ void zero_out(float* dst, int count, int tid) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < count / 4; i += kThreads) reinterpret_cast<f32x4*>(dst)[i] = z;
}
__device__ __forceinline__ void zero_out(short* dst, int count, int tid) {
  const s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < count / 8; i += kThreads) reinterpret_cast<s16x8*>(dst)[i] = z;
}

// ---- G.711: code <-> int16, integer bit operations (nutls.h, "G.711"; the host's statement of the same rule: api_pcm.cpp) ----------------------
// expand: the int16 value of code c (0 .. 255) -- mu-law +-32124, A-law +-32256
__device__ __forceinline__ int g711_expand(ulaw_t, unsigned c) {
  const unsigned u = ~c & 0xFFu;
  const int t = static_cast<int>((((u & 15u) << 3) + 0x84u) << ((u & 0x70u) >> 4));
  return (u & 0x80u) ? 0x84 - t : t - 0x84;
}
__device__ __forceinline__ int g711_expand(alaw_t, unsigned c) {
  const unsigned a = c ^ 0x55u;
  const unsigned g = (a & 0x70u) >> 4;
  int t = static_cast<int>((a & 15u) << 4);
  t = g == 0 ? t + 8 : (t + 0x108) << (g - 1);
  return (a & 0x80u) ? t : -t;
}
// compress: the code of the int16 value s.  The segment is the number of segment ends below the magnitude v: with the ends 2^(i + b) - 1,
// i = 0 .. 7 (b = 6 for mu-law, whose v carries the bias 33 and so has its leading bit at 5 or above; b = 5 for A-law), that is the position
// of v's leading bit minus (b - 1), and 0 for a v below the first end (A-law: v = 0 included, __clz(0) = 32).
__device__ __forceinline__ unsigned g711_compress(ulaw_t, int s) {
  int v = s >> 2;
  unsigned mask = 0xFFu;
  if (v < 0) {
    v = -v;
    mask = 0x7Fu;
  }
  v = min(v, 8159) + 33;                      // 33 .. 8192
  const int seg = 26 - __clz(v);              // 0 .. 8 (8: v = 8192 alone)
  const unsigned code = seg >= 8 ? 0x7Fu : static_cast<unsigned>((seg << 4) | ((v >> (seg + 1)) & 15));
  return code ^ mask;
}
__device__ __forceinline__ unsigned g711_compress(alaw_t, int s) {
  int v = s >> 3;
  unsigned mask = 0xD5u;
  if (v < 0) {
    v = -v - 1;
    mask = 0x55u;
  }
  const int seg = max(27 - __clz(v), 0);      // 0 .. 7 (v <= 4095)
  const unsigned code = seg >= 8 ? 0x7Fu : static_cast<unsigned>((seg << 4) | ((seg < 2 ? v >> 1 : v >> seg) & 15));
  return code ^ mask;
}
// what a zero hop compresses to, in every byte of a word
__device__ __forceinline__ unsigned g711_silence4(ulaw_t) { return 0xFFFFFFFFu; }
__device__ __forceinline__ unsigned g711_silence4(alaw_t) { return 0xD5D5D5D5u; }

// 16 codes per lane and access (src / dst 16-byte aligned, count a multiple of 16); byte k of word w of a lane's 16 bytes is its sample 4 w + k
template <typename G>
__device__ __forceinline__ void g711_stage_in(const G* src, float* lds, int count, int tid) {
  for (int i = tid; i < count / 16; i += kThreads) {
    const u32x4 v = reinterpret_cast<const u32x4*>(src)[i];
    for (int w = 0; w < 4; ++w) {
      f32x4 f;
      for (int k = 0; k < 4; ++k) f[k] = static_cast<float>(g711_expand(G{}, (v[w] >> (8 * k)) & 0xFFu)) * (1.f / 32768.f);      // exact
      reinterpret_cast<f32x4*>(lds)[4 * i + w] = f;
    }
  }
}
template <typename G>
__device__ __forceinline__ void g711_stage_out(const float* lds, G* dst, int count, int tid) {
  for (int i = tid; i < count / 16; i += kThreads) {
    u32x4 v;
    for (int w = 0; w < 4; ++w) {
      const f32x4 f = reinterpret_cast<const f32x4*>(lds)[4 * i + w];
      unsigned word = 0;
      for (int k = 0; k < 4; ++k) word |= g711_compress(G{}, to_s16(f[k])) << (8 * k);
      v[w] = word;
    }
    reinterpret_cast<u32x4*>(dst)[i] = v;
  }
}
template <typename G>
__device__ __forceinline__ void g711_silence_out(G* dst, int count, int tid) {
  const unsigned z = g711_silence4(G{});
  const u32x4 v = {z, z, z, z};
  for (int i = tid; i < count / 16; i += kThreads) reinterpret_cast<u32x4*>(dst)[i] = v;
}
__device__ __forceinline__ void stage_in(const ulaw_t* src, float* lds, int count, int tid) { g711_stage_in(src, lds, count, tid); }
__device__ __forceinline__ void stage_in(const alaw_t* src, float* lds, int count, int tid) { g711_stage_in(src, lds, count, tid); }
__device__ __forceinline__ void stage_out(const float* lds, ulaw_t* dst, int count, int tid) { g711_stage_out(lds, dst, count, tid); }
__device__ __forceinline__ void stage_out(const float* lds, alaw_t* dst, int count, int tid) { g711_stage_out(lds, dst, count, tid); }
__device__ __forceinline__ void zero_out(ulaw_t* dst, int count, int tid) { g711_silence_out(dst, count, tid); }      // "zero": the format's silence
__device__ __forceinline__ void zero_out(alaw_t* dst, int count, int tid) { g711_silence_out(dst, count, tid); }

// ---- follow: the upper band's gain follows the model (nutls.h, "Upper band", follow) ------------------------------------------------------------
// Everything here is fp32 in one fixed order, each operation rounded on its own: the pragma keeps the compiler from contracting a product
// into a sum, and / and __builtin_sqrtf are the correctly rounded ones (this file is built without fast-math).
// E2 of nutls.h for `slots` hops at once, by all 256 threads: s[256 j + i] = sample i of hop j on entry (thread i has written its own), the
// energy of hop j in s[256 j] on return (behind a barrier).  The ONE energy code of both halves: a of the decode half and b of the encode half
// are the same bits on the same samples.
__device__ __forceinline__ void pcm_e2(float* s, int slots, int tid) {
#pragma clang fp contract(off)
  for (int j = 0; j < slots; ++j) {
    const float v = s[256 * j + tid];
    s[256 * j + tid] = v * v;
  }
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h)
      for (int j = 0; j < slots; ++j) s[256 * j + tid] = s[256 * j + tid] + s[256 * j + tid + h];
    __syncthreads();
  }
}

// g of a hop from its two windows, oldest energy last: a1 .. a4 = a_{t-1} .. a_{t-4}, b0 .. b3 = b_t .. b_{t-3}
__device__ __forceinline__ float pcm_follow_gain(float gain, float a1, float a2, float a3, float a4, float b0, float b1, float b2, float b3) {
#pragma clang fp contract(off)
  const float A = ((a1 + a2) + a3) + a4;
  const float Bw = ((b0 + b1) + b2) + b3;
  const float r = __builtin_sqrtf(Bw / fmaxf(A, 0x1p-100f));
  return gain * fminf(r, 1.f);
}

// The samples pcm_e2 works on, in LDS: one array per size, the same one wherever a kernel asks for it
template <int N>
__device__ __forceinline__ float* pcm_follow_lds() {
  __shared__ float s_e[N];
  return s_e;
}

// gamma of the hop's caller sample n (S per hop): the linear ramp from g_prev (reached by the hop in front) to g_prev + delta
template <int S>
__device__ __forceinline__ float pcm_follow_ramp(float g_prev, float delta, int n) {
#pragma clang fp contract(off)
  const float w = static_cast<float>(n + 1) * static_cast<float>(1.0 / S);
  return fmaf(delta, w, g_prev);
}

// ---- one hop of one row: NIN samples in, NIN / Q (DOWN) or NIN * Q (UP) out --------------------------------------------------------------------
// UPPER (nutls_set_pcm_upper_band; rates above 16 kHz, so DOWN is the decode half and UP the encode half; ub: pcm.hpp, PcmUpper):
//   decode: after the hop's decoded samples d, u[n] = fmaf(-Q, c[n], x[n - 2 K Q]) for the hop's S = NIN caller samples, c[n] = pcm_up_chain over
//           d with its 2 K samples of left context (the UP chain without its product: E(D(x))[n] = Q c[n]), written to ub.u.  That context is the
//           carried one (ub.carry_in) for a row's first hop; a later hop of a block COMPUTES it -- the same chains over the same samples, so the
//           same bits -- from 2 K Q more input samples of the row (the decoded hop in front of it is another workgroup's of the same launch);
//   encode: out[n] = fmaf(gain, u'[n], z[n]), z the sample without the upper band, u' the u of the hop in front: ub.u's for a later hop of a
//           block, the carried one (ub.carry_in) for the first.  The workgroup of the row's last real hop carries that hop's u on.
// FOLLOW (nutls_set_pcm_upper_follow; with UPPER only; fo: pcm.hpp, PcmFollow): gain becomes the sample's gamma.
//   decode: a = pcm_e2 of the hop's 256 decoded samples, to fo.a[row, t] (one lane, one store);
//   encode: b of the hop and of the 4 in front of it by pcm_e2 -- the earlier hops of the call read again from the input row, those in front of the
//           call from the carried state, like their a (fo.a inside the call) --, lane 0 forms g_t and g_{t-1}, each from its own two windows, and
//           every lane its samples' gamma = the ramp between them.  The workgroup of the row's last real hop carries the last 5 a, 4 b and g on.
template <int Q, bool UP, int NIN, typename TI, typename TO, bool UPPER = false, bool FOLLOW = false>
__device__ __forceinline__ void pcm_hop(const TI* in, TO* out, const float* taps, const float* hist_in, float* hist_out, const unsigned char* active,
                                        const int* counts, int n_hops, const PcmUpper ub = PcmUpper{}, const PcmFollow fo = PcmFollow{}) {
  constexpr int K = Rate<Q>::k;
  constexpr int HIST = UP ? 2 * K : 2 * K * Q;      // samples of left context
  constexpr int NOUT = UP ? NIN * Q : NIN / Q;
  constexpr bool DEC_UPPER = UPPER && !UP, ENC_UPPER = UPPER && UP;
  constexpr int XPRE = DEC_UPPER ? HIST : 0;        // input samples in front of the left context: what the decoded context is computed from
  constexpr int YPRE = DEC_UPPER ? 2 * K : 0;       // decoded samples of left context in front of the hop's
  constexpr int CARRY = DEC_UPPER ? kPcmUpCtx : kPcmMaxHop, NCARRY = DEC_UPPER ? YPRE : NOUT;      // a row's carried upper-band state: stride, floats in use
  static_assert(HIST <= kPcmMaxHist && HIST <= NIN && NIN <= kPcmMaxHop && NOUT <= kPcmMaxHop, "staging sizes");
  static_assert(HIST % 8 == 0 && NIN % 8 == 0 && NOUT % 8 == 0, "16-byte accesses");
  // one-byte samples: 16 per access on the callers' side (the history is kept as floats: only a block's later hops stage HIST + XPRE codes from the row)
  static_assert((sizeof(TI) != 1 || ((HIST + XPRE) % 16 == 0 && NIN % 16 == 0)) && (sizeof(TO) != 1 || NOUT % 16 == 0), "16-byte accesses, one-byte samples");
  static_assert(!FOLLOW || (UPPER && (UP ? NIN : NOUT) == kThreads && kThreads == 256), "follow: one lane per 16 kHz sample of the hop");
  static_assert(!UPPER || (Q > 1 && YPRE == (DEC_UPPER ? kPcmUpCtx : 0) && YPRE + NOUT <= kPcmMaxHop && XPRE + HIST <= NIN && XPRE % 8 == 0 && YPRE % 8 == 0), "upper band: staging sizes");
  __shared__ __attribute__((aligned(16))) float s_x[(DEC_UPPER ? kPcmMaxHist : 0) + kPcmMaxHist + kPcmMaxHop];
  __shared__ __attribute__((aligned(16))) float s_y[kPcmMaxHop];
  __shared__ float s_p[Rate<kPcmMaxQ>::taps];
  float* const xs = s_x + XPRE;      // xs[0] = the oldest sample of the left context
  const int t = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
  TO* const dst = out + (static_cast<size_t>(row) * n_hops + t) * NOUT;
  if (active && !active[row]) {      // (the whole workgroup: the flag is per row)
    zero_out(dst, NOUT, tid);
    return;
  }
  const int k = counts ? min(max(counts[row], 0), n_hops) : n_hops;      // the row's real hops (the whole workgroup: the count is per row)
  if (t >= k) {      // behind the count: the input row is not read
    zero_out(dst, NOUT, tid);
    if constexpr (HIST > 0) {
      if (k == 0 && t == 0) {      // a held row: its history moves to the buffer the next call reads
        const f32x4* const from = reinterpret_cast<const f32x4*>(hist_in + static_cast<size_t>(row) * kPcmMaxHist);
        f32x4* const to = reinterpret_cast<f32x4*>(hist_out + static_cast<size_t>(row) * kPcmMaxHist);
        for (int i = tid; i < HIST / 4; i += kThreads) to[i] = from[i];
        if constexpr (UPPER) {       // and so does its upper-band state
          const f32x4* const ufrom = reinterpret_cast<const f32x4*>(ub.carry_in + static_cast<size_t>(row) * CARRY);
          f32x4* const uto = reinterpret_cast<f32x4*>(ub.carry_out + static_cast<size_t>(row) * CARRY);
          for (int i = tid; i < NCARRY / 4; i += kThreads) uto[i] = ufrom[i];
        }
        if constexpr (FOLLOW && UP) {      // and its follow state
          if (tid < kPcmFollowCarry) fo.carry_out[static_cast<size_t>(row) * kPcmFollowCarry + tid] = fo.carry_in[static_cast<size_t>(row) * kPcmFollowCarry + tid];
        }
      }
    }
    return;
  }
  const TI* const src = in + (static_cast<size_t>(row) * n_hops + t) * NIN;
  for (int i = tid; i < Rate<Q>::taps; i += kThreads) s_p[i] = taps[i];
  if constexpr (HIST > 0) {
    if (t > 0) {
      stage_in(src - HIST - XPRE, s_x, HIST + XPRE, tid);
    } else {
      stage_in(hist_in + static_cast<size_t>(row) * kPcmMaxHist, xs, HIST, tid);
      if constexpr (DEC_UPPER) stage_in(ub.carry_in + static_cast<size_t>(row) * CARRY, s_y, YPRE, tid);
    }
  }
  stage_in(src, xs + HIST, NIN, tid);
  if constexpr (FOLLOW && UP) {      // slot i of s_e: the 256 samples of hop t - i (a hop in front of the call: zeros, its b is the carried one)
    float* const s_e = pcm_follow_lds<(kPcmFollowHops + 1) * 256>();
    for (int i = 0; i <= kPcmFollowHops; ++i) s_e[i * 256 + tid] = t - i >= 0 ? src[tid - i * 256] : 0.f;
  }
  __syncthreads();
  if constexpr (HIST > 0) {
    // the history the next call starts from: the row's last real hop's.  hist_out may be hist_in only where this workgroup is also the one that read it (n_hops == 1)
    if (t == k - 1) stage_out(xs + NIN, hist_out + static_cast<size_t>(row) * kPcmMaxHist, HIST, tid);
  }
  if constexpr (DEC_UPPER) {
    // s_y = [2 K decoded samples of context | the hop's 256]: a later hop of a block computes the context, the first one has staged it
    for (int n = tid + (t > 0 ? 0 : YPRE); n < YPRE + NOUT; n += kThreads) s_y[n] = pcm_fir<Q, false>(s_p, xs, n - YPRE);
    __syncthreads();
    stage_out(s_y + YPRE, dst, NOUT, tid);
    if (t == k - 1) stage_out(s_y + NOUT, ub.carry_out + static_cast<size_t>(row) * CARRY, YPRE, tid);      // (read before the first barrier, by this workgroup, where it is carry_in)
    // u over the staged input, in place: xs[n] = x[n - 2 K Q] of the hop's sample n, and sample n is thread n's alone (the chain reads s_y and s_p)
    for (int n = tid; n < NIN; n += kThreads) xs[n] = fmaf(-static_cast<float>(Q), pcm_up_chain<Q>(s_p, s_y, n), xs[n]);
    __syncthreads();
    stage_out(xs, ub.u + (static_cast<size_t>(row) * n_hops + t) * NIN, NIN, tid);
    if constexpr (FOLLOW) {      // (s_y: complete behind the barriers above, only read from here on)
      float* const s_e = pcm_follow_lds<256>();
      s_e[tid] = s_y[YPRE + tid];
      pcm_e2(s_e, 1, tid);
      if (tid == 0) fo.a[static_cast<size_t>(row) * n_hops + t] = s_e[0];
    }
    return;
  }
  if constexpr (ENC_UPPER) {
    const float* const before = t > 0 ? ub.u + (static_cast<size_t>(row) * n_hops + t - 1) * NOUT : ub.carry_in + static_cast<size_t>(row) * CARRY;
    if constexpr (FOLLOW) {
      __shared__ float s_g[2];      // g_{t-1} and g_t - g_{t-1}
      float* const s_e = pcm_follow_lds<(kPcmFollowHops + 1) * 256>();
      pcm_e2(s_e, kPcmFollowHops + 1, tid);
      if (tid == 0) {
        const float* const ca = fo.carry_in + static_cast<size_t>(row) * kPcmFollowCarry;
        const float* const ar = fo.a + static_cast<size_t>(row) * n_hops;
        float a[kPcmFollowHops + 1], b[kPcmFollowHops + 1];      // a[i] = a_{t-1-i}, b[i] = b_{t-i}: inside the call or carried (hop -1 - j of the call: ca[j], ca[5 + j])
#pragma unroll
        for (int i = 0; i <= kPcmFollowHops; ++i) {
          a[i] = t - 1 - i >= 0 ? ar[t - 1 - i] : ca[i - t];
          b[i] = t - i >= 0 ? s_e[i * 256] : ca[kPcmFollowHops + i - t];
        }
        const float a_t = ar[t];
        const float g_now = pcm_follow_gain(ub.gain, a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]);
        const float g_prev = pcm_follow_gain(ub.gain, a[1], a[2], a[3], a[4], b[1], b[2], b[3], b[4]);
        s_g[0] = g_prev;
        s_g[1] = g_now - g_prev;
        if (t == k - 1) {      // (every carried value this lane needs is read above: carry_out may be carry_in where n_hops == 1)
          float* const co = fo.carry_out + static_cast<size_t>(row) * kPcmFollowCarry;
          co[0] = a_t;
#pragma unroll
          for (int i = 0; i < kPcmFollowHops; ++i) {
            co[1 + i] = a[i];
            co[kPcmFollowHops + 1 + i] = b[i];
          }
          co[kPcmFollowGainAt] = g_now;
        }
      }
      __syncthreads();
      const float g_prev = s_g[0], delta = s_g[1];
      for (int n = tid; n < NOUT; n += kThreads) s_y[n] = fmaf(pcm_follow_ramp<NOUT>(g_prev, delta, n), before[n], pcm_fir<Q, UP>(s_p, xs, n));
    } else {
      for (int n = tid; n < NOUT; n += kThreads) s_y[n] = fmaf(ub.gain, before[n], pcm_fir<Q, UP>(s_p, xs, n));
    }
  } else {
    for (int n = tid; n < NOUT; n += kThreads) s_y[n] = pcm_fir<Q, UP>(s_p, xs, n);
  }
  __syncthreads();
  stage_out(s_y, dst, NOUT, tid);
  if constexpr (ENC_UPPER) {      // behind the barrier: where carry_out is carry_in (n_hops == 1), every lane has read it.  (stage_out from global memory: a 16-byte copy)
    if (t == k - 1) stage_out(ub.u + (static_cast<size_t>(row) * n_hops + t) * NOUT, ub.carry_out + static_cast<size_t>(row) * CARRY, NOUT, tid);
  }
}

// The one kernel: a workgroup is one pcm_hop.  ub / fo are read by the instantiations with UPPER / FOLLOW alone.
template <int Q, bool UP, int NIN, typename TI, typename TO, bool UPPER, bool FOLLOW>
__global__ __launch_bounds__(kThreads) void pcm_kernel(const TI* in, TO* out, const float* taps, const float* hist_in, float* hist_out,
                                                       const unsigned char* active, const int* counts, int n_hops, PcmUpper ub, PcmFollow fo) {
  pcm_hop<Q, UP, NIN, TI, TO, UPPER, FOLLOW>(in, out, taps, hist_in, hist_out, active, counts, n_hops, ub, fo);
}

// ---- which instantiation a launch runs: each run-time value becomes a compile-time one in one place, and f is called with it ---------------------
template <typename F>
hipError_t with_rate(int rate_hz, F f) {
  switch (rate_hz) {
    case 8000: return f(std::integral_constant<int, 8000>{});
    case 16000: return f(std::integral_constant<int, 16000>{});
    case 32000: return f(std::integral_constant<int, 32000>{});
    case 48000: return f(std::integral_constant<int, 48000>{});
    default: return hipErrorInvalidValue;
  }
}
// (Q, UP) of a rate: the decode half reduces a rate above 16 kHz and doubles 8 kHz, the encode half undoes that
template <int HZ, bool ENC>
struct Resample {
  static constexpr int q = HZ == 16000 ? 1 : HZ == 48000 ? 3 : 2;
  static constexpr bool up = ENC ? HZ > 16000 : HZ < 16000;
};

template <typename F>
hipError_t with_sample_type(int fmt, F f) {
  switch (fmt) {
    case kPcmFmtF32: return f(float{});
    case kPcmFmtS16: return f(short{});
    case kPcmFmtUlaw: return f(ulaw_t{});
    case kPcmFmtAlaw: return f(alaw_t{});
    default: return hipErrorInvalidValue;
  }
}

template <typename F>
hipError_t with_mode(PcmMode mode, F f) {      // f(UPPER, FOLLOW)
  switch (mode) {
    case PcmMode::kPlain: return f(std::false_type{}, std::false_type{});
    case PcmMode::kUpper: return f(std::true_type{}, std::false_type{});
    case PcmMode::kFollow: return f(std::true_type{}, std::true_type{});
    default: return hipErrorInvalidValue;
  }
}

// The 36 kernels: 16 plain (4 rates x float32 / int16 x 2 halves), 4 G.711 (8 kHz, 2 laws x 2 halves), 8 with the upper band (32 / 48 kHz x
// float32 / int16 x 2 halves), 8 with follow (likewise).  Any other combination has no kernel: hipErrorInvalidValue.
template <bool ENC>
hipError_t launch_half(const PcmLaunch& L, hipStream_t s) {
  return with_rate(L.rate_hz, [&](auto hz) {
    return with_sample_type(L.fmt, [&](auto sample) {
      return with_mode(L.mode, [&](auto upper, auto follow) {
        constexpr int HZ = decltype(hz)::value;
        constexpr bool UPPER = decltype(upper)::value, FOLLOW = decltype(follow)::value;
        using T = decltype(sample);
        if constexpr (sizeof(T) == 1 ? HZ == 8000 && !UPPER : !UPPER || HZ > 16000) {
          constexpr int Q = Resample<HZ, ENC>::q;
          constexpr bool UP = Resample<HZ, ENC>::up;
          using TI = std::conditional_t<ENC, float, T>;      // the 16 kHz side is float32
          using TO = std::conditional_t<ENC, T, float>;
          constexpr int NIN = ENC ? 256 : UP ? 256 / Q : 256 * Q;
          hipLaunchKernelGGL((pcm_kernel<Q, UP, NIN, TI, TO, UPPER, FOLLOW>), dim3(L.n_hops, L.rows), dim3(kThreads), 0, s, static_cast<const TI*>(L.in),
                             static_cast<TO*>(L.out), L.taps, L.hist_in, L.hist_out, L.active, L.counts, L.n_hops, L.ub, L.fo);
          return hipGetLastError();
        } else {
          return hipErrorInvalidValue;
        }
      });
    });
  });
}

}  // namespace

int pcm_ratio(int rate_hz) {
  switch (rate_hz) {
    case 16000: return 1;
    case 8000: case 32000: return 2;
    case 48000: return 3;
    default: return 0;
  }
}

std::vector<float> pcm_design(int rate_hz) {
  const int q = pcm_ratio(rate_hz);
  if (q == 0) return {};
  if (q == 1) return {1.0f};
  const int half = kPcmK * q, n = 2 * half + 1;
  const double pi = 3.14159265358979323846, beta = 8.0;
  auto bessel_i0 = [](double x) {      // sum_k ((x / 2)^k / k!)^2
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 64; ++k) {
      term *= (x / 2) / k;
      sum += term * term;
    }
    return sum;
  };
  std::vector<double> p(n);
  double total = 0.0;
  for (int i = 0; i <= half; ++i) {      // one half, mirrored: symmetric to the bit
    const double d = static_cast<double>(i - half);
    // (the sinc's zeros -- every q-th tap off the centre -- are exact zeros, not sin(k pi) of a double: the prototype is a Nyquist filter)
    const double sinc = i == half ? 1.0 : (half - i) % q == 0 ? 0.0 : std::sin(pi * d / q) / (pi * d / q);
    const double r = d / half;
    const double v = sinc / q * bessel_i0(beta * std::sqrt(1.0 - r * r)) / bessel_i0(beta);
    p[i] = p[n - 1 - i] = v;
  }
  for (double v : p) total += v;
  std::vector<float> out(n);
  for (int i = 0; i < n; ++i) out[i] = static_cast<float>(p[i] / total);
  return out;
}

hipError_t launch_pcm(PcmDir dir, const PcmLaunch& L, hipStream_t s) {
  return dir == PcmDir::kEncode ? launch_half<true>(L, s) : launch_half<false>(L, s);
}

}  // namespace nutls
