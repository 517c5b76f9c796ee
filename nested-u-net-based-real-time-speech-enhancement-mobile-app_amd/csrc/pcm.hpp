// PCM gateway (nutls_set_pcm_format, the _pcm entries of nutls.h): what a handle keeps for it and the launcher of the conversion kernel
// (pcm.hip).  Kept apart from nutls_internal.hpp, like ragged.hpp: the frame-step kernels have nothing to do with these.
//
// The library side of both halves is [rows, n_hops * 256] float32 at 16 kHz; the caller side is [rows, n_hops * S] samples of the handle's
// format (float32 or int16; at 8 kHz also one byte of G.711, mu-law or A-law) at its rate, S = 256 * rate / 16000.  q = max(rate, 16000) / min(rate, 16000) in {1, 2, 3}; the prototype
// p[0 .. 2 K q] (K = kPcmK low-rate samples of delay per direction; one tap, 1.0, at 16 kHz) is pcm_design()'s.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

namespace nutls {

constexpr int kPcmK = 24;                        // low-rate samples of delay per direction
constexpr int kPcmMaxQ = 3;
constexpr int kPcmMaxHist = 2 * kPcmK * kPcmMaxQ;      // floats of history per row and direction (the longest: 48 kHz decode)
constexpr int kPcmMaxHop = 256 * kPcmMaxQ;             // samples of a hop at the highest rate
constexpr int kPcmUpCtx = 2 * kPcmK;                   // upper band: decoded samples of left context the decode half carries per row
constexpr int kPcmFollowHops = 4;                      // follow: hops of the two energy windows (NUTLS_PCM_FOLLOW_HOPS)
constexpr int kPcmFollowCarry = 16;                    // follow: floats a row carries -- [0 .. 4] the last 5 a, [5 .. 8] the last 4 b (newest first), [9] the last g
constexpr int kPcmFollowGainAt = 2 * kPcmFollowHops + 1;      // where g sits in them
// The sample formats, as PcmLaunch takes them in `fmt` (the values of NUTLS_PCM_F32, _S16, _ULAW and _ALAW: api_pcm.cpp asserts it)
constexpr int kPcmFmtF32 = 0, kPcmFmtS16 = 1, kPcmFmtUlaw = 2, kPcmFmtAlaw = 3;

// q of a supported rate (8000, 16000, 32000, 48000), else 0
int pcm_ratio(int rate_hz);
// The fp32 prototype of a supported rate: Kaiser-windowed sinc (beta 8) with its cutoff at the lower rate's Nyquist frequency, designed in
// double, normalised to sum 1, rounded once, symmetric to the bit; {1.0f} for 16000.  Host only.
std::vector<float> pcm_design(int rate_hz);

// The two halves of the gateway: caller samples -> 16 kHz float32, and back
enum class PcmDir { kDecode, kEncode };

// What one half carries from call to call, per row.  Every piece has two buffers: a block call of an offline handle reads [par] and writes
// [1 - par], then par flips (the workgroup of the block's first hop reads what the one of its last hop replaces); a streaming handle stays
// on buffer 0 -- one workgroup per stream reads, then writes, and a held stream's is not touched.  One parity for all of a half's pieces:
// they are written by the same workgroups under the same conditions.
struct PcmHalf {
  int up_stride;                               // floats per row of `up`: kPcmUpCtx (decode) / kPcmMaxHop (encode)
  int par = 0;
  float* hist[2] = {nullptr, nullptr};         // [rows][kPcmMaxHist] the last 2 K q input samples of the half's filter (int16 input is kept converted: exact)
  // upper band: decode -- the last 2 K DECODED samples (the left context of E(D(x))); encode -- u of the last real hop it has seen the decode of
  float* up[2] = {nullptr, nullptr};           // [rows][up_stride]
  float* fo[2] = {nullptr, nullptr};           // follow, encode only (decode: null): [rows][kPcmFollowCarry] as of the last real hop
};

// What a handle keeps for its callers' format: allocated when a _pcm entry first needs it (api_pcm.cpp), zeroed by nutls_set_pcm_format and,
// row by row, by nutls_reset.
struct PcmState {
  int rate = 16000, fmt = 0;           // NUTLS_PCM_F32; 2 / 3 (G.711 mu-law / A-law, one byte per sample) at 8000 only
  bool ready = false;                  // the buffers below (the halves' histories included) exist
  int rows = 0;                        // streams of a streaming handle / utterances of an offline one
  float* taps = nullptr;               // the current rate's prototype on the device (2 K q + 1 floats)
  PcmHalf dec = {kPcmUpCtx}, enc = {kPcmMaxHop};
  PcmHalf& half(PcmDir d) { return d == PcmDir::kDecode ? dec : enc; }
  float *f_in = nullptr, *f_out = nullptr;       // 16 kHz float32 around the model: [B, 256] / [utterances, max_frames * 256]
  unsigned char *raw_in = nullptr, *raw_out = nullptr;      // the _host entries' staging of the callers' samples (allocated on first use, sized for float32 at 48 kHz)
  unsigned char* d_active = nullptr;             // [B] device copy of the mask of nutls_enhance_hop_pcm_host_active
  // Upper band (nutls_set_pcm_upper_band; 32 / 48 kHz only): u = the delayed input minus its own low band, formed by the decode half and added
  // one hop later, times the gain, by the encode half.  Allocated when a gain other than 0 is first set; zeroed with the histories.
  float upper = 0.f;                   // the gain; 0: off -- the launches are the ones without the upper band
  bool upper_ready = false;            // the halves' `up` and the buffer below exist
  float* up_u = nullptr;               // [rows, n_hops * S] u of the last decoded hop / block (written by the decode half, read by the encode half)
  // Follow (nutls_set_pcm_upper_follow): the gain above becomes the ceiling of one that follows sqrt(energy handed to the encode half / energy
  // decoded) over kPcmFollowHops hops.  Allocated when follow is first enabled; zeroed with the histories.
  bool follow = false;                 // on: the launches are the upper band's with FOLLOW
  bool follow_ready = false;           // the encode half's `fo` and the buffer below exist
  float* fo_a = nullptr;               // [rows, n_hops] a = E2 of each hop of the last decoded hop / block (the contract of up_u)
};

// What a launch with the upper band gets on top (by value).  Decode: u = where the hops' u goes, [rows, n_hops * S]; carry_in / carry_out =
// [rows][kPcmUpCtx] decoded context.  Encode: u = the same buffer, read; carry_in / carry_out = [rows][kPcmMaxHop], the u of the hop in front of
// the call's first.  carry_in and carry_out follow the rules of hist_in and hist_out.  gain: the encode half's.
struct PcmUpper {
  float gain;
  float* u;
  const float* carry_in;
  float* carry_out;
};

// What a launch with follow gets on top of PcmUpper (by value).  Decode: a = where the hops' energies go, [rows, n_hops]; the rest is not used.
// Encode: a = the same buffer, read; carry_in / carry_out = [rows][kPcmFollowCarry], following the rules of hist_in and hist_out.
struct PcmFollow {
  float* a;
  const float* carry_in;
  float* carry_out;
};

// kUpper: with the upper band (ub is read); kFollow: with the upper band's gain following the model (ub and fo are read)
enum class PcmMode { kPlain, kUpper, kFollow };

// One launch of a half: grid (n_hops, rows).  Decode: in = [rows, n_hops * S] of the format, out = [rows, n_hops * 256] float32; encode: the
// other way round.  hist_in / hist_out: [rows][kPcmMaxHist]; they may be the same buffer when n_hops == 1.  active (device, [rows], may be
// null): a held row's history is not touched, its input is not read, its output hop is zeros (the encode half in a G.711 format: the
// format's silence code).  counts (device, [rows], may be null: every row has n_hops): the row's leading real hops, clamped by the kernel to
// 0 .. n_hops -- the hops behind a count are zeros (silence codes) and their input is not read, the new history is that of the last real
// hop, and a row of count 0 has its history copied from hist_in to hist_out (with counts the two must be different buffers).
// What exists: kPcmFmtF32 and kPcmFmtS16 at every rate, kPcmFmtUlaw and kPcmFmtAlaw at 8000 and kPlain alone, kUpper and kFollow at 32000
// and 48000 alone; ub / fo stay default-constructed where the mode does not read them.
struct PcmLaunch {
  const void* in;
  void* out;
  const float* taps;
  const float* hist_in;
  float* hist_out;
  const unsigned char* active;
  const int* counts;
  int rate_hz, fmt, rows, n_hops;
  PcmMode mode;
  PcmUpper ub;
  PcmFollow fo;
};
// hipErrorInvalidValue for a combination of rate, format and mode that does not exist: nothing is launched
hipError_t launch_pcm(PcmDir dir, const PcmLaunch& L, hipStream_t s);

}  // namespace nutls
