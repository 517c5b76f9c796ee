// PCM gateway (nutls_set_pcm_format, the _pcm entries of nutls.h): what a handle keeps for it and the launchers of the two conversion
// kernels (pcm.hip).  Kept apart from nutls_internal.hpp, like ragged.hpp: the frame-step kernels have nothing to do with these.
//
// The library side of both kernels is [rows, n_hops * 256] float32 at 16 kHz; the caller side is [rows, n_hops * S] samples of the handle's
// format (float32 or int16) at its rate, S = 256 * rate / 16000.  q = max(rate, 16000) / min(rate, 16000) in {1, 2, 3}; the prototype
// p[0 .. 2 K q] (K = kPcmK low-rate samples of delay per direction; one tap, 1.0, at 16 kHz) is pcm_design()'s.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

namespace nutls {

constexpr int kPcmK = 24;                        // low-rate samples of delay per direction
constexpr int kPcmMaxQ = 3;
constexpr int kPcmMaxHist = 2 * kPcmK * kPcmMaxQ;      // floats of history per row and direction (the longest: 48 kHz decode)
constexpr int kPcmMaxHop = 256 * kPcmMaxQ;             // samples of a hop at the highest rate

// q of a supported rate (8000, 16000, 32000, 48000), else 0
int pcm_ratio(int rate_hz);
// The fp32 prototype of a supported rate: Kaiser-windowed sinc (beta 8) with its cutoff at the lower rate's Nyquist frequency, designed in
// double, normalised to sum 1, rounded once, symmetric to the bit; {1.0f} for 16000.  Host only.
std::vector<float> pcm_design(int rate_hz);

// What a handle keeps for its callers' format: allocated when a _pcm entry first needs it (api_pcm.cpp), zeroed by nutls_set_pcm_format and,
// row by row, by nutls_reset.
struct PcmState {
  int rate = 16000, fmt = 0;           // NUTLS_PCM_F32
  bool ready = false;                  // the buffers below exist
  int rows = 0;                        // streams of a streaming handle / utterances of an offline one
  float* taps = nullptr;               // the current rate's prototype on the device (2 K q + 1 floats)
  // the last 2 K q input samples of each direction's filter, [rows][kPcmMaxHist] floats (int16 input is kept converted: exact).  Two buffers
  // each: a block call of an offline handle reads [par] and writes [1 - par] (the workgroup of the block's first hop reads what the one of
  // its last hop replaces); a streaming handle stays on buffer 0 -- one workgroup per stream reads, then writes, and a held stream's is not touched.
  float *hist_dec[2] = {nullptr, nullptr}, *hist_enc[2] = {nullptr, nullptr};
  int dec_par = 0, enc_par = 0;
  float *f_in = nullptr, *f_out = nullptr;       // 16 kHz float32 around the model: [B, 256] / [utterances, max_frames * 256]
  unsigned char *raw_in = nullptr, *raw_out = nullptr;      // the _host entries' staging of the callers' samples (allocated on first use, sized for float32 at 48 kHz)
  unsigned char* d_active = nullptr;             // [B] device copy of the mask of nutls_enhance_hop_pcm_host_active
};

// Caller samples -> 16 kHz float32.  grid (n_hops, rows).  in: [rows, n_hops * S] of the format; out: [rows, n_hops * 256].  hist_in / hist_out:
// [rows][kPcmMaxHist]; they may be the same buffer when n_hops == 1.  active (device, [rows], may be null): a held row's history is not touched,
// its input is not read, its output hop is zeros.  counts (device, [rows], may be null: every row has n_hops): the row's leading real hops, clamped
// by the kernel to 0 .. n_hops -- the hops behind a count are zeros and their input is not read, the new history is that of the last real hop,
// and a row of count 0 has its history copied from hist_in to hist_out (with counts the two must be different buffers).
hipError_t launch_pcm_decode(const void* in, float* out, const float* taps, const float* hist_in, float* hist_out, const unsigned char* active,
                             const int* counts, int rate_hz, int s16, int rows, int n_hops, hipStream_t s);
// 16 kHz float32 -> caller samples; the same conventions the other way round.
hipError_t launch_pcm_encode(const float* in, void* out, const float* taps, const float* hist_in, float* hist_out, const unsigned char* active,
                             const int* counts, int rate_hz, int s16, int rows, int n_hops, hipStream_t s);

}  // namespace nutls
