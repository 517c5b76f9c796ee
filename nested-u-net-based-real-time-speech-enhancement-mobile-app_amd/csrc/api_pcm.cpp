// PCM gateway of the C ABI (include/nutls.h, "PCM gateway"): a handle is told its callers' sample rate and sample type once
// (nutls_set_pcm_format), and the _pcm entries take and return that audio -- hop by hop with masks on streaming handles, block by block on
// offline ones.  Every entry here decodes into a library float32 buffer at 16 kHz, calls the existing entry (nutls_enhance_hop,
// nutls_enhance_hop_active, nutls_enhance_block) on library buffers and encodes: the model path, the masks, hop fusion and the state
// coherence are that code, not copies of it.  At 16000 / float32 the entries ARE the plain ones (forwarded before anything else happens).
// The _pcm_ragged block entries do the same around nutls_enhance_block_ragged, with the per-utterance hop counts handed to both kernels.
// Every launch of either half goes through half_launch, which picks the mode from the handle's settings -- so every entry honours them:
// upper band (nutls_set_pcm_upper_band, 32 / 48 kHz): with a gain other than 0 the launches also form and add the band above 8 kHz;
// follow (nutls_set_pcm_upper_follow): on top of that, the gain follows the model.  With a gain of 0 / follow off nothing here differs.
// G.711 (NUTLS_PCM_ULAW / NUTLS_PCM_ALAW, 8000 Hz only): a format like the others -- nutls_set_pcm_format validates it, sample_bytes is 1, the
// launch gets the format code; nothing else here knows.  The rule itself is stated once on the host (g711_expand / g711_compress below).
// Channels (nutls_set_pcm_channels): with more than one the callers' side of every entry is interleaved frame rows; through_channels splits it
// into one row per stream in front of the path above and joins the result behind it (channels.hip) -- at 16000 / float32 too, around the plain entry.
// The kernel template, its 36 instantiations and the one place that picks among them: pcm.hip.
#include <algorithm>
#include <cstdint>

#include "engine.hpp"

using namespace nutls;

namespace {

bool plain_format(const Engine* e) { return e->pcm.rate == 16000 && e->pcm.fmt == NUTLS_PCM_F32; }
int hop_samples(const Engine* e) { return NUTLS_FRAME_STEP / 16 * (e->pcm.rate / 1000); }      // 256 * rate / 16000
bool g711_format(int fmt) { return fmt == NUTLS_PCM_ULAW || fmt == NUTLS_PCM_ALAW; }
size_t sample_bytes(const Engine* e) { return g711_format(e->pcm.fmt) ? 1 : e->pcm.fmt == NUTLS_PCM_S16 ? sizeof(short) : sizeof(float); }
int max_hops(const Engine* e) { return e->offline ? e->offline : 1; }
static_assert(NUTLS_PCM_F32 == kPcmFmtF32 && NUTLS_PCM_S16 == kPcmFmtS16 && NUTLS_PCM_ULAW == kPcmFmtUlaw && NUTLS_PCM_ALAW == kPcmFmtAlaw,
              "PcmLaunch of pcm.hpp takes the format codes of nutls.h");

// ---- G.711, the rule as nutls.h words it ("G.711"): what nutls_pcm_g711_expand / _compress return and what the kernels of pcm.hip agree with ----
int g711_expand(int fmt, int c) {
  if (fmt == NUTLS_PCM_ULAW) {
    const int u = ~c & 0xFF;
    const int t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4);
    return (u & 0x80) ? 0x84 - t : t - 0x84;
  }
  const int a = c ^ 0x55;
  int t = (a & 15) << 4;
  const int g = (a & 0x70) >> 4;
  t = g == 0 ? t + 8 : (t + 0x108) << (g - 1);
  return (a & 0x80) ? t : -t;
}

int g711_segment(int v, int first_end) {      // how many of the 8 segment ends first_end, 2 first_end + 1, ... v exceeds
  int seg = 0;
  for (int end = first_end; seg < 8 && v > end; end = 2 * end + 1) ++seg;
  return seg;
}

unsigned char g711_compress(int fmt, int s) {
  if (fmt == NUTLS_PCM_ULAW) {
    int v = s >> 2, mask = 0xFF;
    if (v < 0) {
      v = -v;
      mask = 0x7F;
    }
    v = (v < 8159 ? v : 8159) + 33;
    const int seg = g711_segment(v, 0x3F);
    return static_cast<unsigned char>((seg >= 8 ? 0x7F : (seg << 4) | ((v >> (seg + 1)) & 15)) ^ mask);
  }
  int v = s >> 3, mask = 0xD5;
  if (v < 0) {
    v = -v - 1;
    mask = 0x55;
  }
  const int seg = g711_segment(v, 0x1F);
  return static_cast<unsigned char>((seg >= 8 ? 0x7F : (seg << 4) | ((seg < 2 ? v >> 1 : v >> seg) & 15)) ^ mask);
}

int upload_taps(Engine* e) {
  const std::vector<float> p = pcm_design(e->pcm.rate);
  HIP_TRY(hipMemcpy(e->pcm.taps, p.data(), p.size() * sizeof(float), hipMemcpyHostToDevice));
  return NUTLS_OK;
}

// Buffers of the gateway, allocated when an entry first needs them (every later call: nothing happens).
int pcm_init(Engine* e) {
  PcmState& st = e->pcm;
  if (st.ready) return NUTLS_OK;
  st.rows = e->offline ? e->outt : e->B;
  const size_t hist = static_cast<size_t>(st.rows) * kPcmMaxHist;
  const size_t wave = static_cast<size_t>(st.rows) * max_hops(e) * NUTLS_FRAME_STEP;
  if (int rc = dev_alloc_once(e, static_cast<size_t>(2 * kPcmK * kPcmMaxQ + 1), &st.taps, false)) return rc;
  for (PcmHalf* half : {&st.dec, &st.enc})
    for (float*& p : half->hist)
      if (int rc = dev_alloc_once(e, hist, &p, true)) return rc;
  int rc;
  if ((rc = dev_alloc_once(e, wave, &st.f_in, true)) || (rc = dev_alloc_once(e, wave, &st.f_out, true)) || (rc = upload_taps(e))) return rc;
  HIP_TRY(hipDeviceSynchronize());      // the zeroes are in place before a caller's stream reads them
  st.ready = true;
  return NUTLS_OK;
}

// The upper band's buffers (nutls_set_pcm_upper_band), allocated when a gain other than 0 is first set -- after pcm_init.
int upper_init(Engine* e) {
  PcmState& st = e->pcm;
  if (st.upper_ready) return NUTLS_OK;
  const size_t rows = static_cast<size_t>(st.rows);
  for (PcmHalf* half : {&st.dec, &st.enc})
    for (float*& p : half->up)
      if (int rc = dev_alloc_once(e, rows * half->up_stride, &p, true)) return rc;
  if (int rc = dev_alloc_once(e, rows * max_hops(e) * kPcmMaxHop, &st.up_u, true)) return rc;
  st.upper_ready = true;
  return NUTLS_OK;
}

// Follow's buffers (nutls_set_pcm_upper_follow), allocated when follow is first enabled -- after upper_init.  The carry is the encode half's alone.
int follow_init(Engine* e) {
  PcmState& st = e->pcm;
  if (st.follow_ready) return NUTLS_OK;
  const size_t rows = static_cast<size_t>(st.rows);
  if (int rc = dev_alloc_once(e, rows * max_hops(e), &st.fo_a, true)) return rc;
  for (float*& p : st.enc.fo)
    if (int rc = dev_alloc_once(e, rows * kPcmFollowCarry, &p, true)) return rc;
  st.follow_ready = true;
  return NUTLS_OK;
}

// Row idx's (< 0: every row's) carried state in both halves -- resampler histories, upper band, follow --, where it exists.  (up_u and fo_a are
// not state: the encode half reads only what the decode half of the same hop or block wrote there.)
int zero_histories(Engine* e, int idx) {
  PcmState& st = e->pcm;
  if (!st.ready) return NUTLS_OK;
  auto zero = [&](float* p, size_t stride) -> int {
    if (idx < 0) HIP_TRY(hipMemset(p, 0, static_cast<size_t>(st.rows) * stride * sizeof(float)));
    else HIP_TRY(hipMemset(p + static_cast<size_t>(idx) * stride, 0, stride * sizeof(float)));
    return NUTLS_OK;
  };
  for (PcmHalf* half : {&st.dec, &st.enc})
    for (int i = 0; i < 2; ++i) {
      if (int rc = zero(half->hist[i], kPcmMaxHist)) return rc;
      if (st.upper_ready)
        if (int rc = zero(half->up[i], half->up_stride)) return rc;
      if (st.follow_ready && half->fo[i])      // (follow is enabled under a gain other than 0 only: the upper band's buffers exist)
        if (int rc = zero(half->fo[i], kPcmFollowCarry)) return rc;
    }
  return NUTLS_OK;
}

// One launch of a half.  A block call (offline handle) flips the half's buffers -- histories, upper-band and follow carry alike: one parity --;
// a hop call (streaming handle) works in place on buffer 0.  counts: the DEVICE counts of a ragged block or null (the flip is the whole
// handle's: the kernel carries a held row's state across).  The mode is the handle's: with the upper band on (a gain other than 0) the launch
// also forms / adds it, with follow on top its gain follows the model.
int half_launch(Engine* e, PcmDir dir, const void* in, void* out, const unsigned char* active, int n_hops, hipStream_t s, const int* counts = nullptr) {
  PcmState& st = e->pcm;
  PcmHalf& half = st.half(dir);
  if (int rc = enqueue_on(e, s)) return rc;
  const int par = half.par, nxt = e->offline ? 1 - par : par;
  PcmLaunch L = {in, out, st.taps, half.hist[par], half.hist[nxt], active, counts, st.rate, st.fmt, st.rows, n_hops, PcmMode::kPlain, {}, {}};
  if (st.upper != 0.f) {
    L.mode = st.follow ? PcmMode::kFollow : PcmMode::kUpper;
    L.ub = {st.upper, st.up_u, half.up[par], half.up[nxt]};
    if (st.follow) L.fo = {st.fo_a, half.fo[par], half.fo[nxt]};
  }
  HIP_TRY(launch_pcm(dir, L, s));
  half.par = nxt;
  return NUTLS_OK;
}

// the handle's device is current and the gateway's buffers exist
int pcm_ready(Engine* e) {
  HIP_TRY(hipSetDevice(e->device));
  return pcm_init(e);
}

// ---- channels (nutls.h, "Channels"; the kernels: channels.hip) ------------------------------------------------------------------------------
int grow_pair(Engine* e, size_t bytes, unsigned char** a, unsigned char** b, size_t* cap);      // (below, with packet mode)

int handle_rows(const Engine* e) { return e->offline ? e->outt : e->B; }
// at 16000 / float32 with one channel the _pcm entries ARE the plain ones; with more they are split -> the plain entry -> join
bool plain_entry(const Engine* e) { return plain_format(e) && e->chn.C == 1; }

// The callers' side of an entry in the layout in force, on stream s (the handle's device is current, every refusal is behind us).  pcm_in /
// pcm_out: the callers' buffers [rows / C][n * C] -- either may be null: the entry has no such side.  rows_path(in, out) is the 1-channel
// entry on [rows][n].  With one channel it gets the callers' buffers and nothing else happens; with more, pcm_in is split into the
// library's buffer before rows_path runs and its result joined into pcm_out behind it, so pcm_in == pcm_out stays allowed.  The two buffers
// are sized here, at call time, for the largest call the format in force allows (a block of max_frames hops, a packet): they grow only
// behind a change of format or packet length, and those have synchronised.
template <typename F>
int through_channels(Engine* e, const void* pcm_in, void* pcm_out, int n, hipStream_t s, F rows_path) {
  ChannelState& ch = e->chn;
  if (ch.C == 1) return rows_path(pcm_in, pcm_out);
  const int rows = handle_rows(e), bytes = static_cast<int>(sample_bytes(e));
  const size_t most = std::max(static_cast<size_t>(max_hops(e)) * hop_samples(e), static_cast<size_t>(e->pkt.P));
  if (int rc = grow_pair(e, rows * most * bytes, &ch.split, &ch.join, &ch.cap)) return rc;
  const int q = static_cast<int>(static_cast<size_t>(n) * bytes / 16);
  if (pcm_in) {
    if (int rc = enqueue_on(e, s)) return rc;
    HIP_TRY(launch_channels(bytes, ch.C, false, {pcm_in, ch.split, rows / ch.C, q}, s));
  }
  if (int rc = rows_path(pcm_in ? ch.split : nullptr, pcm_out ? ch.join : nullptr)) return rc;
  if (pcm_out) {
    if (int rc = enqueue_on(e, s)) return rc;
    HIP_TRY(launch_channels(bytes, ch.C, true, {ch.join, pcm_out, rows / ch.C, q}, s));
  }
  return NUTLS_OK;
}

// The rule on the host: what nutls_pcm_deinterleave / nutls_pcm_interleave do.  in [outer][inner] -> out [inner][outer], elements of `bytes` bytes.
void transpose_bytes(const unsigned char* in, unsigned char* out, size_t outer, size_t inner, size_t bytes) {
  for (size_t i = 0; i < outer; ++i)
    for (size_t j = 0; j < inner; ++j) std::copy_n(in + (i * inner + j) * bytes, bytes, out + (j * outer + i) * bytes);
}

int channels_host(const char* who, int fmt, int channels, const void* in, void* out, size_t n, bool join) {
  const size_t bytes = fmt == NUTLS_PCM_F32 ? 4 : fmt == NUTLS_PCM_S16 ? 2 : g711_format(fmt) ? 1 : 0;
  if (!bytes) return fail(NUTLS_ERR_ARG, std::string(who) + ": sample format must be NUTLS_PCM_F32, NUTLS_PCM_S16, NUTLS_PCM_ULAW or NUTLS_PCM_ALAW");
  if (channels != 2 && channels != 4) return fail(NUTLS_ERR_ARG, std::string(who) + ": channels must be 2 or 4, not " + std::to_string(channels));
  if (!in || !out) return fail(NUTLS_ERR_ARG, std::string(who) + ": null pointer");
  const size_t c = static_cast<size_t>(channels);
  transpose_bytes(static_cast<const unsigned char*>(in), static_cast<unsigned char*>(out), join ? c : n, join ? n : c, bytes);
  return NUTLS_OK;
}

// what the entries of one half on its own do behind their refusals: the callers' side is `in` of a decode, `out` of an encode
int half_entry(nutls_handle* h, PcmDir dir, const void* in, void* out, const unsigned char* active, int n_hops, void* stream, const int* counts = nullptr) {
  Engine* e = &h->eng;
  if (int rc = pcm_ready(e)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = n_hops * hop_samples(e);
  if (dir == PcmDir::kDecode)
    return through_channels(e, in, nullptr, n, s, [&](const void* rows, void*) { return half_launch(e, dir, rows, out, active, n_hops, s, counts); });
  return through_channels(e, nullptr, out, n, s, [&](const void*, void* rows) { return half_launch(e, dir, in, rows, active, n_hops, s, counts); });
}

// the _host entries' staging of the callers' samples
int raw_init(Engine* e) {
  const size_t bytes = static_cast<size_t>(e->pcm.rows) * max_hops(e) * kPcmMaxHop * sizeof(float);
  if (int rc = dev_alloc_once(e, bytes, &e->pcm.raw_in, false)) return rc;
  return dev_alloc_once(e, bytes, &e->pcm.raw_out, false);
}

int dc_ok(int dc_mode, const char* who) {
  if (dc_mode != NUTLS_DC_EDGE && dc_mode != NUTLS_DC_ZERO) return fail(NUTLS_ERR_ARG, std::string(who) + ": dc_mode must be NUTLS_DC_EDGE or NUTLS_DC_ZERO");
  return NUTLS_OK;
}

// what every hop entry checks first: pointers, then the kind of handle
int hop_args(nutls_handle* h, bool pointers_ok, const char* who) {
  if (!h || !pointers_ok) return fail(NUTLS_ERR_ARG, std::string(who) + ": null pointer");
  if (h->eng.offline)
    return fail(NUTLS_ERR_ARG, std::string(who) + ": offline handle (nutls_create_offline): it takes the callers' samples block by block through nutls_enhance_block_pcm");
  return NUTLS_OK;
}

int block_args(nutls_handle* h, bool pointers_ok, int n_hops, const char* who) {
  if (!h || !pointers_ok) return fail(NUTLS_ERR_ARG, std::string(who) + ": null pointer");
  const Engine* e = &h->eng;
  if (!e->offline)
    return fail(NUTLS_ERR_ARG, std::string(who) + ": not an offline handle (nutls_create_offline); a streaming handle takes the callers' samples hop by hop through nutls_enhance_hop_pcm");
  if (n_hops < 1 || n_hops > e->offline) return fail(NUTLS_ERR_ARG, std::string(who) + ": n_hops out of range (1 .. max_frames)");
  return NUTLS_OK;
}

// Refusals of a converting hop come before the decode: a refused call leaves the resampler histories where they were.
int hop_refusals(nutls_handle* h, const unsigned char* active, int dc_mode, const char* who) {
  if (int rc = dc_ok(dc_mode, who)) return rc;
  if (active)
    if (int rc = check_active(&h->eng, who)) return rc;
  return NUTLS_OK;
}

// One row per stream: decode -> nutls_enhance_hop(_active) on the library's float buffers -> encode (active: device mask or null).  At
// 16000 / float32 (reached with more than one channel only: plain_entry) the rows are the plain entry's.
int hop_rows(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode, void* stream) {
  Engine* e = &h->eng;
  if (int rc = pcm_ready(e)) return rc;
  if (plain_format(e)) return nutls_enhance_hop_active(h, static_cast<const float*>(pcm_in), static_cast<float*>(pcm_out), active, dc_mode, stream);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = half_launch(e, PcmDir::kDecode, pcm_in, e->pcm.f_in, active, 1, s)) return rc;
  if (int rc = nutls_enhance_hop_active(h, e->pcm.f_in, e->pcm.f_out, active, dc_mode, stream)) return rc;
  return half_launch(e, PcmDir::kEncode, e->pcm.f_out, pcm_out, active, 1, s);
}

// ... in the callers' layout
int hop_device(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode, void* stream) {
  Engine* e = &h->eng;
  if (int rc = pcm_ready(e)) return rc;
  return through_channels(e, pcm_in, pcm_out, hop_samples(e), static_cast<hipStream_t>(stream),
                          [&](const void* in, void* out) { return hop_rows(h, in, out, active, dc_mode, stream); });
}

// decode -> nutls_enhance_block(_ragged) on the library's float buffers -> encode.  hops: the DEVICE counts of a ragged block, handed to all
// three parts, or null.  With counts the decode writes zero hops behind them into the library's buffer, nutls_enhance_block_ragged reads none
// of them and writes zeros there, the encode reads none of those.
// One row per utterance; at 16000 / float32 (reached with more than one channel only: plain_entry) the rows are the plain entry's.
int block_rows(nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream) {
  Engine* e = &h->eng;
  if (int rc = pcm_ready(e)) return rc;
  if (plain_format(e)) return nutls_enhance_block_ragged(h, static_cast<const float*>(pcm_in), static_cast<float*>(pcm_out), n_hops, hops, dc_mode, stream);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = half_launch(e, PcmDir::kDecode, pcm_in, e->pcm.f_in, nullptr, n_hops, s, hops)) return rc;
  if (int rc = nutls_enhance_block_ragged(h, e->pcm.f_in, e->pcm.f_out, n_hops, hops, dc_mode, stream)) return rc;      // (null hops: nutls_enhance_block)
  return half_launch(e, PcmDir::kEncode, e->pcm.f_out, pcm_out, nullptr, n_hops, s, hops);
}

// ... in the callers' layout
int block_device(nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream) {
  Engine* e = &h->eng;
  if (int rc = pcm_ready(e)) return rc;
  return through_channels(e, pcm_in, pcm_out, n_hops * hop_samples(e), static_cast<hipStream_t>(stream),
                          [&](const void* in, void* out) { return block_rows(h, in, out, n_hops, hops, dc_mode, stream); });
}

// What the _host entries share, on the library's stream (the entry has put it behind what earlier calls queued on the callers' streams):
// `samples` of the callers' format to the library's staging, device_path(staged in, staged out) on that stream, the results back, one
// synchronisation.
template <typename F>
int through_staging(Engine* e, unsigned char* raw_in, unsigned char* raw_out, const void* pcm_in, void* pcm_out, size_t samples, F device_path) {
  const size_t bytes = samples * sample_bytes(e);
  HIP_TRY(hipMemcpyAsync(raw_in, pcm_in, bytes, hipMemcpyHostToDevice, e->stream));
  if (int rc = device_path(raw_in, raw_out)) return rc;
  HIP_TRY(hipMemcpyAsync(pcm_out, raw_out, bytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  enqueue_idle(e);
  return NUTLS_OK;
}

// ... through the hop and block entries' staging (raw_init)
template <typename F>
int through_staging(Engine* e, const void* pcm_in, void* pcm_out, size_t samples, F device_path) {
  return through_staging(e, e->pcm.raw_in, e->pcm.raw_out, pcm_in, pcm_out, samples, device_path);
}

// hop_device through the staging (active: HOST mask or null).  The mask is handed on as a device mask: the library does not follow it through
// nutls_state_set's bookkeeping as the float _host entries do (nutls.h, nutls_step_active: the more expensive launches then last until one
// call steps all streams).
int hop_host(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode) {
  Engine* e = &h->eng;
  if (int rc = pcm_ready(e)) return rc;
  if (int rc = raw_init(e)) return rc;
  if (int rc = enqueue_on(e, e->stream)) return rc;      // (behind what earlier calls queued on the callers' streams)
  const unsigned char* d_act = nullptr;
  if (active) {
    if (int rc = dev_alloc_once(e, static_cast<size_t>(e->B), &e->pcm.d_active, false)) return rc;
    HIP_TRY(hipMemcpyAsync(e->pcm.d_active, active, static_cast<size_t>(e->B), hipMemcpyHostToDevice, e->stream));
    d_act = e->pcm.d_active;
  }
  return through_staging(e, pcm_in, pcm_out, static_cast<size_t>(e->B) * hop_samples(e),
                         [&](const void* in, void* out) { return hop_device(h, in, out, d_act, dc_mode, e->stream); });
}

// block_device through the staging (hops: DEVICE counts or null; with counts the rows behind them cross the link too: the kernels do not read
// them on the device)
int block_host(nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, const int* hops, int dc_mode) {
  Engine* e = &h->eng;
  return through_staging(e, pcm_in, pcm_out, static_cast<size_t>(e->outt) * n_hops * hop_samples(e),
                         [&](const void* in, void* out) { return block_device(h, in, out, n_hops, hops, dc_mode, e->stream); });
}

// the 16-byte alignment nutls.h asks of every _pcm buffer is checked where counts come with it, as the ragged float entries do
int aligned16(const void* a, const void* b, const char* who) {
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15)
    return fail(NUTLS_ERR_ARG, std::string(who) + ": with hop counts the buffers must be 16-byte aligned");
  return NUTLS_OK;
}

// ---- packet mode (nutls.h, "Packet mode"; the kernels: packet.hip) ------------------------------------------------------------------------------
int gcd_of(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// The length rule, host only: what nutls_pcm_packet_plan states and nutls_set_pcm_packet enforces.
struct PacketPlan {
  int S, bytes, D, R, L;
};
int packet_plan(int rate_hz, int fmt, int samples, PacketPlan* plan, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (!pcm_ratio(rate_hz)) return fail(NUTLS_ERR_ARG, w + "rate must be 8000, 16000, 32000 or 48000");
  if (fmt != NUTLS_PCM_F32 && fmt != NUTLS_PCM_S16 && !g711_format(fmt))
    return fail(NUTLS_ERR_ARG, w + "sample format must be NUTLS_PCM_F32, NUTLS_PCM_S16, NUTLS_PCM_ULAW or NUTLS_PCM_ALAW");
  if (g711_format(fmt) && rate_hz != 8000) return fail(NUTLS_ERR_ARG, w + "NUTLS_PCM_ULAW and NUTLS_PCM_ALAW are G.711, which is 8 kHz: rate must be 8000 with them");
  const int S = NUTLS_FRAME_STEP / 16 * (rate_hz / 1000);
  const int bytes = g711_format(fmt) ? 1 : fmt == NUTLS_PCM_S16 ? 2 : 4;
  if (samples < 1 || samples > kPacketMaxRounds * S)
    return fail(NUTLS_ERR_ARG, w + "a packet has 1 .. " + std::to_string(kPacketMaxRounds * S) + " samples (four hops) at this rate, not " + std::to_string(samples));
  if (samples * bytes % 16)
    return fail(NUTLS_ERR_ARG, w + "a packet's bytes must be a multiple of 16 (rows stay 16-byte aligned): " + std::to_string(samples) + " samples of " +
                                   std::to_string(bytes) + " bytes are not");
  const int g = gcd_of(samples, S);
  *plan = {S, bytes, S - g, (S - g + samples) / S, S - g + samples};
  return NUTLS_OK;
}

// Two device buffers of one size that grow with the largest request a handle has seen (the old ones are freed: nothing is queued on them, the
// callers have synchronised).
int grow_pair(Engine* e, size_t bytes, unsigned char** a, unsigned char** b, size_t* cap) {
  if (*cap >= bytes) return NUTLS_OK;
  for (unsigned char** p : {a, b}) {
    if (*p) {
      e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), static_cast<void*>(*p)));
      HIP_TRY(hipFree(*p));
      *p = nullptr;
    }
    if (int rc = dev_alloc_once(e, bytes, p, true)) return rc;
  }
  *cap = bytes;
  return NUTLS_OK;
}

// Row idx's (< 0: every row's) FIFOs as a stream starts with them: input empty, output D samples of silence (the whole ring row is filled with
// the silence byte, of which the first D samples count).  The mirror follows where the host still has one.
int packet_prime(Engine* e, int idx) {
  PacketState& k = e->pkt;
  if (!k.P) return NUTLS_OK;
  const size_t row = static_cast<size_t>(k.L) * k.bytes, first = idx < 0 ? 0 : static_cast<size_t>(idx), n = idx < 0 ? static_cast<size_t>(e->B) : 1;
  HIP_TRY(hipMemset(k.ctr + first, 0, n * sizeof(PacketCtr)));
  HIP_TRY(hipMemset(k.out_ring + first * row, static_cast<int>(k.silence & 0xFF), n * row));
  if (idx < 0) {
    k.mirror.assign(static_cast<size_t>(e->B), 0);
    k.mirror_known = true;
  } else if (k.mirror_known) {
    k.mirror[first] = 0;
  }
  return NUTLS_OK;
}

// A tick's rounds need masked hops when the packets do not cut into whole hops or when the caller passes a mask: then packet mode works where
// check_active says masks do, and says so with its reason.
bool packet_masked(int samples, int S, const unsigned char* active) { return samples % S != 0 || active != nullptr; }

// what both packet entries check before anything is pushed: a refused call changes nothing
int packet_refusals(nutls_handle* h, bool pointers_ok, const unsigned char* active, int dc_mode, const char* who) {
  if (int rc = hop_args(h, pointers_ok, who)) return rc;
  const Engine* e = &h->eng;
  if (!e->pkt.P) return fail(NUTLS_ERR_ARG, std::string(who) + ": packet mode is off (nutls_set_pcm_packet with the packets' samples first)");
  if (int rc = dc_ok(dc_mode, who)) return rc;
  if (packet_masked(e->pkt.P, e->pkt.S, active)) return check_active(e, who);
  return e->mode == 3 ? NUTLS_OK : refuse_per_layer_in_causal32(e, who);
}

// One hop round on the library's hop buffers: the existing hop entry of the handle's format (ready: DEVICE mask or null)
int packet_hop(nutls_handle* h, const void* in, void* out, const unsigned char* ready, int dc_mode, hipStream_t s) {
  if (plain_format(&h->eng)) return nutls_enhance_hop_active(h, static_cast<const float*>(in), static_cast<float*>(out), ready, dc_mode, s);
  return hop_rows(h, in, out, ready, dc_mode, s);      // (the library's hop buffers: one row per stream whatever the callers' layout)
}

// One tick on stream s (the handle's device is current, every refusal is behind us).  active: the DEVICE mask the kernels read, or null;
// seen: the same mask in HOST memory where the host has it (the _host entry), null otherwise.  How many rounds: while the host has a mirror of
// the counters, exactly those in which some stream is ready -- each round's ready mask goes to note_active, as the float _host entries' masks
// do --; after a DEVICE mask the mirror is unknown and every tick issues R rounds, whose ready masks only the device knows.
int packet_tick(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, const unsigned char* seen, int dc_mode, hipStream_t s) {
  Engine* e = &h->eng;
  PacketState& k = e->pkt;
  const bool masked = packet_masked(k.P, k.S, active);
  if (active && !seen) k.mirror_known = false;
  std::vector<std::vector<unsigned char>> ready;      // per round, while the mirror is known
  int rounds = k.R;
  if (k.mirror_known) {
    for (int b = 0; b < e->B; ++b)
      if (!seen || seen[b]) k.mirror[b] += k.P;
    for (;;) {
      std::vector<unsigned char> m(static_cast<size_t>(e->B), 0);
      bool any = false;
      for (int b = 0; b < e->B; ++b)
        if ((!seen || seen[b]) && k.mirror[b] >= k.S) {
          k.mirror[b] -= k.S;
          m[b] = 1;
          any = true;
        }
      if (!any) break;
      ready.push_back(std::move(m));
    }
    rounds = static_cast<int>(ready.size());
  }
  if (int rc = enqueue_on(e, s)) return rc;
  const int q = 16 / k.bytes;      // samples of a quad
  const PacketLaunch L = {pcm_in, pcm_out, active, k.in_ring, k.out_ring, k.hop_in, k.hop_out, k.ctr, k.ready, e->B, k.P / q, k.S / q, k.D / q, k.L / q, k.silence};
  k.last_rounds = rounds;
  if (rounds == 0) {
    HIP_TRY(launch_packet(PacketBody::kPushPop, L, s));
    return NUTLS_OK;
  }
  HIP_TRY(launch_packet(PacketBody::kPushStage, L, s));
  for (int r = 0; r < rounds; ++r) {
    if (int rc = packet_hop(h, k.hop_in, k.hop_out, masked ? k.ready : nullptr, dc_mode, s)) return rc;
    if (masked && k.mirror_known) note_active(e, ready[r].data());
    HIP_TRY(launch_packet(r + 1 < rounds ? PacketBody::kTurn : PacketBody::kTurnPop, L, s));
  }
  return NUTLS_OK;
}

// ... with the packets in the callers' layout
int packet_device(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, const unsigned char* seen, int dc_mode, hipStream_t s) {
  return through_channels(&h->eng, pcm_in, pcm_out, h->eng.pkt.P, s,
                          [&](const void* in, void* out) { return packet_tick(h, in, out, active, seen, dc_mode, s); });
}

}  // namespace

namespace nutls {

int pcm_reset(Engine* e, int idx) {
  if (int rc = zero_histories(e, idx)) return rc;
  return packet_prime(e, idx);
}

}  // namespace nutls

extern "C" {

// ---- the format of a handle ---------------------------------------------------------------------------------------------------------------
int nutls_pcm_filter_taps(int rate_hz) {
  const int q = pcm_ratio(rate_hz);
  return q == 0 ? -1 : q == 1 ? 1 : 2 * kPcmK * q + 1;
}

int nutls_pcm_filter(int rate_hz, float* taps, int n) {
  if (!taps) return fail(NUTLS_ERR_ARG, "nutls_pcm_filter: null pointer");
  const int want = nutls_pcm_filter_taps(rate_hz);
  if (want < 0) return fail(NUTLS_ERR_ARG, "nutls_pcm_filter: rate must be 8000, 16000, 32000 or 48000");
  if (n != want) return fail(NUTLS_ERR_ARG, "nutls_pcm_filter: the filter of " + std::to_string(rate_hz) + " Hz has " + std::to_string(want) + " taps (nutls_pcm_filter_taps)");
  const std::vector<float> p = pcm_design(rate_hz);
  for (int i = 0; i < n; ++i) taps[i] = p[i];
  return NUTLS_OK;
}

// G.711, host only: the library's statement of the rule (no handle, no device)
int nutls_pcm_g711_expand(int sample_format, short* table, int n) {
  if (!g711_format(sample_format)) return fail(NUTLS_ERR_ARG, "nutls_pcm_g711_expand: sample format must be NUTLS_PCM_ULAW or NUTLS_PCM_ALAW");
  if (!table) return fail(NUTLS_ERR_ARG, "nutls_pcm_g711_expand: null pointer");
  if (n != 256) return fail(NUTLS_ERR_ARG, "nutls_pcm_g711_expand: the table has 256 entries, one per code: n must be 256");
  for (int c = 0; c < 256; ++c) table[c] = static_cast<short>(g711_expand(sample_format, c));
  return NUTLS_OK;
}

int nutls_pcm_g711_compress(int sample_format, const short* in, unsigned char* out, size_t n) {
  if (!g711_format(sample_format)) return fail(NUTLS_ERR_ARG, "nutls_pcm_g711_compress: sample format must be NUTLS_PCM_ULAW or NUTLS_PCM_ALAW");
  if (!in || !out) return fail(NUTLS_ERR_ARG, "nutls_pcm_g711_compress: null pointer");
  for (size_t i = 0; i < n; ++i) out[i] = g711_compress(sample_format, in[i]);
  return NUTLS_OK;
}

int nutls_set_pcm_format(nutls_handle* h, int rate_hz, int sample_format) {
  if (!h) return fail(NUTLS_ERR_ARG, "nutls_set_pcm_format: null handle");
  if (!pcm_ratio(rate_hz)) return fail(NUTLS_ERR_ARG, "nutls_set_pcm_format: rate must be 8000, 16000, 32000 or 48000");
  if (sample_format != NUTLS_PCM_F32 && sample_format != NUTLS_PCM_S16 && !g711_format(sample_format))
    return fail(NUTLS_ERR_ARG, "nutls_set_pcm_format: sample format must be NUTLS_PCM_F32, NUTLS_PCM_S16, NUTLS_PCM_ULAW or NUTLS_PCM_ALAW");
  if (g711_format(sample_format) && rate_hz != 8000)      // (an explicit request never silently becomes another format)
    return fail(NUTLS_ERR_ARG, "nutls_set_pcm_format: NUTLS_PCM_ULAW and NUTLS_PCM_ALAW are G.711, which is 8 kHz: rate must be 8000 with them, not " +
                                   std::to_string(rate_hz));
  Engine* e = &h->eng;
  const bool to_plain = rate_hz == 16000 && sample_format == NUTLS_PCM_F32;
  if (!e->pcm.ready && to_plain) {      // nothing has been converted yet and nothing will be
    e->pcm.rate = rate_hz;
    e->pcm.fmt = sample_format;
    e->pcm.upper = 0.f;
    e->pcm.follow = false;
    e->pkt.P = 0;      // (packet mode is off again: below)
    return NUTLS_OK;
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());      // queued conversions still read the taps and histories that change below
  e->pcm.rate = rate_hz;
  e->pcm.fmt = sample_format;
  e->pcm.upper = 0.f;                   // a new format starts anew: the upper band is off until nutls_set_pcm_upper_band
  e->pcm.follow = false;                // ... and with it follow
  e->pkt.P = 0;                         // ... and packet mode: S changes with the rate (nutls_set_pcm_packet after the format)
  if (!e->pcm.ready) {
    if (int rc = pcm_init(e)) return rc;      // (uploads the taps, zeroes the histories)
  } else {
    if (int rc = upload_taps(e)) return rc;
    if (int rc = zero_histories(e, -1)) return rc;      // a format switch starts a new history for every stream
  }
  HIP_TRY(hipDeviceSynchronize());
  return NUTLS_OK;
}

int nutls_set_pcm_upper_band(nutls_handle* h, float gain) {
  if (!h) return fail(NUTLS_ERR_ARG, "nutls_set_pcm_upper_band: null handle");
  if (!(gain >= 0.f && gain <= 1.f)) return fail(NUTLS_ERR_ARG, "nutls_set_pcm_upper_band: gain must lie in 0 .. 1");      // (NaN fails both)
  Engine* e = &h->eng;
  if (gain == e->pcm.upper) return NUTLS_OK;      // nothing is touched
  if (gain != 0.f && e->pcm.rate <= 16000)
    return fail(NUTLS_ERR_ARG, "nutls_set_pcm_upper_band: the handle's rate is " + std::to_string(e->pcm.rate) +
                                   " Hz: there is no band above 8 kHz (nutls_set_pcm_format with 32000 or 48000 first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());      // queued conversions still read the histories and the upper-band state that change below
  if (int rc = pcm_init(e)) return rc;
  if (gain != 0.f)
    if (int rc = upper_init(e)) return rc;
  if (int rc = zero_histories(e, -1)) return rc;      // like a format switch: every stream starts anew, resamplers and upper band
  e->pcm.upper = gain == 0.f ? 0.f : gain;
  if (gain == 0.f) e->pcm.follow = false;      // nothing is left to follow with; another gain other than 0 keeps it
  HIP_TRY(hipDeviceSynchronize());
  return NUTLS_OK;
}

int nutls_pcm_upper_band(nutls_handle* h, float* gain) {
  if (!h || !gain) return fail(NUTLS_ERR_ARG, "nutls_pcm_upper_band: null pointer");
  *gain = h->eng.pcm.upper;
  return NUTLS_OK;
}

int nutls_set_pcm_upper_follow(nutls_handle* h, int enable) {
  if (!h) return fail(NUTLS_ERR_ARG, "nutls_set_pcm_upper_follow: null handle");
  Engine* e = &h->eng;
  const bool on = enable != 0;
  if (on == e->pcm.follow) return NUTLS_OK;      // nothing is touched
  if (on && e->pcm.upper == 0.f)
    return fail(NUTLS_ERR_ARG, "nutls_set_pcm_upper_follow: the upper band's gain is 0 (rate " + std::to_string(e->pcm.rate) +
                                   " Hz): there is no ceiling to follow under (nutls_set_pcm_upper_band with a gain other than 0 first, at 32000 or 48000 Hz)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());      // queued conversions still read the state that changes below
  if (on)
    if (int rc = follow_init(e)) return rc;      // (a gain other than 0 is in force: pcm_init and upper_init have run)
  if (int rc = zero_histories(e, -1)) return rc;      // like a gain change: every stream starts anew
  e->pcm.follow = on;
  HIP_TRY(hipDeviceSynchronize());
  return NUTLS_OK;
}

int nutls_pcm_upper_follow(nutls_handle* h, int* enable) {
  if (!h || !enable) return fail(NUTLS_ERR_ARG, "nutls_pcm_upper_follow: null pointer");
  *enable = h->eng.pcm.follow ? 1 : 0;
  return NUTLS_OK;
}

int nutls_pcm_follow_gain(nutls_handle* h, float* gains, int n) {
  if (!h || !gains) return fail(NUTLS_ERR_ARG, "nutls_pcm_follow_gain: null pointer");
  Engine* e = &h->eng;
  if (!e->pcm.follow) return fail(NUTLS_ERR_ARG, "nutls_pcm_follow_gain: follow is off (nutls_set_pcm_upper_follow)");
  if (n != e->pcm.rows) return fail(NUTLS_ERR_ARG, "nutls_pcm_follow_gain: n must be the handle's rows, " + std::to_string(e->pcm.rows));
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());      // the encode launches queued on the callers' streams have written what is read here
  HIP_TRY(hipMemcpy2D(gains, sizeof(float), e->pcm.enc.fo[e->pcm.enc.par] + kPcmFollowGainAt, kPcmFollowCarry * sizeof(float), sizeof(float),
                      static_cast<size_t>(n), hipMemcpyDeviceToHost));
  return NUTLS_OK;
}

int nutls_pcm_hop_samples(nutls_handle* h) { return h ? hop_samples(&h->eng) : fail(NUTLS_ERR_ARG, "nutls_pcm_hop_samples: null handle"); }

int nutls_pcm_delay_samples(nutls_handle* h) {
  if (!h) return fail(NUTLS_ERR_ARG, "nutls_pcm_delay_samples: null handle");
  const int rate = h->eng.pcm.rate;
  return rate == 16000 ? 0 : 2 * kPcmK * (rate > 16000 ? rate / 16000 : 1);
}

// ---- streaming handles ----------------------------------------------------------------------------------------------------------------------
int nutls_enhance_hop_pcm(nutls_handle* h, const void* pcm_in, void* pcm_out, int dc_mode, void* stream) {
  if (int rc = hop_args(h, pcm_in && pcm_out, "nutls_enhance_hop_pcm")) return rc;
  if (plain_entry(&h->eng)) return nutls_enhance_hop(h, static_cast<const float*>(pcm_in), static_cast<float*>(pcm_out), dc_mode, stream);
  if (int rc = hop_refusals(h, nullptr, dc_mode, "nutls_enhance_hop_pcm")) return rc;
  return hop_device(h, pcm_in, pcm_out, nullptr, dc_mode, stream);
}

int nutls_enhance_hop_pcm_active(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode, void* stream) {
  if (int rc = hop_args(h, pcm_in && pcm_out, "nutls_enhance_hop_pcm_active")) return rc;
  if (!active) return nutls_enhance_hop_pcm(h, pcm_in, pcm_out, dc_mode, stream);
  if (plain_entry(&h->eng)) return nutls_enhance_hop_active(h, static_cast<const float*>(pcm_in), static_cast<float*>(pcm_out), active, dc_mode, stream);
  if (int rc = hop_refusals(h, active, dc_mode, "nutls_enhance_hop_pcm_active")) return rc;
  return hop_device(h, pcm_in, pcm_out, active, dc_mode, stream);
}

int nutls_enhance_hop_pcm_host(nutls_handle* h, const void* pcm_in, void* pcm_out, int dc_mode) {
  if (int rc = hop_args(h, pcm_in && pcm_out, "nutls_enhance_hop_pcm_host")) return rc;
  if (plain_entry(&h->eng)) return nutls_enhance_hop_host(h, static_cast<const float*>(pcm_in), static_cast<float*>(pcm_out), dc_mode);
  if (int rc = hop_refusals(h, nullptr, dc_mode, "nutls_enhance_hop_pcm_host")) return rc;
  return hop_host(h, pcm_in, pcm_out, nullptr, dc_mode);
}

int nutls_enhance_hop_pcm_host_active(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode) {
  if (int rc = hop_args(h, pcm_in && pcm_out, "nutls_enhance_hop_pcm_host_active")) return rc;
  if (!active) return nutls_enhance_hop_pcm_host(h, pcm_in, pcm_out, dc_mode);
  if (plain_entry(&h->eng))
    return nutls_enhance_hop_host_active(h, static_cast<const float*>(pcm_in), static_cast<float*>(pcm_out), active, dc_mode);
  if (int rc = hop_refusals(h, active, dc_mode, "nutls_enhance_hop_pcm_host_active")) return rc;
  return hop_host(h, pcm_in, pcm_out, active, dc_mode);
}

// The two halves on their own (at 16000 / float32: copies).  They need no model, so a mask is taken on every streaming handle.
int nutls_pcm_decode_hop(nutls_handle* h, const void* pcm_in, float* hop_out, const unsigned char* active, void* stream) {
  if (int rc = hop_args(h, pcm_in && hop_out, "nutls_pcm_decode_hop")) return rc;
  return half_entry(h, PcmDir::kDecode, pcm_in, hop_out, active, 1, stream);
}

int nutls_pcm_encode_hop(nutls_handle* h, const float* hop_in, void* pcm_out, const unsigned char* active, void* stream) {
  if (int rc = hop_args(h, hop_in && pcm_out, "nutls_pcm_encode_hop")) return rc;
  return half_entry(h, PcmDir::kEncode, hop_in, pcm_out, active, 1, stream);
}

// ---- streaming handles, packet mode: the callers' packets re-framed into hops on the device -----------------------------------------------------
int nutls_pcm_packet_plan(int rate_hz, int sample_format, int samples, int* delay, int* rounds, int* fifo) {
  PacketPlan p;
  if (int rc = packet_plan(rate_hz, sample_format, samples, &p, "nutls_pcm_packet_plan")) return rc;
  if (delay) *delay = p.D;
  if (rounds) *rounds = p.R;
  if (fifo) *fifo = p.L;
  return NUTLS_OK;
}

int nutls_set_pcm_packet(nutls_handle* h, int samples) {
  const char* who = "nutls_set_pcm_packet";
  if (!h) return fail(NUTLS_ERR_ARG, std::string(who) + ": null handle");
  Engine* e = &h->eng;
  PacketState& k = e->pkt;
  if (samples == k.P) return NUTLS_OK;      // nothing is touched
  if (e->offline)
    return fail(NUTLS_ERR_ARG, std::string(who) + ": offline handle (nutls_create_offline): packets are a streaming handle's -- nutls_enhance_block_pcm takes any number of hops");
  PacketPlan p = {};
  if (samples != 0) {
    if (int rc = packet_plan(e->pcm.rate, e->pcm.fmt, samples, &p, who)) return rc;
    if (packet_masked(samples, p.S, nullptr))
      if (int rc = check_active(e, who)) return rc;      // (packets that do not cut into whole hops: every tick's rounds are masked hops)
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());      // queued ticks still read the rings and counters that change below
  if (samples == 0) {
    k.P = 0;
    return NUTLS_OK;
  }
  if (!plain_format(e))
    if (int rc = pcm_init(e)) return rc;
  const size_t rows = static_cast<size_t>(e->B);
  int rc;
  if ((rc = grow_pair(e, rows * p.L * p.bytes, &k.in_ring, &k.out_ring, &k.ring_cap)) || (rc = grow_pair(e, rows * p.S * p.bytes, &k.hop_in, &k.hop_out, &k.hop_cap)) ||
      (rc = dev_alloc_once(e, rows, &k.ctr, true)) || (rc = dev_alloc_once(e, rows, &k.ready, true)))
    return rc;
  k.P = samples;
  k.S = p.S;
  k.D = p.D;
  k.R = p.R;
  k.L = p.L;
  k.bytes = p.bytes;
  k.silence = e->pcm.fmt == NUTLS_PCM_ULAW ? 0xFFFFFFFFu : e->pcm.fmt == NUTLS_PCM_ALAW ? 0xD5D5D5D5u : 0u;
  k.last_rounds = 0;
  if ((rc = packet_prime(e, -1))) return rc;      // every stream: input empty, output D samples of silence; the mirror is known again
  HIP_TRY(hipDeviceSynchronize());
  return NUTLS_OK;
}

int nutls_pcm_packet_samples(nutls_handle* h) { return h ? h->eng.pkt.P : fail(NUTLS_ERR_ARG, "nutls_pcm_packet_samples: null handle"); }

int nutls_pcm_packet_delay_samples(nutls_handle* h) {
  if (!h) return fail(NUTLS_ERR_ARG, "nutls_pcm_packet_delay_samples: null handle");
  return h->eng.pkt.P ? h->eng.pkt.D : 0;
}

int nutls_pcm_packet_last_rounds(nutls_handle* h) {
  if (!h) return fail(NUTLS_ERR_ARG, "nutls_pcm_packet_last_rounds: null handle");
  return h->eng.pkt.P ? h->eng.pkt.last_rounds : 0;
}

int nutls_pcm_packet_fill(nutls_handle* h, int* fill, int n) {
  if (!h || !fill) return fail(NUTLS_ERR_ARG, "nutls_pcm_packet_fill: null pointer");
  Engine* e = &h->eng;
  const PacketState& k = e->pkt;
  if (!k.P) return fail(NUTLS_ERR_ARG, "nutls_pcm_packet_fill: packet mode is off (nutls_set_pcm_packet)");
  if (n != e->B) return fail(NUTLS_ERR_ARG, "nutls_pcm_packet_fill: n must be the handle's streams, " + std::to_string(e->B));
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());      // the ticks queued on the callers' streams have written what is read here
  HIP_TRY(hipMemcpy2D(fill, sizeof(int), &k.ctr[0].fill, sizeof(PacketCtr), sizeof(int), static_cast<size_t>(n), hipMemcpyDeviceToHost));
  for (int b = 0; b < n; ++b) fill[b] *= 16 / k.bytes;      // quads -> samples
  return NUTLS_OK;
}

int nutls_enhance_packet_pcm(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode, void* stream) {
  if (int rc = packet_refusals(h, pcm_in && pcm_out, active, dc_mode, "nutls_enhance_packet_pcm")) return rc;
  HIP_TRY(hipSetDevice(h->eng.device));
  return packet_device(h, pcm_in, pcm_out, active, nullptr, dc_mode, static_cast<hipStream_t>(stream));
}

// the tick through the staging (active: HOST mask or null): the host sees the mask, so the mirror of the counters stays known
int nutls_enhance_packet_pcm_host(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode) {
  if (int rc = packet_refusals(h, pcm_in && pcm_out, active, dc_mode, "nutls_enhance_packet_pcm_host")) return rc;
  Engine* e = &h->eng;
  PacketState& k = e->pkt;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = grow_pair(e, static_cast<size_t>(e->B) * k.P * k.bytes, &k.raw_in, &k.raw_out, &k.raw_cap)) return rc;
  if (int rc = enqueue_on(e, e->stream)) return rc;      // (behind what earlier calls queued on the callers' streams)
  const unsigned char* d_act = nullptr;
  if (active) {
    if (int rc = dev_alloc_once(e, static_cast<size_t>(e->B), &e->pcm.d_active, false)) return rc;
    HIP_TRY(hipMemcpyAsync(e->pcm.d_active, active, static_cast<size_t>(e->B), hipMemcpyHostToDevice, e->stream));
    d_act = e->pcm.d_active;
  }
  return through_staging(e, k.raw_in, k.raw_out, pcm_in, pcm_out, static_cast<size_t>(e->B) * k.P,
                         [&](const void* in, void* out) { return packet_device(h, in, out, d_act, active, dc_mode, e->stream); });
}

// ---- channels: the callers' frame layout (streaming and offline handles) ------------------------------------------------------------------------
int nutls_set_pcm_channels(nutls_handle* h, int channels) {
  const char* who = "nutls_set_pcm_channels";
  if (!h) return fail(NUTLS_ERR_ARG, std::string(who) + ": null handle");
  Engine* e = &h->eng;
  if (channels != 1 && channels != 2 && channels != 4)
    return fail(NUTLS_ERR_ARG, std::string(who) + ": channels must be 1 (off), 2 or 4, not " + std::to_string(channels));
  if (handle_rows(e) % channels)
    return fail(NUTLS_ERR_ARG, std::string(who) + ": the handle has " + std::to_string(handle_rows(e)) + (e->offline ? " utterances" : " streams") +
                                   ", which is no multiple of " + std::to_string(channels) + " channels: every frame row holds one stream per channel");
  if (channels == e->chn.C) return NUTLS_OK;      // nothing is touched
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());      // a setting like the attenuation limit: it holds from the next call, behind everything queued so far
  e->chn.C = channels;
  return NUTLS_OK;
}

int nutls_pcm_channels(nutls_handle* h) { return h ? h->eng.chn.C : fail(NUTLS_ERR_ARG, "nutls_pcm_channels: null handle"); }

// host only: the library's statement of the rule (no handle, no device)
int nutls_pcm_deinterleave(int sample_format, int channels, const void* frames, void* rows, size_t n) {
  return channels_host("nutls_pcm_deinterleave", sample_format, channels, frames, rows, n, false);
}

int nutls_pcm_interleave(int sample_format, int channels, const void* rows, void* frames, size_t n) {
  return channels_host("nutls_pcm_interleave", sample_format, channels, rows, frames, n, true);
}

// ---- offline handles --------------------------------------------------------------------------------------------------------------------------
int nutls_enhance_block_pcm(nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, int dc_mode, void* stream) {
  if (int rc = block_args(h, pcm_in && pcm_out, n_hops, "nutls_enhance_block_pcm")) return rc;
  if (plain_entry(&h->eng)) return nutls_enhance_block(h, static_cast<const float*>(pcm_in), static_cast<float*>(pcm_out), n_hops, dc_mode, stream);
  if (int rc = dc_ok(dc_mode, "nutls_enhance_block_pcm")) return rc;
  return block_device(h, pcm_in, pcm_out, n_hops, nullptr, dc_mode, stream);
}

int nutls_enhance_block_pcm_host(nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, int dc_mode) {
  if (int rc = block_args(h, pcm_in && pcm_out, n_hops, "nutls_enhance_block_pcm_host")) return rc;
  if (plain_entry(&h->eng)) return nutls_enhance_block_host(h, static_cast<const float*>(pcm_in), static_cast<float*>(pcm_out), n_hops, dc_mode);
  if (int rc = dc_ok(dc_mode, "nutls_enhance_block_pcm_host")) return rc;
  Engine* e = &h->eng;
  if (int rc = pcm_ready(e)) return rc;
  if (int rc = raw_init(e)) return rc;
  if (int rc = enqueue_on(e, e->stream)) return rc;      // (behind what earlier calls queued on the callers' streams)
  return block_host(h, pcm_in, pcm_out, n_hops, nullptr, dc_mode);
}

int nutls_pcm_decode_block(nutls_handle* h, const void* pcm_in, float* wave_out, int n_hops, void* stream) {
  if (int rc = block_args(h, pcm_in && wave_out, n_hops, "nutls_pcm_decode_block")) return rc;
  return half_entry(h, PcmDir::kDecode, pcm_in, wave_out, nullptr, n_hops, stream);
}

int nutls_pcm_encode_block(nutls_handle* h, const float* wave_in, void* pcm_out, int n_hops, void* stream) {
  if (int rc = block_args(h, wave_in && pcm_out, n_hops, "nutls_pcm_encode_block")) return rc;
  return half_entry(h, PcmDir::kEncode, wave_in, pcm_out, nullptr, n_hops, stream);
}

// ---- offline handles, ragged: per-utterance hop counts in the callers' format ------------------------------------------------------------------
int nutls_enhance_block_pcm_ragged(nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream) {
  const char* who = "nutls_enhance_block_pcm_ragged";
  if (!h) return fail(NUTLS_ERR_ARG, std::string(who) + ": null pointer");
  if (plain_entry(&h->eng))
    return nutls_enhance_block_ragged(h, static_cast<const float*>(pcm_in), static_cast<float*>(pcm_out), n_hops, hops, dc_mode, stream);
  if (!hops) return nutls_enhance_block_pcm(h, pcm_in, pcm_out, n_hops, dc_mode, stream);
  if (int rc = block_args(h, pcm_in && pcm_out, n_hops, who)) return rc;
  if (int rc = dc_ok(dc_mode, who)) return rc;
  if (int rc = aligned16(pcm_in, pcm_out, who)) return rc;
  return block_device(h, pcm_in, pcm_out, n_hops, hops, dc_mode, stream);
}

// hops: HOST.  Every refusal, the counts' included, comes before the first conversion: a refused call leaves the histories where they were.
int nutls_enhance_block_pcm_ragged_host(nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, const int* hops, int dc_mode) {
  const char* who = "nutls_enhance_block_pcm_ragged_host";
  if (!h) return fail(NUTLS_ERR_ARG, std::string(who) + ": null pointer");
  if (plain_entry(&h->eng))
    return nutls_enhance_block_ragged_host(h, static_cast<const float*>(pcm_in), static_cast<float*>(pcm_out), n_hops, hops, dc_mode);
  if (!hops) return nutls_enhance_block_pcm_host(h, pcm_in, pcm_out, n_hops, dc_mode);
  if (int rc = block_args(h, pcm_in && pcm_out, n_hops, who)) return rc;
  if (int rc = dc_ok(dc_mode, who)) return rc;
  Engine* e = &h->eng;
  if (int rc = upload_counts(e, hops, n_hops, who)) return rc;      // (sets the device, puts the library's stream behind the earlier calls)
  if (int rc = pcm_init(e)) return rc;
  if (int rc = raw_init(e)) return rc;
  return block_host(h, pcm_in, pcm_out, n_hops, e->d_counts, dc_mode);
}

int nutls_pcm_decode_block_ragged(nutls_handle* h, const void* pcm_in, float* wave_out, int n_hops, const int* hops, void* stream) {
  if (!hops) return nutls_pcm_decode_block(h, pcm_in, wave_out, n_hops, stream);
  if (int rc = block_args(h, pcm_in && wave_out, n_hops, "nutls_pcm_decode_block_ragged")) return rc;
  if (int rc = aligned16(pcm_in, wave_out, "nutls_pcm_decode_block_ragged")) return rc;
  return half_entry(h, PcmDir::kDecode, pcm_in, wave_out, nullptr, n_hops, stream, hops);
}

int nutls_pcm_encode_block_ragged(nutls_handle* h, const float* wave_in, void* pcm_out, int n_hops, const int* hops, void* stream) {
  if (!hops) return nutls_pcm_encode_block(h, wave_in, pcm_out, n_hops, stream);
  if (int rc = block_args(h, wave_in && pcm_out, n_hops, "nutls_pcm_encode_block_ragged")) return rc;
  if (int rc = aligned16(wave_in, pcm_out, "nutls_pcm_encode_block_ragged")) return rc;
  return half_entry(h, PcmDir::kEncode, wave_in, pcm_out, nullptr, n_hops, stream, hops);
}

}  // extern "C"
