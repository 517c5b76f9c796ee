// Streaming entry points of the C ABI (include/nutls.h): the frame step and the hop (STFT analysis, step, inverse STFT; three launches or the
// single launch of nutls_set_hop_fusion), each from device or host buffers and with or without a per-stream active mask, and the page-locked
// host buffers the _host entries recognise.  The engine they drive: engine.cpp.
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "engine.hpp"

using namespace nutls;

// After a masked step whose mask the host has seen (the _host entries; the rounds of a packet call, api_pcm.cpp): the streams that took the
// frame have replaced every row nutls_state_set gave them; once all have, masked launches go back to leaving the lazily written states to
// states_materialize.  (A device mask is not visible here: with those, eager launches last until a step of all streams -- nutls.h,
// nutls_step_active.)
void nutls::note_active(Engine* e, const unsigned char* active) {
  if (!e->lazy_edited) return;
  bool pending = false;
  for (int b = 0; b < e->B; ++b) {
    if (active[b]) e->lazy_pending[b] = 0;
    pending = pending || e->lazy_pending[b];
  }
  if (!pending) e->lazy_edited = false;
}

extern "C" {

// ---- page-locked host buffers (nutls_host_alloc): base -> bytes ---------------------------------------------------------
static std::mutex g_pin_mu;
static std::map<const char*, size_t> g_pins;

void* nutls_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess || !p) {
    (void)hipGetLastError();
    fail(NUTLS_ERR_HIP, "nutls_host_alloc: hipHostMalloc of " + std::to_string(bytes) + " bytes failed");
    return nullptr;
  }
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_pins[static_cast<const char*>(p)] = bytes;
  return p;
}

void nutls_host_free(void* p) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    if (!g_pins.erase(static_cast<const char*>(p))) return;      // not ours (or freed twice): leave it alone
  }
  (void)hipHostFree(p);
}

static bool host_pinned(const void* p, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_pin_mu);
  auto it = g_pins.upper_bound(static_cast<const char*>(p));
  if (it == g_pins.begin()) return false;
  --it;
  return static_cast<const char*>(p) + bytes <= it->first + it->second;
}

// A buffer that starts inside one of our page-locked allocations and runs past its end.  The runtime finds the allocation behind such a
// pointer and refuses a copy command whose range leaves it (hipErrorInvalidValue), so the staged copies of the _host entries take it
// through a pageable buffer of their own: HostStage.
static bool host_straddles(const void* p, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_pin_mu);
  auto it = g_pins.upper_bound(static_cast<const char*>(p));
  if (it == g_pins.begin()) return false;
  --it;
  const char* end = it->first + it->second;
  return static_cast<const char*>(p) < end && static_cast<const char*>(p) + bytes > end;
}

// The host side of a _host entry's two staged copies: the caller's buffers, or pageable stand-ins for those that straddle (lives until the
// entry has synchronised; `finish` then hands the result over).
struct HostStage {
  const float* in;
  float* out;
  float* caller_out;
  size_t bytes;
  std::vector<float> tmp_in, tmp_out;
  HostStage(const float* host_in, float* host_out, size_t n_bytes) : in(host_in), out(host_out), caller_out(host_out), bytes(n_bytes) {
    if (host_straddles(host_in, bytes)) {
      tmp_in.assign(host_in, host_in + bytes / sizeof(float));
      in = tmp_in.data();
    }
    if (host_straddles(host_out, bytes)) {
      tmp_out.resize(bytes / sizeof(float));
      out = tmp_out.data();
    }
  }
  void finish() const {
    if (out != caller_out) std::memcpy(caller_out, out, bytes);
  }
};

// The B mask bytes of a _host entry, copied to the handle's device buffer on the library's stream (in front of the work that reads them).
static int upload_active(Engine* e, const unsigned char* active) {
  if (int rc = dev_alloc_once(e, static_cast<size_t>(e->B), &e->d_active, false)) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_active, active, static_cast<size_t>(e->B), hipMemcpyHostToDevice, e->stream));
  return NUTLS_OK;
}

// (active non-null: checked by the caller, fused mode)
static int step_impl(nutls_handle* h, const float* mag_in, float* mag_out, const unsigned char* active, void* stream) {
  Engine* e = &h->eng;
  if (e->offline) return fail(NUTLS_ERR_ARG, "nutls_step: offline handle, use nutls_process_block");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = enqueue_on(e, s)) return rc;
  const size_t bytes = static_cast<size_t>(e->B) * NUTLS_BINS * sizeof(float);
  const bool direct = e->mode == 3;      // the fused kernel takes the caller's buffers as they are
  if (!direct && mag_in != e->io_in) HIP_TRY(hipMemcpyAsync(e->io_in, mag_in, bytes, hipMemcpyDeviceToDevice, s));
  const int par = e->next_parity;
  if (e->mode == 3) {
    int rc = run_fused(e, par, s, e->fz_dbg != nullptr, mag_in, mag_out, active);
    if (rc) return rc;
  } else {
    int rc = begin_per_layer_step(e, s);
    if (rc) return rc;
    if (e->mode == 1) HIP_TRY(hipGraphLaunch(e->gexec[par], s));
    else if ((rc = run_plan(e, par, s))) return rc;
  }
  if (!direct && mag_out != e->io_out) HIP_TRY(hipMemcpyAsync(mag_out, e->io_out, bytes, hipMemcpyDeviceToDevice, s));
  advance_frame(e);
  return NUTLS_OK;
}

int nutls_step(nutls_handle* h, const float* mag_in, float* mag_out, void* stream) {
  if (!h || !mag_in || !mag_out) return fail(NUTLS_ERR_ARG, "nutls_step: null pointer");
  return step_impl(h, mag_in, mag_out, nullptr, stream);
}

int nutls_step_active(nutls_handle* h, const float* mag_in, float* mag_out, const unsigned char* active, void* stream) {
  if (!active) return nutls_step(h, mag_in, mag_out, stream);
  if (!h || !mag_in || !mag_out) return fail(NUTLS_ERR_ARG, "nutls_step_active: null pointer");
  if (int rc = check_active(&h->eng, "nutls_step_active")) return rc;
  return step_impl(h, mag_in, mag_out, active, stream);
}

// (active: HOST mask or null; checked by the caller)
static int step_host_impl(nutls_handle* h, const float* mag_in, float* mag_out, const unsigned char* active) {
  Engine* e = &h->eng;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = enqueue_on(e, e->stream)) return rc;      // (behind what earlier calls queued on the callers' streams)
  const size_t bytes = static_cast<size_t>(e->B) * NUTLS_BINS * sizeof(float);
  const unsigned char* d_act = nullptr;
  if (active) {
    if (int rc = upload_active(e, active)) return rc;
    d_act = e->d_active;
  }
  if (e->mode == 3 && host_pinned(mag_in, bytes) && host_pinned(mag_out, bytes)) {
    // the fused kernel takes the caller's buffers as they are: the frame crosses the link inside the launch, no copy commands
    // (B = 1024: 0.976 ms per call against 1.048 through two DMA copies of the same pinned buffers and 1.10-1.11 from pageable memory)
    int rc = step_impl(h, mag_in, mag_out, d_act, e->stream);
    if (rc) return rc;
    if (active) note_active(e, active);
    HIP_TRY(hipStreamSynchronize(e->stream));
    enqueue_idle(e);
    return NUTLS_OK;
  }
  HostStage hs(mag_in, mag_out, bytes);
  HIP_TRY(hipMemcpyAsync(e->io_in, hs.in, bytes, hipMemcpyHostToDevice, e->stream));
  int rc = step_impl(h, e->io_in, e->io_out, d_act, e->stream);
  if (rc) return rc;
  if (active) note_active(e, active);
  HIP_TRY(hipMemcpyAsync(hs.out, e->io_out, bytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  enqueue_idle(e);
  hs.finish();
  return NUTLS_OK;
}

int nutls_step_host(nutls_handle* h, const float* mag_in, float* mag_out) {
  if (!h || !mag_in || !mag_out) return fail(NUTLS_ERR_ARG, "nutls_step_host: null pointer");
  return step_host_impl(h, mag_in, mag_out, nullptr);
}

int nutls_step_host_active(nutls_handle* h, const float* mag_in, float* mag_out, const unsigned char* active) {
  if (!active) return nutls_step_host(h, mag_in, mag_out);
  if (!h || !mag_in || !mag_out) return fail(NUTLS_ERR_ARG, "nutls_step_host_active: null pointer");
  if (int rc = check_active(&h->eng, "nutls_step_host_active")) return rc;
  return step_host_impl(h, mag_in, mag_out, active);
}

// (active: device mask or null -- a held stream's previous hop, magnitudes and phasors stay as they are)
static int stft_hop_impl(nutls_handle* h, const float* pcm_in, const unsigned char* active, void* stream) {
  Engine* e = &h->eng;
  HIP_TRY(hipSetDevice(e->device));
  int rc = frontend_init(e);
  if (rc) return rc;
  if ((rc = enqueue_on(e, static_cast<hipStream_t>(stream)))) return rc;
  HIP_TRY(launch_stft_hop(pcm_in, e->fe_tail, e->fe_win, e->fe_tw, e->io_in, e->fe_ph, e->B, static_cast<hipStream_t>(stream), active));
  return NUTLS_OK;
}

int nutls_stft_hop(nutls_handle* h, const float* pcm_in, void* stream) {
  if (!h || !pcm_in) return fail(NUTLS_ERR_ARG, "nutls_stft_hop: null pointer");
  return stft_hop_impl(h, pcm_in, nullptr, stream);
}

// (active: device mask or null -- a held stream gets a zero hop, its overlap tail stays as it is)
static int istft_hop_impl(nutls_handle* h, float* pcm_out, int dc_mode, const unsigned char* active, void* stream) {
  if (dc_mode != NUTLS_DC_EDGE && dc_mode != NUTLS_DC_ZERO) return fail(NUTLS_ERR_ARG, "dc_mode must be NUTLS_DC_EDGE or NUTLS_DC_ZERO");
  Engine* e = &h->eng;
  HIP_TRY(hipSetDevice(e->device));
  int rc = frontend_init(e);
  if (rc) return rc;
  if ((rc = enqueue_on(e, static_cast<hipStream_t>(stream)))) return rc;
  // an attenuation limit in force (nutls_set_atten_limit): the mix for the whole launch, the noisy rows being io_in as the analysis left them
  // (an offline handle's limits are per utterance, not per arena slot: they belong to its block entries)
  const float* noisy = e->atten_on && !e->offline ? e->io_in : nullptr;
  HIP_TRY(launch_istft_hop(e->io_out, noisy, e->d_atten, e->fe_ph, e->fe_inv, e->fe_tw, e->fe_ola, pcm_out, dc_mode == NUTLS_DC_EDGE ? 1 : 0, e->B,
                           static_cast<hipStream_t>(stream), active));
  return NUTLS_OK;
}

int nutls_istft_hop(nutls_handle* h, float* pcm_out, int dc_mode, void* stream) {
  if (!h || !pcm_out) return fail(NUTLS_ERR_ARG, "nutls_istft_hop: null pointer");
  return istft_hop_impl(h, pcm_out, dc_mode, nullptr, stream);
}

// ---- single-launch hop (nutls_set_hop_fusion) -------------------------------------------------------------------------------------------
int nutls_set_hop_fusion(nutls_handle* h, int enable) {
  if (!h) return fail(NUTLS_ERR_ARG, "nutls_set_hop_fusion: null handle");
  Engine* e = &h->eng;
  if (!enable) { e->hop_fusion = false; return NUTLS_OK; }
  if (int rc = check_hop_fusion(e, "nutls_set_hop_fusion")) return rc;
  if (e->atten_on)
    return fail(NUTLS_ERR_ARG, "nutls_set_hop_fusion: not while an attenuation limit is in force (the single-launch hop has no mix) -- nutls_set_atten_limit(h, NULL, n) first");
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = frontend_init(e)) return rc;
  HIP_TRY(e->fz_plan->set_attributes_hop());
  e->hop_fusion = true;
  return NUTLS_OK;
}

int nutls_launches_per_hop(nutls_handle* h) { return h ? (h->eng.hop_fusion ? 1 : 3) : fail(NUTLS_ERR_ARG, "null handle"); }

// analysis, model step and synthesis in ONE launch of the plan's hop build: magnitudes and estimates still go through the library's io rows, the
// previous hops / overlap tails / phasors through the buffers of the three-launch path -- fusion may change between any two hops of a stream
static int enhance_hop_fused(nutls_handle* h, const float* pcm_in, float* pcm_out, const unsigned char* active, int dc_mode, void* stream) {
  if (dc_mode != NUTLS_DC_EDGE && dc_mode != NUTLS_DC_ZERO) return fail(NUTLS_ERR_ARG, "dc_mode must be NUTLS_DC_EDGE or NUTLS_DC_ZERO");
  Engine* e = &h->eng;
  if (int rc = check_hop_fusion(e, "nutls_enhance_hop")) return rc;      // (cannot fail: everything that would is refused while fusion is on)
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = enqueue_on(e, static_cast<hipStream_t>(stream))) return rc;
  const FzHop hop{pcm_in, pcm_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dc_mode == NUTLS_DC_EDGE ? 1 : 0};
  const int par = e->next_parity;
  if (int rc = run_fused(e, par, static_cast<hipStream_t>(stream), false, e->io_in, e->io_out, active, &hop)) return rc;
  advance_frame(e);
  return NUTLS_OK;
}

// analysis -> model step on the library buffers -> synthesis, all three with the (device) mask or without one
static int enhance_hop_impl(nutls_handle* h, const float* pcm_in, float* pcm_out, const unsigned char* active, int dc_mode, void* stream) {
  if (h->eng.hop_fusion) return enhance_hop_fused(h, pcm_in, pcm_out, active, dc_mode, stream);
  int rc = stft_hop_impl(h, pcm_in, active, stream);
  if (rc) return rc;
  Engine* e = &h->eng;
  if ((rc = step_impl(h, e->io_in, e->io_out, active, stream))) return rc;
  return istft_hop_impl(h, pcm_out, dc_mode, active, stream);
}

int nutls_enhance_hop(nutls_handle* h, const float* pcm_in, float* pcm_out, int dc_mode, void* stream) {
  if (!h || !pcm_in || !pcm_out) return fail(NUTLS_ERR_ARG, "nutls_enhance_hop: null pointer");
  return enhance_hop_impl(h, pcm_in, pcm_out, nullptr, dc_mode, stream);
}

// (refusals come before the analysis: a refused call leaves the previous hops where they were)
static int check_enhance_active(nutls_handle* h, int dc_mode, const char* who) {
  if (int rc = check_active(&h->eng, who)) return rc;
  if (dc_mode != NUTLS_DC_EDGE && dc_mode != NUTLS_DC_ZERO) return fail(NUTLS_ERR_ARG, "dc_mode must be NUTLS_DC_EDGE or NUTLS_DC_ZERO");
  return NUTLS_OK;
}

int nutls_enhance_hop_active(nutls_handle* h, const float* pcm_in, float* pcm_out, const unsigned char* active, int dc_mode, void* stream) {
  if (!active) return nutls_enhance_hop(h, pcm_in, pcm_out, dc_mode, stream);
  if (!h || !pcm_in || !pcm_out) return fail(NUTLS_ERR_ARG, "nutls_enhance_hop_active: null pointer");
  if (int rc = check_enhance_active(h, dc_mode, "nutls_enhance_hop_active")) return rc;
  return enhance_hop_impl(h, pcm_in, pcm_out, active, dc_mode, stream);
}

// (active: HOST mask or null; checked by the caller)
static int enhance_hop_host_impl(nutls_handle* h, const float* pcm_in, float* pcm_out, const unsigned char* active, int dc_mode) {
  Engine* e = &h->eng;
  HIP_TRY(hipSetDevice(e->device));
  int rc = frontend_init(e);
  if (rc) return rc;
  if ((rc = enqueue_on(e, e->stream))) return rc;      // (behind what earlier calls queued on the callers' streams)
  const size_t bytes = static_cast<size_t>(e->B) * NUTLS_FRAME_STEP * sizeof(float);
  const unsigned char* d_act = nullptr;
  if (active) {
    if ((rc = upload_active(e, active))) return rc;
    d_act = e->d_active;
  }
  if (e->hop_fusion && host_pinned(pcm_in, bytes) && host_pinned(pcm_out, bytes)) {
    // the hop build takes the caller's page-locked buffers as they are (like step_host_impl): two 1 KB rows per stream cross the link inside
    // the launch, no copy commands
    if ((rc = enhance_hop_impl(h, pcm_in, pcm_out, d_act, dc_mode, e->stream))) return rc;
    if (active) note_active(e, active);
    HIP_TRY(hipStreamSynchronize(e->stream));
    enqueue_idle(e);
    return NUTLS_OK;
  }
  HostStage hs(pcm_in, pcm_out, bytes);
  HIP_TRY(hipMemcpyAsync(e->fe_pcm_in, hs.in, bytes, hipMemcpyHostToDevice, e->stream));
  if ((rc = enhance_hop_impl(h, e->fe_pcm_in, e->fe_pcm_out, d_act, dc_mode, e->stream))) return rc;
  if (active) note_active(e, active);
  HIP_TRY(hipMemcpyAsync(hs.out, e->fe_pcm_out, bytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  enqueue_idle(e);
  hs.finish();
  return NUTLS_OK;
}

int nutls_enhance_hop_host(nutls_handle* h, const float* pcm_in, float* pcm_out, int dc_mode) {
  if (!h || !pcm_in || !pcm_out) return fail(NUTLS_ERR_ARG, "nutls_enhance_hop_host: null pointer");
  return enhance_hop_host_impl(h, pcm_in, pcm_out, nullptr, dc_mode);
}

int nutls_enhance_hop_host_active(nutls_handle* h, const float* pcm_in, float* pcm_out, const unsigned char* active, int dc_mode) {
  if (!active) return nutls_enhance_hop_host(h, pcm_in, pcm_out, dc_mode);
  if (!h || !pcm_in || !pcm_out) return fail(NUTLS_ERR_ARG, "nutls_enhance_hop_host_active: null pointer");
  if (int rc = check_enhance_active(h, dc_mode, "nutls_enhance_hop_host_active")) return rc;
  return enhance_hop_host_impl(h, pcm_in, pcm_out, active, dc_mode);
}

}  // extern "C"
