// State entry points of the C ABI (include/nutls.h): the recurrent state tensors by name or all of one stream, nutls_reset, and the debug
// tensors of nutls_debug_get.  Everything here looks at device memory from the host: it goes through host_access_begin (engine.cpp) first.
#include <algorithm>
#include <cstring>

#include "engine.hpp"

using namespace nutls;

// per-stream tensor (stream-0 pointer `dev`, `per_stream` floats) <-> dense host array [B][per_stream]
static int copy_stream_tensor(Engine* e, float* dev, size_t per_stream, float* host, bool to_host, int stream_idx = -1) {
  const size_t dpitch = e->sstride * sizeof(float), hpitch = per_stream * sizeof(float);
  const int b0 = stream_idx < 0 ? 0 : stream_idx, nb = stream_idx < 0 ? e->B : 1;
  float* d = dev + static_cast<size_t>(b0) * e->sstride;
  if (to_host) HIP_TRY(hipMemcpy2D(host, hpitch, d, dpitch, hpitch, nb, hipMemcpyDeviceToHost));
  else HIP_TRY(hipMemcpy2D(d, dpitch, host, hpitch, hpitch, nb, hipMemcpyHostToDevice));
  return NUTLS_OK;
}

extern "C" {

int nutls_state_count(nutls_handle* h) { return h ? static_cast<int>(h->eng.states.size()) : fail(NUTLS_ERR_ARG, "null handle"); }

int nutls_state_info(nutls_handle* h, int index, const char** name, int* dim0, int* dim1) {
  if (!h || index < 0 || index >= static_cast<int>(h->eng.states.size())) return fail(NUTLS_ERR_ARG, "nutls_state_info: bad index");
  const StateTensor& st = h->eng.states[index];
  if (name) *name = st.name_prev.c_str();
  if (dim0) *dim0 = st.d0;
  if (dim1) *dim1 = st.d1;
  return NUTLS_OK;
}

// Ring states: the device keeps frame j of the reference's [d, F, C] history (0 = oldest) in physical
// slot (steps + j) mod d.  to_logical: physical -> reference order (get); else reference -> physical (set).
static void rotate_ring(Engine* e, const StateTensor& st, float* host, bool to_logical) {
  const int d = st.ring_d;
  const size_t frame = st.per_stream() / d;
  std::vector<float> tmp(st.per_stream());
  for (int b = 0; b < e->B; ++b) {
    float* base = host + static_cast<size_t>(b) * st.per_stream();
    for (int j = 0; j < d; ++j) {
      const int slot = static_cast<int>((e->steps + j) % d);
      const float* src = base + static_cast<size_t>(to_logical ? slot : j) * frame;
      float* dst = tmp.data() + static_cast<size_t>(to_logical ? j : slot) * frame;
      std::memcpy(dst, src, frame * sizeof(float));
    }
    std::memcpy(base, tmp.data(), st.per_stream() * sizeof(float));
  }
}

static int state_lookup(Engine* e, const char* name, size_t n_floats, StateTensor** out) {
  if (!name) return fail(NUTLS_ERR_ARG, "state name is null");
  auto it = e->state_index.find(name);
  if (it == e->state_index.end()) return fail(NUTLS_ERR_ARG, std::string("unknown state tensor: ") + name);
  StateTensor* st = &e->states[it->second];
  const size_t nb = e->offline ? static_cast<size_t>(e->outt) : static_cast<size_t>(e->B);      // an offline handle: its utterances (carried state of utterance u in arena slot u (offline + 1))
  if (n_floats != st->per_stream() * nb)
    return fail(NUTLS_ERR_ARG, std::string("size mismatch for ") + name + ": expected " + std::to_string(st->per_stream() * nb) +
                                   " floats, got " + std::to_string(n_floats));
  *out = st;
  return NUTLS_OK;
}

int nutls_state_get(nutls_handle* h, const char* name, float* host_buf, size_t n_floats) {
  if (!h || !host_buf) return fail(NUTLS_ERR_ARG, "nutls_state_get: null pointer");
  Engine* e = &h->eng;
  StateTensor* st;
  int rc = state_lookup(e, name, n_floats, &st);
  if (rc) return rc;
  if (int rcm = host_access_begin(e)) return rcm;
  if (e->offline) {
    for (int u = 0; u < e->outt; ++u)
      if (int rcu = copy_stream_tensor(e, st->buf[0], st->per_stream(), host_buf + static_cast<size_t>(u) * st->per_stream(), true, u * (e->offline + 1))) return rcu;
    return NUTLS_OK;
  }
  rc = copy_stream_tensor(e, st->buf[1 - e->next_parity], st->per_stream(), host_buf, true);
  if (rc == NUTLS_OK && st->ring_d > 1) rotate_ring(e, *st, host_buf, true);
  return rc;
}

int nutls_state_set(nutls_handle* h, const char* name, const float* host_buf, size_t n_floats) {
  if (!h || !host_buf) return fail(NUTLS_ERR_ARG, "nutls_state_set: null pointer");
  Engine* e = &h->eng;
  StateTensor* st;
  int rc = state_lookup(e, name, n_floats, &st);
  if (rc) return rc;
  if (int rcm = host_access_begin(e)) return rcm;
  if (e->offline) {
    for (int u = 0; u < e->outt; ++u)
      if (int rcu = copy_stream_tensor(e, st->buf[0], st->per_stream(), const_cast<float*>(host_buf) + static_cast<size_t>(u) * st->per_stream(), false, u * (e->offline + 1))) return rcu;
    return NUTLS_OK;
  }
  e->ys_dirty = true;      // a conv-input state changed under the fused kernel's carried partial sums: rebuilt before its next step
  e->lazy_edited = e->n_lazy != 0;
  if (e->lazy_edited) e->lazy_pending.assign(static_cast<size_t>(e->B), 1);
  // (causal32 CTFA: the 31-frame time-attention history of a streaming handle is library state outside the ABI's tensors.  It is NOT touched
  //  here: nutls_state_set takes [B, ...] buffers, and the per-stream workflow -- get, change one stream's row, set -- must leave the other
  //  B - 1 live streams alone.  A caller that loads a new utterance into stream b calls nutls_reset(h, b) first: nutls.h, nutls_state_set.)
  if (st->ring_d > 1) {
    std::vector<float> tmp(host_buf, host_buf + n_floats);
    rotate_ring(e, *st, tmp.data(), false);
    return copy_stream_tensor(e, st->buf[0], st->per_stream(), tmp.data(), false);
  }
  return copy_stream_tensor(e, st->buf[1 - e->next_parity], st->per_stream(), const_cast<float*>(host_buf), false);
}

/* All state tensors of ONE stream in signature order, concatenated (what the compat runner returns per frame): one
 * device-to-host copy of the stream's `prev`-side state block instead of one copy per tensor. */
int nutls_state_get_all(nutls_handle* h, int stream_idx, float* host_buf, size_t n_floats) {
  if (!h || !host_buf) return fail(NUTLS_ERR_ARG, "nutls_state_get_all: null pointer");
  Engine* e = &h->eng;
  if (e->offline) {      // (offline handles: stream_idx = utterance; its carried state lives in arena slot u (offline + 1))
    if (stream_idx < 0 || stream_idx >= e->outt) return fail(NUTLS_ERR_ARG, "nutls_state_get_all: utterance index out of range");
    stream_idx *= e->offline + 1;
  }
  if (stream_idx < 0 || stream_idx >= e->B) return fail(NUTLS_ERR_ARG, "nutls_state_get_all: stream index out of range");
  size_t total = 0;
  for (const StateTensor& st : e->states) total += st.per_stream();
  if (n_floats != total) return fail(NUTLS_ERR_ARG, "nutls_state_get_all: expected " + std::to_string(total) + " floats");
  if (int rcm = host_access_begin(e)) return rcm;
  // Only what is asked for crosses the bus: the buffers of the `prev`-side parity are one contiguous block of the stream's
  // arena slice (allocate_states), the baseline's history rings a second one -- one copy per run of adjacent buffers, then
  // the tensors are picked out of the host image.
  auto want = [&](const StateTensor& st) { return static_cast<size_t>((e->offline ? st.buf[0] : st.buf[1 - e->next_parity]) - e->arena); };
  std::vector<std::pair<size_t, size_t>> runs;      // [begin, end) offsets inside the slice, sorted and merged
  for (const StateTensor& st : e->states) runs.emplace_back(want(st), want(st) + st.per_stream());
  std::sort(runs.begin(), runs.end());
  size_t span = 0, n_runs = 0;
  for (const auto& r : runs) {
    if (n_runs && r.first <= runs[n_runs - 1].second + 1024) runs[n_runs - 1].second = std::max(runs[n_runs - 1].second, r.second);   // (slot padding between neighbours)
    else runs[n_runs++] = r;
    span = std::max(span, r.second);
  }
  runs.resize(n_runs);
  std::vector<float> slice(span);
  for (const auto& r : runs)
    HIP_TRY(hipMemcpy(slice.data() + r.first, e->arena + e->sstride * stream_idx + r.first, (r.second - r.first) * sizeof(float), hipMemcpyDeviceToHost));
  size_t o = 0;
  for (const StateTensor& st : e->states) {
    const float* src = slice.data() + want(st);
    std::memcpy(host_buf + o, src, st.per_stream() * sizeof(float));
    if (st.ring_d > 1) {      // physical ring order -> the reference's oldest-first order
      const size_t frame = st.per_stream() / st.ring_d;
      for (int j = 0; j < st.ring_d; ++j)
        std::memcpy(host_buf + o + j * frame, src + ((e->steps + j) % st.ring_d) * frame, frame * sizeof(float));
    }
    o += st.per_stream();
  }
  return NUTLS_OK;
}

int nutls_reset(nutls_handle* h, int stream_idx) {
  if (!h) return fail(NUTLS_ERR_ARG, "null handle");
  Engine* e = &h->eng;
  if (stream_idx >= (e->offline ? e->outt : e->B)) return fail(NUTLS_ERR_ARG, "nutls_reset: stream index out of range");
  const int utt = stream_idx;          // offline handles: the utterance (or -1: all); its carried state lives in arena slot u (offline + 1)
  if (e->offline && stream_idx >= 0) stream_idx *= e->offline + 1;
  if (int rcm = host_access_begin(e)) return rcm;
  // a stream's whole slice of the arena (state of both parities + scratch) is contiguous
  if (stream_idx < 0) HIP_TRY(hipMemset(e->arena, 0, e->sstride * sizeof(float) * e->B));
  else HIP_TRY(hipMemset(e->arena + e->sstride * stream_idx, 0, e->sstride * sizeof(float)));
  if (e->ta_hist) {      // offline handles, causal32 CTFA: the utterance's (all utterances') time-attention history
    const size_t per = static_cast<size_t>(12) * (31 + e->offline) * 64;
    if (utt < 0) HIP_TRY(hipMemset(e->ta_hist, 0, per * e->outt * sizeof(float)));
    else HIP_TRY(hipMemset(e->ta_hist + per * utt, 0, per * sizeof(float)));
  }
  if (e->fz_ta_ring) {      // streaming causal32 CTFA: the stream's (all streams') time-attention history
    const size_t per = static_cast<size_t>(12) * 32 * 64;
    if (stream_idx < 0) HIP_TRY(hipMemset(e->fz_ta_ring, 0, per * e->B * sizeof(float)));
    else HIP_TRY(hipMemset(e->fz_ta_ring + per * stream_idx, 0, per * sizeof(float)));
  }
  if (e->fe_tail) {   // STFT front / back end: previous hop and overlap tail
    const size_t hop = NUTLS_FRAME_STEP * sizeof(float);
    if (stream_idx < 0) {
      HIP_TRY(hipMemset(e->fe_tail, 0, hop * e->B));
      HIP_TRY(hipMemset(e->fe_ola, 0, hop * e->B));
    } else {
      HIP_TRY(hipMemset(e->fe_tail + static_cast<size_t>(NUTLS_FRAME_STEP) * stream_idx, 0, hop));
      HIP_TRY(hipMemset(e->fe_ola + static_cast<size_t>(NUTLS_FRAME_STEP) * stream_idx, 0, hop));
    }
  }
  if (e->fb_tw) {   // waveform block mode of an offline handle: the utterance's (all utterances') previous hop and overlap tail, both buffers of each
    const size_t hop = NUTLS_FRAME_STEP * sizeof(float);
    for (float* p : {e->fb_tail[0], e->fb_tail[1], e->fb_ola[0], e->fb_ola[1]}) {
      if (utt < 0) HIP_TRY(hipMemset(p, 0, hop * e->outt));
      else HIP_TRY(hipMemset(p + static_cast<size_t>(NUTLS_FRAME_STEP) * utt, 0, hop));
    }
  }
  if (int rcp = pcm_reset(e, utt)) return rcp;      // PCM gateway: the stream's / utterance's resampler histories
  HIP_TRY(hipDeviceSynchronize());
  return NUTLS_OK;
}

int nutls_debug_get(nutls_handle* h, const char* name, float* host_buf, size_t n_floats) {
  if (!h || !name || !host_buf) return fail(NUTLS_ERR_ARG, "nutls_debug_get: null pointer");
  Engine* e = &h->eng;
  if (std::string(name) == "phasor_block") {      // offline handles: the phasors of the last analysed block, [utterances, its n_hops, 257, 2]
    if (!e->offline) return fail(NUTLS_ERR_ARG, "debug tensor phasor_block: not an offline handle");
    if (!e->fb_ph || !e->fb_hops) return fail(NUTLS_ERR_ARG, "debug tensor not allocated yet: phasor_block");
    if (n_floats != static_cast<size_t>(e->outt) * e->fb_hops * (NUTLS_FRAME_STEP + 1) * 2) return fail(NUTLS_ERR_ARG, "size mismatch for debug tensor phasor_block");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_buf, e->fb_ph, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return NUTLS_OK;
  }
  {   // the I/O staging buffers and the STFT phasors are plain [B, n] arrays
    const std::string nm(name);
    const float* src = nullptr;
    size_t per = 0;
    if (nm == "mag_in") { src = e->io_in; per = NUTLS_BINS; }
    else if (nm == "mag_out") { src = e->io_out; per = NUTLS_BINS; }
    else if (nm == "phasor") { src = e->fe_ph; per = 2 * (NUTLS_FRAME_STEP + 1); }
    if (per) {
      if (!src) return fail(NUTLS_ERR_ARG, "debug tensor not allocated yet: " + nm);
      if (n_floats != per * e->B) return fail(NUTLS_ERR_ARG, "size mismatch for debug tensor " + nm);
      if (int rcm = host_access_begin(e)) return rcm;
      HIP_TRY(hipMemcpy(host_buf, src, n_floats * sizeof(float), hipMemcpyDeviceToHost));
      return NUTLS_OK;
    }
  }
  if (e->fz_dbg && e->mode == 3) {
    // activation trace of the fused kernel's profiling build (nutls_debug_trace): "<stage>.y" of all 12 stages, "<stage>.up" of the 6
    // decoder stages, "input_layer" -- tensors the fused kernel keeps in LDS
    const std::string nm(name);
    int slot = -1;
    size_t per = 0;
    if (nm == "input_layer") { slot = 0; per = 256 * 64; }
    for (int s = 0; s < 6 && slot < 0; ++s) {
      if (nm == std::string(kEncoder[s].prefix) + ".y") { slot = 1 + s; per = static_cast<size_t>(kEncoder[s].f0) * 64; }
      else if (nm == std::string(kDecoder[s].prefix) + ".y") { slot = 7 + s; per = static_cast<size_t>(kDecoder[s].f0) * 64; }
      else if (nm == std::string(kDecoder[s].prefix) + ".up") { slot = 13 + s; per = static_cast<size_t>(kDecoder[s].f0) * 128; }
    }
    if (slot >= 0) {
      if (n_floats != per * e->B) return fail(NUTLS_ERR_ARG, std::string("size mismatch for debug tensor ") + name);
      HIP_TRY(hipSetDevice(e->device));
      HIP_TRY(hipDeviceSynchronize());
      for (int b = 0; b < e->B; ++b)
        HIP_TRY(hipMemcpy(host_buf + per * b, e->fz_dbg + (static_cast<size_t>(b) * kDbgSlots + slot) * kDbgSlotFloats, per * sizeof(float), hipMemcpyDeviceToHost));
      return NUTLS_OK;
    }
  }
  auto it = e->debug.find(name);
  if (it == e->debug.end()) return fail(NUTLS_ERR_ARG, std::string("unknown debug tensor: ") + name);
  if (n_floats != it->second.second * e->B) return fail(NUTLS_ERR_ARG, std::string("size mismatch for debug tensor ") + name);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  return copy_stream_tensor(e, it->second.first, it->second.second, host_buf, true);
}

}  // extern "C"
