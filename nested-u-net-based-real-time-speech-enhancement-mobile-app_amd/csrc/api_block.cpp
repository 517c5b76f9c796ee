// Offline / block entry points of the C ABI (include/nutls.h): the block plan and its chunk pipeline, the waveform front and back end of an
// offline handle, and the nutls_process_block* / nutls_stft_block* / nutls_istft_block* / nutls_enhance_block* families -- uniform or with
// per-utterance counts (ragged), from device or host buffers.  The engine they drive: engine.cpp.
#include <algorithm>
#include <cstdint>

#include "engine.hpp"

namespace nutls {

// ---- offline / block mode -------------------------------------------------------------------------
// plan[0] reads the previous-frame tap of every state tensor from its second ping-pong buffer and writes the
// current frame into the first.  The block plan keeps ONE buffer per tensor: the current frame of block frame
// t is arena slot t+1, its previous frame slot t -- i.e. "cur" pointers move one slot up, "prev" pointers become
// the first buffer at slot 0; the kernels then index slots with the frame number.
int build_offline_plan(Engine* e) {
  const size_t S = e->sstride;
  auto rw = [&](const float* q) -> float* {
    if (!q) return nullptr;
    float* p = const_cast<float*>(q);
    if (p < e->arena || p >= e->arena + S) return p;               // weights, I/O staging
    for (const StateTensor& st : e->states)
      if (st.buf[1] != st.buf[0] && p >= st.buf[1] && p < st.buf[1] + st.per_stream()) return st.buf[0] + (p - st.buf[1]);
    return p + S;
  };
  e->plan_off = e->plan[0];
  for (Launch& L : e->plan_off) {
    switch (L.kind) {
      case Launch::CONV:
        L.conv.src0 = rw(L.conv.src0); L.conv.src1 = rw(L.conv.src1); L.conv.dst0 = rw(L.conv.dst0); L.conv.dst1 = rw(L.conv.dst1);
        break;
      case Launch::LSTM:
        L.lstm.x = rw(L.lstm.x); L.lstm.dst = rw(L.lstm.dst);
        L.lstm.h_in = rw(L.lstm.h_in); L.lstm.c_in = rw(L.lstm.c_in); L.lstm.h_out = rw(L.lstm.h_out); L.lstm.c_out = rw(L.lstm.c_out);
        break;
      case Launch::CTFA: L.ctfa.x = rw(L.ctfa.x); L.ctfa.e0 = rw(L.ctfa.e0); L.ctfa.y = rw(L.ctfa.y); break;
      case Launch::INLAYER: L.inl.y = rw(L.inl.y); break;
      case Launch::OUTCONV: L.outc.x = rw(L.outc.x); break;
      case Launch::DDB: return fail(NUTLS_ERR_ARG, "offline mode: LSTM variant only");
    }
  }
  int g = 0;
  for (const Launch& L : e->plan_off) {
    e->ogroup.push_back(g);
    if (L.kind == Launch::LSTM) ++g;
  }
  if (g + 2 > Engine::kGroups) return fail(NUTLS_ERR_ARG, "offline plan: more bottlenecks than pipeline groups");      // (the last event of a chunk is its join event)
  // (the chunk streams and their events are created when a block first runs with that many chunks: ensure_chunk_streams)
  int rc = dev_alloc(e, (static_cast<size_t>(e->outt) * e->offline + kScanReadAhead) * 84, &e->zx, true);
  if (rc) return rc;
  return dev_alloc(e, static_cast<size_t>(e->outt) * 12 * (31 + e->offline) * 64, &e->ta_hist, true);      // [utterance][stage][31 + frame][64]
}

// The counts of a _host entry: checked (nothing is touched when one is out of range), then copied to the handle's device buffer on the
// library's stream, in front of the work that reads them.
int upload_counts(Engine* e, const int* counts, int n, const char* who) {
  for (int u = 0; u < e->outt; ++u)
    if (counts[u] < 0 || counts[u] > n)
      return fail(NUTLS_ERR_ARG, std::string(who) + ": count " + std::to_string(counts[u]) + " of utterance " + std::to_string(u) + " is outside 0 .. " + std::to_string(n));
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = dev_alloc_once(e, static_cast<size_t>(e->outt), &e->d_counts, false)) return rc;
  if (int rc = enqueue_on(e, e->stream)) return rc;      // (behind what earlier calls queued on the callers' streams)
  HIP_TRY(hipMemcpyAsync(e->d_counts, counts, static_cast<size_t>(e->outt) * sizeof(int), hipMemcpyHostToDevice, e->stream));
  return NUTLS_OK;
}

}  // namespace nutls

using namespace nutls;

extern "C" {

// ---- waveform block mode: front / back end state of an offline handle ---------------------------
// (an offline handle's B counts arena slots, utterances x (max_frames + 1): frontend_init's per-stream buffers are not its shape)
static int frontend_block_init(Engine* e) {
  if (e->fb_tw) return NUTLS_OK;
  const size_t hop = static_cast<size_t>(e->outt) * NUTLS_FRAME_STEP;
  int rc;
  float* twd = nullptr;
  const std::vector<float> tw = stft_block_twiddles();
  if ((rc = dev_alloc(e, hop, &e->fb_tail[0], true)) || (rc = dev_alloc(e, hop, &e->fb_tail[1], true)) || (rc = dev_alloc(e, hop, &e->fb_ola[0], true)) ||
      (rc = dev_alloc(e, hop, &e->fb_ola[1], true)) ||
      (rc = dev_alloc(e, static_cast<size_t>(e->outt) * e->offline * (NUTLS_FRAME_STEP + 1) * 2, &e->fb_ph, true)) ||
      (rc = dev_alloc(e, NUTLS_FRAME_LEN, &e->fb_win, false)) || (rc = dev_alloc(e, NUTLS_FRAME_LEN, &e->fb_inv, false)) || (rc = dev_alloc(e, tw.size(), &twd, false)))
    return rc;
  std::vector<float> win, inv;
  frontend_tables(&win, &inv, nullptr);
  HIP_TRY(hipMemcpy(e->fb_win, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->fb_inv, inv.data(), inv.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(twd, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
  e->fb_tw = twd;
  return NUTLS_OK;
}

// common argument checks of the four block entries; `who` names the entry in the message
static int block_args(nutls_handle* h, bool pointers_ok, int n_hops, const char* who) {
  if (!h || !pointers_ok) return fail(NUTLS_ERR_ARG, std::string(who) + ": null pointer");
  const Engine* e = &h->eng;
  if (!e->offline)
    return fail(NUTLS_ERR_ARG, std::string(who) + ": not an offline handle (nutls_create_offline); a streaming handle takes PCM hop by hop through nutls_enhance_hop");
  if (n_hops < 1 || n_hops > e->offline) return fail(NUTLS_ERR_ARG, std::string(who) + ": n_hops out of range (1 .. max_frames)");
  return NUTLS_OK;
}

static int block_dc(int dc_mode, const char* who) {
  if (dc_mode != NUTLS_DC_EDGE && dc_mode != NUTLS_DC_ZERO) return fail(NUTLS_ERR_ARG, std::string(who) + ": dc_mode must be NUTLS_DC_EDGE or NUTLS_DC_ZERO");
  return NUTLS_OK;
}

static int stft_block_launch(Engine* e, const float* pcm_in, float* mag, int n_hops, hipStream_t s, const int* hops = nullptr) {
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = frontend_block_init(e)) return rc;
  if (int rc = enqueue_on(e, s)) return rc;
  HIP_TRY(launch_stft_block(pcm_in, e->fb_tail[e->fb_tail_par], e->fb_tail[1 - e->fb_tail_par], e->fb_win, e->fb_tw, mag, e->fb_ph, hops, e->outt, n_hops, s));
  e->fb_tail_par ^= 1;
  e->fb_hops = n_hops;
  return NUTLS_OK;
}

// noisy: the magnitudes of the same block (the enhance entries: io_in; nutls_istft_block_mix: the caller's) or null (the stand-alone half, which
// has none).  With noisy rows and an attenuation limit in force (nutls_set_atten_limit) the mix runs for the whole launch.
static int istft_block_launch(Engine* e, const float* mag, const float* noisy, float* pcm_out, int n_hops, int dc_mode, hipStream_t s, const int* hops = nullptr) {
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = frontend_block_init(e)) return rc;
  if (n_hops != e->fb_hops) return fail(NUTLS_ERR_ARG, "nutls_istft_block: n_hops differs from the block the phasors inside the handle belong to (nutls_stft_block first)");
  if (int rc = enqueue_on(e, s)) return rc;
  HIP_TRY(launch_istft_block(mag, e->atten_on ? noisy : nullptr, e->d_atten, e->fb_ph, e->fb_inv, e->fb_tw, e->fb_ola[e->fb_ola_par],
                             e->fb_ola[1 - e->fb_ola_par], pcm_out, dc_mode == NUTLS_DC_EDGE ? 1 : 0, hops, e->outt, n_hops, s));
  e->fb_ola_par ^= 1;
  return NUTLS_OK;
}

int nutls_offline_set_pipeline(nutls_handle* h, int chunks) {
  if (!h || !h->eng.offline) return fail(NUTLS_ERR_ARG, "nutls_offline_set_pipeline: not an offline handle");
  if (chunks < 0 || chunks > Engine::kMaxChunks) return fail(NUTLS_ERR_ARG, "nutls_offline_set_pipeline: chunks must be 0 (automatic) .. 16");
  h->eng.ochunks = chunks;
  return NUTLS_OK;
}

// Launches [first, last) of the block plan for frames [t0, t0 + n) on stream s: every per-frame tensor (arena slots,
// magnitudes in / out, LSTM input products, time-attention history) is addressed from frame t0.
static int launch_block_range(Engine* e, size_t first, size_t last, int t0, int n, bool roll_hist, hipStream_t s, int n_block = 0) {
  // (several utterances: the launches run all of them -- dense stream index u * n + t, SlotMap: utterance u's frames start (offline + 1) slots
  //  after utterance u - 1's; the magnitudes [U, n_block, 256] of the block: a chunk's n frames of utterance u sit n_block rows after those of u - 1)
  const int U = e->outt;
  const SlotMap sm_io = U > 1 ? make_slot_map(n, (n_block > 0 ? n_block : n) - n) : make_slot_map(0, 0);
  const SlotMap sm = U > 1 ? make_slot_map(n, e->offline + 1 - n) : make_slot_map(0, 0);
  const long long utt_stride = static_cast<long long>(e->offline + 1) * static_cast<long long>(e->sstride);
  const long long hist_ustride = static_cast<long long>(12) * (31 + e->offline) * 64;
  const float* a0 = e->arena;
  const float* a1 = e->arena + static_cast<size_t>(U) * (static_cast<size_t>(e->offline) + 1) * e->sstride;
  const size_t d = static_cast<size_t>(t0) * e->sstride;
  auto shc = [&](const float*& q) { if (q && q >= a0 && q < a1) q += d; };
  auto sh = [&](float*& q) { if (q && q >= a0 && q < a1) q += d; };
  int n_ctfa = 0;
  for (size_t i = 0; i < first; ++i) n_ctfa += e->plan_off[i].kind == Launch::CTFA;
  for (size_t i = first; i < last; ++i) {
    Launch L = e->plan_off[i];
    hipError_t err = hipSuccess;
    switch (L.kind) {
      case Launch::CONV:
        shc(L.conv.src0); shc(L.conv.src1); sh(L.conv.dst0); sh(L.conv.dst1);
        L.conv.B = U * n;
        L.conv.sm = sm;
        L.conv.use_bf16 = e->off_bf16 && L.conv.wbf != nullptr;
        err = launch_conv(L.ck, L.conv, s, e->conv_knobs);
        break;
      case Launch::LSTM:
        shc(L.lstm.x); sh(L.lstm.dst); shc(L.lstm.h_in); shc(L.lstm.c_in); sh(L.lstm.h_out); sh(L.lstm.c_out);
        L.lstm.B = U * n;
        L.lstm.sm = sm;
        err = launch_lstm_block(L.lstm, e->zx + static_cast<size_t>(U) * t0 * 84, n, s, U, utt_stride);
        break;
      case Launch::CTFA: {
        shc(L.ctfa.x); shc(L.ctfa.e0); sh(L.ctfa.y);
        L.ctfa.B = U * n;
        L.ctfa.sm = sm;
        float* hist = e->ta_hist + static_cast<size_t>(n_ctfa) * (31 + e->offline) * 64 + static_cast<size_t>(t0) * 64;
        if (e->ctfa_causal) err = launch_ctfa_causal(L.ctfa, hist, roll_hist, s, U, hist_ustride);
        else err = launch_ctfa(L.ctfa, s);
        ++n_ctfa;
        break;
      }
      case Launch::INLAYER:
        L.inl.x += static_cast<size_t>(t0) * NUTLS_BINS; sh(L.inl.y);
        L.inl.n_pos = U * n * NUTLS_BINS;
        L.inl.sm = sm;
        L.inl.sm_io = sm_io;
        err = launch_input_layer(L.inl, s);
        break;
      case Launch::OUTCONV:
        shc(L.outc.x); L.outc.y += static_cast<size_t>(t0) * NUTLS_BINS;
        L.outc.n_pos = U * n * NUTLS_BINS;
        L.outc.sm = sm;
        L.outc.sm_io = sm_io;
        err = launch_out_conv(L.outc, s);
        break;
      default: err = hipErrorInvalidValue;
    }
    if (err != hipSuccess) return fail(NUTLS_ERR_HIP, "block launch " + L.name + ": " + hipGetErrorString(err));
  }
  return NUTLS_OK;
}

// Streams + events of the block pipeline for `chunks` chunks, created on first use (a handle that never pipelines owns none).
static int ensure_chunk_streams(Engine* e, int chunks) {
  if (!e->oev_fork) HIP_TRY(hipEventCreateWithFlags(&e->oev_fork, hipEventDisableTiming));
  while (static_cast<int>(e->ostream.size()) < chunks) {
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    e->ostream.push_back(st);
    for (int k = 0; k < 2 * Engine::kGroups; ++k) {      // per group: convs done, LSTM done
      hipEvent_t ev = nullptr;
      HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      e->oev.push_back(ev);
    }
  }
  return NUTLS_OK;
}

int nutls_offline_set_ctfa_mode(nutls_handle* h, int mode) {
  if (!h || !h->eng.offline) return fail(NUTLS_ERR_ARG, "nutls_offline_set_ctfa_mode: not an offline handle");
  if (mode != NUTLS_CTFA_FRAME && mode != NUTLS_CTFA_CAUSAL32) return fail(NUTLS_ERR_ARG, "nutls_offline_set_ctfa_mode: unknown mode");
  Engine* e = &h->eng;
  if (e->ctfa_causal == (mode == NUTLS_CTFA_CAUSAL32)) return NUTLS_OK;      // already in effect: the history stays
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(e->ta_hist, 0, static_cast<size_t>(e->outt) * 12 * (31 + e->offline) * 64 * sizeof(float)));      // a mode switch starts a new history
  e->ctfa_causal = mode == NUTLS_CTFA_CAUSAL32;
  return NUTLS_OK;
}

// One block of n_frames frames of every utterance.  frames == nullptr: nutls_process_block.  frames != nullptr (DEVICE, [utterances]): the
// ragged block of nutls_process_block_ragged -- every layer is causal in time and utterances never mix, so the block itself runs exactly as
// the uniform one of width n_frames (same launches, same sizes); the rows behind an utterance's count are zeros on the way in and out, and the
// commit behind the block takes what is carried from frame frames[u] instead of frame n_frames.  in_place: the caller (nutls_enhance_block_ragged)
// has staged the library's own buffers -- its analysis wrote the zero rows, its synthesis reads no row behind a count.
static int process_block_impl(nutls_handle* h, const float* mag_in, float* mag_out, int n_frames, const int* frames, bool in_place, void* stream,
                              const char* who) {
  if (!h || !mag_in || !mag_out) return fail(NUTLS_ERR_ARG, std::string(who) + ": null pointer");
  Engine* e = &h->eng;
  if (!e->offline) return fail(NUTLS_ERR_ARG, std::string(who) + ": not an offline handle (nutls_create_offline)");
  if (n_frames < 1 || n_frames > e->offline) return fail(NUTLS_ERR_ARG, std::string(who) + ": n_frames out of range");
  if (frames && ((reinterpret_cast<uintptr_t>(mag_in) | reinterpret_cast<uintptr_t>(mag_out)) & 15))
    return fail(NUTLS_ERR_ARG, std::string(who) + ": with frame counts the magnitude buffers must be 16-byte aligned");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = enqueue_on(e, s)) return rc;
  const int U = e->outt;
  const size_t bytes = static_cast<size_t>(U) * n_frames * NUTLS_BINS * sizeof(float);
  if (frames) {
    if (!in_place) HIP_TRY(launch_ragged_rows(mag_in, e->io_in, frames, U, n_frames, s));
  } else if (mag_in != e->io_in) HIP_TRY(hipMemcpyAsync(e->io_in, mag_in, bytes, hipMemcpyDeviceToDevice, s));
  int C = e->ochunks;
  if (C == 0) C = n_frames >= 768 ? 3 : n_frames >= 256 ? 2 : 1;      // (four compute queues are served at a time: chunk 0 rides on the caller's stream, three chunks = three queues)
  C = std::max(1, std::min({C, static_cast<int>(Engine::kMaxChunks), n_frames}));
  // (several utterances: every launch runs all of them -- their 13 scans side by side on their own wavefronts, the small layers U times fuller;
  //  the chunks cut the frames of every utterance alike)
  if (C == 1) {
    int rc = launch_block_range(e, 0, e->plan_off.size(), 0, n_frames, frames == nullptr, s);      // (ragged: the history is rolled by the commit below)
    if (rc) return rc;
  } else {
    // chunk c, group g (= the layers up to and including bottleneck g) starts when chunk c-1 has finished group g: then
    // the previous-frame taps of all its layers, the LSTM's h / c and the time-attention history of frame t0-1 exist
    const int per = (n_frames + C - 1) / C;
    const int n_groups = e->ogroup.back() + 1;
    // chunk 0 runs on the caller's stream, chunk c > 0 on chunk stream c-1: a block with C chunks keeps C hardware queues
    // busy, not C + 1 with the caller's queue parked on the join -- the GPU serves four compute queues at a time, and a fifth
    // one that holds a dependency of the others serialises the whole pipeline (4 chunks: 11.7 ms instead of < 4.5)
    if (int rc0 = ensure_chunk_streams(e, C - 1)) return rc0;
    auto cs = [&](int c) { return c == 0 ? s : e->ostream[c - 1]; };
    HIP_TRY(hipEventRecord(e->oev_fork, s));
    for (int c = 1; c < C; ++c) HIP_TRY(hipStreamWaitEvent(cs(c), e->oev_fork, 0));
    int rc = NUTLS_OK;
    size_t first = 0;
    for (int g = 0; g < n_groups && rc == NUTLS_OK; ++g) {
      size_t last = first;
      while (last < e->plan_off.size() && e->ogroup[last] == g) ++last;
      // a group = its conv-like layers, then its LSTM (input products, scan, Dense) if it has one: two dependencies per
      // group -- chunk c's convs start when chunk c-1's convs of the group are done (previous-frame taps, time-attention
      // history), its scan when that chunk's scan is (h / c); the convs do not wait for a scan they do not read
      size_t mid = last;
      for (size_t i = first; i < last; ++i)
        if (e->plan_off[i].kind == Launch::LSTM) { mid = i; break; }
      constexpr int EV = 2 * Engine::kGroups;
      for (int c = 0; c < C && rc == NUTLS_OK; ++c) {
        const int t0 = c * per, n = std::min(per, n_frames - t0);
        if (n <= 0) continue;
        for (int half = 0; half < 2 && rc == NUTLS_OK; ++half) {
          const size_t a = half ? mid : first, b = half ? last : mid;
          if (a == b) continue;
          const int slot = half * Engine::kGroups + g;
          if (c > 0 && hipStreamWaitEvent(cs(c), e->oev[(c - 1) * EV + slot], 0) != hipSuccess) rc = fail(NUTLS_ERR_HIP, "block pipeline: hipStreamWaitEvent");
          if (rc == NUTLS_OK) rc = launch_block_range(e, a, b, t0, n, false, cs(c), n_frames);
          if (rc == NUTLS_OK && c + 1 < C && hipEventRecord(e->oev[c * EV + slot], cs(c)) != hipSuccess) rc = fail(NUTLS_ERR_HIP, "block pipeline: hipEventRecord");
        }
      }
      first = last;
    }
    // join: the caller's stream continues after every chunk stream -- also when a launch failed half way, so that
    // whatever was enqueued is ordered before the caller's next work
    for (int c = 1; c < C; ++c) {
      hipEvent_t done = e->oev[(c - 1) * 2 * Engine::kGroups + Engine::kGroups - 1];      // a spare slot of chunk stream c-1's events (groups end at kGroups - 2)
      if (hipEventRecord(done, cs(c)) == hipSuccess) (void)hipStreamWaitEvent(s, done, 0);
    }
    if (rc) return rc;
    if (e->ctfa_causal && !frames)
      for (int k = 0; k < 12; ++k) {
        hipError_t err = launch_ctfa_hist_roll(e->ta_hist + static_cast<size_t>(k) * (31 + e->offline) * 64, n_frames, s, U, static_cast<long long>(12) * (31 + e->offline) * 64);
        if (err != hipSuccess) return fail(NUTLS_ERR_HIP, std::string("time-attention history roll: ") + hipGetErrorString(err));
      }
  }
  if (frames) {
    // stage-out and commit, behind the join of the chunk streams: utterance u's carried state is the slot of its frame frames[u], its
    // time-attention history the 31 rows in front of that frame's; frames[u] = 0 moves nothing
    if (!in_place) HIP_TRY(launch_ragged_rows(e->io_out, mag_out, frames, U, n_frames, s));
    if (e->ctfa_causal) HIP_TRY(launch_ragged_hist_roll(e->ta_hist, 31 + e->offline, frames, U, n_frames, s));
    HIP_TRY(launch_ragged_state_gather(e->arena, static_cast<long long>(e->sstride), e->offline + 1, frames, U, n_frames, s));
    e->steps += n_frames;
    return NUTLS_OK;
  }
  if (mag_out != e->io_out) HIP_TRY(hipMemcpyAsync(mag_out, e->io_out, bytes, hipMemcpyDeviceToDevice, s));
  // the last frame's slot of every utterance becomes its carried state of the next block
  {
    const size_t pitch = (static_cast<size_t>(e->offline) + 1) * e->sstride * sizeof(float);
    HIP_TRY(hipMemcpy2DAsync(e->arena, pitch, e->arena + static_cast<size_t>(n_frames) * e->sstride, pitch, e->sstride * sizeof(float), U, hipMemcpyDeviceToDevice, s));
  }
  e->steps += n_frames;
  return NUTLS_OK;
}

int nutls_process_block(nutls_handle* h, const float* mag_in, float* mag_out, int n_frames, void* stream) {
  return process_block_impl(h, mag_in, mag_out, n_frames, nullptr, false, stream, "nutls_process_block");
}

int nutls_process_block_ragged(nutls_handle* h, const float* mag_in, float* mag_out, int n_frames, const int* frames, void* stream) {
  return process_block_impl(h, mag_in, mag_out, n_frames, frames, false, stream, frames ? "nutls_process_block_ragged" : "nutls_process_block");
}

int nutls_stft_block(nutls_handle* h, const float* pcm_in, float* mag, int n_hops, void* stream) {
  if (int rc = block_args(h, pcm_in && mag, n_hops, "nutls_stft_block")) return rc;
  return stft_block_launch(&h->eng, pcm_in, mag, n_hops, static_cast<hipStream_t>(stream));
}

int nutls_istft_block(nutls_handle* h, const float* mag, float* pcm_out, int n_hops, int dc_mode, void* stream) {
  if (int rc = block_args(h, mag && pcm_out, n_hops, "nutls_istft_block")) return rc;
  if (int rc = block_dc(dc_mode, "nutls_istft_block")) return rc;
  return istft_block_launch(&h->eng, mag, nullptr, pcm_out, n_hops, dc_mode, static_cast<hipStream_t>(stream));
}

int nutls_enhance_block(nutls_handle* h, const float* pcm_in, float* pcm_out, int n_hops, int dc_mode, void* stream) {
  if (int rc = block_args(h, pcm_in && pcm_out, n_hops, "nutls_enhance_block")) return rc;
  if (int rc = block_dc(dc_mode, "nutls_enhance_block")) return rc;
  Engine* e = &h->eng;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // analysis, model and synthesis follow each other on the caller's stream: the chunk streams of the block pipeline fork from it behind the
  // analysis and have joined it again when nutls_process_block returns
  if (int rc = stft_block_launch(e, pcm_in, e->io_in, n_hops, s)) return rc;
  if (int rc = nutls_process_block(h, e->io_in, e->io_out, n_hops, stream)) return rc;
  return istft_block_launch(e, e->io_out, e->io_in, pcm_out, n_hops, dc_mode, s);
}

// ---- ragged waveform blocks: hops [utterances] of int, utterance u has hops[u] real hops in a block whose row stride is n_hops (nutls.h) ----
int nutls_stft_block_ragged(nutls_handle* h, const float* pcm_in, float* mag, int n_hops, const int* hops, void* stream) {
  if (!hops) return nutls_stft_block(h, pcm_in, mag, n_hops, stream);
  if (int rc = block_args(h, pcm_in && mag, n_hops, "nutls_stft_block_ragged")) return rc;
  return stft_block_launch(&h->eng, pcm_in, mag, n_hops, static_cast<hipStream_t>(stream), hops);
}

int nutls_istft_block_ragged(nutls_handle* h, const float* mag, float* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream) {
  if (!hops) return nutls_istft_block(h, mag, pcm_out, n_hops, dc_mode, stream);
  if (int rc = block_args(h, mag && pcm_out, n_hops, "nutls_istft_block_ragged")) return rc;
  if (int rc = block_dc(dc_mode, "nutls_istft_block_ragged")) return rc;
  return istft_block_launch(&h->eng, mag, nullptr, pcm_out, n_hops, dc_mode, static_cast<hipStream_t>(stream), hops);
}

// the synthesis half with the noisy rows in the caller's hands (nutls_stft_block wrote them there): honours the attenuation limit; hops: DEVICE or null
int nutls_istft_block_mix(nutls_handle* h, const float* est, const float* noisy, float* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream) {
  if (int rc = block_args(h, est && noisy && pcm_out, n_hops, "nutls_istft_block_mix")) return rc;
  if (int rc = block_dc(dc_mode, "nutls_istft_block_mix")) return rc;
  return istft_block_launch(&h->eng, est, noisy, pcm_out, n_hops, dc_mode, static_cast<hipStream_t>(stream), hops);
}

int nutls_enhance_block_ragged(nutls_handle* h, const float* pcm_in, float* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream) {
  if (!hops) return nutls_enhance_block(h, pcm_in, pcm_out, n_hops, dc_mode, stream);
  if (int rc = block_args(h, pcm_in && pcm_out, n_hops, "nutls_enhance_block_ragged")) return rc;
  if (int rc = block_dc(dc_mode, "nutls_enhance_block_ragged")) return rc;
  Engine* e = &h->eng;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the analysis writes zero magnitudes behind the counts and the synthesis reads no row there: the block runs in place on the library's buffers
  if (int rc = stft_block_launch(e, pcm_in, e->io_in, n_hops, s, hops)) return rc;
  if (int rc = process_block_impl(h, e->io_in, e->io_out, n_hops, hops, true, stream, "nutls_enhance_block_ragged")) return rc;
  return istft_block_launch(e, e->io_out, e->io_in, pcm_out, n_hops, dc_mode, s, hops);
}

// ---- the _host entries: one body ------------------------------------------------------------------------------------------------------
// The caller's rows to the library's staging buffers, the device entry on the library's stream, the results back, one synchronisation.
// wave: PCM hops through nutls_enhance_block_ragged (staging allocated on first use), else magnitudes through process_block_impl on the
// handle's io buffers.  counts: HOST, or null for the uniform block -- which is the ragged call with null counts.  `who` names the entry.
static int block_host(nutls_handle* h, const float* in, float* out, int n, const int* counts, bool wave, int dc_mode, const char* who) {
  if (wave) {
    if (int rc = block_args(h, in && out, n, who)) return rc;
    if (int rc = block_dc(dc_mode, who)) return rc;
  } else {
    if (!h || !in || !out) return fail(NUTLS_ERR_ARG, std::string(who) + ": null pointer");
    if (!h->eng.offline || n < 1 || n > h->eng.offline) return fail(NUTLS_ERR_ARG, std::string(who) + ": not an offline handle or n_frames out of range");
  }
  Engine* e = &h->eng;
  if (counts)
    if (int rc = upload_counts(e, counts, n, who)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if (wave && !e->fb_pcm_in) {
    const size_t floats = static_cast<size_t>(e->outt) * e->offline * NUTLS_FRAME_STEP;
    if (int rc = dev_alloc(e, floats, &e->fb_pcm_out, false)) return rc;
    if (int rc = dev_alloc(e, floats, &e->fb_pcm_in, false)) return rc;
  }
  float* const d_in = wave ? e->fb_pcm_in : e->io_in;
  float* const d_out = wave ? e->fb_pcm_out : e->io_out;
  const int* const d_counts = counts ? e->d_counts : nullptr;
  // (ragged: the rows behind the counts cross the link too and are zeroed on the device -- the stage-in kernel runs in place on the library's buffer)
  const size_t bytes = static_cast<size_t>(e->outt) * n * (wave ? NUTLS_FRAME_STEP : NUTLS_BINS) * sizeof(float);
  if (int rc = enqueue_on(e, e->stream)) return rc;      // (behind what earlier calls queued on the callers' streams)
  HIP_TRY(hipMemcpyAsync(d_in, in, bytes, hipMemcpyHostToDevice, e->stream));
  if (int rc = wave ? nutls_enhance_block_ragged(h, d_in, d_out, n, d_counts, dc_mode, e->stream)
                    : process_block_impl(h, d_in, d_out, n, d_counts, false, e->stream, who))
    return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  enqueue_idle(e);
  return NUTLS_OK;
}

int nutls_process_block_host(nutls_handle* h, const float* mag_in, float* mag_out, int n_frames) {
  return block_host(h, mag_in, mag_out, n_frames, nullptr, false, 0, "nutls_process_block_host");
}

int nutls_process_block_ragged_host(nutls_handle* h, const float* mag_in, float* mag_out, int n_frames, const int* frames) {
  return block_host(h, mag_in, mag_out, n_frames, frames, false, 0, frames ? "nutls_process_block_ragged_host" : "nutls_process_block_host");
}

int nutls_enhance_block_host(nutls_handle* h, const float* pcm_in, float* pcm_out, int n_hops, int dc_mode) {
  return block_host(h, pcm_in, pcm_out, n_hops, nullptr, true, dc_mode, "nutls_enhance_block_host");
}

int nutls_enhance_block_ragged_host(nutls_handle* h, const float* pcm_in, float* pcm_out, int n_hops, const int* hops, int dc_mode) {
  return block_host(h, pcm_in, pcm_out, n_hops, hops, true, dc_mode, hops ? "nutls_enhance_block_ragged_host" : "nutls_enhance_block_host");
}

}  // extern "C"
