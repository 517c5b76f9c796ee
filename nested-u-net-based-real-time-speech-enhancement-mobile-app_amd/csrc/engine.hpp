// What the host translation units behind the C ABI share -- engine.cpp (the engine) and api_stream.cpp, api_block.cpp, api_state.cpp,
// api_profile.cpp, api_pcm.cpp (the entry points): the Engine inside a handle, the small structs it is made of, the one error slot and the internal
// functions that cross a file boundary.  Host only, like fused_host.hpp: no kernel translation unit includes it.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/nutls.h"
#include "nutls_internal.hpp"
#include "fused_host.hpp"
#include "ragged.hpp"
#include "pcm.hpp"
#include "packet.hpp"
#include "channels.hpp"

namespace nutls {

// The error slot of nutls_last_error (thread-local): ONE definition for the whole library, in engine.cpp.
int fail(int code, const std::string& msg);
#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess)                                                                   \
      return fail(NUTLS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));       \
  } while (0)

// ---------------------------------------------------------------------------------------------
struct StageDesc {
  const char* prefix;
  int depth, f0;
  const char* conv_tag;
  const char* spconv_tag;
  const char* resample;
  int pair;  // decoder: index into kEncoder of the paired encoder stage; encoder: -1
};
// stage order / pairing: converter_proposed.py:221-727 (decoder pairs at :464,500,542,585,627,675)
static const StageDesc kEncoder[6] = {
    {"msfe6_en", 6, 256, "msfe6_ee", "msfe6_ed", "msfe6_down_sampling", -1},
    {"msfe5_en", 5, 128, "msfe5_ee", "msfe5_ed", "msfe5_down_sampling", -1},
    {"msfe4_en", 4, 64, "msfe4_ee", "msfe4_ed", "msfe4_down_sampling", -1},
    {"msfe4_en2", 4, 32, "msfe4_ee2", "msfe4_ed2", "msfe4_down_sampling2", -1},
    {"msfe4_en3", 4, 16, "msfe4_ee3", "msfe4_ed3", "msfe4_down_sampling3", -1},
    {"msfe3_en", 3, 8, "msfe3_ee", "msfe3_ed", "msfe3_down_sampling", -1},
};
static const StageDesc kDecoder[6] = {
    {"msfe3_de", 3, 8, "msfe3_de", "msfe3_dd", "msfe3_upsampling", 5},
    {"msfe4_de", 4, 16, "msfe4_de", "msfe4_dd", "msfe4_upsampling", 4},
    {"msfe4_de2", 4, 32, "msfe4_de2", "msfe4_dd2", "msfe4_upsampling2", 3},
    {"msfe4_de3", 4, 64, "msfe4_de3", "msfe4_dd3", "msfe4_upsampling3", 2},
    {"msfe5_de", 5, 128, "msfe5_de", "msfe5_dd", "msfe5_upsampling", 1},
    {"msfe6_de", 6, 256, "msfe6_de", "msfe6_dd", "msfe6_upsampling", 0},
};

struct StateTensor {
  std::string name_prev, name_cur;
  int d0, d1;        // per-stream dims: (F, C) for conv states, (21, 1) for LSTM states, (d*F, k*G) for ring states
  float* buf[2];     // ping-pong, each [B, d0, d1]; ring / in-place states: buf[0] == buf[1]
  int ring_d = 0;    // > 0: dilated-dense history ring of ring_d frames (physical slot = (step + j) mod d)
  size_t per_stream() const { return static_cast<size_t>(d0) * d1; }
};

struct Launch {
  enum Kind { CONV, LSTM, CTFA, INLAYER, OUTCONV, DDB } kind;
  ConvKind ck;
  ConvParams conv;
  LstmParams lstm;
  CtfaParams ctfa;
  InLayerParams inl;
  OutConvParams outc;
  DdbParams ddb;
  int ddb_index = -1;
  std::string name;
  bool encoder_strided = false;   // one of the 26 encoder (2,3) stride-2 convs (the "encoder conv stack")
};

struct StageStates {
  std::vector<int> conv;    // state index of conv input i (1-based -> [i-1])
  std::vector<int> spconv;  // state index of sub-pixel conv input j
  int h, c;
};

struct ConvLayerW { float *wpk, *bias, *gamma, *beta; float alpha; float *wbf, *wscale; };
struct LstmW { float *wxT, *whT, *bias, *wdT, *bd; int din, dout; };
struct CtfaW { float *w1T, *b1, *w2T, *b2, *w2; };   // w2: [64][16] as stored, w2T: [16][64]

struct Engine {
  // ---- handle and arena ----------------------------------------------------------------------
  int B = 0, device = 0;
  int variant = 0;               // NUTLS_VARIANT_LSTM / NUTLS_VARIANT_BASELINE
  long long steps = 0;           // frames processed (ring position of the baseline's dilated-dense history)
  int next_parity = 0;   // parity the next step writes (`cur`); `prev` is read from 1 - next_parity
  int mode = 0;          // 0 plain per-layer launches, 1 per-layer hipGraph replay, 3 fused kernel (statically scheduled; both variants);
                         // (2 was the plan-interpreter kernel of rounds 1-3, retired)
  int n_cu = 256;
  hipStream_t stream = nullptr;
  // Stream order (nutls.h: calls on one handle take effect in the order they are made, whichever streams they name): the stream the last call
  // enqueued on -- a caller's, the NULL stream or `stream` above; the Engine's own address while there is none, or after a call that left
  // the device idle.  A call that names another stream waits for an event recorded on this one first: enqueue_on, below.
  hipStream_t last_stream = no_stream();
  hipEvent_t ev_order = nullptr;         // created by the first change of stream
  hipStream_t no_stream() const { return reinterpret_cast<hipStream_t>(const_cast<Engine*>(this)); }
  std::vector<void*> allocs;
  float* arena = nullptr;        // stream-major arena: stream b's tensors at arena + b*sstride + slot offset
  size_t sstride = 0;            // floats per stream
  size_t arena_cursor = 0;       // next free slot offset (floats) while the layout is being built
  std::vector<float**> arena_fixups;   // pointers that hold a slot offset until the arena is allocated
  std::vector<StateTensor> states;   // reserve()d up front: slot_reserve keeps pointers into it
  std::unordered_map<std::string, int> state_index;
  float *io_in = nullptr, *io_out = nullptr;
  std::unordered_map<std::string, std::pair<float*, size_t>> debug;   // name -> (ptr, floats per stream)
  // ---- per-layer plan and weights ------------------------------------------------------------
  float* warena = nullptr;       // all weights, one allocation
  size_t wcursor = 0;
  int* d_step = nullptr;         // the same counter on the device (read by the per-layer / plan-interpreter kernels)
  bool d_step_stale = false;     // fused-mode steps take `steps` by value and leave the device counter behind
  std::vector<DdbParams> ddbs;   // baseline: the 13 dilated-dense blocks (host copy, per parity identical)
  DdbParams* d_ddb = nullptr;
  struct DdbStates { int in, blk[6], out; };
  DdbStates ddb_st[13];
  struct DdbW { float *w_in, *b_in, *wg[6], *bg[6], *w1[6], *b1[6], *gamma[6], *beta[6], *w_out, *b_out, *wsmall; float a_in, a_out, alpha[6]; };
  DdbW ddbw[13];
  StageStates enc_st[6], dec_st[6];
  int central_h = -1, central_c = -1;
  std::vector<Launch> plan[2];
  float *t_inlayer = nullptr, *t_y = nullptr, *t_d = nullptr, *t_up = nullptr;
  float* upcat[6] = {nullptr};
  hipGraphExec_t gexec[2] = {nullptr, nullptr};
  std::unordered_map<std::string, ConvLayerW> convw;
  std::unordered_map<std::string, LstmW> lstmw;
  std::unordered_map<std::string, CtfaW> ctfaw;
  float *in_w = nullptr, *in_b = nullptr, *in_g = nullptr, *in_bt = nullptr, *out_w = nullptr;
  float in_alpha = 0.f, out_bias = 0.f;
  // ---- fused plan and coherence flags --------------------------------------------------------
  // carried partial sums of the fused kernel's two-tap convs (S = W[tap 0] x, fused_plan.hpp OpD::ys): two blocks in every stream's
  // arena slice; stale after the conv-input states were written from outside the fused kernel -- rebuilt before the next fused step
  float* ysum = nullptr;
  YsOp* d_ys_ops = nullptr;
  float* d_ys_w = nullptr;
  int n_ys_ops = 0;
  bool ys_dirty = false;
  // Lazily written states (fused_plan.hpp OpD::d0_on = 2: the input states of the strided convs, which the fused kernel never reads): a
  // fused step leaves them unwritten and marks them stale; whoever looks at states from outside the kernel -- nutls_state_get / _set /
  // _get_all, nutls_reset, a step of a per-layer mode, the rebuild of the carried sums -- goes through states_materialize first.
  LazyCopy* d_lazy = nullptr;
  int n_lazy = 0;
  bool eager_states = false, states_stale = false;
  float* fz_blob = nullptr;              // weight blob of the fused kernel (plan order)
  int fz_streams_req = 0;                // nutls_create_plan: the caller's choice of plan (0: the library's)
  const FusedPlan* fz_plan = nullptr;    // the fused plan this handle runs: the one-stream plan of its variant, or a packed plan (2 / 4 streams per workgroup: chosen by the cost model in fused_setup or by nutls_create_plan)
  // CTFA frequency branch of the fused kernel (nutls_internal.hpp FzTa): fz_ta_zero = 64 zeros + a dump row (frame mode); causal32 mode of a
  // streaming handle (nutls_set_ctfa_mode): history ring [B][12][32][64] and the per-step sums [B][12][64]
  float *fz_ta_zero = nullptr, *fz_ta_ring = nullptr, *fz_ta_sum = nullptr;
  float* fz_dbg_buf = nullptr;
  int fz_stop_at = -1;         // >= 0: fused launches run the stop twin and end in front of this op (nutls_profile_production)
  bool lazy_edited = false;    // nutls_state_set wrote a lazily written state and not every stream has stepped since: masked steps then write every state
                               // (a held stream's edited row must not be rebuilt from its older second copy: run_fused)
  std::vector<unsigned char> lazy_pending;   // while lazy_edited: per stream, 1 = has not stepped since the edit (followed through the HOST masks: note_active)
  int fz_skew = 0;             // FzTa::skew of the fused launches (start skew of the workgroups; experiment builds of the kernel: see nutls_debug_knob)
  float* fz_dbg = nullptr;     // activation trace [B][kDbgSlots][kDbgSlotFloats] (nutls_debug_trace): steps then run on the profiling build, which fills it
  std::string fz_reason;                 // why there is none (what the packer said), for nutls_set_mode(3)
  unsigned long long* fz_prof = nullptr; // op boundary stamps of workgroup 0 (profiling build)
  // ---- streaming front end -------------------------------------------------------------------
  // STFT front / back end (allocated on first use): previous hop, overlap tail, phasors, windows, twiddles, staging
  float *fe_tail = nullptr, *fe_ola = nullptr, *fe_ph = nullptr, *fe_win = nullptr, *fe_inv = nullptr, *fe_tw = nullptr;
  float *fe_pcm_in = nullptr, *fe_pcm_out = nullptr;
  float* fe_twb = nullptr;       // stft_block_twiddles(): the wave-level transform of the hop builds of the fused kernel
  bool hop_fusion = false;       // nutls_set_hop_fusion: the nutls_enhance_hop* entries run ONE launch (FusedPlan::launch_hop) instead of three
  unsigned char* d_active = nullptr;     // [B] bytes: device copy of the mask of the _host entries of nutls_step_active / nutls_enhance_hop_active
  // ---- offline block mode --------------------------------------------------------------------
  int offline = 0;       // > 0: offline / block handle for up to this many frames per call (arena slot 0 = carried state)
  int outt = 1;          // utterances of an offline handle (nutls_create_offline_batch): utterance u owns arena slots [u (offline + 1), (u + 1) (offline + 1)):
                         // its carried state, then its frames
  std::vector<Launch> plan_off;   // plan[0] with 'previous frame' = one arena slot earlier
  bool off_bf16 = false;          // block mode: convs on the bf16 matrix pipe where the container holds int8 kernels (NUTLS_OFFLINE_FP32=1: the fp32-MFMA kernels)
  ConvKnobs conv_knobs;           // developer knobs of the per-layer convs' choice of instantiation (NUTLS_OFFLINE_KSPLIT, NUTLS_CONV_TILE_MIN), read when the
                                  // handle is created like NUTLS_OFFLINE_FP32: every per-layer conv launch of this handle, block or streaming, is chosen under them
  float* zx = nullptr;   // [offline + kScanReadAhead][84] LSTM input products of a block
  int ctfa_causal = 0;   // offline handles: 1 = true 32-frame causal average in the CTFA frequency branch (proposed.py:143-147)
  float* ta_hist = nullptr;   // [12 stages][31 + offline][64] time-attention history (causal mode)
  // waveform block mode of an offline handle (stft_block.hip; allocated on first use): previous hop and overlap tail of every utterance [outt][256],
  // two buffers each -- a launch reads [par] and writes [1 - par] --, the phasors of the last analysed block [outt][fb_hops][257] float2, windows,
  // twiddles (stft_block_twiddles) and, for the host entry, PCM staging [outt][offline * 256]
  float *fb_tail[2] = {nullptr, nullptr}, *fb_ola[2] = {nullptr, nullptr}, *fb_ph = nullptr, *fb_win = nullptr, *fb_inv = nullptr, *fb_tw = nullptr;
  float *fb_pcm_in = nullptr, *fb_pcm_out = nullptr;
  int fb_tail_par = 0, fb_ola_par = 0, fb_hops = 0;
  // block pipeline of an offline handle: the block is cut into chunks of consecutive frames, chunk c runs on its own
  // HIP stream one bottleneck behind chunk c-1 (every layer is causal in time: frame t needs frames <= t only)
  static constexpr int kMaxChunks = 16, kGroups = 16;
  std::vector<hipStream_t> ostream;
  std::vector<hipEvent_t> oev;          // [chunk stream][2 * kGroups]: slot g = the chunk's conv-like launches of group g are enqueued, kGroups + g = its LSTM of group g
  hipEvent_t oev_fork = nullptr;
  int ochunks = 0;                      // 0 = chosen from the block length
  int* d_counts = nullptr;              // [outt] ints: device copy of the counts of the _host entries of the ragged block calls (nutls_process_block_ragged_host)
  std::vector<int> ogroup;              // launch index of plan_off -> group (a group ends with an LSTM)
  // ---- attenuation limit ----------------------------------------------------------------------
  // nutls_set_atten_limit: per row (stream / utterance) the limit l in force; a setting, not stream state -- no reset touches it.  d_atten [rows]
  // (l, c) pairs, allocated by the first set; atten_on = some row's l is not 0, and only then do the syntheses run their mix kernels.
  std::vector<float> atten;
  float* d_atten = nullptr;
  bool atten_on = false;
  // ---- PCM gateway ---------------------------------------------------------------------------
  PcmState pcm;          // the callers' sample rate and type (nutls_set_pcm_format) and the resampler histories of the _pcm entries
  PacketState pkt;       // packet mode (nutls_set_pcm_packet): the callers' packet length, the per-stream FIFOs and their counters
  ChannelState chn;      // channels (nutls_set_pcm_channels): the callers' frame layout and the two buffers the split and the join work between

  ~Engine() {
    for (int i = 0; i < 2; ++i)
      if (gexec[i]) (void)hipGraphExecDestroy(gexec[i]);
    for (void* p : allocs) (void)hipFree(p);
    for (hipEvent_t ev : oev) (void)hipEventDestroy(ev);
    if (oev_fork) (void)hipEventDestroy(oev_fork);
    if (ev_order) (void)hipEventDestroy(ev_order);
    for (hipStream_t st : ostream) (void)hipStreamDestroy(st);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// ---- engine.cpp ------------------------------------------------------------------------------
int dev_alloc(Engine* e, size_t floats, float** out, bool zero);

// A typed device array the handle owns, allocated on first use: nothing happens when *out is already there.
template <typename T>
int dev_alloc_once(Engine* e, size_t n, T** out, bool zero) {
  if (*out) return NUTLS_OK;
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, n * sizeof(T)));
  e->allocs.push_back(p);
  if (zero) HIP_TRY(hipMemset(p, 0, n * sizeof(T)));
  *out = static_cast<T*>(p);
  return NUTLS_OK;
}

// Before a call enqueues anything on stream s (the handle's device is current): on the stream of the call before it, a pointer compare and
// nothing else; on another one, one event recorded on the old stream and awaited on s (order_after_last), so that the call's work runs
// behind everything the handle has queued so far.  enqueue_idle: the call has synchronised with all of that -- there is nothing to wait for.
int order_after_last(Engine* e, hipStream_t s);
inline int enqueue_on(Engine* e, hipStream_t s) { return s == e->last_stream ? NUTLS_OK : order_after_last(e, s); }
inline void enqueue_idle(Engine* e) { e->last_stream = e->no_stream(); }

hipError_t run_launch(const Launch& L, hipStream_t s, const ConvKnobs& kn);
int run_plan(Engine* e, int par, hipStream_t s);
int states_materialize(Engine* e, hipStream_t s);
int run_fused(Engine* e, int par, hipStream_t s, bool prof, const float* mag_in = nullptr, float* mag_out = nullptr,
              const unsigned char* active = nullptr, const FzHop* hop = nullptr);
// frame bookkeeping: the only places that do these things (see their definitions)
void advance_frame(Engine* e);
int host_access_begin(Engine* e);
int begin_per_layer_step(Engine* e, hipStream_t s);
void frontend_tables(std::vector<float>* win_out, std::vector<float>* inv_out, std::vector<float>* tw_out);
int frontend_init(Engine* e);
// what this handle can do: each refuses with a message that starts with the entry's name `who`
int refuse_per_layer_in_causal32(const Engine* e, const char* who);
int refuse_in_hop_fusion(const Engine* e, const char* who);
int check_active(const Engine* e, const char* who);
int check_hop_fusion(const Engine* e, const char* who);

// ---- api_block.cpp ---------------------------------------------------------------------------
int build_offline_plan(Engine* e);
// The HOST counts of a ragged _host entry (`who`): checked -- one outside 0 .. n is NUTLS_ERR_ARG and nothing has been touched --, then copied
// to e->d_counts on the library's stream, in front of the work that reads them.
int upload_counts(Engine* e, const int* counts, int n, const char* who);

// ---- api_stream.cpp --------------------------------------------------------------------------
// After a masked step whose HOST mask `active` [B] the library has seen: the lazy_pending bookkeeping behind nutls_state_set (see there)
void note_active(Engine* e, const unsigned char* active);

// ---- api_pcm.cpp -----------------------------------------------------------------------------
// nutls_reset: zero the resampler histories and the upper-band state of row `idx` (stream / utterance; < 0: every row's) where they exist,
// and re-prime the row's packet FIFOs while packet mode is on
int pcm_reset(Engine* e, int idx);

}  // namespace nutls

struct nutls_handle {
  nutls::Engine eng;
};
