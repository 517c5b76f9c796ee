// Profiling and debug entry points of the C ABI (include/nutls.h): the debug knobs and the activation trace, what a per-layer launch is
// and costs, per-launch / per-op timings of a step, and the host-only questions about the fused plans (op tables, weight blobs).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>

#include "engine.hpp"

using namespace nutls;

extern "C" {

int nutls_debug_knob(nutls_handle* h, const char* name, int value) {
  if (!h || !name) return fail(NUTLS_ERR_ARG, "nutls_debug_knob: null pointer");
  Engine* e = &h->eng;
  if (std::strcmp(name, "skew") == 0) { e->fz_skew = value; return NUTLS_OK; }
  return fail(NUTLS_ERR_ARG, std::string("nutls_debug_knob: unknown knob ") + name);
}

int nutls_debug_trace(nutls_handle* h, int enable) {
  if (!h) return fail(NUTLS_ERR_ARG, "nutls_debug_trace: null handle");
  Engine* e = &h->eng;
  if (!enable) { e->fz_dbg = nullptr; return NUTLS_OK; }      // (the buffer stays allocated with the handle)
  if (int rc = refuse_in_hop_fusion(e, "nutls_debug_trace")) return rc;      // (the trace is the profiling build's; the hop builds have none)
  if (e->offline || !e->fz_blob) return fail(NUTLS_ERR_ARG, "nutls_debug_trace: the activation trace is the fused kernel's (streaming handle, int8 container)");
  if (e->fz_plan->streams != 1) return fail(NUTLS_ERR_ARG, "nutls_debug_trace: the packed plans have no profiling build in the library (nutls_create_plan(..., 1) for the one-stream plan)");
  if (e->B > 64) return fail(NUTLS_ERR_ARG, "nutls_debug_trace: at most 64 streams (2.5 MB of trace per stream)");
  HIP_TRY(hipSetDevice(e->device));
  if (!e->fz_dbg_buf) {
    int rc = dev_alloc(e, static_cast<size_t>(e->B) * kDbgSlots * kDbgSlotFloats, &e->fz_dbg_buf, true);
    if (rc) return rc;
  }
  e->fz_dbg = e->fz_dbg_buf;
  return NUTLS_OK;
}

static const char* family_name(const Launch& L, int B, const ConvKnobs& kn) {
  static const char* conv_names[CONV_KIND_COUNT] = {"conv_el_c32", "conv_el_c64", "conv_el_c128", "conv_dl_n64", "conv_dl_n128",
                                                    "conv_in_c64", "conv_in_c128", "conv_down", "conv_up_even", "conv_up_odd"};
  static std::string tmp[2 * CONV_KIND_COUNT];
  switch (L.kind) {
    case Launch::CONV: {
      const int nw = conv_choose(L.ck, B, L.conv.F_out, false, kn).nw;
      std::string& t = tmp[2 * L.ck + (nw == 4)];
      t = std::string(conv_names[L.ck]) + (nw == 4 ? "/w4" : "/w1");
      return t.c_str();
    }
    case Launch::LSTM: return "lstm_dense";
    case Launch::CTFA: return "ctfa";
    case Launch::INLAYER: return "input_layer";
    case Launch::OUTCONV: return "out_conv";
    case Launch::DDB: return "dilated_dense";
  }
  return "?";
}

int nutls_launch_info(nutls_handle* h, int index, const char** layer, const char** family, double* flops, double* bytes) {
  if (!h || index < 0 || index >= static_cast<int>(h->eng.plan[0].size())) return fail(NUTLS_ERR_ARG, "nutls_launch_info: bad index");
  const Engine* e = &h->eng;
  const Launch& L = e->plan[0][index];
  const double B = e->B;
  double fl = 0, by = 0;
  switch (L.kind) {
    case Launch::CONV: {
      const ConvShape sh = conv_shape(L.ck);
      const double k = static_cast<double>(sh.tt) * sh.kf * sh.cin, n = 32.0 * sh.nt;
      fl = 2.0 * B * L.conv.F_out * k * n;
      by = 4.0 * B * (static_cast<double>(sh.tt) * L.conv.F_in * sh.cin + L.conv.F_out * n);
      break;
    }
    case Launch::LSTM:
      fl = 2.0 * B * (84.0 * (L.lstm.Din + 21) + 21.0 * L.lstm.Dout);
      by = 4.0 * B * (L.lstm.Din + L.lstm.Dout + 4 * 21);
      break;
    case Launch::CTFA:
      fl = B * (3.0 * L.ctfa.F * 64 + 2.0 * 4 * 64 * 16);
      by = 4.0 * B * 3 * L.ctfa.F * 64;
      break;
    case Launch::INLAYER:
      fl = 2.0 * L.inl.n_pos * 64;
      by = 4.0 * L.inl.n_pos * 65;
      break;
    case Launch::OUTCONV:
      fl = 2.0 * L.outc.n_pos * 64;
      by = 4.0 * L.outc.n_pos * 65;
      break;
    case Launch::DDB: {
      const double F = L.ddb.F, C = L.ddb.C, G = C / 2;
      double mac = 2 * 6.0 * C * G * F;                               // in + out convs
      for (int k = 1; k <= 6; ++k) mac += F * G * (6.0 * k + G);       // grouped dilated conv + 1x1
      fl = 2.0 * B * mac;
      by = 4.0 * B * F * (2 * C + 2 * 321.0 * G);                     // history read + written once per step
      break;
    }
  }
  if (layer) *layer = L.name.c_str();
  if (family) *family = family_name(L, e->B, e->conv_knobs);
  if (flops) *flops = fl;
  if (bytes) *bytes = by;
  return NUTLS_OK;
}

int nutls_launch_conv_shape(nutls_handle* h, int index, int* kind, int* f_out) {
  if (!h || !kind || !f_out || index < 0 || index >= static_cast<int>(h->eng.plan[0].size())) return fail(NUTLS_ERR_ARG, "nutls_launch_conv_shape: null pointer or bad index");
  const Launch& L = h->eng.plan[0][index];
  const bool conv = L.kind == Launch::CONV;
  *kind = conv ? static_cast<int>(L.ck) : -1;
  *f_out = conv ? L.conv.F_out : 0;
  return NUTLS_OK;
}

int nutls_conv_dispatch(int kind, int batch, int f_out, int bf16, int ksplit, long long tile_min, int* nw, int* all, int* tile, long long* grid, long long* lds_bytes) {
  if (kind < 0 || kind >= CONV_KIND_COUNT) return fail(NUTLS_ERR_ARG, "nutls_conv_dispatch: unknown conv kind");
  if (batch < 1 || f_out < 1 || (f_out & (f_out - 1))) return fail(NUTLS_ERR_ARG, "nutls_conv_dispatch: batch must be >= 1 and f_out a power of two");
  ConvKnobs kn;
  kn.ksplit = ksplit != 0;
  kn.tile_min = tile_min;
  const ConvChoice c = conv_choose(static_cast<ConvKind>(kind), batch, f_out, bf16 != 0, kn);
  if (nw) *nw = c.nw;
  if (all) *all = c.all;
  if (tile) *tile = c.tile;
  if (grid) *grid = c.grid;
  if (lds_bytes) *lds_bytes = static_cast<long long>(c.lds);
  return NUTLS_OK;
}

int nutls_profile_step(nutls_handle* h, float* ms, int n) {
  if (!h || !ms) return fail(NUTLS_ERR_ARG, "nutls_profile_step: null pointer");
  Engine* e = &h->eng;
  const int par = e->next_parity;
  const std::vector<Launch>& plan = e->plan[par];
  if (n != static_cast<int>(plan.size())) return fail(NUTLS_ERR_ARG, "nutls_profile_step: n must equal nutls_launches_per_step");
  if (int rc = refuse_in_hop_fusion(e, "nutls_profile_step")) return rc;
  if (int rc = refuse_per_layer_in_causal32(e, "nutls_profile_step")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  std::vector<hipEvent_t> ev(plan.size() + 1);
  for (auto& x : ev) HIP_TRY(hipEventCreate(&x));
  if (int rc = enqueue_on(e, e->stream)) return rc;
  if (int rc = begin_per_layer_step(e, e->stream)) return rc;
  HIP_TRY(hipEventRecord(ev[0], e->stream));
  for (size_t i = 0; i < plan.size(); ++i) {
    HIP_TRY(run_launch(plan[i], e->stream, e->conv_knobs));
    HIP_TRY(hipEventRecord(ev[i + 1], e->stream));
  }
  if (e->variant == NUTLS_VARIANT_BASELINE) HIP_TRY(launch_incr_step(e->d_step, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t i = 0; i < plan.size(); ++i) HIP_TRY(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
  for (auto& x : ev) (void)hipEventDestroy(x);
  advance_frame(e);
  return NUTLS_OK;
}

int nutls_fused_num_ops(int variant) { return nutls_fused_plan_num_ops(variant, 1); }

int nutls_fused_blob_floats(int variant) { return nutls_fused_plan_blob_floats(variant, 1); }

/* Host-only (no GPU needed): the weight blob of the fused kernel for a container, for tests of the packing. */
int nutls_fused_pack_blob(const void* weights, size_t n_bytes, int variant, float* out, size_t n_floats) {
  return nutls_fused_pack_blob_plan(weights, n_bytes, variant, 1, out, n_floats);
}

int nutls_fused_plan_num_ops(int variant, int streams) {
  const FusedPlan* p = fused_plan(variant, streams);
  return p ? p->num_ops : 0;
}

int nutls_fused_plan_op_info(int variant, int streams, int index, const char** name, double* flops) {
  const FusedPlan* p = fused_plan(variant, streams);
  if (!p) return fail(NUTLS_ERR_ARG, "nutls_fused_plan_op_info: no such plan");
  if (index < 0 || index >= p->num_ops) return fail(NUTLS_ERR_ARG, "nutls_fused_plan_op_info: bad index");
  if (name) *name = p->op_names[index];
  if (flops) *flops = p->op_flops[index];
  return NUTLS_OK;
}

int nutls_fused_plan_blob_floats(int variant, int streams) {
  const FusedPlan* p = fused_plan(variant, streams);
  return p ? p->blob_floats : 0;
}

int nutls_fused_pack_blob_plan(const void* weights, size_t n_bytes, int variant, int streams, float* out, size_t n_floats) {
  if (!weights || !out) return fail(NUTLS_ERR_ARG, "nutls_fused_pack_blob: null pointer");
  if (!fused_plan(variant, 1)) return fail(NUTLS_ERR_ARG, "nutls_fused_pack_blob: unknown variant");
  const FusedPlan* p = fused_plan(variant, streams);
  if (!p) return fail(NUTLS_ERR_ARG, "nutls_fused_pack_blob: no plan for that many streams per workgroup");
  if (n_floats != static_cast<size_t>(p->blob_floats)) return fail(NUTLS_ERR_ARG, "nutls_fused_pack_blob: n_floats must equal nutls_fused_blob_floats()");
  WeightMap wm;
  std::string err;
  std::vector<float> blob;
  try {
    if (!parse_weight_blob(weights, n_bytes, &wm, &err)) return fail(NUTLS_ERR_WEIGHTS, err);
    if (fused_pack_blob(*p, wm, &blob, &err) != FZ_PACK_OK) return fail(NUTLS_ERR_WEIGHTS, err);
  } catch (const std::exception& ex) {
    return fail(NUTLS_ERR_WEIGHTS, std::string("weight container: ") + ex.what());
  }
  std::memcpy(out, blob.data(), blob.size() * sizeof(float));
  return NUTLS_OK;
}

int nutls_fused_op_info(int variant, int index, const char** name, double* flops) {
  const FusedPlan* p = fused_plan(variant, 1);
  if (!p) return fail(NUTLS_ERR_ARG, "nutls_fused_op_info: unknown variant");
  if (index < 0 || index >= p->num_ops) return fail(NUTLS_ERR_ARG, "nutls_fused_op_info: bad index");
  if (name) *name = p->op_names[index];
  if (flops) *flops = p->op_flops[index];
  return NUTLS_OK;
}

int nutls_profile_production(nutls_handle* h, double* cum_us, int n, int reps, int steps) {
  if (!h || !cum_us) return fail(NUTLS_ERR_ARG, "nutls_profile_production: null pointer");
  Engine* e = &h->eng;
  if (e->offline || e->mode != 3 || !e->fz_blob || e->variant != NUTLS_VARIANT_LSTM || e->fz_plan->streams != 1 || e->ctfa_causal)
    return fail(NUTLS_ERR_ARG, "nutls_profile_production: a streaming handle of the LSTM variant in the fused mode on the one-stream plan, per-frame CTFA "
                               "(the stop twin exists for that kernel only)");
  if (int rc = refuse_in_hop_fusion(e, "nutls_profile_production")) return rc;
  const int nops = e->fz_plan->num_ops;
  if (n != nops + 1) return fail(NUTLS_ERR_ARG, "nutls_profile_production: n must equal nutls_fused_num_ops(variant) + 1");
  if (reps < 1 || steps < 1) return fail(NUTLS_ERR_ARG, "nutls_profile_production: reps and steps must be positive");
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = enqueue_on(e, e->stream)) return rc;
  HIP_TRY(fused_step_stop_set_attributes());
  hipEvent_t ev[2];
  HIP_TRY(hipEventCreate(&ev[0]));
  HIP_TRY(hipEventCreate(&ev[1]));
  int rc = NUTLS_OK;
  const int stop_before = e->fz_stop_at;      // (NUTLS_FUSED_STOP_TWIN handles keep running the twin afterwards)
  auto run = [&](int stop, int count) {
    e->fz_stop_at = stop;
    for (int i = 0; i < count && !rc; ++i) {
      rc = run_fused(e, e->next_parity, e->stream, false);
      advance_frame(e);
    }
  };
  run(nops, 300);      // (clocks; op index nops is never reached: the whole step)
  for (int stop = 0; stop <= nops && !rc; ++stop) {
    double best = 1e30;
    run(stop, 8);
    for (int r = 0; r < reps && !rc; ++r) {
      if (hipEventRecord(ev[0], e->stream) != hipSuccess) { rc = fail(NUTLS_ERR_HIP, "nutls_profile_production: hipEventRecord"); break; }
      run(stop, steps);
      float ms = 0.f;
      if (rc || hipEventRecord(ev[1], e->stream) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess ||
          hipEventElapsedTime(&ms, ev[0], ev[1]) != hipSuccess) { if (!rc) rc = fail(NUTLS_ERR_HIP, "nutls_profile_production: event timing"); break; }
      best = std::min(best, 1e3 * static_cast<double>(ms) / steps);
    }
    cum_us[stop] = best;
  }
  e->fz_stop_at = stop_before;
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  if (rc) return rc;
  return nutls_reset(h, -1);      // (the truncated launches left every stream's state between two frames)
}

int nutls_profile_fused(nutls_handle* h, double* us, int n) {
  if (!h || !us) return fail(NUTLS_ERR_ARG, "nutls_profile_fused: null pointer");
  Engine* e = &h->eng;
  if (n != e->fz_plan->num_ops)
    return fail(NUTLS_ERR_ARG, "nutls_profile_fused: n must equal nutls_fused_plan_num_ops(variant, nutls_streams_per_workgroup(h))");
  if (int rc = refuse_in_hop_fusion(e, "nutls_profile_fused")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = enqueue_on(e, e->stream)) return rc;
  const int par = e->next_parity;
  int rc = run_fused(e, par, e->stream, true);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::vector<unsigned long long> t(n + 1);
  HIP_TRY(hipMemcpy(t.data(), e->fz_prof, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  int khz = 100000;
  (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, e->device);
  if (khz <= 0) khz = 100000;
  for (int i = 0; i < n; ++i) us[i] = static_cast<double>(t[i + 1] - t[i]) * 1000.0 / khz;
  advance_frame(e);
  if (const char* wt = getenv("NUTLS_FUSED_WTRACE")) {       // debugging aid: the raw per-wave trace [8 waves][ops][12] of an FZ_WTRACE build (zeros otherwise)
    std::vector<unsigned long long> tr(static_cast<size_t>(n) * 8 * 12);
    HIP_TRY(hipMemcpy(tr.data(), e->fz_prof + static_cast<size_t>(n) * 9 + 1, tr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(wt, "wb")) {
      fwrite(tr.data(), sizeof(unsigned long long), tr.size(), f);
      fclose(f);
    }
  }
  if (const char* dump = getenv("NUTLS_FUSED_PHASES")) {     // debugging aid: phase stamps of every conv op (wave 0 of workgroup 0)
    std::vector<unsigned long long> sub(static_cast<size_t>(n) * 8);
    HIP_TRY(hipMemcpy(sub.data(), e->fz_prof + n + 1, sub.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(dump, "w")) {
      for (int i = 0; i < n; ++i) {
        fprintf(f, "%-24s total %6.2f |", e->fz_plan->op_names[i], us[i]);
        // stamp slots in chronological order: 0 loads issued, 5 carried weights arrived, 6 MFMA loop done (4x4 path),
        // 1 partials / parameters written, 2 past barrier 1, 3 epilogue done, 4 next image built
        const int order[7] = {0, 5, 6, 1, 2, 3, 4};
        const char* nm_conv[7] = {"issue", "wwait", "mloop", "mfma", "bar1", "epi", "build"};
        // CTFA ops: loads issued | column sums | barrier | time-attention perceptron | frequency-attention perceptron + gate | barrier; the rest (bar2) = gate applied
        const char* nm_ctfa[7] = {"issue", "colsum", "-", "bar1", "mlp_ta", "mlp_fa", "barg"};
        const char* opn = e->fz_plan->op_names[i];
        const size_t ol = std::strlen(opn);
        const char* const* nm = (ol >= 4 && std::strcmp(opn + ol - 4, "ctfa") == 0) ? nm_ctfa : nm_conv;
        unsigned long long prev = t[i];
        for (int k = 0; k < 7; ++k) {
          const unsigned long long v = sub[8 * i + order[k]];
          if (v >= prev && v <= t[i + 1]) { fprintf(f, " %s %5.2f", nm[k], static_cast<double>(v - prev) * 1000.0 / khz); prev = v; }
        }
        fprintf(f, " bar2 %5.2f\n", static_cast<double>(t[i + 1] - prev) * 1000.0 / khz);
      }
      fclose(f);
    }
  }
  return NUTLS_OK;
}

}  // extern "C"
