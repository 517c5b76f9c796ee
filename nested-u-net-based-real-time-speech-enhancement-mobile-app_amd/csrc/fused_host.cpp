// Host side of the fused frame-step kernel (fused_step.hip / fused_base.hip): the descriptor of every static plan (fused_host.hpp), the
// weight blob packed in the order of a plan, and the arena layout the plan addresses, which engine.cpp checks against its own.
#include <cstring>

#include "../../include/nutls.h"
#include "fused_host.hpp"
#include "fused_plan.hpp"

namespace nutls {
namespace {

const HostTensor* get(const WeightMap& w, const std::string& k, std::string* err) {
  auto it = w.find(k);
  if (it == w.end()) {
    if (err->empty()) *err = "weight tensor missing: " + k;
    return nullptr;
  }
  return &it->second;
}

// (fused_host_impl.inc: the generated tables of a plan file, whose element types are that plan's own, copied into the descriptor's)
template <class T, size_t N> std::vector<FusedBlobItem> copy_items(const T (&a)[N]) {
  std::vector<FusedBlobItem> v;
  for (const T& b : a) v.push_back(FusedBlobItem{b.off, b.floats, b.what, b.op, b.key});
  return v;
}
template <class T, size_t N> std::vector<FusedOff> copy_offs(const T (&a)[N]) {
  std::vector<FusedOff> v;
  for (const T& s : a) v.push_back(FusedOff{s.name, s.off});
  return v;
}

namespace lstm_plan {
namespace fz {
using namespace ::nutls::fz;
#include "fused_plan_lstm.inc"
}  // namespace fz
#include "fused_host_impl.inc"
}  // namespace lstm_plan

// packed plan of the LSTM variant: two streams per workgroup (fused_step_g2.hip)
namespace lstm_g2_plan {
namespace fz {
using namespace ::nutls::fz;
#include "fused_plan_lstm_g2.inc"
}  // namespace fz
#include "fused_host_impl.inc"
}  // namespace lstm_g2_plan

// ... and four (fused_step_g4.hip)
namespace lstm_g4_plan {
namespace fz {
using namespace ::nutls::fz;
#include "fused_plan_lstm_g4.inc"
}  // namespace fz
#include "fused_host_impl.inc"
}  // namespace lstm_g4_plan

namespace base_plan {
namespace fz {
using namespace ::nutls::fz;
#include "fused_plan_base.inc"
}  // namespace fz
#include "fused_host_impl.inc"
}  // namespace base_plan

// Output-channel order of a conv op: the sub-pixel shuffle (proposed.py:227-251) is folded into it, so that
// packed channel r * gc + c of position f IS out[2 f + r, c].
std::vector<int> channel_perm(const fz::OpD& d) {
  std::vector<int> p(d.N);
  for (int n = 0; n < d.N; ++n) p[n] = n;
  if (d.kind == fz::K_DL && d.N == 64)
    for (int r = 0; r < 2; ++r)
      for (int c = 0; c < 32; ++c) p[r * 32 + c] = 2 * c + r;
  if (d.kind == fz::K_DL && d.N == 128)
    for (int r = 0; r < 2; ++r)
      for (int c2 = 0; c2 < 64; ++c2) p[r * 64 + c2] = r * 64 + (c2 % 32) * 2 + c2 / 32;
  return p;
}

}  // namespace

// The only place that knows which plans exist, and which kernel runs which.
const FusedPlan* fused_plan(int variant, int streams) {
  if (variant == NUTLS_VARIANT_LSTM && streams == 1) return lstm_plan::describe(variant, launch_fused_step, fused_step_set_attributes, launch_fused_step_hop, fused_step_hop_set_attributes);
  if (variant == NUTLS_VARIANT_LSTM && streams == 2) return lstm_g2_plan::describe(variant, launch_fused_step_g2, fused_step_g2_set_attributes, launch_fused_step_g2_hop,
                                  fused_step_g2_hop_set_attributes);
  if (variant == NUTLS_VARIANT_LSTM && streams == 4) return lstm_g4_plan::describe(variant, launch_fused_step_g4, fused_step_g4_set_attributes);
  if (variant == NUTLS_VARIANT_BASELINE && streams == 1) return base_plan::describe(variant, launch_fused_base_step, fused_base_step_set_attributes);
  return nullptr;
}

// the state tensors a launch leaves unwritten unless it is asked for eager states (OpD::d0_on = 2): where their rows can be copied from
void fused_lazy_table(const FusedPlan& p, std::vector<LazyCopy>* tab) {
  tab->clear();
  for (int i = 0; i < p.num_ops; ++i) {
    const fz::OpD& d = p.ops[i];
    if (d.type == fz::T_CONV && d.d0_on == 2 && d.d1_on == 1 && d.d0_src == fz::S_CUR && d.d1_src == fz::S_CUR)
      tab->push_back(LazyCopy{d.d1_off, d.d1_ld, d.d0_off, d.d0_ld, d.P * d.R, d.gc});
    // (OpD::d1_on = 2: the second copy of an encoder sub-pixel conv's rows -- the skip half of the paired decoder conv's input state)
    if (d.type == fz::T_CONV && d.d1_on == 2 && d.d0_on == 1 && d.d0_src == fz::S_CUR && d.d1_src == fz::S_CUR)
      tab->push_back(LazyCopy{d.d0_off, d.d0_ld, d.d1_off, d.d1_ld, d.P * d.R, d.gc});
  }
}

// Two-tap convs: S = W[time tap 0] x is carried from frame to frame (fused_plan.hpp OpD::ys).  The table for the device-side
// rebuild of S from the conv-input state tensors: per op its shape and offsets, weights [packed channel][frequency tap][cin].
bool fused_ys_table(const FusedPlan& p, const WeightMap& wm, std::vector<YsOp>* ops, std::vector<float>* wq, std::string* err) {
  ops->clear();
  wq->clear();
  for (int i = 0; i < p.num_ops; ++i) {
    const fz::OpD& d = p.ops[i];
    if (d.type != fz::T_CONV || !d.ys || d.g0 != 0) continue;      // (packed plans: one entry per layer, not per instance)
    // (the conv's weight key: the blob item of its fragments)
    const char* key = nullptr;
    for (int it = 0; it < p.num_blob_items; ++it)
      if (p.blob_items[it].off == d.w_off && p.blob_items[it].what == 0) key = p.blob_items[it].key;
    if (!key) { *err = "no weight item for op " + std::string(p.op_names[i]); return false; }
    const HostTensor* w = get(wm, std::string(key) + ".w", err);
    if (!w) return false;
    if (w->q.size() != w->data.size() || w->dims.size() != 4 || w->dims[0] != d.N || w->dims[1] < 2 || w->dims[2] < 3 || w->dims[3] != d.cin) {
      *err = std::string(key) + ".w is not an int8 [N][2][3][cin] tensor";
      return false;
    }
    const std::vector<int> perm = channel_perm(d);
    YsOp o{};
    o.P = d.P; o.cin = d.cin; o.N = d.N; o.stride = d.kind == fz::K_EL ? 2 : 1;
    o.xs_off = d.xs_off; o.xs_ld = d.xs_ld; o.ys_off = d.ys_off; o.w_off = static_cast<int>(wq->size());
    o.r32 = d.path == fz::P_R32B ? 1 : 0; o.PT = d.PT; o.NT = d.NT; o.PG = d.PG;
    const int th = w->dims[1], kw = w->dims[2];
    for (int n = 0; n < d.N; ++n)
      for (int k = 0; k < 3; ++k)
        for (int c = 0; c < d.cin; ++c) wq->push_back(static_cast<float>(w->q[((static_cast<size_t>(perm[n]) * th + 0) * kw + k) * d.cin + c]));
    ops->push_back(o);
  }
  return true;
}

// Weight blob of the fused kernel, in plan order.  Returns FZ_PACK_OK, FZ_PACK_NOT_INT8 (a float container: no int8 payload to
// keep on the device) or FZ_PACK_MALFORMED (missing tensor, unexpected shape, ...); `err` says which tensor.  Conv kernels stay int8 (the container's payload, what the reference's
// .tflite stores; `w = q * scale[out channel]`, converter_proposed.py:901) and the kernel applies the scale in its epilogue.
//   conv fragments: for weight task for fragment f of the task (2 fragments = 16 bytes per lane) for lane for q = 0..7
//       fragment f -> K segment (time tap t, frequency tap kw), K step g, channel tile T  (same walk as fused_step.hip)
//       32x32x16 tiles: n' = 32 T + (lane & 31), c = 16 g + 8 (lane >> 5) + q
//       16x16x32 tiles: n' = 16 T + (lane & 15), c = 32 g + 8 (lane >> 4) + q      (T = ct NT + f % NT, K step f / NT)
//       byte = Q[perm[n']][t][kw][c]                        (OHWI weights, converter_proposed.py Conv2D kernels)
int fused_pack_blob(const FusedPlan& p, const WeightMap& wm, std::vector<float>* out, std::string* err) {
  out->assign(static_cast<size_t>(p.blob_floats), 0.f);
  err->clear();
  for (int it = 0; it < p.num_blob_items; ++it) {
    const FusedBlobItem& bi = p.blob_items[it];
    const fz::OpD& d = p.ops[bi.op];
    float* dst = out->data() + bi.off;
    const std::string key = bi.key;
    if (bi.what == 0) {
      const HostTensor* w = get(wm, key + ".w", err);
      if (!w) return FZ_PACK_MALFORMED;
      if (w->dims.size() != 4 || w->dims[0] != d.N || w->dims[3] != d.cin) { *err = "unexpected weight shape for " + key; return FZ_PACK_MALFORMED; }
      if (w->q.size() != w->data.size() || (w->scales.size() != 1 && static_cast<int>(w->scales.size()) != d.N)) {
        *err = "fused mode keeps conv weights int8 on the device; " + key + ".w is not an int8 tensor of the container";
        return FZ_PACK_NOT_INT8;
      }
      const int th = w->dims[1], kw = w->dims[2];
      const std::vector<int> perm = channel_perm(d);
      const bool r32 = d.path == fz::P_R32B;
      const int G = d.cin / (r32 ? 16 : 32), GW = G / d.KSg;
      // (two-tap convs on 32x32 tiles, d.ys: waves 0..3 walk the three segments of time tap 0, waves 4..7 those of tap 1)
      const bool r32two = r32 && d.ys != 0;
      const int segw = d.kind == fz::K_UP ? 3 : (r32two ? 3 : d.nseg / d.KSt);
      const int nf = segw * GW * d.NT, nsf = (nf + 1) / 2, wtasks = r32 ? (r32two ? 2 * d.CG : d.CG) : d.CG * d.KSt * d.KSg;
      if (wtasks * nsf * 256 != bi.floats) { *err = "fragment count mismatch for " + key; return FZ_PACK_MALFORMED; }
      int8_t* dst8 = reinterpret_cast<int8_t*>(dst);
      for (int task = 0; task < wtasks; ++task) {
        const int ct = task % d.CG, ks = task / d.CG, ks_g = ks % d.KSg, ks_t = ks / d.KSg;
        for (int f = 0; f < nf; ++f) {
          int sg, g, T;
          if (r32) {
            const int nt = f % d.NT, sgi = f / d.NT;
            sg = (r32two ? ks * 3 : 0) + sgi / G; g = sgi % G; T = ct * d.NT + nt;
          } else {
            // (K-split-first tilings: NT channel tiles per task, the tile index fastest; NT = 1 everywhere else)
            const int nt = f % d.NT, r = f / d.NT;
            sg = ks_t * segw + r / GW; g = ks_g * GW + r % GW; T = ct * d.NT + nt;
          }
          const int t = p.seg_tk[bi.op][sg] >> 2, k = p.seg_tk[bi.op][sg] & 3;
          if (sg >= d.nseg || t >= th || k >= kw) { *err = "segment outside the kernel of " + key; return FZ_PACK_MALFORMED; }
          for (int lane = 0; lane < 64; ++lane)
            for (int q = 0; q < 8; ++q) {
              const int np = r32 ? 32 * T + (lane & 31) : 16 * T + (lane & 15);
              const int c = r32 ? 16 * g + 8 * (lane >> 5) + q : 32 * g + 8 * (lane >> 4) + q;
              dst8[((static_cast<size_t>(task) * nsf + f / 2) * 64 + lane) * 16 + (f % 2) * 8 + q] =
                  w->q[((static_cast<size_t>(perm[np]) * th + t) * kw + k) * d.cin + c];
            }
        }
      }
    } else if (bi.what == 1) {
      // bias | per-channel weight scale | gamma | beta | alpha   (packed channel order)
      const HostTensor* b = get(wm, key + ".b", err);
      const HostTensor* w = get(wm, key + ".w", err);
      if (!b || !w) return FZ_PACK_MALFORMED;
      if (static_cast<int>(b->size()) != d.N) { *err = "unexpected bias size for " + key; return FZ_PACK_MALFORMED; }
      if (w->scales.size() != 1 && static_cast<int>(w->scales.size()) != d.N) { *err = "unexpected scale count for " + key; return FZ_PACK_MALFORMED; }
      const std::vector<int> perm = channel_perm(d);
      const int reps = d.kind == fz::K_UP ? 2 : 1;         // the up-sampling layer's parameters apply to even and odd output rows
      const int nt = reps * d.N;
      for (int r = 0; r < reps; ++r)
        for (int n = 0; n < d.N; ++n) {
          dst[r * d.N + n] = b->data[perm[n]];
          dst[nt + r * d.N + n] = w->scales.size() == 1 ? w->scales[0] : w->scales[perm[n]];
        }
      if (d.ln) {
        const HostTensor* g = get(wm, key + ".gamma", err);
        const HostTensor* bt = get(wm, key + ".beta", err);
        const HostTensor* al = get(wm, key + ".alpha", err);
        if (!g || !bt || !al) return FZ_PACK_MALFORMED;
        if (static_cast<int>(g->size()) != d.gc || static_cast<int>(bt->size()) != d.gc || al->size() < 1) { *err = "unexpected LayerNorm / PReLU size for " + key; return FZ_PACK_MALFORMED; }
        std::memcpy(dst + 2 * nt, g->data.data(), d.gc * sizeof(float));
        std::memcpy(dst + 2 * nt + d.gc, bt->data.data(), d.gc * sizeof(float));
        dst[2 * nt + 2 * d.gc] = al->data[0];
      }
    } else if (bi.what == 2) {
      const std::string ln = key.empty() ? "lstm" : key + "_lstm", dn = key.empty() ? "dense" : key + "_dense";
      const HostTensor* wx = get(wm, ln + ".wx", err);
      const HostTensor* wh = get(wm, ln + ".wh", err);
      const HostTensor* b = get(wm, ln + ".b", err);
      const HostTensor* wd = get(wm, dn + ".w", err);
      const HostTensor* bd = get(wm, dn + ".b", err);
      if (!wx || !wh || !b || !wd || !bd) return FZ_PACK_MALFORMED;
      const int din = d.din, dout = d.dout;
      if (wx->dims.size() != 2 || wx->dims[0] != 84 || wx->dims[1] != din || wh->size() != 84u * 21u || b->size() != 84u ||
          wd->dims.size() != 2 || wd->dims[0] != dout || wd->dims[1] != 21 || static_cast<int>(bd->size()) != dout) {
        *err = "unexpected LSTM / Dense shape for " + ln;
        return FZ_PACK_MALFORMED;
      }
      // Blob layout of an LSTM + Dense op (fused_plan.hpp): the int8 gate kernels as the container stores them (FULLY_CONNECTED, one scale per
      // tensor; z = b + s_x (Qx x) + s_h (Qh h)), [K slice][unit][row] with the four gates of a unit in one dword
      if (wx->q.size() != wx->data.size() || wh->q.size() != wh->data.size() || wx->scales.size() != 1 || wh->scales.size() != 1) {
        *err = "fused mode keeps the LSTM kernels int8 on the device; " + ln + ".wx / .wh are not int8 tensors with one scale each";
        return FZ_PACK_NOT_INT8;
      }
      if (fz::lstm_blob_f(din, dout) != bi.floats) { *err = "blob size mismatch for " + ln; return FZ_PACK_MALFORMED; }
      const int KN = fz::lstm_kn(din), NRP = fz::lstm_nrp(din);
      int8_t* g8 = reinterpret_cast<int8_t*>(dst);      // (the region is zeroed: padding rows stay 0)
      for (int sl = 0; sl < 20; ++sl)
        for (int u = 0; u < 21; ++u)
          for (int j = 0; j < (sl < 16 ? KN : 6); ++j)
            for (int g = 0; g < 4; ++g) {      // Keras gate order i, f, g, o: column g * 21 + u (converter_proposed.py LSTM cell)
              int8_t q = 0;
              if (sl < 16) q = wx->q[static_cast<size_t>(g * 21 + u) * din + sl * KN + j];
              else if (6 * (sl - 16) + j < 21) q = wh->q[static_cast<size_t>(g * 21 + u) * 21 + 6 * (sl - 16) + j];
              g8[(static_cast<size_t>(sl * 21 + u) * NRP + j) * 4 + g] = q;
            }
      float* rec = dst + fz::lstm_gates_f(din);
      for (int u = 0; u < 21; ++u)
        for (int g = 0; g < 4; ++g) rec[4 * u + g] = b->data[g * 21 + u];
      rec[84] = wx->scales[0];
      rec[85] = wh->scales[0];
      float* wdr = rec + fz::lstm_rec_f();
      if (fz::lstm_dense_i8(dout)) {
        // Dense rows: 24 int8 (21 weights) | fp32 bias | fp32 scale
        if (wd->q.size() != wd->data.size() || wd->scales.size() != 1) {
          *err = "fused mode keeps the Dense kernels with >= 64 outputs int8 on the device; " + dn + ".w is not an int8 tensor with one scale";
          return FZ_PACK_NOT_INT8;
        }
        for (int n = 0; n < dout; ++n) {
          int8_t* r8 = reinterpret_cast<int8_t*>(wdr + n * 8);
          for (int u = 0; u < 21; ++u) r8[u] = wd->q[static_cast<size_t>(n) * 21 + u];
          wdr[n * 8 + 6] = bd->data[n];
          wdr[n * 8 + 7] = wd->scales[0];
        }
      } else {
        // (the 32 x 21 Dense kernels: fp32 in the reference's .tflite -- fewer than 1024 elements; an int8 one is de-quantised, w = q * scale)
        for (int n = 0; n < dout; ++n) {
          for (int u = 0; u < 21; ++u) wdr[n * 24 + u] = wd->data[static_cast<size_t>(n) * 21 + u];
          wdr[n * 24 + 21] = bd->data[n];
        }
      }
    } else if (bi.what == 3) {
      int o = 0;
      for (const char* br : {"_ta", "_fa"}) {
        const HostTensor* w1 = get(wm, key + br + ".w1", err);
        const HostTensor* b1 = get(wm, key + br + ".b1", err);
        const HostTensor* w2 = get(wm, key + br + ".w2", err);
        const HostTensor* b2 = get(wm, key + br + ".b2", err);
        if (!w1 || !b1 || !w2 || !b2) return FZ_PACK_MALFORMED;
        if (w1->size() != 16u * 64u || w2->size() != 64u * 16u || b1->size() != 16u || b2->size() != 64u) { *err = "unexpected CTFA shape " + key + br; return FZ_PACK_MALFORMED; }
        // first layer, lane-major: lane (u = lane & 15, q = lane >> 4) keeps w1[u][16 q + i], i = 0..15 (fused_step.hip gate_mlp)
        for (int lane = 0; lane < 64; ++lane)
          for (int i = 0; i < 16; ++i) dst[o + lane * 16 + i] = w1->data[static_cast<size_t>(lane & 15) * 64 + 16 * (lane >> 4) + i];
        std::memcpy(dst + o + 1024, b1->data.data(), 16 * sizeof(float));
        std::memcpy(dst + o + 1040, w2->data.data(), 1024 * sizeof(float));                                // w2 [64][16] as stored
        std::memcpy(dst + o + 2064, b2->data.data(), 64 * sizeof(float));
        o += 2128;
      }
      const HostTensor* ow = get(wm, "out_conv.w", err);
      const HostTensor* ob = get(wm, "out_conv.b", err);
      if (!ow || !ob) return FZ_PACK_MALFORMED;
      if (ow->size() != 64u || ob->size() < 1) { *err = "unexpected output conv shape"; return FZ_PACK_MALFORMED; }
      std::memcpy(dst + 4256, ow->data.data(), 64 * sizeof(float));
      dst[4320] = ob->data[0];
    } else {
      const HostTensor* iw = get(wm, "input_layer.w", err);
      const HostTensor* ib = get(wm, "input_layer.b", err);
      const HostTensor* ig = get(wm, "input_layer.gamma", err);
      const HostTensor* ibt = get(wm, "input_layer.beta", err);
      const HostTensor* ia = get(wm, "input_layer.alpha", err);
      if (!iw || !ib || !ig || !ibt || !ia) return FZ_PACK_MALFORMED;
      if (iw->size() != 64u || ib->size() != 64u || ig->size() != 64u || ibt->size() != 64u || ia->size() < 1) { *err = "unexpected input layer shape"; return FZ_PACK_MALFORMED; }
      std::memcpy(dst, iw->data.data(), 256);
      std::memcpy(dst + 64, ib->data.data(), 256);
      std::memcpy(dst + 128, ig->data.data(), 256);
      std::memcpy(dst + 192, ibt->data.data(), 256);
      dst[256] = ia->data[0];
    }
  }
  return FZ_PACK_OK;
}

}  // namespace nutls
