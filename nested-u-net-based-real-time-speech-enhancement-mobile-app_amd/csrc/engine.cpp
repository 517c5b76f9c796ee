// Host engine behind the C ABI of include/nutls.h: weight upload, HBM-resident recurrent state
// (ping-pong: the `cur` tensors of frame t are the `prev` tensors of frame t+1, no copy), the
// per-frame launch plan that wires the kernels of kernels.hip exactly like
// TFL_SIGNITURE.nutls_lstm (/root/reference/dnn_model/converter_proposed.py:188-867), and
// optional hipGraph capture of that plan; the fused plan's set-up and the coherence of what the fused kernel
// leaves to the host; handle creation and the handle-wide switches.  The other entry points of the ABI live in
// api_stream.cpp, api_block.cpp, api_state.cpp and api_profile.cpp; engine.hpp is what the five files share.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <new>

#include "engine.hpp"

namespace nutls {

static thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

static int decoder_of_encoder(int enc) { return 5 - enc; }

// ------------------------------------------------------------------------------- helpers ------
static int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

int dev_alloc(Engine* e, size_t floats, float** out, bool zero) {
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, floats * sizeof(float)));
  e->allocs.push_back(p);
  if (zero) HIP_TRY(hipMemset(p, 0, floats * sizeof(float)));
  *out = static_cast<float*>(p);
  return NUTLS_OK;
}

// Reserves `floats` per stream inside the stream-major arena; *out temporarily holds the slot offset
// (as a fake pointer) and is patched to the stream-0 address by arena_commit().
static void slot_reserve(Engine* e, size_t floats, float** out) {
  const size_t off = e->arena_cursor;
  e->arena_cursor += (floats + 63) & ~static_cast<size_t>(63);     // 256-byte aligned slots
  *out = reinterpret_cast<float*>(off * sizeof(float));
  e->arena_fixups.push_back(out);
}

static int arena_commit(Engine* e) {
  // Stream stride = an ODD number of 256-byte lines: at any moment all workgroups touch the same
  // slot offset of their own stream, so a power-of-two-ish stride would line every CU up on the
  // same HBM channel / L2 slice.
  e->sstride = (e->arena_cursor + 63) & ~static_cast<size_t>(63);
  if (const char* sk = getenv("NUTLS_STRIDE_ALIGN")) { const size_t a = static_cast<size_t>(atol(sk)); e->sstride = (e->arena_cursor + a - 1) / a * a; }
  else if (((e->sstride / 64) & 1) == 0) e->sstride += 64;
  void* p = nullptr;
  const size_t bytes = e->sstride * sizeof(float) * e->B;
  HIP_TRY(hipMalloc(&p, bytes));
  e->allocs.push_back(p);
  HIP_TRY(hipMemset(p, 0, bytes));
  e->arena = static_cast<float*>(p);
  for (float** f : e->arena_fixups) *f = e->arena + reinterpret_cast<size_t>(*f) / sizeof(float);
  e->arena_fixups.clear();
  for (StateTensor& st : e->states)
    if (st.ring_d > 0) st.buf[1] = st.buf[0];
  return NUTLS_OK;
}

// All weights live in ONE device allocation (bump-allocated, 256-byte aligned pieces) so the
// persistent kernel can address them with 32-bit offsets from a single base.
static constexpr size_t kWeightArenaFloats = 8u << 20;   // 32 MiB: 11.5 MB of parameters + packing padding

static int upload(Engine* e, const std::vector<float>& v, float** out) {
  if (!e->warena) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, kWeightArenaFloats * sizeof(float)));
    e->allocs.push_back(p);
    HIP_TRY(hipMemset(p, 0, kWeightArenaFloats * sizeof(float)));
    e->warena = static_cast<float*>(p);
  }
  const size_t n = (v.size() + 63) & ~static_cast<size_t>(63);
  if (e->wcursor + n > kWeightArenaFloats) return fail(NUTLS_ERR_WEIGHTS, "weight arena exhausted");
  *out = e->warena + e->wcursor;
  e->wcursor += n;
  HIP_TRY(hipMemcpy(*out, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  return NUTLS_OK;
}

static const HostTensor* find(const WeightMap& w, const std::string& k, std::string* err) {
  auto it = w.find(k);
  if (it == w.end()) {
    *err = "weight tensor missing: " + k;
    return nullptr;
  }
  return &it->second;
}

static std::vector<float> transpose2d(const HostTensor& t, int rows, int cols) {  // [rows][cols] -> [cols][rows]
  std::vector<float> o(static_cast<size_t>(rows) * cols);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) o[static_cast<size_t>(c) * rows + r] = t.data[static_cast<size_t>(r) * cols + c];
  return o;
}

// Uploads one conv-like layer in MFMA streaming order.
static int prep_conv(Engine* e, const WeightMap& wm, const std::string& layer, const std::string& key, ConvKind kind,
                     const std::vector<int>& perm, const std::vector<std::pair<int, int>>& taps) {
  std::string err;
  const ConvShape sh = conv_shape(kind);
  const HostTensor* w = find(wm, layer + ".w", &err);
  const HostTensor* b = find(wm, layer + ".b", &err);
  if (!w || !b) return fail(NUTLS_ERR_WEIGHTS, err);
  int max_kw = 0;
  for (const auto& tk : taps) max_kw = std::max(max_kw, tk.second);
  int max_perm = -1;
  for (int q : perm) max_perm = std::max(max_perm, q);
  if (w->dims.size() != 4 || w->dims[3] != sh.cin || static_cast<int>(perm.size()) != 32 * sh.nt || w->dims[0] <= max_perm ||
      w->dims[1] < sh.tt || w->dims[2] <= max_kw || static_cast<int>(b->size()) <= max_perm)
    return fail(NUTLS_ERR_WEIGHTS, "unexpected weight / bias shape for " + layer);
  ConvLayerW cw{};
  int rc = upload(e, pack_conv_weights(*w, perm, taps, sh.tt, sh.cin, sh.nt), &cw.wpk);
  if (rc) return rc;
  std::vector<float> bp(perm.size());
  for (size_t i = 0; i < perm.size(); ++i) bp[i] = b->data[perm[i]];
  if ((rc = upload(e, bp, &cw.bias))) return rc;
  if (e->off_bf16) {
    // block mode on an int8 container: the int8 payload as bf16 fragments + the per-channel scale (conv_bf16x3_kernel)
    const std::vector<float> wb = pack_conv_weights_bf16(*w, perm, taps, sh.tt, sh.cin, sh.nt);
    if (!wb.empty() && (w->scales.size() == 1 || static_cast<int>(w->scales.size()) == w->dims[0])) {
      std::vector<float> sc(perm.size(), 0.f);
      for (size_t i = 0; i < perm.size(); ++i)
        if (perm[i] >= 0) sc[i] = w->scales.size() == 1 ? w->scales[0] : w->scales[perm[i]];
      if ((rc = upload(e, wb, &cw.wbf))) return rc;
      if ((rc = upload(e, sc, &cw.wscale))) return rc;
    }
  }
  if (sh.epi_ln) {
    const HostTensor* g = find(wm, layer + ".gamma", &err);
    const HostTensor* bt = find(wm, layer + ".beta", &err);
    const HostTensor* al = find(wm, layer + ".alpha", &err);
    if (!g || !bt || !al) return fail(NUTLS_ERR_WEIGHTS, err);
    if (static_cast<int>(g->size()) != 32 * sh.g || static_cast<int>(bt->size()) != 32 * sh.g || al->size() < 1)
      return fail(NUTLS_ERR_WEIGHTS, "unexpected LayerNorm / PReLU size for " + layer);
    if ((rc = upload(e, g->data, &cw.gamma))) return rc;
    if ((rc = upload(e, bt->data, &cw.beta))) return rc;
    cw.alpha = al->data[0];
  }
  e->convw[key] = cw;
  return NUTLS_OK;
}

static std::vector<int> iota_perm(int n) {
  std::vector<int> p(n);
  for (int i = 0; i < n; ++i) p[i] = i;
  return p;
}
// Sub-pixel shuffle folded into the output-channel order (proposed.py:240-251):
// packed channel r*32+c of position f IS out[2f+r, c].
static std::vector<int> perm_shuffle64() {
  std::vector<int> p(64);
  for (int r = 0; r < 2; ++r)
    for (int c = 0; c < 32; ++c) p[r * 32 + c] = 2 * c + r;
  return p;
}
// 128-channel variant: the reference reshapes with the *input* channel count (32,2), so
// out[2f+r, C2] = y[f, r*64 + (C2%32)*2 + C2/32].
static std::vector<int> perm_shuffle128() {
  std::vector<int> p(128);
  for (int r = 0; r < 2; ++r)
    for (int c2 = 0; c2 < 64; ++c2) p[r * 64 + c2] = r * 64 + (c2 % 32) * 2 + c2 / 32;
  return p;
}

// [O][2][3][I] (OHWI) -> [t][kw][i][o]: the output channel becomes the fastest index
static std::vector<float> ohwi_to_tkio(const HostTensor& w) {
  const int O = w.dims[0], T = w.dims[1], K = w.dims[2], I = w.dims[3];
  std::vector<float> o(w.data.size());
  for (int oc = 0; oc < O; ++oc)
    for (int t = 0; t < T; ++t)
      for (int k = 0; k < K; ++k)
        for (int i = 0; i < I; ++i) o[((static_cast<size_t>(t) * K + k) * I + i) * O + oc] = w.data[((static_cast<size_t>(oc) * T + t) * K + k) * I + i];
  return o;
}

static int prep_ddb_weights(Engine* e, const WeightMap& wm) {
  std::string err;
  int rc;
  for (int b = 0; b < 13; ++b) {
    const bool central = b == 6;
    const std::string tag = central ? "ddb" : std::string((b < 6 ? kEncoder[b] : kDecoder[b - 7]).prefix) + "_ddb";
    Engine::DdbW& W = e->ddbw[b];
    auto conv_prelu = [&](const std::string& n, float** w, float** bias, float* alpha) -> int {
      const HostTensor* tw = find(wm, n + ".w", &err);
      const HostTensor* tb = find(wm, n + ".b", &err);
      const HostTensor* ta = find(wm, n + ".alpha", &err);
      if (!tw || !tb || !ta || tw->dims.size() != 4 || tw->dims[1] != 2 || tw->dims[2] != 3 || static_cast<int>(tb->size()) != tw->dims[0] || ta->size() < 1)
        return fail(NUTLS_ERR_WEIGHTS, err.empty() ? "bad ddb conv " + n : err);
      int r;
      if ((r = upload(e, ohwi_to_tkio(*tw), w))) return r;
      if ((r = upload(e, tb->data, bias))) return r;
      *alpha = ta->data[0];
      return NUTLS_OK;
    };
    if ((rc = conv_prelu(tag + "_in", &W.w_in, &W.b_in, &W.a_in))) return rc;
    if ((rc = conv_prelu(tag + "_out", &W.w_out, &W.b_out, &W.a_out))) return rc;
    // the LDS image of ddb_block_wg (ddb_device.hpp): wg all blocks [G][2][3][k] | w1 all blocks [G out][G in] |
    // bg, b1, gamma, beta per block | b_in | b_out -- a thread's grouped kernel and its 1x1 row are contiguous
    std::vector<float> pk_wg, pk_w1, pk_sm;
    for (int k = 1; k <= 6; ++k) {
      const std::string n = tag + "_" + std::to_string(k);
      const HostTensor* wg = find(wm, n + ".wg", &err);
      const HostTensor* bg = find(wm, n + ".bg", &err);
      const HostTensor* w1 = find(wm, n + ".w1", &err);
      const HostTensor* b1 = find(wm, n + ".b1", &err);
      const HostTensor* gm = find(wm, n + ".gamma", &err);
      const HostTensor* bt = find(wm, n + ".beta", &err);
      const HostTensor* al = find(wm, n + ".alpha", &err);
      if (!wg || !bg || !w1 || !b1 || !gm || !bt || !al) return fail(NUTLS_ERR_WEIGHTS, err);
      if (wg->dims.size() != 4 || wg->dims[3] != k || wg->dims[1] != 2 || wg->dims[2] != 3) return fail(NUTLS_ERR_WEIGHTS, "unexpected grouped-conv shape " + n);
      const int G = wg->dims[0];
      if (w1->size() != static_cast<size_t>(G) * G || static_cast<int>(bg->size()) != G || static_cast<int>(b1->size()) != G ||
          static_cast<int>(gm->size()) != G || static_cast<int>(bt->size()) != G || al->size() < 1)
        return fail(NUTLS_ERR_WEIGHTS, "unexpected 1x1 / LayerNorm size in " + n);
      if ((rc = upload(e, ohwi_to_tkio(*wg), &W.wg[k - 1]))) return rc;
      if ((rc = upload(e, bg->data, &W.bg[k - 1]))) return rc;
      if ((rc = upload(e, transpose2d(*w1, G, G), &W.w1[k - 1]))) return rc;
      if ((rc = upload(e, b1->data, &W.b1[k - 1]))) return rc;
      if ((rc = upload(e, gm->data, &W.gamma[k - 1]))) return rc;
      if ((rc = upload(e, bt->data, &W.beta[k - 1]))) return rc;
      W.alpha[k - 1] = al->data[0];
      pk_wg.insert(pk_wg.end(), wg->data.begin(), wg->data.end());
      pk_w1.insert(pk_w1.end(), w1->data.begin(), w1->data.end());
      for (const HostTensor* t : {bg, b1, gm, bt}) pk_sm.insert(pk_sm.end(), t->data.begin(), t->data.end());
    }
    pk_wg.insert(pk_wg.end(), pk_w1.begin(), pk_w1.end());
    pk_wg.insert(pk_wg.end(), pk_sm.begin(), pk_sm.end());
    for (const char* bn : {"_in.b", "_out.b"}) {
      const HostTensor* tb = find(wm, tag + bn, &err);
      if (!tb) return fail(NUTLS_ERR_WEIGHTS, err);
      pk_wg.insert(pk_wg.end(), tb->data.begin(), tb->data.end());
    }
    // the fused kernel's copy of the 1x1 kernels (ddb_fused.hpp): row g pre-rotated for DPP row rotations,
    // entry n = w1[g][((g - n) mod 16) + 16 h], first the lane's own half h of the row, then (G = 32) the other one
    {
      const int G = static_cast<int>(pk_sm.size()) / 24;
      for (int k = 0; k < 6; ++k)
        for (int g = 0; g < G; ++g)
          for (int half = 0; half < G / 16; ++half)
            for (int n = 0; n < 16; ++n) {
              const int h = half == 0 ? g >> 4 : 1 - (g >> 4);
              pk_wg.push_back(pk_w1[(static_cast<size_t>(k) * G + g) * G + ((g - n) & 15) + 16 * h]);
            }
    }
    if ((rc = upload(e, pk_wg, &W.wsmall))) return rc;
  }
  return NUTLS_OK;
}

static int prep_weights(Engine* e, const WeightMap& wm) {
  std::string err;
  int rc;
  const std::vector<std::pair<int, int>> taps3 = {{0, 0}, {0, 1}, {0, 2}};
  const std::vector<std::pair<int, int>> tap1 = {{0, 0}};
  for (int side = 0; side < 2; ++side)
    for (int s = 0; s < 6; ++s) {
      const StageDesc& st = side ? kDecoder[s] : kEncoder[s];
      const std::string P = st.prefix;
      if ((rc = prep_conv(e, wm, P + "_in", P + "_in", side ? CONV_IN_C128 : CONV_IN_C64, iota_perm(64), tap1))) return rc;
      for (int i = 1; i <= st.depth; ++i) {
        const int cin = (i == 1) ? (side ? 128 : 64) : (side ? 64 : 32);
        const ConvKind k = cin == 32 ? CONV_EL_C32 : cin == 64 ? CONV_EL_C64 : CONV_EL_C128;
        const std::string L = P + "_conv" + std::to_string(i);
        if ((rc = prep_conv(e, wm, L, L, k, iota_perm(32), taps3))) return rc;
      }
      for (int j = 1; j <= st.depth; ++j) {
        const std::string L = P + "_spconv" + std::to_string(j);
        if (j < st.depth) rc = prep_conv(e, wm, L, L, CONV_DL_N64, perm_shuffle64(), taps3);
        else rc = prep_conv(e, wm, L, L, CONV_DL_N128, perm_shuffle128(), taps3);
        if (rc) return rc;
      }
      if (!side) {
        if ((rc = prep_conv(e, wm, st.resample, st.resample, CONV_DOWN, iota_perm(64), taps3))) return rc;
      } else {
        // Conv2DTranspose (1,3) stride 2 (proposed.py:260-265):  out[2i] = W0 x[i] + W2 x[i-1],
        // out[2i+1] = W1 x[i]  
        if ((rc = prep_conv(e, wm, st.resample, std::string(st.resample) + "#even", CONV_UP_EVEN, iota_perm(128), {{0, 2}, {0, 0}}))) return rc;
        if ((rc = prep_conv(e, wm, st.resample, std::string(st.resample) + "#odd", CONV_UP_ODD, iota_perm(128), {{0, 1}}))) return rc;
      }
      // CTFA MLPs
      for (const char* br : {"_ta", "_fa"}) {
        const HostTensor* w1 = find(wm, P + br + ".w1", &err);
        const HostTensor* b1 = find(wm, P + br + ".b1", &err);
        const HostTensor* w2 = find(wm, P + br + ".w2", &err);
        const HostTensor* b2 = find(wm, P + br + ".b2", &err);
        if (!w1 || !b1 || !w2 || !b2) return fail(NUTLS_ERR_WEIGHTS, err);
        if (w1->size() != 16 * 64 || w2->size() != 64 * 16 || b1->size() != 16u || b2->size() != 64u) return fail(NUTLS_ERR_WEIGHTS, "unexpected CTFA shape " + P + br);
        CtfaW cw{};
        if ((rc = upload(e, transpose2d(*w1, 16, 64), &cw.w1T))) return rc;
        if ((rc = upload(e, b1->data, &cw.b1))) return rc;
        if ((rc = upload(e, transpose2d(*w2, 64, 16), &cw.w2T))) return rc;
        if ((rc = upload(e, w2->data, &cw.w2))) return rc;
        if ((rc = upload(e, b2->data, &cw.b2))) return rc;
        e->ctfaw[P + br] = cw;
      }
    }
  if (e->variant == NUTLS_VARIANT_BASELINE) {
    if ((rc = prep_ddb_weights(e, wm))) return rc;
  }
  // LSTM + Dense pairs (13)
  std::vector<std::pair<std::string, std::string>> lstms;
  for (int s = 0; s < 6; ++s) lstms.push_back({std::string(kEncoder[s].prefix) + "_lstm", std::string(kEncoder[s].prefix) + "_dense"});
  lstms.push_back({"lstm", "dense"});
  for (int s = 0; s < 6; ++s) lstms.push_back({std::string(kDecoder[s].prefix) + "_lstm", std::string(kDecoder[s].prefix) + "_dense"});
  if (e->variant != NUTLS_VARIANT_LSTM) lstms.clear();
  for (auto& ld : lstms) {
    const HostTensor* wx = find(wm, ld.first + ".wx", &err);
    const HostTensor* wh = find(wm, ld.first + ".wh", &err);
    const HostTensor* b = find(wm, ld.first + ".b", &err);
    const HostTensor* wd = find(wm, ld.second + ".w", &err);
    const HostTensor* bd = find(wm, ld.second + ".b", &err);
    if (!wx || !wh || !b || !wd || !bd) return fail(NUTLS_ERR_WEIGHTS, err);
    LstmW lw{};
    if (wx->dims.size() != 2 || wh->dims.size() != 2 || wd->dims.size() != 2 || wx->dims[0] != 84 || wh->dims[0] != 84 || wh->dims[1] != 21 ||
        wd->dims[1] != 21 || b->size() != 84u || static_cast<int>(bd->size()) != wd->dims[0])
      return fail(NUTLS_ERR_WEIGHTS, "unexpected LSTM shape " + ld.first);
    lw.din = wx->dims[1];
    lw.dout = wd->dims[0];
    if ((rc = upload(e, transpose2d(*wx, 84, lw.din), &lw.wxT))) return rc;
    if ((rc = upload(e, transpose2d(*wh, 84, 21), &lw.whT))) return rc;
    if ((rc = upload(e, b->data, &lw.bias))) return rc;
    if ((rc = upload(e, transpose2d(*wd, lw.dout, 21), &lw.wdT))) return rc;
    if ((rc = upload(e, bd->data, &lw.bd))) return rc;
    e->lstmw[ld.first] = lw;
  }
  // input layer / output conv
  const HostTensor* iw = find(wm, "input_layer.w", &err);
  const HostTensor* ib = find(wm, "input_layer.b", &err);
  const HostTensor* ig = find(wm, "input_layer.gamma", &err);
  const HostTensor* ibt = find(wm, "input_layer.beta", &err);
  const HostTensor* ia = find(wm, "input_layer.alpha", &err);
  const HostTensor* ow = find(wm, "out_conv.w", &err);
  const HostTensor* ob = find(wm, "out_conv.b", &err);
  if (!iw || !ib || !ig || !ibt || !ia || !ow || !ob) return fail(NUTLS_ERR_WEIGHTS, err);
  if (iw->size() != 64u || ib->size() != 64u || ig->size() != 64u || ibt->size() != 64u || ia->size() < 1 || ow->size() != 64u || ob->size() < 1)
    return fail(NUTLS_ERR_WEIGHTS, "unexpected input layer / output conv shape");
  if ((rc = upload(e, iw->data, &e->in_w))) return rc;
  if ((rc = upload(e, ib->data, &e->in_b))) return rc;
  if ((rc = upload(e, ig->data, &e->in_g))) return rc;
  if ((rc = upload(e, ibt->data, &e->in_bt))) return rc;
  if ((rc = upload(e, ow->data, &e->out_w))) return rc;
  e->in_alpha = ia->data[0];
  e->out_bias = ob->data[0];
  return NUTLS_OK;
}

// ------------------------------------------------------------------------------- state --------
static int add_state(Engine* e, const std::string& prev, const std::string& cur, int d0, int d1, int ring_d = 0) {
  StateTensor st;
  st.ring_d = ring_d;
  st.name_prev = prev;
  st.name_cur = cur;
  st.d0 = d0;
  st.d1 = d1;
  const int idx = static_cast<int>(e->states.size());
  e->states.push_back(st);
  e->states[idx].buf[0] = e->states[idx].buf[1] = nullptr;      // slots: allocate_states()
  e->state_index[prev] = idx;
  e->state_index[cur] = idx;
  return idx;
}

// Arena slots of the state tensors: all first buffers in signature order, then all second buffers in the same
// order -- `cur` and `prev` of EVERY ping-pong tensor are the same constant apart (the fused kernel addresses
// them as parity base + one offset, tools/gen_fused_plan.py mirrors this layout) -- then the in-place rings.
static void allocate_states(Engine* e) {
  for (int b = 0; b < 2; ++b)
    for (StateTensor& st : e->states)
      if (st.ring_d == 0) slot_reserve(e, st.per_stream(), &st.buf[b]);
  for (StateTensor& st : e->states)
    if (st.ring_d > 0) slot_reserve(e, st.per_stream(), &st.buf[0]);      // single buffer; buf[1] aliased after arena_commit
}

// State inventory in the order of the reference's signature (converter_proposed.py:27-186).
static int build_states(Engine* e) {
  for (int side = 0; side < 2; ++side)
    for (int s = 0; s < 6; ++s) {
      const StageDesc& st = side ? kDecoder[s] : kEncoder[s];
      StageStates& ss = side ? e->dec_st[s] : e->enc_st[s];
      for (int i = 1; i <= st.depth; ++i) {
        const int f = st.f0 >> (i - 1);
        const int c = (i == 1) ? (side ? 128 : 64) : (side ? 64 : 32);
        const std::string tag = st.conv_tag;
        int idx = add_state(e, tag + "_prev" + std::to_string(i), tag + "_cur" + std::to_string(i), f, c);
        if (idx < 0) return idx;
        ss.conv.push_back(idx);
      }
      for (int j = 1; j <= st.depth; ++j) {
        const int f = (st.f0 >> st.depth) << (j - 1);
        const std::string tag = st.spconv_tag;
        int idx = add_state(e, tag + "_prev" + std::to_string(j), tag + "_cur" + std::to_string(j), f, 64);
        if (idx < 0) return idx;
        ss.spconv.push_back(idx);
      }
    }
  if (e->variant == NUTLS_VARIANT_BASELINE) {
    // dilated-dense block states (converter_nunet_tls.py:173-180, :228-235): 13 bottlenecks in
    // network order -- 6 encoder stages, the central block ("ddb"), 6 decoder stages
    for (int b = 0; b < 13; ++b) {
      const bool central = b == 6;
      const StageDesc* st = central ? nullptr : (b < 6 ? &kEncoder[b] : &kDecoder[b - 7]);
      const int F = central ? 4 : (st->f0 >> st->depth), C = central ? 64 : 32, G = C / 2;
      const std::string tag = central ? "ddb" : std::string(st->prefix) + "_ddb";
      Engine::DdbStates& ds = e->ddb_st[b];
      if ((ds.in = add_state(e, tag + "_prev_in", tag + "_cur_in", F, C, 1)) < 0) return ds.in;
      for (int k = 1; k <= 6; ++k) {
        const int d = 1 << (k - 1);
        if ((ds.blk[k - 1] = add_state(e, tag + "_prev" + std::to_string(k), tag + "_cur" + std::to_string(k), d * F, k * G, d)) < 0)
          return ds.blk[k - 1];
      }
      if ((ds.out = add_state(e, tag + "_prev_out", tag + "_cur_out", F, G, 1)) < 0) return ds.out;
    }
    return NUTLS_OK;
  }
  auto add_hc = [&](const std::string& base, int* h, int* c) -> int {
    *h = add_state(e, base + "_h", base + "_h", NUTLS_LSTM_UNITS, 1);
    if (*h < 0) return *h;
    *c = add_state(e, base + "_c", base + "_c", NUTLS_LSTM_UNITS, 1);
    return *c < 0 ? *c : 0;
  };
  int rc;
  for (int s = 0; s < 6; ++s)
    if ((rc = add_hc(kEncoder[s].prefix, &e->enc_st[s].h, &e->enc_st[s].c)) < 0) return rc;
  if ((rc = add_hc("state", &e->central_h, &e->central_c)) < 0) return rc;
  for (int s = 0; s < 6; ++s)
    if ((rc = add_hc(kDecoder[s].prefix, &e->dec_st[s].h, &e->dec_st[s].c)) < 0) return rc;
  return NUTLS_OK;
}

// ------------------------------------------------------------------------------- plan ---------
static void push_conv(Engine* e, std::vector<Launch>* plan, const std::string& wkey, ConvKind k, const float* src0,
                      const float* src1, int src_ld, int f_in, int f_out, float* dst0, int ld0, float* dst1, int ld1,
                      int row_mul, int row_add, bool enc_strided = false) {
  const ConvLayerW& w = e->convw.at(wkey);
  Launch L{};
  L.kind = Launch::CONV;
  L.ck = k;
  L.name = wkey;
  L.encoder_strided = enc_strided;
  ConvParams& p = L.conv;
  p.src0 = src0; p.src1 = src1; p.wpk = w.wpk; p.bias = w.bias; p.gamma = w.gamma; p.beta = w.beta;
  p.wbf = w.wbf; p.wscale = w.wscale; p.use_bf16 = 0;
  p.dst0 = dst0; p.dst1 = dst1; p.src_ld = src_ld; p.ld0 = ld0; p.ld1 = ld1;
  p.B = e->B; p.F_in = f_in; p.F_out = f_out; p.log2_fout = ilog2(f_out);
  p.row_mul = row_mul; p.row_add = row_add; p.alpha = w.alpha; p.sstride = static_cast<long long>(e->sstride);
  plan->push_back(L);
}

// Baseline bottleneck b (0..12): same input / output placement as the LSTM + Dense it replaces.
static void push_ddb(Engine* e, std::vector<Launch>* plan, int par, int b, const std::string& name, const float* x, int x_ld, float* dst,
                     int dst_ld, int F, int C) {
  const Engine::DdbW& W = e->ddbw[b];
  const Engine::DdbStates& S = e->ddb_st[b];
  DdbParams p{};
  p.x = x; p.x_ld = x_ld; p.dst = dst; p.dst_ld = dst_ld;
  p.st_in = e->states[S.in].buf[0];
  for (int k = 0; k < 6; ++k) p.st_blk[k] = e->states[S.blk[k]].buf[0];
  p.st_out = e->states[S.out].buf[0];
  p.w_in = W.w_in; p.b_in = W.b_in; p.a_in = W.a_in;
  for (int k = 0; k < 6; ++k) {
    p.wg[k] = W.wg[k]; p.bg[k] = W.bg[k]; p.w1[k] = W.w1[k]; p.b1[k] = W.b1[k];
    p.gamma[k] = W.gamma[k]; p.beta[k] = W.beta[k]; p.alpha[k] = W.alpha[k];
  }
  p.w_out = W.w_out; p.b_out = W.b_out; p.a_out = W.a_out;
  p.wsmall = W.wsmall;
  p.step = e->d_step; p.F = F; p.C = C; p.B = e->B; p.sstride = static_cast<long long>(e->sstride);
  Launch L{};
  L.kind = Launch::DDB;
  L.name = name;
  L.ddb = p;
  L.ddb_index = par * 13 + b;          // x / dst live in parity-specific state tensors: one table entry per parity
  plan->push_back(L);
  if (e->ddbs.size() < 26) e->ddbs.resize(26);
  e->ddbs[L.ddb_index] = p;
}

static void push_lstm(Engine* e, std::vector<Launch>* plan, const std::string& lname, const float* x, int x_ld, int x_rows,
                      int x_cols, float* dst, int dst_ld, int dst_rows, int dst_cols, int h_idx, int c_idx, int par) {
  const LstmW& w = e->lstmw.at(lname);
  Launch L{};
  L.kind = Launch::LSTM;
  L.name = lname;
  LstmParams& p = L.lstm;
  p.x = x; p.x_ld = x_ld; p.x_rows = x_rows; p.x_cols = x_cols;
  p.wxT = w.wxT; p.whT = w.whT; p.bias = w.bias; p.wdT = w.wdT; p.bd = w.bd;
  p.h_in = e->states[h_idx].buf[1 - par]; p.c_in = e->states[c_idx].buf[1 - par];
  p.h_out = e->states[h_idx].buf[par]; p.c_out = e->states[c_idx].buf[par];
  p.dst = dst; p.dst_ld = dst_ld; p.dst_rows = dst_rows; p.dst_cols = dst_cols;
  p.Din = w.din; p.Dout = w.dout; p.B = e->B; p.sstride = static_cast<long long>(e->sstride);
  plan->push_back(L);
}

// One MSFE stage (converter_proposed.py:225-262 encoder, :467-498 decoder).
static void build_stage(Engine* e, std::vector<Launch>* plan, int side, int s, int par, const float* x_src, int x_ld,
                        float* y_dst, int y_ld) {
  const StageDesc& st = side ? kDecoder[s] : kEncoder[s];
  const StageStates& ss = side ? e->dec_st[s] : e->enc_st[s];
  const StageStates* pair_dec = side ? nullptr : &e->dec_st[decoder_of_encoder(s)];
  const std::string P = st.prefix;
  const int D = st.depth, FD = st.f0 >> D;
  auto cur = [&](int idx) { return e->states[idx].buf[par]; };
  auto prev = [&](int idx) { return e->states[idx].buf[1 - par]; };
  const int c1 = side ? 128 : 64;
  // e0 = inconv(x)  -> channels [0,64) of the first strided conv's input
  push_conv(e, plan, P + "_in", side ? CONV_IN_C128 : CONV_IN_C64, x_src, nullptr, x_ld, st.f0, st.f0, cur(ss.conv[0]), c1,
            nullptr, 0, 1, 0);
  // e_i = EL_i([prev_i ; cur_i]); e_i feeds conv i+1 and the stage's own sub-pixel conv D-i+1
  for (int i = 1; i <= D; ++i) {
    const int ci = e->states[ss.conv[i - 1]].d1, fi = st.f0 >> (i - 1);
    const ConvKind k = ci == 32 ? CONV_EL_C32 : ci == 64 ? CONV_EL_C64 : CONV_EL_C128;
    float *d0, *d1 = nullptr;
    int l0, l1 = 0;
    if (i < D) {
      d0 = cur(ss.conv[i]); l0 = e->states[ss.conv[i]].d1;
      d1 = cur(ss.spconv[D - i]) + 32; l1 = 64;          // sub-pixel conv j = D-i+1 -> index D-i
    } else {
      d0 = cur(ss.spconv[0]) + 32; l0 = 64;
    }
    push_conv(e, plan, P + "_conv" + std::to_string(i), k, prev(ss.conv[i - 1]), cur(ss.conv[i - 1]), ci, fi, fi / 2, d0, l0,
              d1, l1, 1, 0, side == 0);
  }
  // d_0 = Dense(LSTM(flatten(e_D)))  -> channels [0,32) of the first sub-pixel conv's input
  if (e->variant == NUTLS_VARIANT_BASELINE)
    push_ddb(e, plan, par, side ? 7 + s : s, P + "_ddb", cur(ss.spconv[0]) + 32, 64, cur(ss.spconv[0]), 64, FD, 32);
  else
    push_lstm(e, plan, P + "_lstm", cur(ss.spconv[0]) + 32, 64, FD, 32, cur(ss.spconv[0]), 64, FD, 32, ss.h, ss.c, par);
  // d_j = DL_j([prev_j ; cur_j])
  const float* dD = nullptr;
  int dD_ld = 0;
  for (int j = 1; j <= D; ++j) {
    const int fj = FD << (j - 1);
    float *d0, *d1 = nullptr;
    int l0, l1 = 0;
    if (j < D) {
      d0 = cur(ss.spconv[j]); l0 = 64;
      if (pair_dec) { d1 = cur(pair_dec->conv[D - j]) + 32; l1 = 64; }   // decoder conv i = D-j+1 (second-level skip)
      push_conv(e, plan, P + "_spconv" + std::to_string(j), CONV_DL_N64, prev(ss.spconv[j - 1]), cur(ss.spconv[j - 1]), 64, fj,
                fj, d0, l0, d1, l1, 2, 0);
    } else {
      if (pair_dec) { d0 = cur(pair_dec->conv[0]) + 64; l0 = 128; }      // skip into decoder conv 1
      else { d0 = e->t_d; l0 = 64; }
      dD = d0; dD_ld = l0;
      push_conv(e, plan, P + "_spconv" + std::to_string(j), CONV_DL_N128, prev(ss.spconv[j - 1]), cur(ss.spconv[j - 1]), 64, fj,
                fj, d0, l0, nullptr, 0, 2, 0);
    }
  }
  // y = d_D * (TA*FA) + e0
  Launch L{};
  L.kind = Launch::CTFA;
  L.name = P + "_ctfa";
  CtfaParams& c = L.ctfa;
  const CtfaW& ta = e->ctfaw.at(P + "_ta");
  const CtfaW& fa = e->ctfaw.at(P + "_fa");
  c.x = dD; c.x_ld = dD_ld; c.e0 = cur(ss.conv[0]); c.e0_ld = c1; c.y = y_dst; c.y_ld = y_ld;
  c.ta_w1T = ta.w1T; c.ta_b1 = ta.b1; c.ta_w2T = ta.w2T; c.ta_b2 = ta.b2;
  c.fa_w1T = fa.w1T; c.fa_b1 = fa.b1; c.fa_w2T = fa.w2T; c.fa_b2 = fa.b2;
  c.ta_w2 = ta.w2; c.fa_w2 = fa.w2;
  c.B = e->B; c.F = st.f0; c.sstride = static_cast<long long>(e->sstride);
  plan->push_back(L);
}

static void build_plan(Engine* e, int par) {
  std::vector<Launch>* plan = &e->plan[par];
  plan->clear();
  {
    Launch L{};
    L.kind = Launch::INLAYER;
    L.name = "input_layer";
    L.inl = InLayerParams{e->io_in, e->t_inlayer, e->in_w, e->in_b, e->in_g, e->in_bt, e->in_alpha, e->B * NUTLS_BINS,
                          static_cast<long long>(e->sstride)};
    plan->push_back(L);
  }
  const float* x = e->t_inlayer;
  int x_ld = 64;
  for (int s = 0; s < 6; ++s) {
    const StageDesc& st = kEncoder[s];
    build_stage(e, plan, 0, s, par, x, x_ld, e->t_y, 64);
    // down-sampling output lives in channels [64,128) of the paired decoder's up-sampling input
    float* cat = e->upcat[decoder_of_encoder(s)];
    push_conv(e, plan, st.resample, CONV_DOWN, e->t_y, nullptr, 64, st.f0, st.f0 / 2, cat + 64, 128, nullptr, 0, 1, 0);
    x = cat + 64;
    x_ld = 128;
  }
  // central LSTM over flatten([4,64]) (converter_proposed.py:456-459)
  if (e->variant == NUTLS_VARIANT_BASELINE)
    push_ddb(e, plan, par, 6, "ddb", e->upcat[0] + 64, 128, e->upcat[0], 128, 4, 64);
  else
    push_lstm(e, plan, "lstm", e->upcat[0] + 64, 128, 4, 64, e->upcat[0], 128, 4, 64, e->central_h, e->central_c, par);
  for (int s = 0; s < 6; ++s) {
    const StageDesc& st = kDecoder[s];
    const int fin = st.f0 / 2;
    push_conv(e, plan, std::string(st.resample) + "#even", CONV_UP_EVEN, e->upcat[s], nullptr, 128, fin, fin, e->t_up, 128, nullptr,
              0, 2, 0);
    push_conv(e, plan, std::string(st.resample) + "#odd", CONV_UP_ODD, e->upcat[s], nullptr, 128, fin, fin, e->t_up, 128, nullptr, 0,
              2, 1);
    float* y = (s < 5) ? e->upcat[s + 1] : e->t_y;
    build_stage(e, plan, 1, s, par, e->t_up, 128, y, (s < 5) ? 128 : 64);
  }
  Launch L{};
  L.kind = Launch::OUTCONV;
  L.name = "out_conv";
  L.outc = OutConvParams{e->t_y, 64, e->io_out, e->out_w, e->out_bias, e->B * NUTLS_BINS, static_cast<long long>(e->sstride)};
  plan->push_back(L);
}

hipError_t run_launch(const Launch& L, hipStream_t s, const ConvKnobs& kn) {
  switch (L.kind) {
    case Launch::CONV: return launch_conv(L.ck, L.conv, s, kn);
    case Launch::LSTM: return launch_lstm(L.lstm, s);
    case Launch::CTFA: return launch_ctfa(L.ctfa, s);
    case Launch::INLAYER: return launch_input_layer(L.inl, s);
    case Launch::OUTCONV: return launch_out_conv(L.outc, s);
    case Launch::DDB: return launch_ddb(L.ddb, s);
  }
  return hipErrorInvalidValue;
}

int run_plan(Engine* e, int par, hipStream_t s) {
  for (const Launch& L : e->plan[par]) {
    hipError_t err = run_launch(L, s, e->conv_knobs);
    if (err != hipSuccess) return fail(NUTLS_ERR_HIP, "launch " + L.name + ": " + hipGetErrorString(err));
  }
  if (e->variant == NUTLS_VARIANT_BASELINE) HIP_TRY(launch_incr_step(e->d_step, s));   // ring position of the dilated-dense history
  return NUTLS_OK;
}

// Regions of HBM a launch writes, for the hand-off analysis: (row-0 pointer incl. channel offset, ld, channels)
struct WriteRegion { const float* ptr; int ld, nchan, launch; };

static void collect_writes(const Launch& L, int idx, std::vector<WriteRegion>* out) {
  switch (L.kind) {
    case Launch::CONV: {
      const ConvShape sh = conv_shape(L.ck);
      const int gc = 32 * sh.g;
      out->push_back({L.conv.dst0, L.conv.ld0, gc, idx});
      if (L.conv.dst1) out->push_back({L.conv.dst1, L.conv.ld1, gc, idx});
      break;
    }
    case Launch::LSTM: out->push_back({L.lstm.dst, L.lstm.dst_ld, L.lstm.dst_cols, idx}); break;
    case Launch::CTFA: out->push_back({L.ctfa.y, L.ctfa.y_ld, 64, idx}); break;
    case Launch::INLAYER: out->push_back({L.inl.y, 64, 64, idx}); break;
    case Launch::OUTCONV: break;
    case Launch::DDB: out->push_back({L.ddb.dst, L.ddb.dst_ld, L.ddb.C, idx}); break;
  }
}

// Decides, for every pair of consecutive conv layers (L, N), whether L completes N's LDS image
// (hand-off) -- possible when N keeps all its phases resident and every channel of N's current-frame
// input was written either by L itself (then L forwards those rows from its epilogue) or by a launch
// before L (then L prefetches them from HBM while its own MFMAs run).
// The baseline variant's 13 dilated-dense blocks, as the device-side table every kernel family reads (host copy: Engine::ddbs).
static int upload_ddb_table(Engine* e) {
  if (!e->ddbs.empty()) {
    void* t = nullptr;
    HIP_TRY(hipMalloc(&t, e->ddbs.size() * sizeof(DdbParams)));
    e->allocs.push_back(t);
    HIP_TRY(hipMemcpy(t, e->ddbs.data(), e->ddbs.size() * sizeof(DdbParams), hipMemcpyHostToDevice));
    e->d_ddb = static_cast<DdbParams*>(t);
  }
  return NUTLS_OK;
}

// ---- fused kernel (mode 3): weight blob in plan order + the check that the arena is laid out as the plan says ----
static int fused_setup(Engine* e, const WeightMap& wm) {
  const int v = e->variant;
  const FusedPlan& one = *fused_plan(v, 1);      // (every variant has a one-stream plan: the arena is laid out for it)
  const bool same_count = static_cast<int>(e->states.size()) == one.num_states;
  bool ok = same_count && e->sstride >= static_cast<size_t>(one.arena_floats);
  for (int i = 0; ok && i < one.num_states; ++i) {
    const StateTensor& st = e->states[i];
    const bool ring = i >= one.num_pingpong;        // baseline: the dilated-dense history rings are updated in place
    ok = st.name_prev == one.states[i].name && st.buf[0] - e->arena == one.states[i].off &&
         st.buf[1] - st.buf[0] == (ring ? 0 : one.parity_stride);
  }
  const float* scratch[11] = {e->t_inlayer, e->t_y, e->t_d, e->t_up, e->upcat[0], e->upcat[1], e->upcat[2], e->upcat[3], e->upcat[4], e->upcat[5], e->ysum};
  ok = ok && one.num_scratch == 11 && e->ysum && e->ysum - e->arena == one.ys_off;
  for (int i = 0; ok && i < one.num_scratch && i < 11; ++i) ok = scratch[i] - e->arena == one.scratch[i].off;
  if (ok && v == NUTLS_VARIANT_BASELINE) ok = e->d_ddb != nullptr && e->ddbs.size() == 26;
  if (!ok) return fail(NUTLS_ERR_ARG, "fused plan (tools/gen_fused_plan.py) does not match the engine's arena layout");
  // Which plan: one stream per workgroup, or a packed plan (two / four streams per workgroup: one weight fetch / conversion and one latency
  // chain for all of them in the layers whose images fit LDS that often).  NUTLS_FUSED_STREAMS=1 / 2 / 4 overrides (the stream count must be
  // a multiple).
  // Choice by a two-number cost model: a step takes ceil(workgroups / CUs) rounds of the plan's step time, and those are 1 : 1.65 : 3.44 for
  // 1 / 2 / 4 streams per workgroup (0.284 / 0.467 / 0.976 ms, round 6: profiles/plan_cost_model.json, tools/gpu_plan_cost.py -- the cache policy
  // of round 6 took 15 % off the one- and two-stream kernels and nothing off the four-stream one; round 4 measured 1 : 1.58 : 2.82).  256 streams:
  // one per workgroup (one round); 300 .. 512: two (one round instead of two); 768: one (three rounds of 1.0 < one round of fours at 3.44);
  // 1024, 1536, 2048: two (2 / 3 / 4 rounds of 1.65 < 1 / 2 / 2 rounds of 3.44 -- measured: 1 048 k against 996 k frames/s at 1024 streams,
  // 1 073 k against 1 018 k at 2048, tools/exp/plan_ab.py).  The four-stream plan is still built and selectable (nutls_create_plan).
  int streams = 1;
  {
    const double t_plan[5] = {0.0, 1.0, 1.65, 0.0, 3.44};
    double best = 0.0;
    for (int g : {1, 2, 4}) {
      if (e->B % g != 0 || !fused_plan(v, g)) continue;
      const int wgs = e->B / g, rounds = (wgs + e->n_cu - 1) / e->n_cu;
      const double t = rounds * t_plan[g];
      if (best == 0.0 || t < best * 0.98) { best = t; streams = g; }      // (ties and near-ties: the smaller group)
    }
  }
  if (const char* ev = getenv("NUTLS_FUSED_STREAMS")) streams = atoi(ev);      // (developer override; falls back like the library's own choice)
  if (streams < 1 || !fused_plan(v, streams) || e->B % streams != 0) streams = 1;
  if (e->fz_streams_req > 0) {          // nutls_create_plan: the caller's choice wins -- or the call fails, it never silently becomes another plan
    if (!fused_plan(v, e->fz_streams_req))
      return fail(NUTLS_ERR_ARG, "nutls_create_plan: no fused plan with that many streams per workgroup for this variant (plans: 1, 2, 4 for the LSTM variant, 1 for the baseline)");
    if (e->B % e->fz_streams_req != 0)
      return fail(NUTLS_ERR_ARG, "nutls_create_plan: the batch must be a multiple of streams_per_workgroup");
    streams = e->fz_streams_req;
  }
  const FusedPlan& plan = *fused_plan(v, streams);
  if (plan.arena_floats != one.arena_floats || plan.parity_stride != one.parity_stride || plan.ys_off != one.ys_off || plan.ys_block != one.ys_block)
    return fail(NUTLS_ERR_ARG, "packed fused plan does not share the arena layout of the one-stream plan");
  e->fz_plan = &plan;
  std::vector<float> blob;
  std::string err;
  if (fused_pack_blob(plan, wm, &blob, &err) != FZ_PACK_OK) {
    // Not packable for the fused kernel -- float conv kernels (no int8 payload), only some of them int8, a scale count that
    // does not match ... -- is not an error of the handle: the per-layer modes only need the de-quantised floats, the handle
    // runs on them (hipGraph replay, mode 1, chosen at the end of nutls_create), and nutls_set_mode(3) reports the reason kept here.
    e->fz_reason = err;
    // ... unless the caller asked for a plan of the fused kernel by name (nutls_create_plan): that request never silently becomes another
    // plan or another kernel family
    if (e->fz_streams_req > 0)
      return fail(NUTLS_ERR_WEIGHTS, "nutls_create_plan: the container cannot run on the fused kernel (" + err + "); nutls_create picks the per-layer kernels for it");
    return NUTLS_OK;
  }
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, blob.size() * sizeof(float)));
  e->allocs.push_back(p);
  HIP_TRY(hipMemcpy(p, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice));
  e->fz_blob = static_cast<float*>(p);
  int rcz = dev_alloc(e, 128, &e->fz_ta_zero, true);
  if (rcz) return rcz;
  void* q = nullptr;
  // op starts + 8 phase stamps per op (wave 0) + the per-wave trace of the FZ_WTRACE build: 8 waves x ops x 12 shader-clock stamps
  const size_t n_stamps = static_cast<size_t>(plan.num_ops) * (9 + 8 * 12) + 1;
  HIP_TRY(hipMalloc(&q, n_stamps * sizeof(unsigned long long)));
  e->allocs.push_back(q);
  HIP_TRY(hipMemset(q, 0, n_stamps * sizeof(unsigned long long)));
  e->fz_prof = static_cast<unsigned long long*>(q);
  HIP_TRY(plan.set_attributes());
  // the table for rebuilding the carried partial sums (ysum_refresh)
  std::vector<YsOp> yops;
  std::vector<float> yw;
  if (!fused_ys_table(plan, wm, &yops, &yw, &err)) return fail(NUTLS_ERR_WEIGHTS, "fused plan: " + err);
  void* yo = nullptr;
  HIP_TRY(hipMalloc(&yo, yops.size() * sizeof(YsOp)));
  e->allocs.push_back(yo);
  HIP_TRY(hipMemcpy(yo, yops.data(), yops.size() * sizeof(YsOp), hipMemcpyHostToDevice));
  e->d_ys_ops = static_cast<YsOp*>(yo);
  e->n_ys_ops = static_cast<int>(yops.size());
  int rc = upload(e, yw, &e->d_ys_w);
  if (rc) return rc;
  // the lazily written states of the one-stream plans (the packed plans hand rows over through some of them: they write everything)
  std::vector<LazyCopy> lazy;
  if (plan.streams == 1) fused_lazy_table(plan, &lazy);
  e->n_lazy = static_cast<int>(lazy.size());
  if (e->n_lazy) {
    void* lz = nullptr;
    HIP_TRY(hipMalloc(&lz, lazy.size() * sizeof(LazyCopy)));
    e->allocs.push_back(lz);
    HIP_TRY(hipMemcpy(lz, lazy.data(), lazy.size() * sizeof(LazyCopy), hipMemcpyHostToDevice));
    e->d_lazy = static_cast<LazyCopy*>(lz);
  }
  if (const char* ev = getenv("NUTLS_EAGER_STATES")) e->eager_states = atoi(ev) != 0;      // (developer knob: every launch writes every state)
  if (const char* ev = getenv("NUTLS_FUSED_SKEW")) e->fz_skew = atoi(ev);
  // (developer knob: every step of the handle runs the stop twin to the end -- op index num_ops is never reached -- so that a test can hold
  //  its instruction stream to the production kernel's results; one-stream plan of the LSTM variant, the only kernel that has a twin)
  if (const char* ev = getenv("NUTLS_FUSED_STOP_TWIN")) {
    if (atoi(ev) != 0) {
      if (e->variant != NUTLS_VARIANT_LSTM || plan.streams != 1)
        return fail(NUTLS_ERR_ARG, "NUTLS_FUSED_STOP_TWIN: the stop twin exists for the one-stream plan of the LSTM variant only");
      HIP_TRY(fused_step_stop_set_attributes());
      e->fz_stop_at = plan.num_ops;
    }
  }
  return NUTLS_OK;
}

// The state tensors the last fused step left unwritten, rebuilt from their second copy (the skip-connection slices it did write), in the
// parity that step wrote -- the one every reader outside the kernel looks at.
int states_materialize(Engine* e, hipStream_t s) {
  if (!e->states_stale || !e->n_lazy) { e->states_stale = false; return NUTLS_OK; }
  if (!s) HIP_TRY(hipDeviceSynchronize());      // (called from a host-side accessor: the step may have run on any stream)
  const int block = (1 - e->next_parity) ? e->fz_plan->parity_stride : 0;
  HIP_TRY(launch_lazy_states(e->arena, static_cast<long long>(e->sstride), block, e->d_lazy, e->n_lazy, e->B, s));
  e->states_stale = false;
  return NUTLS_OK;
}

// Before a fused step: the partial sums the step reads (the block of the parity it does not write) from the conv-input states it
// would have read as the previous frame -- if anything but the fused kernel wrote those since (ys_dirty).
static int ysum_refresh(Engine* e, int par, hipStream_t s) {
  if (!e->ys_dirty || !e->n_ys_ops) return NUTLS_OK;
  if (int rc = states_materialize(e, s)) return rc;      // (the sums are rebuilt from the conv-input states)
  const FusedPlan& p = *e->fz_plan;
  const int x_block = par ? 0 : p.parity_stride;                   // the `prev` parity of this step
  const int ys_block = p.ys_off + (par ? 0 : p.ys_block);          // the block this step reads
  HIP_TRY(launch_ysum_refresh(e->arena, static_cast<long long>(e->sstride), x_block, ys_block, e->d_ys_ops, e->d_ys_w, e->n_ys_ops, e->B, s));
  e->ys_dirty = false;
  return NUTLS_OK;
}

// (mag_in / mag_out: the caller's device buffers, read by the input layer and written by the last op directly -- no staging copies)
// (active: device mask of nutls_step_active, null = every stream takes the frame)
// (hop: the single-launch hop of nutls_set_hop_fusion -- the plan's hop build analyses hop->pcm_in in front of the step and synthesises
//  hop->pcm_out behind it; the caller fills in the two PCM pointers and dc_edge, the handle's front / back end buffers are added here)
int run_fused(Engine* e, int par, hipStream_t s, bool prof, const float* mag_in, float* mag_out, const unsigned char* active, const FzHop* hop) {
  if (!e->fz_blob) return fail(NUTLS_ERR_ARG, "fused mode is not available for this handle");
  const bool base = e->variant == NUTLS_VARIANT_BASELINE;
  if (hop && (!e->fz_plan->launch_hop || !e->fe_twb || prof || e->fz_stop_at >= 0))
    return fail(NUTLS_ERR_ARG, "single-launch hop: not available for this handle (nutls_set_hop_fusion)");
  if (int rc = ysum_refresh(e, par, s)) return rc;
  auto launch = hop ? e->fz_plan->launch_hop : e->fz_plan->launch;
  int skew = e->fz_skew;            // (NUTLS_FUSED_SKEW at creation, nutls_debug_knob(h, "skew", v) later)
  if (e->fz_stop_at >= 0) {         // (nutls_profile_production: one-stream LSTM plan only, checked there)
    launch = launch_fused_step_stop;
    skew = e->fz_stop_at;
  }
  int eager = (e->eager_states || !e->n_lazy) ? 1 : 0;
  if (active && e->lazy_edited && !eager) {
    // A held stream keeps the rows nutls_state_set gave it, and states_materialize would rebuild its lazily written states from second copies
    // that may be older than the edit.  Until a step of all streams has replaced every edited row, masked launches write every state
    // themselves: nothing is left for states_materialize to rebuild (nutls_state_set left the `prev` side complete).
    if (int rc = states_materialize(e, s)) return rc;
    eager = 1;
  }
  float* const dbg = prof ? e->fz_dbg : nullptr;      // (activation trace: the profiling builds only)
  const long long dbg_ss = static_cast<long long>(kDbgSlots) * kDbgSlotFloats;
  FzTa ta{e->fz_ta_zero, e->fz_ta_zero + 64, 0, 0, 0, 0, skew, eager, dbg, dbg_ss};
  if (e->ctfa_causal && e->fz_ta_ring) {
    const int slot = static_cast<int>(e->steps & 31);          // this frame's row of the history: the sums leave it out, the step overwrites it
    HIP_TRY(launch_ta_sum(e->fz_ta_ring, e->fz_ta_sum, slot, e->B, s));
    ta = FzTa{e->fz_ta_sum, e->fz_ta_ring + slot * 64, 12 * 64, 64, 12 * 32 * 64, 32 * 64, skew, eager, dbg, dbg_ss};
  }
  ta.active = active;
  if (hop) ta.hop = FzHop{hop->pcm_in, hop->pcm_out, e->fe_tail, e->fe_ola, e->fe_ph, e->fe_win, e->fe_inv, e->fe_twb, hop->dc_edge};
  hipError_t err = launch(e->arena, static_cast<long long>(e->sstride), e->fz_blob, mag_in ? mag_in : e->io_in,
                          mag_out ? mag_out : e->io_out, e->B, par, prof ? e->fz_prof : nullptr,
                          base ? e->d_ddb : nullptr, static_cast<int>(e->steps & 0x3fffffff), e->B / e->fz_plan->streams, s, ta);
  if (err == hipErrorNotSupported && prof)
    return fail(NUTLS_ERR_ARG, "this packed fused plan has no profiling build in the library (NUTLS_BUILD_G4_PROF=1 python -m nunet_amd.build adds the 4-stream one; "
                               "NUTLS_FUSED_STREAMS=1 selects the one-stream plan)");
  if (err != hipSuccess) return fail(NUTLS_ERR_HIP, std::string("fused step launch: ") + hipGetErrorString(err));
  if (base) e->d_step_stale = true;      // ring position of the dilated-dense history went in by value: one launch per step
  e->states_stale = !eager;              // (materialised on demand: states_materialize)
  if (!active) e->lazy_edited = false;   // (every stream stepped: every edited row has been consumed and replaced; masked steps: note_active)
  return NUTLS_OK;
}

// Before a step of any other mode: bring the device-side frame counter up to date if fused-mode steps ran since.
static int sync_step_counter(Engine* e, hipStream_t s) {
  if (e->d_step_stale && e->d_step) {
    HIP_TRY(launch_set_step(e->d_step, static_cast<int>(e->steps & 0x3fffffff), s));
    e->d_step_stale = false;
  }
  return NUTLS_OK;
}

static int capture_graphs(Engine* e) {
  for (int par = 0; par < 2; ++par) {
    if (e->gexec[par]) continue;
    hipGraph_t g = nullptr;
    HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    int rc = run_plan(e, par, e->stream);
    hipError_t ee = hipStreamEndCapture(e->stream, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }      // (a launch failed during capture: the half-built graph is not kept)
    if (ee != hipSuccess) { if (g) (void)hipGraphDestroy(g); return fail(NUTLS_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ee)); }
    hipError_t ie = hipGraphInstantiate(&e->gexec[par], g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ie != hipSuccess) return fail(NUTLS_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
  }
  return NUTLS_OK;
}

// ---- stream order ---------------------------------------------------------------------------
// The slow path of enqueue_on: this call names another stream than the last one.
int order_after_last(Engine* e, hipStream_t s) {
  if (e->last_stream != e->no_stream()) {
    if (!e->ev_order) HIP_TRY(hipEventCreateWithFlags(&e->ev_order, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(e->ev_order, e->last_stream));
    HIP_TRY(hipStreamWaitEvent(s, e->ev_order, 0));
  }
  e->last_stream = s;
  return NUTLS_OK;
}

// ---- frame bookkeeping ----------------------------------------------------------------------
// A frame of every stream has been enqueued: the next step writes the other parity.  The only place that flips the parity and counts frames.
void advance_frame(Engine* e) {
  e->next_parity = 1 - e->next_parity;
  e->steps += 1;
}

// Before the host reads or writes device memory the kernels keep (the state accessors, nutls_reset, nutls_debug_get): the handle's device,
// the lazily written states, and everything enqueued so far finished.
int host_access_begin(Engine* e) {
  HIP_TRY(hipSetDevice(e->device));
  if (int rcm = states_materialize(e, nullptr)) return rcm;      // (lazily written states: brought up to date before anything outside the kernel looks)
  HIP_TRY(hipDeviceSynchronize());
  enqueue_idle(e);
  return NUTLS_OK;
}

// A step of a per-layer mode (plain launches, graph replay, nutls_profile_step) is about to write the states on stream s: its kernels read
// the device-side frame counter and every conv-input state, and leave the fused kernel's carried partial sums behind.
int begin_per_layer_step(Engine* e, hipStream_t s) {
  if (int rc = sync_step_counter(e, s)) return rc;
  if (int rc = states_materialize(e, s)) return rc;      // (the per-layer kernels read every conv-input state)
  e->ys_dirty = true;
  return NUTLS_OK;
}

// ---- STFT front / back end state ---------------------------------------------------------------
// windows in float32 like tf.signal.hann_window (interpreter_proposed.py:20-26); twiddles e^{-2 pi i k / 512}, k = 0..255, from double
void frontend_tables(std::vector<float>* win_out, std::vector<float>* inv_out, std::vector<float>* tw_out) {
  std::vector<float> hann(NUTLS_FRAME_LEN), win(NUTLS_FRAME_LEN), inv(NUTLS_FRAME_LEN), tw(NUTLS_FRAME_LEN);
  for (int k = 0; k < NUTLS_FRAME_LEN; ++k) {
    const float arg = 6.28318530717958647692f * static_cast<float>(k) / static_cast<float>(NUTLS_FRAME_LEN);
    hann[k] = 0.5f - 0.5f * std::cos(arg);
  }
  win = hann;
  win[0] = 1e-7f; win[NUTLS_FRAME_LEN - 1] = 1e-7f;
  for (int k = 0; k < NUTLS_FRAME_LEN; ++k) {
    const int k2 = (k + NUTLS_FRAME_STEP) % NUTLS_FRAME_LEN;
    inv[k] = hann[k] / (hann[k] * hann[k] + hann[k2] * hann[k2]);
  }
  for (int k = 0; k < NUTLS_FRAME_LEN / 2; ++k) {
    const double a = -2.0 * 3.14159265358979323846 * k / NUTLS_FRAME_LEN;
    tw[2 * k] = static_cast<float>(std::cos(a));
    tw[2 * k + 1] = static_cast<float>(std::sin(a));
  }
  *win_out = win; *inv_out = inv;
  if (tw_out) *tw_out = tw;
}

int frontend_init(Engine* e) {
  if (e->fe_tail) return NUTLS_OK;
  const size_t hop = static_cast<size_t>(e->B) * NUTLS_FRAME_STEP;
  auto dalloc = [&](float** p, size_t n) -> int {
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, n * sizeof(float)));
    HIP_TRY(hipMemset(q, 0, n * sizeof(float)));
    e->allocs.push_back(q);
    *p = static_cast<float*>(q);
    return NUTLS_OK;
  };
  int rc;
  float* tail = nullptr;
  if ((rc = dalloc(&tail, hop)) || (rc = dalloc(&e->fe_ola, hop)) || (rc = dalloc(&e->fe_ph, static_cast<size_t>(e->B) * (NUTLS_FRAME_STEP + 1) * 2)) ||
      (rc = dalloc(&e->fe_win, NUTLS_FRAME_LEN)) || (rc = dalloc(&e->fe_inv, NUTLS_FRAME_LEN)) || (rc = dalloc(&e->fe_tw, NUTLS_FRAME_LEN)) ||
      (rc = dalloc(&e->fe_pcm_in, hop)) || (rc = dalloc(&e->fe_pcm_out, hop)))
    return rc;
  std::vector<float> win, inv, tw;
  frontend_tables(&win, &inv, &tw);
  const std::vector<float> twb = stft_block_twiddles();      // (the hop builds of the fused kernel: nutls_set_hop_fusion)
  if ((rc = dalloc(&e->fe_twb, twb.size()))) return rc;
  HIP_TRY(hipMemcpy(e->fe_twb, twb.data(), twb.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->fe_win, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->fe_inv, inv.data(), inv.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->fe_tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
  e->fe_tail = tail;
  return NUTLS_OK;
}

// ---- what this handle can do --------------------------------------------------------------------------------------------------------
// The causal32 CTFA of a streaming handle lives in the fused kernel only: the per-layer kernels compute the frame-mode attention and
// never write the history ring, so every path that would run them on such a handle refuses instead of mixing the two silently.
int refuse_per_layer_in_causal32(const Engine* e, const char* who) {
  if (e->ctfa_causal && !e->offline)
    return fail(NUTLS_ERR_ARG, std::string(who) + ": the causal32 CTFA of a streaming handle runs on the fused kernel (mode 3) only -- nutls_set_ctfa_mode(NUTLS_CTFA_FRAME) first");
  return NUTLS_OK;
}

// While hop fusion is on (nutls_set_hop_fusion) the handle stays what the single launch needs -- fused mode, production kernel: whatever would
// take it elsewhere refuses, so that an explicit request for one launch per hop never silently becomes three.
int refuse_in_hop_fusion(const Engine* e, const char* who) {
  if (e->hop_fusion)
    return fail(NUTLS_ERR_ARG, std::string(who) + ": not while hop fusion is on (the single-launch hop runs the fused production kernel) -- nutls_set_hop_fusion(h, 0) first");
  return NUTLS_OK;
}

// Where a per-stream active mask is supported: streaming handles of the LSTM variant on the fused kernel with the frame-mode CTFA.  Everything
// else keeps per-stream time in places a mask cannot reach (nutls.h, nutls_step_active) and refuses -- never a silent full step.
int check_active(const Engine* e, const char* who) {
  const std::string w = std::string(who) + ": a per-stream active mask ";
  if (e->offline) return fail(NUTLS_ERR_ARG, w + "needs a streaming handle (an offline handle steps whole blocks: nutls_process_block)");
  if (e->variant != NUTLS_VARIANT_LSTM)
    return fail(NUTLS_ERR_ARG, w + "is not supported for the baseline variant: its dilated-dense history rings are updated in place at a slot derived from the handle's frame counter");
  if (e->ctfa_causal)
    return fail(NUTLS_ERR_ARG, w + "is not supported with NUTLS_CTFA_CAUSAL32: the time-attention ring is addressed by the handle's frame counter -- nutls_set_ctfa_mode(NUTLS_CTFA_FRAME) first");
  if (e->mode != 3 || !e->fz_blob)
    return fail(NUTLS_ERR_ARG, w + "needs the fused kernel (mode 3): the per-layer plans and captured graphs of modes 0 / 1 are handle-wide");
  if (e->fz_stop_at >= 0) return fail(NUTLS_ERR_ARG, w + "cannot be combined with nutls_profile_production");
  return NUTLS_OK;
}

// Where the hop builds of the fused kernel exist: streaming handles of the LSTM variant in the fused mode on the one- or two-stream plan,
// production kernel (no activation trace, no stop twin).  Everything else refuses -- never a silent three-launch hop.
int check_hop_fusion(const Engine* e, const char* who) {
  const std::string w = std::string(who) + ": the single-launch hop ";
  if (e->offline) return fail(NUTLS_ERR_ARG, w + "needs a streaming handle (an offline handle takes PCM through nutls_enhance_block)");
  if (e->variant != NUTLS_VARIANT_LSTM) return fail(NUTLS_ERR_ARG, w + "is not built for the baseline variant (hop builds: LSTM variant, one- and two-stream plans)");
  if (e->mode != 3 || !e->fz_blob) return fail(NUTLS_ERR_ARG, w + "is a build of the fused kernel (mode 3): modes 0 / 1 run one kernel per layer -- nutls_set_mode(h, 3) first");
  if (!e->fz_plan->launch_hop)
    return fail(NUTLS_ERR_ARG, w + "is not built for the " + std::to_string(e->fz_plan->streams) + "-stream plan (nutls_create_plan(..., 1) or (..., 2))");
  if (e->fz_dbg) return fail(NUTLS_ERR_ARG, w + "runs the production kernel, the activation trace the profiling build -- nutls_debug_trace(h, 0) first");
  if (e->fz_stop_at >= 0) return fail(NUTLS_ERR_ARG, w + "cannot be combined with nutls_profile_production");
  return NUTLS_OK;
}

}  // namespace nutls

// =================================================================================================
//  C ABI
// =================================================================================================
using namespace nutls;

extern "C" {

const char* nutls_last_error(void) { return g_last_error.c_str(); }
const char* nutls_version(void) { return "nutls-hip 0.4 (gfx950; fused step: fp32 results on the bf16 matrix pipe)"; }

static int create_body(const void* weights, size_t n_bytes, int variant, int batch, int device, int offline_frames, nutls_handle** out, int streams_req) {
  if (!weights || !out || batch < 1) return fail(NUTLS_ERR_ARG, "nutls_create: null pointer or batch < 1");
  if (variant != NUTLS_VARIANT_LSTM && variant != NUTLS_VARIANT_BASELINE) return fail(NUTLS_ERR_ARG, "nutls_create: unknown variant");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(NUTLS_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(NUTLS_ERR_ARG, "nutls_create: device ordinal out of range");
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(NUTLS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
  WeightMap wm;
  std::string err;
  if (!parse_weight_blob(weights, n_bytes, &wm, &err)) return fail(NUTLS_ERR_WEIGHTS, err);
  std::unique_ptr<nutls_handle> h(new nutls_handle());
  Engine* e = &h->eng;
  e->B = batch;
  e->device = device;
  e->variant = variant;
  e->fz_plan = fused_plan(variant, 1);      // (until fused_setup chooses: what the handle-independent questions about "the plan" mean)
  e->off_bf16 = offline_frames > 0 && getenv("NUTLS_OFFLINE_FP32") == nullptr;      // (developer knob: block mode on the fp32-MFMA kernels)
  // (developer knobs of conv_choose: the small bf16 launches on the 1-wave kernels; the positions per launch from which the 128-position tiles run)
  if (const char* ev = getenv("NUTLS_OFFLINE_KSPLIT")) e->conv_knobs.ksplit = atoi(ev) != 0;
  if (const char* ev = getenv("NUTLS_CONV_TILE_MIN")) e->conv_knobs.tile_min = atoll(ev);
  HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  int rc;
  if ((rc = prep_weights(e, wm))) return rc;
  if ((rc = dev_alloc_once(e, 1, &e->d_step, true))) return rc;
  e->states.reserve(320);   // slot_reserve keeps pointers into this vector: it must never reallocate (130 or 208 states)
  if ((rc = build_states(e))) return rc;
  allocate_states(e);
  const size_t B = static_cast<size_t>(batch);
  if ((rc = dev_alloc(e, B * NUTLS_BINS, &e->io_in, true))) return rc;
  if ((rc = dev_alloc(e, B * NUTLS_BINS, &e->io_out, true))) return rc;
  slot_reserve(e, 256 * 64, &e->t_inlayer);
  slot_reserve(e, 256 * 64, &e->t_y);
  slot_reserve(e, 256 * 64, &e->t_d);
  slot_reserve(e, 256 * 128, &e->t_up);
  for (int s = 0; s < 6; ++s) slot_reserve(e, static_cast<size_t>(kDecoder[s].f0 / 2) * 128, &e->upcat[s]);
  if (offline_frames == 0) slot_reserve(e, static_cast<size_t>(2) * e->fz_plan->ys_block, &e->ysum);      // (streaming handles: the fused kernel's carried partial sums)
  if ((rc = arena_commit(e))) return rc;
  build_plan(e, 0);
  build_plan(e, 1);
  try {
    rc = upload_ddb_table(e);
  } catch (const std::exception& ex) {     // planning invariants (weights.cpp) are reported, never thrown through the C ABI
    return fail(NUTLS_ERR_ARG, std::string("plan: ") + ex.what());
  }
  if (rc) return rc;
  e->fz_streams_req = streams_req;
  e->n_cu = prop.multiProcessorCount;
  if (offline_frames == 0) {
    try {
      rc = fused_setup(e, wm);
    } catch (const std::exception& ex) {
      return fail(NUTLS_ERR_WEIGHTS, std::string("fused plan weights: ") + ex.what());
    }
    if (rc) return rc;
    if (e->fz_blob) {
      e->mode = 3;          // the default for streaming handles whose container holds int8 conv kernels
      // NUTLS_HOP_FUSION=1: the nutls_enhance_hop* entries of this handle run one launch per hop where a hop build exists (LSTM variant, one-
      // and two-stream plans) -- the switch nutls_set_hop_fusion turns, for callers that cannot be edited (bench.py --frontend); quietly off elsewhere
      if (const char* ev = getenv("NUTLS_HOP_FUSION")) {
        if (atoi(ev) != 0 && variant == NUTLS_VARIANT_LSTM && e->fz_plan->launch_hop) {
          if ((rc = frontend_init(e))) return rc;
          HIP_TRY(e->fz_plan->set_attributes_hop());
          e->hop_fusion = true;
        }
      }
    } else {
      // float containers: the per-layer kernels, replayed as a hipGraph -- the same default for C and Python callers
      if ((rc = capture_graphs(e))) return rc;
      e->mode = 1;
    }
  }
  e->debug["input_layer"] = {e->t_inlayer, 256 * 64};
  e->debug["msfe6_de.y"] = {e->t_y, 256 * 64};
  e->debug["msfe6_de.up"] = {e->t_up, 256 * 128};
  e->debug["msfe6_de.d"] = {e->t_d, 256 * 64};
  for (int s = 0; s < 6; ++s) e->debug[std::string(kDecoder[s].prefix) + ".upcat"] = {e->upcat[s], static_cast<size_t>(kDecoder[s].f0 / 2) * 128};
  if (offline_frames > 0) {
    e->offline = offline_frames;
    e->outt = batch / (offline_frames + 1);
    e->mode = 0;
    if ((rc = build_offline_plan(e))) return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  *out = h.release();
  return NUTLS_OK;
}

// (nothing may be thrown through the C ABI: a malformed container or an allocation failure is an error code)
static int create_common(const void* weights, size_t n_bytes, int variant, int batch, int device, int offline_frames, nutls_handle** out,
                         int streams_req = 0) {
  try {
    return create_body(weights, n_bytes, variant, batch, device, offline_frames, out, streams_req);
  } catch (const std::bad_alloc&) {
    return fail(NUTLS_ERR_WEIGHTS, "nutls_create: out of host memory (malformed weight container?)");
  } catch (const std::exception& ex) {
    return fail(NUTLS_ERR_WEIGHTS, std::string("nutls_create: ") + ex.what());
  }
}

int nutls_create(const void* weights, size_t n_bytes, int variant, int batch, int device, nutls_handle** out) {
  return create_common(weights, n_bytes, variant, batch, device, 0, out);
}

int nutls_create_plan(const void* weights, size_t n_bytes, int variant, int batch, int device, int streams_per_workgroup, nutls_handle** out) {
  if (streams_per_workgroup < 0) return fail(NUTLS_ERR_ARG, "nutls_create_plan: streams_per_workgroup must be 0 (library's choice), 1, 2 or 4");
  return create_common(weights, n_bytes, variant, batch, device, 0, out, streams_per_workgroup);
}

int nutls_create_offline(const void* weights, size_t n_bytes, int max_frames, int device, nutls_handle** out) {
  return nutls_create_offline_batch(weights, n_bytes, max_frames, 1, device, out);
}

int nutls_create_offline_batch(const void* weights, size_t n_bytes, int max_frames, int utterances, int device, nutls_handle** out) {
  if (max_frames < 1 || max_frames > 4096) return fail(NUTLS_ERR_ARG, "nutls_create_offline: max_frames must be 1..4096");
  if (utterances < 1 || utterances > 256) return fail(NUTLS_ERR_ARG, "nutls_create_offline_batch: utterances must be 1..256");
  if (static_cast<long long>(utterances) * max_frames > 65536) return fail(NUTLS_ERR_ARG, "nutls_create_offline_batch: utterances x max_frames must be <= 65536");
  // per utterance: one arena slot for the state carried in from the previous block, then max_frames slots for the frames of the block
  return create_common(weights, n_bytes, NUTLS_VARIANT_LSTM, utterances * (max_frames + 1), device, max_frames, out);
}

/* Streaming handles: the same choice for the fused kernel's CTFA (mode 3).  Causal32 keeps, outside the arena, the time attention of the
 * last 32 frames of every stream and stage; the sums over the 31 frames before the current one are formed by a small kernel in front of
 * the step (two launches per frame in this mode), the step itself is the same kernel. */
int nutls_set_ctfa_mode(nutls_handle* h, int mode) {
  if (!h) return fail(NUTLS_ERR_ARG, "nutls_set_ctfa_mode: null handle");
  if (h->eng.offline) return nutls_offline_set_ctfa_mode(h, mode);
  if (mode != NUTLS_CTFA_FRAME && mode != NUTLS_CTFA_CAUSAL32) return fail(NUTLS_ERR_ARG, "nutls_set_ctfa_mode: unknown mode");
  Engine* e = &h->eng;
  if (e->ctfa_causal == (mode == NUTLS_CTFA_CAUSAL32)) return NUTLS_OK;      // already in effect: the history stays
  if (mode == NUTLS_CTFA_CAUSAL32 && (!e->fz_blob || e->mode != 3))
    return fail(NUTLS_ERR_ARG, "nutls_set_ctfa_mode: the causal32 CTFA of a streaming handle runs on the fused kernel (mode 3) only");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t ring = static_cast<size_t>(e->B) * 12 * 32 * 64;
  if (mode == NUTLS_CTFA_CAUSAL32 && !e->fz_ta_ring) {
    int rc = dev_alloc(e, ring, &e->fz_ta_ring, true);
    if (!rc) rc = dev_alloc(e, static_cast<size_t>(e->B) * 12 * 64, &e->fz_ta_sum, true);
    if (rc) return rc;
  }
  if (e->fz_ta_ring) HIP_TRY(hipMemset(e->fz_ta_ring, 0, ring * sizeof(float)));      // a mode switch starts a new history
  e->ctfa_causal = mode == NUTLS_CTFA_CAUSAL32;
  return NUTLS_OK;
}

/* Attenuation limit (nutls.h): per row the pair (l, c = 1 - l) the mix kernels of the two syntheses read.  A control-plane call: everything is
 * checked first -- a refused call changes nothing --, then the device is synchronised and the array written.  While every row is 0 the
 * syntheses launch the kernels they always launched; the array is allocated by the first set that is not all zero. */
int nutls_set_atten_limit(nutls_handle* h, const float* limit, int n) {
  if (!h) return fail(NUTLS_ERR_ARG, "nutls_set_atten_limit: null handle");
  Engine* e = &h->eng;
  const int rows = e->offline ? e->outt : e->B;
  if (n != rows) return fail(NUTLS_ERR_ARG, "nutls_set_atten_limit: n = " + std::to_string(n) + ", the handle has " + std::to_string(rows) + " rows (streams / utterances)");
  bool on = false;
  for (int r = 0; limit && r < rows; ++r) {
    if (!(limit[r] >= 0.f && limit[r] <= 1.f))      // (a NaN fails both comparisons)
      return fail(NUTLS_ERR_ARG, "nutls_set_atten_limit: limit " + std::to_string(limit[r]) + " of row " + std::to_string(r) + " is outside 0 .. 1");
    on = on || limit[r] != 0.f;
  }
  if (on)
    if (int rc = refuse_in_hop_fusion(e, "nutls_set_atten_limit")) return rc;      // (the one-launch hop builds have no mix)
  if (!on && !e->d_atten) return NUTLS_OK;                                         // all zero on a handle that never had a limit: nothing to write
  std::vector<float> lc(static_cast<size_t>(rows) * 2);
  for (int r = 0; r < rows; ++r) {
    const float l = limit ? limit[r] + 0.f : 0.f;                                  // (-0 becomes +0)
    lc[2 * static_cast<size_t>(r)] = l;
    lc[2 * static_cast<size_t>(r) + 1] = static_cast<float>(1.0 - static_cast<double>(l));
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  if (int rc = dev_alloc_once(e, lc.size(), &e->d_atten, false)) return rc;
  HIP_TRY(hipMemcpy(e->d_atten, lc.data(), lc.size() * sizeof(float), hipMemcpyHostToDevice));
  e->atten.resize(static_cast<size_t>(rows));
  for (int r = 0; r < rows; ++r) e->atten[static_cast<size_t>(r)] = lc[2 * static_cast<size_t>(r)];
  e->atten_on = on;
  return NUTLS_OK;
}

int nutls_atten_limit(nutls_handle* h, float* limit, int n) {
  if (!h || !limit) return fail(NUTLS_ERR_ARG, "nutls_atten_limit: null pointer");
  const Engine* e = &h->eng;
  const int rows = e->offline ? e->outt : e->B;
  if (n != rows) return fail(NUTLS_ERR_ARG, "nutls_atten_limit: n = " + std::to_string(n) + ", the handle has " + std::to_string(rows) + " rows (streams / utterances)");
  for (int r = 0; r < rows; ++r) limit[r] = e->atten.empty() ? 0.f : e->atten[static_cast<size_t>(r)];
  return NUTLS_OK;
}

int nutls_destroy(nutls_handle* h) {
  if (!h) return NUTLS_OK;
  (void)hipSetDevice(h->eng.device);
  (void)hipDeviceSynchronize();
  delete h;
  return NUTLS_OK;
}

int nutls_batch(nutls_handle* h) { return h ? h->eng.B : fail(NUTLS_ERR_ARG, "null handle"); }
int nutls_streams_per_workgroup(nutls_handle* h) { return h ? (h->eng.fz_blob ? h->eng.fz_plan->streams : 1) : fail(NUTLS_ERR_ARG, "null handle"); }
int nutls_launches_per_step(nutls_handle* h) { return h ? static_cast<int>(h->eng.plan[0].size()) : fail(NUTLS_ERR_ARG, "null handle"); }

int nutls_io_buffers(nutls_handle* h, float** mag_in, float** mag_out) {
  if (!h || !mag_in || !mag_out) return fail(NUTLS_ERR_ARG, "nutls_io_buffers: null pointer");
  *mag_in = h->eng.io_in;
  *mag_out = h->eng.io_out;
  return NUTLS_OK;
}

int nutls_use_graph(nutls_handle* h, int enable) {
  if (!h) return fail(NUTLS_ERR_ARG, "null handle");
  Engine* e = &h->eng;
  if (int rc = refuse_in_hop_fusion(e, "nutls_use_graph")) return rc;
  if (int rc = refuse_per_layer_in_causal32(e, "nutls_use_graph")) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if (enable) {
    int rc = capture_graphs(e);
    if (rc) return rc;
  }
  e->mode = enable ? 1 : 0;
  return NUTLS_OK;
}

int nutls_set_mode(nutls_handle* h, int mode) {
  if (!h || mode < 0 || mode > 3) return fail(NUTLS_ERR_ARG, "nutls_set_mode: mode must be 0, 1 or 3");
  if (mode == 2) return fail(NUTLS_ERR_ARG, "nutls_set_mode: mode 2 (the plan-interpreter kernel of rounds 1-3) was retired: 3 = fused kernel, 1 / 0 = one kernel per layer");
  if (mode == 3 && !h->eng.fz_blob)
    return fail(NUTLS_ERR_ARG, "nutls_set_mode: mode 3 (fused kernel) needs a streaming handle made from a container with int8 conv kernels" +
                                   (h->eng.fz_reason.empty() ? std::string() : " (" + h->eng.fz_reason + ")"));
  if (h->eng.offline && mode != 0) return fail(NUTLS_ERR_ARG, "nutls_set_mode: offline handles run per-layer launches (mode 0)");
  if (mode != 3)
    if (int rc = refuse_in_hop_fusion(&h->eng, "nutls_set_mode")) return rc;
  if (mode != 3)
    if (int rc = refuse_per_layer_in_causal32(&h->eng, "nutls_set_mode")) return rc;
  if (mode == 1) return nutls_use_graph(h, 1);
  h->eng.mode = mode;
  return NUTLS_OK;
}

}  // extern "C"
