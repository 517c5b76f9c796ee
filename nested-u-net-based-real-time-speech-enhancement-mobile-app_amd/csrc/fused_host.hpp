// What the host knows about a static plan of the fused frame-step kernel (fused_plan_*.inc): one immutable descriptor per plan.
// Host only: fused_host.cpp and, through engine.hpp, the five files of the host engine (engine.cpp, api_stream.cpp, api_block.cpp, api_state.cpp,
// api_profile.cpp) include it, no kernel translation unit does (an edit here re-compiles no kernel).
#pragma once

#include "nutls_internal.hpp"

namespace nutls {
namespace fz { struct OpD; }      // fused_plan.hpp

// (the generated BlobItem / StateOff of a plan file, which are types of that plan's namespace: fused_host_impl.inc copies them into these)
struct FusedBlobItem { int off, floats, what, op; const char* key; };      // what: 0 conv fragments, 1 conv params, 2 lstm, 3 ctfa, 4 input layer
struct FusedOff { const char* name; int off; };

struct FusedPlan {
  int variant, streams;                // NUTLS_VARIANT_*, streams per workgroup (1: the plan every handle can run; 2 / 4: packed plans, OpD::gs)
  int num_ops, blob_floats;
  // arena layout the plan addresses.  The packed plans share the one-stream plan's (checked in fused_setup); the blob and the layout of the
  // carried partial sums inside their blocks are the plan's own.
  int arena_floats, parity_stride;
  int ys_off, ys_block;                // arena offset of the first block of carried partial sums, floats of one block (the "ysum" scratch holds two)
  const fz::OpD* ops;                  // [num_ops]
  const char* const* op_names;
  const double* op_flops;
  const int (*seg_tk)[6];              // per op: (time tap << 2 | frequency tap) of its K segments
  const FusedBlobItem* blob_items; int num_blob_items;
  const FusedOff* states; int num_states, num_pingpong;      // the first num_pingpong states are ping-pong pairs, the rest in-place history rings
  const FusedOff* scratch; int num_scratch;
  // the plan's kernel (each dispatches to its profiling twin itself when `prof` is non-null)
  decltype(&launch_fused_step) launch;
  hipError_t (*set_attributes)();
  // the plan's hop build (FZ_HOP: STFT analysis and inverse STFT inside the launch, nutls_set_hop_fusion), null where none is built
  decltype(&launch_fused_step) launch_hop;
  hipError_t (*set_attributes_hop)();
};

// The plans that exist: 1 / 2 / 4 streams per workgroup for the LSTM variant, 1 for the baseline.  nullptr: no such plan.
const FusedPlan* fused_plan(int variant, int streams);

// Weight blob of the plan's kernel, in plan order -> FusedPack (nutls_internal.hpp); `err` says which tensor
int fused_pack_blob(const FusedPlan& p, const WeightMap& wm, std::vector<float>* out, std::string* err);
// the table launch_ysum_refresh needs (w: all ops' tap-0 weights, int8 values as floats); false + err if a tensor has no int8 payload
bool fused_ys_table(const FusedPlan& p, const WeightMap& wm, std::vector<YsOp>* ops, std::vector<float>* w, std::string* err);
// the state tensors a launch of the plan leaves unwritten unless asked for eager states (empty when the plan writes every state)
void fused_lazy_table(const FusedPlan& p, std::vector<LazyCopy>* tab);

}  // namespace nutls
