// Included by fused_host.cpp once per plan, inside that plan's namespace (where `fz::` is the plan file): the plan's generated tables as a
// FusedPlan.  Everything else the host does with a plan -- the blob packer among it -- is compiled once, in fused_host.cpp.
const FusedPlan* describe(int variant, decltype(FusedPlan::launch) launch, hipError_t (*set_attributes)(), decltype(FusedPlan::launch) launch_hop = nullptr,
                          hipError_t (*set_attributes_hop)() = nullptr) {
  static const std::vector<FusedBlobItem> items = copy_items(fz::kBlobItems);
  static const std::vector<FusedOff> states = copy_offs(fz::kStateOffs), scratch = copy_offs(fz::kScratchOffs);
  static const FusedPlan plan{variant, fz::kStreams, fz::kNumOps, fz::kBlobFloats, fz::kArenaFloats, fz::kParityStride, fz::kYsOff, fz::kYsBlock,
                              fz::kOps, fz::kOpNames, fz::kOpFlops, fz::kSegTk, items.data(), fz::kNumBlobItems, states.data(), fz::kNumStateOffs,
                              fz::kNumPingPong, scratch.data(), static_cast<int>(scratch.size()), launch, set_attributes, launch_hop, set_attributes_hop};
  return &plan;
}
