// Packet mode of the PCM gateway (packet.hpp; nutls.h, "Packet mode"): the kernels that re-frame the callers' packets into the model's hops and
// back.  They move bytes between five places -- the callers' packet rows, the two rings, the library's two hop buffers -- and know nothing of
// sample types: lengths and positions are in quads of 16 bytes, the silence word is an argument.
//
// Alignment, and why the length rule of nutls_pcm_packet_plan exists: S * bytes is a multiple of 128 and P * bytes a multiple of 16, so
// g * bytes (g = gcd(P, S)), every ring position and the ring length (S - g + P) * bytes are multiples of 16.  Every access below is therefore ONE
// aligned 16-byte vector load or store, and a quad never straddles the wrap of a ring: the wrap is a whole-quad index modulo Lq.
//
// Shape: rows are independent -- one wavefront per row, kRowsPerGroup rows per workgroup, no LDS, no atomics, nothing between workgroups.  A
// row's counters are read once by every lane (one 16-byte load of the same address) and written back by lane 0.  No body reads through the
// rings what the same launch wrote there: where a hop or a packet is made of quads that were waiting AND of quads that arrive in this launch,
// the latter are taken from where they come from (the packet row, the hop buffer), so no launch depends on the order of its own stores and
// loads.  Row offsets are size_t.
#include "packet.hpp"

namespace nutls {

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerGroup = 4;

// PUSH: append the packet to the input ring.  TURN: for a ready row, append hop_out to the output ring and take the hop off the input FIFO.
// STAGE: rows with a whole hop waiting get it copied to hop_in, and every row its ready byte.  POP: the oldest P samples of the output FIFO to
// pcm_out, the silence word for a held row.  The four combinations that exist: PacketBody.
template <bool PUSH, bool TURN, bool STAGE, bool POP>
__global__ __launch_bounds__(kWave* kRowsPerGroup) void packet_kernel(const PacketLaunch L) {
  const int lane = static_cast<int>(threadIdx.x) & (kWave - 1);
  const int row = static_cast<int>(blockIdx.x) * kRowsPerGroup + (static_cast<int>(threadIdx.x) >> 6);
  if (row >= L.rows) return;
  const int Pq = L.Pq, Sq = L.Sq, Lq = L.Lq;
  const size_t r = static_cast<size_t>(row);
  uint4* const in_ring = reinterpret_cast<uint4*>(L.in_ring) + r * Lq;
  uint4* const out_ring = reinterpret_cast<uint4*>(L.out_ring) + r * Lq;
  uint4* const hop_in = reinterpret_cast<uint4*>(L.hop_in) + r * Sq;
  const uint4* const hop_out = reinterpret_cast<const uint4*>(L.hop_out) + r * Sq;
  const uint4* const pkt_in = reinterpret_cast<const uint4*>(L.pcm_in) + r * Pq;      // (formed, not read, where the body does not push)
  uint4* const pkt_out = reinterpret_cast<uint4*>(L.pcm_out) + r * Pq;
  const bool act = (PUSH || POP) ? (!L.active || L.active[row] != 0) : false;
  PacketCtr c = L.ctr[row];
  bool dirty = false;
  int appended_at = Lq + Pq;      // POP: quads of the output FIFO from this position on are still in hop_out (a TURN of this launch); beyond reach: none

  if (PUSH) {
    bool ready = false;
    if (act) {
      const int wr = (c.in_rd + c.fill) % Lq;
      for (int k = lane; k < Pq; k += kWave) in_ring[(wr + k) % Lq] = pkt_in[k];
      if (STAGE && c.fill + Pq >= Sq) {      // round 0: the quads that were waiting, then the head of this packet
        ready = true;
        for (int k = lane; k < Sq; k += kWave) hop_in[k] = k < c.fill ? in_ring[(c.in_rd + k) % Lq] : pkt_in[k - c.fill];
      }
      c.fill += Pq;
      dirty = true;
    }
    if (STAGE && lane == 0) L.ready[row] = ready ? 1 : 0;
  }

  if (TURN) {
    if (L.ready[row] != 0) {      // (the hop of this round has run behind the launch that set the byte: same stream)
      const int have = L.Dq + Pq - c.fill;      // quads in the output FIFO: between push and pop fill_in + fill_out = D + P
      const int wr = (c.out_rd + have) % Lq;
      for (int k = lane; k < Sq; k += kWave) out_ring[(wr + k) % Lq] = hop_out[k];
      if (POP) appended_at = have;
      c.fill -= Sq;
      c.in_rd = (c.in_rd + Sq) % Lq;
      dirty = true;
      if (STAGE) {      // the next round: a row can be ready in it only if it was in this one
        const bool next = c.fill >= Sq;
        if (next)
          for (int k = lane; k < Sq; k += kWave) hop_in[k] = in_ring[(c.in_rd + k) % Lq];
        if (lane == 0) L.ready[row] = next ? 1 : 0;
      }
    }
  }

  if (POP) {
    if (act) {
      for (int k = lane; k < Pq; k += kWave) pkt_out[k] = k < appended_at ? out_ring[(c.out_rd + k) % Lq] : hop_out[k - appended_at];
      c.out_rd = (c.out_rd + Pq) % Lq;
      dirty = true;
    } else {
      const uint4 sil = make_uint4(L.silence, L.silence, L.silence, L.silence);
      for (int k = lane; k < Pq; k += kWave) pkt_out[k] = sil;
    }
  }

  if (dirty && lane == 0) L.ctr[row] = c;
}

}  // namespace

hipError_t launch_packet(PacketBody body, const PacketLaunch& L, hipStream_t s) {
  if (L.rows < 1 || L.Pq < 1 || L.Sq < 1 || L.Lq < L.Pq || L.Lq < L.Sq || L.Dq < 0 || L.Dq + L.Pq != L.Lq) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>((L.rows + kRowsPerGroup - 1) / kRowsPerGroup)), block(kWave * kRowsPerGroup);
  switch (body) {
    case PacketBody::kPushStage: hipLaunchKernelGGL((packet_kernel<true, false, true, false>), grid, block, 0, s, L); break;
    case PacketBody::kTurn: hipLaunchKernelGGL((packet_kernel<false, true, true, false>), grid, block, 0, s, L); break;
    case PacketBody::kTurnPop: hipLaunchKernelGGL((packet_kernel<false, true, false, true>), grid, block, 0, s, L); break;
    case PacketBody::kPushPop: hipLaunchKernelGGL((packet_kernel<true, false, false, true>), grid, block, 0, s, L); break;
  }
  return hipGetLastError();
}

}  // namespace nutls
