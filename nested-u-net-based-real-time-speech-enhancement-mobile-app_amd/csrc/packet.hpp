// Packet mode of the PCM gateway (nutls_set_pcm_packet, the _packet entries of nutls.h): what a handle keeps for it and the launcher of the
// re-framing kernels (packet.hip).  The callers' packets of P samples are cut into the model's hops of S samples and back on the device: per
// stream an input FIFO and an output FIFO, byte rings of S - g + P samples each, g = gcd(P, S).
//
// The kernels move bytes and know nothing of sample types: every length and position here is in QUADS of 16 bytes.  S * bytes is a multiple
// of 128 and P * bytes a multiple of 16 (the length rule of nutls_pcm_packet_plan exists for this), so g * bytes, every ring position and
// the ring length are multiples of 16: every access is one aligned 16-byte vector access that never straddles the wrap.
//
// The arithmetic (nutls.h, "Packet mode"): the output FIFO starts with D = S - g samples of silence; after every tick fill_in + fill_out = D,
// and between a tick's push and its pop fill_in + fill_out = D + P -- so ONE counter per stream, fill_in, describes both FIFOs.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

namespace nutls {

constexpr int kPacketMaxRounds = 4;      // hop rounds of a tick at the most: P <= 4 S

// Per stream, on the device (16 bytes: one vector access): quads waiting in the input FIFO, the read positions of the two rings.
struct PacketCtr {
  int fill, in_rd, out_rd, pad;
};

// What a streaming handle keeps for packet mode, next to PcmState.  Lengths in samples describe the contract, lengths in quads the kernels.
struct PacketState {
  int P = 0;                           // the packet length in samples; 0: off
  int S = 0, D = 0, R = 0, L = 0;      // while on: the hop, the priming S - g, the rounds a tick can take, the ring length S - g + P
  int bytes = 0;                       // of a sample
  unsigned silence = 0;                // the silence word: 0, 0xFFFFFFFF (mu-law) or 0xD5D5D5D5 (A-law)
  unsigned char *in_ring = nullptr, *out_ring = nullptr;      // [B][L * bytes]
  size_t ring_cap = 0;                 // bytes each ring was allocated with (they grow with the largest packet a handle has been set to)
  unsigned char *hop_in = nullptr, *hop_out = nullptr;        // [B][S * bytes]: the library's hop buffers, what the hop entry reads and writes
  size_t hop_cap = 0;
  unsigned char *raw_in = nullptr, *raw_out = nullptr;        // [B][P * bytes]: staging of the _host entry
  size_t raw_cap = 0;
  PacketCtr* ctr = nullptr;            // [B]: the authoritative counters
  unsigned char* ready = nullptr;      // [B]: the ready mask of the current round, formed by the kernels
  // The host's mirror of ctr[b].fill, in samples: kept for as long as the host has seen every mask (active == NULL, or the _host entry).
  // A DEVICE mask makes it unknown; nutls_reset(h, -1) and nutls_set_pcm_packet make it known again.
  std::vector<int> mirror;
  bool mirror_known = false;
  int last_rounds = 0;                 // hop rounds the last packet call issued
};

// The three bodies of a tick, fused so that a tick of r rounds is r + 1 launches beside its r hops:
//   kPushStage  append the packet; rows with a whole hop waiting get it copied to hop_in and their ready byte set       (in front of round 0)
//   kTurn       ready rows: append hop_out to the output ring, take the hop off the input FIFO; stage the next round    (between two rounds)
//   kTurnPop    the last round's turn without a next stage, then P samples to pcm_out -- held rows: the silence word   (behind the last round)
//   kPushPop    a tick of no rounds: push and pop in one launch
enum class PacketBody { kPushStage, kTurn, kTurnPop, kPushPop };

// One launch: rows workgroup-independent, one wavefront per row.  Everything in quads; `active` (device, [rows], may be null: all rows) is read
// by the bodies that push or pop, `ready` by every body.  pcm_in is read by the pushing bodies, pcm_out written by the popping ones.
struct PacketLaunch {
  const void* pcm_in;
  void* pcm_out;
  const unsigned char* active;
  unsigned char *in_ring, *out_ring, *hop_in, *hop_out;
  PacketCtr* ctr;
  unsigned char* ready;
  int rows, Pq, Sq, Dq, Lq;
  unsigned silence;
};
hipError_t launch_packet(PacketBody body, const PacketLaunch& L, hipStream_t s);

}  // namespace nutls
