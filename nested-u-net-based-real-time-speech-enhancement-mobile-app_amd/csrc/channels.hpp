// Channels of the PCM gateway (nutls_set_pcm_channels, nutls.h "Channels"): what a handle keeps for it and the launcher of the split / join
// kernels (channels.hip).  A handle told "C channels" takes and returns frame rows [rows / C][n * C] on the callers' side of every _pcm entry:
// channel c of frame row r is stream r * C + c.  A split makes the stream rows [rows][n] of a frame buffer in front of the entry's
// existing path, a join makes the frame rows of its result behind it; everything between is the 1-channel code on library buffers.
//
// The kernels move bytes: they know sample sizes (1, 2, 4 bytes) but not sample types, and every length here is in QUADS of 16 bytes.  S * bytes
// is a multiple of 128 and P * bytes a multiple of 16, so a stream row is a whole number of quads, and the C quads j * C .. j * C + C - 1 of a
// frame row hold exactly the 16 / bytes frames whose samples are quad j of each of the row's C streams.
#pragma once

#include <hip/hip_runtime.h>

namespace nutls {

// What a handle keeps for the setting: the channel count in force and the two library buffers [rows][n * bytes] between which the 1-channel
// path runs -- `split` holds the stream rows of the callers' input, `join` the stream rows of the result.  They grow with the largest request
// the handle has seen (`cap` bytes each), sized when an entry needs them.
struct ChannelState {
  int C = 1;
  unsigned char *split = nullptr, *join = nullptr;
  size_t cap = 0;
};

// One launch.  frames: [frame_rows][C * q] quads, interleaved; rows: [frame_rows * C][q] quads, one row per stream.  A split reads `frames`
// and writes `rows`, a join the reverse; the two must not overlap.
struct ChannelsLaunch {
  const void* in;
  void* out;
  int frame_rows;      // rows / C
  int q;               // quads of one stream's row
};
// bytes: 1, 2 or 4 (of a sample); channels: 2 or 4; anything else, or a length below 1, is hipErrorInvalidValue and nothing is launched.
hipError_t launch_channels(int bytes, int channels, bool join, const ChannelsLaunch& L, hipStream_t s);

}  // namespace nutls
