// Channels of the PCM gateway (channels.hpp; nutls.h, "Channels"): the kernels that split the callers' interleaved frame rows into one row per
// stream and join them back.  They move bytes and know nothing of sample types: the sample size is a template argument, lengths are in quads
// of 16 bytes.
//
// Shape: a lane owns quad j of the C streams of one frame row.  Split: it loads the C consecutive quads j * C .. j * C + C - 1 of the frame
// row -- 16 / BYTES whole frames --, rearranges their elements in registers (every index below is a compile-time constant once the loops are
// unrolled: no LDS, no atomics, no array in scratch) and stores quad j of each of the C stream rows.  Join is the same body with source and
// destination exchanged.  Every global access is ONE aligned 16-byte load or store; a lane's C accesses on the frame side are consecutive,
// on the stream side one row apart, where the lanes of a wavefront are consecutive.  Grid: chunks of kChunk quads in x (the last one partly
// filled), frame rows in y.  Row offsets are size_t.
#include "channels.hpp"

namespace nutls {

namespace {

constexpr int kChunk = 256;             // quads of a stream row per workgroup: one per lane
constexpr int kMaxGridY = 65535;

// element e (of BYTES bytes) of the words w[], e a constant
template <int BYTES>
__device__ __forceinline__ unsigned element(const unsigned* w, int e) {
  if constexpr (BYTES == 4) return w[e];
  else if constexpr (BYTES == 2) return (w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
  else return (w[e >> 2] >> ((e & 3) * 8)) & 0xFFu;
}

template <int BYTES, int C, bool JOIN>
__global__ __launch_bounds__(kChunk) void channels_kernel(const ChannelsLaunch L) {
  constexpr int E = 16 / BYTES;        // elements of a quad = frames a lane moves
  constexpr int PER_WORD = 4 / BYTES;
  const int j = static_cast<int>(blockIdx.x) * kChunk + static_cast<int>(threadIdx.x);
  if (j >= L.q) return;
  const size_t q = static_cast<size_t>(L.q), base = static_cast<size_t>(blockIdx.y) * C * q;      // both sides: the frame row's first quad
  const size_t at_frames = base + static_cast<size_t>(j) * C, at_rows = base + static_cast<size_t>(j);
  const uint4* const src = reinterpret_cast<const uint4*>(L.in) + (JOIN ? at_rows : at_frames);
  uint4* const dst = reinterpret_cast<uint4*>(L.out) + (JOIN ? at_frames : at_rows);
  const size_t src_step = JOIN ? q : 1, dst_step = JOIN ? 1 : q;

  unsigned in[4 * C], out[4 * C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const uint4 v = src[c * src_step];
    in[4 * c + 0] = v.x;
    in[4 * c + 1] = v.y;
    in[4 * c + 2] = v.z;
    in[4 * c + 3] = v.w;
  }
  // Destination element d of the lane's C quads.  Split: d = c * E + i (stream c, sample i) comes from frame element i * C + c;
  // join: d = i * C + c comes from stream element c * E + i.
#pragma unroll
  for (int w = 0; w < 4 * C; ++w) {
    unsigned word = 0;
#pragma unroll
    for (int t = 0; t < PER_WORD; ++t) {
      const int d = w * PER_WORD + t;
      const int from = JOIN ? (d % C) * E + d / C : (d % E) * C + d / E;
      word |= element<BYTES>(in, from) << (t * 8 * BYTES % 32);
    }
    out[w] = word;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) dst[c * dst_step] = make_uint4(out[4 * c + 0], out[4 * c + 1], out[4 * c + 2], out[4 * c + 3]);
}

template <int BYTES, int C>
void launch(bool join, const dim3& grid, const ChannelsLaunch& L, hipStream_t s) {
  if (join) hipLaunchKernelGGL((channels_kernel<BYTES, C, true>), grid, dim3(kChunk), 0, s, L);
  else hipLaunchKernelGGL((channels_kernel<BYTES, C, false>), grid, dim3(kChunk), 0, s, L);
}

template <int BYTES>
void launch(int channels, bool join, const dim3& grid, const ChannelsLaunch& L, hipStream_t s) {
  if (channels == 2) launch<BYTES, 2>(join, grid, L, s);
  else launch<BYTES, 4>(join, grid, L, s);
}

}  // namespace

hipError_t launch_channels(int bytes, int channels, bool join, const ChannelsLaunch& L, hipStream_t s) {
  if ((bytes != 1 && bytes != 2 && bytes != 4) || (channels != 2 && channels != 4) || !L.in || !L.out || L.frame_rows < 1 || L.q < 1) return hipErrorInvalidValue;
  const unsigned chunks = static_cast<unsigned>((L.q + kChunk - 1) / kChunk);
  const size_t row_bytes = static_cast<size_t>(channels) * L.q * 16;      // of a frame row, on either side
  for (int first = 0; first < L.frame_rows; first += kMaxGridY) {        // (grid.y holds 65535 rows: more take another launch)
    ChannelsLaunch part = L;
    part.in = static_cast<const unsigned char*>(L.in) + first * row_bytes;
    part.out = static_cast<unsigned char*>(L.out) + first * row_bytes;
    part.frame_rows = L.frame_rows - first < kMaxGridY ? L.frame_rows - first : kMaxGridY;
    const dim3 grid(chunks, static_cast<unsigned>(part.frame_rows));
    if (bytes == 1) launch<1>(channels, join, grid, part, s);
    else if (bytes == 2) launch<2>(channels, join, grid, part, s);
    else launch<4>(channels, join, grid, part, s);
  }
  return hipGetLastError();
}

}  // namespace nutls
