// The arithmetic the analysis streams share (pyin_stream.hip, loudness_stream.hip): frames of 2 W samples
// every hop, frame t covering [hop t - W, hop t + W) of the row padded by reflection, computed as soon as all its samples exist.
#pragma once

namespace {

// F(n): frames computed after n samples (frame 0's reflection reads sample W, hence n > W)
__host__ __device__ inline long long frames_done(long long n, int W, int hop) { return n <= W ? 0 : 1 + (n - W) / hop; }

// first sample the history keeps: what the frames still to come need, and what a flush reflects about n
__host__ __device__ inline long long hist_start(long long n, int W, int hop) {
  const long long a = hop * frames_done(n, W, hop) - W, b = n - W - 1;
  const long long s = a < b ? a : b;
  return s < 0 ? 0 : s;
}

}  // namespace
