// What the S2S decoder's forward recurrence (aligner.hip) and its backward (aligner_train.hip) share: the geometry of
// one decoder workgroup, the fixed-order workgroup reduction and the location conv over one tile of frames.
#pragma once
#include <hip/hip_runtime.h>

namespace s2s {

constexpr int DT = 512;                    // threads
constexpr int DH = 128;                    // decoder_rnn_dim = attention_dim = memory width
constexpr int DF = 32, DK = 63, DP = 31;   // location conv: filters, taps, padding
constexpr int DTL = 128;                   // frames per location-conv tile
constexpr int DSTRIP = 8;                  // frames per thread of the location conv

// frames rounded up to whole tiles, and the padded length of a weights array (frame l at [DP + l], zeros around)
constexpr int tiles_up(int L) { return (L + DTL - 1) / DTL * DTL; }
constexpr int padded(int L) { return tiles_up(L) + 2 * DP; }

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// sum / max over the workgroup in a fixed order: a butterfly inside each wave, then the waves' values in wave order.
// red holds one float per wave; two barriers, so red can be reused right after.
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const float o = __shfl_xor(v, s);
    v = MAX ? fmaxf(v, o) : v + o;
  }
  const int nw = (int)(blockDim.x >> 6);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < nw; ++w) r = MAX ? fmaxf(r, red[w]) : r + red[w];
  __syncthreads();
  return r;
}

// location conv of the frames [l0, l0 + DTL) into s_conv[frame - l0][DF + 1]: thread (f, strip) owns DSTRIP frames of
// filter f; s_wp / s_wc are the padded previous / cumulative weights, s_wloc the taps [2][DK][DF].  The caller
// synchronises.
__device__ __forceinline__ void loc_conv_tile(const float* s_wp, const float* s_wc, const float* s_wloc, int l0, int L,
                                              float* s_conv) {
  const int tid = threadIdx.x;
  const int f = tid & (DF - 1), strip = tid >> 5, lb = l0 + strip * DSTRIP;
  if (lb < L) {
    float acc[DSTRIP] = {};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float* arr = (c ? s_wc : s_wp) + lb;  // arr[j + k] = frame lb + j + k - DP
      float win[DSTRIP + DK - 1];
#pragma unroll
      for (int j = 0; j < DSTRIP + DK - 1; ++j) win[j] = arr[j];
#pragma unroll
      for (int k = 0; k < DK; ++k) {
        const float w = s_wloc[(c * DK + k) * DF + f];
#pragma unroll
        for (int j = 0; j < DSTRIP; ++j) acc[j] = fmaf(w, win[j + k], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < DSTRIP; ++j) s_conv[(strip * DSTRIP + j) * (DF + 1) + f] = acc[j];
  }
}

}  // namespace s2s
