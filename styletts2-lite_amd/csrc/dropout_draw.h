// The counter draw of train-mode dropout, shared by stts_dropout (trainops.hip) and the fused forms of
// aligner_cnn_train.hip: one definition, so a fused kernel keeps flat element i of a tensor exactly when
// stts_dropout(seed) keeps element i of the same tensor (the fused result is bitwise the unfused pair).
#pragma once
#include <hip/hip_runtime.h>

namespace drop {

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {  // splitmix64's finaliser
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// keep element i when its counter draw u(seed, i) >= p
__device__ __forceinline__ bool keep(unsigned long long seed, long long i, float p) {
  const unsigned long long z = mix64(seed ^ mix64((unsigned long long)i * 0xD1B54A32D192ED03ULL));
  return (float)(z >> 40) * (1.0f / 16777216.0f) >= p;
}

}  // namespace drop
