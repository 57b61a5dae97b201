// Pitch extractor (Modules/JDC/model.py JDCNet, eval mode) and the log-norm target (utils.py:48-53) of the
// training step (train.py:260-262): the pieces around the conv engine and the BiLSTM recurrence.
//   k_mel_to_padded_t    mel [B][1][nb][T] -> the zero-padded (T x nb) image the convs read (the reference
//                        transposes the mel first: model.py:112)
//   k_bn_affine          pack time: BatchNorm running statistics -> per-channel (scale, shift)
//   k_bn_lrelu_maxpool   ResBlock.pre_conv / pool_block: BatchNorm -> LeakyReLU -> MaxPool2d((1, p)) in one pass,
//                        into the next padded image; the last block also writes the BiLSTM input and the
//                        reference's GAN_feature / poolblock_out layouts
//   k_linear_abs         classifier Linear(512, num_class) + abs
//   k_log_norm           log(|| exp(x std + mean) ||_2) over the mel bins
// All of them are memory-bound streams over a few MB: 16-byte accesses along the channel axis, no atomics, every
// sum in a fixed order.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NT = 256;

unsigned grid_of(long long n) {
  const long long g = (n + NT - 1) / NT;
  return (unsigned)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

template <typename T>
__global__ void __launch_bounds__(NT) k_mel_to_padded_t(const float* __restrict__ mel, int B, int nb, int Tn,
                                                        T* __restrict__ dst) {
  const long long n = (long long)B * nb * Tn;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int t = (int)(i % Tn), w = (int)((i / Tn) % nb), b = (int)(i / ((long long)Tn * nb));
    const size_t row = (size_t)b * (Tn + 2) * (nb + 2) + (size_t)(t + 1) * (nb + 2) + (w + 1);
    dst[row * 8] = from_f32<T>(mel[i]);
  }
}

__global__ void __launch_bounds__(NT) k_bn_affine(const float* __restrict__ w, const float* __restrict__ b,
                                                  const float* __restrict__ mean, const float* __restrict__ var, int C,
                                                  float eps, float* __restrict__ ab) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= C) return;
  const float a = w[c] / sqrtf(var[c] + eps);
  ab[c] = a;
  ab[C + c] = b[c] - mean[c] * a;
}

__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void store8(bf16_t* p, const float (&v)[8]) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16_t)v[j];
  *reinterpret_cast<bf16x8*>(p) = o;
}

// One thread per (utterance, padded output pixel, 8 channels).  Border pixels of y are written as zeros, so the
// image needs no clearing before this launch.
template <typename T>
__global__ void __launch_bounds__(NT) k_bn_lrelu_maxpool(const T* __restrict__ x, int B, int H, int W, int C,
                                                         const float* __restrict__ ab, float slope, int p,
                                                         T* __restrict__ y, float* __restrict__ seq,
                                                         float* __restrict__ gan, float* __restrict__ pool) {
  const int Wo = W / p, C8 = C >> 3;
  const long long n = (long long)B * (H + 2) * (Wo + 2) * C8;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int c = (int)(i % C8) << 3;
    const long long r = i / C8;
    const int wp = (int)(r % (Wo + 2)), hp = (int)((r / (Wo + 2)) % (H + 2));
    const int b = (int)(r / ((long long)(Wo + 2) * (H + 2)));
    T* yo = y ? y + ((size_t)b * (H + 2) * (Wo + 2) + (size_t)hp * (Wo + 2) + wp) * C + c : nullptr;
    float m[8];
    if (hp == 0 || hp == H + 1 || wp == 0 || wp == Wo + 1) {
#pragma unroll
      for (int k = 0; k < 8; ++k) m[k] = 0.f;
      if (yo) store8(yo, m);
      continue;
    }
    const int h = hp - 1, wo = wp - 1;
    float sc[8], sh[8];
    load8(ab + c, sc);
    load8(ab + C + c, sh);
    const T* xr = x + ((size_t)b * (H + 2) * (W + 2) + (size_t)(h + 1) * (W + 2) + 1) * C + c;
    // the last output column also walks the dropped tail for gan (the map before the pooling)
    const int w0 = wo * p, w1 = (gan && wo == Wo - 1) ? W : w0 + p;
    for (int w = w0; w < w1; ++w) {
      float v[8];
      load8(xr + (size_t)w * C, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[k] = fmaf(v[k], sc[k], sh[k]);
        v[k] = v[k] > 0.f ? v[k] : v[k] * slope;
      }
      if (gan) {
#pragma unroll
        for (int k = 0; k < 8; ++k) gan[(((size_t)b * C + c + k) * W + w) * H + h] = v[k];
      }
      if (w == w0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) m[k] = v[k];
      } else if (w < w0 + p) {
#pragma unroll
        for (int k = 0; k < 8; ++k) m[k] = v[k] > m[k] ? v[k] : m[k];
      }
    }
    if (yo) store8(yo, m);
    if (seq) {
#pragma unroll
      for (int k = 0; k < 8; ++k) seq[((size_t)b * H + h) * ((size_t)C * Wo) + (size_t)(c + k) * Wo + wo] = m[k];
    }
    if (pool) {
#pragma unroll
      for (int k = 0; k < 8; ++k) pool[(((size_t)b * C + c + k) * H + h) * Wo + wo] = m[k];
    }
  }
}

// one wave per output: lane l sums k = l, l + 64, .. in order, then a fixed butterfly
__global__ void __launch_bounds__(NT) k_linear_abs(const float* __restrict__ x, long long rows, int K,
                                                   const float* __restrict__ w, const float* __restrict__ bias, int N,
                                                   float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long n = rows * N;
  for (long long o = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6); o < n; o += (long long)gridDim.x * (NT / 64)) {
    const long long r = o / N;
    const int j = (int)(o % N);
    const float* xr = x + r * K;
    const float* wr = w + (size_t)j * K;
    float a = 0.f;
    for (int k = lane; k < K; k += 64) a = fmaf(xr[k], wr[k], a);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) a += __shfl_xor(a, s);
    if (lane == 0) out[o] = fabsf(a + (bias ? bias[j] : 0.f));
  }
}

// the reference's order: exp, square, sum over the bins (bin order), sqrt, log
__global__ void __launch_bounds__(NT) k_log_norm(const float* __restrict__ mel, int B, int M, int Tn, float mean,
                                                 float std, float* __restrict__ out) {
  const long long n = (long long)B * Tn;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int t = (int)(i % Tn);
    const long long b = i / Tn;
    const float* xb = mel + (size_t)b * M * Tn + t;
    float s = 0.f;
    for (int m = 0; m < M; ++m) {
      const float e = expf(xb[(size_t)m * Tn] * std + mean);
      s += e * e;
    }
    out[i] = logf(sqrtf(s));
  }
}

}  // namespace

int st_mel_to_padded_t(const float* mel, int B, int nb, int T, void* dst, int dtype, hipStream_t s) {
  if (!mel || !dst || B <= 0 || nb <= 0 || T <= 0) return ST_EINVAL;
  const long long n = (long long)B * nb * T;
  if (dtype == ST_FP32)
    hipLaunchKernelGGL(k_mel_to_padded_t<float>, dim3(grid_of(n)), dim3(NT), 0, s, mel, B, nb, T, (float*)dst);
  else if (dtype == ST_BF16)
    hipLaunchKernelGGL(k_mel_to_padded_t<bf16_t>, dim3(grid_of(n)), dim3(NT), 0, s, mel, B, nb, T, (bf16_t*)dst);
  else
    return ST_EDTYPE;
  return (int)hipGetLastError();
}

int st_bn_affine(const float* w, const float* b, const float* mean, const float* var, int C, float eps, float* ab,
                 hipStream_t s) {
  if (!w || !b || !mean || !var || !ab || C <= 0) return ST_EINVAL;
  hipLaunchKernelGGL(k_bn_affine, dim3((C + NT - 1) / NT), dim3(NT), 0, s, w, b, mean, var, C, eps, ab);
  return (int)hipGetLastError();
}

int st_bn_lrelu_maxpool(const void* x, int B, int H, int W, int C, const float* ab, float slope, int p, void* y,
                        float* seq, float* gan, float* pool, int dtype, hipStream_t s) {
  if (!x || !ab || B <= 0 || H <= 0 || p <= 0 || W < p || C <= 0 || (C & 7)) return ST_EINVAL;
  const long long n = (long long)B * (H + 2) * (W / p + 2) * (C >> 3);
  if (dtype == ST_FP32)
    hipLaunchKernelGGL(k_bn_lrelu_maxpool<float>, dim3(grid_of(n)), dim3(NT), 0, s, (const float*)x, B, H, W, C, ab,
                       slope, p, (float*)y, seq, gan, pool);
  else if (dtype == ST_BF16)
    hipLaunchKernelGGL(k_bn_lrelu_maxpool<bf16_t>, dim3(grid_of(n)), dim3(NT), 0, s, (const bf16_t*)x, B, H, W, C, ab,
                       slope, p, (bf16_t*)y, seq, gan, pool);
  else
    return ST_EDTYPE;
  return (int)hipGetLastError();
}

int st_linear_abs(const float* x, long long rows, int K, const float* w, const float* bias, int N, float* out,
                  hipStream_t s) {
  if (!x || !w || !out || rows <= 0 || K <= 0 || N <= 0) return ST_EINVAL;
  hipLaunchKernelGGL(k_linear_abs, dim3(grid_of(rows * N * 64)), dim3(NT), 0, s, x, rows, K, w, bias, N, out);
  return (int)hipGetLastError();
}

int st_log_norm(const float* mel, int B, int n_mels, int T, float mean, float std, float* out, hipStream_t s) {
  if (!mel || !out || B <= 0 || n_mels <= 0 || T <= 0) return ST_EINVAL;
  hipLaunchKernelGGL(k_log_norm, dim3(grid_of((long long)B * T)), dim3(NT), 0, s, mel, B, n_mels, T, mean, std, out);
  return (int)hipGetLastError();
}
