// Training layers of the Vocos decoder (reference Modules/vocos.py) that the conv engines and the
// AdaIN / LayerNorm pairs do not cover (include/stts2_train.h), gfx950, fp32 frames [B][L][C]:
//   k_dwconv         ConvNeXtBlock.dwconv (:45) forward, and its dx (the same conv of dy, taps reversed)
//   k_dwconv_wgrad   dw [C][K] / db [C] as fp64 row-slice partials, folded in slice order by k_dwconv_fold
//   k_gelu_*         erf GELU (:48) and its backward from the saved pre-activation (16-byte accesses)
//   k_ls_*           layer scale + residual (:64-68): y = r + gamma x; dx = gamma dy, dgamma = colsum(dy x)
//   k_head_frames    ISTFTHead (:282-296) + irfft + window (:210-212), one workgroup per STFT frame
//   k_head_ola       the fold overlap-add / envelope division / trim (:214-231), one sample per thread
//   k_head_bwd       the adjoint of both: gather dframe from dy (each element reads one sample: no
//                    atomics), a forward real DFT in LDS, then the exp / clip / cos / sin chain
// The DFTs use the two-factor N = N1 * N2 Cooley-Tukey scheme of k_istft_frames (csrc/vocos.hip), so
// n_fft = 1200 and 1024 both run.  All are HBM-streaming VALU kernels; the parameter sums are fp64
// partials added in a fixed order (no atomics): bitwise reproducible run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/stts2.h"
#include "../../include/stts2_train.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NT = 256;
constexpr int DW_ROWS = 32;     // output frames per thread (as k_dwconv7)
constexpr int DW_KMAX = 11;
constexpr int DW_CMAX = 65536;  // channels: any count in [1, DW_CMAX]
constexpr int DW_SMAX = 64;     // row slices per utterance of the dw / db partials
constexpr int LS_SMAX = 256;    // row slices of the dgamma partials

inline size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

inline unsigned grid_for(long long n, int per_thread = 1) {
  long long b = (n + (long long)NT * per_thread - 1) / ((long long)NT * per_thread);
  return (unsigned)std::max<long long>(1, std::min<long long>(b, 1 << 20));
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------ depthwise conv
// y[b][t][c] = bias[c] + sum_k w[c][flip ? K-1-k : k] * x[b][t + k - K/2][c] (zero padded).  A thread
// owns one channel and DW_ROWS consecutive frames (sliding K-tap window in registers); the 256
// threads of a block cover 256 consecutive channels, so every row access is coalesced.
template <int K>
__global__ void __launch_bounds__(256) k_dwconv(const float* __restrict__ x, const float* __restrict__ w,
                                                const float* __restrict__ bias, int L, int C, int flip,
                                                float* __restrict__ y) {
  const int b = blockIdx.y, c = blockIdx.z * 256 + threadIdx.x;
  if (c >= C) return;
  constexpr int P = K / 2;
  const int r0 = blockIdx.x * DW_ROWS;
  const float* xb = x + (size_t)b * L * C + c;
  float* yb = y + (size_t)b * L * C + c;
  float wk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) wk[k] = w[c * K + (flip ? K - 1 - k : k)];
  const float bc = bias ? bias[c] : 0.f;
  float win[K];
#pragma unroll
  for (int k = 0; k < K - 1; ++k) {
    const int r = r0 - P + k;
    win[k] = (r >= 0 && r < L) ? xb[(size_t)r * C] : 0.f;
  }
  const int r1 = min(r0 + DW_ROWS, L);
  for (int t = r0; t < r1; ++t) {
    const int r = t + P;
    win[K - 1] = r < L ? xb[(size_t)r * C] : 0.f;
    float v = bc;
#pragma unroll
    for (int k = 0; k < K; ++k) v = fmaf(wk[k], win[k], v);
    yb[(size_t)t * C] = v;
#pragma unroll
    for (int k = 0; k < K - 1; ++k) win[k] = win[k + 1];
  }
}

inline int dw_slices(int L) { return std::max(1, std::min(DW_SMAX, (L + DW_ROWS - 1) / DW_ROWS)); }

// part[(b S + s)][c][K + 1] (fp64): sum over the slice's rows t of dy[t] x[t + k - K/2] (k < K) and of dy[t]
template <int K>
__global__ void __launch_bounds__(256) k_dwconv_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                      int L, int C, int S, double* __restrict__ part) {
  const int s = blockIdx.x, b = blockIdx.y, c = blockIdx.z * 256 + threadIdx.x;
  if (c >= C) return;
  constexpr int P = K / 2;
  const int r0 = (int)((long long)L * s / S), r1 = (int)((long long)L * (s + 1) / S);
  const float* xb = x + (size_t)b * L * C + c;
  const float* gb = dy + (size_t)b * L * C + c;
  double acc[K + 1];
#pragma unroll
  for (int k = 0; k <= K; ++k) acc[k] = 0.0;
  float win[K];
#pragma unroll
  for (int k = 0; k < K - 1; ++k) {
    const int r = r0 - P + k;
    win[k] = (x && r >= 0 && r < L) ? xb[(size_t)r * C] : 0.f;
  }
  for (int t = r0; t < r1; ++t) {
    const int r = t + P;
    win[K - 1] = (x && r < L) ? xb[(size_t)r * C] : 0.f;
    const float g = gb[(size_t)t * C];
    if (x) {
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] += (double)g * (double)win[k];
    }
    acc[K] += (double)g;
#pragma unroll
    for (int k = 0; k < K - 1; ++k) win[k] = win[k + 1];
  }
  double* d = part + (((size_t)b * S + s) * C + c) * (K + 1);
#pragma unroll
  for (int k = 0; k <= K; ++k) d[k] = acc[k];
}

// one thread per (c, k): the nslice partials added in slice order
__global__ void __launch_bounds__(256) k_dwconv_fold(const double* __restrict__ part, int nslice, int C, int K,
                                                     float* __restrict__ dw, float* __restrict__ db) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * (K + 1)) return;
  const int c = i / (K + 1), k = i - c * (K + 1);
  double t = 0.0;
  for (int s = 0; s < nslice; ++s) t += part[((size_t)s * C + c) * (K + 1) + k];
  if (k < K) {
    if (dw) dw[c * K + k] = (float)t;
  } else if (db) {
    db[c] = (float)t;
  }
}

template <int K>
int launch_dwconv(const float* x, const float* w, const float* bias, int B, int L, int C, int flip, float* y,
                  hipStream_t s) {
  dim3 grid((L + DW_ROWS - 1) / DW_ROWS, B, (C + 255) / 256);
  hipLaunchKernelGGL(k_dwconv<K>, grid, dim3(256), 0, s, x, w, bias, L, C, flip, y);
  return (int)hipGetLastError();
}

template <int K>
int launch_dwconv_wgrad(const float* x, const float* dy, int B, int L, int C, int S, double* part, hipStream_t s) {
  hipLaunchKernelGGL(k_dwconv_wgrad<K>, dim3(S, B, (C + 255) / 256), dim3(256), 0, s, x, dy, L, C, S, part);
  return (int)hipGetLastError();
}

#define DW_SWITCH(K, call)            \
  switch (K) {                        \
    case 1: { constexpr int KK = 1; return call; }   \
    case 3: { constexpr int KK = 3; return call; }   \
    case 5: { constexpr int KK = 5; return call; }   \
    case 7: { constexpr int KK = 7; return call; }   \
    case 9: { constexpr int KK = 9; return call; }   \
    case 11: { constexpr int KK = 11; return call; } \
    default: return ST_EINVAL;        \
  }

int dwconv_any(int K, const float* x, const float* w, const float* bias, int B, int L, int C, int flip, float* y,
               hipStream_t s) {
  DW_SWITCH(K, (launch_dwconv<KK>(x, w, bias, B, L, C, flip, y, s)));
}

int dwconv_wgrad_any(int K, const float* x, const float* dy, int B, int L, int C, int S, double* part, hipStream_t s) {
  DW_SWITCH(K, (launch_dwconv_wgrad<KK>(x, dy, B, L, C, S, part, s)));
}

inline bool dw_shape_ok(int B, int L, int C, int K) {
  return B > 0 && B <= 65535 && L > 0 && C > 0 && C <= DW_CMAX && K >= 1 && K <= DW_KMAX && (K & 1);
}

// ------------------------------------------------------------------ GELU (erf)
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

// d/dx [x Phi(x)] = Phi(x) + x phi(x)
__device__ __forceinline__ float gelu_d(float x) {
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
  const float pdf = 0.39894228040143268f * expf(-0.5f * x * x);
  return fmaf(x, pdf, cdf);
}

// n4 float4 groups, then the n - 4 n4 tail values one by one (n4 = 0 when a pointer is not 16-byte aligned)
__global__ void __launch_bounds__(256) k_gelu_fwd(const float* __restrict__ x, long long n, long long n4,
                                                  float* __restrict__ y) {
  const long long stride = (long long)gridDim.x * NT, i0 = (long long)blockIdx.x * NT + threadIdx.x;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float4* y4 = reinterpret_cast<float4*>(y);
  for (long long i = i0; i < n4; i += stride) {
    const float4 v = x4[i];
    y4[i] = make_float4(gelu_f(v.x), gelu_f(v.y), gelu_f(v.z), gelu_f(v.w));
  }
  for (long long i = 4 * n4 + i0; i < n; i += stride) y[i] = gelu_f(x[i]);
}

__global__ void __launch_bounds__(256) k_gelu_bwd(const float* __restrict__ x, const float* __restrict__ dy,
                                                  long long n, long long n4, float* __restrict__ dx) {
  const long long stride = (long long)gridDim.x * NT, i0 = (long long)blockIdx.x * NT + threadIdx.x;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const float4* g4 = reinterpret_cast<const float4*>(dy);
  float4* d4 = reinterpret_cast<float4*>(dx);
  for (long long i = i0; i < n4; i += stride) {
    const float4 v = x4[i], g = g4[i];
    d4[i] = make_float4(g.x * gelu_d(v.x), g.y * gelu_d(v.y), g.z * gelu_d(v.z), g.w * gelu_d(v.w));
  }
  for (long long i = 4 * n4 + i0; i < n; i += stride) dx[i] = dy[i] * gelu_d(x[i]);
}

// ------------------------------------------------------------------ layer scale + residual
__global__ void __launch_bounds__(256) k_ls_fwd(const float* __restrict__ x, const float* __restrict__ r,
                                                const float* __restrict__ gamma, int C, long long n,
                                                float* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT)
    y[i] = fmaf(gamma[(int)(i % C)], x[i], r[i]);
}

// C % 4 == 0 and 16-byte aligned pointers: four channels per thread
__global__ void __launch_bounds__(256) k_ls_fwd4(const float4* __restrict__ x, const float4* __restrict__ r,
                                                 const float4* __restrict__ gamma, int C4, long long n4,
                                                 float4* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long long)gridDim.x * NT) {
    const float4 g = gamma[(int)(i % C4)], v = x[i], q = r[i];
    y[i] = make_float4(fmaf(g.x, v.x, q.x), fmaf(g.y, v.y, q.y), fmaf(g.z, v.z, q.z), fmaf(g.w, v.w, q.w));
  }
}

inline int ls_slices(long long R) { return (int)std::max<long long>(1, std::min<long long>(LS_SMAX, R / 16)); }

// rows [R = B L][C]: dx = gamma dy, part[s][c] = sum over the slice's rows of dy x (fp64).  64 channels x
// 4 row lanes per block, as k_snake_bwd.
__global__ void __launch_bounds__(256) k_ls_bwd(const float* __restrict__ x, const float* __restrict__ gamma,
                                                const float* __restrict__ dy, long long R, int C, int S,
                                                float* __restrict__ dx, double* __restrict__ part) {
  __shared__ double red[4][64];
  const int l = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + l, s = blockIdx.y;
  const long long r0 = R * s / S, r1 = R * (s + 1) / S;
  double acc = 0.0;
  if (c < C) {
    const float g = dx ? gamma[c] : 0.f;
    for (long long r = r0 + rl; r < r1; r += 4) {
      const size_t i = (size_t)r * C + c;
      const float d = dy[i];
      if (dx) dx[i] = g * d;
      if (part) acc += (double)d * (double)x[i];
    }
  }
  red[rl][l] = acc;
  __syncthreads();
  if (part && rl == 0 && c < C) part[(size_t)s * C + c] = ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l];
}

__global__ void __launch_bounds__(256) k_ls_fold(const double* __restrict__ part, int S, int C,
                                                 float* __restrict__ dgamma) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double t = 0.0;
  for (int s = 0; s < S; ++s) t += part[(size_t)s * C + c];
  dgamma[c] = (float)t;
}

// ------------------------------------------------------------------ ISTFT head
// e^{2 pi i m / M}
__device__ __forceinline__ float2 cis(int m, int M) {
  float sn, cs;
  sincospif(2.0f * (float)m / (float)M, &sn, &cs);
  return make_float2(cs, sn);
}

// One STFT frame, as k_istft_frames (csrc/vocos.hip): spec[k] = min(exp(h[k]), 100) (cos h[nb + k] + i sin h[nb + k]),
// x[n] = (1/N) sum_k X[k] e^{2 pi i k n / N} over the Hermitian extension (Im of DC / Nyquist dropped),
// frame[n] = x[n] window[n].  k = k1 + N1 k2, n = N2 n1 + n2.
__global__ void __launch_bounds__(256) k_head_frames(const float* __restrict__ h, int F, int N, int N1, int N2,
                                                     const float* __restrict__ window, float* __restrict__ fr) {
  extern __shared__ float2 sm[];
  float2* X = sm;        // [N]
  float2* Y = sm + N;    // [N1][N2]
  float2* t1 = Y + N;    // [N1]
  float2* t2 = t1 + N1;  // [N2]
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int nb = N / 2 + 1;
  const float* hr = h + ((size_t)b * F + f) * (2 * nb);
  for (int k = tid; k < N; k += 256) {
    const bool mir = k > N / 2;
    const int src = mir ? N - k : k;
    const float mag = fminf(expf(hr[src]), 100.0f);
    float sn, cs;
    sincosf(hr[nb + src], &sn, &cs);
    float re = mag * cs, im = mag * sn;
    if (src == 0 || 2 * src == N) im = 0.f;
    X[k] = make_float2(re, mir ? -im : im);
  }
  for (int m = tid; m < N1; m += 256) t1[m] = cis(m, N1);
  for (int m = tid; m < N2; m += 256) t2[m] = cis(m, N2);
  __syncthreads();
  for (int i = tid; i < N; i += 256) {
    const int k1 = i / N2, n2 = i - k1 * N2;
    float re = 0.f, im = 0.f;
    int e = 0;  // (k2 * n2) mod N2
    for (int k2 = 0; k2 < N2; ++k2) {
      const float2 xv = X[k1 + N1 * k2], tw = t2[e];
      re = fmaf(xv.x, tw.x, fmaf(-xv.y, tw.y, re));
      im = fmaf(xv.x, tw.y, fmaf(xv.y, tw.x, im));
      e += n2;
      if (e >= N2) e -= N2;
    }
    const float2 tw = cis((k1 * n2) % N, N);
    Y[i] = make_float2(re * tw.x - im * tw.y, re * tw.y + im * tw.x);
  }
  __syncthreads();
  const float invN = 1.0f / (float)N;
  float* fo = fr + ((size_t)b * F + f) * N;
  for (int n = tid; n < N; n += 256) {
    const int n1 = n / N2, n2 = n - n1 * N2;
    float re = 0.f;
    int e = 0;  // (k1 * n1) mod N1
    for (int k1 = 0; k1 < N1; ++k1) {
      const float2 yv = Y[k1 * N2 + n2], tw = t1[e];
      re = fmaf(yv.x, tw.x, fmaf(-yv.y, tw.y, re));
      e += n1;
      if (e >= N1) e -= N1;
    }
    fo[n] = re * invN * window[n];
  }
}

// env[p] = sum over the frames t covering position p of window[p - t hop]^2
__device__ __forceinline__ float env_at(int p, int F, int N, int hop, const float* __restrict__ window) {
  int t0 = p - N + 1;
  t0 = t0 <= 0 ? 0 : (t0 + hop - 1) / hop;
  const int t1 = min(F - 1, p / hop);
  float env = 0.f;
  for (int t = t0; t <= t1; ++t) {
    const float wv = window[p - t * hop];
    env = fmaf(wv, wv, env);
  }
  return env;
}

// audio[b][j] = sum_t fr[b][t][p - t hop] / env[p],  p = j + pad
__global__ void __launch_bounds__(256) k_head_ola(const float* __restrict__ fr, int F, int N, int hop, int pad,
                                                  const float* __restrict__ window, float* __restrict__ out, int Lout) {
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= Lout) return;
  const int p = j + pad;
  int t0 = p - N + 1;
  t0 = t0 <= 0 ? 0 : (t0 + hop - 1) / hop;
  const int t1 = min(F - 1, p / hop);
  float y = 0.f;
  for (int t = t0; t <= t1; ++t) y += fr[((size_t)b * F + t) * N + (p - t * hop)];
  out[(size_t)b * Lout + j] = y / env_at(p, F, N, hop, window);
}

// The adjoint for one frame t: d[n] = window[n] dy[t hop + n - pad] / env[t hop + n] (0 outside the kept range);
// D[k] = sum_n d[n] e^{-2 pi i k n / N} by the same two factors run the other way:
//   Z[k1][n2] = e^{-2 pi i k1 n2 / N} sum_n1 d[N2 n1 + n2] e^{-2 pi i k1 n1 / N1}
//   D[k1 + N1 k2] = sum_n2 Z[k1][n2] e^{-2 pi i k2 n2 / N2}
// dXr = (c_k / N) Re D, dXi = (c_k / N) Im D (0 at DC / Nyquist), c_k = 1 at DC / Nyquist, else 2; then
//   dp = mag (dXi cos p - dXr sin p),  dh_mag = (dXr cos p + dXi sin p) exp(h_mag) where exp(h_mag) <= 100, else 0.
__global__ void __launch_bounds__(256) k_head_bwd(const float* __restrict__ h, const float* __restrict__ dy, int F,
                                                  int N, int N1, int N2, int hop, int pad, int Lout,
                                                  const float* __restrict__ window, float* __restrict__ dh) {
  extern __shared__ float2 sm[];
  float2* Z = sm;                                   // [N1][N2]
  float2* t1 = Z + N;                               // [N1]
  float2* t2 = t1 + N1;                             // [N2]
  float* d = reinterpret_cast<float*>(t2 + N2);     // [N]
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int nb = N / 2 + 1;
  for (int n = tid; n < N; n += 256) {
    const int p = f * hop + n, j = p - pad;
    float v = 0.f;
    if (j >= 0 && j < Lout) v = window[n] * dy[(size_t)b * Lout + j] / env_at(p, F, N, hop, window);
    d[n] = v;
  }
  for (int m = tid; m < N1; m += 256) t1[m] = cis(m, N1);
  for (int m = tid; m < N2; m += 256) t2[m] = cis(m, N2);
  __syncthreads();
  for (int i = tid; i < N; i += 256) {
    const int k1 = i / N2, n2 = i - k1 * N2;
    float re = 0.f, im = 0.f;
    int e = 0;  // (k1 * n1) mod N1
    for (int n1 = 0; n1 < N1; ++n1) {
      const float v = d[N2 * n1 + n2];
      const float2 tw = t1[e];
      re = fmaf(v, tw.x, re);
      im = fmaf(-v, tw.y, im);
      e += k1;
      if (e >= N1) e -= N1;
    }
    const float2 tw = cis((k1 * n2) % N, N);  // times its conjugate
    Z[i] = make_float2(re * tw.x + im * tw.y, im * tw.x - re * tw.y);
  }
  __syncthreads();
  const float invN = 1.0f / (float)N;
  const float* hr = h + ((size_t)b * F + f) * (2 * nb);
  float* dr = dh + ((size_t)b * F + f) * (2 * nb);
  for (int k = tid; k < nb; k += 256) {
    const int k2 = k / N1, k1 = k - k2 * N1;
    float re = 0.f, im = 0.f;
    int e = 0;  // (k2 * n2) mod N2
    for (int n2 = 0; n2 < N2; ++n2) {
      const float2 zv = Z[k1 * N2 + n2], tw = t2[e];
      re = fmaf(zv.x, tw.x, fmaf(zv.y, tw.y, re));
      im = fmaf(zv.y, tw.x, fmaf(-zv.x, tw.y, im));
      e += k2;
      if (e >= N2) e -= N2;
    }
    const bool edge = k == 0 || 2 * k == N;
    const float ck = edge ? invN : 2.0f * invN;
    const float dXr = ck * re, dXi = edge ? 0.f : ck * im;
    const float ex = expf(hr[k]);
    const float mag = fminf(ex, 100.0f);
    float sn, cs;
    sincosf(hr[nb + k], &sn, &cs);
    dr[k] = ex <= 100.0f ? (dXr * cs + dXi * sn) * ex : 0.f;
    dr[nb + k] = mag * (dXi * cs - dXr * sn);
  }
}

struct HeadGeo {
  int N1, N2, pad, Lout;
  size_t lds_fwd, lds_bwd;
};

// n_fft even with a two-factor split (both <= 64), 0 < hop < n_fft, n_fft - hop even ('same' padding: F hop samples)
int head_geo(int B, int F, int n_fft, int hop, HeadGeo* g) {
  if (B <= 0 || B > 65535 || F <= 0 || n_fft < 4 || (n_fft & 1) || hop <= 0 || hop >= n_fft || ((n_fft - hop) & 1))
    return ST_EINVAL;
  if (st_istft_factor(n_fft, &g->N1, &g->N2) != ST_OK) return ST_EINVAL;
  g->pad = (n_fft - hop) / 2;
  const long long lout = (long long)F * hop;
  if (lout > 0x7fffffffLL) return ST_EINVAL;
  g->Lout = (int)lout;
  g->lds_fwd = (size_t)(2 * n_fft + g->N1 + g->N2) * sizeof(float2);
  g->lds_bwd = (size_t)(n_fft + g->N1 + g->N2) * sizeof(float2) + (size_t)n_fft * sizeof(float);
  if (g->lds_fwd > 64 * 1024 || g->lds_bwd > 64 * 1024) return ST_EINVAL;
  return ST_OK;
}

}  // namespace

// ================================================================== C-ABI
extern "C" int stts_dwconv1d_fwd(const float* x, const float* w, const float* bias, int B, int L, int C, int K,
                                 float* y, void* stream) {
  if (!dw_shape_ok(B, L, C, K)) return ST_EINVAL;
  if (!x || !w || !y) return ST_EINVAL;
  return dwconv_any(K, x, w, bias, B, L, C, 0, y, (hipStream_t)stream);
}

extern "C" long long stts_dwconv1d_bwd_workspace_bytes(int B, int L, int C, int K) {
  if (!dw_shape_ok(B, L, C, K)) return ST_EINVAL;
  return (long long)al((size_t)B * dw_slices(L) * C * (K + 1) * sizeof(double));
}

extern "C" int stts_dwconv1d_bwd(const float* x, const float* w, const float* dy, int B, int L, int C, int K,
                                 float* dx, float* dw, float* db, void* ws, long long ws_bytes, void* stream) {
  const long long need = stts_dwconv1d_bwd_workspace_bytes(B, L, C, K);
  if (need < 0) return (int)need;
  if (!dy || (dx && !w) || (dw && !x)) return ST_EINVAL;
  if (!dx && !dw && !db) return 0;
  hipStream_t s = (hipStream_t)stream;
  if ((dw || db) && (!ws || ws_bytes < need)) return ST_EWORKSPACE;
  if (dx) ST_CHECK(dwconv_any(K, dy, w, nullptr, B, L, C, 1, dx, s));
  if (dw || db) {
    const int S = dw_slices(L);
    double* part = (double*)ws;
    ST_CHECK(dwconv_wgrad_any(K, x, dy, B, L, C, S, part, s));
    hipLaunchKernelGGL(k_dwconv_fold, dim3((C * (K + 1) + 255) / 256), dim3(256), 0, s, part, B * S, C, K, dw, db);
    ST_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

extern "C" int stts_gelu_fwd(const float* x, long long n, float* y, void* stream) {
  if (!x || !y || n < 0) return ST_EINVAL;
  if (n == 0) return 0;
  const long long n4 = (aligned16(x) && aligned16(y)) ? n / 4 : 0;
  hipLaunchKernelGGL(k_gelu_fwd, dim3(grid_for(n, 8)), dim3(NT), 0, (hipStream_t)stream, x, n, n4, y);
  return (int)hipGetLastError();
}

extern "C" int stts_gelu_bwd(const float* x, const float* dy, long long n, float* dx, void* stream) {
  if (!x || !dy || !dx || n < 0) return ST_EINVAL;
  if (n == 0) return 0;
  const long long n4 = (aligned16(x) && aligned16(dy) && aligned16(dx)) ? n / 4 : 0;
  hipLaunchKernelGGL(k_gelu_bwd, dim3(grid_for(n, 8)), dim3(NT), 0, (hipStream_t)stream, x, dy, n, n4, dx);
  return (int)hipGetLastError();
}

extern "C" int stts_layer_scale_res_fwd(const float* x, const float* r, const float* gamma, int B, int L, int C,
                                        float* y, void* stream) {
  if (B <= 0 || L <= 0 || C <= 0) return ST_EINVAL;
  if (!x || !r || !gamma || !y) return ST_EINVAL;
  const long long n = (long long)B * L * C;
  hipStream_t s = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(x) && aligned16(r) && aligned16(gamma) && aligned16(y))
    hipLaunchKernelGGL(k_ls_fwd4, dim3(grid_for(n / 4, 2)), dim3(NT), 0, s, (const float4*)x, (const float4*)r,
                       (const float4*)gamma, C / 4, n / 4, (float4*)y);
  else
    hipLaunchKernelGGL(k_ls_fwd, dim3(grid_for(n, 4)), dim3(NT), 0, s, x, r, gamma, C, n, y);
  return (int)hipGetLastError();
}

extern "C" long long stts_layer_scale_res_bwd_workspace_bytes(int B, int L, int C) {
  if (B <= 0 || L <= 0 || C <= 0) return ST_EINVAL;
  return (long long)al((size_t)ls_slices((long long)B * L) * C * sizeof(double));
}

extern "C" int stts_layer_scale_res_bwd(const float* x, const float* gamma, const float* dy, int B, int L, int C,
                                        float* dx, float* dgamma, void* ws, long long ws_bytes, void* stream) {
  const long long need = stts_layer_scale_res_bwd_workspace_bytes(B, L, C);
  if (need < 0) return (int)need;
  if (!dy || (dx && !gamma) || (dgamma && !x)) return ST_EINVAL;
  if (!dx && !dgamma) return 0;
  if (dgamma && (!ws || ws_bytes < need)) return ST_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const long long R = (long long)B * L;
  const int S = ls_slices(R);
  double* part = dgamma ? (double*)ws : nullptr;
  hipLaunchKernelGGL(k_ls_bwd, dim3((C + 63) / 64, S), dim3(256), 0, s, x, gamma, dy, R, C, S, dx, part);
  ST_CHECK_HIP(hipGetLastError());
  if (dgamma) {
    hipLaunchKernelGGL(k_ls_fold, dim3((C + 255) / 256), dim3(256), 0, s, part, S, C, dgamma);
    ST_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

extern "C" long long stts_istft_head_workspace_bytes(int B, int F, int n_fft, int hop) {
  HeadGeo g;
  const int rc = head_geo(B, F, n_fft, hop, &g);
  if (rc != ST_OK) return rc;
  return (long long)al((size_t)B * F * n_fft * sizeof(float));
}

extern "C" int stts_istft_head_fwd(const float* h, const float* window, int B, int F, int n_fft, int hop, float* audio,
                                   void* ws, long long ws_bytes, void* stream) {
  const long long need = stts_istft_head_workspace_bytes(B, F, n_fft, hop);
  if (need < 0) return (int)need;
  if (!h || !window || !audio) return ST_EINVAL;
  if (!ws || ws_bytes < need) return ST_EWORKSPACE;
  HeadGeo g;
  ST_CHECK(head_geo(B, F, n_fft, hop, &g));
  hipStream_t s = (hipStream_t)stream;
  float* fr = (float*)ws;
  hipLaunchKernelGGL(k_head_frames, dim3(F, B), dim3(256), g.lds_fwd, s, h, F, n_fft, g.N1, g.N2, window, fr);
  ST_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_head_ola, dim3((g.Lout + 255) / 256, B), dim3(256), 0, s, fr, F, n_fft, hop, g.pad, window,
                     audio, g.Lout);
  return (int)hipGetLastError();
}

extern "C" int stts_istft_head_bwd(const float* h, const float* window, const float* dy, int B, int F, int n_fft,
                                   int hop, float* dh, void* ws, long long ws_bytes, void* stream) {
  const long long need = stts_istft_head_workspace_bytes(B, F, n_fft, hop);
  if (need < 0) return (int)need;
  if (!h || !window || !dy || !dh) return ST_EINVAL;
  (void)ws;  // the adjoint gathers straight from dy: no frame buffer (the argument keeps the pair's signature)
  (void)ws_bytes;
  HeadGeo g;
  ST_CHECK(head_geo(B, F, n_fft, hop, &g));
  hipLaunchKernelGGL(k_head_bwd, dim3(F, B), dim3(256), g.lds_bwd, (hipStream_t)stream, h, dy, F, n_fft, g.N1, g.N2,
                     hop, g.pad, g.Lout, window, dh);
  return (int)hipGetLastError();
}
