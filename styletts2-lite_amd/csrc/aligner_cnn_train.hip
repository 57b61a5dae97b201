// The text aligner's conv stack under training (Modules/ASR/models.py ASRCNN :37-48, layers.py ConvBlock :105-131;
// train.py:206, 318, 328): what the conv engines (stts_conv1d_fwd_act / stts_conv1d_bwd) do not already cover.
//   stts_groupnorm_fwd_train   y = dropout(GroupNorm(G)([ReLU] x)), the statistics kept for the backward
//   stts_groupnorm_bwd         dx, dw, db from dy (through the same dropout, redrawn or re-read, and the ReLU)
//   stts_dropout_add_fwd       y = r + dropout(x), the ConvBlock tail `x = block(x); x += res`
//   stts_mfcc_frames           mel [B][80][T] -> MFCC frames [B][T][40] (aligner.hip's launcher, exported)
// Frames layout [B][L][C] fp32.  Grid rule: every utterance's L rows are cut into S = slices_of(L) row slices (a
// function of L alone, never of B); a workgroup = 64 channels x 4 row lanes over one slice of one utterance writes
// fp64 per-channel partials (normbwd.hip's k_stats_part pattern); a second pass adds them per (utterance, group) in
// channel order, slices ascending, and, for dw / db, utterances ascending.  No atomics: every sum has one order, and
// a batch row's y and dx are bitwise the B = 1 result.  GroupNorm(1, 256) at B = 2, L = 400 is 200 workgroups for the
// partials (the eval kernel's one workgroup per (utterance, group) would be 2).
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "../../include/stts2.h"
#include "../../include/stts2_train.h"
#include "common.h"
#include "dropout_draw.h"
#include "kernels.h"

namespace {

constexpr int NT = 256;
constexpr double kEps = 1e-5;

// row slices per utterance: 16 rows each, at most 256
int slices_of(int L) { return std::max(1, std::min(256, L / 16)); }

inline size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

unsigned grid_of(long long n) {
  const long long g = (n + NT - 1) / NT;
  return (unsigned)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

// dropout of one value: the injected keep mask when given, else the counter draw of flat element i (p > 0), else
// the identity.  __fmul_rn: the product is rounded on its own (never contracted into a following add), as the
// unfused stts_dropout stores it.
__device__ __forceinline__ float drop_of(float v, long long i, float p, float scale, unsigned long long seed,
                                         const float* __restrict__ mask) {
  if (mask) return mask[i] != 0.f ? __fmul_rn(v, scale) : 0.f;
  if (p > 0.f) return drop::keep(seed, i, p) ? __fmul_rn(v, scale) : 0.f;
  return v;
}

// fixed-order sum of one double per thread over the workgroup (tree in LDS); every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* red) {
  __syncthreads();  // (red may still be read from the previous call)
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

// per (utterance, slice, channel): sum v, sum v^2 with v = [ReLU] x
__global__ __launch_bounds__(NT) void k_gn_stats_part(const float* __restrict__ x, int L, int C, int S, int relu,
                                                       double* __restrict__ part) {
  __shared__ double red[2][4][64];
  const int l = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + l, s = blockIdx.y, b = blockIdx.z;
  const int r0 = (int)((long long)L * s / S), r1 = (int)((long long)L * (s + 1) / S);
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    const float* xb = x + (size_t)b * L * C + c;
    for (int r = r0 + rl; r < r1; r += 4) {
      float f = xb[(size_t)r * C];
      if (relu) f = fmaxf(f, 0.f);
      const double v = f;
      s1 += v;
      s2 += v * v;
    }
  }
  red[0][rl][l] = s1;
  red[1][rl][l] = s2;
  __syncthreads();
  if (rl == 0 && c < C) {
    double* p = part + (((size_t)b * S + s) * C + c) * 2;
    p[0] = ((red[0][0][l] + red[0][1][l]) + red[0][2][l]) + red[0][3][l];
    p[1] = ((red[1][0][l] + red[1][1][l]) + red[1][2][l]) + red[1][3][l];
  }
}

// one workgroup per (utterance, group): a thread adds its channels' slices in ascending order, the workgroup adds
// the threads in a fixed tree; stats[(b G + g) 2 + {0, 1}] = mean, rstd (biased variance)
__global__ __launch_bounds__(NT) void k_gn_stats_final(const double* __restrict__ part, int L, int C, int G, int S,
                                                        float* __restrict__ stats) {
  __shared__ double red[NT];
  const int b = blockIdx.x / G, g = blockIdx.x % G, cg = C / G;
  double s1 = 0.0, s2 = 0.0;
  for (int c = threadIdx.x; c < cg; c += NT) {
    const double* p = part + ((size_t)b * S * C + (size_t)g * cg + c) * 2;
    for (int s = 0; s < S; ++s) {
      s1 += p[(size_t)s * C * 2];
      s2 += p[(size_t)s * C * 2 + 1];
    }
  }
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  if (threadIdx.x == 0) {
    const double n = (double)L * cg;
    const double mean = s1 / n;
    const double var = fmax(s2 / n - mean * mean, 0.0);
    stats[2 * blockIdx.x] = (float)mean;
    stats[2 * blockIdx.x + 1] = (float)(1.0 / sqrt(var + kEps));
  }
}

__global__ __launch_bounds__(NT) void k_gn_apply(const float* __restrict__ x, const float* __restrict__ w,
                                                 const float* __restrict__ bias, const float* __restrict__ stats,
                                                 int L, int C, int G, int relu, float p, float scale,
                                                 unsigned long long seed, const float* __restrict__ mask,
                                                 float* __restrict__ y, long long n) {
  const int cg = C / G;
  const long long LC = (long long)L * C;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int c = (int)(i % C);
    const long long bg = (i / LC) * G + c / cg;
    float v = x[i];
    if (relu) v = fmaxf(v, 0.f);
    const float y0 = (v - stats[2 * bg]) * stats[2 * bg + 1] * w[c] + bias[c];
    y[i] = drop_of(y0, i, p, scale, seed, mask);
  }
}

// per (utterance, slice, channel): sum g, sum g xhat with g = dropout(dy)
__global__ __launch_bounds__(NT) void k_gn_bwd_part(const float* __restrict__ x, const float* __restrict__ dy,
                                                    const float* __restrict__ stats, int L, int C, int G, int S,
                                                    int relu, float p, float scale, unsigned long long seed,
                                                    const float* __restrict__ mask, double* __restrict__ part) {
  __shared__ double red[2][4][64];
  const int l = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + l, s = blockIdx.y, b = blockIdx.z;
  const int r0 = (int)((long long)L * s / S), r1 = (int)((long long)L * (s + 1) / S);
  double a1 = 0.0, a2 = 0.0;
  if (c < C) {
    const int bg = b * G + c / (C / G);
    const float mean = stats[2 * bg], rstd = stats[2 * bg + 1];
    const size_t base = (size_t)b * L * C + c;
    for (int r = r0 + rl; r < r1; r += 4) {
      const size_t i = base + (size_t)r * C;
      float v = x[i];
      if (relu) v = fmaxf(v, 0.f);
      const float xh = (v - mean) * rstd;
      const float g = drop_of(dy[i], (long long)i, p, scale, seed, mask);
      a1 += g;
      a2 += (double)g * xh;
    }
  }
  red[0][rl][l] = a1;
  red[1][rl][l] = a2;
  __syncthreads();
  if (rl == 0 && c < C) {
    double* q = part + (((size_t)b * S + s) * C + c) * 2;
    q[0] = ((red[0][0][l] + red[0][1][l]) + red[0][2][l]) + red[0][3][l];
    q[1] = ((red[1][0][l] + red[1][1][l]) + red[1][2][l]) + red[1][3][l];
  }
}

// one workgroup per group.  Per channel (a thread's own): the slices of every utterance in ascending order ->
// tot[b][c] = (sum g, sum g xhat), and dw[c] / db[c] over the utterances in ascending b.  Then per utterance the
// group's sums[(b G + g) 2 + {0, 1}] = sum_c w[c] tot[b][c][{0, 1}] = (sum g', sum g' xhat), channels in a fixed tree.
__global__ __launch_bounds__(NT) void k_gn_bwd_final(const double* __restrict__ part, const float* __restrict__ w,
                                                     int B, int C, int G, int S, double* __restrict__ tot,
                                                     double* __restrict__ sums, float* __restrict__ dw,
                                                     float* __restrict__ db) {
  __shared__ double red[NT];
  const int g = blockIdx.x, cg = C / G;
  for (int c = threadIdx.x; c < cg; c += NT) {
    const int cc = g * cg + c;
    double tw = 0.0, tb = 0.0;
    for (int b = 0; b < B; ++b) {
      const double* q = part + ((size_t)b * S * C + cc) * 2;
      double a1 = 0.0, a2 = 0.0;
      for (int s = 0; s < S; ++s) {
        a1 += q[(size_t)s * C * 2];
        a2 += q[(size_t)s * C * 2 + 1];
      }
      tot[((size_t)b * C + cc) * 2] = a1;
      tot[((size_t)b * C + cc) * 2 + 1] = a2;
      tb += a1;
      tw += a2;
    }
    if (dw) dw[cc] = (float)tw;
    if (db) db[cc] = (float)tb;
  }
  for (int b = 0; b < B; ++b) {
    double a1 = 0.0, a2 = 0.0;
    for (int c = threadIdx.x; c < cg; c += NT) {  // (the thread's own writes above)
      const int cc = g * cg + c;
      const double wc = w[cc];
      a1 += wc * tot[((size_t)b * C + cc) * 2];
      a2 += wc * tot[((size_t)b * C + cc) * 2 + 1];
    }
    a1 = block_sum(a1, red);
    a2 = block_sum(a2, red);
    if (threadIdx.x == 0) {
      sums[2 * ((size_t)b * G + g)] = a1;
      sums[2 * ((size_t)b * G + g) + 1] = a2;
    }
  }
}

__global__ __launch_bounds__(NT) void k_gn_bwd_dx(const float* __restrict__ x, const float* __restrict__ dy,
                                                  const float* __restrict__ w, const float* __restrict__ stats,
                                                  const double* __restrict__ sums, int L, int C, int G, int relu,
                                                  float p, float scale, unsigned long long seed,
                                                  const float* __restrict__ mask, float* __restrict__ dx,
                                                  long long n) {
  const int cg = C / G;
  const long long LC = (long long)L * C;
  const double cnt = (double)L * cg;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int c = (int)(i % C);
    const long long bg = (i / LC) * G + c / cg;
    const float mean = stats[2 * bg], rstd = stats[2 * bg + 1];
    const float xv = x[i];
    const float v = relu ? fmaxf(xv, 0.f) : xv;
    const float xh = (v - mean) * rstd;
    const float gp = drop_of(dy[i], i, p, scale, seed, mask) * w[c];
    const float m1 = (float)(sums[2 * bg] / cnt), m2 = (float)(sums[2 * bg + 1] / cnt);
    const float dv = rstd * (gp - m1 - xh * m2);
    dx[i] = (relu && !(xv > 0.f)) ? 0.f : dv;
  }
}

__global__ __launch_bounds__(NT) void k_dropout_add(const float* __restrict__ x, const float* __restrict__ r,
                                                    long long n, float p, float scale, unsigned long long seed,
                                                    const float* __restrict__ mask, float* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT)
    y[i] = r[i] + drop_of(x[i], i, p, scale, seed, mask);
}

bool geometry_ok(int B, int L, int C, int G) {
  return B >= 1 && L >= 1 && C >= 1 && G >= 1 && C % G == 0 && B <= 65535 && (C + 63) / 64 <= 65535;
}

bool p_ok(float p) { return p >= 0.f && p < 1.f; }

}  // namespace

extern "C" long long stts_groupnorm_fwd_train_workspace_bytes(int B, int L, int C, int G) {
  if (!geometry_ok(B, L, C, G)) return ST_EINVAL;
  return (long long)al((size_t)B * slices_of(L) * C * 2 * sizeof(double));
}

extern "C" int stts_groupnorm_fwd_train(const float* x, const float* w, const float* b, int B, int L, int C, int G,
                                        int relu, float p, unsigned long long seed, const float* keep_mask, float* y,
                                        float* stats, void* ws, long long ws_bytes, void* stream) {
  const long long need = stts_groupnorm_fwd_train_workspace_bytes(B, L, C, G);
  if (need < 0) return (int)need;
  if (!x || !w || !b || !y || !stats || !p_ok(p)) return ST_EINVAL;
  if (!ws || ws_bytes < need) return ST_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int S = slices_of(L);
  double* part = (double*)ws;
  hipLaunchKernelGGL(k_gn_stats_part, dim3((C + 63) / 64, S, B), dim3(NT), 0, s, x, L, C, S, relu, part);
  ST_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_gn_stats_final, dim3((unsigned)(B * G)), dim3(NT), 0, s, part, L, C, G, S, stats);
  ST_CHECK_HIP(hipGetLastError());
  const long long n = (long long)B * L * C;
  hipLaunchKernelGGL(k_gn_apply, dim3(grid_of(n)), dim3(NT), 0, s, x, w, b, stats, L, C, G, relu, p,
                     1.0f / (1.0f - p), seed, keep_mask, y, n);
  return (int)hipGetLastError();
}

extern "C" long long stts_groupnorm_bwd_workspace_bytes(int B, int L, int C, int G) {
  if (!geometry_ok(B, L, C, G)) return ST_EINVAL;
  return (long long)(al((size_t)B * slices_of(L) * C * 2 * sizeof(double)) + al((size_t)B * C * 2 * sizeof(double)) +
                     al((size_t)B * G * 2 * sizeof(double)));
}

extern "C" int stts_groupnorm_bwd(const float* x, const float* w, const float* stats, const float* dy, int B, int L,
                                  int C, int G, int relu, float p, unsigned long long seed, const float* keep_mask,
                                  float* dx, float* dw, float* db, void* ws, long long ws_bytes, void* stream) {
  const long long need = stts_groupnorm_bwd_workspace_bytes(B, L, C, G);
  if (need < 0) return (int)need;
  if (!x || !w || !stats || !dy || !p_ok(p)) return ST_EINVAL;
  if (!ws || ws_bytes < need) return ST_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int S = slices_of(L);
  double* part = (double*)ws;
  double* tot = (double*)((char*)ws + al((size_t)B * S * C * 2 * sizeof(double)));
  double* sums = (double*)((char*)tot + al((size_t)B * C * 2 * sizeof(double)));
  const float scale = 1.0f / (1.0f - p);
  hipLaunchKernelGGL(k_gn_bwd_part, dim3((C + 63) / 64, S, B), dim3(NT), 0, s, x, dy, stats, L, C, G, S, relu, p, scale,
                     seed, keep_mask, part);
  ST_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_gn_bwd_final, dim3((unsigned)G), dim3(NT), 0, s, part, w, B, C, G, S, tot, sums, dw, db);
  ST_CHECK_HIP(hipGetLastError());
  if (dx) {
    const long long n = (long long)B * L * C;
    hipLaunchKernelGGL(k_gn_bwd_dx, dim3(grid_of(n)), dim3(NT), 0, s, x, dy, w, stats, sums, L, C, G, relu, p, scale,
                       seed, keep_mask, dx, n);
    ST_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

extern "C" int stts_dropout_add_fwd(const float* x, const float* r, long long n, float p, unsigned long long seed,
                                    const float* keep_mask, float* y, void* stream) {
  if (!x || !r || !y || n < 1 || !p_ok(p)) return ST_EINVAL;
  hipLaunchKernelGGL(k_dropout_add, dim3(grid_of(n)), dim3(NT), 0, (hipStream_t)stream, x, r, n, p, 1.0f / (1.0f - p),
                     seed, keep_mask, y);
  return (int)hipGetLastError();
}

extern "C" int stts_mfcc_frames(const float* mel, const float* dct, int B, int n_mels, int T, int n_mfcc, float* out,
                                void* stream) {
  return st_mfcc_frames(mel, dct, B, n_mels, T, n_mfcc, n_mfcc, out, (hipStream_t)stream);
}
