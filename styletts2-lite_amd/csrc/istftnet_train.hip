// Training layers of the iSTFTNet decoder (reference Modules/istftnet.py) that the conv engines and the
// AdaIN pairs do not cover (include/stts2_train.h), gfx950, fp32 frames [B][L][C]:
//   stts_cstft_fwd   CustomSTFT.transform of the harmonic source (:207-243): st_stft (csrc/misc.hip) at fp32.
//                    The reference computes it under no_grad (:544-550): no backward.
//   k_padl_add*      the last stage's reflection_pad((1, 0)) fused with x + x_source (:558-561) and its adjoint
//   k_cistft_fwd     exp / sin -> CustomSTFT.inverse (:571-573, :246-293).  A workgroup owns HD_TF hops of output
//                    samples: it copies the contributing frames of `post` (the tile and its halo, one contiguous
//                    range) and both inverse bases into LDS, evaluates exp / sin / cos / sin once per (frame, bin)
//                    in place, then overlap-adds from LDS, one sample per thread.
//   k_cistft_bwd     the exact adjoint: a workgroup owns HD_TF frames, stages their window of dy in LDS (zero
//                    outside the kept samples: the trim's gradient) and the bases, one (frame, bin) per thread:
//                    two n_fft-term dot products, then the chain through cos / sin / exp / sin from `post`.
// LDS rows are padded to an odd stride (frames: 2 nb | 1, bases: n_fft | 1), so lanes on different frames or
// different bins fall on different banks.  No atomics, fixed summation order: bitwise reproducible run to run.
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
constexpr int HD_TF = 64;      // hops of output per forward workgroup / frames per backward workgroup
constexpr int HD_NFFT_MAX = 64;

inline unsigned grid_for(long long n, int per_thread = 1) {
  long long b = (n + (long long)NT * per_thread - 1) / ((long long)NT * per_thread);
  return (unsigned)std::max<long long>(1, std::min<long long>(b, 1 << 20));
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// n_fft even in [4, 64], 1 <= hop <= n_fft: the CustomSTFT geometries of this file
inline bool stft_geo_ok(int n_fft, int hop) {
  return n_fft >= 4 && n_fft <= HD_NFFT_MAX && !(n_fft & 1) && hop >= 1 && hop <= n_fft;
}

// ------------------------------------------------------------------ reflection_pad((1, 0)) + add
// y [B][L + 1][C]: y[0] = x[1] + src[0], y[t] = x[t - 1] + src[t].  V = float or float4 (C counts V elements).
template <typename V>
__device__ __forceinline__ V vadd(V a, V b);
template <>
__device__ __forceinline__ float vadd<float>(float a, float b) { return a + b; }
template <>
__device__ __forceinline__ float4 vadd<float4>(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

template <typename V>
__global__ void __launch_bounds__(256) k_padl_add(const V* __restrict__ x, const V* __restrict__ src, int L, int C,
                                                  long long n, V* __restrict__ y) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const long long r = i / C;
    const int c = (int)(i - r * C);
    const long long b = r / (L + 1);
    const int t = (int)(r - b * (L + 1));
    const int xs = t == 0 ? 1 : t - 1;
    y[i] = vadd(x[(b * L + xs) * C + c], src[i]);
  }
}

// dx [B][L][C]: dx[t] = dy[t + 1] + (t == 1 ? dy[0] : 0)
template <typename V>
__global__ void __launch_bounds__(256) k_padl_add_bwd(const V* __restrict__ dy, int L, int C, long long n,
                                                      V* __restrict__ dx) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const long long r = i / C;
    const int c = (int)(i - r * C);
    const long long b = r / L;
    const int t = (int)(r - b * L);
    const V* row0 = dy + b * (L + 1) * C + c;
    V v = row0[(long long)(t + 1) * C];
    if (t == 1) v = vadd(v, row0[0]);
    dx[i] = v;
  }
}

// ------------------------------------------------------------------ exp / sin -> CustomSTFT.inverse
struct HeadGeo {
  int nb, W, ldp, ldb, nfmax, ndymax, Lout, tiles_fwd, tiles_bwd;
  size_t lds_fwd, lds_bwd;
};

int head_geo(int B, int F, int n_fft, int hop, HeadGeo* g) {
  if (B < 1 || B > 65535 || F < 2 || !stft_geo_ok(n_fft, hop)) return ST_EINVAL;
  const long long lout = (long long)(F - 1) * hop;
  if (lout > 0x7fffffffLL - 2 * HD_NFFT_MAX || (long long)F * (n_fft + 2) > 0x7fffffffLL) return ST_EINVAL;
  g->nb = n_fft / 2 + 1;
  g->W = 2 * g->nb;
  g->ldp = g->W | 1;
  g->ldb = n_fft | 1;
  g->nfmax = HD_TF + (n_fft - 2) / hop + 2;  // the tile's frames and its ceil(n_fft / hop) - 1 frames of halo
  g->ndymax = (HD_TF - 1) * hop + n_fft;
  g->Lout = (int)lout;
  g->tiles_fwd = (F - 1 + HD_TF - 1) / HD_TF;
  g->tiles_bwd = (F + HD_TF - 1) / HD_TF;
  const size_t bases = (size_t)2 * g->nb * g->ldb;
  g->lds_fwd = (bases + (size_t)g->nfmax * g->ldp) * sizeof(float);
  g->lds_bwd = (bases + (size_t)g->ndymax) * sizeof(float);
  if (g->lds_fwd > 64 * 1024 || g->lds_bwd > 64 * 1024) return ST_EINVAL;
  return ST_OK;
}

// both bases [nb][n_fft] -> LDS rows of stride ldb
__device__ __forceinline__ void stage_bases(const float* __restrict__ br, const float* __restrict__ bi, int nb,
                                            int n_fft, int ldb, float* sbr, float* sbi) {
  for (int i = threadIdx.x; i < nb * n_fft; i += NT) {
    const int k = i / n_fft, n = i - k * n_fft;
    sbr[k * ldb + n] = br[i];
    sbi[k * ldb + n] = bi[i];
  }
}

__global__ void __launch_bounds__(256) k_cistft_fwd(const float* __restrict__ post, const float* __restrict__ br,
                                                    const float* __restrict__ bi, int F, int n_fft, int hop, int ldp,
                                                    int ldb, int nfmax, int Lout, float* __restrict__ audio) {
  extern __shared__ float lds[];
  const int nb = n_fft / 2 + 1, W = 2 * nb, P = n_fft / 2;
  float* sbr = lds;
  float* sbi = sbr + nb * ldb;
  float* sp = sbi + nb * ldb;  // [nf][ldp]: post, then re (bins 0 .. nb - 1) and im (nb .. 2 nb - 1) in place
  const int b = blockIdx.y;
  const int j0 = blockIdx.x * HD_TF * hop;
  const int j1 = min(j0 + HD_TF * hop, Lout);
  // frames t with 0 <= j + P - t hop < n_fft for some j in [j0, j1)
  const int lo = j0 - P + 1;
  const int tlo = lo <= 0 ? 0 : (lo + hop - 1) / hop;
  const int thi = min((j1 - 1 + P) / hop, F - 1);
  const int nf = min(thi - tlo + 1, nfmax);
  stage_bases(br, bi, nb, n_fft, ldb, sbr, sbi);
  const float* src = post + ((size_t)b * F + tlo) * W;
  for (int i = threadIdx.x; i < nf * W; i += NT) {
    const int t = i / W, c = i - t * W;
    sp[t * ldp + c] = src[i];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nf * nb; i += NT) {
    const int t = i / nb, k = i - t * nb;
    float* row = sp + t * ldp;
    const float mag = expf(row[k]);
    const float ph = sinf(row[nb + k]);
    float sn, cs;
    sincosf(ph, &sn, &cs);
    row[k] = mag * cs;
    row[nb + k] = mag * sn;
  }
  __syncthreads();
  float* out = audio + (size_t)b * Lout;
  for (int j = j0 + threadIdx.x; j < j1; j += NT) {
    const int p = j + P;
    const int l = p - n_fft + 1;
    const int ta = max(l <= 0 ? 0 : (l + hop - 1) / hop, tlo);
    const int tb = min(p / hop, tlo + nf - 1);
    float rr = 0.f, ii = 0.f;
    for (int t = ta; t <= tb; ++t) {
      const int n = p - t * hop;
      const float* row = sp + (t - tlo) * ldp;
      for (int k = 0; k < nb; ++k) {
        rr = fmaf(row[k], sbr[k * ldb + n], rr);
        ii = fmaf(row[nb + k], sbi[k * ldb + n], ii);
      }
    }
    out[j] = rr - ii;
  }
}

__global__ void __launch_bounds__(256) k_cistft_bwd(const float* __restrict__ post, const float* __restrict__ br,
                                                    const float* __restrict__ bi, const float* __restrict__ dy, int F,
                                                    int n_fft, int hop, int ldb, int ndymax, int Lout,
                                                    float* __restrict__ dpost) {
  extern __shared__ float lds[];
  const int nb = n_fft / 2 + 1, W = 2 * nb, P = n_fft / 2;
  float* sbr = lds;
  float* sbi = sbr + nb * ldb;
  float* sdy = sbi + nb * ldb;  // dy[jlo + i], zero outside [0, Lout)
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * HD_TF;
  const int ntf = min(HD_TF, F - t0);
  const int jlo = t0 * hop - P;
  const int ndy = min((ntf - 1) * hop + n_fft, ndymax);
  stage_bases(br, bi, nb, n_fft, ldb, sbr, sbi);
  const float* g = dy + (size_t)b * Lout;
  for (int i = threadIdx.x; i < ndy; i += NT) {
    const int j = jlo + i;
    sdy[i] = (j >= 0 && j < Lout) ? g[j] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ntf * nb; i += NT) {
    const int t = i / nb, k = i - t * nb;
    const float* d = sdy + t * hop;
    const float* wr = sbr + k * ldb;
    const float* wi = sbi + k * ldb;
    float dre = 0.f, dim = 0.f;
    for (int n = 0; n < n_fft; ++n) {
      dre = fmaf(d[n], wr[n], dre);
      dim = fmaf(d[n], wi[n], dim);
    }
    dim = -dim;
    const size_t row = ((size_t)b * F + t0 + t) * W;
    const float y = post[row + nb + k];
    const float mag = expf(post[row + k]);
    float sy, cy, sn, cs;
    sincosf(y, &sy, &cy);
    sincosf(sy, &sn, &cs);  // ph = sin(y)
    const float dmag = dre * cs + dim * sn;
    const float dph = mag * (dim * cs - dre * sn);
    dpost[row + k] = dmag * mag;
    dpost[row + nb + k] = dph * cy;
  }
}

}  // namespace

// ================================================================== C-ABI
extern "C" int stts_cstft_fwd(const float* wave, const float* wr, const float* wi, int B, int L, int n_fft, int hop,
                              float* out, void* stream) {
  if (B < 1 || B > 65535 || L < 1 || !stft_geo_ok(n_fft, hop)) return ST_EINVAL;
  if (((long long)L / hop + 1) * (n_fft / 2 + 1) > 0x7fffffffLL - 256) return ST_EINVAL;
  if (!wave || !wr || !wi || !out) return ST_EINVAL;
  return st_stft(wave, B, L, n_fft, hop, wr, wi, out, n_fft + 2, ST_FP32, (hipStream_t)stream);
}

extern "C" int stts_padl_add_fwd(const float* x, const float* src, int B, int L, int C, float* y, void* stream) {
  if (B < 1 || L < 2 || C < 1 || L == 0x7fffffff) return ST_EINVAL;
  if (!x || !src || !y) return ST_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long long n = (long long)B * (L + 1) * C;
  if (C % 4 == 0 && aligned16(x) && aligned16(src) && aligned16(y))
    hipLaunchKernelGGL(k_padl_add<float4>, dim3(grid_for(n / 4, 2)), dim3(NT), 0, s, (const float4*)x,
                       (const float4*)src, L, C / 4, n / 4, (float4*)y);
  else
    hipLaunchKernelGGL(k_padl_add<float>, dim3(grid_for(n, 4)), dim3(NT), 0, s, x, src, L, C, n, y);
  return (int)hipGetLastError();
}

extern "C" int stts_padl_add_bwd(const float* dy, int B, int L, int C, float* dx, void* stream) {
  if (B < 1 || L < 2 || C < 1 || L == 0x7fffffff) return ST_EINVAL;
  if (!dy || !dx) return ST_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long long n = (long long)B * L * C;
  if (C % 4 == 0 && aligned16(dy) && aligned16(dx))
    hipLaunchKernelGGL(k_padl_add_bwd<float4>, dim3(grid_for(n / 4, 2)), dim3(NT), 0, s, (const float4*)dy, L, C / 4,
                       n / 4, (float4*)dx);
  else
    hipLaunchKernelGGL(k_padl_add_bwd<float>, dim3(grid_for(n, 4)), dim3(NT), 0, s, dy, L, C, n, dx);
  return (int)hipGetLastError();
}

extern "C" int stts_cistft_head_fwd(const float* post, const float* br, const float* bi, int B, int F, int n_fft,
                                    int hop, float* audio, void* stream) {
  HeadGeo g;
  ST_CHECK(head_geo(B, F, n_fft, hop, &g));
  if (!post || !br || !bi || !audio) return ST_EINVAL;
  hipLaunchKernelGGL(k_cistft_fwd, dim3(g.tiles_fwd, B), dim3(NT), g.lds_fwd, (hipStream_t)stream, post, br, bi, F,
                     n_fft, hop, g.ldp, g.ldb, g.nfmax, g.Lout, audio);
  return (int)hipGetLastError();
}

extern "C" int stts_cistft_head_bwd(const float* post, const float* br, const float* bi, const float* dy, int B, int F,
                                    int n_fft, int hop, float* dpost, void* stream) {
  HeadGeo g;
  ST_CHECK(head_geo(B, F, n_fft, hop, &g));
  if (!post || !br || !bi || !dy || !dpost) return ST_EINVAL;
  hipLaunchKernelGGL(k_cistft_bwd, dim3(g.tiles_bwd, B), dim3(NT), g.lds_bwd, (hipStream_t)stream, post, br, bi, dy, F,
                     n_fft, hop, g.ldb, g.ndymax, g.Lout, dpost);
  return (int)hipGetLastError();
}
