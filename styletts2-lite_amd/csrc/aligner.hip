// Text aligner (Modules/ASR/models.py ASRCNN, eval mode) and the monotonic alignment search (utils.py:14-27): the
// pieces around the conv engine.
//   k_mfcc_frames     mel [B][80][T] -> MFCC frames [B][T][ld] (the per-frame 80 -> 40 product with dct_mat)
//   k_groupnorm       GroupNorm(G) of [ReLU of] frames: one workgroup per (utterance, group), two-pass statistics
//   k_add             x += r (the ConvBlock residual: the conv engine's epilogue adds before it activates)
//   k_gemm_nt         C = act(A W^T + bias): every hoisted product of the S2S decoder and ctc_linear
//   k_embed           token rows with the unknown-token mask and the SOS row
//   k_transpose       pack time: the recurrent weights k-major, so that lanes read them side by side
//   k_s2s_decode      the attention decoder's recurrence: one persistent workgroup per utterance walks all steps
//   k_frames_to_ncl   frames [B][L][C] -> [B][C][L]
//   k_max_path        the Glow-TTS search: one workgroup per utterance, forward columns in LDS, backtrack on the device
// Everything here is fp32 with every sum in a fixed order and no atomics: a row of a batch is bitwise the B = 1 result.
#include "common.h"
#include "kernels.h"
#include "s2s_common.h"

namespace {

using namespace s2s;

constexpr int NT = 256;

unsigned grid_of(long long n) {
  const long long g = (n + NT - 1) / NT;
  return (unsigned)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

__global__ void __launch_bounds__(NT) k_mfcc_frames(const float* __restrict__ mel, const float* __restrict__ dct, int B,
                                                    int nm, int Tn, int nc, int ld, float* __restrict__ dst) {
  const long long n = (long long)B * Tn * ld;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int c = (int)(i % ld), t = (int)((i / ld) % Tn);
    const long long b = i / ((long long)ld * Tn);
    float v = 0.f;
    if (c < nc) {
      const float* mb = mel + (size_t)b * nm * Tn + t;
      for (int m = 0; m < nm; ++m) v = fmaf(mb[(size_t)m * Tn], dct[m * nc + c], v);
    }
    dst[i] = v;
  }
}

// statistics per (utterance, group) over the group's channels x all L frames: mean, then the biased variance around
// it; y may be x
__global__ void __launch_bounds__(NT) k_groupnorm(const float* x, int L, int ld, int C, int G, int relu,
                                                  const float* __restrict__ w, const float* __restrict__ bias, float eps,
                                                  float* y) {
  __shared__ float red[NT / 64];
  const int b = blockIdx.x / G, g = blockIdx.x % G, cg = C / G;
  const long long n = (long long)L * cg;
  const float* xb = x + (size_t)b * L * ld + (size_t)g * cg;
  float* yb = y + (size_t)b * L * ld + (size_t)g * cg;
  float s = 0.f;
  for (long long i = threadIdx.x; i < n; i += NT) {
    float v = xb[(size_t)(i / cg) * ld + (i % cg)];
    if (relu) v = fmaxf(v, 0.f);
    s += v;
  }
  const float mean = block_reduce<false>(s, red) / (float)n;
  float q = 0.f;
  for (long long i = threadIdx.x; i < n; i += NT) {
    float v = xb[(size_t)(i / cg) * ld + (i % cg)];
    if (relu) v = fmaxf(v, 0.f);
    q = fmaf(v - mean, v - mean, q);
  }
  const float rstd = 1.0f / sqrtf(block_reduce<false>(q, red) / (float)n + eps);
  for (long long i = threadIdx.x; i < n; i += NT) {
    const int c = (int)(i % cg);
    const size_t o = (size_t)(i / cg) * ld + c;
    float v = xb[o];
    if (relu) v = fmaxf(v, 0.f);
    yb[o] = (v - mean) * rstd * w[g * cg + c] + bias[g * cg + c];
  }
}

__global__ void __launch_bounds__(NT) k_add(float* __restrict__ x, const float* __restrict__ r, long long n) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) x[i] += r[i];
}

__global__ void __launch_bounds__(NT) k_frames_to_ncl(const float* __restrict__ x, int B, int L, int C,
                                                      float* __restrict__ out) {
  const long long n = (long long)B * C * L;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int l = (int)(i % L), c = (int)((i / L) % C);
    const long long b = i / ((long long)L * C);
    out[i] = x[((size_t)b * L + l) * C + c];
  }
}

// dst[c][r] = src[r * ld + c0 + c]
__global__ void __launch_bounds__(NT) k_transpose(const float* __restrict__ src, int rows, int cols, int ld, int c0,
                                                  float* __restrict__ dst) {
  const long long n = (long long)rows * cols;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int r = (int)(i % rows), c = (int)(i / rows);
    dst[i] = src[(size_t)r * ld + c0 + c];
  }
}

// C[r][n] = act(bias[n] + bias2[n] + sum_k A[r][k] W[n][k]), k ascending for every output (64 x 64 tiles, 4 x 4 per
// thread); act: 0 none, 1 ReLU, 2 tanh
constexpr int GT = 64, GK = 16;
__global__ void __launch_bounds__(NT) k_gemm_nt(const float* __restrict__ A, long long rows, int K, int lda,
                                                const float* __restrict__ W, int N, int ldw,
                                                const float* __restrict__ bias, const float* __restrict__ bias2, int act,
                                                float* __restrict__ Cm, int ldc) {
  __shared__ float As[GK][GT + 4], Ws[GK][GT + 4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long r0 = (long long)blockIdx.x * GT;
  const int n0 = blockIdx.y * GT;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < K; k0 += GK) {
#pragma unroll
    for (int j = 0; j < (GT * GK) / NT; ++j) {
      const int idx = tid + NT * j, rr = idx / GK, kk = idx % GK;
      const bool kin = k0 + kk < K;
      As[kk][rr] = (kin && r0 + rr < rows) ? A[(size_t)(r0 + rr) * lda + k0 + kk] : 0.f;
      Ws[kk][rr] = (kin && n0 + rr < N) ? W[(size_t)(n0 + rr) * ldw + k0 + kk] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GK; ++kk) {
      float a[4], w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = As[kk][ty * 4 + i];
        w[i] = Ws[kk][tx * 4 + i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], w[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long r = r0 + ty * 4 + i;
    if (r >= rows) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + tx * 4 + j;
      if (n >= N) continue;
      float v = acc[i][j] + (bias ? bias[n] : 0.f);
      if (bias2) v += bias2[n];
      if (act == 1) v = fmaxf(v, 0.f);
      if (act == 2) v = tanhf(v);
      Cm[(size_t)r * ldc + n] = v;
    }
  }
}

// decoder inputs [B][Tt + 1][E]: row 0 the SOS embedding, row t + 1 the token's (index `unk` where the mask is set)
__global__ void __launch_bounds__(NT) k_embed(const int* __restrict__ tok, const unsigned char* __restrict__ um, int B,
                                              int Tt, int E, int ntok, int sos, int unk, const float* __restrict__ emb,
                                              float* __restrict__ out) {
  const long long n = (long long)B * (Tt + 1) * E;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int e = (int)(i % E), t = (int)((i / E) % (Tt + 1));
    const long long b = i / ((long long)E * (Tt + 1));
    int id = sos;
    if (t > 0) {
      id = (um && um[b * Tt + t - 1]) ? unk : tok[b * Tt + t - 1];
      id = id < 0 ? 0 : (id >= ntok ? ntok - 1 : id);  // (the host refuses indices outside the table)
    }
    out[i] = emb[(size_t)id * E + e];
  }
}

// ------------------------------------------------------------------------------------------------ S2S recurrence
// ASRS2S.decode (Modules/ASR/models.py:150-176) for all Tt + 1 steps of one utterance per workgroup: the LSTMCell on
// [embedding part (hoisted, gin); context; h], the location-sensitive attention over the L memory frames, the context.
// The state (h, context, previous and cumulative weights) stays in LDS, the cell state in registers; the recurrent
// weights (k-major) and memory / processed memory stream from L2.  No workgroup waits for another one.
// SAVE (the training forward, stts_s2s_fwd_train): every step also stores what the backward reads, the four gate
// activations [B][steps][4 DH], the cell state [B][steps][DH] and the cumulative weights before the step [B][steps][L].
template <bool SAVE>
__global__ void __launch_bounds__(DT) k_s2s_decode(const float* __restrict__ gin, const float* __restrict__ wc_t,
                                                   const float* __restrict__ wq_t, const float* __restrict__ wloc_t,
                                                   const float* __restrict__ wd, const float* __restrict__ vv,
                                                   const float* __restrict__ mem, const float* __restrict__ pmem,
                                                   const unsigned char* __restrict__ mask, int L, int steps,
                                                   float* __restrict__ attn, float* __restrict__ hc,
                                                   float* __restrict__ sv_gates, float* __restrict__ sv_cell,
                                                   float* __restrict__ sv_cum) {
  extern __shared__ float dyn[];
  __shared__ float s_h[DH], s_ctx[DH], s_q[DH], s_gates[4 * DH], s_part[4 * DH], s_red[DT / 64];
  __shared__ float s_wloc[2 * DK * DF], s_conv[DTL * (DF + 1)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int Lr = (L + DTL - 1) / DTL * DTL, LP = Lr + 2 * DP;
  float* s_wp = dyn;            // previous weights, frame l at [DP + l], zeros around
  float* s_wc = dyn + LP;       // cumulative weights, the same layout
  float* s_e = dyn + 2 * LP;    // energies [L]
  for (int i = tid; i < 2 * LP; i += DT) dyn[i] = 0.f;
  for (int i = tid; i < 2 * DK * DF; i += DT) s_wloc[i] = wloc_t[i];
  if (tid < DH) s_h[tid] = s_ctx[tid] = 0.f;
  float cell = 0.f;  // (threads < DH)
  const int d0 = lane, d1 = lane + 64;
  float wd0[DF], wd1[DF];
#pragma unroll
  for (int f = 0; f < DF; ++f) {
    wd0[f] = wd[d0 * DF + f];
    wd1[f] = wd[d1 * DF + f];
  }
  const float v0 = vv[d0], v1 = vv[d1];
  const float* memb = mem + (size_t)b * L * DH;
  const float* pmb = pmem + (size_t)b * L * DH;
  const unsigned char* mb = mask ? mask + (size_t)b * L : nullptr;
  __syncthreads();
  for (int t = 0; t < steps; ++t) {
    // 1. LSTMCell gates (torch order i, f, g, o)
    {
      float a = gin[((size_t)b * steps + t) * (4 * DH) + tid];
#pragma unroll 8
      for (int k = 0; k < DH; ++k) a = fmaf(wc_t[(size_t)k * (4 * DH) + tid], s_ctx[k], a);
#pragma unroll 8
      for (int k = 0; k < DH; ++k) a = fmaf(wc_t[(size_t)(DH + k) * (4 * DH) + tid], s_h[k], a);
      s_gates[tid] = a;
    }
    __syncthreads();
    if (tid < DH) {
      const float ig = sigmoidf_(s_gates[tid]), fg = sigmoidf_(s_gates[DH + tid]);
      const float gg = tanhf(s_gates[2 * DH + tid]), og = sigmoidf_(s_gates[3 * DH + tid]);
      cell = fg * cell + ig * gg;
      const float h = og * tanhf(cell);
      s_h[tid] = h;
      hc[((size_t)b * steps + t) * (2 * DH) + tid] = h;
      if (SAVE) {
        float* g = sv_gates + ((size_t)b * steps + t) * (4 * DH);
        g[tid] = ig;
        g[DH + tid] = fg;
        g[2 * DH + tid] = gg;
        g[3 * DH + tid] = og;
        sv_cell[((size_t)b * steps + t) * DH + tid] = cell;
      }
    }
    __syncthreads();
    // 2. the query projection: 4 partial sums of 32 k each, added in part order
    {
      const int d = tid & (DH - 1), g = tid >> 7;
      float a = 0.f;
#pragma unroll 8
      for (int k = g * 32; k < g * 32 + 32; ++k) a = fmaf(wq_t[k * DH + d], s_h[k], a);
      s_part[g * DH + d] = a;
    }
    __syncthreads();
    if (tid < DH) s_q[tid] = ((s_part[tid] + s_part[DH + tid]) + s_part[2 * DH + tid]) + s_part[3 * DH + tid];
    __syncthreads();
    // 3-5. per tile of DTL frames: the location conv into LDS, then dense + tanh + v
    for (int l0 = 0; l0 < L; l0 += DTL) {
      loc_conv_tile(s_wp, s_wc, s_wloc, l0, L, s_conv);
      __syncthreads();
      const int lend = min(DTL, L - l0);
      for (int li = wave; li < lend; li += DT / 64) {
        const int l = l0 + li;
        if (mb && mb[l]) continue;  // (uniform over the wave) masked: -inf below
        const float* cv = s_conv + li * (DF + 1);
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int f = 0; f < DF; ++f) {
          const float x = cv[f];
          a0 = fmaf(wd0[f], x, a0);
          a1 = fmaf(wd1[f], x, a1);
        }
        float p = v0 * tanhf((s_q[d0] + a0) + pmb[(size_t)l * DH + d0]) +
                  v1 * tanhf((s_q[d1] + a1) + pmb[(size_t)l * DH + d1]);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) p += __shfl_xor(p, s);
        if (lane == 0) s_e[l] = p;
      }
      __syncthreads();
    }
    // 6. mask -> softmax over L (max-subtracted; each thread keeps its own frames)
    float m = -INFINITY;
    for (int l = tid; l < L; l += DT) {
      const float e = (mb && mb[l]) ? -INFINITY : s_e[l];
      s_e[l] = e;
      m = fmaxf(m, e);
    }
    m = block_reduce<true>(m, s_red);
    float sum = 0.f;
    for (int l = tid; l < L; l += DT) {
      const float ex = expf(s_e[l] - m);
      s_e[l] = ex;
      sum += ex;
    }
    sum = block_reduce<false>(sum, s_red);
    // 8. the new weights become the previous ones, cumulative += weights
    for (int l = tid; l < L; l += DT) {
      const float w = s_e[l] / sum;
      if (SAVE) sv_cum[((size_t)b * steps + t) * L + l] = s_wc[DP + l];
      s_wp[DP + l] = w;
      s_wc[DP + l] += w;
      if (attn) attn[((size_t)b * steps + t) * L + l] = w;
    }
    __syncthreads();
    // 7. context = weights . memory: 4 partial sums over l = g, g + 4, .., added in part order
    {
      const int d = tid & (DH - 1), g = tid >> 7;
      float a = 0.f;
      for (int l = g; l < L; l += 4) a = fmaf(s_wp[DP + l], memb[(size_t)l * DH + d], a);
      s_part[g * DH + d] = a;
    }
    __syncthreads();
    if (tid < DH) {
      const float cx = ((s_part[tid] + s_part[DH + tid]) + s_part[2 * DH + tid]) + s_part[3 * DH + tid];
      s_ctx[tid] = cx;
      hc[((size_t)b * steps + t) * (2 * DH) + DH + tid] = cx;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ alignment search
// value [B][Tx][Ty] -> vt [B][Ty][Tx], so that a column of the search is contiguous
__global__ void __launch_bounds__(NT) k_value_t(const float* __restrict__ v, int B, int Tx, int Ty,
                                                float* __restrict__ vt) {
  const long long n = (long long)B * Tx * Ty;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int x = (int)(i % Tx), y = (int)((i / Tx) % Ty);
    const long long b = i / ((long long)Tx * Ty);
    vt[i] = v[((size_t)b * Tx + x) * Ty + y];
  }
}

// One workgroup per utterance.  Column y of the forward pass needs column y - 1 only: two columns live in LDS, and
// what the backtrack asks of column y - 1 ("step down at (x, y)": x == y, or v[x][y-1] < v[x-1][y-1]) is stored as
// one byte per cell while both values are at hand.  One add and one max per cell, as the host restatement.
// The lengths are host values: they travel as launch arguments, MP_CHUNK utterances a launch.
constexpr int MP_CHUNK = 64;
struct MPLens {
  int tx[MP_CHUNK], ty[MP_CHUNK];
};
__global__ void __launch_bounds__(NT) k_max_path(const float* __restrict__ vt, MPLens lens, int b0, int Tx, int Ty,
                                                 float* __restrict__ path, unsigned char* __restrict__ dec) {
  extern __shared__ float col[];  // [2][Tx]
  const int b = b0 + blockIdx.x, tx = lens.tx[blockIdx.x], ty = lens.ty[blockIdx.x];
  float* pb = path + (size_t)b * Tx * Ty;
  for (long long i = threadIdx.x; i < (long long)Tx * Ty; i += NT) pb[i] = 0.f;
  if (tx < 1 || tx > ty || tx > Tx || ty > Ty) return;  // (refused on the host)
  const float* vb = vt + (size_t)b * Tx * Ty;
  unsigned char* db = dec + (size_t)b * Tx * Ty;
  const float NEG = -1e9f;
  float* prev = col;
  float* cur = col + Tx;
  for (int y = 0; y < ty; ++y) {
    const int xlo = max(0, tx + y - ty), xhi = min(tx, y + 1);
    for (int x = xlo + (int)threadIdx.x; x < xhi; x += NT) {
      const float vc = x == y ? NEG : prev[x];
      const float vp = x == 0 ? (y == 0 ? 0.f : NEG) : prev[x - 1];
      cur[x] = (vp > vc ? vp : vc) + vb[(size_t)y * Tx + x];
      db[(size_t)y * Tx + x] = (x == y || (x > 0 && vc < vp)) ? 1 : 0;
    }
    __syncthreads();
    float* t = prev;
    prev = cur;
    cur = t;
  }
  if (threadIdx.x == 0) {
    int idx = tx - 1;
    for (int y = ty - 1; y >= 0; --y) {
      pb[(size_t)idx * Ty + y] = 1.f;
      if (idx != 0 && db[(size_t)y * Tx + idx]) --idx;
    }
  }
}

}  // namespace

int st_mfcc_frames(const float* mel, const float* dct, int B, int nm, int T, int nc, int ld, float* dst, hipStream_t s) {
  if (!mel || !dct || !dst || B <= 0 || nm <= 0 || T <= 0 || nc <= 0 || ld < nc) return ST_EINVAL;
  hipLaunchKernelGGL(k_mfcc_frames, dim3(grid_of((long long)B * T * ld)), dim3(NT), 0, s, mel, dct, B, nm, T, nc, ld, dst);
  return (int)hipGetLastError();
}

int st_groupnorm(const float* x, int B, int L, int ld, int C, int G, int relu, const float* w, const float* b, float eps,
                 float* y, hipStream_t s) {
  if (!x || !y || !w || !b || B <= 0 || L <= 0 || C <= 0 || G <= 0 || C % G || ld < C) return ST_EINVAL;
  hipLaunchKernelGGL(k_groupnorm, dim3((unsigned)(B * G)), dim3(NT), 0, s, x, L, ld, C, G, relu, w, b, eps, y);
  return (int)hipGetLastError();
}

int st_add(float* x, const float* r, long long n, hipStream_t s) {
  if (!x || !r || n <= 0) return ST_EINVAL;
  hipLaunchKernelGGL(k_add, dim3(grid_of(n)), dim3(NT), 0, s, x, r, n);
  return (int)hipGetLastError();
}

int st_frames_to_ncl(const float* x, int B, int L, int C, float* out, hipStream_t s) {
  if (!x || !out || B <= 0 || L <= 0 || C <= 0) return ST_EINVAL;
  hipLaunchKernelGGL(k_frames_to_ncl, dim3(grid_of((long long)B * L * C)), dim3(NT), 0, s, x, B, L, C, out);
  return (int)hipGetLastError();
}

int st_transpose(const float* src, int rows, int cols, int ld, int c0, float* dst, hipStream_t s) {
  if (!src || !dst || rows <= 0 || cols <= 0 || c0 < 0 || ld < c0 + cols) return ST_EINVAL;
  hipLaunchKernelGGL(k_transpose, dim3(grid_of((long long)rows * cols)), dim3(NT), 0, s, src, rows, cols, ld, c0, dst);
  return (int)hipGetLastError();
}

int st_gemm_nt(const float* A, long long rows, int K, int lda, const float* W, int N, int ldw, const float* bias,
               const float* bias2, int act, float* C, int ldc, hipStream_t s) {
  if (!A || !W || !C || rows <= 0 || K <= 0 || N <= 0 || lda < K || ldw < K || ldc < N) return ST_EINVAL;
  const long long gx = (rows + GT - 1) / GT;
  if (gx > 0x7fffffffLL) return ST_EINVAL;
  hipLaunchKernelGGL(k_gemm_nt, dim3((unsigned)gx, (unsigned)((N + GT - 1) / GT)), dim3(NT), 0, s, A, rows, K, lda, W, N,
                     ldw, bias, bias2, act, C, ldc);
  return (int)hipGetLastError();
}

int st_s2s_embed(const int* tok, const unsigned char* unk_mask, int B, int Tt, int E, int ntok, const float* emb,
                 float* out, hipStream_t s) {
  if (!tok || !emb || !out || B <= 0 || Tt <= 0 || E <= 0 || ntok < 4) return ST_EINVAL;
  hipLaunchKernelGGL(k_embed, dim3(grid_of((long long)B * (Tt + 1) * E)), dim3(NT), 0, s, tok, unk_mask, B, Tt, E, ntok,
                     1, 3, emb, out);
  return (int)hipGetLastError();
}

namespace {
template <bool SAVE>
int s2s_decode_launch(const float* gin, const float* wc_t, const float* wq_t, const float* wloc_t, const float* wd,
                      const float* v, const float* mem, const float* pmem, const unsigned char* mask, int B, int L,
                      int steps, float* attn, float* hc, float* sv_gates, float* sv_cell, float* sv_cum,
                      hipStream_t s) {
  if (!gin || !wc_t || !wq_t || !wloc_t || !wd || !v || !mem || !pmem || !hc) return ST_EINVAL;
  if (B <= 0 || L <= 0 || L > ST_ALIGNER_MAX_L || steps <= 0) return ST_EINVAL;
  const size_t lds = ((size_t)2 * padded(L) + L) * sizeof(float);
  static std::mutex mu;
  static bool raised = false;
  {
    std::lock_guard<std::mutex> lk(mu);
    if (!raised) {  // the longest utterances need more than the default 64 KB of LDS per workgroup
      const size_t lmax = ((size_t)2 * padded(ST_ALIGNER_MAX_L) + ST_ALIGNER_MAX_L) * sizeof(float);
      ST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_s2s_decode<SAVE>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lmax));
      raised = true;
    }
  }
  hipLaunchKernelGGL(k_s2s_decode<SAVE>, dim3((unsigned)B), dim3(DT), lds, s, gin, wc_t, wq_t, wloc_t, wd, v, mem, pmem,
                     mask, L, steps, attn, hc, sv_gates, sv_cell, sv_cum);
  return (int)hipGetLastError();
}
}  // namespace

int st_s2s_decode(const float* gin, const float* wc_t, const float* wq_t, const float* wloc_t, const float* wd,
                  const float* v, const float* mem, const float* pmem, const unsigned char* mask, int B, int L, int steps,
                  float* attn, float* hc, hipStream_t s) {
  return s2s_decode_launch<false>(gin, wc_t, wq_t, wloc_t, wd, v, mem, pmem, mask, B, L, steps, attn, hc, nullptr,
                                  nullptr, nullptr, s);
}

int st_s2s_decode_train(const float* gin, const float* wc_t, const float* wq_t, const float* wloc_t, const float* wd,
                        const float* v, const float* mem, const float* pmem, const unsigned char* mask, int B, int L,
                        int steps, float* attn, float* hc, float* sv_gates, float* sv_cell, float* sv_cum,
                        hipStream_t s) {
  if (!attn || !sv_gates || !sv_cell || !sv_cum) return ST_EINVAL;
  return s2s_decode_launch<true>(gin, wc_t, wq_t, wloc_t, wd, v, mem, pmem, mask, B, L, steps, attn, hc, sv_gates,
                                 sv_cell, sv_cum, s);
}

long long st_max_path_workspace_bytes(int B, int Tx, int Ty) {
  if (B <= 0 || Tx <= 0 || Ty <= 0 || Tx > ST_MAXPATH_MAX_TX) return ST_EINVAL;
  const long long n = (long long)B * Tx * Ty;
  return (n * 4 + 255) / 256 * 256 + n;
}

int st_max_path(const float* value, const int* tx_len, const int* ty_len, int B, int Tx, int Ty, float* path, void* ws,
                long long ws_bytes, hipStream_t s) {
  if (!value || !tx_len || !ty_len || !path) return ST_EINVAL;
  const long long need = st_max_path_workspace_bytes(B, Tx, Ty);
  if (need < 0) return (int)need;
  if (!ws || ws_bytes < need) return ST_EWORKSPACE;
  const long long n = (long long)B * Tx * Ty;
  float* vt = reinterpret_cast<float*>(ws);
  unsigned char* dec = reinterpret_cast<unsigned char*>(ws) + (n * 4 + 255) / 256 * 256;
  hipLaunchKernelGGL(k_value_t, dim3(grid_of(n)), dim3(NT), 0, s, value, B, Tx, Ty, vt);
  for (int b0 = 0; b0 < B; b0 += MP_CHUNK) {
    MPLens lens;
    const int nb = B - b0 < MP_CHUNK ? B - b0 : MP_CHUNK;
    for (int i = 0; i < MP_CHUNK; ++i) {
      lens.tx[i] = i < nb ? tx_len[b0 + i] : 0;
      lens.ty[i] = i < nb ? ty_len[b0 + i] : 0;
    }
    hipLaunchKernelGGL(k_max_path, dim3((unsigned)nb), dim3(NT), (size_t)2 * Tx * sizeof(float), s, vt, lens, b0, Tx, Ty,
                       path, dec);
  }
  return (int)hipGetLastError();
}
