// Training the aligner's S2S decoder (Modules/ASR/models.py ASRS2S :118-176) and the two losses that reach it
// (train.py:301-306).
//   stts_s2s_fwd_train   the recurrence of k_s2s_decode (aligner.hip, the same kernel body) that also keeps each
//                        step's gate activations, cell state and cumulative weights; products outside it as GEMMs
//   k_s2s_bwd            back-propagation through time: one persistent workgroup per utterance walks the steps
//                        backwards; the tanh argument is recomputed tile by tile from the saved weights
//   stts_s2s_bwd         the hoisted products before (project_to_n_symbols, dropout, tanh, project_to_hidden) and
//                        after the loop (every weight gradient, the embedding scatter, dmemory)
//   k_s2s_loss, k_mono_loss   loss_s2s and loss_mono, value and gradient in one launch each
// Everything is fp32 (loss sums fp64) with every sum in a fixed order and no atomics; parameter gradients sum the
// utterances in utterance order, and a row of dmemory is bitwise the B = 1 result.  No workgroup waits for another.
#include "common.h"
#include "kernels.h"
#include "s2s_common.h"
#include "s2s_layout.h"
#include "stts2_train.h"

namespace {

using namespace s2s;
static_assert(kD == DH, "layout and kernel widths");
static_assert(STTS_S2S_BWD_MAX_L == ST_S2S_BWD_MAX_L, "the header states the backward's frame cap");

constexpr int NT = 256;
unsigned grid_of(long long n) {
  const long long g = (n + NT - 1) / NT;
  return (unsigned)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

// ------------------------------------------------------------------------------------------------ small kernels
__global__ void __launch_bounds__(NT) k_mul(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                            float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) out[i] = a[i] * b[i];
}

// gradient at project_to_hidden's tanh argument: (dhidden + dhd * scale) (1 - hidden^2); dhidden, dhd, scale nullable
__global__ void __launch_bounds__(NT) k_hidden_bwd(const float* __restrict__ dhidden, const float* __restrict__ dhd,
                                                   const float* __restrict__ scale, const float* __restrict__ hidden,
                                                   long long n, float* __restrict__ dpre) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    float g = dhidden ? dhidden[i] : 0.f;
    if (dhd) g += scale ? dhd[i] * scale[i] : dhd[i];
    const float h = hidden[i];
    dpre[i] = g * (1.0f - h * h);
  }
}

// out1[c] (and out2[c]) = sum_r x[r][c], r ascending
__global__ void __launch_bounds__(NT) k_colsum(const float* __restrict__ x, long long rows, int cols,
                                               float* __restrict__ out1, float* __restrict__ out2) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= cols) return;
  float a = 0.f;
  for (long long r = 0; r < rows; ++r) a += x[(size_t)r * cols + c];
  if (out1) out1[c] = a;
  if (out2) out2[c] = a;
}

// the LSTMCell's inputs of step t: xh[row] = [emb_t; context_{t-1}], hprev[row] = h_{t-1} (zeros at t = 0)
__global__ void __launch_bounds__(NT) k_lstm_inputs(const float* __restrict__ emb, const float* __restrict__ hc, int B,
                                                    int steps, int E, float* __restrict__ xh,
                                                    float* __restrict__ hprev) {
  const int W = E + 2 * DH;
  const long long n = (long long)B * steps * W;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int c = (int)(i % W);
    const long long row = i / W;
    const int t = (int)(row % steps);
    if (c < E) {
      xh[(size_t)row * (E + DH) + c] = emb[(size_t)row * E + c];
    } else if (c < E + DH) {
      xh[(size_t)row * (E + DH) + c] = t > 0 ? hc[(size_t)(row - 1) * (2 * DH) + DH + (c - E)] : 0.f;
    } else {
      hprev[(size_t)row * DH + (c - E - DH)] = t > 0 ? hc[(size_t)(row - 1) * (2 * DH) + (c - E - DH)] : 0.f;
    }
  }
}

// the embedding rows the decoder read: SOS (1) at step 0, then the tokens, 3 where the unknown mask is set
__global__ void __launch_bounds__(NT) k_eff_tokens(const int* __restrict__ tok, const unsigned char* __restrict__ um,
                                                   int B, int Tt, int ntok, long long* __restrict__ out) {
  const long long n = (long long)B * (Tt + 1);
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int t = (int)(i % (Tt + 1));
    const long long b = i / (Tt + 1);
    int id = 1;
    if (t > 0) {
      id = (um && um[b * Tt + t - 1]) ? 3 : tok[b * Tt + t - 1];
      id = id < 0 ? 0 : (id >= ntok ? ntok - 1 : id);  // (as k_embed; the host refuses indices outside the table)
    }
    out[i] = id;
  }
}

// dmem[b][l][d] += sum_t attn[b][t][l] dctx[b][t][d], t ascending (the context's share of dmemory)
__global__ void __launch_bounds__(NT) k_attn_ctx_bwd(const float* __restrict__ attn, const float* __restrict__ dctx,
                                                     int B, int L, int steps, float* __restrict__ dmem) {
  const long long n = (long long)B * L * DH;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    const int d = (int)(i % DH), l = (int)((i / DH) % L);
    const long long b = i / ((long long)DH * L);
    const float* ab = attn + (size_t)b * steps * L + l;
    const float* cb = dctx + (size_t)b * steps * DH + d;
    float a = 0.f;
    for (int t = 0; t < steps; ++t) a = fmaf(ab[(size_t)t * L], cb[(size_t)t * DH], a);
    dmem[i] += a;
  }
}

// out[j] = sum_b part[b][n] in utterance order; loc: part is [c][k][f] (as the kernel keeps the taps), out [f][c][k]
__global__ void __launch_bounds__(NT) k_sum_partials(const float* __restrict__ part, int B, int n, int loc,
                                                     float* __restrict__ out) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  float a = 0.f;
  for (int b = 0; b < B; ++b) a += part[(size_t)b * n + i];
  if (loc) {
    const int f = i % DF, ck = i / DF;
    out[f * (2 * DK) + ck] = a;
  } else {
    out[i] = a;
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

// ------------------------------------------------------------------------------------------------ BPTT
// Per step t = steps - 1 .. 0 of utterance b, with w_t = attn[t], w_{t-1} and cum_{t-1} the location conv's inputs:
//   dctx_t  = dHC[t][context half] + (W_ih[:, E:]^T dgates_{t+1})
//   dw      = dattn[t] + mem dctx_t + dw_prev + dcum;   de = w_t (dw - sum w_t dw)
//   per tile: conv -> dense -> tanh recomputed; dpre = de v (1 - tanh^2) feeds dv, dq, dpmem, d(dense weight) and
//   dconv = dpre W_dense; dconv feeds d(conv weight) and, through the transposed 63-tap conv, dw_prev (channel 0:
//   the gradient of w_{t-1}) and dcum (channel 1: cum_{t-1}, which also passes dcum_t on)
//   dh      = dHC[t][h half] + (W_hh^T dgates_{t+1}) + W_query^T dq;  LSTMCell backward -> dgates_t, dcell
// Carried in LDS / registers: dh and dctx from the next step's gates, dcell, dw_prev[L], dcum[L].
constexpr int BSTRIP = 12;  // output frames per thread of the transposed conv: 16 strips cover DTL + 2 DP frames
static_assert((DT / DF) * BSTRIP >= DTL + 2 * DP, "transposed conv strips");
constexpr size_t kBwdStaticLds =
    sizeof(float) * (2 * DK * DF + 2 * DTL * (DF + 1) + 4 * DH + 4 * DH + (DT / 64) * DH + 5 * DH + DT / 64);
constexpr size_t bwd_dyn_lds(int L) { return sizeof(float) * ((size_t)4 * padded(L) + L); }
static_assert(kBwdStaticLds + bwd_dyn_lds(ST_S2S_BWD_MAX_L) <= 160 * 1024, "the backward's frame cap fits a CU's LDS");

__global__ void __launch_bounds__(DT) k_s2s_bwd(
    const float* __restrict__ mem, const float* __restrict__ pmem, const unsigned char* __restrict__ mask,
    const float* __restrict__ attn, const float* __restrict__ cum, const float* __restrict__ gates,
    const float* __restrict__ cellv, const float* __restrict__ qv, const float* __restrict__ dhc,
    const float* __restrict__ dattn, const float* __restrict__ wq, const float* __restrict__ wih_ctx, int ld_ih,
    const float* __restrict__ whh, const float* __restrict__ wloc, const float* __restrict__ wd,
    const float* __restrict__ vv, int L, int steps, float* __restrict__ dgates, float* __restrict__ dq_out,
    float* __restrict__ dctx_out, float* __restrict__ dpmem, float* __restrict__ pv, float* __restrict__ pwd,
    float* __restrict__ ploc) {
  extern __shared__ float dyn[];
  __shared__ float s_wloc[2 * DK * DF], s_conv[DTL * (DF + 1)], s_dconv[DTL * (DF + 1)];
  __shared__ float s_part[4 * DH], s_dg[4 * DH], s_wv[(DT / 64) * DH];
  __shared__ float s_dhc[DH], s_dctxc[DH], s_dctxt[DH], s_dq[DH], s_q[DH], s_red[DT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int LP = padded(L);
  float* s_wp = dyn;             // w_{t-1}, frame l at [DP + l], zeros around
  float* s_wc = dyn + LP;        // cum_{t-1}, the same layout
  float* s_dwp = dyn + 2 * LP;   // gradient of w_t from step t + 1's conv (channel 0)
  float* s_dcum = dyn + 3 * LP;  // gradient of cum_t from all later steps' convs (channel 1)
  float* s_de = dyn + 4 * LP;    // dw, then de [L]
  for (int i = tid; i < 4 * LP; i += DT) dyn[i] = 0.f;
  for (int i = tid; i < 2 * DK * DF; i += DT) {  // [f][c][k] -> [c][k][f]
    const int f = i % DF, ck = i / DF;
    s_wloc[i] = wloc[f * (2 * DK) + ck];
  }
  if (tid < DH) s_dhc[tid] = s_dctxc[tid] = 0.f;
  float dcell = 0.f;  // (threads < DH)
  const int d0 = lane, d1 = lane + 64;
  float wd0[DF], wd1[DF], dwd0[DF] = {}, dwd1[DF] = {};
#pragma unroll
  for (int f = 0; f < DF; ++f) {
    wd0[f] = wd[d0 * DF + f];
    wd1[f] = wd[d1 * DF + f];
  }
  const float v0 = vv[d0], v1 = vv[d1];
  float dv0 = 0.f, dv1 = 0.f;
  float dloc[8] = {};
  const int cf = tid & (DF - 1), cgrp = tid >> 5;  // phase-2 roles: filter, and tap group / output strip
  const int cc = cgrp >> 3, ck0 = (cgrp & 7) * 8;
  const float* memb = mem + (size_t)b * L * DH;
  const float* pmb = pmem + (size_t)b * L * DH;
  float* dpm = dpmem + (size_t)b * L * DH;
  const unsigned char* mb = mask ? mask + (size_t)b * L : nullptr;
  const float* attnb = attn + (size_t)b * steps * L;
  const float* cumb = cum + (size_t)b * steps * L;
  const float* dattnb = dattn ? dattn + (size_t)b * steps * L : nullptr;
  __syncthreads();
  for (int t = steps - 1; t >= 0; --t) {
    const size_t row = (size_t)b * steps + t;
    // A. the conv's inputs of this step, the total context gradient, the query
    for (int l = tid; l < L; l += DT) {
      s_wp[DP + l] = t > 0 ? attnb[(size_t)(t - 1) * L + l] : 0.f;
      s_wc[DP + l] = cumb[(size_t)t * L + l];
    }
    if (tid < DH) {
      const float x = dhc[row * (2 * DH) + DH + tid] + s_dctxc[tid];
      s_dctxt[tid] = x;
      dctx_out[row * DH + tid] = x;
      s_q[tid] = qv[row * DH + tid];
    }
    __syncthreads();
    // B. dw[l]
    {
      const float c0 = s_dctxt[d0], c1 = s_dctxt[d1];
      for (int l = wave; l < L; l += DT / 64) {
        const float p = wave_sum(fmaf(c0, memb[(size_t)l * DH + d0], c1 * memb[(size_t)l * DH + d1]));
        if (lane == 0) {
          s_de[l] = (((dattnb ? dattnb[(size_t)t * L + l] : 0.f) + p) + s_dwp[DP + l]) + s_dcum[DP + l];
          s_dwp[DP + l] = 0.f;  // consumed: the tiles below collect the gradient of w_{t-1} here
        }
      }
    }
    __syncthreads();
    // C. softmax backward; masked frames have w = 0 and get exactly 0
    {
      float sd = 0.f;
      for (int l = tid; l < L; l += DT) sd = fmaf(attnb[(size_t)t * L + l], s_de[l], sd);
      sd = block_reduce<false>(sd, s_red);
      for (int l = tid; l < L; l += DT) s_de[l] = attnb[(size_t)t * L + l] * (s_de[l] - sd);
    }
    __syncthreads();
    float dq0 = 0.f, dq1 = 0.f;
    // D. per tile of DTL frames
    for (int l0 = 0; l0 < L; l0 += DTL) {
      loc_conv_tile(s_wp, s_wc, s_wloc, l0, L, s_conv);
      __syncthreads();
      const int lend = min(DTL, L - l0);
      for (int li = wave; li < lend; li += DT / 64) {
        const int l = l0 + li;
        float mine = 0.f;
        if (!(mb && mb[l])) {  // (uniform over the wave)
          const float de = s_de[l];
          const float* cv = s_conv + li * (DF + 1);
          float a0 = 0.f, a1 = 0.f;
#pragma unroll
          for (int f = 0; f < DF; ++f) {
            const float x = cv[f];
            a0 = fmaf(wd0[f], x, a0);
            a1 = fmaf(wd1[f], x, a1);
          }
          const float th0 = tanhf((s_q[d0] + a0) + pmb[(size_t)l * DH + d0]);
          const float th1 = tanhf((s_q[d1] + a1) + pmb[(size_t)l * DH + d1]);
          const float g0 = de * v0 * (1.0f - th0 * th0), g1 = de * v1 * (1.0f - th1 * th1);
          dv0 = fmaf(de, th0, dv0);
          dv1 = fmaf(de, th1, dv1);
          dq0 += g0;
          dq1 += g1;
          dpm[(size_t)l * DH + d0] += g0;  // (this thread alone touches the element, step after step)
          dpm[(size_t)l * DH + d1] += g1;
#pragma unroll
          for (int f = 0; f < DF; ++f) {
            const float x = cv[f];
            dwd0[f] = fmaf(g0, x, dwd0[f]);
            dwd1[f] = fmaf(g1, x, dwd1[f]);
            const float r = wave_sum(fmaf(g0, wd0[f], g1 * wd1[f]));
            if (lane == f) mine = r;
          }
        }
        if (lane < DF) s_dconv[li * (DF + 1) + lane] = mine;
      }
      __syncthreads();
      // d(conv weight): thread (filter, 8 taps of one channel) over the tile's frames in order
      {
        const float* arr = (cc ? s_wc : s_wp) + l0 + ck0;  // arr[li + j] = frame l0 + li + (ck0 + j) - DP
        for (int li = 0; li < lend; ++li) {
          const float x = s_dconv[li * (DF + 1) + cf];
#pragma unroll
          for (int j = 0; j < 8; ++j) dloc[j] = fmaf(x, arr[li + j], dloc[j]);
        }
      }
      // the transposed conv: thread (filter, strip of BSTRIP frames j) gathers dconv[j - k + DP] over the taps, the
      // filters are then summed by a butterfly over the 32 lanes that share the strip
      {
        const int jb = cgrp * BSTRIP;  // frame j = l0 - DP + jb + p
        float win[BSTRIP + DK - 1];
#pragma unroll
        for (int q = 0; q < BSTRIP + DK - 1; ++q) {
          const int li = jb - (DK - 1) + q;
          win[q] = (li >= 0 && li < lend) ? s_dconv[li * (DF + 1) + cf] : 0.f;
        }
        float acc[2][BSTRIP] = {};
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int k = 0; k < DK; ++k) {
            const float w = s_wloc[(c * DK + k) * DF + cf];
#pragma unroll
            for (int p = 0; p < BSTRIP; ++p) acc[c][p] = fmaf(w, win[p - k + DK - 1], acc[c][p]);
          }
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int p = 0; p < BSTRIP; ++p) {
            float r = acc[c][p];
#pragma unroll
            for (int s = 16; s >= 1; s >>= 1) r += __shfl_xor(r, s);
            const int j = l0 - DP + jb + p;
            if (cf == 0 && j >= 0 && j < L) (c ? s_dcum : s_dwp)[DP + j] += r;
          }
      }
      __syncthreads();
    }
    // E. dq: the waves' shares in wave order
    s_wv[wave * DH + d0] = dq0;
    s_wv[wave * DH + d1] = dq1;
    __syncthreads();
    if (tid < DH) {
      float x = s_wv[tid];
      for (int w = 1; w < DT / 64; ++w) x += s_wv[w * DH + tid];
      s_dq[tid] = x;
      dq_out[row * DH + tid] = x;
    }
    __syncthreads();
    // F. W_query^T dq: 4 partial sums of 32 rows each, added in part order
    {
      const int k = tid & (DH - 1), g = tid >> 7;
      float a = 0.f;
#pragma unroll 8
      for (int d = g * 32; d < g * 32 + 32; ++d) a = fmaf(wq[d * DH + k], s_dq[d], a);
      s_part[g * DH + k] = a;
    }
    __syncthreads();
    // G. the LSTMCell backward (torch's gate order i, f, g, o)
    if (tid < DH) {
      const float dh = (dhc[row * (2 * DH) + tid] + s_dhc[tid]) +
                       (((s_part[tid] + s_part[DH + tid]) + s_part[2 * DH + tid]) + s_part[3 * DH + tid]);
      const float* g = gates + row * (4 * DH);
      const float ig = g[tid], fg = g[DH + tid], gg = g[2 * DH + tid], og = g[3 * DH + tid];
      const float c = cellv[row * DH + tid], cprev = t > 0 ? cellv[(row - 1) * DH + tid] : 0.f;
      const float tc = tanhf(c);
      const float dc = dcell + dh * og * (1.0f - tc * tc);
      const float zi = dc * gg * ig * (1.0f - ig), zf = dc * cprev * fg * (1.0f - fg);
      const float zg = dc * ig * (1.0f - gg * gg), zo = dh * tc * og * (1.0f - og);
      dcell = dc * fg;
      float* o = dgates + row * (4 * DH);
      s_dg[tid] = o[tid] = zi;
      s_dg[DH + tid] = o[DH + tid] = zf;
      s_dg[2 * DH + tid] = o[2 * DH + tid] = zg;
      s_dg[3 * DH + tid] = o[3 * DH + tid] = zo;
    }
    __syncthreads();
    // H. the gradients step t - 1 receives through the gates: W_ih[:, E:]^T dgates (context) and W_hh^T dgates (h);
    // two partial sums of 256 gate rows each
    {
      const int o = tid & (2 * DH - 1), g = tid >> 8;
      const float* W = o < DH ? wih_ctx + o : whh + (o - DH);
      const int ld = o < DH ? ld_ih : DH;
      float a = 0.f;
#pragma unroll 8
      for (int j = g * 2 * DH; j < (g + 1) * 2 * DH; ++j) a = fmaf(W[(size_t)j * ld], s_dg[j], a);
      s_part[g * 2 * DH + o] = a;
    }
    __syncthreads();
    if (tid < DH) {
      s_dctxc[tid] = s_part[tid] + s_part[2 * DH + tid];
      s_dhc[tid] = s_part[DH + tid] + s_part[3 * DH + tid];
    }
    __syncthreads();
  }
  // this utterance's shares of dv, d(dense weight), d(conv weight): the waves in wave order
  s_wv[wave * DH + d0] = dv0;
  s_wv[wave * DH + d1] = dv1;
  __syncthreads();
  if (tid < DH) {
    float x = s_wv[tid];
    for (int w = 1; w < DT / 64; ++w) x += s_wv[w * DH + tid];
    pv[(size_t)b * DH + tid] = x;
  }
  for (int w = 0; w < DT / 64; ++w) {  // s_conv as [DH][DF]
    if (wave == w) {
#pragma unroll
      for (int f = 0; f < DF; ++f) {
        s_conv[d0 * DF + f] = w ? s_conv[d0 * DF + f] + dwd0[f] : dwd0[f];
        s_conv[d1 * DF + f] = w ? s_conv[d1 * DF + f] + dwd1[f] : dwd1[f];
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < DH * DF; i += DT) pwd[(size_t)b * DH * DF + i] = s_conv[i];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (ck0 + j < DK) ploc[(size_t)b * kLocTaps + (cc * DK + ck0 + j) * DF + cf] = dloc[j];
}

// ------------------------------------------------------------------------------------------------ losses
// loss_s2s (train.py:301-304), one workgroup per utterance: part[b] = mean_{p < len} (logsumexp(z[p]) - z[p][tok[p]])
// in fp64; with dz the gradient g / B / len (softmax - onehot), rows p >= len zero.
__global__ void __launch_bounds__(NT) k_s2s_loss(const float* __restrict__ z, long long zs_b, long long zs_t, int B,
                                                 int T, int K, const long long* __restrict__ tok, long long tok_b,
                                                 const int* __restrict__ lengths, double* __restrict__ part,
                                                 float* __restrict__ dz, const float* __restrict__ gp) {
  __shared__ double s_w[NT / 64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int len = lengths ? lengths[b] : T;
  len = len < 0 ? 0 : (len > T ? T : len);
  const float* zb = z + (size_t)b * zs_b;
  const double gs = dz ? (double)(gp ? *gp : 0.f) / B / (double)len : 0.0;
  double acc = 0.0;
  for (int p = w; p < T; p += NT / 64) {
    float* dr = dz ? dz + ((size_t)b * T + p) * K : nullptr;
    if (p >= len) {
      if (dr)
        for (int k = lane; k < K; k += 64) dr[k] = 0.f;
      continue;
    }
    const float* zr = zb + (size_t)p * zs_t;
    float m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, zr[k]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s));
    double se = 0.0;
    for (int k = lane; k < K; k += 64) se += exp((double)zr[k] - (double)m);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) se += __shfl_xor(se, s);
    long long id = tok[(size_t)b * tok_b + p];
    id = id < 0 ? 0 : (id >= K ? K - 1 : id);  // (the host refuses indices outside the table)
    if (lane == 0) acc += ((double)m + log(se)) - (double)zr[id];
    if (dr)
      for (int k = lane; k < K; k += 64)
        dr[k] = (float)(gs * (exp((double)zr[k] - (double)m) / se - (k == id ? 1.0 : 0.0)));
  }
  if (lane == 0) s_w[w] = acc;  // wave w holds the rows p = w, w + 4, ..: a fixed split
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = s_w[0];
    for (int i = 1; i < NT / 64; ++i) a += s_w[i];
    part[b] = a / (double)len;  // (0 / 0 = NaN for an empty utterance, as F.cross_entropy over no rows)
  }
}

__global__ void k_s2s_loss_final(const double* __restrict__ part, int B, double* __restrict__ loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a = 0.0;
  for (int b = 0; b < B; ++b) a += part[b];
  loss[0] = a / B;
}

// loss_mono = 10 mean |a - m| (train.py:306).  Every workgroup writes its slice of da = g 10 / n sign(a - m); workgroup
// 0 also forms the whole sum in fp64 (a fixed split over its threads, then the fixed-order workgroup sum).
constexpr int MT = 1024;
__global__ void __launch_bounds__(MT) k_mono_loss(const float* __restrict__ a, const float* __restrict__ m, long long n,
                                                  double* __restrict__ loss, float* __restrict__ da,
                                                  const float* __restrict__ gp) {
  __shared__ double s_w[MT / 64];
  if (da) {
    const float gs = (float)((double)(gp ? *gp : 0.f) * 10.0 / (double)n);
    for (long long i = (long long)blockIdx.x * MT + threadIdx.x; i < n; i += (long long)gridDim.x * MT) {
      const float d = a[i] - m[i];
      da[i] = d > 0.f ? gs : (d < 0.f ? -gs : 0.f);  // torch's l1 backward: sign, 0 at 0
    }
  }
  if (blockIdx.x != 0) return;
  double acc = 0.0;
  for (long long i = threadIdx.x; i < n; i += MT) acc += fabs((double)a[i] - (double)m[i]);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = s_w[0];
    for (int i = 1; i < MT / 64; ++i) t += s_w[i];
    loss[0] = 10.0 * t / (double)n;
  }
}

// the 14 parameters of ASRS2S in named_parameters() order
enum {
  P_EMB, P_PNS_W, P_PNS_B, P_QUERY, P_MEMORY, P_V, P_LOC, P_DENSE, P_WIH, P_WHH, P_BIH, P_BHH, P_PH_W, P_PH_B, P_N
};

float* at(void* ws, long long off) { return reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + off); }

#define RUN(x) ST_CHECK(x)
#define LAUNCHED() ST_CHECK_HIP(hipGetLastError())

}  // namespace

extern "C" long long stts_s2s_save_bytes(int B, int L, int Tt) {
  const Dims d{B, L, Tt, 4, 1};
  if (!d.ok() || L > ST_ALIGNER_MAX_L) return ST_EINVAL;
  return SaveLayout(d).bytes;
}

extern "C" long long stts_s2s_fwd_train_workspace_bytes(int B, int L, int Tt, int n_token, int E) {
  const Dims d{B, L, Tt, n_token, E};
  if (!d.ok() || L > ST_ALIGNER_MAX_L) return ST_EINVAL;
  return FwdLayout(d).bytes + SaveLayout(d).bytes;  // (room for the state when the caller keeps none)
}

extern "C" int stts_s2s_fwd_train(const float* memory, const unsigned char* memory_mask, const int* tokens,
                                  const unsigned char* unk_mask, const float* const* params, int B, int L, int Tt,
                                  int n_token, int E, const float* drop_scale, float* hidden, float* logit, float* attn,
                                  void* save, void* ws, long long ws_bytes, void* stream) {
  if (!memory || !tokens || !params || !hidden || !logit || !attn) return ST_EINVAL;
  const Dims d{B, L, Tt, n_token, E};
  if (!d.ok() || L > ST_ALIGNER_MAX_L) return ST_EINVAL;
  for (int i = 0; i < P_N; ++i)
    if (!params[i]) return ST_EPARAMS;
  const FwdLayout w(d);
  const SaveLayout sv(d);
  if (!ws || ws_bytes < w.bytes + sv.bytes) return ST_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int D = DH, steps = Tt + 1;
  const long long rows = d.rows(), srows = d.srows();
  void* st = save ? save : reinterpret_cast<char*>(ws) + w.bytes;
  float *wc = at(ws, w.wc_t), *wqt = at(ws, w.wq_t), *wlt = at(ws, w.wloc_t), *EMB = at(ws, w.emb), *GIN = at(ws, w.gin);
  float *HC = at(st, sv.hc), *PM = at(st, sv.pm);
  RUN(st_transpose(params[P_WIH], 4 * D, D, E + D, E, wc, s));  // W_ih[:, E:] (the context part), k-major
  RUN(st_transpose(params[P_WHH], 4 * D, D, D, 0, wc + (size_t)D * 4 * D, s));
  RUN(st_transpose(params[P_QUERY], D, D, D, 0, wqt, s));
  RUN(st_transpose(params[P_LOC], DF, 2 * DK, 2 * DK, 0, wlt, s));
  RUN(st_s2s_embed(tokens, unk_mask, B, Tt, E, n_token, params[P_EMB], EMB, s));
  RUN(st_gemm_nt(EMB, srows, E, E, params[P_WIH], 4 * D, E + D, params[P_BIH], params[P_BHH], 0, GIN, 4 * D, s));
  RUN(st_gemm_nt(memory, rows, D, D, params[P_MEMORY], D, D, nullptr, nullptr, 0, PM, D, s));
  if (save)
    RUN(st_s2s_decode_train(GIN, wc, wqt, wlt, params[P_DENSE], params[P_V], memory, PM, memory_mask, B, L, steps, attn,
                            HC, at(st, sv.gates), at(st, sv.cell), at(st, sv.cum), s));
  else
    RUN(st_s2s_decode(GIN, wc, wqt, wlt, params[P_DENSE], params[P_V], memory, PM, memory_mask, B, L, steps, attn, HC,
                      s));
  RUN(st_gemm_nt(HC, srows, 2 * D, 2 * D, params[P_PH_W], D, 2 * D, params[P_PH_B], nullptr, 2, hidden, D, s));
  const float* hd = hidden;
  if (drop_scale) {  // F.dropout(hidden, 0.5) (models.py:174): the caller's keep mask / (1 - p)
    hipLaunchKernelGGL(k_mul, dim3(grid_of(srows * D)), dim3(NT), 0, s, hidden, drop_scale, srows * D, at(ws, w.hd));
    LAUNCHED();
    hd = at(ws, w.hd);
  }
  RUN(st_gemm_nt(hd, srows, D, D, params[P_PNS_W], n_token, D, params[P_PNS_B], nullptr, 0, logit, n_token, s));
  return 0;
}

extern "C" long long stts_s2s_bwd_workspace_bytes(int B, int L, int Tt, int n_token, int E) {
  const Dims d{B, L, Tt, n_token, E};
  if (!d.ok() || L > ST_S2S_BWD_MAX_L) return ST_EINVAL;
  return BwdLayout(d).bytes;
}

extern "C" int stts_s2s_bwd(const float* memory, const unsigned char* memory_mask, const int* tokens,
                            const unsigned char* unk_mask, const float* const* params, int B, int L, int Tt,
                            int n_token, int E, const float* drop_scale, const float* hidden, const float* attn,
                            const void* save, const float* dhidden, const float* dlogit, const float* dattn,
                            float* dmemory, float* const* grads, void* ws, long long ws_bytes, void* stream) {
  if (!memory || !tokens || !params || !hidden || !attn || !save || !grads) return ST_EINVAL;
  const Dims d{B, L, Tt, n_token, E};
  if (!d.ok() || L > ST_S2S_BWD_MAX_L) return ST_EINVAL;
  for (int i = 0; i < P_N; ++i)
    if (!params[i]) return ST_EPARAMS;
  const BwdLayout w(d);
  const SaveLayout sv(d);
  if (!ws || ws_bytes < w.bytes) return ST_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int D = DH, steps = Tt + 1, S = (int)d.srows(), R = (int)d.rows();
  const long long srows = d.srows(), rows = d.rows();
  const float* HC = at(const_cast<void*>(save), sv.hc);
  const float* PM = at(const_cast<void*>(save), sv.pm);
  float *TA = at(ws, w.ta), *TB = at(ws, w.tb), *TW = at(ws, w.tw);
  float *DPRE = at(ws, w.dpre), *DHC = at(ws, w.dhc), *DG = at(ws, w.dgates), *DQ = at(ws, w.dq), *DCTX = at(ws, w.dctx);
  float *DPM = at(ws, w.dpmem), *Q = at(ws, w.q);
  // ---- before the loop: logit = project_to_n_symbols(hidden * scale), hidden = tanh(project_to_hidden(hc))
  const float* dhd = nullptr;
  if (dlogit) {
    const float* hd = hidden;
    if (drop_scale) {
      hipLaunchKernelGGL(k_mul, dim3(grid_of(srows * D)), dim3(NT), 0, s, hidden, drop_scale, srows * D, at(ws, w.hd));
      LAUNCHED();
      hd = at(ws, w.hd);
    }
    if (grads[P_PNS_W]) {  // dW[n][k] = sum_r dlogit[r][n] hd[r][k]
      RUN(st_transpose(dlogit, S, n_token, n_token, 0, TA, s));
      RUN(st_transpose(hd, S, D, D, 0, TB, s));
      RUN(st_gemm_nt(TA, n_token, S, S, TB, D, S, nullptr, nullptr, 0, grads[P_PNS_W], D, s));
    }
    if (grads[P_PNS_B]) {
      hipLaunchKernelGGL(k_colsum, dim3((n_token + NT - 1) / NT), dim3(NT), 0, s, dlogit, srows, n_token,
                         grads[P_PNS_B], (float*)nullptr);
      LAUNCHED();
    }
    RUN(st_transpose(params[P_PNS_W], n_token, D, D, 0, TW, s));  // [D][n_token]
    RUN(st_gemm_nt(dlogit, srows, n_token, n_token, TW, D, n_token, nullptr, nullptr, 0, at(ws, w.hd), D, s));
    dhd = at(ws, w.hd);  // (hidden * scale was consumed above)
  } else {
    if (grads[P_PNS_W]) ST_CHECK_HIP(hipMemsetAsync(grads[P_PNS_W], 0, sizeof(float) * n_token * D, s));
    if (grads[P_PNS_B]) ST_CHECK_HIP(hipMemsetAsync(grads[P_PNS_B], 0, sizeof(float) * n_token, s));
  }
  hipLaunchKernelGGL(k_hidden_bwd, dim3(grid_of(srows * D)), dim3(NT), 0, s, dhidden, dhd, drop_scale, hidden, srows * D,
                     DPRE);
  LAUNCHED();
  RUN(st_transpose(DPRE, S, D, D, 0, TA, s));
  if (grads[P_PH_W]) {
    RUN(st_transpose(HC, S, 2 * D, 2 * D, 0, TB, s));
    RUN(st_gemm_nt(TA, D, S, S, TB, 2 * D, S, nullptr, nullptr, 0, grads[P_PH_W], 2 * D, s));
  }
  if (grads[P_PH_B]) {
    hipLaunchKernelGGL(k_colsum, dim3(1), dim3(NT), 0, s, DPRE, srows, D, grads[P_PH_B], (float*)nullptr);
    LAUNCHED();
  }
  RUN(st_transpose(params[P_PH_W], D, 2 * D, 2 * D, 0, TW, s));  // [2D][D]
  RUN(st_gemm_nt(DPRE, srows, D, D, TW, 2 * D, D, nullptr, nullptr, 0, DHC, 2 * D, s));
  RUN(st_gemm_nt(HC, srows, D, 2 * D, params[P_QUERY], D, D, nullptr, nullptr, 0, Q, D, s));  // the queries again
  // ---- the recurrence
  ST_CHECK_HIP(hipMemsetAsync(DPM, 0, sizeof(float) * rows * D, s));
  {
    static std::mutex mu;
    static bool raised = false;
    std::lock_guard<std::mutex> lk(mu);
    if (!raised) {
      ST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_s2s_bwd),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)bwd_dyn_lds(ST_S2S_BWD_MAX_L)));
      raised = true;
    }
  }
  hipLaunchKernelGGL(k_s2s_bwd, dim3((unsigned)B), dim3(DT), bwd_dyn_lds(L), s, memory, PM, memory_mask, attn,
                     at(const_cast<void*>(save), sv.cum), at(const_cast<void*>(save), sv.gates),
                     at(const_cast<void*>(save), sv.cell), Q, DHC, dattn, params[P_QUERY], params[P_WIH] + E, E + D,
                     params[P_WHH], params[P_LOC], params[P_DENSE], params[P_V], L, steps, DG, DQ, DCTX, DPM,
                     at(ws, w.pv), at(ws, w.pwd), at(ws, w.ploc));
  LAUNCHED();
  // ---- after the loop
  if (grads[P_V]) {
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(NT), 0, s, at(ws, w.pv), B, D, 0, grads[P_V]);
    LAUNCHED();
  }
  if (grads[P_DENSE]) {
    hipLaunchKernelGGL(k_sum_partials, dim3(D * DF / NT), dim3(NT), 0, s, at(ws, w.pwd), B, D * DF, 0, grads[P_DENSE]);
    LAUNCHED();
  }
  if (grads[P_LOC]) {
    hipLaunchKernelGGL(k_sum_partials, dim3((kLocTaps + NT - 1) / NT), dim3(NT), 0, s, at(ws, w.ploc), B, kLocTaps, 1,
                       grads[P_LOC]);
    LAUNCHED();
  }
  if (grads[P_BIH] || grads[P_BHH]) {
    hipLaunchKernelGGL(k_colsum, dim3(4 * D / NT), dim3(NT), 0, s, DG, srows, 4 * D, grads[P_BIH], grads[P_BHH]);
    LAUNCHED();
  }
  const bool need_emb = grads[P_EMB] || grads[P_WIH];
  float* EMB = at(ws, w.emb);
  if (need_emb) RUN(st_s2s_embed(tokens, unk_mask, B, Tt, E, n_token, params[P_EMB], EMB, s));
  if (grads[P_WIH] || grads[P_WHH] || grads[P_QUERY]) {
    hipLaunchKernelGGL(k_lstm_inputs, dim3(grid_of(srows * (E + 2 * D))), dim3(NT), 0, s, EMB, HC, B, steps, E,
                       at(ws, w.xh), at(ws, w.hprev));
    LAUNCHED();
    RUN(st_transpose(DG, S, 4 * D, 4 * D, 0, TA, s));
    if (grads[P_WIH]) {
      RUN(st_transpose(at(ws, w.xh), S, E + D, E + D, 0, TB, s));
      RUN(st_gemm_nt(TA, 4 * D, S, S, TB, E + D, S, nullptr, nullptr, 0, grads[P_WIH], E + D, s));
    }
    if (grads[P_WHH]) {
      RUN(st_transpose(at(ws, w.hprev), S, D, D, 0, TB, s));
      RUN(st_gemm_nt(TA, 4 * D, S, S, TB, D, S, nullptr, nullptr, 0, grads[P_WHH], D, s));
    }
    if (grads[P_QUERY]) {  // q = W_query h_t
      RUN(st_transpose(DQ, S, D, D, 0, TA, s));
      RUN(st_transpose(HC, S, D, 2 * D, 0, TB, s));
      RUN(st_gemm_nt(TA, D, S, S, TB, D, S, nullptr, nullptr, 0, grads[P_QUERY], D, s));
    }
  }
  if (grads[P_EMB]) {  // rows of dgates W_ih[:, :E], scattered by token in row order
    RUN(st_transpose(params[P_WIH], 4 * D, E, E + D, 0, TW, s));  // [E][4D]
    RUN(st_gemm_nt(DG, srows, 4 * D, 4 * D, TW, E, 4 * D, nullptr, nullptr, 0, at(ws, w.demb), E, s));
    long long* tok = reinterpret_cast<long long*>(at(ws, w.tok));
    hipLaunchKernelGGL(k_eff_tokens, dim3(grid_of(srows)), dim3(NT), 0, s, tokens, unk_mask, B, Tt, n_token, tok);
    LAUNCHED();
    RUN(stts_embedding_bwd(tok, B, steps, nullptr, at(ws, w.demb), (long long)steps * E, E, n_token, E, grads[P_EMB],
                           stream));
  }
  if (grads[P_MEMORY]) {  // processed memory = memory W_memory^T
    RUN(st_transpose(DPM, R, D, D, 0, TA, s));
    RUN(st_transpose(memory, R, D, D, 0, TB, s));
    RUN(st_gemm_nt(TA, D, R, R, TB, D, R, nullptr, nullptr, 0, grads[P_MEMORY], D, s));
  }
  if (dmemory) {
    RUN(st_transpose(params[P_MEMORY], D, D, D, 0, TW, s));
    RUN(st_gemm_nt(DPM, rows, D, D, TW, D, D, nullptr, nullptr, 0, dmemory, D, s));
    hipLaunchKernelGGL(k_attn_ctx_bwd, dim3(grid_of(rows * D)), dim3(NT), 0, s, attn, DCTX, B, L, steps, dmemory);
    LAUNCHED();
  }
  return 0;
}

extern "C" long long stts_s2s_loss_workspace_bytes(int B) { return B < 0 ? ST_EINVAL : 8LL * (B > 0 ? B : 1); }

extern "C" int stts_s2s_loss(const float* logits, long long ls_b, long long ls_t, int B, int T, int K,
                             const long long* tokens, long long tok_b, const int* lengths, double* loss, float* dlogits,
                             const float* g, void* ws, long long ws_bytes, void* stream) {
  if (B <= 0 || T <= 0 || K <= 0 || !logits || !tokens || !loss) return ST_EINVAL;
  if (!ws || ws_bytes < stts_s2s_loss_workspace_bytes(B)) return ST_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(k_s2s_loss, dim3((unsigned)B), dim3(NT), 0, s, logits, ls_b, ls_t, B, T, K, tokens, tok_b, lengths,
                     part, dlogits, g);
  LAUNCHED();
  hipLaunchKernelGGL(k_s2s_loss_final, dim3(1), dim3(64), 0, s, part, B, loss);
  return (int)hipGetLastError();
}

extern "C" int stts_mono_loss(const float* attn, const float* attn_mono, long long n, double* loss, float* dattn,
                              const float* g, void* stream) {
  if (!attn || !attn_mono || !loss || n <= 0) return ST_EINVAL;
  const long long gr = (n + MT - 1) / MT;
  hipLaunchKernelGGL(k_mono_loss, dim3((unsigned)(gr < 1024 ? gr : 1024)), dim3(MT), 0, (hipStream_t)stream, attn,
                     attn_mono, n, loss, dattn, g);
  return (int)hipGetLastError();
}
