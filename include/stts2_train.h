/*
 * stts2_train.h — training-step (BASELINE config 5) entry points of libstts2.so, beyond the layer
 * forward / backward pairs already in stts2.h (conv1d, ConvTranspose1d, AdaIN1d + activation, Linear,
 * weight norm, pool, LeakyReLU).
 *
 * The reference's fine-tune step (train.py:267-327) runs, per batch: the decoder forward
 * (Modules/hifigan.py:446-475), DiscriminatorLoss (losses.py:170-190) + backward + AdamW on the MPD /
 * MSD (Modules/discriminators.py), then MultiResolutionSTFTLoss (losses.py:58-94) + GeneratorLoss
 * (:149-168) + backward + AdamW on the decoder (optimizers.py:65-73).  Everything below is one piece of
 * that autograd graph that stts2.h does not already cover; stts2_mi355x/training.py, losses.py and
 * optim.py string them together as torch.autograd.Functions.
 *
 * Conventions as stts2.h: DEVICE pointers to contiguous fp32 data, sizes as ints, `stream` a
 * hipStream_t (0 = default), caller-owned memory and workspaces, asynchronous, 0 = ok, >0 hipError_t,
 * <0 STTS_E*.  Every reduction is a fixed-order sum (fp64 partials, added in order): results are
 * bitwise reproducible run to run.  `go` arguments are DEVICE pointers to the autograd upstream
 * gradient of a scalar loss (read by the kernel, so no host synchronisation is needed).
 */
#ifndef STTS2_TRAIN_H
#define STTS2_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

/* Snake with a learned per-channel alpha, the Generator's stage activations (hifigan.py:329, :343):
 * y = x + (1 / alpha_c) sin^2(alpha_c x) on frames x, y, dy, dx [B][L][C], alpha [C].  Backward: dx
 * and dalpha [C] (each nullable); workspace >= stts_snake_workspace_bytes(B, L, C). */
long long stts_snake_workspace_bytes(int B, int L, int C);
int stts_snake_fwd(const float* x, const float* alpha, int B, int L, int C, float* y, void* stream);
int stts_snake_bwd(const float* x, const float* alpha, const float* dy, int B, int L, int C, float* dx,
                   float* dalpha, void* ws, long long ws_bytes, void* stream);

/* tanh over n values (hifigan.py:345 after conv_post) and its backward from the output. */
int stts_tanh_fwd(const float* x, long long n, float* y, void* stream);
int stts_tanh_bwd(const float* y, const float* dy, long long n, float* dx, void* stream);

/* y = (xs[0] + xs[1] + ... + xs[k-1]) / div over n values, added left to right: `x + x_source`
 * (hifigan.py:334, div 1) and the resblock average `xs / num_kernels` (:337-342).  `xs` is a HOST array
 * of k <= 8 device pointers.  stts_div: y = x / div (the backward of the average). */
int stts_sum_div(const float* const* xs, int k, long long n, float div, float* y, void* stream);
int stts_div(const float* x, long long n, float div, float* y, void* stream);

/* SourceModuleHnNSF for training (hifigan.py:221-268): f0_curve [B][n] (the Decoder's F0_curve; the
 * Generator upsamples it x scale, :323) -> sw [B][n*scale][9] = the SineGen output sine_waves * uv + noise
 * (computed under no_grad in the reference, :262-263) and har [B][n*scale] = tanh(l_linear(sw)) (:264).
 * noise [B][n*scale][9] = the randn_like draw of :213, or NULL for the counter RNG keyed by
 * (seed, utt_offset + b, sample, harmonic) as stts_decoder_fwd.  Backward: dW [9] and db [1] of l_linear
 * from dhar (the only parameters with a gradient there).  Workspace >= stts_source_workspace_bytes(B, n). */
long long stts_source_workspace_bytes(int B, int n);
int stts_source_fwd(const float* f0_curve, const float* lw, const float* lb, const float* noise,
                    unsigned long long seed, long long utt_offset, int B, int n, int scale, float* sw, float* har,
                    void* ws, long long ws_bytes, void* stream);
/* The same with the seed read from DEVICE memory (seed_dev, or noise given): a hipGraph capture of the training step
 * replays with the seed the caller writes there before each replay (round 5). */
int stts_source_fwd_seed_dev(const float* f0_curve, const float* lw, const float* lb, const float* noise,
                             const unsigned long long* seed_dev, long long utt_offset, int B, int n, int scale,
                             float* sw, float* har, void* ws, long long ws_bytes, void* stream);
int stts_source_bwd(const float* sw, const float* har, const float* dhar, int B, long long L, float* dW, float* db,
                    void* ws, long long ws_bytes, void* stream);

/* Decoder.forward's train-mode F0 / N smoothing (hifigan.py:447-455):
 * y = conv1d(x, ones(1, 1, k), padding k // 2) / k per row of x [B][n], k odd; and its backward. */
int stts_box_smooth_fwd(const float* x, int B, int n, int k, float* y, void* stream);
int stts_box_smooth_bwd(const float* dy, int B, int n, int k, float* dx, void* stream);

/* A (3, kw) Conv2d over (frames, bins) (SpecDiscriminator, discriminators.py:39-47) as a 1-D conv
 * along the bins over 3 C channels: x3[s][h][w][c * 3 + dh] = y[s][h + dh - 1][w][c] (0 outside
 * [0, H)), so the reference's [Cout][C][3][kw] weight is the [Cout][3C][kw] conv1d weight.  Backward:
 * dy[s][h][w][c] = sum_dh dx3[s][h - dh + 1][w][c * 3 + dh]. */
int stts_time_expand3(const float* y, int S, int H, int W, int C, float* x3, void* stream);
int stts_time_expand3_bwd(const float* dx3, int S, int H, int W, int C, float* dy, void* stream);

/* |torch.stft(x, n_fft, hop, win, hann(win), center, reflect, onesided)| (discriminators.py:11-27,
 * :53): wave [S][ld] (L > n_fft / 2 samples) -> mag [S][F][nb] (F = 1 + L / hop, nb = n_fft / 2 + 1:
 * the reference's [S, 1, F, nb] image) and spec [S][F][nb][2] (re, im, kept for the backward).
 * Backward: dwave [S][L] = the stft adjoint (per frame an inverse FFT in LDS, window, then a fixed-order
 * overlap-add gather that folds the reflect padding back) of dspec = dmag * spec / |spec|
 * (0 where |spec| = 0, as torch.abs).  n_fft a power of two <= 2048.
 * Workspace >= stts_stft_mag_workspace_bytes(S, L, n_fft, win, hop). */
long long stts_stft_mag_workspace_bytes(int S, long long L, int n_fft, int win, int hop);
int stts_stft_mag_fwd(const float* wave, int S, long long L, long long ld, int n_fft, int win, int hop, float* mag,
                      float* spec, void* stream);
int stts_stft_mag_bwd(const float* spec, const float* dmag, int S, long long L, int n_fft, int win, int hop,
                      float* dwave, void* ws, long long ws_bytes, void* stream);

/* MultiResolutionSTFTLoss backward (losses.py:24-94; stts_mrstft_loss is the forward): dx [B][L]
 * = go * d loss / d x for x the predicted signal (train.py:281 stft_loss(y_rec, wav)) and y the target.
 * Per resolution: log-mel of y, ||y_mag||_1, then per frame of x the FFT, mel, d|mag| = -sign(y - x) /
 * (n_res ||y_mag||_1), the log / filterbank / power adjoints and the inverse FFT; the frames are
 * overlap-added in fixed order.  The int arrays are HOST pointers.
 * Workspace >= stts_mrstft_bwd_workspace_bytes(B, L, n_ffts, hops, wins, n_res, n_mels). */
long long stts_mrstft_bwd_workspace_bytes(int B, long long L, const int* n_ffts, const int* hops, const int* wins,
                                          int n_res, int n_mels);
int stts_mrstft_loss_bwd(const float* x, const float* y, int B, long long L, long long ld, const int* n_ffts,
                         const int* hops, const int* wins, int n_res, int sample_rate, int n_mels, const float* go,
                         float* dx, void* ws, long long ws_bytes, void* stream);

/* GAN loss terms: the sums GeneratorLoss / DiscriminatorLoss form (losses.py:97-190).  A term reads
 * two equally laid out tensors a, b of n values (a = the real side, b = the generated side):
 *   STTS_GAN_FEATURE  2 mean|a - b|                    feature_loss (:97-103, fmap_r, fmap_g)
 *   STTS_GAN_GEN      mean((1 - b)^2)                  generator_loss (:120-128, b = D(y_hat))
 *   STTS_GAN_DISC     mean((1 - a)^2) + mean(b^2)      discriminator_loss (:106-117)
 *   STTS_GAN_TPRLS    tau - relu(tau - mean(((a - b) - m)^2 over a < b + m)),  m = median(a - b)
 *                     (the lower median, as torch.median), tau = 0.04: discriminator_TPRLS_loss(dr, dg)
 *                     with (a, b) = (dr, dg) and generator_TPRLS_loss(dr, dg) with (a, b) = (dg, dr)
 *                     (:131-147; the latter's loop swaps the names).
 * stts_gan_loss: loss (device, 1 double) = the sum of the terms in order; it also leaves per-term
 * results (median, selected count, mean) in the workspace for the backward.  stts_gan_loss_bwd (after
 * the forward, same terms and workspace): da[i] / db[i] (device, n values each, nullable) = go * the
 * term's gradient w.r.t. a / b (torch's: sign(0) = 0; the median's gradient shared evenly by the
 * elements equal to it; relu'(0) = 0).  `terms`, `da`, `db` are HOST arrays; n_terms <= 256.
 * Workspace >= stts_gan_workspace_bytes(n_terms). */
typedef struct {
  const float* a;
  const float* b;
  long long n;
  int kind;
} stts_gan_term;
#define STTS_GAN_FEATURE 0
#define STTS_GAN_GEN 1
#define STTS_GAN_DISC 2
#define STTS_GAN_TPRLS 3
long long stts_gan_workspace_bytes(int n_terms);
int stts_gan_loss(const stts_gan_term* terms, int n_terms, double* loss, void* ws, long long ws_bytes, void* stream);
int stts_gan_loss_bwd(const stts_gan_term* terms, float* const* da, float* const* db, int n_terms, const float* go,
                      const void* ws, long long ws_bytes, void* stream);

/* AdamW step (torch.optim.AdamW, single-tensor arithmetic order, amsgrad off), as build_optimizer makes it
 * (optimizers.py:65-73: betas (0.0, 0.99), eps 1e-9, weight_decay 1e-4): for every tensor
 *   p *= 1 - lr wd;  m = lerp(m, g, 1 - beta1);  v = v beta2 + (1 - beta2) g g;
 *   p += (-lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * with `step` the tensor's step count after the increment (1 on the first call).  `tensors` is a HOST
 * array; any number of tensors (one launch per 32).  The hyper-parameters are doubles (Python floats): the
 * scalars 1 - lr wd, 1 - beta1, 1 - beta2, the bias corrections and lr / bc1 are formed in double and rounded
 * to fp32 once, as torch forms them, so the update is bitwise torch's. */
typedef struct {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long long n;
} stts_adamw_tensor;
int stts_adamw_step(const stts_adamw_tensor* tensors, int n_tensors, double lr, double beta1, double beta2,
                    double eps, double weight_decay, long long step, void* stream);
/* Capturable form (round 5; torch's `capturable=True`): the step count lives in DEVICE memory, state[0] (fp64,
 * >= 8 doubles of state), advanced and turned into the step's scalars by a one-thread launch on the stream, so a
 * hipGraph replay of the call takes the next step's bias corrections without the host.  The scalars are formed in
 * device fp64 (pow: the device library's), so an update may differ from the host form in the last fp32 bit. */
int stts_adamw_step_dev(const stts_adamw_tensor* tensors, int n_tensors, double lr, double beta1, double beta2,
                        double eps, double weight_decay, double* state, void* stream);

/* ---- ProsodyPredictor.F0Ntrain under train.py's G step (train.py:265, 318, 323; models.py:448-461) */

/* Training forward of the bidirectional nn.LSTM(batch_first) layers under train.py's G step: ProsodyPredictor.shared
 * (models.py:449, full-length rows) and, with `lengths` (device int32 [B], NULL = every row has length T; ABI 5), the
 * packed-sequence LSTMs of TextEncoder (models.py:267-279), DurationEncoder (:510-518) and ProsodyPredictor.lstm
 * (:421-430): stts_bilstm_fwd's output y [B][T][2H] (rows t >= len zero; same params, same workspace size) plus
 * every step's cell state c_seq [2][B][T][H] for the backward. */
int stts_bilstm_fwd_train(const float* x, long long xs_b, long long xs_t, long long xs_c, int B, int T, int Cin,
                          const int* lengths, const float* const* params, int H, float* y, float* c_seq,
                          void* workspace, long long ws_bytes, void* stream);
/* Its backward (what autograd computes for nn.LSTM over a packed sequence): x frames [B][T][Cin] contiguous, the same
 * lengths, y and c_seq from the training forward, dy [B][T][2H] -> dx [B][T][Cin] (NULL: not computed; rows t >= len
 * zero) and grads[8] in torch's parameter order (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, then the
 * _reverse four; NULL entries skipped).  Deterministic (no atomics; the bias gradients summed over utterances in
 * order). */
long long stts_bilstm_bwd_workspace_bytes(int B, int T, int Cin, int H);
int stts_bilstm_bwd(const float* x, int B, int T, int Cin, const int* lengths, const float* const* params, int H,
                    const float* y, const float* c_seq, const float* dy, float* dx, float* const* grads,
                    void* workspace, long long ws_bytes, void* stream);

/* ---- The text / duration path under train.py's G step (train.py:217, 230-233, 286-299, 318, 323, 327; round 5) */

/* Backward of stts_row_norm (include/stts2.h: mode 0 LayerNorm(gamma, beta) + optional LeakyReLU(slope) <- models.py
 * :229-240, 246-249; mode 1 AdaLayerNorm with gb [b][2C] rows gb_sb apart <- :372-392, 503-507; mode 2 the copy of
 * the DurationEncoder's input concat <- :497-501), each with the row mask t >= lengths[b] and E concatenated style
 * columns: x, gamma, beta, gb_sb, eps, lrelu, slope, lengths as the forward; dy [b][t][C + E] (rows dys_b / dys_t
 * apart).  Writes (each nullable) dx [B][T][C] contiguous (masked rows 0), dgamma / dbeta [C] (mode 0),
 * dgb [B][2C] (mode 1: the gradient of the style projection fc(s), gamma half then beta half) and
 * dextra [B][E] = sum_{t < len} dy[b][t][C + e].  Parameter sums are fp64 in row order (deterministic); they need a
 * workspace >= stts_row_norm_bwd_workspace_bytes(B, T, C). */
long long stts_row_norm_bwd_workspace_bytes(int B, int T, int C);
int stts_row_norm_bwd(const float* x, long long xs_b, long long xs_t, long long xs_c, int B, int T, int C, int mode,
                      const float* gamma, const float* beta, long long gb_sb, float eps, int lrelu, float slope,
                      const int* lengths, const float* dy, long long dys_b, long long dys_t, int E, float* dx,
                      float* dgamma, float* dbeta, float* dgb, float* dextra, void* workspace, long long ws_bytes,
                      void* stream);
/* nn.Embedding backward with the masked_fill_ of TextEncoder.forward (models.py:257-260): dW [n_symbols][C] (C <=
 * 1024) = the sum of dy rows (b, t < len) per token id, in row order (deterministic); ids outside range add nothing. */
int stts_embedding_bwd(const long long* tokens, int B, int T, const int* lengths, const float* dy, long long dys_b,
                       long long dys_t, int n_symbols, int C, float* dW, void* stream);
/* The duration losses of train.py:286-299 over the predictor's logits d [B][T][K] (rows ls_b / ls_t apart), the
 * text lengths and d_gt [B][T] (s2s_attn_mono.sum(-1), integer-valued, rows dg_b apart): loss[0] = loss_dur =
 * mean_b l1(sum_k sigmoid(d[b][p]), d_gt[b][p]) over 1 <= p < len - 1, loss[1] = loss_ce = mean_b BCEWithLogits(d[b][:len],
 * trg) with trg[p][k] = k < d_gt[b][p] (fp64, utterance order).  With dlogits [B][T][K] (nullable) also the gradient of
 * g_dur loss_dur + g_ce loss_ce, the two upstream scalars read from DEVICE floats (nullable: 0), so the call needs no
 * host sync.  Workspace >= stts_dur_losses_workspace_bytes(B); T <= 4096. */
long long stts_dur_losses_workspace_bytes(int B);
int stts_dur_losses(const float* logits, long long ls_b, long long ls_t, int B, int T, int K, const int* lengths,
                    const float* d_gt, long long dg_b, double* loss, float* dlogits, const float* g_dur,
                    const float* g_ce, void* workspace, long long ws_bytes, void* stream);

/* nn.Dropout(p) in train mode (the predictor's AdainResBlk1d dropout, models.py:335, 358-367): y = x / (1 - p) where
 * a counter draw u(seed, i) >= p, else 0.  The backward is the same call on dy with the same seed (the mask is
 * redrawn, not stored).  The draws are not torch's (no implementation reproduces those); the seed comes from
 * torch's default generator in the Python layer, so torch.manual_seed governs them. */
int stts_dropout(const float* x, long long n, float p, unsigned long long seed, float* y, void* stream);
/* The same with the keep mask given: y[i] = mask[i] != 0 ? x[i] / (1 - p) : 0 (backward: the same call on dy).  Used
 * when a caller injects the masks (training.set_dropout_masks: train-mode parity against the reference run with the
 * same masks, tests/golden/make_golden_train_text.py). */
int stts_dropout_mask(const float* x, const float* mask, long long n, float p, float* y, void* stream);

/* ---- StyleEncoder under train.py's G step (train.py:258, 324; models.py:125-150), frames images [B][H][W][C] */
/* Row expansion for a k x k Conv2d with padding `pad` in H: xe[b][ho][w][c k + dh] = x[b][ho + dh - pad][w][c]
 * (0 outside), Ho = H + 2 pad - k + 1; the conv then runs as conv1d over W (stts_conv1d_fwd / _bwd) with the
 * reference weight [Cout][Cin][k][k] read as [Cout][Cin k][k].  _bwd: its adjoint (sums over dh in order). */
int stts_rowexp_fwd(const float* x, int B, int H, int W, int C, int k, int pad, float* xe, void* stream);
int stts_rowexp_bwd(const float* dxe, int B, int H, int W, int C, int k, int pad, float* dx, void* stream);
/* LearnedDownSample('half') = depthwise Conv2d(C, C, 3, stride 2, pad 1, groups C) (models.py:13-28):
 * y [B][(H-1)/2+1][(W-1)/2+1][C]; w [C][1][3][3]; bias [C] or NULL.  _bwd: dx, dw, db (each may be NULL), dw / db
 * as fixed-order split sums (workspace >= stts_dwconv2d_s2_workspace_bytes(C)). */
int stts_dwconv2d_s2_fwd(const float* x, const float* w, const float* bias, int B, int H, int W, int C, float* y,
                         void* stream);
long long stts_dwconv2d_s2_workspace_bytes(int C);
int stts_dwconv2d_s2_bwd(const float* x, const float* w, const float* dy, int B, int H, int W, int C, float* dx,
                         float* dw, float* db, void* ws, long long ws_bytes, void* stream);
/* DownSample('half') (models.py:48-62): W odd -> the last column repeated, then avg_pool2d(2):
 * y [B][H/2][(W+1)/2][C]; _bwd its adjoint. */
int stts_avgpool2_fwd(const float* x, int B, int H, int W, int C, float* y, void* stream);
int stts_avgpool2_bwd(const float* dy, int B, int H, int W, int C, float* dx, void* stream);
/* AdaptiveAvgPool2d(1) (models.py:139) over the P = H W positions: y [B][C]; _bwd: dx = dy / P. */
int stts_spatial_mean_fwd(const float* x, int B, int P, int C, float* y, void* stream);
int stts_spatial_mean_bwd(const float* dy, int B, int P, int C, float* dx, void* stream);

/* F.smooth_l1_loss(x, y) (beta 1, mean) <- train.py:269-270 (loss_F0_rec, loss_norm_rec): loss (device, 1 double)
 * from one workgroup's fixed-order fp64 sum; _bwd: dx = g dL/dx, dy = -dx (either may be NULL), g a device float. */
int stts_smooth_l1_loss(const float* x, const float* y, long long n, double* loss, void* stream);
int stts_smooth_l1_loss_bwd(const float* x, const float* y, long long n, const float* g, float* dx, float* dy,
                            void* stream);

/* ---- The Vocos decoder under the G step (Modules/vocos.py; csrc/vocos_train.hip).  Frames [B][L][C] fp32. */

/* ConvNeXtBlock.dwconv (vocos.py:45): depthwise Conv1d(C, C, K, padding K / 2, groups C) + bias,
 * y[b][t][c] = bias[c] + sum_k w[c][k] x[b][t + k - K / 2][c] (zero padded); w [C][K] (the reference's [C][1][K]),
 * bias [C] or NULL.  K odd, 1 <= K <= 11; 1 <= C <= 65536 (any count: no multiple of the 256-channel block is
 * needed); B <= 65535.  Outside these: STTS_EINVAL (the workspace query returns it as a negative size).
 * _bwd: dx = the same conv of dy with the taps reversed; dw [C][K] and db [C] as fp64 row-slice partial sums
 * folded in slice order (each of dx, dw, db may be NULL; x is read for dw, w for dx).
 * Workspace (dw / db only) >= stts_dwconv1d_bwd_workspace_bytes(B, L, C, K) = B S C (K + 1) doubles rounded up to
 * 256 bytes, S = min(64, ceil(L / 32)) row slices per utterance. */
int stts_dwconv1d_fwd(const float* x, const float* w, const float* bias, int B, int L, int C, int K, float* y,
                      void* stream);
long long stts_dwconv1d_bwd_workspace_bytes(int B, int L, int C, int K);
int stts_dwconv1d_bwd(const float* x, const float* w, const float* dy, int B, int L, int C, int K, float* dx, float* dw,
                      float* db, void* ws, long long ws_bytes, void* stream);

/* nn.GELU() (erf form, vocos.py:48) over n values: y = x Phi(x); _bwd from the saved pre-activation x:
 * dx = dy (Phi(x) + x phi(x)).  16-byte accesses when the pointers are 16-byte aligned; any n. */
int stts_gelu_fwd(const float* x, long long n, float* y, void* stream);
int stts_gelu_bwd(const float* x, const float* dy, long long n, float* dx, void* stream);

/* Layer scale + residual (vocos.py:64-68): y = r + gamma[c] x.  _bwd: dx = gamma dy and dgamma [C] = the column
 * sums of dy x (fp64 row-slice partials in slice order), each nullable; the residual's gradient is dy itself.
 * Workspace (dgamma only) >= stts_layer_scale_res_bwd_workspace_bytes(B, L, C) = S C doubles rounded up to 256
 * bytes, S = min(256, max(1, B L / 16)) row slices. */
int stts_layer_scale_res_fwd(const float* x, const float* r, const float* gamma, int B, int L, int C, float* y,
                             void* stream);
long long stts_layer_scale_res_bwd_workspace_bytes(int B, int L, int C);
int stts_layer_scale_res_bwd(const float* x, const float* gamma, const float* dy, int B, int L, int C, float* dx,
                             float* dgamma, void* ws, long long ws_bytes, void* stream);

/* ISTFTHead.forward after its Linear + ISTFT.forward, padding "same" (vocos.py:282-296, :190-232):
 * h [B][F][2 nb] (nb = n_fft / 2 + 1 log-magnitude channels, then nb phase channels), window [n_fft] ->
 * audio [B][F hop]:  mag = min(exp(h_k), 100), X_k = mag (cos p_k + i sin p_k), frame = irfft(X) window (the
 * imaginary parts of DC and Nyquist dropped), audio[j] = sum_t frame[t][j + pad - t hop] / env[j + pad] with env the
 * overlap-added squared window and pad = (n_fft - hop) / 2.  One workgroup per frame, a two-factor DFT in LDS:
 * n_fft even, n_fft = N1 N2 with both factors <= 64 (1200 = 30 x 40, 1024 = 32 x 32), 0 < hop < n_fft,
 * n_fft - hop even; otherwise STTS_EINVAL.
 * _bwd: dh [B][F][2 nb] from dy [B][F hop], the exact adjoint (dframe gathered from dy, one sample per element, a
 * forward DFT, then the chain through cos / sin / exp; the clip passes the gradient where exp(h_k) <= 100, as
 * torch.clip).  The window is a buffer: no gradient.
 * Workspace >= stts_istft_head_workspace_bytes(B, F, n_fft, hop) = B F n_fft floats rounded up to 256 bytes (the
 * frames of the forward; _bwd takes the same arguments and uses none of it, so NULL is accepted there). */
long long stts_istft_head_workspace_bytes(int B, int F, int n_fft, int hop);
int stts_istft_head_fwd(const float* h, const float* window, int B, int F, int n_fft, int hop, float* audio, void* ws,
                        long long ws_bytes, void* stream);
int stts_istft_head_bwd(const float* h, const float* window, const float* dy, int B, int F, int n_fft, int hop,
                        float* dh, void* ws, long long ws_bytes, void* stream);

/* ---- The iSTFTNet decoder under the G step (Modules/istftnet.py; csrc/istftnet_train.hip).  The CustomSTFT
 * geometries accepted here: n_fft even, 4 <= n_fft <= 64, 1 <= hop <= n_fft, B <= 65535 (the reference's 20 / 5
 * and the lite configurations; stts_model_create itself takes any positive pair for inference); otherwise
 * STTS_EINVAL before any launch.  None of these entries needs a workspace. */

/* CustomSTFT.transform (istftnet.py:207-243) of the harmonic source: wave [B][L], wr / wi = the module's
 * weight_forward_real / _imag buffers [n_fft / 2 + 1][n_fft] -> out [B][F][n_fft + 2], F = L / hop + 1: replicate
 * padding of n_fft / 2, mag = sqrt(re^2 + im^2 + 1e-14) in channels 0 .. n_fft / 2, then phase = atan2(im, re) with
 * (im == 0 and re < 0) -> pi.  The reference runs it under no_grad (:544-550): there is no backward. */
int stts_cstft_fwd(const float* wave, const float* wr, const float* wi, int B, int L, int n_fft, int hop, float* out,
                   void* stream);

/* The last stage's reflection_pad((1, 0)) fused with x + x_source (istftnet.py:558-561): x [B][L][C],
 * src [B][L + 1][C] -> y [B][L + 1][C], y[0] = x[1] + src[0], y[t] = x[t - 1] + src[t].  L >= 2, any C (16-byte
 * accesses when C % 4 == 0 and the pointers are 16-byte aligned).
 * _bwd: dx [B][L][C] from dy [B][L + 1][C], dx[t] = dy[t + 1] + (t == 1 ? dy[0] : 0); the gradient of src is dy
 * itself (not written). */
int stts_padl_add_fwd(const float* x, const float* src, int B, int L, int C, float* y, void* stream);
int stts_padl_add_bwd(const float* dy, int B, int L, int C, float* dx, void* stream);

/* Generator.forward's head (istftnet.py:571-573) + CustomSTFT.inverse (:246-293): post [B][F][2 nb] (conv_post's
 * output, nb = n_fft / 2 + 1), br / bi = the module's weight_backward_real / _imag buffers [nb][n_fft] ->
 * audio [B][(F - 1) hop]:  mag = exp(post_k), ph = sin(post_{nb + k}), re = mag cos ph, im = mag sin ph,
 * audio[j] = sum_t sum_k (re[t][k] br[k][p - t hop] - im[t][k] bi[k][p - t hop]) over 0 <= p - t hop < n_fft,
 * p = j + n_fft / 2 (the trim); no window-sum normalisation, no clip.  F >= 2.  A workgroup owns 64 hops of
 * samples: the transcendentals are evaluated once per (frame, bin) of its frames and halo in LDS.
 * _bwd: dpost [B][F][2 nb] from dy [B][(F - 1) hop], the exact adjoint with the forward values recomputed from
 * post (nothing else is saved): dre[t][k] = sum_n dy[t hop + n - n_fft / 2] br[k][n], dim = -sum_n dy[.] bi[k][n]
 * (dy zero outside its range), dmag = dre cos ph + dim sin ph, dph = mag (dim cos ph - dre sin ph),
 * dpost_k = dmag mag, dpost_{nb + k} = dph cos(post_{nb + k}).  The bases are buffers: no gradient. */
int stts_cistft_head_fwd(const float* post, const float* br, const float* bi, int B, int F, int n_fft, int hop,
                         float* audio, void* stream);
int stts_cistft_head_bwd(const float* post, const float* br, const float* bi, const float* dy, int B, int F, int n_fft,
                         int hop, float* dpost, void* stream);

/* ---- The text aligner's S2S decoder under train.py's step (Modules/ASR/models.py ASRS2S :118-176; train.py:206,
 * 301-306; csrc/aligner_train.hip).  The decoder is built for hidden_dim = 128 (decoder, attention and memory width),
 * 32 location filters of 63 taps.  `params` / `grads` are HOST arrays of 14 DEVICE pointers in ASRS2S's
 * named_parameters() order:
 *    0 embedding.weight [n_token][E]                      7 ...location_dense.linear_layer.weight [128][32]
 *    1 project_to_n_symbols.weight [n_token][128]         8 decoder_rnn.weight_ih [512][E + 128]
 *    2 project_to_n_symbols.bias [n_token]                9 decoder_rnn.weight_hh [512][128]
 *    3 attention_layer.query_layer...weight [128][128]   10 decoder_rnn.bias_ih [512]
 *    4 attention_layer.memory_layer...weight [128][128]  11 decoder_rnn.bias_hh [512]
 *    5 attention_layer.v...weight [1][128]               12 project_to_hidden.0.linear_layer.weight [128][256]
 *    6 ...location_conv.conv.weight [32][2][63]          13 project_to_hidden.0.linear_layer.bias [128]
 * Frame caps: L <= 4096 for the forward (STTS_ALIGNER_MAX_L) and L <= STTS_S2S_BWD_MAX_L for the backward, whose
 * workgroup keeps five [L] arrays (83 KB at the cap) next to 61 KB of tiles and state in the 160 KiB of a CU; above
 * the cap STTS_EINVAL, checked on the host (the workspace queries return it as a negative size).  1 <= E <= 1024,
 * 4 <= n_token <= 65536, Tt >= 1. */
#define STTS_S2S_BWD_MAX_L 4096

/* ASRS2S.forward (models.py:118-147) for training:
 *   memory       [B][L][128]    the CNN feature, frames (models.py:124)
 *   memory_mask  bytes [B][L], 1 = padded frame (the attention's masked_fill, layers.py), or NULL
 *   tokens       int32 [B][Tt]  text_input (:127); indices in [0, n_token): the caller checks
 *   unk_mask     bytes [B][Tt]  the random_mask draw of :126 (1 = replaced by index 3), or NULL
 *   drop_scale   [B][Tt + 1][128]  keep mask / (1 - p) of F.dropout(hidden, 0.5) (:174), or NULL (eval: no dropout)
 *   hidden       [B][Tt + 1][128], logit [B][Tt + 1][n_token], attn [B][Tt + 1][L]   the three outputs (:143-147)
 *   save         stts_s2s_save_bytes(B, L, Tt) bytes kept for stts_s2s_bwd: per step the four gate activations, the
 *                cell state, the cumulative weights before the step, [h; context], and the processed memory.  NULL:
 *                nothing is kept (the forward without grad), and the plain decoder kernel of stts_aligner_fwd runs.
 * Workspace >= stts_s2s_fwd_train_workspace_bytes(B, L, Tt, n_token, E). */
long long stts_s2s_save_bytes(int B, int L, int Tt);
long long stts_s2s_fwd_train_workspace_bytes(int B, int L, int Tt, int n_token, int E);
int stts_s2s_fwd_train(const float* memory, const unsigned char* memory_mask, const int* tokens,
                       const unsigned char* unk_mask, const float* const* params, int B, int L, int Tt, int n_token,
                       int E, const float* drop_scale, float* hidden, float* logit, float* attn, void* save, void* ws,
                       long long ws_bytes, void* stream);
/* Its backward: the same memory, masks, tokens, params and drop_scale; hidden, attn and save from the forward;
 * dhidden / dlogit / dattn = the upstream gradients of the three outputs (each nullable: zero).  Writes dmemory
 * [B][L][128] (nullable; exactly 0 at masked frames) and grads[14] (a NULL entry: not computed, the others
 * unchanged bit for bit).  One persistent workgroup per utterance walks the steps backwards; every weight gradient
 * is a fixed-order product over all rows after it, the embedding rows (SOS into row 1, unknown-masked tokens into
 * row 3) are scattered in row order: bitwise reproducible, and a row of dmemory does not depend on the batch.
 * Workspace >= stts_s2s_bwd_workspace_bytes(B, L, Tt, n_token, E). */
long long stts_s2s_bwd_workspace_bytes(int B, int L, int Tt, int n_token, int E);
int stts_s2s_bwd(const float* memory, const unsigned char* memory_mask, const int* tokens,
                 const unsigned char* unk_mask, const float* const* params, int B, int L, int Tt, int n_token, int E,
                 const float* drop_scale, const float* hidden, const float* attn, const void* save,
                 const float* dhidden, const float* dlogit, const float* dattn, float* dmemory, float* const* grads,
                 void* ws, long long ws_bytes, void* stream);

/* loss_s2s (train.py:301-304) over logits [B][T][K] (rows ls_b / ls_t apart), tokens int64 [B][..] (rows tok_b
 * apart) and the text lengths (device int32 [B], NULL = T): loss (device, 1 double) = mean_b cross_entropy(logits[b,
 * :len_b], tokens[b, :len_b]) in fp64, utterance order.  With dlogits [B][T][K] (nullable) also g times its gradient
 * (rows >= len_b zero), g read from a DEVICE float (NULL: 0).  Workspace >= stts_s2s_loss_workspace_bytes(B). */
long long stts_s2s_loss_workspace_bytes(int B);
int stts_s2s_loss(const float* logits, long long ls_b, long long ls_t, int B, int T, int K, const long long* tokens,
                  long long tok_b, const int* lengths, double* loss, float* dlogits, const float* g, void* ws,
                  long long ws_bytes, void* stream);
/* loss_mono (train.py:306) = 10 l1_loss(attn, attn_mono) over n values: loss (device, 1 double; a fixed-order fp64
 * sum) and, with dattn (nullable), g 10 / n sign(attn - attn_mono) (sign(0) = 0), g a DEVICE float (NULL: 0). */
int stts_mono_loss(const float* attn, const float* attn_mono, long long n, double* loss, float* dattn, const float* g,
                   void* stream);

/* ---- The text aligner's conv stack under train.py's step (Modules/ASR/models.py ASRCNN :37-48, layers.py ConvBlock
 * :105-131; csrc/aligner_cnn_train.hip).  fp32 frames [B][L][C]; every sum in a fixed order, no atomics.  The convs
 * themselves (with their ReLU) are stts_conv1d_fwd_act / stts_conv1d_bwd.
 *
 * Dropout arguments (p, seed, keep_mask), the same in the four entry points that take them: p = 0 is the identity;
 * with keep_mask (fp32, laid out as the tensor it applies to, 1 = kept) y = mask != 0 ? v / (1 - p) : 0, as
 * stts_dropout_mask; otherwise flat element i is kept exactly when stts_dropout(seed) keeps element i of the same
 * tensor, so a fused result is bitwise the unfused pair and a backward redraws instead of storing.  0 <= p < 1. */

/* nn.GroupNorm(G, C) (eps 1e-5, biased variance) of v = relu ? max(x, 0) : x over each (utterance, group)'s C / G
 * channels x L frames, then the dropout above:  y = dropout((v - mean) rstd w[c] + b[c]).  stats [B][G][2] keeps
 * (mean, rstd) for the backward.  The L rows are cut into S row slices, S a function of L alone (16 rows each, at
 * most 256): a workgroup per (64 channels, slice, utterance) writes fp64 partials, a second pass adds them in channel
 * and slice order, so a batch row's y is bitwise its B = 1 result.  C % G == 0; B <= 65535.
 * Workspace >= stts_groupnorm_fwd_train_workspace_bytes(B, L, C, G) = B S C 2 doubles rounded up to 256 bytes. */
long long stts_groupnorm_fwd_train_workspace_bytes(int B, int L, int C, int G);
int stts_groupnorm_fwd_train(const float* x, const float* w, const float* b, int B, int L, int C, int G, int relu,
                             float p, unsigned long long seed, const float* keep_mask, float* y, float* stats,
                             void* ws, long long ws_bytes, void* stream);
/* Its backward from dy (the gradient of y, after the dropout): with g = dropout(dy), g' = g w[c],
 * xhat = (v - mean) rstd, n = L C / G:  dv = rstd (g' - sum g' / n - xhat sum(g' xhat) / n),
 * dx = relu ? dv (x > 0) : dv,  dw[c] = sum_{b,l} g xhat,  db[c] = sum_{b,l} g (utterances in ascending b).
 * dx, dw, db are each nullable.  Same x, w, stats, relu and dropout arguments as the forward. */
long long stts_groupnorm_bwd_workspace_bytes(int B, int L, int C, int G);
int stts_groupnorm_bwd(const float* x, const float* w, const float* stats, const float* dy, int B, int L, int C, int G,
                       int relu, float p, unsigned long long seed, const float* keep_mask, float* dx, float* dw,
                       float* db, void* ws, long long ws_bytes, void* stream);
/* The ConvBlock tail `x = block(x); x += res` (layers.py:116-118): y = r + dropout(x) over n >= 1 values.  Backward:
 * dx = stts_dropout / stts_dropout_mask of dy, dr = dy itself. */
int stts_dropout_add_fwd(const float* x, const float* r, long long n, float p, unsigned long long seed,
                         const float* keep_mask, float* y, void* stream);
/* MFCC.forward (layers.py:60-74): mel [B][n_mels][T], dct [n_mels][n_mfcc] (the module's dct_mat buffer) ->
 * out frames [B][T][n_mfcc].  No backward: the mel is data and dct_mat a buffer. */
int stts_mfcc_frames(const float* mel, const float* dct, int B, int n_mels, int T, int n_mfcc, float* out,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STTS2_TRAIN_H */
