// Model plans (HiFi-GAN / iSTFTNet decoders, F0/N conv stacks, style encoder, pitch extractor) and the
// C-ABI declared in include/stts2.h.  A plan is built from the constructor arguments of the
// reference module, names every parameter exactly like the reference state dict, packs the
// weights (weight-norm fold + MFMA layout) into a caller buffer, and strings the gfx950
// kernels together for one forward.  All launches go to the caller's stream; the workspace
// is carved by a bump allocator whose dry run gives stts_workspace_bytes().
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/stts2.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr size_t ALIGN = 256;
inline size_t rup(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline int rup8(int x) { return (x + 7) & ~7; }

// ----------------------------------------------------------------------- profiling
struct Prof {
  bool on = false;
  std::vector<hipEvent_t> ev;  // pairs
  size_t used = 0;
  long long launches = 0;
  double flops = 0, bytes = 0;
  struct Rec { int shape[8]; double flops, bytes; };
  std::vector<Rec> rec;  // one per timed launch, in launch order
} g_prof;

// ----------------------------------------------------------------------- parameters
struct Params {
  std::vector<std::string> names;
  std::vector<long long> numel;
  std::vector<const float*> ptr;
  int add(const std::string& n, long long k) {
    names.push_back(n);
    numel.push_back(k);
    ptr.push_back(nullptr);
    return (int)names.size() - 1;
  }
  const float* operator[](int i) const { return i < 0 ? nullptr : ptr[i]; }
};

// An eval-mode BatchNorm2d: its running statistics folded at pack time into (scale, shift) in the aux area
struct BNorm {
  int w = -1, b = -1, mean = -1, var = -1, C = 0;
  size_t off = 0;  // aux: scale [C], then shift [C]
};

// A convolution whose weights are packed for conv1d_igemm.
struct WConv {
  int v = -1, g = -1, bias = -1;
  int Cin = 0, Cout = 0, K = 0, transposed = 0, u = 1;
  int reframe = 0;  // > 0: a Conv1d(1, Cout, 2S, stride S) packed as a 2-tap conv over S-sample frames
  // pack-time prep (Vocos): rows scaled by parameter `rs` (layer scale), or only `src_rows` < Cout rows
  // in the parameter (the rest packed as zero columns); the bias then lives folded / padded in aux
  int rs = -1, src_rows = 0;
  size_t bias_aux = 0;
  bool aux_bias = false;
  // pack-time prep (pitch extractor): the BatchNorm that follows the conv folded into it (rows scaled by its
  // scale, its shift as the bias)
  const BNorm* bn = nullptr;
  size_t off[ST_NDTYPES] = {0, 0, 0};
  // fold > 1: a stride-`fold` conv (padding fpad0) packed as the stride-1 conv over phase-folded frames
  // (fold consecutive input rows side by side): fold Cin channels, fK taps, padding fpad (k_fold_w)
  int fold = 0, fpad0 = 0, fK = 0, fpad = 0;
  int taps() const { return fold ? fK : (transposed ? (K + u - 1) / u : K); }
  int N() const { return transposed ? u * Cout : Cout; }
  int pCin() const { return fold ? fold * Cin : Cin; }
};

// the stride-1 form of a stride-st conv (K taps, padding pad): input row st q + t - pad = st (q + s') + ph
void set_fold(WConv& c, int st, int pad) {
  int smin = 1 << 30, smax = -(1 << 30);
  for (int t = 0; t < c.K; ++t) {
    const int j = t - pad;
    const int sq = j >= 0 ? j / st : -((-j + st - 1) / st);  // floor(j / st)
    smin = std::min(smin, sq);
    smax = std::max(smax, sq);
  }
  c.fold = st;
  c.fpad0 = pad;
  c.fK = smax - smin + 1;
  c.fpad = -smin;
}

struct WAdaIN {
  int w = -1, b = -1, C = 0, hoff = 0;
};

struct ResBlock1 {  // AdaINResBlock1 (hifigan.py:26-80)
  int C = 0, K = 0, dil[3] = {1, 3, 5};
  WConv c1[3], c2[3];
  WAdaIN a1[3], a2[3];
  int al1[3], al2[3];
};

struct AdainBlk {  // AdainResBlk1d (hifigan.py:359-403)
  int cin = 0, cout = 0;
  bool up = false, learned = false;
  WConv conv1, conv2, sc;
  WAdaIN n1, n2;
  int pool_v = -1, pool_g = -1, pool_b = -1;
  size_t pool_off = 0;  // folded fp32 [cin][3] in the aux area
};

struct Small {  // weight-norm conv folded to fp32 for a VALU kernel
  int v = -1, g = -1, bias = -1;
  long long rows = 0, inner = 0;
  size_t off = 0;
};

// The small-batch decoder's side streams (decoder_forward): a stage's resblocks 1.. run on streams 0.., every noise
// branch on stream NOISE.  Streams and events are made on first use and live as long as the model.
struct SideStreams {
  enum { N = 4, NOISE = 2, FORK = 0, JOIN = N, MARK = 2 * N, NEV = 2 * N + 8 };
  hipStream_t st[N] = {};
  hipEvent_t ev[NEV] = {};  // FORK + the first stream forked, JOIN + the stream joined, MARK + k
  ~SideStreams() {
    for (auto& s : st)
      if (s) (void)hipStreamDestroy(s);
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int record(int k, hipStream_t s) {
    if (!ev[k]) ST_CHECK_HIP(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
    return (int)hipEventRecord(ev[k], s);
  }

  // One forward's forks from its stream `main`.  It knows which side streams run ahead of `main`, and on scope exit
  // joins those that are not joined back yet: an error return leaves no side-stream work outside a hipGraph capture
  // or still writing the workspace after the call returns.
  struct Forks {
    SideStreams& r;
    hipStream_t main;
    bool ahead[N] = {};
    int marked[N] = {};  // the last mark recorded on a stream that is ahead
    ~Forks() {
      for (int i = 0; i < N; ++i)
        if (ahead[i]) (void)join(i);
    }
    // streams i0 .. i0 + n - 1 go on after everything queued so far on main
    int fork(int i0, int n = 1) {
      for (int i = i0; i < i0 + n; ++i)
        if (!r.st[i]) ST_CHECK_HIP(hipStreamCreateWithFlags(&r.st[i], hipStreamNonBlocking));
      ST_CHECK(r.record(FORK + i0, main));
      for (int i = i0; i < i0 + n; ++i) {
        ST_CHECK_HIP(hipStreamWaitEvent(r.st[i], r.ev[FORK + i0], 0));
        ahead[i] = true;
        marked[i] = -1;
      }
      return 0;
    }
    // main goes on after everything queued so far on stream i
    int join(int i) {
      ahead[i] = false;
      ST_CHECK(r.record(JOIN + i, r.st[i]));
      return (int)hipStreamWaitEvent(main, r.ev[JOIN + i], 0);
    }
    // a join in two halves: mark k is a point on stream i that main waits for later (the noise branches: one mark
    // per stage, reused across forwards); waiting for the stream's last mark joins it
    int mark(int i, int k) {
      marked[i] = k;
      return r.record(MARK + k, r.st[i]);
    }
    int wait(int i, int k) {
      if (marked[i] == k) ahead[i] = false;
      return (int)hipStreamWaitEvent(main, r.ev[MARK + k], 0);
    }
  };
};

}  // namespace

struct stts_model {
  int kind = 0;
  Params P;
  SideStreams side;
  // the side streams and events are per model: concurrent forwards of one model (with their own workspaces and
  // streams) take turns through the forks and joins, so each wait sees its own forward's record
  std::mutex branch_mu;
  stts_model() = default;
  stts_model(const stts_model&) = delete;
  stts_model& operator=(const stts_model&) = delete;
  // -------- decoder config
  int dim_in = 512, style_dim = 128, init_ch = 512, n_fft = 0, hop = 0;
  std::vector<int> rates, kernels, rbk;
  std::vector<std::vector<int>> rbd;
  // -------- decoder layers
  AdainBlk encode, decode[4];
  Small F0_conv, N_conv;
  WConv asr_res;
  int l_lin_w = -1, l_lin_b = -1;
  std::vector<int> nc_w, nc_b;      // hifigan noise_convs (Cin=1): raw [C][K] (VALU kernel), -1 if nc_mm
  std::vector<WConv> nc_mm;         // hifigan noise_convs with K >= 16: 2-tap MFMA conv over S-sample frames
  std::vector<WConv> nc_conv;       // istftnet noise_convs (Cin=n_fft+2): igemm
  std::vector<WConv> ups;
  std::vector<ResBlock1> noise_res, resblocks;
  std::vector<int> alphas;
  WConv conv_post;
  int stft_fr = -1, stft_fi = -1, stft_br = -1, stft_bi = -1;
  // -------- Vocos generator (Modules/vocos.py:108-162, ISTFTHead :248-296)
  bool pwn = false;  // weight norm as torch.nn.utils.parametrizations (original0 = g, original1 = v)
  int vc_inter = 0, vc_layers = 0;
  struct CNX {
    int dw_w = -1, dw_b = -1, gamma = -1;
    WAdaIN norm;
    WConv pw1, pw2;
  };
  std::vector<CNX> cnx;
  int ln_w = -1, ln_b = -1, vwin = -1;
  WConv vhead;  // -------- F0N
  int d_hid = 512;
  AdainBlk f0blk[3], nblk[3];
  WConv f0_proj, n_proj;
  // -------- style encoder (models.py:125-150)
  struct SEBlk {
    int cin = 0, cout = 0;
    bool learned = false;
    WConv conv1, conv2, sc;
    int dw_w = -1, dw_b = -1;
  } se_blk[4];
  WConv se_conv0, se_last;
  int se_lin_w = -1, se_lin_b = -1, se_dim = 0;
  // -------- MultiPeriodDiscriminator (Modules/discriminators.py:96-156)
  struct DiscP {
    int period = 0;
    WConv convs[5], post;
  };
  std::vector<DiscP> mpd;
  // -------- MultiResSpecDiscriminator (Modules/discriminators.py:29-94)
  struct DiscS {
    int n_fft = 0, hop = 0, win = 0;
    WConv convs[5], out;
  };
  std::vector<DiscS> msd;
  // -------- pitch extractor (Modules/JDC/model.py JDCNet; forward :102-137)
  struct PEBlk {
    int cin = 0, cout = 0;
    BNorm pre, mid;
    WConv c1, c2, sc;
  } pe_blk[3];
  WConv pe_c0, pe_c1;
  BNorm pe_bn0, pe_pool;
  int pe_lstm[8] = {-1, -1, -1, -1, -1, -1, -1, -1}, pe_cls_w = -1, pe_cls_b = -1, pe_nclass = 0;
  std::vector<BNorm*> bns;
  // -------- text aligner (Modules/ASR/models.py ASRCNN; forward :37-48, ASRS2S :118-176)
  struct ALBlk {  // one entry of ConvBlock.blocks: conv(dil) -> ReLU -> GroupNorm(8) -> conv -> ReLU, + input
    WConv c1, c2;
    int dil = 1, gn_w = -1, gn_b = -1;
  };
  struct ALLayer {  // ConvBlock, GroupNorm(1)
    ALBlk blk[3];
    int gn_w = -1, gn_b = -1;
  };
  std::vector<ALLayer> al_layers;
  WConv al_init, al_proj;
  int al_ntok = 0, al_emb = 0;
  int al_dct = -1, al_ctc_w[2] = {-1, -1}, al_ctc_b[2] = {-1, -1}, al_embw = -1, al_pns_w = -1, al_pns_b = -1,
      al_query = -1, al_memory = -1, al_v = -1, al_loc = -1, al_dense = -1, al_wih = -1, al_whh = -1, al_bih = -1,
      al_bhh = -1, al_ph_w = -1, al_ph_b = -1;
  size_t al_wc_t = 0, al_wq_t = 0, al_wloc_t = 0;  // aux: the recurrence's weights k-major (pack_model)
  // -------- AdaIN projections (all AdaIN layers share one GEMV: H = s @ Wt + b)
  std::vector<WAdaIN*> adains;
  int Htot = 0;
  size_t wt_off = 0, bcat_off = 0;  // fp32 Wt [style_dim][Htot], bias [Htot] in the aux area
  // -------- packing
  std::vector<WConv*> convs;
  std::vector<Small*> smalls;
  std::vector<AdainBlk*> pools;
  size_t conv_bytes[ST_NDTYPES] = {0, 0, 0};
  size_t aux_off[ST_NDTYPES] = {0, 0, 0}, aux_bytes = 0, scratch_off[ST_NDTYPES] = {0, 0, 0}, scratch_bytes = 0;
  size_t total_bytes[ST_NDTYPES] = {0, 0, 0};
  const char* packed[ST_NDTYPES] = {nullptr, nullptr, nullptr};
};

namespace {

using Model = stts_model;

// ----------------------------------------------------------------------- builders
void add_wconv(Model& m, WConv& c, const std::string& p, int cin, int cout, int k, bool wn, bool bias,
               int transposed = 0, int u = 1, int groups = 1) {
  c.Cin = cin;
  c.Cout = cout;
  c.K = k;
  c.transposed = transposed;
  c.u = u;
  if (bias) c.bias = m.P.add(p + ".bias", cout);
  if (wn) {
    c.g = m.P.add(p + (m.pwn ? ".parametrizations.weight.original0" : ".weight_g"), transposed ? cin : cout);
    c.v = m.P.add(p + (m.pwn ? ".parametrizations.weight.original1" : ".weight_v"), (long long)cin * cout / groups * k);
  } else {
    c.v = m.P.add(p + ".weight", (long long)cin * cout / groups * k);
  }
  m.convs.push_back(&c);
}

void add_adain(Model& m, WAdaIN& a, const std::string& p, int C) {
  a.C = C;
  a.w = m.P.add(p + ".fc.weight", (long long)2 * C * m.style_dim);
  a.b = m.P.add(p + ".fc.bias", 2 * C);
  m.adains.push_back(&a);
}

void add_resblock1(Model& m, ResBlock1& r, const std::string& p, int C, int K, const int* dil) {
  r.C = C;
  r.K = K;
  for (int j = 0; j < 3; ++j) r.dil[j] = dil[j];
  for (int j = 0; j < 3; ++j) add_wconv(m, r.c1[j], p + ".convs1." + std::to_string(j), C, C, K, true, true);
  for (int j = 0; j < 3; ++j) add_wconv(m, r.c2[j], p + ".convs2." + std::to_string(j), C, C, K, true, true);
  for (int j = 0; j < 3; ++j) add_adain(m, r.a1[j], p + ".adain1." + std::to_string(j), C);
  for (int j = 0; j < 3; ++j) add_adain(m, r.a2[j], p + ".adain2." + std::to_string(j), C);
  for (int j = 0; j < 3; ++j) r.al1[j] = m.P.add(p + ".alpha1." + std::to_string(j), C);
  for (int j = 0; j < 3; ++j) r.al2[j] = m.P.add(p + ".alpha2." + std::to_string(j), C);
}

void add_adainblk(Model& m, AdainBlk& b, const std::string& p, int cin, int cout, bool up) {
  b.cin = cin;
  b.cout = cout;
  b.up = up;
  b.learned = cin != cout;
  add_wconv(m, b.conv1, p + ".conv1", cin, cout, 3, true, true);
  add_wconv(m, b.conv2, p + ".conv2", cout, cout, 3, true, true);
  add_adain(m, b.n1, p + ".norm1", cin);
  add_adain(m, b.n2, p + ".norm2", cout);
  if (b.learned) add_wconv(m, b.sc, p + ".conv1x1", cin, cout, 1, true, false);
  if (up) {
    b.pool_b = m.P.add(p + ".pool.bias", cin);
    b.pool_g = m.P.add(p + (m.pwn ? ".pool.parametrizations.weight.original0" : ".pool.weight_g"), cin);
    b.pool_v = m.P.add(p + (m.pwn ? ".pool.parametrizations.weight.original1" : ".pool.weight_v"), (long long)cin * 3);
    m.pools.push_back(&b);
  }
}

void add_small_wn(Model& m, Small& s, const std::string& p, long long rows, long long inner) {
  s.rows = rows;
  s.inner = inner;
  s.bias = m.P.add(p + ".bias", rows);
  s.g = m.P.add(p + (m.pwn ? ".parametrizations.weight.original0" : ".weight_g"), rows);
  s.v = m.P.add(p + (m.pwn ? ".parametrizations.weight.original1" : ".weight_v"), rows * inner);
  m.smalls.push_back(&s);
}

// decoder front-end (hifigan.py:427-440 == istftnet.py:673-686 == vocos.py:370-390)
void add_frontend(Model& m) {
  add_adainblk(m, m.encode, "encode", m.dim_in + 2, 1024, false);
  for (int k = 0; k < 4; ++k)
    add_adainblk(m, m.decode[k], "decode." + std::to_string(k), 1024 + 2 + 64, k == 3 ? 512 : 1024, k == 3);
  add_small_wn(m, m.F0_conv, "F0_conv", 1, 3);
  add_small_wn(m, m.N_conv, "N_conv", 1, 3);
  add_wconv(m, m.asr_res, "asr_res.0", m.dim_in, 64, 1, true, true);
}

// Vocos Decoder (Modules/vocos.py:364-390): cfg = dim_in, style_dim, intermediate_dim, num_layers,
// n_fft, hop.  The generator's dim is dim_in and its input is decode.3's 512 channels, so the
// reference itself only runs with dim_in = 512.
int build_vocos(Model& m, const int* cfg, int n) {
  if (n != 6) return ST_EINVAL;
  m.dim_in = cfg[0];
  m.style_dim = cfg[1];
  m.vc_inter = cfg[2];
  m.vc_layers = cfg[3];
  m.n_fft = cfg[4];
  m.hop = cfg[5];
  if (m.dim_in != 512 || m.style_dim <= 0 || m.vc_inter <= 0 || m.vc_inter % 32 || m.vc_layers <= 0 ||
      m.vc_layers > 64 || m.hop <= 0 || m.hop > m.n_fft || (m.n_fft - m.hop) / 2 <= 0)
    return ST_EINVAL;
  int n1 = 0, n2 = 0;
  if (st_istft_factor(m.n_fft, &n1, &n2) != ST_OK) return ST_EINVAL;
  m.pwn = true;
  add_frontend(m);
  const int d = m.dim_in;
  m.cnx.resize(m.vc_layers);  // sized once: add_wconv / add_adain keep pointers into it
  for (int i = 0; i < m.vc_layers; ++i) {
    auto& b = m.cnx[i];
    const std::string p = "generator.convnext." + std::to_string(i);
    b.dw_w = m.P.add(p + ".dwconv.weight", (long long)d * 7);
    b.dw_b = m.P.add(p + ".dwconv.bias", d);
    add_adain(m, b.norm, p + ".norm", d);
    add_wconv(m, b.pw1, p + ".pwconv1", d, m.vc_inter, 1, false, true);  // nn.Linear == [Cout][Cin][1]
    add_wconv(m, b.pw2, p + ".pwconv2", m.vc_inter, d, 1, false, true);
    b.gamma = m.P.add(p + ".gamma", d);
    b.pw2.rs = b.gamma;  // gamma * (W x + b) folded into the packed weights and bias
    b.pw2.aux_bias = true;
  }
  m.ln_w = m.P.add("generator.final_layer_norm.weight", d);
  m.ln_b = m.P.add("generator.final_layer_norm.bias", d);
  const int nout = 2 * (m.n_fft / 2 + 1);
  add_wconv(m, m.vhead, "generator.stft.out", d, nout, 1, false, true);
  m.vhead.src_rows = nout;  // columns padded to the MFMA 16-column multiple (the wide epilogue)
  m.vhead.Cout = (nout + 15) & ~15;
  m.vhead.aux_bias = true;
  m.vwin = m.P.add("generator.stft.istft.window", m.n_fft);
  return ST_OK;
}

int build_decoder(Model& m, const int* cfg, int n) {
  int i = 0;
  auto take = [&](int& dst) -> bool {
    if (i >= n) return false;
    dst = cfg[i++];
    return true;
  };
  int nup = 0, nrb = 0;
  if (!take(m.dim_in) || !take(m.style_dim) || !take(m.init_ch) || !take(nup) || nup <= 0 || nup > 8) return ST_EINVAL;
  m.rates.resize(nup);
  m.kernels.resize(nup);
  for (auto& r : m.rates)
    if (!take(r) || r <= 0) return ST_EINVAL;
  for (auto& k : m.kernels)
    if (!take(k) || k <= 0) return ST_EINVAL;
  if (!take(nrb) || nrb <= 0 || nrb > 8) return ST_EINVAL;
  m.rbk.resize(nrb);
  m.rbd.assign(nrb, std::vector<int>(3));
  for (auto& k : m.rbk)
    if (!take(k) || k <= 0 || k % 2 == 0) return ST_EINVAL;
  for (auto& d : m.rbd)
    for (auto& x : d)
      if (!take(x) || x <= 0) return ST_EINVAL;
  if (m.kind == STTS_KIND_ISTFTNET) {
    if (!take(m.n_fft) || !take(m.hop) || m.n_fft <= 0 || m.hop <= 0) return ST_EINVAL;
  }
  if (i != n) return ST_EINVAL;
  if (m.init_ch != 512) return ST_EINVAL;  // decode.3 emits 512 channels (hifigan.py:432)
  const bool ist = m.kind == STTS_KIND_ISTFTNET;
  add_frontend(m);
  // generator (hifigan.py:272-319 / istftnet.py:494-540)
  m.l_lin_w = m.P.add("generator.m_source.l_linear.weight", 9);
  m.l_lin_b = m.P.add("generator.m_source.l_linear.bias", 1);
  m.ups.resize(nup);
  m.noise_res.resize(nup);
  m.resblocks.resize((size_t)nup * nrb);
  if (ist) m.nc_conv.resize(nup);
  else m.nc_mm.resize(nup);
  static const int d135[3] = {1, 3, 5};
  for (int s = 0; s < nup; ++s) {
    const int u = m.rates[s], k = m.kernels[s];
    const int cin = m.init_ch >> s, c = m.init_ch >> (s + 1);
    const std::string gp = "generator.";
    add_wconv(m, m.ups[s], gp + "ups." + std::to_string(s), cin, c, k, true, true, 1, u);
    int sf = 1;
    for (int j = s + 1; j < nup; ++j) sf *= m.rates[j];
    const bool last = s + 1 == nup;
    const int nk = last ? 1 : 2 * sf;
    if (ist) {
      add_wconv(m, m.nc_conv[s], gp + "noise_convs." + std::to_string(s), m.n_fft + 2, c, nk, false, true);
    } else if (nk >= 16 && nk == 2 * sf && sf <= 32) {
      // stride-S conv over the source = 2-tap conv over S-sample frames (k_har_frames)
      add_wconv(m, m.nc_mm[s], gp + "noise_convs." + std::to_string(s), sf, c, 2, false, true);
      m.nc_mm[s].reframe = sf;
      m.nc_w.push_back(-1);
      m.nc_b.push_back(-1);
    } else {
      m.nc_w.push_back(m.P.add(gp + "noise_convs." + std::to_string(s) + ".weight", (long long)c * nk));
      m.nc_b.push_back(m.P.add(gp + "noise_convs." + std::to_string(s) + ".bias", c));
    }
    add_resblock1(m, m.noise_res[s], gp + "noise_res." + std::to_string(s), c, last ? 11 : 7, d135);
  }
  if (!ist) m.alphas.push_back(m.P.add("generator.alphas.0", m.init_ch));
  for (int s = 0; s < nup; ++s) {
    const int c = m.init_ch >> (s + 1);
    if (!ist) m.alphas.push_back(m.P.add("generator.alphas." + std::to_string(s + 1), c));
    for (int j = 0; j < nrb; ++j)
      add_resblock1(m, m.resblocks[(size_t)s * nrb + j], "generator.resblocks." + std::to_string(s * nrb + j), c,
                    m.rbk[j], m.rbd[j].data());
  }
  const int clast = m.init_ch >> nup;
  add_wconv(m, m.conv_post, "generator.conv_post", clast, ist ? m.n_fft + 2 : 1, 7, true, true);
  if (ist) {
    const int nb = m.n_fft / 2 + 1;
    m.P.add("generator.stft.window", m.n_fft);
    m.stft_fr = m.P.add("generator.stft.weight_forward_real", (long long)nb * m.n_fft);
    m.stft_fi = m.P.add("generator.stft.weight_forward_imag", (long long)nb * m.n_fft);
    m.stft_br = m.P.add("generator.stft.weight_backward_real", (long long)nb * m.n_fft);
    m.stft_bi = m.P.add("generator.stft.weight_backward_imag", (long long)nb * m.n_fft);
  }
  return ST_OK;
}

int build_f0n(Model& m, const int* cfg, int n) {
  if (n != 2 || cfg[0] <= 0 || cfg[0] % 2 || cfg[1] <= 0) return ST_EINVAL;
  m.d_hid = cfg[0];
  m.style_dim = cfg[1];
  const int d = m.d_hid;
  const char* br[2] = {"F0", "N"};
  AdainBlk* blks[2] = {m.f0blk, m.nblk};
  for (int b = 0; b < 2; ++b) {
    const std::string p = br[b];
    add_adainblk(m, blks[b][0], p + ".0", d, d, false);
    add_adainblk(m, blks[b][1], p + ".1", d, d / 2, true);
    add_adainblk(m, blks[b][2], p + ".2", d / 2, d / 2, false);
  }
  add_wconv(m, m.f0_proj, "F0_proj", d / 2, 1, 1, false, true);
  add_wconv(m, m.n_proj, "N_proj", d / 2, 1, 1, false, true);
  return ST_OK;
}

int build_style(Model& m, const int* cfg, int n) {
  if (n != 3 || cfg[0] <= 0 || cfg[1] <= 0 || cfg[2] <= 0) return ST_EINVAL;
  int d = cfg[0];
  m.style_dim = cfg[1];
  add_wconv(m, m.se_conv0, "shared.0", 1, d, 9, false, true);
  for (int i = 0; i < 4; ++i) {
    auto& b = m.se_blk[i];
    const int dout = std::min(d * 2, cfg[2]);
    const std::string p = "shared." + std::to_string(i + 1);
    b.cin = d;
    b.cout = dout;
    b.learned = d != dout;
    add_wconv(m, b.conv1, p + ".conv1", d, d, 9, false, true);
    add_wconv(m, b.conv2, p + ".conv2", d, dout, 9, false, true);
    if (b.learned) add_wconv(m, b.sc, p + ".conv1x1", d, dout, 1, false, false);
    b.dw_w = m.P.add(p + ".downsample_res.conv.weight", (long long)d * 9);
    b.dw_b = m.P.add(p + ".downsample_res.conv.bias", d);
    d = dout;
  }
  add_wconv(m, m.se_last, "shared.6", d, d, 25, false, true);
  m.se_lin_w = m.P.add("unshared.weight", (long long)m.style_dim * d);
  m.se_lin_b = m.P.add("unshared.bias", m.style_dim);
  m.se_dim = d;
  return ST_OK;
}

void add_bn(Model& m, BNorm& bn, const std::string& p, int C) {
  bn.C = C;
  bn.w = m.P.add(p + ".weight", C);
  bn.b = m.P.add(p + ".bias", C);
  bn.mean = m.P.add(p + ".running_mean", C);
  bn.var = m.P.add(p + ".running_var", C);
  m.bns.push_back(&bn);
}

// JDCNet(num_class) (Modules/JDC/model.py:14-72), the layers forward runs: conv_block, res_block1..3, pool_block,
// bilstm_classifier, classifier.  The 3x3 weights [Cout][Cin][3][3] (frames x bins) are the 9-tap weights of the
// (T x 80) image as they lie.  The detector branch is never run by forward and is not part of the plan.
constexpr int kPitchCh[4] = {64, 128, 192, 256};
constexpr int kPitchBins = 80, kPitchH = 256;
constexpr float kPitchSlope = 0.01f;
int build_pitch(Model& m, const int* cfg, int n) {
  if (n != 1 || cfg[0] <= 0) return ST_EINVAL;
  m.pe_nclass = cfg[0];
  add_wconv(m, m.pe_c0, "conv_block.0", 1, 64, 9, false, false);
  add_bn(m, m.pe_bn0, "conv_block.1", 64);
  m.pe_c0.bn = &m.pe_bn0;
  add_wconv(m, m.pe_c1, "conv_block.3", 64, 64, 9, false, false);
  for (int i = 0; i < 3; ++i) {
    auto& b = m.pe_blk[i];
    const std::string p = "res_block" + std::to_string(i + 1);
    b.cin = kPitchCh[i];
    b.cout = kPitchCh[i + 1];
    add_bn(m, b.pre, p + ".pre_conv.0", b.cin);
    add_wconv(m, b.c1, p + ".conv.0", b.cin, b.cout, 9, false, false);
    add_bn(m, b.mid, p + ".conv.1", b.cout);
    b.c1.bn = &b.mid;
    add_wconv(m, b.c2, p + ".conv.3", b.cout, b.cout, 9, false, false);
    add_wconv(m, b.sc, p + ".conv1by1", b.cin, b.cout, 1, false, false);
  }
  add_bn(m, m.pe_pool, "pool_block.0", 256);
  static const char* const ln[4] = {"weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"};
  for (int d = 0; d < 2; ++d)
    for (int k = 0; k < 4; ++k) {
      const long long numel = k == 0 ? 4LL * kPitchH * 512 : (k == 1 ? 4LL * kPitchH * kPitchH : 4LL * kPitchH);
      m.pe_lstm[4 * d + k] = m.P.add(std::string("bilstm_classifier.") + ln[k] + (d ? "_reverse" : ""), numel);
    }
  m.pe_cls_w = m.P.add("classifier.weight", (long long)m.pe_nclass * 512);
  m.pe_cls_b = m.P.add("classifier.bias", m.pe_nclass);
  return ST_OK;
}

// ASRCNN(input_dim, hidden_dim, n_token, n_layers, token_embedding_dim) (Modules/ASR/models.py:9-35): every one of
// its 143 state-dict entries is read by forward, so the plan's names are the state dict's.  The kernels are built for
// the reference's widths: 80 mel bins -> 40 MFCCs, hidden_dim 256 (memory, decoder and attention width 128).
constexpr int kAlMel = 80, kAlMfcc = 40, kAlHid = 256, kAlDec = 128, kAlLocF = 32, kAlLocK = 63;
int build_aligner(Model& m, const int* cfg, int n) {
  if (n != 5 || cfg[0] != kAlMel || cfg[1] != kAlHid || cfg[2] < 4 || cfg[3] < 1 || cfg[3] > 64 || cfg[4] < 1)
    return ST_EINVAL;
  m.al_ntok = cfg[2];
  m.al_emb = cfg[4];
  const int H = kAlHid, D = kAlDec;
  m.al_dct = m.P.add("to_mfcc.dct_mat", (long long)kAlMel * kAlMfcc);
  add_wconv(m, m.al_init, "init_cnn.conv", kAlMfcc, H, 7, false, true);
  m.al_layers.resize(cfg[3]);  // sized once: add_wconv keeps pointers into it
  for (int i = 0; i < cfg[3]; ++i) {
    auto& l = m.al_layers[i];
    const std::string p = "cnns." + std::to_string(i);
    for (int j = 0, dil = 1; j < 3; ++j, dil *= 3) {
      auto& b = l.blk[j];
      const std::string q = p + ".0.blocks." + std::to_string(j);
      b.dil = dil;
      add_wconv(m, b.c1, q + ".0.conv", H, H, 3, false, true);
      b.gn_w = m.P.add(q + ".2.weight", H);
      b.gn_b = m.P.add(q + ".2.bias", H);
      add_wconv(m, b.c2, q + ".4.conv", H, H, 3, false, true);
    }
    l.gn_w = m.P.add(p + ".1.weight", H);
    l.gn_b = m.P.add(p + ".1.bias", H);
  }
  add_wconv(m, m.al_proj, "projection.conv", H, D, 1, false, true);
  m.al_ctc_w[0] = m.P.add("ctc_linear.0.linear_layer.weight", (long long)H * D);
  m.al_ctc_b[0] = m.P.add("ctc_linear.0.linear_layer.bias", H);
  m.al_ctc_w[1] = m.P.add("ctc_linear.2.linear_layer.weight", (long long)m.al_ntok * H);
  m.al_ctc_b[1] = m.P.add("ctc_linear.2.linear_layer.bias", m.al_ntok);
  const std::string s = "asr_s2s.", a = s + "attention_layer.";
  m.al_embw = m.P.add(s + "embedding.weight", (long long)m.al_ntok * m.al_emb);
  m.al_pns_w = m.P.add(s + "project_to_n_symbols.weight", (long long)m.al_ntok * D);
  m.al_pns_b = m.P.add(s + "project_to_n_symbols.bias", m.al_ntok);
  m.al_query = m.P.add(a + "query_layer.linear_layer.weight", (long long)D * D);
  m.al_memory = m.P.add(a + "memory_layer.linear_layer.weight", (long long)D * D);
  m.al_v = m.P.add(a + "v.linear_layer.weight", D);
  m.al_loc = m.P.add(a + "location_layer.location_conv.conv.weight", (long long)kAlLocF * 2 * kAlLocK);
  m.al_dense = m.P.add(a + "location_layer.location_dense.linear_layer.weight", (long long)D * kAlLocF);
  m.al_wih = m.P.add(s + "decoder_rnn.weight_ih", 4LL * D * (D + m.al_emb));
  m.al_whh = m.P.add(s + "decoder_rnn.weight_hh", 4LL * D * D);
  m.al_bih = m.P.add(s + "decoder_rnn.bias_ih", 4 * D);
  m.al_bhh = m.P.add(s + "decoder_rnn.bias_hh", 4 * D);
  m.al_ph_w = m.P.add(s + "project_to_hidden.0.linear_layer.weight", (long long)D * 2 * D);
  m.al_ph_b = m.P.add(s + "project_to_hidden.0.linear_layer.bias", D);
  return ST_OK;
}

// MultiPeriodDiscriminator: DiscriminatorP(p) for each period (discriminators.py:132-141); each is
// 5 weight-norm Conv2d (k, 1) stride (3, 1) [the last stride 1] + conv_post (3, 1)
// (discriminators.py:96-106), i.e. 1-d convs along T/p with the same weight memory layout
constexpr int kMpdCh[6] = {1, 32, 128, 512, 1024, 1024};
int build_mpd(Model& m, const int* cfg, int n) {
  if (n < 2 || cfg[0] != n - 1) return ST_EINVAL;
  m.mpd.resize(cfg[0]);  // sized once: add_wconv keeps pointers into it
  for (int i = 0; i < cfg[0]; ++i) {
    if (cfg[1 + i] < 1) return ST_EINVAL;
    auto& d = m.mpd[i];
    d.period = cfg[1 + i];
    const std::string p = "discriminators." + std::to_string(i);
    for (int j = 0; j < 5; ++j)
      add_wconv(m, d.convs[j], p + ".convs." + std::to_string(j), kMpdCh[j], kMpdCh[j + 1], 5, true, true);
    add_wconv(m, d.post, p + ".conv_post", 1024, 1, 3, true, true);
  }
  return ST_OK;
}

// MultiResSpecDiscriminator: SpecDiscriminator(n_fft, hop, win) per resolution (discriminators.py:73-78),
// each 4 weight-norm Conv2d (3, 9) [strides (1,1), (1,2) x 3] + Conv2d (3, 3) + out Conv2d(32, 1, 3)
// (:38-45), cfg = {n, (n_fft, hop, win) x n}
constexpr int kMsdCh = 32;
int build_msd(Model& m, const int* cfg, int n) {
  if (n < 4 || (n - 1) != 3 * cfg[0]) return ST_EINVAL;
  m.msd.resize(cfg[0]);
  for (int i = 0; i < cfg[0]; ++i) {
    auto& d = m.msd[i];
    d.n_fft = cfg[1 + 3 * i];
    d.hop = cfg[2 + 3 * i];
    d.win = cfg[3 + 3 * i];
    if (d.n_fft < 16 || d.n_fft > 2048 || (d.n_fft & (d.n_fft - 1)) || d.hop <= 0 || d.win <= 0 || d.win > d.n_fft)
      return ST_EINVAL;
    const std::string p = "discriminators." + std::to_string(i);
    // a (3, kw) Conv2d runs as a 1-D conv along the bins over 3 C (time-expanded) channels: the
    // reference's [Cout][C][3][kw] weight is exactly the [Cout][3C][kw] Conv1d weight
    for (int j = 0; j < 5; ++j)
      add_wconv(m, d.convs[j], p + ".discriminators." + std::to_string(j), 3 * (j == 0 ? 1 : kMsdCh), kMsdCh,
                j < 4 ? 9 : 3, true, true);
    // the stride (1, 2) layers run folded: stride-1 convs over [W / 2][2 x 96] (N = 32 tiles fill the MFMA
    // columns; the strided tile left 3/4 of them idle)
    if (g_opt_msdfold)
      for (int j = 1; j <= 3; ++j) set_fold(d.convs[j], 2, 4);
    add_wconv(m, d.out, p + ".out", 3 * kMsdCh, 1, 3, true, true);
  }
  return ST_OK;
}

// geometry of SpecDiscriminator over Tn samples: H frames, widths W[0..5] (W[0] = bins; layers 1-3
// halve with kernel 9, pad 4, stride 2)
struct MsdGeom {
  int H, W[6];
};
MsdGeom msd_geom(const Model::DiscS& d, int Tn) {
  MsdGeom g;
  g.H = 1 + Tn / d.hop;
  g.W[0] = g.W[1] = d.n_fft / 2 + 1;
  for (int j = 2; j <= 4; ++j) g.W[j] = (g.W[j - 1] - 1) / 2 + 1;
  g.W[5] = g.W[4];
  return g;
}

// The feature maps one discriminator forward over B signals writes to its flat `out` buffer, in output order (6 per
// period / resolution, the last of them the score map): the one statement of that order and of the sizes, which
// the forwards, stts_*_out_elems and the GAN losses all read.
struct DiscMap {
  long long off, elems;  // start in `out`, size (both in floats, for the B signals the list was made for)
  bool score;
};
using DiscMaps = std::vector<DiscMap>;
long long maps_elems(const DiscMaps& v) { return v.empty() ? 0 : v.back().off + v.back().elems; }  // of all maps
void add_map(DiscMaps& v, long long elems, bool score) { v.push_back({maps_elems(v), elems, score}); }

DiscMaps msd_maps(const Model& m, int S, int Tn) {
  DiscMaps v;
  v.reserve(6 * m.msd.size());
  for (const auto& d : m.msd) {
    const MsdGeom g = msd_geom(d, Tn);
    for (int j = 1; j <= 5; ++j) add_map(v, (long long)S * g.H * g.W[j] * kMsdCh, false);
    add_map(v, (long long)S * g.H * g.W[5], true);
  }
  return v;
}

// per-layer frame counts of DiscriminatorP(p) over Tn samples: L[0] = ceil(Tn / p), then the 4
// stride-3 convs (k5, pad 2), then the stride-1 conv and conv_post keep L[4]
void mpd_lengths(int Tn, int p, int (&L)[6]) {
  L[0] = (Tn + p - 1) / p;
  for (int j = 0; j < 4; ++j) L[j + 1] = (L[j] + 4 - 5) / 3 + 1;
  L[5] = L[4];
}

DiscMaps mpd_maps(const Model& m, int B, int Tn) {
  DiscMaps v;
  v.reserve(6 * m.mpd.size());
  for (const auto& d : m.mpd) {
    int L[6];
    mpd_lengths(Tn, d.period, L);
    for (int j = 1; j <= 5; ++j) add_map(v, (long long)B * d.period * L[j] * kMpdCh[j], false);
    add_map(v, (long long)B * d.period * L[5], true);
  }
  return v;
}

void finalize_layout(Model& m) {
  m.Htot = 0;
  for (auto* a : m.adains) {
    a->hoff = m.Htot;
    m.Htot += 2 * a->C;
  }
  for (int dt = 0; dt < ST_NDTYPES; ++dt) {
    const size_t esz = dt == ST_BF16 ? 2 : 4;  // ST_SPLIT: bf16 hi + lo
    size_t off = 0;
    for (auto* c : m.convs) {
      c->off[dt] = off;
      off += rup(st_packed_conv_elems(c->pCin(), c->Cout, c->fold ? c->fK : c->K, c->transposed, c->u) * esz, ALIGN);
    }
    m.conv_bytes[dt] = off;
  }
  // aux fp32 area: AdaIN Wt + bias, folded small convs, pools (dtype independent)
  size_t a = 0;
  m.wt_off = a;
  a += rup((size_t)m.style_dim * m.Htot * 4, ALIGN);
  m.bcat_off = a;
  a += rup((size_t)m.Htot * 4, ALIGN);
  for (auto* s : m.smalls) {
    s->off = a;
    a += rup((size_t)s->rows * s->inner * 4, ALIGN);
  }
  for (auto* p : m.pools) {
    p->pool_off = a;
    a += rup((size_t)p->cin * 3 * 4, ALIGN);
  }
  for (auto* c : m.convs)
    if (c->aux_bias) {
      c->bias_aux = a;
      a += rup((size_t)c->Cout * 4, ALIGN);
    }
  for (auto* bn : m.bns) {
    bn->off = a;
    a += rup((size_t)2 * bn->C * 4, ALIGN);
  }
  if (m.kind == STTS_KIND_ALIGNER) {
    m.al_wc_t = a;  // [context (128); h (128)][512 gate rows]
    a += rup((size_t)2 * kAlDec * 4 * kAlDec * 4, ALIGN);
    m.al_wq_t = a;  // [h (128)][128]
    a += rup((size_t)kAlDec * kAlDec * 4, ALIGN);
    m.al_wloc_t = a;  // [channel (2) x tap (63)][32 filters]
    a += rup((size_t)2 * kAlLocK * kAlLocF * 4, ALIGN);
  }
  m.aux_bytes = a;
  size_t sc = 0;
  for (auto* c : m.convs) {
    if (c->g >= 0 || c->reframe || c->rs >= 0 || c->src_rows || c->bn) sc = std::max(sc, (size_t)c->Cin * c->Cout * c->K * 4);
    if (c->fold) sc = std::max(sc, rup((size_t)c->Cin * c->Cout * c->K * 4, ALIGN) + (size_t)c->pCin() * c->Cout * c->fK * 4);
  }
  m.scratch_bytes = rup(sc, ALIGN);
  for (int dt = 0; dt < ST_NDTYPES; ++dt) {
    m.aux_off[dt] = m.conv_bytes[dt];
    m.scratch_off[dt] = m.aux_off[dt] + m.aux_bytes;
    m.total_bytes[dt] = m.scratch_off[dt] + m.scratch_bytes;
  }
}

// ----------------------------------------------------------------------- forward context
struct Buf {
  char* p = nullptr;
  long long bs = 0;  // batch stride (elements)
  int ld = 0, L = 0;
  void* at(int c0, size_t esz) const { return p + (size_t)c0 * esz; }
  // the same memory seen as L_ rows of ld_ per batch entry
  Buf view(int L_, int ld_) const { return Buf{p, (long long)L_ * ld_, ld_, L_}; }
};

struct Ctx {
  Model* m;
  int dtype;  // activation storage (ST_FP32 in the split accuracy mode)
  size_t esz;
  int B;
  hipStream_t s;
  bool dry;
  char* ws;
  size_t off = 0;
  size_t stats_begin = 0, stats_off = 0;
  // small batches: conv statistics spread over `slots` copies so that the persistent grids' fp64
  // atomics do not all land on the same few (utterance, channel) addresses (B = 1: ~200-450 us a
  // launch measured, tools/phase_profile.py with PHASE_B=1), folded after each producing launch
  int slots = 1;
  // small batches: fp32 scratch for the split-K partials of the short-conv engine (pwgemm.hip)
  float* splitk = nullptr;
  long long splitk_elems = 0;
  void alloc_splitk(long long rows_x_cols) {
    if (B > 4) return;
    splitk_elems = 8LL * B * rows_x_cols;  // up to 8 slices
    splitk = reinterpret_cast<float*>(alloc((size_t)splitk_elems * 4));
  }
  float* H = nullptr;
  bool h_ready = false;  // H (every AdaIN layer's style projection) already computed this forward
  const char* packed;
  char* aux;
  int cdtype = 0;  // conv engines / packed weights: the run's dtype (ST_SPLIT in the accuracy mode)

  char* alloc(size_t bytes) {
    char* p = dry ? nullptr : ws + off;
    off += rup(bytes, ALIGN);
    return p;
  }
  Buf frames(int L, int ld) {
    Buf b = Buf().view(L, ld);
    b.p = alloc((size_t)B * L * ld * esz);
    return b;
  }
  // n equally sized temporaries of `elems` elements per batch entry; a stage sees them through Buf::view
  void temps(Buf* g, int n, long long elems) {
    for (int i = 0; i < n; ++i) {
      g[i].p = alloc((size_t)B * elems * esz);
      g[i].bs = elems;
    }
  }
  double* stat(int C) {
    double* p = dry ? nullptr : reinterpret_cast<double*>(ws + stats_off);
    stats_off += rup((size_t)slots * B * C * ST_W * sizeof(double), ALIGN);
    return p;
  }
  const void* wpk(const WConv& c) const { return packed + c.off[cdtype]; }
  const float* aux_f(size_t o) const { return reinterpret_cast<const float*>(aux + o); }
  const float* P(int i) const { return m->P[i]; }
};

#define RUN(expr)                \
  do {                           \
    if (!c.dry) {                \
      int _r = (expr);           \
      if (_r != 0) return _r;    \
    }                            \
  } while (0)

Prologue pro_none() {
  Prologue p;
  memset(&p, 0, sizeof(p));
  return p;
}

Prologue pro_adain(Ctx& c, const WAdaIN& a, const double* stats, int stats_ld, int L, int extra, int alpha,
                   float slope) {
  Prologue p = pro_none();
  p.mode = PRO_AFFINE | extra;
  p.stats = stats;
  p.stats_ld = stats_ld;
  p.inv_n = 1.0 / (double)L;
  p.gamma = c.H ? c.H + a.hoff : nullptr;
  p.gb_ld = c.m->Htot;
  p.gb_C = a.C;
  p.alpha = alpha >= 0 ? c.P(alpha) : nullptr;
  p.slope = slope;
  p.stats_slots = c.slots;  // every stats buffer of the arena has c.slots copies (unused ones zero)
  p.stats_slot_bs = (long long)c.B * stats_ld * ST_W;
  return p;
}

ConvParams conv_base(Ctx& c, const WConv& w, const Buf& x, int c0) {
  ConvParams p;
  memset(&p, 0, sizeof(p));
  p.x = x.at(c0, c.esz);
  p.x_bs = x.bs;
  p.x_ld = x.ld;
  p.Lin = x.L;
  p.Cin = w.pCin();
  p.B = c.B;
  p.KS = w.taps();
  p.dil = 1;
  p.stride = 1;
  p.pad = 0;
  p.N = w.N();
  p.w = c.wpk(w);
  p.nchunks = (w.pCin() + 31) / 32;
  p.bias = w.bn ? c.aux_f(w.bn->off) + w.bn->C : (w.aux_bias ? c.aux_f(w.bias_aux) : c.P(w.bias));
  p.Cout = w.Cout;
  p.pro = pro_none();
  p.up = 1;
  p.out_scale = 1.0f;
  p.splitk_ws = c.splitk;
  p.splitk_ws_elems = c.splitk_elems;
  return p;
}

void conv_out(ConvParams& p, Ctx& c, const Buf& y, int c0, int Lout) {
  p.y = y.at(c0, c.esz);
  p.y_bs = y.bs;
  p.y_ld = y.ld;
  p.Lout = Lout;
}
void conv_res(ConvParams& p, Ctx& c, const Buf& r, int c0 = 0) {  // + r (from channel c0) in the epilogue
  p.res = r.at(c0, c.esz);
  p.res_bs = r.bs;
  p.res_ld = r.ld;
}
void conv_acc(ConvParams& p, const Buf& a) {  // + the running sum a
  p.accb = a.p;
  p.acc_bs = a.bs;
  p.acc_ld = a.ld;
}
void conv_stats(ConvParams& p, double* st, int ld) {  // the output's InstanceNorm statistics into st
  p.stats = st;
  p.stats_ld = ld;
}

// runs `call` with the launches going to side stream i and the split-K partials to that stream's scratch; c.s and
// c.splitk are put back on every path
template <typename F>
int on_side(Ctx& c, int i, float* splitk, F&& call) {
  const hipStream_t s0 = c.s;
  float* const splitk0 = c.splitk;
  if (!c.dry) c.s = c.m->side.st[i];
  c.splitk = splitk;
  const int rc = call();
  c.s = s0;
  c.splitk = splitk0;
  return rc;
}

// hipEvent pair around one profiled launch (stts_profile_*)
int prof_begin(Ctx& c) {
  while (g_prof.ev.size() < g_prof.used + 2) {
    hipEvent_t e;
    ST_CHECK_HIP(hipEventCreate(&e));
    g_prof.ev.push_back(e);
  }
  ST_CHECK_HIP(hipEventRecord(g_prof.ev[g_prof.used], c.s));
  return 0;
}
int prof_end(Ctx& c, const int (&shape)[8], double fl, double by) {
  ST_CHECK_HIP(hipEventRecord(g_prof.ev[g_prof.used + 1], c.s));
  g_prof.used += 2;
  g_prof.launches++;
  g_prof.flops += fl;
  g_prof.bytes += by;
  Prof::Rec r;
  for (int k = 0; k < 8; ++k) r.shape[k] = shape[k];
  r.flops = fl;
  r.bytes = by;
  g_prof.rec.push_back(r);
  return 0;
}

int conv_run(Ctx& c, ConvParams& p) {
  if (c.dry) return 0;
  const bool prof = g_prof.on;
  if (prof) ST_CHECK(prof_begin(c));
  p.stats_slots = p.stats ? c.slots : 1;
  p.stats_slot_bs = (long long)c.B * p.stats_ld * ST_W;
  int r = st_conv1d(p, c.cdtype, c.s);
  if (r) return r;
  // statistics slots are summed by the consumers' prologues (adain_coeffs): no fold launch
  if (prof) {
    // algorithmic work: a (transposed) conv is 2 * rows * N * Cin * taps flops on its GEMM view;
    // bytes = one read of the input, residual and running sum, one write of the output (none for a
    // statistics-only launch, y == null)
    const double fl = 2.0 * p.B * (double)p.Lq * p.N * p.Cin * p.KS;
    const double outs = (p.y ? 1 : 0) + (p.res ? 1 : 0) + (p.accb ? 1 : 0);
    double elems = (double)p.B * ((double)p.Lin * p.Cin + (double)p.Lout * p.Cout * outs);
    const double by = elems * c.esz + (p.y_f32 ? (double)p.B * p.Lout * p.Cout * (4.0 - c.esz) : 0.0);
    const int flags = (p.res ? 1 : 0) | (p.accb ? 2 : 0) | (st_conv1d_engine(p, c.cdtype) << 4);
    ST_CHECK(prof_end(c, {p.B, p.Lq, p.N, p.Cin, p.KS, p.dil, p.Lout, flags}, fl, by));
  }
  return 0;
}

// front-end buffers (hifigan.py:458-472); X0 = decode.3's output [B][2T][512].  H1, SC, POOL are adain_blk's
// temporaries (the F0/N stacks fill those three alone)
struct FrontBufs {
  Buf ENC, CAT[2], H1, SC, POOL, X0;
  int ld_enc = 0, ld_cat = 0;
};

// AdainResBlk1d forward (hifigan.py:390-403).  x frames (ld, L); output into y at channel c0.
int adain_blk(Ctx& c, const AdainBlk& k, const Buf& x, int xc0, const double* st_x, int st_x_ld, const Buf& y,
              int yc0, double* st_y, int st_y_ld, const FrontBufs& f) {
  const int L = x.L, Lr = k.up ? 2 * L : L;
  const float slope = 0.2f;
  // shortcut: conv1x1 at the input rate (nearest x2 commutes with a 1x1 conv)
  const Buf sc = f.SC.view(L, k.cout);
  if (k.learned) {
    ConvParams p = conv_base(c, k.sc, x, xc0);
    p.Lq = L;
    conv_out(p, c, sc, 0, L);
    RUN(conv_run(c, p));
  }
  // residual: norm1 -> lrelu -> [pool] -> conv1
  const Buf h1 = f.H1.view(Lr, k.cout);
  double* st_h1 = c.stat(k.cout);
  {
    ConvParams p;
    if (k.up) {
      const Buf pool = f.POOL.view(Lr, rup8(k.cin));
      Prologue pr = pro_adain(c, k.n1, st_x, st_x_ld, L, PRO_LRELU, -1, slope);
      RUN(st_pool_dw(x.at(xc0, c.esz), x.bs, x.ld, c.B, L, k.cin, c.aux_f(k.pool_off), c.P(k.pool_b), pr, pool.p,
                     pool.bs, pool.ld, c.dtype, c.s));
      p = conv_base(c, k.conv1, pool, 0);
    } else {
      p = conv_base(c, k.conv1, x, xc0);
      p.pro = pro_adain(c, k.n1, st_x, st_x_ld, L, PRO_LRELU, -1, slope);
    }
    p.pad = 1;
    p.Lq = Lr;
    conv_out(p, c, h1, 0, Lr);
    conv_stats(p, st_h1, k.cout);
    RUN(conv_run(c, p));
  }
  // norm2 -> lrelu -> conv2, + shortcut, / sqrt(2)
  {
    ConvParams p = conv_base(c, k.conv2, h1, 0);
    p.pro = pro_adain(c, k.n2, st_h1, k.cout, Lr, PRO_LRELU, -1, slope);
    p.pad = 1;
    p.Lq = Lr;
    conv_out(p, c, y, yc0, Lr);
    if (k.learned) conv_res(p, c, sc);
    else conv_res(p, c, x, xc0);
    p.res_shift = k.up ? 1 : 0;
    p.out_scale = (float)(1.0 / sqrt(2.0));
    conv_stats(p, st_y, st_y_ld);
    RUN(conv_run(c, p));
  }
  return 0;
}

enum ResOut { RO_PLAIN = 0, RO_ACC_FIRST, RO_ACC_MID, RO_ACC_LAST };

// AdaINResBlock1 forward (hifigan.py:65-74).  Input X (stats st_x); temps R, XT; the final
// iteration writes R (RO_PLAIN) or accumulates into ACC (resblock average, hifigan.py:336-342).
int resblock1(Ctx& c, const ResBlock1& rb, const Buf& X, const double* st_x, Buf& R, Buf& XT, int ro, Buf* ACC,
              int nk) {
  const int L = X.L, C = rb.C;
  const Buf* xc = &X;
  const double* st_c = st_x;
  for (int d = 0; d < 3; ++d) {
    double* st_xt = c.stat(C);
    {
      ConvParams p = conv_base(c, rb.c1[d], *xc, 0);
      p.pro = pro_adain(c, rb.a1[d], st_c, C, L, PRO_SNAKE, rb.al1[d], 0.f);
      p.dil = rb.dil[d];
      p.pad = rb.dil[d] * (rb.K - 1) / 2;
      p.Lq = L;
      conv_out(p, c, XT, 0, L);
      conv_stats(p, st_xt, C);
      RUN(conv_run(c, p));
    }
    {
      ConvParams p = conv_base(c, rb.c2[d], XT, 0);
      p.pro = pro_adain(c, rb.a2[d], st_xt, C, L, PRO_SNAKE, rb.al2[d], 0.f);
      p.pad = (rb.K - 1) / 2;
      p.Lq = L;
      conv_res(p, c, *xc);
      const bool final = d == 2;
      if (final && ro != RO_PLAIN) {
        conv_out(p, c, *ACC, 0, L);
        if (ro != RO_ACC_FIRST) {
          conv_acc(p, *ACC);
          if (ro == RO_ACC_LAST) p.acc_div = (float)nk;
        }
      } else {
        conv_out(p, c, R, 0, L);
        if (!final) {
          double* st_r = c.stat(C);
          conv_stats(p, st_r, C);
          st_c = st_r;
        }
      }
      RUN(conv_run(c, p));
    }
    xc = &R;
  }
  return 0;
}

// --------------------------------------------------------------------- decoder forward
struct DecIO {
  const float *asr, *f0, *n, *s, *noise;
  unsigned long long seed;
  long long utt;
  int T;
  float* out;
};

FrontBufs alloc_front(Ctx& c, int T) {
  Model& m = *c.m;
  FrontBufs f;
  f.ld_enc = rup8(m.dim_in + 2);
  f.ld_cat = rup8(1024 + 2 + 64);
  f.ENC = c.frames(T, f.ld_enc);
  f.CAT[0] = c.frames(T, f.ld_cat);
  f.CAT[1] = c.frames(T, f.ld_cat);
  f.H1 = c.frames(2 * T, 1024);
  f.SC = c.frames(T, 1024);
  f.POOL = c.frames(2 * T, f.ld_cat);
  f.X0 = c.frames(2 * T, 512);
  c.H = reinterpret_cast<float*>(c.alloc((size_t)c.B * m.Htot * 4));
  c.alloc_splitk((long long)T * 1024);  // the largest front-end conv output: T x 1024 = 2T x 512
  return f;
}

// the style projections of every AdaIN layer, then the front-end (hifigan.py:458-472 ==
// istftnet.py:704-718 == vocos.py:404-419, eval branch) into f.X0
int run_front(Ctx& c, const DecIO& io, FrontBufs& f) {
  Model& m = *c.m;
  const int B = c.B, T = io.T, n = 2 * T;
  const int ld_enc = f.ld_enc, ld_cat = f.ld_cat;
  Buf &ENC = f.ENC, *CAT = f.CAT;
  if (!c.h_ready) RUN(st_linear(io.s, B, m.style_dim, c.aux_f(m.wt_off), c.aux_f(m.bcat_off), m.Htot, c.H, c.s));
  double* S_enc = c.stat(ld_enc);
  RUN(st_ncl_to_frames(io.asr, B, m.dim_in, T, ENC.p, ld_enc, 0, ENC.bs, S_enc, ld_enc, c.dtype, c.s));
  double* S_cat[4];
  for (int k = 0; k < 4; ++k) S_cat[k] = c.stat(ld_cat);
  for (int w = 0; w < 2; ++w) {
    const Small& sm = w == 0 ? m.F0_conv : m.N_conv;
    const float* src = w == 0 ? io.f0 : io.n;
    SmallConvDst d[3];
    d[0] = {ENC.p, ENC.bs, ld_enc, m.dim_in + w, S_enc, ld_enc};
    d[1] = {CAT[0].p, CAT[0].bs, ld_cat, 1024 + 64 + w, S_cat[0], ld_cat};
    d[2] = {CAT[1].p, CAT[1].bs, ld_cat, 1024 + 64 + w, nullptr, 0};
    RUN(st_conv_cin1(src, n, n, B, c.aux_f(sm.off), c.P(sm.bias), 1, 3, 2, 1, T, d, 3, c.dtype, c.s));
  }
  for (int w = 0; w < 2; ++w) {  // asr_res (hifigan.py:438-440, 464) into both concat buffers
    ConvParams p = conv_base(c, m.asr_res, ENC, 0);
    p.Lq = T;
    conv_out(p, c, CAT[w], 1024, T);
    if (w == 0) conv_stats(p, S_cat[0] + 1024 * ST_W, ld_cat);
    RUN(conv_run(c, p));
    // these statistics are copied slot 0 only into the other concat buffers' stats below: fold
    if (w == 0 && c.slots > 1)
      RUN(st_stats_fold(p.stats, c.B, p.stats_ld, p.Cout, c.slots, (long long)c.B * p.stats_ld * ST_W, c.s));
  }
  if (!c.dry) {  // the constant concat channels share their statistics across the 4 blocks
    for (int k = 1; k < 4; ++k)
      ST_CHECK_HIP(hipMemcpy2DAsync(S_cat[k] + 1024 * ST_W, (size_t)ld_cat * ST_W * 8, S_cat[0] + 1024 * ST_W,
                                    (size_t)ld_cat * ST_W * 8, 66 * ST_W * 8, B, hipMemcpyDeviceToDevice, c.s));
  }
  ST_CHECK(adain_blk(c, m.encode, ENC, 0, S_enc, ld_enc, CAT[0], 0, S_cat[0], ld_cat, f));
  ST_CHECK(adain_blk(c, m.decode[0], CAT[0], 0, S_cat[0], ld_cat, CAT[1], 0, S_cat[1], ld_cat, f));
  ST_CHECK(adain_blk(c, m.decode[1], CAT[1], 0, S_cat[1], ld_cat, CAT[0], 0, S_cat[2], ld_cat, f));
  ST_CHECK(adain_blk(c, m.decode[2], CAT[0], 0, S_cat[2], ld_cat, CAT[1], 0, S_cat[3], ld_cat, f));
  ST_CHECK(adain_blk(c, m.decode[3], CAT[1], 0, S_cat[3], ld_cat, f.X0, 0, nullptr, 0, f));
  return 0;
}

// Everything decoder_forward allocates ahead of the statistics (alloc_decoder: identical in dry and real runs), with
// the stage geometry and the side-stream decisions
struct DecBufs {
  FrontBufs fb;
  bool ist = false, br = false, nbr = false;
  int nup = 0, nrb = 0, scale = 1, L = 0;  // L output samples = 2T * scale
  int F = 0, ld_h = 0;                     // istftnet: spectrogram frames, their leading dimension
  std::vector<int> Ls, Cs;                 // stage s: Ls[s] rows of Cs[s] channels (the largest: smax elements)
  long long smax = 0;
  float *PH = nullptr, *HAR = nullptr;
  Buf G[6], GB[8], NB[2];  // stage temporaries: the caller's stream, the resblock side streams, the noise stream
  Buf HFR;                 // S-sample frames of the source for the MFMA noise_convs (largest such stage)
  Buf HARF, POST, NSO[8];
  float *splitk_br[4] = {}, *splitk_nb = nullptr;
  Buf stage(const Buf& g, int s) const { return g.view(Ls[s], Cs[s]); }
};

DecBufs alloc_decoder(Ctx& c, int T) {
  Model& m = *c.m;
  const int B = c.B;
  DecBufs b;
  const bool ist = b.ist = m.kind == STTS_KIND_ISTFTNET;
  const int nup = b.nup = (int)m.rates.size(), nrb = b.nrb = (int)m.rbk.size();
  b.fb = alloc_front(c, T);
  for (int r : m.rates) b.scale *= r;
  if (ist) b.scale *= m.hop;
  b.L = 2 * T * b.scale;
  b.PH = reinterpret_cast<float*>(c.alloc((size_t)B * 9 * 2 * T * 4));
  b.HAR = reinterpret_cast<float*>(c.alloc((size_t)B * b.L * 4));
  // generator stage geometry
  b.Ls.resize(nup);
  b.Cs.resize(nup);
  for (int s = 0, Lc = 2 * T; s < nup; ++s) {
    Lc *= m.rates[s];
    b.Ls[s] = Lc + ((ist && s == nup - 1) ? 1 : 0);
    b.Cs[s] = m.init_ch >> (s + 1);
    b.smax = std::max(b.smax, (long long)b.Ls[s] * b.Cs[s]);
  }
  if (c.cdtype == ST_SPLIT) {  // the fp32 partials of the two-pass C = 64 split resblock convs (ressplit.hip)
    c.splitk_elems = (long long)B * b.smax;
    c.splitk = reinterpret_cast<float*>(c.alloc((size_t)B * b.smax * 4));
  }
  c.temps(b.G, 6, b.smax);
  // small batches (STTS_OPT_BRANCHES, default B <= 8): a stage's resblocks 1 .. nrb-1 run beside resblock 0 on side
  // streams, each with its own temporaries and output, averaged afterwards (st_branch_avg) instead of through the
  // running sum: at B = 1 one resblock conv fills 64-512 workgroups, so three side by side fill the chip better.
  // Not in the split accuracy mode (its two-pass C = 64 convs share the one fp32 partial buffer)
  b.br = g_opt_branches > 0 && B <= g_opt_branches && nrb > 1 && nrb <= 5 && c.cdtype != ST_SPLIT;
  if (b.br) {
    c.temps(b.GB, 2 * (nrb - 1), b.smax);
    // each side-stream resblock also gets its own split-K scratch (the short-conv engine's fp32 partials,
    // st_pw_split): branches that shared c.splitk would write and reduce their partial sums in the same memory
    if (c.splitk_elems)
      for (int j = 0; j + 1 < nrb; ++j) b.splitk_br[j] = reinterpret_cast<float*>(c.alloc((size_t)c.splitk_elems * 4));
  }
  int rows = 0;
  for (int s = 0; s < nup; ++s)
    if (!ist && m.nc_mm[s].reframe) rows = std::max(rows, b.Ls[s] + 1);
  if (rows) b.HFR = c.frames(rows, 32);
  if (ist) {
    b.F = b.L / m.hop + 1;
    b.ld_h = rup8(m.n_fft + 2);
    b.HARF = c.frames(b.F, b.ld_h);
    b.POST = c.frames(b.F, b.ld_h);
  }
  // small batches (with the resblock branches): every stage's noise branch (noise_convs -> noise_res, which reads
  // only the harmonic source) runs on a third side stream from the start, beside the front-end and the stages;
  // stage s's ups conv waits for its output (per-stage buffers NSO)
  b.nbr = (b.br || (g_opt_nbranch > 0 && B <= g_opt_nbranch && c.cdtype != ST_SPLIT)) && nup <= 8;
  if (b.nbr) {
    for (int s = 0; s < nup; ++s) b.NSO[s] = c.frames(b.Ls[s], b.Cs[s]);
    c.temps(b.NB, 2, b.smax);
    // the side stream's own split-K scratch (the front-end's short convs use c.splitk)
    if (c.splitk_elems) b.splitk_nb = reinterpret_cast<float*>(c.alloc((size_t)c.splitk_elems * 4));
  }
  return b;
}

// noise branch of stage s (hifigan.py:330-331): noise_convs -> NS -> noise_res -> R
int noise_branch(Ctx& c, const DecBufs& b, int s, const Buf& NS, Buf R, Buf XT) {
  Model& m = *c.m;
  const int B = c.B, L = b.L, C = b.Cs[s], Ls_ = b.Ls[s];
  const bool last = s + 1 == b.nup;
  double* S_ns = c.stat(C);
  int sf = 1;
  for (int j = s + 1; j < b.nup; ++j) sf *= m.rates[j];
  if (!b.ist && m.nc_mm[s].reframe) {  // noise_convs[s] on the MFMA engine over S-sample frames
    const int S = m.nc_mm[s].reframe;
    const Buf hf = b.HFR.view(Ls_ + 1, 32);
    RUN(st_har_frames(b.HAR, B, L, S, (S + 1) / 2, Ls_ + 1, 32, hf.p, c.dtype, c.s));
    ConvParams p = conv_base(c, m.nc_mm[s], hf, 0);
    p.Lq = Ls_;
    conv_out(p, c, NS, 0, Ls_);
    conv_stats(p, S_ns, C);
    RUN(conv_run(c, p));
  } else if (!b.ist) {
    const int K = last ? 1 : 2 * sf, st = last ? 1 : sf, pd = last ? 0 : (sf + 1) / 2;
    if ((K == 1 || K == 4 || K == 12) && C % 8 == 0 && 256 % (C / 8) == 0) {
      RUN(st_noise_conv(b.HAR, B, L, c.P(m.nc_w[s]), c.P(m.nc_b[s]), C, K, st, pd, Ls_, NS.p, S_ns, c.dtype, c.s));
    } else {
      SmallConvDst d = {NS.p, NS.bs, C, 0, S_ns, C};
      RUN(st_conv_cin1(b.HAR, L, L, B, c.P(m.nc_w[s]), c.P(m.nc_b[s]), C, K, st, pd, Ls_, &d, 1, c.dtype, c.s));
    }
  } else {
    ConvParams p = conv_base(c, m.nc_conv[s], b.HARF, 0);
    if (!last) {
      p.stride = sf;
      p.pad = (sf + 1) / 2;
    }
    p.Lq = Ls_;
    conv_out(p, c, NS, 0, Ls_);
    conv_stats(p, S_ns, C);
    RUN(conv_run(c, p));
  }
  return resblock1(c, m.noise_res[s], NS, S_ns, R, XT, RO_PLAIN, nullptr, 0);
}
// ups of stage s: Snake(alpha_s) / LReLU(0.1) prologue, polyphase ConvTranspose1d of xin into X, + x_source XS in the
// epilogue (hifigan.py:327-332), statistics into S_x
int ups_conv(Ctx& c, const DecBufs& b, int s, const Buf& xin, const Buf& XS, const Buf& X, double* S_x) {
  Model& m = *c.m;
  const WConv& w = m.ups[s];
  const int u = m.rates[s];
  ConvParams p = conv_base(c, w, xin, 0);
  p.Cin = xin.ld;
  if (!b.ist) {
    p.pro.mode = PRO_SNAKE;
    p.pro.alpha = c.P(m.alphas[s]);
  } else {
    p.pro.mode = PRO_LRELU;
    p.pro.slope = 0.1f;
  }
  const int padT = b.ist ? (w.K - u) / 2 : u / 2 + u % 2;
  const int Lout = xin.L * u;
  p.pad = w.taps() - 1;
  p.Lq = (Lout - 1 + padT) / u + 1;
  p.up = u;
  p.opad = padT;
  conv_out(p, c, X, 0, Lout);
  if (b.ist && s + 1 == b.nup) {
    p.y_row_off = 1;
    p.reflect_front = 1;
  }
  conv_res(p, c, XS);
  conv_stats(p, S_x, b.Cs[s]);
  return conv_run(c, p);
}

// the resblocks of stage s over X (statistics S_x) and their average into ACC (hifigan.py:336-342)
int stage_resblocks(Ctx& c, const DecBufs& b, SideStreams::Forks& fk, int s, const Buf& X, const double* S_x, Buf R,
                    Buf XT, Buf ACC) {
  const int nrb = b.nrb;
  const ResBlock1* rb = &c.m->resblocks[(size_t)s * nrb];
  if (!b.br) {  // one stream: the running sum, through the epilogue of each resblock's last conv
    for (int j = 0; j < nrb; ++j) {
      const int ro = j == 0 ? RO_ACC_FIRST : (j == nrb - 1 ? RO_ACC_LAST : RO_ACC_MID);
      ST_CHECK(resblock1(c, rb[j], X, S_x, R, XT, ro, &ACC, nrb));
    }
    return 0;
  }
  // fork: side stream j - 1 runs resblock j after everything queued so far on the caller's stream
  if (!c.dry) ST_CHECK(fk.fork(0, nrb - 1));
  ST_CHECK(resblock1(c, rb[0], X, S_x, R, XT, RO_ACC_FIRST, &ACC, nrb));
  const void* rs[4];
  for (int j = 1; j < nrb; ++j) {
    Buf Rj = b.stage(b.GB[2 * (j - 1)], s), XTj = b.stage(b.GB[2 * (j - 1) + 1], s);
    ST_CHECK(on_side(c, j - 1, b.splitk_br[j - 1],
                     [&] { return resblock1(c, rb[j], X, S_x, Rj, XTj, RO_PLAIN, nullptr, 0); }));
    rs[j - 1] = Rj.p;
  }
  // join, then ACC = ((ACC + R_1) + R_2 ...) / nrb
  if (!c.dry)
    for (int j = 0; j + 1 < nrb; ++j) ST_CHECK(fk.join(j));
  RUN(st_branch_avg(ACC.p, rs, nrb - 1, (float)nrb, (long long)c.B * X.L * X.ld, c.dtype, c.s));
  return 0;
}

int output_head(Ctx& c, const DecBufs& b, const DecIO& io, const Buf& xin) {
  Model& m = *c.m;
  ConvParams p = conv_base(c, m.conv_post, xin, 0);
  p.pad = 3;
  p.Lq = xin.L;
  if (!b.ist) {  // Snake(alpha_last) -> conv_post -> tanh  (hifigan.py:343-345)
    p.pro.mode = PRO_SNAKE;
    p.pro.alpha = c.P(m.alphas[b.nup]);
    p.y = io.out;
    p.y_bs = xin.L;
    p.y_ld = 1;
    p.y_f32 = 1;
    p.Lout = xin.L;
    p.epi_tanh = 1;
    return conv_run(c, p);
  }
  // LReLU(0.01) -> conv_post -> exp/sin -> CustomSTFT.inverse (istftnet.py:569-573)
  p.pro.mode = PRO_LRELU;
  p.pro.slope = 0.01f;
  conv_out(p, c, b.POST, 0, xin.L);
  RUN(conv_run(c, p));
  RUN(st_istft(b.POST.p, c.B, b.F, b.ld_h, m.n_fft, m.hop, c.P(m.stft_br), c.P(m.stft_bi), io.out, b.L, c.dtype,
               c.s));
  return 0;
}

// Decoder.forward (hifigan.py:446-475 / istftnet.py:692-721); after the front-end it reads as Generator.forward
// (hifigan.py:321-347 / istftnet.py:542-575)
int decoder_forward(Ctx& c, const DecIO& io) {
  Model& m = *c.m;
  const int B = c.B, n = 2 * io.T;
  enum { NOISE = SideStreams::NOISE };
  DecBufs b = alloc_decoder(c, io.T);
  c.stats_begin = c.stats_off = c.off;  // stats region follows; its size is known after the dry run
  // ---------------- harmonic source (hifigan.py:323-326 / istftnet.py:544-550)
  RUN(st_sine_phase(io.f0, B, n, b.scale, b.PH, c.s));
  RUN(st_sine_source(io.f0, b.PH, B, n, b.scale, c.P(m.l_lin_w), c.P(m.l_lin_b), io.noise, io.seed, io.utt, b.HAR,
                     c.s));
  if (b.ist) {
    RUN(st_stft(b.HAR, B, b.L, m.n_fft, m.hop, c.P(m.stft_fr), c.P(m.stft_fi), b.HARF.p, b.ld_h, c.dtype, c.s));
  }
  std::unique_lock<std::mutex> branch_lock;
  if ((b.br || b.nbr) && !c.dry) branch_lock = std::unique_lock<std::mutex>(m.branch_mu);
  SideStreams::Forks fk{m.side, c.s};
  if (b.nbr) {
    // the noise branches' AdaIN layers read H (the style projections): computed before the fork
    RUN(st_linear(io.s, B, m.style_dim, c.aux_f(m.wt_off), c.aux_f(m.bcat_off), m.Htot, c.H, c.s));
    c.h_ready = true;
    if (!c.dry) ST_CHECK(fk.fork(NOISE));
    for (int s = 0; s < b.nup; ++s) {
      ST_CHECK(on_side(c, NOISE, b.splitk_nb, [&] {
        return noise_branch(c, b, s, b.stage(b.NB[0], s), b.NSO[s], b.stage(b.NB[1], s));
      }));
      if (!c.dry) ST_CHECK(fk.mark(NOISE, s));  // stage s waits for this
    }
  }
  // ---------------- style projections + front-end (hifigan.py:458-472)
  ST_CHECK(run_front(c, io, b.fb));
  // ---------------- generator stages
  Buf xin = b.fb.X0;
  for (int s = 0; s < b.nup; ++s) {
    Buf R = b.stage(b.G[1], s), XT = b.stage(b.G[2], s), X = b.stage(b.G[3], s), ACC = b.stage(b.G[4 + s % 2], s);
    Buf XS = R;  // x_source: the noise branch's output
    if (b.nbr) {  // this stage's noise branch ran on the side stream
      XS = b.NSO[s];
      if (!c.dry) ST_CHECK(fk.wait(NOISE, s));
    } else {
      ST_CHECK(noise_branch(c, b, s, b.stage(b.G[0], s), R, XT));
    }
    double* S_x = c.stat(b.Cs[s]);
    ST_CHECK(ups_conv(c, b, s, xin, XS, X, S_x));
    ST_CHECK(stage_resblocks(c, b, fk, s, X, S_x, R, XT, ACC));
    xin = ACC;
  }
  return output_head(c, b, io, xin);
}

// --------------------------------------------------------------------- Vocos forward
// Decoder.forward (Modules/vocos.py:392-421, eval): the front-end, then Generator.forward (:157-162):
// per ConvNeXtBlock (:56-69) dwconv (+ InstanceNorm statistics) -> [AdaIN prologue] pwconv1 [GELU
// epilogue] -> pwconv2 with gamma folded [+ residual epilogue]; final LayerNorm; ISTFTHead.out, and
// the exp / clip / cos / sin + irfft + window + overlap-add of ISTFTHead / ISTFT (:271-296, :190-232).
int vocos_forward(Ctx& c, const DecIO& io) {
  Model& m = *c.m;
  const int B = c.B, T = io.T, L = 2 * T, d = m.dim_in;
  FrontBufs fb = alloc_front(c, T);
  Buf XB = c.frames(L, d), D = c.frames(L, d), HI = c.frames(L, m.vc_inter);
  Buf POST = c.frames(L, m.vhead.Cout);
  float* FR = reinterpret_cast<float*>(c.alloc((size_t)B * L * m.n_fft * 4));
  c.stats_begin = c.stats_off = c.off;
  ST_CHECK(run_front(c, io, fb));
  Buf* x = &fb.X0;
  Buf* y = &XB;
  for (const auto& b : m.cnx) {
    double* S_d = c.stat(d);
    RUN(st_dwconv7(x->p, x->bs, x->ld, B, L, d, c.P(b.dw_w), c.P(b.dw_b), D.p, D.bs, D.ld, S_d, d, c.slots,
                   (long long)B * d * ST_W, c.dtype, c.s));
    {
      ConvParams p = conv_base(c, b.pw1, D, 0);
      p.pro = pro_adain(c, b.norm, S_d, d, L, 0, -1, 0.f);
      p.Lq = L;
      conv_out(p, c, HI, 0, L);
      p.epi_gelu = 1;
      RUN(conv_run(c, p));
    }
    {
      ConvParams p = conv_base(c, b.pw2, HI, 0);
      p.Lq = L;
      conv_out(p, c, *y, 0, L);
      conv_res(p, c, *x);
      RUN(conv_run(c, p));
    }
    std::swap(x, y);
  }
  // final LayerNorm (eps 1e-6) into D, the head Linear into POST
  RUN(st_frame_ln(x->p, x->ld, (long long)B * L, d, 1e-6f, c.P(m.ln_w), c.P(m.ln_b), D.p, D.ld, c.dtype, c.s));
  {
    ConvParams p = conv_base(c, m.vhead, D, 0);
    p.Lq = L;
    conv_out(p, c, POST, 0, L);
    RUN(conv_run(c, p));
  }
  RUN(st_istft_head(POST.p, B, L, POST.ld, m.n_fft, m.hop, c.P(m.vwin), FR, io.out, c.dtype, c.s));
  return 0;
}

// --------------------------------------------------------------------- MPD forward
// DiscriminatorP.forward (discriminators.py:108-129) for every period: reflect pad + 1-d -> 2-d
// view (k_period_frames), 5 convs with LeakyReLU(0.1) fused into the epilogue (the activated
// output is the feature map AND the next conv's input), conv_post.  `out` (fp32) receives, per
// period in order, the 6 feature maps as frames [B*p][L_j][C_j] (the reference's [B, C_j, L_j, p]
// tensors permuted; conv_post's map, C = 1, is also the score before flatten).
int mpd_forward(Ctx& c, const float* wave, int Tn, float* out) {
  Model& m = *c.m;
  const int B0 = c.B;
  const DiscMaps maps = mpd_maps(m, B0, Tn);
  size_t k = 0;  // the map being written
  for (const auto& d : m.mpd) {
    const int p = d.period;
    int L[6];
    mpd_lengths(Tn, p, L);
    c.B = B0 * p;  // the conv batch: every (utterance, column) sequence
    Buf x = c.frames(L[0], 8);
    RUN(st_period_frames(wave, B0, Tn, p, L[0], x.p, c.dtype, c.s));
    for (int j = 0; j < 5; ++j) {
      Buf y = c.frames(L[j + 1], kMpdCh[j + 1]);
      ConvParams q = conv_base(c, d.convs[j], x, 0);
      q.stride = j < 4 ? 3 : 1;
      q.pad = 2;
      q.Lq = L[j + 1];
      conv_out(q, c, y, 0, L[j + 1]);
      q.epi_lrelu = 1;
      q.epi_slope = 0.1f;  // LRELU_SLOPE (discriminators.py:9)
      RUN(conv_run(c, q));
      RUN(st_frames_to_f32(y.p, c.B, L[j + 1], kMpdCh[j + 1], y.ld, out ? out + maps[k].off : nullptr, c.dtype,
                           c.s));
      ++k;
      x = y;
    }
    {
      ConvParams q = conv_base(c, d.post, x, 0);
      q.pad = 1;
      q.Lq = L[5];
      q.y = out ? out + maps[k].off : nullptr;
      q.y_bs = L[5];
      q.y_ld = 1;
      q.y_f32 = 1;
      q.Lout = L[5];
      RUN(conv_run(c, q));
      ++k;
    }
    c.B = B0;
  }
  c.stats_begin = c.stats_off = c.off;  // no statistics: the workspace is the buffers above
  return 0;
}

// --------------------------------------------------------------------- MSD forward
// SpecDiscriminator.forward (discriminators.py:47-63) for every resolution over S signals: |STFT| ->
// 4 Conv2d (3, 9) + LeakyReLU(0.1) [the last three with stride (1, 2)] -> Conv2d (3, 3) + LeakyReLU
// -> out Conv2d (3, 3).  Each (3, kw) Conv2d over the (frames, bins) image runs as a 1-D conv along the
// bins of every frame (batch = S * H sequences) over 3 C time-expanded channels (k_time_expand /
// k_stft_mag write x3[h][w][c * 3 + dh] = y[h + dh - 1][w][c]).  `out` (fp32) receives, per resolution,
// the 5 activated feature maps [S][H][W_j][32] and the out map [S][H][W_5] (the reference's
// [S, C, H, W] tensors permuted).
int msd_forward(Ctx& c, const float* wave, int Tn, float* out) {
  Model& m = *c.m;
  const int S = c.B;
  const DiscMaps maps = msd_maps(m, S, Tn);
  size_t k = 0;  // the map being written
  for (const auto& d : m.msd) {
    const MsdGeom g = msd_geom(d, Tn);
    c.B = S * g.H;  // the conv batch: every (signal, frame) row of bins
    Buf x3 = c.frames(g.W[0], 8);
    if (!c.dry) ST_CHECK_HIP(hipMemsetAsync(x3.p, 0, (size_t)c.B * x3.bs * c.esz, c.s));
    RUN(st_stft_mag_x3(wave, S, Tn, Tn, d.n_fft, d.win, d.hop, x3.p, c.dtype, c.s));
    for (int j = 0; j < 5; ++j) {
      Buf y = c.frames(g.W[j + 1], kMsdCh);
      const WConv& cw = d.convs[j];
      // a folded stride-2 layer reads [W_even / 2][2 x 96] rows of the same memory
      const Buf xin = cw.fold ? x3.view(x3.L / cw.fold, x3.ld * cw.fold) : x3;
      ConvParams q = conv_base(c, cw, xin, 0);
      q.stride = cw.fold ? 1 : ((j >= 1 && j <= 3) ? 2 : 1);
      q.pad = cw.fold ? cw.fpad : (j < 4 ? 4 : 1);
      q.Lq = g.W[j + 1];
      conv_out(q, c, y, 0, g.W[j + 1]);
      q.epi_lrelu = 1;
      q.epi_slope = 0.1f;  // LRELU_SLOPE (discriminators.py:9)
      RUN(conv_run(c, q));
      RUN(st_frames_to_f32(y.p, c.B, g.W[j + 1], kMsdCh, kMsdCh, out ? out + maps[k].off : nullptr, c.dtype, c.s));
      ++k;
      // the next layer's input; a folded (stride-2) next layer reads an even number of rows per sequence
      const int fnext = j + 1 < 5 ? d.convs[j + 1].fold : 0;
      const int We = fnext ? (g.W[j + 1] + fnext - 1) / fnext * fnext : g.W[j + 1];
      x3 = c.frames(We, 3 * kMsdCh);
      RUN(st_time_expand(y.p, S, g.H, g.W[j + 1], kMsdCh, x3.p, c.dtype, c.s, We));
    }
    {  // out: Conv2d(32, 1, 3, 1, 1) straight into the fp32 output
      ConvParams q = conv_base(c, d.out, x3, 0);
      q.pad = 1;
      q.Lq = g.W[5];
      q.y = out ? out + maps[k].off : nullptr;
      q.y_bs = g.W[5];
      q.y_ld = 1;
      q.y_f32 = 1;
      q.Lout = g.W[5];
      RUN(conv_run(c, q));
      ++k;
    }
    c.B = S;
  }
  c.stats_begin = c.stats_off = c.off;  // no statistics: the workspace is the buffers above
  return 0;
}

// --------------------------------------------------------------------- F0/N forward
int f0n_forward(Ctx& c, const float* x, const float* s, int T, float* F0, float* Nout) {
  Model& m = *c.m;
  const int B = c.B, d = m.d_hid;
  Buf XL = c.frames(T, d);
  Buf Y0 = c.frames(T, d), Y1 = c.frames(2 * T, d / 2), Y2 = c.frames(2 * T, d / 2);
  FrontBufs t;
  t.H1 = c.frames(2 * T, d);
  t.SC = c.frames(T, d);
  t.POOL = c.frames(2 * T, rup8(d));
  c.H = reinterpret_cast<float*>(c.alloc((size_t)B * m.Htot * 4));
  c.alloc_splitk((long long)T * d);  // the largest conv output of the stacks: T x d = 2T x d/2
  c.stats_begin = c.stats_off = c.off;
  RUN(st_linear(s, B, m.style_dim, c.aux_f(m.wt_off), c.aux_f(m.bcat_off), m.Htot, c.H, c.s));
  double* S0 = c.stat(d);
  RUN(st_frames_convert(x, B, T, d, d, XL.p, d, S0, d, c.dtype, c.s));
  for (int br = 0; br < 2; ++br) {
    AdainBlk* blk = br == 0 ? m.f0blk : m.nblk;
    double* S1 = c.stat(d);
    double* S2 = c.stat(d / 2);
    ST_CHECK(adain_blk(c, blk[0], XL, 0, S0, d, Y0, 0, S1, d, t));
    ST_CHECK(adain_blk(c, blk[1], Y0, 0, S1, d, Y1, 0, S2, d / 2, t));
    ST_CHECK(adain_blk(c, blk[2], Y1, 0, S2, d / 2, Y2, 0, nullptr, 0, t));
    ConvParams p = conv_base(c, br == 0 ? m.f0_proj : m.n_proj, Y2, 0);
    p.Lq = 2 * T;
    p.y = br == 0 ? F0 : Nout;
    p.y_bs = 2 * T;
    p.y_ld = 1;
    p.y_f32 = 1;
    p.Lout = 2 * T;
    RUN(conv_run(c, p));
  }
  return 0;
}

// --------------------------------------------------------------------- style forward
// An image [H][W] is kept zero-padded and row-flattened: row (h+1)*(W+2) + (w+1) holds pixel
// (h, w).  A 3x3 / pad-1 conv is then the 1-D implicit GEMM with 2-level taps
// (row_off = W+2, dil = 1) over output rows q = h*(W+2) + w, written at offset W+3, with the
// two wrap-around columns per image row forced to 0 (they are the next image's padding).
struct Img {
  Buf b;
  int H = 0, W = 0, C = 0;
};

Img img_alloc(Ctx& c, int H, int W, int C) {
  Img im;
  im.H = H;
  im.W = W;
  im.C = C;
  im.b = c.frames((H + 2) * (W + 2), C);
  return im;
}

int conv3x3(Ctx& c, const WConv& w, const Img& x, const Img& y, int pro_lrelu, const Img* res, float slope = 0.2f,
            float res_scale = 0.70710678118654752440f) {
  ConvParams p = conv_base(c, w, x.b, 0);
  p.KS = 9;
  p.kw = 3;
  p.row_off = x.W + 2;
  p.Lq = x.H * (x.W + 2);
  p.zc_period = x.W + 2;
  p.zc_valid = x.W;
  if (pro_lrelu) {
    p.pro.mode = PRO_LRELU;
    p.pro.slope = slope;
  }
  p.y = y.b.p ? y.b.p + (size_t)(x.W + 3) * y.C * c.esz : nullptr;
  p.y_bs = y.b.bs;
  p.y_ld = y.C;
  p.Lout = p.Lq;
  if (res) {
    p.res = res->b.p ? res->b.p + (size_t)(x.W + 3) * res->C * c.esz : nullptr;
    p.res_bs = res->b.bs;
    p.res_ld = res->C;
    p.out_scale = res_scale;
  }
  return conv_run(c, p);
}

int style_forward(Ctx& c, const float* mel, int T, float* out) {
  Model& m = *c.m;
  const int B = c.B;
  int H = 80, W = T;
  Img M = img_alloc(c, H, W, 8);
  Img A = img_alloc(c, H, W, m.se_conv0.Cout);
  struct BI {
    Img t1, d, scf, scp, y;
  } bi[4];
  {
    int h = H, w = W;
    for (int i = 0; i < 4; ++i) {
      const auto& k = m.se_blk[i];
      const int ho = h / 2, wo = (w + 1) / 2;
      bi[i].t1 = img_alloc(c, h, w, k.cin);
      bi[i].d = img_alloc(c, ho, wo, k.cin);
      if (k.learned) bi[i].scf = img_alloc(c, h, w, k.cout);
      bi[i].scp = img_alloc(c, ho, wo, k.cout);
      bi[i].y = img_alloc(c, ho, wo, k.cout);
      h = ho;
      w = wo;
    }
    if (h < 5 || w < 5) return ST_EINVAL;  // conv 5x5 'valid' needs a 5 x 5 map (T >= 65)
  }
  const Img& X4 = bi[3].y;
  const int Wz = X4.W + 2;
  Buf Z = c.frames(Wz, m.se_dim);
  const size_t style_end = c.off;
  c.stats_begin = c.stats_off = c.off;
  if (!c.dry) ST_CHECK_HIP(hipMemsetAsync(c.ws, 0, style_end, c.s));  // zero image borders
  RUN(st_mel_to_padded(mel, B, H, W, M.b.p, c.dtype, c.s));
  RUN(conv3x3(c, m.se_conv0, M, A, 0, nullptr));
  const Img* x = &A;
  for (int i = 0; i < 4; ++i) {
    const auto& k = m.se_blk[i];
    BI& t = bi[i];
    if (k.learned) {  // shortcut: conv1x1 over every padded row (borders stay 0: no bias)
      ConvParams p = conv_base(c, k.sc, x->b, 0);
      p.Lq = (x->H + 2) * (x->W + 2);
      conv_out(p, c, t.scf.b, 0, p.Lq);
      RUN(conv_run(c, p));
      RUN(st_avgpool_half(t.scf.b.p, B, x->H, x->W, k.cout, t.scp.b.p, c.dtype, c.s));
    } else {
      RUN(st_avgpool_half(x->b.p, B, x->H, x->W, k.cin, t.scp.b.p, c.dtype, c.s));
    }
    RUN(conv3x3(c, k.conv1, *x, t.t1, 1, nullptr));                                     // lrelu -> conv1
    RUN(st_dw_s2(t.t1.b.p, B, x->H, x->W, k.cin, c.P(k.dw_w), c.P(k.dw_b), t.d.b.p, c.dtype, c.s));  // dw s2
    RUN(conv3x3(c, k.conv2, t.d, t.y, 1, &t.scp));                                       // lrelu -> conv2, +sc, /sqrt2
    x = &t.y;
  }
  {  // LeakyReLU -> Conv2d(C, C, 5, 1, 0) over the 5 x W4 map (models.py:137-138)
    ConvParams p = conv_base(c, m.se_last, X4.b, 0);
    p.x = X4.b.p ? X4.b.p + (size_t)(X4.W + 3) * X4.C * c.esz : nullptr;
    p.Lin = (X4.H + 2) * (X4.W + 2) - (X4.W + 3);
    p.KS = 25;
    p.kw = 5;
    p.row_off = X4.W + 2;
    p.Lq = Wz;
    p.zc_period = Wz;
    p.zc_valid = X4.W - 4;
    p.pro.mode = PRO_LRELU;
    p.pro.slope = 0.2f;
    conv_out(p, c, Z, 0, Wz);
    RUN(conv_run(c, p));
  }
  RUN(st_gap_linear(Z.p, B, Wz, X4.W - 4, m.se_dim, c.P(m.se_lin_w), c.P(m.se_lin_b), m.style_dim, out, c.dtype,
                    c.s));
  return 0;
}

// --------------------------------------------------------------------- pitch extractor forward
// JDCNet.forward (Modules/JDC/model.py:102-137), eval mode.  The reference transposes the mel to (T frames x 80
// bins) and pools the bins only, so the image is laid out H = T, W = bins: its Conv2d weights are conv3x3's taps as
// they lie, MaxPool2d((1, p)) joins p adjacent rows of the flattened image, and every frame stays one image row up
// to the [B][T][512] BiLSTM input.  err_off (may be null) receives the workspace offset of the BiLSTM error word.
int pitch_forward(Ctx& c, const float* mel, int T, float* f0, float* gan, float* pool, size_t* err_off) {
  Model& m = *c.m;
  const int B = c.B, H = T;
  Img M = img_alloc(c, H, kPitchBins, 8);
  Img A = img_alloc(c, H, kPitchBins, 64);
  Img X = img_alloc(c, H, kPitchBins, 64);
  struct BI {
    Img p, t, sc, y;
  } bi[3];
  int w = kPitchBins;
  for (int i = 0; i < 3; ++i) {
    const auto& k = m.pe_blk[i];
    w /= 2;
    bi[i].p = img_alloc(c, H, w, k.cin);
    bi[i].t = img_alloc(c, H, w, k.cout);
    bi[i].sc = img_alloc(c, H, w, k.cout);
    bi[i].y = img_alloc(c, H, w, k.cout);
  }
  const size_t img_end = c.off;
  const int F = kPitchCh[3] * (w / 4);  // 512 BiLSTM input features: channel c (w / 4) + bin
  float* SEQ = reinterpret_cast<float*>(c.alloc((size_t)B * T * F * 4));
  float* Y = reinterpret_cast<float*>(c.alloc((size_t)B * T * 2 * kPitchH * 4));
  const long long lstm_bytes = stts_bilstm_workspace_bytes(B, T, kPitchH);
  if (err_off) *err_off = c.off + (size_t)stts_bilstm_error_offset(B, T, kPitchH);
  char* LW = c.alloc((size_t)lstm_bytes);
  c.stats_begin = c.stats_off = c.off;
  // zero borders of the images the convs write (and the unused channels of M)
  if (!c.dry) ST_CHECK_HIP(hipMemsetAsync(c.ws, 0, img_end, c.s));
  RUN(st_mel_to_padded_t(mel, B, kPitchBins, T, M.b.p, c.dtype, c.s));
  RUN(conv3x3(c, m.pe_c0, M, A, 0, nullptr));                    // conv -> BN (folded)
  RUN(conv3x3(c, m.pe_c1, A, X, 1, nullptr, kPitchSlope));       // LReLU -> conv
  const Img* x = &X;
  for (int i = 0; i < 3; ++i) {
    const auto& k = m.pe_blk[i];
    BI& t = bi[i];
    RUN(st_bn_lrelu_maxpool(x->b.p, B, H, x->W, k.cin, c.aux_f(k.pre.off), kPitchSlope, 2, t.p.b.p, nullptr, nullptr,
                            nullptr, c.dtype, c.s));            // pre_conv
    {  // conv1by1 over every padded row of the pooled map (borders stay 0: no bias)
      ConvParams p = conv_base(c, k.sc, t.p.b, 0);
      p.Lq = (H + 2) * (t.p.W + 2);
      conv_out(p, c, t.sc.b, 0, p.Lq);
      RUN(conv_run(c, p));
    }
    RUN(conv3x3(c, k.c1, t.p, t.t, 0, nullptr));                            // conv -> BN (folded)
    RUN(conv3x3(c, k.c2, t.t, t.y, 1, &t.sc, kPitchSlope, 1.0f));           // LReLU -> conv, + shortcut
    x = &t.y;
  }
  RUN(st_bn_lrelu_maxpool(x->b.p, B, H, x->W, kPitchCh[3], c.aux_f(m.pe_pool.off), kPitchSlope, 4, nullptr, SEQ, gan,
                          pool, c.dtype, c.s));                  // pool_block
  if (!c.dry) {
    const float* lp[8];
    for (int k = 0; k < 8; ++k) lp[k] = c.P(m.pe_lstm[k]);
    ST_CHECK(st_bilstm_fwd(SEQ, (long long)T * F, F, 1, B, T, F, nullptr, lp, kPitchH, Y, nullptr, nullptr, LW,
                           lstm_bytes, 0, c.s));
  }
  RUN(st_linear_abs(Y, (long long)B * T, 2 * kPitchH, c.P(m.pe_cls_w), c.P(m.pe_cls_b), m.pe_nclass, f0, c.s));
  return 0;
}

// --------------------------------------------------------------------- text aligner forward
// ASRCNN.forward (Modules/ASR/models.py:37-48), eval mode.  The CNN sees the zero-padded batch as it is (GroupNorm
// statistics over all L frames); only the attention reads pad_mask.  Everything the recurrence does not feed back is
// a product outside it: the embedded tokens through W_ih[:, :E] (+ both biases), memory_layer(memory), and after the
// loop project_to_hidden and project_to_n_symbols over the stored [h; context] rows.
struct AlignIO {
  const float* mel;
  const unsigned char *pad_mask, *unk_mask;
  const int* tokens;
  int T, Tt;  // Tt = 0: no tokens, the CNN outputs alone
  float *ctc, *s2s, *attn, *feature;
};
int aligner_forward(Ctx& c, const AlignIO& io) {
  Model& m = *c.m;
  if (c.dtype != ST_FP32) return ST_EDTYPE;  // fp32 storage: STTS_FP32 and STTS_SPLIT (the dtype is the convs')
  const int B = c.B, T = io.T, L = (T + 1) / 2, H = kAlHid, D = kAlDec, E = m.al_emb, steps = io.Tt + 1;
  if (L > ST_ALIGNER_MAX_L) return ST_EINVAL;
  const long long rows = (long long)B * L, srows = (long long)B * steps;
  auto f32 = [&](long long n) { return reinterpret_cast<float*>(c.alloc((size_t)n * 4)); };
  const Buf M = c.frames(T, 64), X = c.frames(L, H), Y = c.frames(L, H), R = c.frames(L, H), F = c.frames(L, D);
  float* C1 = f32(rows * H);
  float *EMB = nullptr, *GIN = nullptr, *PM = nullptr, *HC = nullptr, *HID = nullptr;
  if (io.Tt > 0) {
    EMB = f32(srows * E);
    GIN = f32(srows * 4 * D);
    PM = f32(rows * D);
    HC = f32(srows * 2 * D);
    HID = f32(srows * D);
  }
  c.stats_begin = c.stats_off = c.off;  // (no statistics region: nothing of the workspace needs clearing)
  float* x = reinterpret_cast<float*>(X.p);
  RUN(st_mfcc_frames(io.mel, c.P(m.al_dct), B, kAlMel, T, kAlMfcc, M.ld, reinterpret_cast<float*>(M.p), c.s));
  {
    ConvParams p = conv_base(c, m.al_init, M, 0);
    p.stride = 2;
    p.pad = 3;
    p.Lq = L;
    conv_out(p, c, X, 0, L);
    RUN(conv_run(c, p));
  }
  for (const auto& l : m.al_layers) {
    for (const auto& b : l.blk) {
      ConvParams p = conv_base(c, b.c1, X, 0);
      p.dil = p.pad = b.dil;
      p.Lq = L;
      conv_out(p, c, Y, 0, L);
      RUN(conv_run(c, p));
      float* y = reinterpret_cast<float*>(Y.p);
      RUN(st_groupnorm(y, B, L, H, H, 8, 1, c.P(b.gn_w), c.P(b.gn_b), 1e-5f, y, c.s));  // ReLU -> GroupNorm(8)
      ConvParams q = conv_base(c, b.c2, Y, 0);
      q.pad = 1;
      q.Lq = L;
      conv_out(q, c, R, 0, L);
      q.epi_lrelu = 1;  // ReLU, then + the block's input (the engines' epilogue adds a residual before activating)
      q.epi_slope = 0.f;
      RUN(conv_run(c, q));
      RUN(st_add(x, reinterpret_cast<const float*>(R.p), rows * H, c.s));
    }
    RUN(st_groupnorm(x, B, L, H, H, 1, 0, c.P(l.gn_w), c.P(l.gn_b), 1e-5f, x, c.s));
  }
  {
    ConvParams p = conv_base(c, m.al_proj, X, 0);
    p.Lq = L;
    conv_out(p, c, F, 0, L);
    RUN(conv_run(c, p));
  }
  const float* mem = reinterpret_cast<const float*>(F.p);  // [B][L][128]: x.transpose(1, 2), the attention's memory
  if (io.feature) RUN(st_frames_to_ncl(mem, B, L, D, io.feature, c.s));
  if (io.ctc) {
    RUN(st_gemm_nt(mem, rows, D, D, c.P(m.al_ctc_w[0]), H, D, c.P(m.al_ctc_b[0]), nullptr, 1, C1, H, c.s));
    RUN(st_gemm_nt(C1, rows, H, H, c.P(m.al_ctc_w[1]), m.al_ntok, H, c.P(m.al_ctc_b[1]), nullptr, 0, io.ctc, m.al_ntok,
                   c.s));
  }
  if (io.Tt <= 0) return 0;
  RUN(st_s2s_embed(io.tokens, io.unk_mask, B, io.Tt, E, m.al_ntok, c.P(m.al_embw), EMB, c.s));
  RUN(st_gemm_nt(EMB, srows, E, E, c.P(m.al_wih), 4 * D, E + D, c.P(m.al_bih), c.P(m.al_bhh), 0, GIN, 4 * D, c.s));
  RUN(st_gemm_nt(mem, rows, D, D, c.P(m.al_memory), D, D, nullptr, nullptr, 0, PM, D, c.s));
  RUN(st_s2s_decode(GIN, c.aux_f(m.al_wc_t), c.aux_f(m.al_wq_t), c.aux_f(m.al_wloc_t), c.P(m.al_dense), c.P(m.al_v), mem,
                    PM, io.pad_mask, B, L, steps, io.attn, HC, c.s));
  if (io.s2s) {
    RUN(st_gemm_nt(HC, srows, 2 * D, 2 * D, c.P(m.al_ph_w), D, 2 * D, c.P(m.al_ph_b), nullptr, 2, HID, D, c.s));
    RUN(st_gemm_nt(HID, srows, D, D, c.P(m.al_pns_w), m.al_ntok, D, c.P(m.al_pns_b), nullptr, 0, io.s2s, m.al_ntok,
                   c.s));
  }
  return 0;
}

// --------------------------------------------------------------------- packing
int pack_model(Model& m, int dt, char* base, hipStream_t s) {
  char* aux = base + m.aux_off[dt];
  float* scratch = reinterpret_cast<float*>(base + m.scratch_off[dt]);
  for (auto* bn : m.bns)
    ST_CHECK(st_bn_affine(m.P[bn->w], m.P[bn->b], m.P[bn->mean], m.P[bn->var], bn->C, 1e-5f,
                          reinterpret_cast<float*>(aux + bn->off), s));
  for (auto* c : m.convs) {
    const float* v = m.P[c->v];
    const float* src = v;
    if (c->g >= 0) {
      const int rows = c->transposed ? c->Cin : c->Cout;
      const long long inner = (long long)c->Cin * c->Cout * c->K / rows;
      ST_CHECK(st_wn_fold(v, m.P[c->g], rows, (int)inner, scratch, s));
      src = scratch;
    } else if (c->reframe) {
      ST_CHECK(st_reframe_w(v, c->Cout, c->reframe, scratch, s));
      src = scratch;
    } else if (c->bn) {
      ST_CHECK(st_scale_rows(v, reinterpret_cast<const float*>(aux + c->bn->off), c->Cout, (long long)c->Cin * c->K,
                             c->Cout, scratch, s));
      src = scratch;
    } else if (c->rs >= 0 || c->src_rows) {
      const int rows = c->src_rows ? c->src_rows : c->Cout;
      ST_CHECK(st_scale_rows(v, c->rs >= 0 ? m.P[c->rs] : nullptr, rows, (long long)c->Cin * c->K, c->Cout, scratch, s));
      src = scratch;
    }
    if (c->aux_bias)
      ST_CHECK(st_scale_rows(m.P[c->bias], c->rs >= 0 ? m.P[c->rs] : nullptr, c->src_rows ? c->src_rows : c->Cout, 1,
                             c->Cout, reinterpret_cast<float*>(aux + c->bias_aux), s));
    if (c->fold) {
      float* fo = scratch + rup((size_t)c->Cin * c->Cout * c->K * 4, ALIGN) / 4;
      ST_CHECK(st_fold_w(src, c->Cout, c->Cin, c->K, c->fold, c->fpad0, c->fK, c->fpad, fo, s));
      src = fo;
    }
    ST_CHECK(st_pack_conv(src, c->pCin(), c->Cout, c->fold ? c->fK : c->K, c->transposed, c->u, base + c->off[dt], dt,
                          s));
  }
  // AdaIN projections: Wt[k][hoff + n] = fc.weight[n][k]; bias concat
  float* Wt = reinterpret_cast<float*>(aux + m.wt_off);
  float* bc = reinterpret_cast<float*>(aux + m.bcat_off);
  for (auto* a : m.adains) {
    ST_CHECK(st_ncl_to_frames(m.P[a->w], 1, 2 * a->C, m.style_dim, Wt, m.Htot, a->hoff, 0, nullptr, 0, ST_FP32, s));
    ST_CHECK_HIP(hipMemcpyAsync(bc + a->hoff, m.P[a->b], (size_t)2 * a->C * 4, hipMemcpyDeviceToDevice, s));
  }
  for (auto* sm : m.smalls)
    ST_CHECK(st_wn_fold(m.P[sm->v], m.P[sm->g], (int)sm->rows, (int)sm->inner,
                        reinterpret_cast<float*>(aux + sm->off), s));
  for (auto* p : m.pools)
    ST_CHECK(st_wn_fold(m.P[p->pool_v], m.P[p->pool_g], p->cin, 3, reinterpret_cast<float*>(aux + p->pool_off), s));
  if (m.kind == STTS_KIND_ALIGNER) {
    // the recurrence reads its weights k-major: lanes (output rows) side by side
    const int D = kAlDec, E = m.al_emb;
    float* wc = reinterpret_cast<float*>(aux + m.al_wc_t);
    ST_CHECK(st_transpose(m.P[m.al_wih], 4 * D, D, E + D, E, wc, s));              // W_ih[:, E:] (the context part)
    ST_CHECK(st_transpose(m.P[m.al_whh], 4 * D, D, D, 0, wc + (size_t)D * 4 * D, s));
    ST_CHECK(st_transpose(m.P[m.al_query], D, D, D, 0, reinterpret_cast<float*>(aux + m.al_wq_t), s));
    ST_CHECK(st_transpose(m.P[m.al_loc], kAlLocF, 2 * kAlLocK, 2 * kAlLocK, 0,
                          reinterpret_cast<float*>(aux + m.al_wloc_t), s));
  }
  return 0;
}

int check_params(const Model& m) {
  for (size_t i = 0; i < m.P.ptr.size(); ++i)
    if (!m.P.ptr[i]) return ST_EPARAMS;
  return 0;
}

template <typename F>
int with_ctx(Model* m, int dtype, int B, void* ws, long long ws_bytes, void* stream, F&& body, size_t* need) {
  if (dtype != ST_FP32 && dtype != ST_BF16 && dtype != ST_SPLIT) return ST_EDTYPE;
  const int adt = dtype == ST_BF16 ? ST_BF16 : ST_FP32;  // activation storage
  Ctx c{m, adt, (size_t)(adt == ST_FP32 ? 4 : 2), B, (hipStream_t)stream, true, nullptr};
  c.cdtype = dtype;
  c.slots = g_opt_stats_slots > 0 ? g_opt_stats_slots : (B <= 4 ? 16 : (B <= 16 ? 4 : 1));  // tools/slots_sweep.py
  c.packed = m->packed[dtype];
  c.aux = m->packed[dtype] ? const_cast<char*>(m->packed[dtype]) + m->aux_off[dtype] : nullptr;
  ST_CHECK(body(c));  // dry run: layout
  // the statistics region follows the buffers (stats_off >= off when the body set it); a body
  // without statistics may leave it unset: the buffers alone then size the workspace
  const size_t total = std::max(c.stats_off, c.off);
  if (need) {
    *need = total;
    return 0;
  }
  if (!m->packed[dtype]) return ST_ENOTPACKED;
  if ((long long)total > ws_bytes || !ws) return ST_EWORKSPACE;
  const size_t stats_begin = c.stats_begin;
  Ctx r{m, adt, c.esz, B, (hipStream_t)stream, false, reinterpret_cast<char*>(ws)};
  r.cdtype = dtype;
  r.slots = c.slots;
  r.packed = c.packed;
  r.aux = c.aux;
  if (total > stats_begin) ST_CHECK_HIP(hipMemsetAsync(r.ws + stats_begin, 0, total - stats_begin, r.s));
  return body(r);
}

// The model kinds: how stts_model_create builds one and which forward sizes its workspace (the dry run takes no
// inputs or outputs).  A new kind is one row here and its typed forward entry point.
struct Kind {
  int kind;
  int (*build)(Model&, const int*, int);
  int (*dry)(Ctx&, int T);
};
DecIO dry_io(int T) {
  DecIO io{};
  io.T = T;
  return io;
}
int dry_decoder(Ctx& c, int T) { return decoder_forward(c, dry_io(T)); }
const Kind kKinds[] = {
    {STTS_KIND_HIFIGAN, build_decoder, dry_decoder},
    {STTS_KIND_ISTFTNET, build_decoder, dry_decoder},
    {STTS_KIND_F0N, build_f0n, [](Ctx& c, int T) { return f0n_forward(c, nullptr, nullptr, T, nullptr, nullptr); }},
    {STTS_KIND_STYLE, build_style, [](Ctx& c, int T) { return style_forward(c, nullptr, T, nullptr); }},
    {STTS_KIND_MPD, build_mpd, [](Ctx& c, int T) { return mpd_forward(c, nullptr, T, nullptr); }},
    {STTS_KIND_VOCOS, build_vocos, [](Ctx& c, int T) { return vocos_forward(c, dry_io(T)); }},
    {STTS_KIND_MSD, build_msd, [](Ctx& c, int T) { return msd_forward(c, nullptr, T, nullptr); }},
    {STTS_KIND_PITCH, build_pitch,
     [](Ctx& c, int T) { return pitch_forward(c, nullptr, T, nullptr, nullptr, nullptr, nullptr); }},
    // (the CNN outputs alone; stts_aligner_workspace_bytes sizes a forward with tokens)
    {STTS_KIND_ALIGNER, build_aligner, [](Ctx& c, int T) {
       AlignIO io{};
       io.T = T;
       return aligner_forward(c, io);
     }},
};
const Kind* find_kind(int kind) {
  for (const Kind& k : kKinds)
    if (k.kind == kind) return &k;
  return nullptr;
}

// stts_mpd_losses / stts_msd_losses over the maps of B real then B generated signals (`maps` made for B: a map's real
// half is its size, and the pair starts at twice its offset)
int disc_losses(const DiscMaps& maps, const float* out, double* scratch, long long scratch_bytes, double* loss,
                void* stream) {
  MpdLossSegs sg;
  memset(&sg, 0, sizeof(sg));
  for (const DiscMap& mp : maps) {
    if (sg.n >= kMpdMaxSegs) return ST_EINVAL;
    sg.off[sg.n] = 2 * mp.off;
    sg.half[sg.n] = mp.elems;
    sg.score[sg.n] = mp.score;
    ++sg.n;
  }
  if (scratch_bytes < (long long)sg.n * kMpdLossBlocks * 4 * (long long)sizeof(double)) return ST_EWORKSPACE;
  return st_mpd_losses(out, sg, scratch, loss, (hipStream_t)stream);
}

}  // namespace

// ======================================================================= C-ABI
extern "C" {

int stts_model_create(int kind, const int* cfg, int ncfg, stts_model** out) {
  if (!out || (ncfg > 0 && !cfg)) return ST_EINVAL;
  *out = nullptr;
  const Kind* k = find_kind(kind);
  if (!k) return ST_EINVAL;
  Model* m = new Model();
  m->kind = kind;
  const int r = k->build(*m, cfg, ncfg);
  if (r != 0) {
    delete m;
    return r;
  }
  finalize_layout(*m);
  *out = m;
  return 0;
}

void stts_model_destroy(stts_model* m) { delete m; }

int stts_param_count(const stts_model* m) { return m ? (int)m->P.names.size() : ST_EINVAL; }

const char* stts_param_name(const stts_model* m, int i) {
  if (!m || i < 0 || i >= (int)m->P.names.size()) return nullptr;
  return m->P.names[i].c_str();
}

long long stts_param_numel(const stts_model* m, int i) {
  if (!m || i < 0 || i >= (int)m->P.names.size()) return ST_EINVAL;
  return m->P.numel[i];
}

int stts_set_param(stts_model* m, int i, const float* p) {
  if (!m || i < 0 || i >= (int)m->P.names.size()) return ST_EINVAL;
  m->P.ptr[i] = p;
  for (auto& pk : m->packed) pk = nullptr;  // weights changed: repack required
  return 0;
}

long long stts_packed_bytes(const stts_model* m, int dtype) {
  if (!m) return ST_EINVAL;
  if (dtype != ST_FP32 && dtype != ST_BF16 && dtype != ST_SPLIT) return ST_EDTYPE;
  return (long long)m->total_bytes[dtype];
}

int stts_pack(stts_model* m, int dtype, void* packed, long long bytes, void* stream) {
  if (!m || !packed) return ST_EINVAL;
  if (dtype != ST_FP32 && dtype != ST_BF16 && dtype != ST_SPLIT) return ST_EDTYPE;
  if (bytes < (long long)m->total_bytes[dtype]) return ST_EWORKSPACE;
  ST_CHECK(check_params(*m));
  ST_CHECK(pack_model(*m, dtype, reinterpret_cast<char*>(packed), (hipStream_t)stream));
  m->packed[dtype] = reinterpret_cast<const char*>(packed);
  return 0;
}

long long stts_workspace_bytes(const stts_model* mc, int dtype, int B, int T) {
  if (!mc || B <= 0 || T <= 0) return ST_EINVAL;
  const Kind* k = find_kind(mc->kind);
  if (!k) return ST_EINVAL;
  size_t need = 0;
  const int r = with_ctx(const_cast<Model*>(mc), dtype, B, nullptr, 0, nullptr, [&](Ctx& c) { return k->dry(c, T); },
                         &need);
  return r ? r : (long long)need;
}

int stts_decoder_fwd(stts_model* m, int dtype, const float* asr, const float* f0, const float* n, const float* s,
                     const float* noise, unsigned long long seed, long long utt_offset, int B, int T, float* out,
                     void* ws, long long ws_bytes, void* stream) {
  if (!m || (m->kind != STTS_KIND_HIFIGAN && m->kind != STTS_KIND_ISTFTNET && m->kind != STTS_KIND_VOCOS))
    return ST_EINVAL;
  if (B <= 0 || T <= 0 || !asr || !f0 || !n || !s || !out) return ST_EINVAL;
  ST_CHECK(check_params(*m));
  DecIO io{asr, f0, n, s, noise, seed, utt_offset, T, out};
  if (m->kind == STTS_KIND_VOCOS)
    return with_ctx(m, dtype, B, ws, ws_bytes, stream, [&](Ctx& c) { return vocos_forward(c, io); }, nullptr);
  return with_ctx(m, dtype, B, ws, ws_bytes, stream, [&](Ctx& c) { return decoder_forward(c, io); }, nullptr);
}

int stts_f0n_fwd(stts_model* m, int dtype, const float* x, const float* s, int B, int T, float* F0, float* N,
                 void* ws, long long ws_bytes, void* stream) {
  if (!m || m->kind != STTS_KIND_F0N) return ST_EINVAL;
  if (B <= 0 || T <= 0 || !x || !s || !F0 || !N) return ST_EINVAL;
  ST_CHECK(check_params(*m));
  return with_ctx(m, dtype, B, ws, ws_bytes, stream, [&](Ctx& c) { return f0n_forward(c, x, s, T, F0, N); },
                  nullptr);
}

int stts_style_fwd(stts_model* m, int dtype, const float* mel, int B, int T, float* out, void* ws, long long ws_bytes,
                   void* stream) {
  if (!m || m->kind != STTS_KIND_STYLE) return ST_EINVAL;
  if (B <= 0 || T <= 0 || !mel || !out) return ST_EINVAL;
  ST_CHECK(check_params(*m));
  return with_ctx(m, dtype, B, ws, ws_bytes, stream, [&](Ctx& c) { return style_forward(c, mel, T, out); }, nullptr);
}

int stts_pitch_fwd(stts_model* m, int dtype, const float* mel, int B, int T, float* f0, float* gan_feature,
                   float* pool_out, void* ws, long long ws_bytes, void* stream) {
  if (!m || m->kind != STTS_KIND_PITCH) return ST_EINVAL;
  if (B <= 0 || T <= 0 || !mel || !f0) return ST_EINVAL;
  ST_CHECK(check_params(*m));
  return with_ctx(m, dtype, B, ws, ws_bytes, stream,
                  [&](Ctx& c) { return pitch_forward(c, mel, T, f0, gan_feature, pool_out, nullptr); }, nullptr);
}

long long stts_pitch_error_offset(const stts_model* mc, int dtype, int B, int T) {
  if (!mc || mc->kind != STTS_KIND_PITCH || B <= 0 || T <= 0) return ST_EINVAL;
  size_t need = 0, off = 0;
  const int r = with_ctx(const_cast<Model*>(mc), dtype, B, nullptr, 0, nullptr,
                         [&](Ctx& c) { return pitch_forward(c, nullptr, T, nullptr, nullptr, nullptr, &off); }, &need);
  return r ? r : (long long)off;
}

int stts_log_norm(const float* mel, int B, int n_mels, int T, float mean, float std, float* out, void* stream) {
  return st_log_norm(mel, B, n_mels, T, mean, std, out, (hipStream_t)stream);
}

int stts_aligner_fwd(stts_model* m, int dtype, const float* mel, const unsigned char* pad_mask, const int* tokens,
                     const unsigned char* unk_mask, int B, int T, int Tt, float* ctc, float* s2s_logit, float* attn,
                     float* feature, void* ws, long long ws_bytes, void* stream) {
  if (!m || m->kind != STTS_KIND_ALIGNER) return ST_EINVAL;
  if (dtype == ST_BF16) return ST_EDTYPE;  // the recurrence and GroupNorm are fp32: fp32 storage only
  if (B <= 0 || T <= 0 || !mel || (tokens && Tt <= 0) || Tt < 0) return ST_EINVAL;
  ST_CHECK(check_params(*m));
  AlignIO io{mel, pad_mask, unk_mask, tokens, T, tokens ? Tt : 0, ctc, s2s_logit, attn, feature};
  if (!tokens) io.s2s = io.attn = nullptr;
  return with_ctx(m, dtype, B, ws, ws_bytes, stream, [&](Ctx& c) { return aligner_forward(c, io); }, nullptr);
}

long long stts_aligner_workspace_bytes(const stts_model* mc, int dtype, int B, int T, int Tt) {
  if (!mc || mc->kind != STTS_KIND_ALIGNER || B <= 0 || T <= 0 || Tt < 0) return ST_EINVAL;
  if (dtype == ST_BF16) return ST_EDTYPE;
  AlignIO io{};
  io.T = T;
  io.Tt = Tt;
  size_t need = 0;
  const int r = with_ctx(const_cast<Model*>(mc), dtype, B, nullptr, 0, nullptr,
                         [&](Ctx& c) { return aligner_forward(c, io); }, &need);
  return r ? r : (long long)need;
}

long long stts_maximum_path_workspace_bytes(int B, int Tx, int Ty) { return st_max_path_workspace_bytes(B, Tx, Ty); }

int stts_maximum_path(const float* value, const int* tx_len, const int* ty_len, int B, int Tx, int Ty, float* path,
                      void* workspace, long long ws_bytes, void* stream) {
  if (!value || !tx_len || !ty_len || !path || B <= 0 || Tx <= 0 || Ty <= 0) return ST_EINVAL;
  for (int b = 0; b < B; ++b)  // the search is undefined outside 1 <= tx <= ty (host values: refused here)
    if (tx_len[b] < 1 || tx_len[b] > ty_len[b] || tx_len[b] > Tx || ty_len[b] > Ty) return ST_EINVAL;
  return st_max_path(value, tx_len, ty_len, B, Tx, Ty, path, workspace, ws_bytes, (hipStream_t)stream);
}

long long stts_mpd_out_elems(const stts_model* m, int B, int T) {
  if (!m || m->kind != STTS_KIND_MPD || B <= 0 || T <= 0) return ST_EINVAL;
  return maps_elems(mpd_maps(*m, B, T));
}

int stts_mpd_fwd(stts_model* m, int dtype, const float* wave, int B, int T, float* out, long long out_elems,
                 void* ws, long long ws_bytes, void* stream) {
  if (!m || m->kind != STTS_KIND_MPD) return ST_EINVAL;
  if (B <= 0 || !wave || !out) return ST_EINVAL;
  for (const auto& d : m->mpd)  // the reference's reflect pad needs the pad < T
    if (T < 2 || (T + d.period - 1) / d.period * d.period - T >= T) return ST_EINVAL;
  if (out_elems < maps_elems(mpd_maps(*m, B, T))) return ST_EINVAL;
  ST_CHECK(check_params(*m));
  return with_ctx(m, dtype, B, ws, ws_bytes, stream, [&](Ctx& c) { return mpd_forward(c, wave, T, out); }, nullptr);
}

// scratch of stts_mpd_losses / stts_msd_losses: kMpdLossBlocks partial blocks x 4 sums per (discriminator,
// layer) segment (6 per period / resolution)
long long stts_gan_losses_scratch_bytes(const stts_model* m) {
  if (!m) return ST_EINVAL;
  size_t segs;  // (the number of maps depends on neither the batch nor the length)
  if (m->kind == STTS_KIND_MPD) segs = mpd_maps(*m, 1, 1).size();
  else if (m->kind == STTS_KIND_MSD) segs = msd_maps(*m, 1, 1).size();
  else return ST_EINVAL;
  return (long long)segs * kMpdLossBlocks * 4 * (long long)sizeof(double);
}

int stts_mpd_losses(const stts_model* m, int B, int T, const float* out, double* scratch,
                    long long scratch_bytes, double* loss, void* stream) {
  if (!m || m->kind != STTS_KIND_MPD || B <= 0 || T <= 0 || !out || !scratch || !loss) return ST_EINVAL;
  return disc_losses(mpd_maps(*m, B, T), out, scratch, scratch_bytes, loss, stream);
}

// MultiResolutionSTFTLoss (losses.py:55-94): workspace = the per-resolution partial sums (fixed-order
// reduction) + one resolution's log-mels of both signals (resolutions run one after the other on the stream)
long long stts_mrstft_workspace_bytes(int B, long long L, const int* hops, int n_res, int n_mels) {
  if (B <= 0 || L <= 0 || !hops || n_res <= 0 || n_res > 16 || n_mels <= 0) return ST_EINVAL;
  long long f = 0;
  for (int r = 0; r < n_res; ++r) {
    if (hops[r] <= 0) return ST_EINVAL;
    f = std::max(f, st_stft_frames(L, hops[r]));
  }
  return ((st_sc_part_bytes(n_res) + 255) & ~255LL) + 2LL * B * n_mels * f * 4;
}

int stts_mrstft_loss(const float* x, const float* y, int B, long long L, long long ld, const int* n_ffts,
                     const int* hops, const int* wins, int n_res, int sample_rate, int n_mels, double* loss, void* ws,
                     long long ws_bytes, void* stream) {
  if (!x || !y || !loss || !n_ffts || !hops || !wins || B <= 0 || sample_rate <= 0) return ST_EINVAL;
  const long long need = stts_mrstft_workspace_bytes(B, L, hops, n_res, n_mels);
  if (need < 0) return (int)need;
  if (!ws || ws_bytes < need) return ST_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  const long long pb = (st_sc_part_bytes(n_res) + 255) & ~255LL;
  float* mx = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + pb);
  for (int r = 0; r < n_res; ++r) {
    const long long F = st_stft_frames(L, hops[r]);
    float* my = mx + (size_t)B * n_mels * F;
    ST_CHECK(st_logmel(x, B, L, ld, n_ffts[r], wins[r], hops[r], n_mels, (float)sample_rate, mx, s));
    ST_CHECK(st_logmel(y, B, L, ld, n_ffts[r], wins[r], hops[r], n_mels, (float)sample_rate, my, s));
    ST_CHECK(st_sc_sums(mx, my, (long long)B * n_mels * F, part + (size_t)r * st_sc_part_bytes(1) / 8, s));
  }
  return st_sc_final(part, n_res, loss, s);
}

long long stts_msd_out_elems(const stts_model* m, int B, int T) {
  if (!m || m->kind != STTS_KIND_MSD || B <= 0 || T <= 0) return ST_EINVAL;
  return maps_elems(msd_maps(*m, B, T));
}

int stts_msd_fwd(stts_model* m, int dtype, const float* wave, int B, int T, float* out, long long out_elems,
                 void* ws, long long ws_bytes, void* stream) {
  if (!m || m->kind != STTS_KIND_MSD) return ST_EINVAL;
  if (B <= 0 || !wave || !out) return ST_EINVAL;
  for (const auto& d : m->msd)  // torch.stft's reflect pad needs n_fft / 2 < T
    if (T <= d.n_fft / 2) return ST_EINVAL;
  if (out_elems < maps_elems(msd_maps(*m, B, T))) return ST_EINVAL;
  ST_CHECK(check_params(*m));
  return with_ctx(m, dtype, B, ws, ws_bytes, stream, [&](Ctx& c) { return msd_forward(c, wave, T, out); }, nullptr);
}

int stts_msd_losses(const stts_model* m, int B, int T, const float* out, double* scratch,
                    long long scratch_bytes, double* loss, void* stream) {
  if (!m || m->kind != STTS_KIND_MSD || B <= 0 || T <= 0 || !out || !scratch || !loss) return ST_EINVAL;
  return disc_losses(msd_maps(*m, B, T), out, scratch, scratch_bytes, loss, stream);
}

long long stts_mel_frames(long long L) { return st_mel_frames(L); }

long long stts_mel_workspace_bytes(void) { return st_mel_workspace_bytes(); }

int stts_wave_preprocess(const float* wave, int B, long long L, long long wave_ld, float* mel, void* ws,
                         long long ws_bytes, void* stream) {
  return st_wave_preprocess(wave, B, L, wave_ld, mel, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int stts_abi_version(void) { return STTS_ABI_VERSION; }

const char* stts_error_string(int code) {
  switch (code) {
    case 0: return "ok";
    case ST_EINVAL: return "invalid argument or shape";
    case ST_EDTYPE: return "unsupported dtype";
    case ST_EPARAMS: return "parameter table incomplete";
    case ST_EWORKSPACE: return "workspace / buffer too small";
    case ST_ENOTPACKED: return "weights not packed for this dtype";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
  }
}

int stts_set_debug_buffer(void* buf) {
  g_dbg_stamps = reinterpret_cast<unsigned long long*>(buf);
  return 0;
}

int stts_profile_enable(int on) {
  g_prof.on = on != 0;
  g_prof.used = 0;
  g_prof.launches = 0;
  g_prof.flops = g_prof.bytes = 0;
  g_prof.rec.clear();
  return 0;
}

int stts_profile_launch(long long i, int* shape, double* ms_flops_bytes) {
  if (i < 0 || (size_t)i >= g_prof.rec.size() || 2 * (size_t)i + 1 >= g_prof.used) return ST_EINVAL;
  float ms = 0;
  ST_CHECK_HIP(hipEventSynchronize(g_prof.ev[2 * i + 1]));
  ST_CHECK_HIP(hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]));
  const auto& r = g_prof.rec[i];
  if (shape)
    for (int k = 0; k < 8; ++k) shape[k] = r.shape[k];
  if (ms_flops_bytes) {
    ms_flops_bytes[0] = ms;
    ms_flops_bytes[1] = r.flops;
    ms_flops_bytes[2] = r.bytes;
  }
  return 0;
}

int stts_profile_read(double* total_ms, long long* launches, double* alg_flops, double* alg_bytes) {
  double t = 0;
  for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
    float ms = 0;
    ST_CHECK_HIP(hipEventSynchronize(g_prof.ev[i + 1]));
    ST_CHECK_HIP(hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]));
    t += ms;
  }
  if (total_ms) *total_ms = t;
  if (launches) *launches = g_prof.launches;
  if (alg_flops) *alg_flops = g_prof.flops;
  if (alg_bytes) *alg_bytes = g_prof.bytes;
  return 0;
}

}  // extern "C"
