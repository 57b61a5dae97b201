// Host-only byte layouts of the S2S training entries (aligner_train.hip): the state the training forward keeps for
// the backward, and the two workspaces.  Plain C++ with no device code, so a stand-alone host program can walk it.
#pragma once

namespace s2s {

constexpr int kD = 128;                         // decoder / attention / memory width
constexpr int kLocTaps = 2 * 63 * 32;           // location conv weight
constexpr long long kMaxRows = 1LL << 24;       // B * L and B * (Tt + 1): keeps every float offset far below 2^40

struct Dims {
  int B, L, Tt, ntok, E;
  long long rows() const { return (long long)B * L; }
  long long srows() const { return (long long)B * (Tt + 1); }
  bool ok() const {
    return B > 0 && L > 0 && Tt > 0 && ntok >= 4 && ntok <= 65536 && E > 0 && E <= 1024 && rows() <= kMaxRows &&
           srows() <= kMaxRows;
  }
};

struct Bump {
  long long off = 0;
  long long take(long long floats) {  // byte offset of `floats` floats, 256-byte aligned
    const long long o = off;
    off += (floats * 4 + 255) / 256 * 256;
    return o;
  }
};

// saved by stts_s2s_fwd_train for stts_s2s_bwd
struct SaveLayout {
  long long gates, cell, cum, hc, pm, bytes;
  explicit SaveLayout(const Dims& d) {
    Bump b;
    gates = b.take(d.srows() * 4 * kD);
    cell = b.take(d.srows() * kD);
    cum = b.take(d.srows() * d.L);
    hc = b.take(d.srows() * 2 * kD);
    pm = b.take(d.rows() * kD);
    bytes = b.off;
  }
};

struct FwdLayout {
  long long wc_t, wq_t, wloc_t, emb, gin, hd, bytes;
  explicit FwdLayout(const Dims& d) {
    Bump b;
    wc_t = b.take(2LL * kD * 4 * kD);
    wq_t = b.take((long long)kD * kD);
    wloc_t = b.take(kLocTaps);
    emb = b.take(d.srows() * d.E);
    gin = b.take(d.srows() * 4 * kD);
    hd = b.take(d.srows() * kD);
    bytes = b.off;
  }
};

inline long long max2(long long a, long long b) { return a > b ? a : b; }

struct BwdLayout {
  long long emb, tok, hd, dpre, dhc, dgates, dq, dctx, q, dpmem, xh, hprev, demb, pv, pwd, ploc, ta, tb, tw, bytes;
  explicit BwdLayout(const Dims& d) {
    const long long S = d.srows(), R = d.rows();
    Bump b;
    emb = b.take(S * d.E);
    tok = b.take(S * 2);  // int64 effective token ids
    hd = b.take(S * kD);
    dpre = b.take(S * kD);
    dhc = b.take(S * 2 * kD);
    dgates = b.take(S * 4 * kD);
    dq = b.take(S * kD);
    dctx = b.take(S * kD);
    q = b.take(S * kD);
    dpmem = b.take(R * kD);
    xh = b.take(S * (d.E + kD));
    hprev = b.take(S * kD);
    demb = b.take(S * d.E);
    pv = b.take((long long)d.B * kD);
    pwd = b.take((long long)d.B * kD * 32);
    ploc = b.take((long long)d.B * kLocTaps);
    ta = b.take(max2(max2((long long)d.ntok, 4 * kD) * S, kD * R));   // A^T of the weight-gradient products
    tb = b.take(max2(max2(2 * kD, d.E + kD) * S, kD * R));            // X^T of the same
    tw = b.take(max2(max2((long long)kD * d.ntok, 2LL * kD * kD), 4LL * kD * d.E));  // a transposed weight
    bytes = b.off;
  }
};

}  // namespace s2s
