// Stand-alone host check of the S2S training entries' byte layouts (csrc/s2s_layout.h); build it with
//   c++ -std=c++17 -fsanitize=address,undefined -I styletts2-lite_amd/csrc tools/s2s_layout_check.cpp
// and run it: every region of every layout is 256-byte aligned, lies inside the reported size and overlaps no other,
// over a sweep of shapes up to the caps.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "s2s_layout.h"

using namespace s2s;

static int check(const char* what, std::vector<std::pair<long long, long long>> r, long long bytes) {
  std::sort(r.begin(), r.end());
  for (size_t i = 0; i < r.size(); ++i) {
    const long long end = r[i].first + r[i].second * 4;
    const long long next = i + 1 < r.size() ? r[i + 1].first : bytes;
    if (r[i].first < 0 || r[i].first % 256 || r[i].second <= 0 || end > next) {
      std::printf("%s: region %zu [%lld, %lld) next %lld\n", what, i, r[i].first, end, next);
      return 1;
    }
  }
  return 0;
}

int main() {
  int bad = 0;
  long long n = 0;
  for (int B : {1, 2, 3, 16, 64})
    for (int L : {1, 7, 127, 128, 129, 400, 4096})
      for (int Tt : {1, 5, 150, 1000})
        for (int ntok : {4, 35, 178, 65536})
          for (int E : {1, 256, 512, 1024}) {
            const Dims d{B, L, Tt, ntok, E};
            if (!d.ok()) continue;
            const long long S = d.srows(), R = d.rows();
            const SaveLayout s(d);
            bad += check("save", {{s.gates, S * 4 * kD}, {s.cell, S * kD}, {s.cum, S * L}, {s.hc, S * 2 * kD}, {s.pm, R * kD}},
                         s.bytes);
            const FwdLayout f(d);
            bad += check("fwd", {{f.wc_t, 2LL * kD * 4 * kD}, {f.wq_t, (long long)kD * kD}, {f.wloc_t, kLocTaps},
                                 {f.emb, S * E}, {f.gin, S * 4 * kD}, {f.hd, S * kD}}, f.bytes);
            const BwdLayout w(d);
            const long long ta = std::max(std::max((long long)ntok, 4LL * kD) * S, kD * R);
            const long long tb = std::max(std::max(2LL * kD, (long long)E + kD) * S, kD * R);
            const long long tw = std::max(std::max((long long)kD * ntok, 2LL * kD * kD), 4LL * kD * E);
            bad += check("bwd", {{w.emb, S * E}, {w.tok, S * 2}, {w.hd, S * kD}, {w.dpre, S * kD}, {w.dhc, S * 2 * kD},
                                 {w.dgates, S * 4 * kD}, {w.dq, S * kD}, {w.dctx, S * kD}, {w.q, S * kD}, {w.dpmem, R * kD},
                                 {w.xh, S * (E + kD)}, {w.hprev, S * kD}, {w.demb, S * E}, {w.pv, (long long)B * kD},
                                 {w.pwd, (long long)B * kD * 32}, {w.ploc, (long long)B * kLocTaps}, {w.ta, ta},
                                 {w.tb, tb}, {w.tw, tw}}, w.bytes);
            ++n;
          }
  std::printf("%lld shapes, %d bad\n", n, bad);
  return bad ? 1 : 0;
}
