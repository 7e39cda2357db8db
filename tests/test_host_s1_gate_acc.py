"""Host check of the row gate's accumulated-drift form (csrc/km_s1_gate.h:
s1g_acc_add, s1g_acc_up, s1g_acc_dn, s1g_acc_pass, s1g_base, s1g_keep).

The kernels no longer step a margin every pass.  A row stores
base = round_down(marg_fresh + acc_dn[label]) and the gate only compares it
with acc_up[label], where acc[j] is the float64 running total of
shift[j] + (largest other shift) over the gated passes.  Like
test_host_s1_gate.py this compiles the header into a stand-alone program and
checks in float64:

  * over random cases and sequences of 1 .. 300 centroid moves, starting from
    an arbitrary earlier total: "base > acc_up[label]" implies that the label
    is still the strict argmin (kmeans_spark.py:153-159: np.argmin, first
    minimum -- a strict argmin is the same under any tie rule);
  * shifts of 0, denormal size, 1e30, inf and NaN never leave a row unlisted in
    the pass they occur in (inf, NaN), and after such a pass the totals are 0
    again; the case then goes on as the kernels do: the centroid whose move was
    unbounded stands somewhere finite (a repair), the row is screened, gets a
    new base against acc_dn = 0 under its new label, and the implication must
    hold over the passes that follow;
  * s1g_xnorm(fp32 sum of squares) >= ||x|| in float64 for rows of 8 .. 128
    features of every scale, denormal and near-overflow ones included, and a
    row with an inf or a NaN never gets a finite bound (k_s1's `bad` test);
  * drift: after one move of 10 and 1e4 moves of 1e-7 of both the row's own
    centroid and its nearest rival, a row whose true margin is still above
    1e-3 is still not listed.  A float total inflated by s1g_up per pass
    (8 u relative of ~10: 4.8e-6 a pass, 4.8e-2 over the sequence) would list
    it; the float64 total's error is one float ulp of acc (<= 4e-6 for
    acc ~ 10 .. 50), 200 times below the 1e-3.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "assignment--2-group7-distributed-k-means_amd", "csrc")

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include "km_s1_gate.h"

using namespace km;
static const int D = 8, K = 6;

static double dist(const float* x, const double* c) {
  double s = 0.0;
  for (int f = 0; f < D; ++f) s += ((double)x[f] - c[f]) * ((double)x[f] - c[f]);
  return std::sqrt(s);
}

static bool strict_argmin(const float* x, const double (*C)[D], int lab) {
  const double dl = dist(x, C[lab]);
  for (int j = 0; j < K; ++j)
    if (j != lab && !(dl < dist(x, C[j]))) return false;
  return true;
}

// one pass: shifts sh[] into the totals, the images of every cluster
static void pass(double* acc, const float* sh, float* up, float* dn) {
  float m1 = -1.0f, m2 = -1.0f;
  int a1 = 0;
  for (int j = 0; j < K; ++j) {
    if (sh[j] > m1) {
      m2 = m1;
      m1 = sh[j];
      a1 = j;
    } else {
      m2 = std::fmax(m2, sh[j]);
    }
  }
  m2 = std::fmax(m2, 0.0f);
  for (int j = 0; j < K; ++j) acc[j] = s1g_acc_pass(acc[j], sh[j], j == a1 ? m2 : m1, m1, false, &up[j], &dn[j]);
}

int main() {
  std::mt19937_64 rng(4321);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  std::normal_distribution<double> N(0.0, 1.0);
  const float RHO = 255.0f * 1.1920928955078125e-07f * 1.0001f, RP = RHO * (1.0f + 2.0f * RHO);
  long cases = 0, passes = 0, kept = 0, long_kept = 0, bad_label = 0, bad_special = 0, bad_recover = 0;
  long recovered = 0, recovered_kept = 0;
  for (int it = 0; it < 200000; ++it) {
    ++cases;
    const double scale = std::pow(10.0, 3.0 * U(rng));            // data scale 1e-3 .. 1e3
    const double spread = std::pow(10.0, -1.0 + 1.5 * U(rng));    // centroid spread relative to it
    float x[D];
    double C[K][D];
    for (int f = 0; f < D; ++f) x[f] = (float)(scale * N(rng));
    for (int j = 0; j < K; ++j)
      for (int f = 0; f < D; ++f) C[j][f] = (double)x[f] + scale * spread * (j + 1) * N(rng);
    if (it % 7 == 0) std::memcpy(C[4], C[1], sizeof(C[1]));       // duplicate centroids
    int e;
    (void)std::frexp(scale * 8.0, &e);
    const float s = std::ldexp(1.0f, 10 - e);
    double Kx[K], kmax = 0.0;
    for (int j = 0; j < K; ++j) {
      double cc = 0.0, cx = 0.0;
      for (int f = 0; f < D; ++f) {
        cc += C[j][f] * C[j][f];
        cx += C[j][f] * (double)x[f];
      }
      Kx[j] = (double)s * s * (cc - 2.0 * cx);
      kmax = std::fmax(kmax, std::fabs(Kx[j]));
    }
    const double Es = kmax * std::pow(10.0, -6.0 + 3.0 * std::fabs(U(rng))) + 1e-30;  // |e| <= E
    float key[K];
    for (int j = 0; j < K; ++j) {
      float kf = (float)(Kx[j] + 0.9 * Es * U(rng));
      if (std::fabs((double)kf - Kx[j]) > Es) kf = (float)Kx[j];
      uint32_t b;
      std::memcpy(&b, &kf, 4);
      b = (b & ~255u) | (uint32_t)(rng() & 255u);                  // the id packing
      std::memcpy(&key[j], &b, 4);
    }
    int lab = 0;
    for (int j = 1; j < K; ++j)
      if (dist(x, C[j]) < dist(x, C[lab])) lab = j;
    bool after_wild = false;
    float xs = 0.0f;
    for (int f = 0; f < D; ++f) xs = fmaf(x[f], x[f], xs);
    const S1GRow r = s1g_row(s, (float)(Es * (1.0 + 1e-6)), xs);
    float ko = std::numeric_limits<float>::max();
    for (int j = 0; j < K; ++j)
      if (j != lab) ko = std::fmin(ko, key[j]);
    const float marg = s1g_margin(s1g_lb(ko, RP, r), s1g_ub(key[lab], RP, r));
    // the totals of an epoch already under way (or a new one), then the base
    double acc[K];
    float up[K], dn[K];
    const int prior = (int)(rng() % 4);
    for (int j = 0; j < K; ++j) {
      acc[j] = prior == 0 ? 0.0 : scale * spread * std::pow(10.0, 2.0 * U(rng)) * (prior == 3 ? 1e3 : 1.0);
      dn[j] = s1g_acc_dn(acc[j]);
    }
    float base = s1g_base(marg, dn[lab]);
    // 1 .. 300 passes of moves, small against the margin so that sequences last
    const int len = 1 + (int)(rng() % ((it % 16 == 0) ? 300 : 24));
    const double mexp = -5.0 + 2.0 * U(rng);
    int p = 0;
    for (; p < len; ++p) {
      ++passes;
      float sh[K];
      bool special = false;
      for (int j = 0; j < K; ++j) {
        const int kind = (int)(rng() % 64);
        double mag = scale * spread * std::pow(10.0, mexp + 1.5 * U(rng));
        if (kind == 0) mag = 0.0;
        if (kind == 1) mag = 1e-310;
        if (kind == 2 && it % 5 == 0) mag = 1e30;
        if (kind == 3 && it % 11 == 0) mag = std::numeric_limits<double>::infinity();
        if (kind == 4 && it % 13 == 0) mag = std::numeric_limits<double>::quiet_NaN();
        if (!(mag <= 1e300)) special = true;
        double dir[D], nn = 0.0, sq = 0.0;
        for (int f = 0; f < D; ++f) {
          dir[f] = N(rng);
          nn += dir[f] * dir[f];
        }
        for (int f = 0; f < D; ++f) {
          const double nv = C[j][f] + mag * dir[f] / std::sqrt(nn);
          const double df = nv - C[j][f];
          sq = std::fma(df, df, sq);
          C[j][f] = nv;
        }
        sh[j] = s1g_shift(sq);  // (inf, NaN: +inf)
        // an unbounded move ends somewhere finite (a repaired centroid): the
        // shift stays +inf, which bounds any move
        if (!(mag <= 1e300))
          for (int f = 0; f < D; ++f) C[j][f] = (double)x[f] + scale * spread * (j + 1) * N(rng);
      }
      pass(acc, sh, up, dn);
      if (special) {
        // the pass lists every row and leaves the totals at 0 ...
        for (int j = 0; j < K; ++j)
          if (s1g_keep(base, up[j]) || s1g_keep(3.0e38f, up[j])) ++bad_special;
        for (int j = 0; j < K; ++j)
          if (!(acc[j] == 0.0) || !(dn[j] == 0.0f)) ++bad_recover;
        // ... and the row, screened, gets a new base against them under its
        // new label (bounds from the exact distances, rounded outwards); a row
        // that is no strict argmin would be queued: base 0, listed next time
        lab = 0;
        for (int j = 1; j < K; ++j)
          if (dist(x, C[j]) < dist(x, C[lab])) lab = j;
        if (!strict_argmin(x, C, lab)) break;
        double dother = 1e300;
        for (int j = 0; j < K; ++j)
          if (j != lab) dother = std::fmin(dother, dist(x, C[j]));
        const float ubf = std::nextafter((float)dist(x, C[lab]), INFINITY);
        const float lbf = std::nextafter((float)dother, -INFINITY);
        base = s1g_base(s1g_margin(lbf, ubf), dn[lab]);
        after_wild = true;
        ++recovered;
        continue;
      }
      if (!s1g_keep(base, up[lab])) break;  // listed: the row would be screened and get a new base
      ++kept;
      if (after_wild) ++recovered_kept;
      if (p >= 100) ++long_kept;
      if (!strict_argmin(x, C, lab)) ++bad_label;
    }
  }

  // s1g_xnorm: an upper bound of ||x|| from the fp32 sum of squares as k_s1
  // forms it (four lanes' fma chains, then (l0 + l1) + (l2 + l3)); rows of 8 ..
  // 128 features at scales from denormal to overflow, some with inf or NaN
  long xn_cases = 0, xn_bad = 0, xn_nonfinite = 0, xn_nonfinite_bad = 0;
  for (int it = 0; it < 200000; ++it) {
    ++xn_cases;
    const int len = 8 << (it % 5);  // 8 .. 128
    float xv[128];
    const int mode = it % 8;
    const double sc = mode == 0 ? 1e-42 : mode == 1 ? 1e-22 : mode == 2 ? 1.5e18 : mode == 3 ? 3e19
                                 : std::pow(10.0, 12.0 * U(rng));
    for (int f = 0; f < len; ++f) xv[f] = (float)(sc * N(rng));
    if (it % 16 == 5) std::memset(xv, 0, sizeof(float) * len);
    bool nonfinite = false;
    if (it % 29 == 0) { xv[rng() % len] = std::numeric_limits<float>::infinity(); nonfinite = true; }
    if (it % 31 == 0) { xv[rng() % len] = std::numeric_limits<float>::quiet_NaN(); nonfinite = true; }
    float part[4];
    double nn = 0.0;
    for (int l = 0; l < 4; ++l) {
      float a = 0.0f;
      for (int f = l * (len / 4); f < (l + 1) * (len / 4); ++f) {
        a = fmaf(xv[f], xv[f], a);
        nn += (double)xv[f] * (double)xv[f];
      }
      part[l] = a;
    }
    const float xs = (part[0] + part[1]) + (part[2] + part[3]);
    const float xn = s1g_xnorm(xs);
    if (nonfinite) {
      ++xn_nonfinite;
      if (xn <= 3.0e38f) ++xn_nonfinite_bad;
    } else if (!((double)xn >= std::sqrt(nn))) {
      ++xn_bad;  // (an overflowing sum gives +inf: still a bound, and `bad` in k_s1)
    }
  }

  // drift: x at the origin, its centroid at distance 1, the nearest rival at
  // 11.004, the rest far away.  Pass 1: the rival comes 10 nearer.  Then 1e4
  // passes in which the row's centroid moves 1e-7 away and the rival 1e-7
  // nearer: the worst case the bound assumes is what really happens, so the
  // true margin ends at 11.004 - 10 - 1 - 2e-3 = 2e-3.
  long drift_passes = 0, drift_listed = 0, drift_bad_label = 0;
  double drift_margin = 0.0;
  {
    float x[D] = {0};
    double C[K][D] = {{0}};
    const int lab = 2, riv = 4;
    for (int j = 0; j < K; ++j) C[j][j] = 60.0 + j;
    std::memset(C[lab], 0, sizeof(C[lab]));
    std::memset(C[riv], 0, sizeof(C[riv]));
    C[lab][0] = 1.0;
    C[riv][1] = 11.004;
    double acc[K] = {37.5, 12.25, 41.0625, 3.0, 29.0, 0.0};  // an epoch under way
    float up[K], dn[K];
    for (int j = 0; j < K; ++j) dn[j] = s1g_acc_dn(acc[j]);
    const float ubf = std::nextafter((float)dist(x, C[lab]), INFINITY);
    const float lbf = std::nextafter((float)dist(x, C[riv]), -INFINITY);
    const float base = s1g_base(s1g_margin(lbf, ubf), dn[lab]);
    for (int p = 0; p <= 10000; ++p) {
      ++drift_passes;
      double old[K][D];
      std::memcpy(old, C, sizeof(C));
      if (p == 0) {
        C[riv][1] -= 10.0;
      } else {
        C[lab][0] += 1e-7;
        C[riv][1] -= 1e-7;
      }
      float sh[K];
      for (int j = 0; j < K; ++j) {
        double sq = 0.0;
        for (int f = 0; f < D; ++f) sq = std::fma(C[j][f] - old[j][f], C[j][f] - old[j][f], sq);
        sh[j] = s1g_shift(sq);
      }
      pass(acc, sh, up, dn);
      if (!s1g_keep(base, up[lab])) ++drift_listed;
      else if (!strict_argmin(x, C, lab)) ++drift_bad_label;
    }
    drift_margin = dist(x, C[riv]) - dist(x, C[lab]);
  }
  std::printf("recovered %ld recovered_kept %ld xn_cases %ld xn_bad %ld xn_nonfinite %ld xn_nonfinite_bad %ld ",
              recovered, recovered_kept, xn_cases, xn_bad, xn_nonfinite, xn_nonfinite_bad);
  std::printf("cases %ld passes %ld kept %ld long_kept %ld bad_label %ld bad_special %ld bad_recover %ld "
              "drift_passes %ld drift_listed %ld drift_bad_label %ld drift_margin_e9 %ld\n",
              cases, passes, kept, long_kept, bad_label, bad_special, bad_recover, drift_passes, drift_listed,
              drift_bad_label, (long)(drift_margin * 1e9));
  return 0;
}
"""


def _compiler():
    for cc in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cc)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def test_base_above_total_implies_unchanged_strict_argmin(tmp_path):
    src = tmp_path / "s1_gate_acc_check.cpp"
    exe = tmp_path / "s1_gate_acc_check"
    src.write_text(PROGRAM)
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe), "-lm"],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    print(out)
    vals = dict(zip(out.split()[0::2], map(int, out.split()[1::2])))
    assert vals["cases"] >= 200000
    assert vals["bad_label"] == 0 and vals["bad_special"] == 0 and vals["bad_recover"] == 0, out
    # the recovery after an inf / NaN pass is exercised: new bases against the
    # zeroed totals keep rows unlisted over later passes (bad_label covers them)
    assert vals["recovered"] >= 1000 and vals["recovered_kept"] >= vals["recovered"], out
    # the row-norm bound: never below ||x||, never finite for an inf / NaN row
    assert vals["xn_cases"] >= 200000 and vals["xn_bad"] == 0, out
    assert vals["xn_nonfinite"] >= 1000 and vals["xn_nonfinite_bad"] == 0, out
    # not vacuous: rows stay unlisted over many passes, some beyond a hundred
    assert vals["kept"] >= 5 * vals["cases"] and vals["long_kept"] > 0, out
    # the drift sequence: one move of 10 and 1e4 of 1e-7; the true margin is
    # still above 1e-3 at the end, the row was never listed, its label held
    assert vals["drift_passes"] == 10001
    assert vals["drift_margin_e9"] > 1_000_000, out
    assert vals["drift_listed"] == 0 and vals["drift_bad_label"] == 0, out
