// Bound arithmetic of the delta-mode row gate (km_screen1.hip: k_s1_gate,
// k_s1_shift and the gated instance of k_s1).  DESIGN.md section 2, "Row gate".
//
// Per row the gate keeps one float, marg = lb - ub, where for the float64
// centroids c the margin was computed against
//   ub >= ||x - c_label||,   lb <= min over j != label of ||x - c_j||.
// When the centroids move by shift[j] >= ||c_j' - c_j||, the triangle
// inequality gives ub' = ub + shift[label] and lb' = lb - max over j != label
// of shift[j], so marg' = marg - shift[label] - max other shift.  A row whose
// margin stays strictly positive keeps its label: its centroid is strictly
// nearer than every other one, so the reference's argmin (lowest index among
// ties) cannot pick another.  Such a row is not screened at all; every other
// row is, and gets a fresh margin from the screen's own bounds.
//
// Rounding: every step is rounded away from the side that would help the
// test -- upper bounds by s1g_up, lower bounds and margins by s1g_dn (8 u
// relative plus 1e-30 absolute per step, u = 2^-24: above the one or two
// roundings of the step itself and above anything a flushed or denormal
// intermediate can lose).  NaN propagates into the margin and +-inf may
// appear; s1g_margin maps both to 0, and the gate lists every row whose
// margin is not > 0.
//
// Accumulated-drift form (what the kernels store).  Stepping every margin
// every pass means writing every margin every pass.  Instead the runtime keeps
// one running total per cluster,
//   acc[j] = sum over the gated passes of (shift[j] + largest other shift),
// since the margins' epoch began (a dense pass that rewrites every margin, or
// a pass with a non-finite shift, which lists every row: acc = 0 again), and a
// row stores base = round_down(marg_fresh + acc_dn[label]) with acc_dn <= acc
// at the time its margin was fresh.  The gate's test is the bare comparison
//   base > acc_up[label],  acc_up >= acc now,
// no arithmetic, no rounding, nothing written back.  Proof (real arithmetic;
// `then`: when the margin was fresh; the label has not changed since, or the
// row would have been listed and given a new base):
//   marg_now >= marg_fresh - (acc_now - acc_then)      (the steps' sum; every
//                                         accumulation is rounded up)
//            >= (base - acc_dn_then) + acc_then - acc_now   (base rounded down)
//            >= base - acc_now >= base - acc_up_now > 0.
// A queued, non-finite or undecided row stores 0, and acc_up > 0 always, so it
// is listed.  acc is float64, each addition rounded up by 1 + 2^-50, and is
// published as two floats per pass (s1g_acc_up, s1g_acc_dn: one float ulp of
// acc either way).  Why not a float total rounded by s1g_up: its 8 u relative
// inflation of acc ~ 50 is 2.5e-5 per pass, more than the real shifts of a
// converged fit, so every row would slowly be listed again; the float64 form's
// error is constant, one ulp of acc.  A non-finite shift makes acc_up +inf:
// the comparison fails for every row.
//
// Plain C++ (no HIP headers): tests/test_host_s1_gate.py and
// tests/test_host_s1_gate_acc.py compile it into host programs and check the
// certificate in float64.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KM_S1G_FN __host__ __device__ inline
#else
#define KM_S1G_FN inline
#endif

namespace km {

constexpr float S1G_U = 5.9604644775390625e-08f;  // 2^-24
constexpr float S1G_TINY = 1e-30f;

KM_S1G_FN float s1g_up(float v) { return fmaf(fabsf(v), 8.0f * S1G_U, v) + S1G_TINY; }
KM_S1G_FN float s1g_dn(float v) { return fmaf(fabsf(v), -8.0f * S1G_U, v) - S1G_TINY; }

// square root within 2 ulp (4 u): v_sqrt_f32 on the device, sqrtf on the host
KM_S1G_FN float s1g_sqrt(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sqrtf(v);
#else
  return sqrtf(v);
#endif
}

// ||c' - c|| rounded up to float from its float64 square (the sum's
// roundings, (d + 2) 2^-53 relative, and the square root's are far inside the
// 1e-12; the float conversion's half ulp is inside the 2^-23).  Non-finite
// squares (a NaN centroid) give +inf: every row is listed.
KM_S1G_FN float s1g_shift(double sq) {
  const double v = sqrt(sq) * (1.0 + 1e-12);
  const float f = (float)v;
  const float r = fmaf(f, 0x1p-23f, f) + S1G_TINY;
  return (r <= 3.0e38f) ? r : INFINITY;
}

// one gate step: the margin after the centroids moved (sl: the row's own
// centroid's shift, so: the largest shift of any other centroid)
KM_S1G_FN float s1g_step(float marg, float sl, float so) { return s1g_dn(marg - s1g_up(sl + so)); }

// A row's constants for turning screen keys into distances.  The screen's
// keys are K~ = s^2 (||c||^2 - 2 c.x) + e, |e| <= E, further perturbed by the
// id packing (relative rp), so s^2 ||x - c||^2 = K + s^2 ||x||^2 lies within
// rp |K~| + E of K~ + s^2 ||x||^2.  Everything below is in unscaled units
// (s is a power of two: is2 = 1 / s^2 is exact).
struct S1GRow {
  float is2;  // 1 / s^2
  float E;    // screen error bound, unscaled squared-distance units, rounded up
  float xlo;  // lower bound of ||x||^2
  float xhi;  // upper bound of ||x||^2
};

// xs: the fp32 sum of the row's squares, at most 64 roundings (row length up
// to 128 over four lanes: 32 fused steps and the quad's two additions)
KM_S1G_FN S1GRow s1g_row(float s, float E_scaled, float xs) {
  S1GRow r;
  r.is2 = 1.0f / (s * s);
  r.E = s1g_up(E_scaled * r.is2);
  r.xhi = s1g_up(xs * (1.0f + 64.0f * S1G_U));
  r.xlo = s1g_dn(xs * (1.0f - 64.0f * S1G_U));
  return r;
}

// the scale is usable: is2 and the products with it stay normal numbers for
// every key the screen can hold (|key| < 2^14 s ... 2^29 s^2)
KM_S1G_FN bool s1g_scale_ok(float s) { return s >= 0x1p-30f && s <= 0x1p30f; }

// upper bound of ||x - c|| for a centroid whose packed key is <= key
KM_S1G_FN float s1g_ub(float key, float rp, const S1GRow& r) {
  const float p = key * r.is2;
  float v = s1g_up(p + s1g_up(rp * fabsf(p)));
  v = s1g_up(v + r.E);
  v = s1g_up(v + r.xhi);
  v = !(v < 0x1p-96f) ? v : 0x1p-96f;  // (NaN stays NaN; below 2^-96 the hardware root loses accuracy)
  return s1g_up(s1g_up(s1g_sqrt(v)));
}

// lower bound of ||x - c|| for every centroid whose packed key is >= key
KM_S1G_FN float s1g_lb(float key, float rp, const S1GRow& r) {
  const float p = key * r.is2;
  float v = s1g_dn(p - s1g_up(rp * fabsf(p)));
  v = s1g_dn(v - r.E);
  v = s1g_dn(v + r.xlo);
  return (v >= 0x1p-96f) ? s1g_dn(s1g_dn(s1g_sqrt(v))) : 0.0f;  // (NaN: 0, always a lower bound)
}

// lb - ub rounded down; anything non-finite becomes 0 (the row is screened
// again at the next pass)
KM_S1G_FN float s1g_margin(float lb, float ub) {
  const float m = s1g_dn(lb - ub);
  return (fabsf(m) <= 3.0e38f) ? m : 0.0f;
}

// --- accumulated-drift form -------------------------------------------------
// one pass's step added to a cluster's running total (sl: its own shift, so:
// the largest shift of any other centroid; both >= 0 or +inf from s1g_shift).
// The two float64 additions lose at most 2^-52 relative, the factor puts back
// 2^-50: the result is >= the real sum.  +inf (and NaN) stay non-finite
KM_S1G_FN double s1g_acc_add(double acc, float sl, float so) {
  return (acc + ((double)sl + (double)so)) * (1.0 + 0x1p-50);
}
// acc as a float from above: the conversion's half ulp is inside the 2^-23
// (s1g_shift's form); anything non-finite or beyond the float range: +inf
KM_S1G_FN float s1g_acc_up(double acc) {
  const float f = (float)acc;
  const float r = fmaf(f, 0x1p-23f, f) + S1G_TINY;
  return (r <= 3.0e38f) ? r : INFINITY;
}
// acc as a float from below (f - f 2^-23 is at least one ulp under f, which is
// within half an ulp of acc), never negative; non-finite acc: 0, a lower bound
KM_S1G_FN float s1g_acc_dn(double acc) {
  if (!(acc <= 3.0e38)) return 0.0f;
  const float f = (float)acc;
  const float r = fmaf(f, -0x1p-23f, f) - S1G_TINY;
  return r > 0.0f ? r : 0.0f;
}
// one cluster's total over one gated pass, with the two images published for
// it (k_s1_shift runs this per cluster).  sl, so as in s1g_acc_add; top: the
// pass's largest shift.  `reset`: every margin is rewritten by the pass (the
// dense sweep): a new epoch, acc = 0.  A non-finite top shift also starts a
// new epoch, but with the upper image +inf for this pass: the gate lists
// every row, every listed row gets a new base against the lower image 0, and
// the totals are finite again afterwards (as a stepped margin would be).
// A large FINITE shift does not: it stays in acc until the next dense sweep,
// and from then on a row is kept only while its fresh margin exceeds the
// width acc_up - acc_dn, about two float ulps of acc.  That is always safe,
// but a move that is huge against the data's scale (1e30, say) leaves every
// row listed at every pass until new centroids or rows start a new epoch,
// where a stepped margin recovered after one pass.  Lloyd's own moves shrink,
// and acc stays within a small multiple of the first moves
KM_S1G_FN double s1g_acc_pass(double acc, float sl, float so, float top, bool reset, float* up, float* dn) {
  const bool wild = !(top <= 3.0e38f);
  const double a = (reset || wild) ? 0.0 : s1g_acc_add(acc, sl, so);
  *up = (wild && !reset) ? INFINITY : s1g_acc_up(a);
  *dn = s1g_acc_dn(a);
  return a;
}
// what a decided row stores: its fresh margin (s1g_margin: finite) plus the
// lower total of its label, rounded down; 0 (listed next time) if that is not
// a finite number
KM_S1G_FN float s1g_base(float marg, float acc_dn) {
  const float b = s1g_dn(marg + acc_dn);
  return (fabsf(b) <= 3.0e38f) ? b : 0.0f;
}
// the gate's test: the row keeps its label and is not screened
KM_S1G_FN bool s1g_keep(float base, float acc_up) { return base > acc_up; }

// upper bound of ||x|| from the fp32 sum of the row's squares (s1g_row's xhi,
// the root rounded up twice as in s1g_ub); NaN stays NaN, overflow gives +inf
KM_S1G_FN float s1g_xnorm(float xs) {
  float v = s1g_up(xs * (1.0f + 64.0f * S1G_U));
  v = !(v < 0x1p-96f) ? v : 0x1p-96f;
  return s1g_up(s1g_up(s1g_sqrt(v)));
}

}  // namespace km
