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
// Plain C++ (no HIP headers): tests/test_host_s1_gate.py compiles it into a
// host program and checks the certificate in float64.
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

}  // namespace km
