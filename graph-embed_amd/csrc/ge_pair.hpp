// ge_pair.hpp -- per-pair / per-edge ForceAtlas terms shared by the kernels.
//
// Each function evaluates one term of include/forceatlas.hpp exactly as the
// reference writes it (operand order, one rounding per operation).  With
// SHARED = true the three divisions by one denominator reuse its reciprocal
// (ge_math.hpp): same instructions, same bits, valid when the caller has checked
// coord_ok() for every coordinate involved.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "ge_dims.hpp"
#include "ge_internal.hpp"
#include "ge_math.hpp"

namespace ge {

constexpr double kFaEps = 0.00001;  // include/forceatlas.hpp:110, :337

struct FaConst {
  double ks_gS;  // ks * globalSpeed, globalSpeed = tolerate * 1.0 / 1.0 (:228, :242, :244)
  double gS;
  double ksmax, repel, attract, gravity, delta;
  int use_weights, linlog, nohubs;
};

inline FaConst make_fa_const(const ge_fa_params& p) {
  FaConst c;
  c.gS = p.tolerate * 1.0 / 1.0;
  c.ks_gS = p.ks * c.gS;
  c.ksmax = p.ksmax;
  c.repel = p.repel;
  c.attract = p.attract;
  c.gravity = p.gravity;
  c.delta = p.delta;
  c.use_weights = p.use_weights;
  c.linlog = p.linlog;
  c.nohubs = p.nohubs;
  return c;
}

__device__ __forceinline__ double clamp_eps(double x) { return x < kFaEps ? kFaEps : x; }

// Attraction magnitude (:176-196).  linlog / delta != 1 use device log / pow
// (ocml), which may differ from glibc in the last ulp: only the default branch
// is bit-exact.
__device__ __forceinline__ double attraction_mag(double dis, double a, double dip1,
                                                 const FaConst& c) {
  double f = dis;
  if (c.linlog) f = log(1 + f);
  if (c.delta == 1.0) {
    f = f * a;
  } else if (c.delta != 0.0) {
    const double sgn = (a < 0) ? -1.0 : 1.0;
    const double mg = (a < 0) ? -a : a;
    f = sgn * pow(mg, c.delta) * f;
  }
  if (c.nohubs) f = f / dip1;
  return c.attract * f;
}

// The clamped distance of a pair and the refined reciprocals of dis and dis^2
// (round 5).  The IEEE quotient n / d the kernels replay (ge_math.hpp div_by) is
// q0 = n y, r = fma(-d, q0, n), q0 + r y rounded once: its result is the correctly
// rounded n / d for any y within a fraction of an ulp of 1 / d (q0 + r y = n / d +
// (d y - 1)(n / d - q0), an error of ~2^-106 relative), and recip_of gets such a y
// from v_rcp_f64 and two Newton steps.  Here the reciprocals come without v_rcp:
//   1 / dis   from the sqrt's own Goldschmidt half-reciprocal h1 ~ 1 / (2 sqrt(s))
//             (one Newton step of v_rsq_f64 already), y0 = 2 h1 (capped at 1e5 ~ 1 /
//             eps: s below eps^2, or s = 0 where h1 is NaN and fmin takes 1e5), then
//             one Newton step: y = y0 + y0 (1 - dis y0);
//   1 / dis^2 from (1 / dis)^2 (within ~2 ulp), then one Newton step.
// Each y is then within 2^-80 of 1 / d before its last rounding, like recip_of's (its
// second Newton step starts from ~2^-44), so the two differ only where 1 / d lies
// within ~2^-80 of a rounding boundary, and a y off by one ulp changes the quotient
// only where n / d lies within ~2^-106 of one.  For random operands that is a
// probability of ~2^-80 per division (ge_selftest.hip compares every term with the rcp
// path and with `/` on 2^30 draws per test call, tests/test_gpu_parity.py); for
// structured ones it is not: a denominator whose significand is all ones,
// d = 2^k (2 - 2^-52), has 1 / d = 2^-k-1 (1 + 2^-53 + 2^-106 ...), 2^-106 above the
// boundary between 2^-k-1 and the double after it.  A Newton step reaches 1 / d from
// below, so it lands under the boundary and rounds to the power of two, and with
// that y every numerator that is a power of two gets the quotient one ulp low
// (n y exact, remainder n 2^-53, an exact tie rounded to even).  This is the known
// exception of the correction step (Markstein): with y = RN(1 / d) the quotient is
// correctly rounded for every numerator, and a Newton step yields RN(1 / d) except
// for this d.  Measured on an MI355X
// (tests/test_gpu_math_exact.py, exact references from tests/math_cases.py): the
// uncorrected pair_den missed exactly these, 1 098 of 144 447 directed (s, n, c) cases
// -- the nine all-ones distances times the 122 power-of-two numerators -- while
// v_rcp_f64 + two steps (recip_of) and the compiler's `/` and sqrt missed none of
// 599 375 quotients and 1 612 roots.  Distances of that form are reachable from
// coordinates (e = (0.5, 0x1.bb67ae8584caap-1) has |e| = 1 - 2^-53).  pair_den
// therefore sets y to RN(1 / d) when d's significand is all ones (three
// instructions per pair).  dis^2 cannot take that form (no double's rounded square
// has an all-ones significand), so 1 / dis^2 needs no such step.  Two quarter-rate
// v_rcp_f64 and two FMAs fewer per pair than rcp-based reciprocals.
struct PairDen {
  double dis;
  Recip rdis, rdd;  // {dis, ~1/dis}, {dis * dis, ~1/dis^2}
};
// sqrt_normal(s) (ge_math.hpp: the same sequence) that also hands out its Goldschmidt
// half-reciprocal h1 ~ 1 / (2 sqrt(s)).  NaN for s == 0.  NEG: -sqrt_normal(s) from the
// last fma with both addends negated -- the same rounding of the negated sum, so the
// negated bits for every s > 0 -- for callers that only ever use the root negated.
template <bool NEG = false>
__device__ __forceinline__ double sqrt_half_recip(double s, double& h1) {
  const double y = __builtin_amdgcn_rsq(s);
  const double g0 = s * y;
  const double h0 = y * 0.5;
  const double r0 = __builtin_fma(-h0, g0, 0.5);
  h1 = __builtin_fma(h0, r0, h0);
  const double g1 = __builtin_fma(g0, r0, g0);
  const double d0 = __builtin_fma(-g1, g1, s);
  const double g2 = __builtin_fma(d0, h1, g1);
  const double d1 = __builtin_fma(-g2, g2, s);
  return NEG ? __builtin_fma(-d1, h1, -g2) : __builtin_fma(d1, h1, g2);
}

// pair_den from the unclamped root g3 and h1: the clamps, the Newton steps and the
// all-ones correction.
__device__ __forceinline__ PairDen pair_den_from(double g3, double h1) {
  // sqrt_normal(s), clamped (s == 0: NaN, and fmax takes eps)
  const double dis = fmax(g3, kFaEps);
  const double y0 = fmin(h1 + h1, 1e5);
  const double yd = __builtin_fma(y0, __builtin_fma(-dis, y0, 1.0), y0);
  const double dd = dis * dis;
  const double z0 = yd * yd;
  const double ydd = __builtin_fma(z0, __builtin_fma(-dd, z0, 1.0), z0);
  // The structured exception (header comment): dis = 2^k (2 - 2^-52), significand all
  // ones.  Its reciprocal 2^-k-1 (1 + 2^-53 + 2^-106 ...) lies 2^-106 above a rounding
  // boundary and the Newton step arrives from below, so yd came out as the power of two
  // 2^-k-1 where RN(1 / dis) is the double above it: low word 1, high word as computed.
  const bool ones = __builtin_amdgcn_frexp_mant(dis) == 0x1.fffffffffffffp-1;
  const double yr = __hiloint2double(__double2hiint(yd), ones ? 1 : __double2loint(yd));
  return PairDen{dis, Recip{dis, yr}, Recip{dd, ydd}};
}
__device__ __forceinline__ PairDen pair_den(double s) {
  double h1;
  const double g3 = sqrt_half_recip(s, h1);
  return pair_den_from(g3, h1);
}

// pair_den in detect-then-fix form (round 14): the same bits, five instructions fewer
// per pair where no lane of the wave needs them.  Of pair_den's instructions the two
// clamps (fmax, fmin) and the all-ones correction (frexp_mant, compare, select) change
// a bit only for a pair closer than eps (or coincident: g3 NaN) and for a distance
// whose significand is all ones.  Here each lane computes the unclamped, uncorrected
// values and two flags,
//   low    !(g3 >= kFaDetect), kFaDetect = eps (1 + 2^-20): true for NaN too;
//   ones   the low word of g3 is 0xFFFFFFFF: necessary for an all-ones significand
//          (true by chance for one distance in 2^32),
// and when any lane of the wave has one set (a wave-uniform branch on the two compare
// masks: no exec-mask divergence, `fixed` reports it), every lane takes
// pair_den_from(g3, h1) instead -- pair_den's own code on pair_den's own g3 and h1,
// hence its bits.  A lane with neither flag set gets pair_den's bits without it,
// because every instruction left out was an identity for it:
//   fmax   g3 >= kFaDetect > eps and g3 is not NaN, so fmax(g3, eps) = g3;
//   fmin   h1 is one Newton step of v_rsq_f64, 2 h1 = (1 + d) / sqrt(s) with |d| far
//          below 2^-21 (the step squares the estimate's error: the bound holds for
//          any estimate good to 2^-11, and v_rsq_f64's is ~2^-26), and g3 =
//          RN(sqrt(s)) >= eps (1 + 2^-20) gives sqrt(s) >= eps (1 + 2^-20)(1 - 2^-53),
//          so 2 h1 <= (1 / eps)(1 + 2^-21)(1 + 2^-52) / (1 + 2^-20) < 1e5 (1 - 2^-22)
//          with eps = RN(1e-5) within 2^-53 of 1e-5: fmin(2 h1, 1e5) = 2 h1.  (At
//          g3 == eps itself the margin is not clean -- 2 h1 may exceed 1e5 by an ulp
//          -- which is why the flag is wider than the clamp);
//   select the low word is not all ones, so the significand is not: yr = yd.
// The rare block rewrites the four results in place and nothing else stays live for
// it but g3 and h1.  (Measured and not kept, DESIGN.md 5i: the compares issued with the
// reciprocals, the masks held in scalar registers through the quotients and the branch
// after the term's last multiply, the rare block redoing the whole term -- the wave
// then never waits for its flags, and it ran 0.3-0.7 ms slower than the branch right
// after the root.)  Callers: the sweeps' tile_steps (ge_sym.hpp), whose rows never meet
// themselves.  A kernel in which every row meets its own column in each block (the
// diagonal tiles, the resident, packed and one-workgroup kernels) would take the
// branch every time and keeps pair_den.
constexpr double kFaDetect = kFaEps * (1.0 + 0x1p-20);
// Every use of the two denominators is a negated one (the Newton steps, div_by_nz's
// remainders fma(-d, q, n)), so this form keeps them negated: ndis = -dis from the
// root's last fma with both addends negated, ndd = ndis * -ndis.  (With dis itself
// joined across a branch the compiler copied -dis into a second register pair on the
// common path, two moves per pair.)
struct PairDenNeg {
  double ndis, yd, ndd, ydd;  // -dis, ~1/dis, -(dis * dis), ~1/dis^2
};
// div_by_nz(num, Recip{-nd, y}): the same instructions.
__device__ __forceinline__ double div_by_nz_neg(double num, double nd, double y) {
  const double q = num * y;
  const double rem = __builtin_fma(nd, q, num);
  return __builtin_fma(rem, y, q);
}
__device__ __forceinline__ PairDenNeg pair_den_detect(double s, bool& fixed) {
  double h1;
  const double ng3 = sqrt_half_recip<true>(s, h1);
  const double y0 = h1 + h1;
  const double yd = __builtin_fma(y0, __builtin_fma(ng3, y0, 1.0), y0);
  const double ndd = ng3 * -ng3;
  const double z0 = yd * yd;
  const double ydd = __builtin_fma(z0, __builtin_fma(ndd, z0, 1.0), z0);
  PairDenNeg pn{ng3, yd, ndd, ydd};
  const bool low = !(ng3 <= -kFaDetect);
  const bool ones = __double2loint(ng3) == -1;
  fixed = __builtin_amdgcn_ballot_w64(low || ones) != 0;
  if (__builtin_expect(fixed, 0)) {
    const PairDen pd = pair_den_from(-ng3, h1);
    pn = PairDenNeg{-pd.dis, pd.rdis.y, -pd.rdd.ds, pd.rdd.y};
    // opaque: keeps this block a plain out-of-line detour that rewrites the four
    // values in place (without it the join came out with two register copies)
    asm volatile("" : "+v"(pn.ndis), "+v"(pn.ndd));
  }
  return pn;
}

// Repulsion of j on i (:152-166): the term added to row i's sum, out[k] =
// (e_k / dis) * val.  e = x_i - x_j equals -(x_j - x_i) up to the sign of zero,
// and a zero term never changes the sum (see ge_fa.hip); the j == i term is
// +-0 for the same reason.  DETECT (with SHARED): the detect-then-fix form of the
// denominators (pair_den_detect), and *fixed says whether the wave took its fix-up.
template <int D, bool SHARED, bool REPEL_ONE, bool DETECT = false>
__device__ __forceinline__ void rep_term(const double (&xi)[D], const double* __restrict__ xj,
                                         double dip1, double djp1, double repel,
                                         double (&out)[D], bool* fixed = nullptr) {
  static_assert(SHARED || !DETECT, "the detect-then-fix form is a shared-reciprocal form");
  double e[D];
#pragma unroll
  for (int k = 0; k < D; ++k) e[k] = xi[k] - xj[k];
  double s = e[0] * e[0];
#pragma unroll
  for (int k = 1; k < D; ++k) s = s + e[k] * e[k];
  double cij = dip1 * djp1;
  if (!REPEL_ONE) cij = cij * repel;
  if (SHARED) {
    // In-domain s is 0 or >= 2^-504 (>= 2^-767: sqrt_normal is exact).  For
    // s == 0 (the j == i pair, coincident points) sqrt_normal returns NaN
    // (rsq(0) = inf, 0 * inf), and fmax returns its non-NaN operand, so dis is
    // eps exactly as the reference's clamp of sqrt(0) = 0.
#ifdef GE_PAIR_RCP  // A/B variant builds only (scripts/build_variant.sh): recip_of's reciprocals
    const double dis = fmax(sqrt_normal(s), kFaEps);
    const double val = div_by_nz(cij, recip_of(dis * dis));
    const Recip rdis = recip_of(dis);
#pragma unroll
    for (int k = 0; k < D; ++k) out[k] = div_by_nz(e[k], rdis) * val;
#else
    if (DETECT) {
      bool fx;
      const PairDenNeg pn = pair_den_detect(s, fx);
      if (fixed) *fixed = fx;
      const double val = div_by_nz_neg(cij, pn.ndd, pn.ydd);
#pragma unroll
      for (int k = 0; k < D; ++k) out[k] = div_by_nz_neg(e[k], pn.ndis, pn.yd) * val;
    } else {
      const PairDen pd = pair_den(s);
      const double val = div_by_nz(cij, pd.rdd);  // cij > 0 in-domain
#pragma unroll
      for (int k = 0; k < D; ++k) out[k] = div_by_nz(e[k], pd.rdis) * val;
    }
#endif
  } else {
    const double dis = clamp_eps(sqrt(s));
    const double val = cij / (dis * dis);
#pragma unroll
    for (int k = 0; k < D; ++k) out[k] = (e[k] / dis) * val;
  }
}

// rep_term<SHARED> with recip_of's reciprocals (the form before round 5): the
// selftest's reference for pair_den.
template <int D, bool REPEL_ONE>
__device__ __forceinline__ void rep_term_rcp(const double (&xi)[D], const double* __restrict__ xj,
                                             double dip1, double djp1, double repel,
                                             double (&out)[D]) {
  double e[D];
#pragma unroll
  for (int k = 0; k < D; ++k) e[k] = xi[k] - xj[k];
  double s = e[0] * e[0];
#pragma unroll
  for (int k = 1; k < D; ++k) s = s + e[k] * e[k];
  double cij = dip1 * djp1;
  if (!REPEL_ONE) cij = cij * repel;
  const double dis = fmax(sqrt_normal(s), kFaEps);
  const double dd = dis * dis;
  const double val = div_by_nz(cij, recip_of(dd));
  const Recip rc = recip_of(dis);
#pragma unroll
  for (int k = 0; k < D; ++k) out[k] = div_by_nz(e[k], rc) * val;
}

// rep_term added to acc.  Every sum that receives terms starts from a +0.0
// accumulator and is never seeded with a term: a term may be -0 (e_k = -0), and
// only the +0 start makes adding it an identity (RN: +0 + -0 = +0).
template <int D, bool SHARED, bool REPEL_ONE>
__device__ __forceinline__ void rep_pair(const double (&xi)[D], const double* __restrict__ xj,
                                         double dip1, double djp1, double repel,
                                         double (&acc)[D]) {
  double t[D];
  rep_term<D, SHARED, REPEL_ONE>(xi, xj, dip1, djp1, repel, t);
#pragma unroll
  for (int k = 0; k < D; ++k) acc[k] = acc[k] + t[k];
}

// The out-of-domain (`/`) form with the self pair skipped as the reference does
// (j != i, :151).  In the shared-reciprocal domain the self term is +-0 and may
// be accumulated, but outside it cij / eps^2 can overflow (cij > ~1.8e298) and
// 0 * inf would put a NaN into the row's sum.
template <int D, bool REPEL_ONE>
__device__ __forceinline__ void rep_pair_fb(const double (&xi)[D], const double* __restrict__ xj,
                                            double dip1, double djp1, double repel, bool self,
                                            double (&acc)[D]) {
  if (!self) rep_pair<D, false, REPEL_ONE>(xi, xj, dip1, djp1, repel, acc);
}

// FAST mode's repulsion of j on i in closed form, added to row i's sum:
// acc_k = fma(e_k, w, acc_k), e = x_i - x_j, w = dir * djp1 * y^3, with
// y = 1 / max(|e|, eps) from v_rsq_f64 and two Newton steps; dir is the row's
// (deg + 1) * repel.  s == 0 (the self pair, coincident members) gives rsq = inf,
// NaN after the Newton steps, and fmin takes 1 / eps; e = 0 then makes the term 0.
// Members closer than eps are clamped the same way (the reference's clamp_eps).
// Every multiply-add is an explicit fma and nothing else can contract, so a row's
// sum over partners j = 0, 1, ... has the same bits in every kernel that calls this
// in that order (fa_repulse_fast, ge_fa.hip; faml_fast_repulse, ge_faml.hip).
template <int D>
__device__ __forceinline__ void fast_rep_pair(const double (&xi)[D], const double (&xj)[D],
                                              double dir, double djp1, double (&acc)[D]) {
  constexpr double inv_eps = 1.0 / kFaEps;
  double e[D];
#pragma unroll
  for (int k = 0; k < D; ++k) e[k] = xi[k] - xj[k];
  double s = e[0] * e[0];
#pragma unroll
  for (int k = 1; k < D; ++k) s = fma(e[k], e[k], s);
  double y = __builtin_amdgcn_rsq(s);
  const double hs = 0.5 * s;
  y = y * fma(-hs * y, y, 1.5);
  y = y * fma(-hs * y, y, 1.5);
  y = fmin(y, inv_eps);
  const double w = dir * djp1 * (y * y * y);
#pragma unroll
  for (int k = 0; k < D; ++k) acc[k] = fma(e[k], w, acc[k]);
}

// attraction_mag for linlog == 0 and delta == 1 (the defaults): no log / pow
// code, which keeps register-tight kernels within their budget.
__device__ __forceinline__ double attraction_mag_linear(double dis, double a, double dip1,
                                                        const FaConst& c) {
  double f = dis * a;
  if (c.nohubs) f = f / dip1;
  return c.attract * f;
}

// Attraction along one CSR entry (:169-203): t = x_j - x_i.  LINEAR: the caller
// guarantees linlog == 0 and delta == 1.
template <int D, bool SHARED, bool LINEAR = false>
__device__ __forceinline__ void attr_edge(const double (&xi)[D], const double* __restrict__ xj,
                                          double a, double dip1, const FaConst& c,
                                          double (&acc)[D]) {
  double t[D];
#pragma unroll
  for (int k = 0; k < D; ++k) t[k] = xj[k] - xi[k];
  double s = t[0] * t[0];
#pragma unroll
  for (int k = 1; k < D; ++k) s = s + t[k] * t[k];
  const double dis = clamp_eps(SHARED ? (s == 0.0 ? 0.0 : sqrt_normal(s)) : sqrt(s));
  const double Fa = LINEAR ? attraction_mag_linear(dis, a, dip1, c) : attraction_mag(dis, a, dip1, c);
  if (SHARED) {
    const Recip rc = recip_of(dis);
#pragma unroll
    for (int k = 0; k < D; ++k) acc[k] = acc[k] + div_by(t[k], dis, rc) * Fa;
  } else {
#pragma unroll
    for (int k = 0; k < D; ++k) acc[k] = acc[k] + (t[k] / dis) * Fa;
  }
}

template <int D>
__device__ __forceinline__ bool all_coord_ok(const double* x) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < D; ++k) ok = ok && coord_ok(x[k]);
  return ok;
}

// A vertex whose coordinates and deg+1 lie in the exact shared-reciprocal
// domain of rep_pair<SHARED = true>.
template <int D>
__device__ __forceinline__ bool vertex_ok(const double* x, double dp1) {
  return all_coord_ok<D>(x) && weight_ok(dp1);
}

// -x_k / mag for all k (:208 single level, :471 multilevel).
template <int D>
__device__ __forceinline__ void neg_over(const double (&x)[D], double mag, double (&out)[D]) {
  double nx[D];
#pragma unroll
  for (int k = 0; k < D; ++k) nx[k] = -x[k];
  if (exact_den(mag) && all_coord_ok<D>(x)) {
    const Recip rc = recip_of(mag);
#pragma unroll
    for (int k = 0; k < D; ++k) out[k] = div_by(nx[k], mag, rc);
  } else {
#pragma unroll
    for (int k = 0; k < D; ++k) out[k] = nx[k] / mag;
  }
}

// The wide schedule (ge_dims.hpp: kNarrowMaxDim) from this dimension up.
inline bool wide_dim(int dim) {
  int lo = kNarrowMaxDim + 1;
  if (const char* e = std::getenv("GE_WIDE_MIN_DIM")) lo = std::min(lo, std::max(1, std::atoi(e)));
  return dim >= lo;
}

#define GE_DIM_CASE(N) \
  case N: f(std::integral_constant<int, N>()); break;

template <class F>
void dispatch_dim(int dim, F&& f) {
  switch (dim) {
    GE_DIM_CASE(1) GE_DIM_CASE(2) GE_DIM_CASE(3) GE_DIM_CASE(4)
    GE_DIM_CASE(5) GE_DIM_CASE(6) GE_DIM_CASE(7) GE_DIM_CASE(8)
    GE_DIM_CASE(9) GE_DIM_CASE(10) GE_DIM_CASE(11) GE_DIM_CASE(12)
    GE_DIM_CASE(13) GE_DIM_CASE(14) GE_DIM_CASE(15) GE_DIM_CASE(16)
    default: throw Error(GE_ERR_ARG, "dimension must be 1..16");
  }
}

// The schedules compiled for D <= kNarrowMaxDim only (callers check wide_dim first).
template <class F>
void dispatch_dim_narrow(int dim, F&& f) {
  switch (dim) {
    GE_DIM_CASE(1) GE_DIM_CASE(2) GE_DIM_CASE(3) GE_DIM_CASE(4)
    default: throw Error(GE_ERR_STATE, "this schedule is built for dimensions 1..4 only");
  }
}

}  // namespace ge
