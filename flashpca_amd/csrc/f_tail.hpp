// f_tail.hpp -- the upper tail of the F distribution for UCCA (RandomPCA::ucca -> wilks, randompca.cpp:103-119, where Boost's
// fisher_f supplies it), as ONE __host__ __device__ source: the finishing kernel of ucca.hip runs it per SNP, and the host build of
// the same code is exported as fpca_debug_f_sf for the CPU suite (fpca_debug_f_sf_dev runs the device build on a grid of r2).
//
// With r2 the squared multiple correlation of a SNP on k phenotypes and n samples, F = r2 / (1 - r2) (n - k - 1) / k and
//   P = Pr[F(k, n - k - 1) > F] = I_{1 - r2}(a, b),   a = (n - k - 1) / 2,  b = k / 2,
// the regularised incomplete beta function, evaluated from r2 itself and never through F: the logarithms of both arguments come
// from log(r2) and log1p(-r2).  The method is the classical one: the prefactor x^a y^b / (a B(a, b)) in log space, the continued
// fraction by the modified Lentz algorithm, and the symmetry I_x(a, b) = 1 - I_y(b, a) on the side of the mean where the fraction
// would converge slowly.  The one refinement: with a in the hundreds of thousands, lgamma(a + b) - lgamma(a) is taken from the
// difference of the Stirling series rather than as a difference of two numbers near 10^7, so the PREFACTOR keeps its relative
// accuracy (~1e-13) all the way down to the smallest normal P.  Below ~1e-300 P underflows to 0.
//
// What holds for P as a whole, against scipy's betaincc(k/2, (n-k-1)/2, r2) wherever that is >= 1e-290, k <= 256 (the table
// tests/test_gpu_f_tail.py prints, the device build on the MI355X and the host build alike; the tests assert 1e-8):
//     n <= 10: 1.9e-14     n = 957: 2.5e-13     n = 500,000: 3.1e-11     n = 1,000,000: 6.4e-11 (k = 1, r2 = 4.4e-6, P = 0.036)
// The loss at large n is not the prefactor's.  It sits on the I_x(a, b) side of the switch (x = 1 - r2 < (a + 1) / (a + b + 2)), just
// above it -- r2 of a few k / n, where most SNPs of a large scan lie: the FRACTION there receives the rounded 1.0 - r2, a relative
// error of eps / r2 in y = r2, and carries it into P.  Making the first Lentz term cancellation-free repairs k = 2 alone; a fraction
// re-derived in y would repair the rest and has not been done.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FPCA_HD __host__ __device__
#else
#define FPCA_HD
#endif

namespace fpca {
namespace ftail {

// lgamma(z) - [(z - 1/2) ln z - z + ln(2 pi) / 2], z >= 10: the asymptotic series to the z^-13 term (next term < 4e-17 there)
FPCA_HD inline double stirling_corr(double z)
{
   const double r = 1.0 / z, r2 = r * r;
   return r * (1.0 / 12 + r2 * (-1.0 / 360 + r2 * (1.0 / 1260 + r2 * (-1.0 / 1680 + r2 * (1.0 / 1188 + r2 * (-691.0 / 360360 + r2 * (1.0 / 156)))))));
}

// -ln B(a, b) = lgamma(a + b) - lgamma(a) - lgamma(b)
FPCA_HD inline double neg_lbeta(double a, double b)
{
   const double big = a > b ? a : b, sml = a > b ? b : a;
   if (big < 10.0) return lgamma(a + b) - lgamma(a) - lgamma(b);
   // lgamma(big + sml) - lgamma(big) from the two Stirling series: no cancellation between numbers of size big ln big
   const double d = (big - 0.5) * log1p(sml / big) + sml * log(big + sml) - sml + stirling_corr(big + sml) - stirling_corr(big);
   return d - lgamma(sml);
}

// continued fraction of I_x(a, b) (x < (a + 1) / (a + b + 2)), modified Lentz.  Two details keep its cost what the mathematics
// says it is.  The stopping tolerance is a few ulps of 1, not less than one: below one ulp (doubles just above 1 are 2.2e-16 apart) the
// test demands del == 1 exactly, and under fused multiply-adds the factor dithers an ulp or two around 1 instead -- lanes of the
// finishing kernel then ran on for thousands of iterations.  And the recurrence is evaluated without contraction, on the device as on the
// host, so that the host build the CPU suite checks (fpca_debug_f_sf) runs the same arithmetic: with fused multiply-adds, x near 1
// and a large (aa near -1), the factors stall at the 1e-13 level for thousands of iterations after h has converged.  So evaluated,
// the fraction stops within ~60 iterations for n <= 10^6, k <= 256, and within 12 near the null at n = 5e5, k = 10; the cap only
// bounds a runaway.
FPCA_HD inline double betacf(double a, double b, double x)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
   const double tiny = 1e-300, eps = 1e-15;
   const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
   double c = 1.0, d = 1.0 - qab * x / qap;
   if (fabs(d) < tiny) d = tiny;
   d = 1.0 / d;
   double h = d;
   for (int m = 1; m <= 2000; m++) {
      const double m2 = 2.0 * m;
      double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
      d = 1.0 + aa * d;
      if (fabs(d) < tiny) d = tiny;
      c = 1.0 + aa / c;
      if (fabs(c) < tiny) c = tiny;
      d = 1.0 / d;
      h *= d * c;
      aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
      d = 1.0 + aa * d;
      if (fabs(d) < tiny) d = tiny;
      c = 1.0 + aa / c;
      if (fabs(c) < tiny) c = tiny;
      d = 1.0 / d;
      const double del = d * c;
      h *= del;
      if (fabs(del - 1.0) <= eps) break;
   }
   return h;
}

// I_x(a, b) with y = 1 - x given exactly through its logarithm: lx = ln x, ly = ln y
FPCA_HD inline double ibeta_cf(double a, double b, double x, double lx, double ly)
{
   const double lpre = a * lx + b * ly + neg_lbeta(a, b) - log(a);
   return exp(lpre) * betacf(a, b, x);
}

// F statistic and its upper-tail probability for r2 on n samples and k phenotypes (k >= 1, n >= k + 2).
//   r2 <= 0: F = 0, P = 1;  r2 >= 1: F = +inf, P = 0;  NaN r2: NaN, NaN.
FPCA_HD inline void f_sf(double r2, uint64_t n, int k, double *F, double *P)
{
   const double d2 = (double)(n - (uint64_t)k - 1), d1 = (double)k;
   if (!(r2 == r2)) {
      *F = r2;
      *P = r2;
      return;
   }
   if (r2 >= 1.0) {
      *F = INFINITY;
      *P = 0.0;
      return;
   }
   if (r2 <= 0.0) {
      *F = 0.0;
      *P = 1.0;
      return;
   }
   *F = r2 / (1.0 - r2) * d2 / d1;
   const double a = 0.5 * d2, b = 0.5 * d1;
   const double lx = log1p(-r2), ly = log(r2); // x = 1 - r2, y = r2
   if (1.0 - r2 < (a + 1.0) / (a + b + 2.0))
      *P = ibeta_cf(a, b, 1.0 - r2, lx, ly);
   else
      *P = 1.0 - ibeta_cf(b, a, r2, ly, lx);
}

} // namespace ftail
} // namespace fpca
