"""CPU checks of the step loop's trimmed arithmetic (swrt_kernels.hpp), as
small C programs built with -O2 -ffp-contract=off and fma(), in the style of
tests/test_divconst.py:

* lagrange_wi with kScale<I> carried by the running product (its magnitude in
  the constants of one Markstein step, its sign on the last multiply) against
  the trailing-multiply form, bit for bit, zero signs included;
* cell_frac's short paths (exact reciprocal of a power-of-two period, one
  wrap for iperiod == nx) against the general path."""
import subprocess

WEIGHTS = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
static uint64_t s = 0x2545F4914F6CDD1Dull;
static uint64_t nxt(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static int oddp(int d) { d = d < 0 ? -d : d; while (d % 2 == 0) d /= 2; return d; }
static double scl(int d) { double c = d < 0 ? -1.0 : 1.0; d = d < 0 ? -d : d; while (d % 2 == 0) { d /= 2; c *= 0.5; } return c; }
static double kscale(int i) { double c = 1.0; for (int j = -2; j <= 3; ++j) if (j != i) c *= scl(j - i); return c; }
/* div_const for a positive odd part */
static double divc(double x, int a) {
  if (a == 1) return x * 1.0;
  double R = 1.0 / a, q0 = x * R, r = fma(-q0, (double)a, x);
  return fma(r, R, q0);
}
/* div_const_scaled: S * (x / a), S = 2^-e in the Markstein step's constants */
static double divc_s(double x, int a, double S) {
  double R = (1.0 / a) * S, A = (double)a / S;
  double q0 = x * R, r = fma(-q0, A, x);
  return fma(r, R, q0);
}
/* today's formulation: running product of the odd-part divisions, then * kScale */
static double w_cur(const double* t, int i) {
  double v = 1.0;
  for (int j = -2; j <= 3; ++j) if (j != i) v = divc(v * t[j + 2], oddp(j - i));
  double S = kscale(i);
  return S == 1.0 ? v : v * S;
}
/* the folded formulation (wstep): |kScale| in the first Markstein step, its
   sign on the last step's multiply; weight I = 1 keeps the trailing multiply */
static double w_new(const double* t, int i) {
  if (i == 1) return w_cur(t, i);
  const double S = kscale(i), M = fabs(S);
  int fold = 99, last = -9;
  for (int j = -2; j <= 3; ++j) if (j != i) { last = j; if (oddp(j - i) != 1 && fold == 99) fold = j; }
  double v = 1.0;
  for (int j = -2; j <= 3; ++j) {
    if (j == i) continue;
    double x = (j == last && S < 0) ? (-v) * t[j + 2] : v * t[j + 2];
    const int a = oddp(j - i);
    v = j == fold ? divc_s(x, a, M) : divc(x, a);
  }
  return v;
}
/* interpolate.m:37, IEEE divisions by j - i */
static double w_ref(const double* t, int i) {
  double w = 1.0;
  for (int j = -2; j <= 3; ++j) if (j != i) w = w * t[j + 2] / (double)(j - i);
  return w;
}
static long check(double a, double bump, int ref) {
  long bad = 0;
  double t[6];
  for (int j = -2; j <= 3; ++j) t[j + 2] = (a - (double)j) + bump;
  for (int i = -2; i <= 3; ++i) {
    double c = w_cur(t, i), n = w_new(t, i);
    if (memcmp(&c, &n, 8)) { ++bad; if (bad < 20) printf("a=%a bump=%a i=%d cur=%a new=%a\n", a, bump, i, c, n); }
    if (ref) { double r = w_ref(t, i); if (memcmp(&c, &r, 8)) { ++bad; if (bad < 20) printf("ref a=%a bump=%a i=%d cur=%a ref=%a\n", a, bump, i, c, r); } }
  }
  return bad;
}
int main(void) {
  long bad = 0;
  const double bumps[] = {0.0, 1e-10, -1e-10};
  /* random offsets: folded == current == reference order with true divisions */
  for (long n = 0; n < 10000002; ++n) {
    uint64_t m = nxt() >> 12; double a = (double)m / 4503599627370496.0;
    bad += check(a, bumps[n % 3], 1);
  }
  /* special offsets and exact-zero factors (a = j - bump), every bump: folded == current */
  const double sp[] = {0.0, 0x1p-52, 0x1p-1074, 0.5, 1 - 0x1p-53};
  for (int b = 0; b < 3; ++b) {
    for (int q = 0; q < 5; ++q) bad += check(sp[q], bumps[b], 0);
    for (int j = -2; j <= 3; ++j) {
      bad += check((double)j - bumps[b], bumps[b], 0);
      bad += check(-((double)j - bumps[b]), bumps[b], 0);  /* and the factor -0 where j = 0 */
    }
  }
  bad += check(-0.0, 0.0, 0);
  printf("%ld\n", bad);
  return bad != 0;
}
"""

CELL = r"""
#include <math.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t nxt(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static int cvt_sat(double v) {  /* v_cvt_i32_f64: NaN -> 0, saturating */
  if (isnan(v)) return 0;
  if (v >= 2147483647.0) return INT_MAX;
  if (v <= -2147483648.0) return INT_MIN;
  return (int)v;
}
static unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
static double div_rn(double a, double b, double rb) { double q0 = a * rb, r = fma(-q0, b, a); return fma(r, rb, q0); }
/* cell_frac: exact = the power-of-two short path, one = the single wrap */
static int cell_frac(double x, double dx, double inv_dx, double period, double inv_period, int iperiod, int nx,
                     double* a, int exact, int one) {
  const double q = div_rn(x, dx, inv_dx);
  double r = q * inv_period;
  if (!exact) r = fma(fma(-r, period, q), inv_period, r);
  const double xl = q - floor(r) * period;
  const double fl = floor(xl);
  *a = (1.0 + xl) - (1.0 + fl);
  int c = cvt_sat(fl);
  c = (unsigned)c > (unsigned)iperiod ? 0 : c;
  c = (int)umin((unsigned)c, (unsigned)(c - nx));
  if (one) return c;
  c = (int)umin((unsigned)c, (unsigned)(c - nx));
  if (iperiod >= 3 * nx) c %= nx;
  return c;
}
/* equal bits; two NaNs count as equal (their payloads are the host's, not the GPU's) */
static int same(double a, double b) { return (isnan(a) && isnan(b)) || memcmp(&a, &b, 8) == 0; }
static long one_x(double x, double dx, int nx, int ip) {
  const double p = (double)ip;
  double a0, a1;
  const int c0 = cell_frac(x, dx, 1.0 / dx, p, 1.0 / p, ip, nx, &a0, 0, 0);
  const int c1 = cell_frac(x, dx, 1.0 / dx, p, 1.0 / p, ip, nx, &a1, 1, ip == nx);
  if (c0 != c1 || !same(a0, a1)) { printf("x=%a nx=%d p=%d: %d %a vs %d %a\n", x, nx, ip, c0, a0, c1, a1); return 1; }
  return 0;
}
int main(void) {
  long bad = 0;
  const int cfg[4][2] = {{64, 64}, {128, 128}, {1024, 1024}, {512, 1024}};  /* nx, period */
  for (int g = 0; g < 4; ++g) {
    const int nx = cfg[g][0], ip = cfg[g][1];
    const double dx = 6.283185307179586 / nx;
    for (long i = 0; i < 10000000; ++i) {
      /* |x| <= 1e6*dx, half of them log-distributed down to 2^-60 of that */
      double u = ((double)(nxt() >> 11) / 9007199254740992.0 * 2.0 - 1.0) * 1e6 * dx;
      if (i & 1) u = ldexp(u, -(int)(nxt() % 61));
      bad += one_x(u, dx, nx, ip);
    }
    for (int k = -3 * ip - 2; k <= 3 * ip + 2; ++k) {  /* exact multiples of dx, next to them, and of the period */
      const double x = (double)k * dx;
      bad += one_x(x, dx, nx, ip);
      bad += one_x(nextafter(x, INFINITY), dx, nx, ip);
      bad += one_x(nextafter(x, -INFINITY), dx, nx, ip);
      bad += one_x((double)k * ((double)ip * dx), dx, nx, ip);
    }
    const double spec[] = {0.0, -0.0, NAN, INFINITY, -INFINITY, 0x1p-1074, -0x1p-1074, 1e300, -1e300};
    for (unsigned q = 0; q < sizeof spec / sizeof spec[0]; ++q) bad += one_x(spec[q], dx, nx, ip);
  }
  /* iperiod == nx: one unsigned-min wrap equals two for every c in [0, nx] */
  const int nxs[] = {8, 48, 64, 100, 512, 4096};
  for (unsigned a = 0; a < sizeof nxs / sizeof nxs[0]; ++a) {
    const int nx = nxs[a];
    for (int c = 0; c <= nx; ++c) {
      const int c1 = (int)umin((unsigned)c, (unsigned)(c - nx));
      const int c2 = (int)umin((unsigned)c1, (unsigned)(c1 - nx));
      if (c1 != c2 || c1 != c % nx) ++bad;
    }
  }
  printf("%ld\n", bad);
  return bad != 0;
}
"""


def _run(tmp_path, name, src):
    c = tmp_path / (name + ".c")
    c.write_text(src)
    exe = tmp_path / name
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(c), "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout[-2000:]


def test_weights_with_scale_folded_into_markstein_step_are_bit_exact(tmp_path):
    """For each I in -2..3 the folded weight equals the running product of
    odd-part divisions times kScale bit for bit (1e7 random a in [0, 1) over
    bumps 0 and +-1e-10, where that form is also pinned to interpolate.m's
    ((w*t)/d) with true divisions; a in {0, 2^-52, 2^-1074, 0.5, 1 - 2^-53}
    and the a = j - bump that zero a factor, every bump).  Weight I = 1
    keeps its trailing multiply: folded, it differs at a = 2^-1074, bump 0
    (-0 against -2^-1073, a subnormal product)."""
    _run(tmp_path, "wfold", WEIGHTS)


def test_cell_frac_short_paths_match_general_path(tmp_path):
    """Periods 64, 128, 1024 and 2*512: q*inv_period in place of div_rn gives
    the same cell and offset for 1e7 random x in +-1e6*dx each, multiples of
    dx and of the period and their neighbours, +-0, subnormals, NaN and Inf;
    with iperiod == nx one wrap equals two for every c in [0, nx]."""
    _run(tmp_path, "cellshort", CELL)
