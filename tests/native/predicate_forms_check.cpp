// Check of the lane predicates of the render kernel's common light iteration
// (rt_device.h: renorm_t_ok, renorm_near_one, light_common -- the code the
// kernels run, here on the CPU, where frexp_exp is the C library's exponent)
// against a copy of the text each of them had.  Every new form is an equal
// form: it passes with 0 differences, and every class its edge generator aims
// at is counted so that none passes by absence.  The renderer-shaped
// directions are generated here -- unit vectors, unit vectors normalised again,
// reflections of one about another, unit vectors moved a few ulps, exact zero
// components -- the kinds num_check.cpp and exact_forms_check.cpp make for
// their shadow directions (unit(unit(..)), unit(ldir)), without the spheres
// around them, which these predicates do not read.  Prints one line per predicate,
//   <name> <inputs> diff <n> <class> <n> ...
//   hipcc -O2 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -I csrc predicate_forms_check.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

#include "rt_device.h"

using rtk::D3;
using rtk::SphGeo;

namespace {
const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kHuge = std::numeric_limits<double>::infinity();
double up(double x) { return std::nextafter(x, kHuge); }
double dn(double x) { return std::nextafter(x, -kHuge); }
bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// ---- the texts that were replaced ------------------------------------------
bool old_t_ok(double t) { return t >= -4.0 && t <= 6.0; }
bool old_near_one(D3 a, double &t) {
  const double s = (a.x * a.x + a.y * a.y) + a.z * a.z;
  t = (s - 1.0) * 0x1p53;
  auto usable = [](double x) { return __builtin_fabs(x) >= 0x1p-959 || x == 0.0; };
  return t >= -4.0 && t <= 6.0 && usable(a.x) && usable(a.y) && usable(a.z);
}
bool old_light_common(bool off_free, rtk::LgRange cell, double dist, D3 ldir, double &t) {
  return old_near_one(ldir, t) && off_free && cell.cb >= 0 && dist >= 0x1p-900;
}
struct V {
  double x, y, z;
};
V sub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V scl(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V unit(V a) {
  const double l = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
  return {a.x / l, a.y / l, a.z / l};
}
D3 d3(V v) { return D3{v.x, v.y, v.z}; }

struct Counts {
  // range compare on t
  long t_n = 0, t_diff = 0, t_in = 0, t_below = 0, t_above = 0, t_nan = 0, t_off = 0;
  // renorm_near_one / light_common
  long g_n = 0, g_diff = 0, g_common = 0, g_lost = 0, g_zero = 0, g_tiny = 0, g_edge_in = 0, g_edge_out = 0,
       g_nonfinite = 0, g_offfree0 = 0, g_nocell = 0, g_dist = 0, g_tclass[15] = {0};
};

void t_case(Counts &n, double t) {
  ++n.t_n;
  const bool o = old_t_ok(t), w = rtk::renorm_t_ok(t, 5.0);
  n.t_diff += o != w;
  n.t_in += o;
  n.t_below += t < -4.0;
  n.t_above += t > 6.0;
  n.t_nan += t != t;
  // the width of a scene whose lines the host has not bounded (off_free
  // false made the old guard false for every t): counted where the new form
  // refuses t as well, a difference where it does not
  if (rtk::renorm_t_ok(t, rtk::light_common_width(false))) ++n.t_diff;
  else ++n.t_off;
}

// One direction with every setting of the guard's other inputs; `shaped`: a
// renderer-shaped direction, where no lane may be lost.
void guard_case(Counts &n, V a, bool shaped) {
  double t0, t1;
  const bool o = old_near_one(d3(a), t0), w = rtk::renorm_near_one(d3(a), t1);
  ++n.g_n;
  if (o != w || !same_bits(t0, t1)) {
    if (++n.g_diff <= 5) std::printf("near_one differs: (%a %a %a) old %d new %d\n", a.x, a.y, a.z, o, w);
  }
  n.g_common += o;
  n.g_lost += shaped && o && !w;
  const double c[3] = {a.x, a.y, a.z};
  const bool range = old_t_ok(t0);
  for (double x : c) {
    const double m = std::fabs(x);
    if (range) {
      n.g_zero += x == 0.0;
      n.g_tiny += x != 0.0 && m < 0x1p-959;
      n.g_edge_in += m == 0x1p-959;
      n.g_edge_out += m == dn(0x1p-959);
    }
    n.g_nonfinite += !(m < kHuge);
  }
  if (t0 >= -6.0 && t0 <= 8.0 && t0 == std::floor(t0)) ++n.g_tclass[(int)t0 + 6];
  // light_common over off_free x binnable cell x distance
  const double dists[] = {1.0, 0x1p-900, dn(0x1p-900), 0.0, kNaN, kHuge};
  for (int off_free = 0; off_free < 2; ++off_free)
    for (int cb = -1; cb < 2; ++cb)
      for (double dist : dists) {
        const rtk::LgRange cell{cb, cb + 1};
        double u0, u1;
        const bool lo = old_light_common(off_free != 0, cell, dist, d3(a), u0);
        const bool lw = rtk::light_common(rtk::light_common_width(off_free != 0), cell, dist, d3(a), u1);
        ++n.g_n;
        if (lo != lw || !same_bits(u0, u1)) {
          if (++n.g_diff <= 5) std::printf("light_common differs: (%a %a %a) off_free %d cb %d dist %a\n", a.x, a.y, a.z, off_free, cb, dist);
        }
        n.g_offfree0 += o && !off_free;
        n.g_nocell += o && cb < 0;
        n.g_dist += o && !(dist >= 0x1p-900);
      }
}

}  // namespace

int main(int argc, char **argv) {
  const long N = argc > 1 ? std::atol(argv[1]) : 400000;
  std::mt19937_64 rng(24681357);
  std::uniform_real_distribution<double> U(-1.0, 1.0), U01(0.0, 1.0);
  auto rdir = [&] {
    V v;
    do v = {U(rng), U(rng), U(rng)};
    while (dot(v, v) > 1.0 || dot(v, v) < 1e-6);
    return unit(v);
  };
  auto rexp = [&](double lo, double hi) { return std::pow(2.0, lo + (hi - lo) * U01(rng)); };
  Counts n;

  // ---- t: the integers -6..8, their neighbours, the edges' neighbours, specials, random values
  for (int k = -6; k <= 8; ++k) {
    t_case(n, (double)k);
    t_case(n, up((double)k));
    t_case(n, dn((double)k));
  }
  const double tsp[] = {kNaN, kHuge, -kHuge, 0.0, -0.0, 1e300, -1e300, 0x1p-1074, -0x1p-1074, 0x1p53, -0x1p53};
  for (double t : tsp) t_case(n, t);
  for (long i = 0; i < N; ++i) {
    t_case(n, U(rng) * 12.0);
    t_case(n, (U01(rng) < 0.5 ? -1.0 : 1.0) * rexp(-1074.0, 1023.0));
    // the (s - 1) 2^53 of a sum of squares near 1
    const V v = rdir();
    t_case(n, (((v.x * v.x + v.y * v.y) + v.z * v.z) - 1.0) * 0x1p53);
  }

  // ---- the guard on renderer-shaped directions: normalised, normalised twice,
  // reflected about a unit normal, a few ulps off
  for (long i = 0; i < N; ++i) {
    const V a = rdir(), b = rdir();
    guard_case(n, a, true);
    guard_case(n, unit(a), true);
    const V l = scl(a, -1.0);
    guard_case(n, sub(l, scl(scl(b, 2.0), dot(l, b))), true);
    V p = a;
    for (int k = (int)(U01(rng) * 4.0); k > 0; --k) {
      double &c = (k & 1) ? p.x : (k & 2) ? p.y : p.z;
      c = U01(rng) < 0.5 ? up(c) : dn(c);
    }
    guard_case(n, p, false);
    // axis-aligned and in-plane directions: exact zeros
    if ((i & 7) == 0) {
      V z = a;
      ((i >> 3) % 3 == 0 ? z.x : (i >> 3) % 3 == 1 ? z.y : z.z) = (i & 8) ? 0.0 : -0.0;
      guard_case(n, unit(z), true);
      guard_case(n, V{0.0, (i & 16) ? 1.0 : -1.0, -0.0}, true);
    }
  }
  // ---- the guard's component edges: one component special, the others a
  // unit vector of the plane (the special one's square underflows: s = 1 or
  // within 6 u of it, the range holds and usable() decides)
  const double comps[] = {0.0, -0.0, 0x1p-1074, -0x1p-1074, 0x1p-1023, 0x1p-1022, 0x1p-1000, dn(0x1p-959), -dn(0x1p-959),
                          0x1p-959, -0x1p-959, up(0x1p-959), 0x1p-958, 0x1p-600, kNaN, kHuge, -kHuge, 1e200};
  for (long i = 0; i < N / 16 + 64; ++i) {
    V v = rdir();
    v.z = 0.0;
    v = unit(v);
    if (i & 1) v = V{(i & 2) ? 1.0 : -1.0, 0.0, 0.0};
    for (double c : comps)
      for (int pos = 0; pos < 3; ++pos) {
        const V a = pos == 0 ? V{c, v.x, v.y} : pos == 1 ? V{v.x, c, v.y} : V{v.x, v.y, c};
        guard_case(n, a, false);
        guard_case(n, V{c, c, pos == 0 ? 1.0 : c}, false);
      }
    guard_case(n, V{rexp(-1074.0, -900.0), rexp(-1074.0, -900.0), 1.0}, false);
  }

  std::printf("range %ld diff %ld in %ld below %ld above %ld nan %ld unbounded %ld\n", n.t_n, n.t_diff, n.t_in, n.t_below,
              n.t_above, n.t_nan, n.t_off);
  std::printf("guard %ld diff %ld common %ld lost %ld zero %ld tiny %ld edge_in %ld edge_out %ld nonfinite %ld "
              "unbounded %ld nocell %ld dist %ld",
              n.g_n, n.g_diff, n.g_common, n.g_lost, n.g_zero, n.g_tiny, n.g_edge_in, n.g_edge_out, n.g_nonfinite,
              n.g_offfree0, n.g_nocell, n.g_dist);
  for (int k = 0; k < 15; ++k) std::printf(" t%+d %ld", k - 6, n.g_tclass[k]);
  std::printf("\n");
  return (n.t_diff || n.g_diff || n.g_lost) ? 1 : 0;
}
