// Check of the predicated exact ray-sphere tests of the list loops
// (rt_device.h exact_num, shadow_exact, closest_test: the code the kernels
// run, here on the CPU, where any_lane(x) is x) against the chain of per-lane
// branches around intersect_num they replace:
//  * shadow queries: shadow_exact's decision equals shadow_chain's
//    (intersect_num with qocc = qlo, the qlo / qhi band, intersect() for the
//    cold class) and the reference's (sphere.h:26-59, scene.h:78-82) for
//    every pair;
//  * closest hits: closest_test folded over a ray's candidates leaves the same
//    (bt, bi) and the same bn as the chain form (closest_chain below, the
//    text closest_test had) after every candidate.
// The pairs are num_check.cpp's generators (copied: shaded points on a first
// sphere, lights far, near and on it, second spheres along the query's line,
// grazing and exactly tangent), plus a generator for the band class (a root
// within 2^-47 of the light's distance: on axis-aligned lines, two of the
// eight spheres centred at o + d (dist + |r|)(1 + k 2^-50), k in -8..8) and
// the lanes that are not `fast` (a NaN direction, a2 outside a2_ok, dist below
// 2^-900).  Prints
//   shadow <pairs> diff <n> wrong <n> tangent <n> early <n> sqfree <n> tiny <n> band <n> notfast <n>
//   closest <pairs> diff <n> hits <n> cold <n> notfast <n>
//   hipcc -O2 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -I csrc exact_forms_check.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "rt_device.h"

using rtk::D3;
using rtk::SphGeo;

namespace {
struct V {
  double x, y, z;
};
V add(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V sub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V scl(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V unit(V a) {
  const double l = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
  return {a.x / l, a.y / l, a.z / l};
}
// sphere.h:26-59
bool ref_hit(V c, double rr, V o, V d, double &t) {
  const V oc = sub(o, c);
  const double a = dot(d, d), b = 2.0 * dot(oc, d), cc = dot(oc, oc) - rr;
  const double disc = b * b - 4 * a * cc;
  if (disc < 0) return false;
  if (disc == 0) {
    t = -b / (2 * a);
    return true;
  }
  const double t1 = (-b - std::sqrt(disc)) / (2 * a), t2 = (-b + std::sqrt(disc)) / (2 * a);
  if ((t1 < t2 ? t2 : t1) < 0) return false;
  t = (t2 < t1) ? t2 : t1;
  if (t < 0) t = (t1 < t2) ? t2 : t1;
  return true;
}
D3 d3(V v) { return D3{v.x, v.y, v.z}; }

// The chain form of one closest-hit candidate: per-lane branches around
// intersect_num's class.
void closest_chain(const SphGeo &s, int i, D3 o, D3 d, double a4, double a2, bool fast, double &bt, double &bn,
                   int &bi) {
  double num;
  const int r = fast ? rtk::intersect_num(s, o, d, a4, num) : 2;
  if (r == 1) {
    if (num < bn || i < bi) {
      const double t = num / a2;
      if (t < bt || (t == bt && i < bi)) {
        bt = t;
        bn = num;
        bi = i;
      }
    }
  } else if (r == 2) {
    double t;
    if (rtk::intersect(s, o, d, a4, a2, t) && (t < bt || (t == bt && i < bi))) {
      bt = t;
      bn = __builtin_inf();
      bi = i;
    }
  }
}
bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Counts {
  long sh = 0, sh_diff = 0, sh_wrong = 0, tangent = 0, early = 0, sqfree = 0, tiny = 0, band = 0, notfast = 0;
  long cl = 0, cl_diff = 0, cl_hit = 0, cl_cold = 0, cl_notfast = 0;
};

// One shadow pair: the two forms and the reference; the class counts.
void shadow_pair(Counts &n, const SphGeo &s, V c, V o, V d, double dist) {
  const double a = (d.x * d.x + d.y * d.y) + d.z * d.z, a4 = 4.0 * a, a2 = 2.0 * a;
  const double T = dist < rtk::kInf ? dist : rtk::kInf;
  const bool fast = rtk::a2_ok(a2) && dist == dist && T >= 0x1p-900;
  const double q = a2 * T, qlo = q * (1.0 - 0x1p-48), qhi = q * (1.0 + 0x1p-48);
  double t;
  const bool want = ref_hit(c, s.rr, o, d, t) && t < rtk::kInf && t < dist;  // scene.h:78-82
  const bool chain = rtk::shadow_chain(s, d3(o), d3(d), a4, a2, fast, qlo, qhi, dist);
  const bool pred = rtk::shadow_exact(s, d3(o), d3(d), a4, a2, fast, qlo, qhi, dist);
  ++n.sh;
  if (!fast) {
    ++n.notfast;
  } else {
    double num = 0.0;
    const int res = rtk::intersect_num(s, d3(o), d3(d), a4, num, qlo);
    const V oc = sub(o, c);
    const double b = 2.0 * ((oc.x * d.x + oc.y * d.y) + oc.z * d.z);
    const double cc = ((oc.x * oc.x + oc.y * oc.y) + oc.z * oc.z) - s.rr;
    const double disc = b * b - a4 * cc;
    n.tangent += disc == 0.0;
    n.early += res == 3;
    n.sqfree += res == 3 || (res == 0 && disc > 0.0);
    n.tiny += res == 2;
    n.band += res == 1 && !(num < qlo) && !(num > qhi);
  }
  if (pred != chain && ++n.sh_diff <= 5)
    std::printf("shadow differs: c (%.17g %.17g %.17g) rr %.17g o (%.17g %.17g %.17g) d (%.17g %.17g %.17g) "
                "dist %.17g chain %d predicated %d\n",
                c.x, c.y, c.z, s.rr, o.x, o.y, o.z, d.x, d.y, d.z, dist, chain, pred);
  if (pred != want && ++n.sh_wrong <= 5)
    std::printf("shadow wrong: c (%.17g %.17g %.17g) rr %.17g o (%.17g %.17g %.17g) d (%.17g %.17g %.17g) "
                "dist %.17g want %d predicated %d\n",
                c.x, c.y, c.z, s.rr, o.x, o.y, o.z, d.x, d.y, d.z, dist, want, pred);
}

// One ray's closest hit over its candidates, in an index order that is not
// ascending (so the i < bi arm of the update is taken): both forms after
// every candidate.
void closest_fold(Counts &n, const SphGeo *s, int cnt, V o, V d) {
  const double a = (d.x * d.x + d.y * d.y) + d.z * d.z, a4 = 4.0 * a, a2 = 2.0 * a;
  const bool fast = rtk::a2_ok(a2);
  double bt0 = rtk::kInf, bn0 = __builtin_inf(), bt1 = bt0, bn1 = bn0;
  int bi0 = -1, bi1 = -1;
  for (int k = 0; k < cnt; ++k) {
    const int i = (k * 3 + 1) % cnt;  // cnt = 8: a permutation
    closest_chain(s[i], i, d3(o), d3(d), a4, a2, fast, bt0, bn0, bi0);
    rtk::closest_test(s[i], i, d3(o), d3(d), a4, a2, fast, bt1, bn1, bi1);
    ++n.cl;
    if (!fast) {
      ++n.cl_notfast;
    } else {
      double num;
      const int r = rtk::intersect_num(s[i], d3(o), d3(d), a4, num);
      n.cl_hit += r == 1;
      n.cl_cold += r == 2;
    }
    if ((!same_bits(bt0, bt1) || bi0 != bi1 || !same_bits(bn0, bn1)) && ++n.cl_diff <= 5)
      std::printf("closest differs at candidate %d: chain (%.17g, %d, %.17g) predicated (%.17g, %d, %.17g)\n", i, bt0,
                  bi0, bn0, bt1, bi1, bn1);
  }
}
}  // namespace

int main(int argc, char **argv) {
  const long N = argc > 1 ? std::atol(argv[1]) : 1000000;
  std::mt19937_64 rng(7654321);
  std::uniform_real_distribution<double> U(-1.0, 1.0), U01(0.0, 1.0);
  auto rdir = [&] {
    V v;
    do v = {U(rng), U(rng), U(rng)};
    while (dot(v, v) > 1.0 || dot(v, v) < 1e-6);
    return unit(v);
  };
  auto rrad = [&] { return std::pow(10.0, -4.0 + 9.0 * U01(rng)) * (U01(rng) < 0.05 ? -1.0 : 1.0); };
  Counts n;
  // N accepted iterations of 8 spheres each: 8 N shadow pairs and 16 N
  // closest pairs from the generators alone, the other lanes on top
  for (long it = 0; it < N;) {
    // the shaded point: a camera-like ray's hit on a first sphere
    const double r0 = rrad();
    const V c0 = scl({U(rng), U(rng), U(rng)}, std::pow(10.0, 3.0 * U01(rng)));
    const V n0 = rdir();
    const V o0 = add(c0, scl(n0, std::fabs(r0) * std::pow(10.0, 3.0 * U01(rng)) + 1.0));
    const V d0 = unit(unit(sub(add(c0, scl(rdir(), std::fabs(r0) * U01(rng))), o0)));
    double t0;
    if (!ref_hit(c0, r0 * r0, o0, d0, t0)) continue;
    const V hp = add(o0, scl(d0, t0));
    V L;
    const double mode = U01(rng);
    if (mode < 0.1) L = add(c0, scl(rdir(), std::fabs(r0) * (0.5 + U01(rng))));
    else if (mode < 0.3) L = add(hp, scl(rdir(), std::fabs(r0) * std::pow(10.0, -6.0 + 6.0 * U01(rng))));
    else L = add(hp, scl(rdir(), std::fabs(r0) * std::pow(10.0, 4.0 * U01(rng))));
    // axis-aligned shadow rays now and then: exact tangents below
    const bool axis = U01(rng) < 0.1;
    if (axis) {
      const int ax = (int)(U01(rng) * 3.0) % 3;
      const double len = std::pow(10.0, -2.0 + 5.0 * U01(rng)) * (U01(rng) < 0.5 ? -1.0 : 1.0);
      L = hp;
      (ax == 0 ? L.x : ax == 1 ? L.y : L.z) += len;
    }
    const V to_light = sub(L, hp);
    const double dist = std::sqrt(dot(to_light, to_light));
    const V ldir = unit(to_light);
    const V o = add(hp, scl(ldir, 0.001)), d = unit(ldir);
    // a perpendicular for offsets from the line
    V perp = cross(d, rdir());
    if (dot(perp, perp) < 1e-12) continue;
    perp = unit(perp);
    ++it;
    SphGeo sph[8];
    V ctr[8];
    for (int k = 0; k < 8; ++k) {
      const double r = rrad();
      const double rr = r * r;
      // the centre's position along the line: behind the origin, between, beyond the light
      const double u = U01(rng);
      const double tc = u < 0.3 ? -dist * std::pow(10.0, -3.0 + 4.0 * U01(rng)) - std::fabs(r) * U01(rng)
                        : u < 0.75 ? dist * U01(rng)
                                   : dist * (1.0 + std::pow(10.0, -3.0 + 4.0 * U01(rng)));
      const double hm = U01(rng);
      double h;
      if (hm < 0.3) h = std::fabs(r) * (1.0 + (U01(rng) < 0.5 ? -1.0 : 1.0) * std::pow(10.0, -15.0 * U01(rng)));
      else if (hm < 0.4) h = 0.0;
      else h = std::fabs(r) * 2.0 * U01(rng);
      V c = add(add(o, scl(d, tc)), scl(perp, h));
      if (axis && U01(rng) < 0.5) {  // exactly tangent to the axis-aligned line: offset along another axis
        const V pc = add(o, scl(d, tc));
        c = pc;
        if (std::fabs(d.x) < 0.5) c.x += std::fabs(r);
        else c.y += std::fabs(r);
      }
      if (axis && k < 2) {  // the band: the near root within a few 2^-50 of the light's distance
        const int kk = (int)(U01(rng) * 17.0) % 17 - 8;
        c = add(o, scl(d, (dist + std::fabs(r)) * (1.0 + kk * 0x1p-50)));
      }
      ctr[k] = c;
      sph[k] = SphGeo{c.x, c.y, c.z, rr};
      shadow_pair(n, sph[k], c, o, d, dist);
    }
    // closest hits of the shadow ray and of the camera-like ray over the eight
    closest_fold(n, sph, 8, o, d);
    closest_fold(n, sph, 8, o0, d0);
    // the lanes that are not `fast`, every 16th iteration: a NaN direction, a
    // direction of length 2^40 (a2 = 2^81), a distance below 2^-900
    if ((it & 15) == 0) {
      const V dn = {d.x, std::nan(""), d.z}, dl = scl(d, 0x1p40);
      for (int k = 0; k < 8; ++k) {
        shadow_pair(n, sph[k], ctr[k], o, dn, dist);
        shadow_pair(n, sph[k], ctr[k], o, dl, dist);
        shadow_pair(n, sph[k], ctr[k], o, d, 0x1p-950);
        shadow_pair(n, sph[k], ctr[k], o, d, std::nan(""));
      }
      closest_fold(n, sph, 8, o, dn);
      closest_fold(n, sph, 8, o, dl);
      closest_fold(n, sph, 8, o0, scl(d0, 0x1p-40));
    }
  }
  std::printf("shadow %ld diff %ld wrong %ld tangent %ld early %ld sqfree %ld tiny %ld band %ld notfast %ld\n", n.sh,
              n.sh_diff, n.sh_wrong, n.tangent, n.early, n.sqfree, n.tiny, n.band, n.notfast);
  std::printf("closest %ld diff %ld hits %ld cold %ld notfast %ld\n", n.cl, n.cl_diff, n.cl_hit, n.cl_cold,
              n.cl_notfast);
  return (n.sh_diff || n.sh_wrong || n.cl_diff) ? 1 : 0;
}
