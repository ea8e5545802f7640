// The ray table's launch policy (rt_sched.h ray_table_policy, RayKey) on the
// CPU: every combination of mode, frame count, uniform / mixed keys, kept and
// previous key against the rule written out here, the key's byte-wise
// equality field by field, and a sequence of launches as a context runs them
// (rt_kernel.hip ray_table_prepare keeps `kept` and `prev` the same way).
// Prints "checked N ok"; exits 1 at the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_sched.h"

using namespace rtk;

static long long checked = 0;
static void expect(bool ok, const char *what, int a = 0, int b = 0, int c = 0) {
  ++checked;
  if (!ok) {
    std::printf("FAILED %s (%d %d %d)\n", what, a, b, c);
    std::exit(1);
  }
}

static RayKey key_of(int orient, int W, int H, int first) {
  RayKey k{};
  for (int i = 0; i < 10; i++) k.orient[i] = 0.1 * (i + 1) + orient;
  k.W = W, k.H = H;
  k.band = 8, k.first = first, k.stride = 3, k.count = 16;
  return k;
}

// a context's table state across launches
struct Ctx {
  RayKey kept{}, prev{};
  bool has_kept = false, has_prev = false;
  int builds = 0;
  RayUse launch(int mode, bool uniform, int nframes, const RayKey &key) {
    const RayUse u = ray_table_policy(mode, uniform, nframes, key, has_kept ? &kept : nullptr, has_prev ? &prev : nullptr);
    prev = key, has_prev = uniform;
    if (u == kRayBuild) kept = key, has_kept = true, ++builds;
    return u;
  }
};

int main() {
  // the key: equal to a copy, different in every single field, and compared by bytes (-0.0 is not 0.0)
  const RayKey a = key_of(0, 64, 48, 1);
  RayKey b = a;
  expect(ray_key_equal(a, b), "copy equal");
  for (int i = 0; i < 10; i++) {
    b = a;
    b.orient[i] += 1e-9;
    expect(!ray_key_equal(a, b), "orient differs", i);
  }
  int RayKey::*const ints[] = {&RayKey::W, &RayKey::H, &RayKey::band, &RayKey::first, &RayKey::stride, &RayKey::count};
  for (size_t i = 0; i < sizeof(ints) / sizeof(ints[0]); i++) {
    b = a;
    b.*ints[i] += 1;
    expect(!ray_key_equal(a, b), "int field differs", (int)i);
  }
  b = a;
  b.orient[3] = 0.0;
  RayKey c = b;
  c.orient[3] = -0.0;
  expect(!ray_key_equal(b, c), "signed zero");

  // the truth table
  const RayKey other = key_of(1, 64, 48, 1);
  for (int mode = -1; mode <= 3; mode++)
    for (int uniform = 0; uniform <= 1; uniform++)
      for (int nf = 0; nf <= 33; nf++)
        for (int kept = 0; kept <= 2; kept++)      // none, this key, another
          for (int prev = 0; prev <= 2; prev++) {  // none, this key, another
            const RayKey *kp = kept == 0 ? nullptr : kept == 1 ? &a : &other;
            const RayKey *pp = prev == 0 ? nullptr : prev == 1 ? &a : &other;
            RayUse want;
            if (mode <= 0 || !uniform || nf < 1) want = kRayInline;
            else if (kept == 1) want = kRayReuse;
            else if (mode >= 2 || nf >= 2 || prev == 1) want = kRayBuild;
            else want = kRayInline;
            expect(ray_table_policy(mode, uniform != 0, nf, a, kp, pp) == want, "truth table", mode, nf, kept * 3 + prev);
          }

  // a context's launches, default mode
  {
    Ctx x;
    expect(x.launch(1, true, 8, a) == kRayBuild, "8 frames build");
    expect(x.launch(1, true, 8, a) == kRayReuse, "again: reuse");
    expect(x.launch(1, true, 1, a) == kRayReuse, "one frame of the kept key: reuse");
    expect(x.launch(1, false, 8, a) == kRayInline, "mixed orientations: inline");
    expect(x.launch(1, true, 8, a) == kRayReuse, "the kept table survives a mixed launch");
    expect(x.launch(1, true, 8, other) == kRayBuild, "another orientation: rebuilt");
    expect(x.launch(1, true, 8, a) == kRayBuild, "and back: rebuilt");
    expect(x.launch(1, true, 8, key_of(0, 61, 45, 1)) == kRayBuild, "another size");
    expect(x.launch(1, true, 8, key_of(0, 61, 45, 2)) == kRayBuild, "another shard");
    expect(x.builds == 5, "five builds", x.builds);
  }
  {
    Ctx x;
    const RayKey k1 = key_of(2, 8, 8, 0), k2 = key_of(3, 8, 8, 0);
    expect(x.launch(1, true, 1, k1) == kRayInline, "first sighting inline");
    expect(x.launch(1, true, 1, k1) == kRayBuild, "second sighting builds");
    expect(x.launch(1, true, 1, k1) == kRayReuse, "third reuses");
    expect(x.launch(1, true, 1, k2) == kRayInline, "a new key: inline");
    expect(x.launch(1, true, 1, k1) == kRayReuse, "the kept key is still there");
    expect(x.launch(1, true, 1, k2) == kRayInline, "k2 after k1: not a second sighting in a row");
    expect(x.launch(1, false, 2, k2) == kRayInline, "mixed");
    expect(x.launch(1, true, 1, k2) == kRayInline, "a mixed launch leaves no previous key");
    expect(x.builds == 1, "one build", x.builds);
  }
  {
    Ctx x;  // mode 2: a first one-frame launch builds; mode 0: never
    const RayKey k1 = key_of(2, 8, 8, 0);
    expect(x.launch(2, true, 1, k1) == kRayBuild, "mode 2 first sighting builds");
    expect(x.launch(2, true, 1, k1) == kRayReuse, "mode 2 reuse");
    expect(x.launch(2, false, 4, k1) == kRayInline, "mode 2 mixed: inline");
    Ctx y;
    for (int i = 0; i < 4; i++) expect(y.launch(0, true, 8, k1) == kRayInline, "mode 0");
    expect(y.builds == 0, "mode 0 builds nothing");
  }
  std::printf("checked %lld ok\n", checked);
  return 0;
}
