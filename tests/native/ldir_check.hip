// ldir_check.hip -- GPU check of the two halves of rtk::div3 as the light loop
// uses them (rt_device.h light_common, rt_kernel.hip shade_hit): wherever
// div3_ok(a, b) holds, div3_shared(a, b) -- formed with no guard around it --
// has the bits of the three IEEE divisions a.x / b, a.y / b, a.z / b as the
// compiler lowers them.  div_check.hip's four operand kinds.  A stand-alone
// program, compiled by tests/test_gpu_ldir.py at test time:
//   ldir_check SEED N   prints, per kind, "kind K tested T ok O bad B" and the
//   last mismatching operands; exit status 0 unless a HIP call failed.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../cs420-ray-tracer_amd/csrc/rt_device.h"

namespace {

__device__ uint64_t mix(uint64_t z) {  // splitmix64 finaliser
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__device__ double unit(uint64_t z) { return (double)(z >> 11) * 0x1p-53; }

// One operand triple per (thread, kind): kind 0 = a random scene vector over
// its own length (the light direction's case), 1 = a near-unit vector over its
// length, 2 = random signs / exponents over the whole double range (b
// positive), 3 = edge values (zeros, subnormals, infinities, NaN, the guard's
// boundaries from both sides).
__device__ void operands(uint64_t seed, uint64_t i, int kind, rtk::D3 &a, double &b) {
  const uint64_t z0 = mix(seed ^ (i * 4 + kind)), z1 = mix(z0), z2 = mix(z1), z3 = mix(z2);
  if (kind == 0 || kind == 1) {
    const double s = kind == 0 ? __builtin_ldexp(1.0, (int)(z3 % 64) - 32) : 1.0;
    a = rtk::mk((unit(z0) - 0.5) * s, (unit(z1) - 0.5) * s, (unit(z2) - 0.5) * s);
    if (kind == 1) a = rtk::normalized(a);
    if ((z3 >> 20) % 16 == 0) a.y = 0.0;
    if ((z3 >> 24) % 32 == 0) a.x = -0.0;
    b = rtk::length(a);
    return;
  }
  if (kind == 2) {
    auto rnd = [](uint64_t z) {
      const int e = (int)(z % 2100) - 1075;
      return __builtin_copysign(__builtin_ldexp(1.0 + unit(mix(z)), e), (z >> 63) ? -1.0 : 1.0);
    };
    a = rtk::mk(rnd(z0), rnd(z1), rnd(z2));
    b = __builtin_fabs(rnd(z3));
    return;
  }
  const double edge[] = {0.0, -0.0, 0x1p-1074, -0x1p-1070, 0x1p-1022, 0x1p-601, 0x1p-600, -0x1p-600, 0x1p-599,
                         0x1p-301, 0x1p-300, 0x1p-299, 0x1p299, 0x1p300, 0x1p301, 0x1p399, 0x1p400, -0x1p400, 0x1p401,
                         1.0, -1.0, 1.0 + 0x1p-52, 1.0 - 0x1p-53, __builtin_inf(), -__builtin_inf(),
                         __builtin_nan(""), 3.0, 0.1, 1e300, 1e-300, 2.5e-200};
  const int ne = sizeof(edge) / sizeof(edge[0]);
  a = rtk::mk(edge[z0 % ne], edge[z1 % ne], edge[z2 % ne]);
  b = __builtin_fabs(edge[z3 % ne]) * ((z3 >> 40) % 3 == 0 ? (1.0 + unit(z2)) : 1.0);
}

__device__ bool same(double x, double y) {
  return __double_as_longlong(x) == __double_as_longlong(y) || (x != x && y != y);
}

// out[kind * 3 + {0, 1, 2}] = tested, div3_ok, mismatches under div3_ok; out[12..15] = a mismatch's a.x, a.y, a.z, b
__global__ void check(uint64_t seed, uint64_t n, unsigned long long *out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int kind = 0; kind < 4; ++kind) {
    rtk::D3 a;
    double b;
    operands(seed, i, kind, a, b);
    const rtk::D3 f = rtk::div3_shared(a, b);  // every lane, as the light loop forms it
    const bool ok = rtk::div3_ok(a, b);
    volatile double vb = b;  // keep the reference divisions independent of div3_shared's code
    const double bb = vb;
    const rtk::D3 r = rtk::mk(a.x / bb, a.y / bb, a.z / bb);
    atomicAdd(&out[kind * 3 + 0], 1ull);
    if (ok) {
      atomicAdd(&out[kind * 3 + 1], 1ull);
      if (!(same(f.x, r.x) && same(f.y, r.y) && same(f.z, r.z))) {
        atomicAdd(&out[kind * 3 + 2], 1ull);
        out[12] = __double_as_longlong(a.x);
        out[13] = __double_as_longlong(a.y);
        out[14] = __double_as_longlong(a.z);
        out[15] = __double_as_longlong(b);
      }
    }
  }
}

}  // namespace

#define HIP_OK(call)                                                            \
  do {                                                                          \
    const hipError_t e_ = (call);                                               \
    if (e_ != hipSuccess) {                                                     \
      std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));           \
      return 2;                                                                 \
    }                                                                           \
  } while (0)

int main(int argc, char **argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: ldir_check SEED N\n");
    return 2;
  }
  const unsigned long long seed = std::strtoull(argv[1], nullptr, 10), n = std::strtoull(argv[2], nullptr, 10);
  unsigned long long *d = nullptr, h[16];
  HIP_OK(hipMalloc(&d, sizeof(h)));
  HIP_OK(hipMemset(d, 0, sizeof(h)));
  hipLaunchKernelGGL(check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (uint64_t)seed, (uint64_t)n, d);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d));
  for (int k = 0; k < 4; ++k) std::printf("kind %d tested %llu ok %llu bad %llu\n", k, h[3 * k], h[3 * k + 1], h[3 * k + 2]);
  std::printf("last %#llx %#llx %#llx %#llx\n", h[12], h[13], h[14], h[15]);
  return 0;
}
