// Error of the transcendentals the activation functions are built from (pytc_common.h gelu_erf / gelu_fast / gelu_grad, pw_common.h
// apply_act), each evaluated ALONE against fp64: v_exp_f32 (__builtin_amdgcn_exp2f), v_rcp_f32 (__builtin_amdgcn_rcpf), __expf, erff,
// tanhf.  The installed headers state no bound for them; tests/activation_domain_cases.py takes its budgets from this program's
// output (profiles/activation_domain_probe.txt), never from the kernels it tests.
//
// Argument sets: every finite bf16 value; the fp32 grid (each bf16 value's two fp32 neighbours and the midpoint to the next bf16
// value, 2^18 equally spaced points of [-10, 10]); and the ranges the models feed: exp2 on [-150, 128], rcp on [1, 2^128),
// __expf on -x^2/2 and -x, erff on x/sqrt(2).  The error is counted in units of the fp32 spacing at the correctly rounded reference,
// 2^-126 below the normal range (v_exp_f32 / v_rcp_f32 flush there).  budget = largest error, rounded up to a whole unit, plus one.
//
//   hipcc -O3 --offload-arch=gfx950 tools/probes/intrinsic_ulp_probe.hip -o intrinsic_ulp_probe && ./intrinsic_ulp_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

enum { EXP2 = 0, RCP, EXPF, ERFF, TANHF, NFN };
static const char* NAMES[NFN] = {"exp2", "rcp", "expf", "erff", "tanhf"};

__global__ void __launch_bounds__(256) eval_kernel(const float* __restrict__ x, float* __restrict__ y, long n, int fn) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  float r;
  switch (fn) {
    case EXP2: r = __builtin_amdgcn_exp2f(v); break;
    case RCP: r = __builtin_amdgcn_rcpf(v); break;
    case EXPF: r = __expf(v); break;
    case ERFF: r = erff(v); break;
    case TANHF: r = tanhf(v); break;
    default: r = __builtin_amdgcn_exp2f(v * 1.44269504088896340736f); break;      // what __expf is expected to compile to
  }
  y[i] = r;
}

static double ref64(int fn, double v) {
  switch (fn) {
    case EXP2: return std::exp2(v);
    case RCP: return 1.0 / v;
    case EXPF: return std::exp(v);
    case ERFF: return std::erf(v);
    case TANHF: return std::tanh(v);
    default: return std::exp(v);
  }
}

static double unit_at(double ref) {
  const float r = std::fabs((float)ref);
  if (!(r >= 0x1p-126f)) return 0x1p-126;
  if (std::isinf(r)) return 0x1p104;                        // spacing at FLT_MAX
  return (double)std::nextafterf(r, INFINITY) - (double)r;
}

static float bf16_value(unsigned b) {
  const uint32_t u = b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

static std::vector<float> set_bf16() {
  std::vector<float> v;
  for (unsigned b = 0; b < 65536; ++b)
    if (std::isfinite(bf16_value(b))) v.push_back(bf16_value(b));
  return v;
}

static std::vector<float> set_grid() {
  std::vector<float> v;
  for (float f : set_bf16()) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u |= 0x8000u;
    float mid;
    std::memcpy(&mid, &u, 4);
    for (float c : {std::nextafterf(f, INFINITY), std::nextafterf(f, -INFINITY), mid})
      if (std::isfinite(c)) v.push_back(c);
  }
  for (int i = 0; i < (1 << 18); ++i) v.push_back((float)(-10.0 + 20.0 * i / ((1 << 18) - 1)));
  for (float c : {3.75f, -3.75f, 8.0f, -8.0f}) v.push_back(c);
  return v;
}

static std::vector<float> set_range(double lo, double hi, int n) {
  std::vector<float> v;
  for (int i = 0; i < n; ++i) v.push_back((float)(lo + (hi - lo) * i / (n - 1)));
  return v;
}

static std::vector<float> set_rcp_range() {        // 4096 mantissas in every binade of [1, 2^128)
  std::vector<float> v;
  for (int e = 0; e < 128; ++e)
    for (int m = 0; m < 4096; ++m) v.push_back(std::ldexp(1.0f + (m * 2048 + (m * 37) % 2048) * 0x1p-23f, e));
  return v;
}

template <typename FN>
static std::vector<float> mapped(const std::vector<float>& src, FN f) {
  std::vector<float> v;
  for (float s : src) v.push_back(f(s));
  return v;
}

static double worst[NFN];

// __expf(v) against v_exp_f32(v * log2(e)) bit for bit: with no mismatch the models may restate __expf as that product and instruction
static void compare_expf(const char* set, const std::vector<float>& x, float* dx, float* dy) {
  const long n = (long)x.size();
  std::vector<float> a(n), c(n);
  if (hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) { printf("copy failed\n"); exit(1); }
  if (hipMemset(dy, 0xff, n * 4) != hipSuccess) { printf("memset failed\n"); exit(1); }      // a launch that did not run leaves NaNs, not stale results
  hipLaunchKernelGGL(eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dy, n, (int)EXPF);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(a.data(), dy, n * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); exit(1); }
  if (hipMemset(dy, 0xff, n * 4) != hipSuccess) { printf("memset failed\n"); exit(1); }
  hipLaunchKernelGGL(eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dy, n, (int)NFN);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(c.data(), dy, n * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); exit(1); }
  long unwritten = 0;
  for (long i = 0; i < n; ++i) unwritten += (std::isnan(a[i]) || std::isnan(c[i])) && !std::isnan(x[i]);
  if (unwritten) { printf("expf   %s: %ld results were never written\n", set, unwritten); exit(1); }
  long diff = 0, first = -1;
  for (long i = 0; i < n; ++i)
    if (std::memcmp(&a[i], &c[i], 4) != 0 && !(std::isnan(a[i]) && std::isnan(c[i]))) { if (first < 0) first = i; ++diff; }
  printf("expf   %-22s n=%7ld  __expf(v) != v_exp_f32(v * log2e) at %ld arguments", set, n, diff);
  if (first >= 0) printf(" (first: v = %.9g, %.9g vs %.9g)", x[first], a[first], c[first]);
  printf("\n");
}

// references that are fp32 numbers themselves: reciprocals of powers of two, 2^integer, f(0).  The models leave these un-nudged.
static void exact_cases(float* dx, float* dy) {
  struct { int fn; std::vector<float> x; } sets[] = {{RCP, {}}, {EXP2, {}}, {EXPF, {0.f, -0.f}}, {ERFF, {0.f, -0.f}}, {TANHF, {0.f, -0.f}}};
  for (int e = -126; e <= 126; ++e) sets[0].x.push_back(std::ldexp(1.0f, e));
  for (int e = -126; e <= 127; ++e) sets[1].x.push_back((float)e);
  for (auto& s : sets) {
    const long n = (long)s.x.size();
    std::vector<float> y(n);
    if (hipMemcpy(dx, s.x.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) { printf("copy failed\n"); exit(1); }
    hipLaunchKernelGGL(eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dy, n, s.fn);
    if (hipMemcpy(y.data(), dy, n * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); exit(1); }
    long bad = 0;
    for (long i = 0; i < n; ++i) bad += (double)y[i] != ref64(s.fn, (double)s.x[i]);
    printf("%-6s exact cases           n=%7ld  results that differ from the exactly representable reference: %ld\n", NAMES[s.fn], n, bad);
  }
}

static void run(int fn, const char* set, const std::vector<float>& x, float* dx, float* dy) {
  const long n = (long)x.size();
  std::vector<float> y(n);
  if (hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) { printf("copy failed\n"); exit(1); }
  hipLaunchKernelGGL(eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dy, n, fn);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(y.data(), dy, n * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); exit(1); }
  double m = 0.0;
  long at = 0, nans = 0;
  for (long i = 0; i < n; ++i) {
    const double r = ref64(fn, (double)x[i]);
    if (std::isnan(y[i])) { ++nans; continue; }
    const float rf = (float)r;
    double e;
    if (std::isinf(rf) || std::isinf(y[i])) e = (rf == y[i]) ? 0.0 : std::fabs((double)std::fmin(std::fabs(y[i]), 3.4028234663852886e38f) - std::fmin(std::fabs(r), 3.4028234663852886e38)) / unit_at(r) + 1.0;
    else e = std::fabs((double)y[i] - r) / unit_at(r);
    if (e > m) { m = e; at = i; }
  }
  printf("%-6s %-22s n=%7ld  max error %8.3f units at x = %.9g (got %.9g, fp64 %.17g)  NaN results %ld\n", NAMES[fn], set, n, m, x[at], y[at],
         ref64(fn, (double)x[at]), nans);
  if (m > worst[fn]) worst[fn] = m;
}

int main() {
  const std::vector<float> b = set_bf16(), g = set_grid();
  const size_t cap = 1 << 21;
  float *dx, *dy;
  if (hipMalloc(&dx, cap * 4) != hipSuccess || hipMalloc(&dy, cap * 4) != hipSuccess) { printf("no device memory\n"); return 1; }
  auto positive = [](const std::vector<float>& s) { std::vector<float> v; for (float f : s) if (f >= 1.0f) v.push_back(f); return v; };
  auto clip = [](const std::vector<float>& s, float lo, float hi) { std::vector<float> v; for (float f : s) if (f >= lo && f <= hi) v.push_back(f); return v; };
  // the two hardware instructions, on the sets and on the ranges the models feed them
  run(EXP2, "bf16 in [-150, 128]", clip(b, -150.f, 128.f), dx, dy);
  run(EXP2, "grid in [-150, 128]", clip(g, -150.f, 128.f), dx, dy);
  run(EXP2, "range [-150, 0]", set_range(-150.0, 0.0, 1 << 20), dx, dy);
  run(EXP2, "range [0, 128]", set_range(0.0, 128.0, 1 << 20), dx, dy);
  run(RCP, "bf16 >= 1", positive(b), dx, dy);
  run(RCP, "grid >= 1", positive(g), dx, dy);
  run(RCP, "range [1, 2^128)", set_rcp_range(), dx, dy);
  run(RCP, "range [1, 2]", set_range(1.0, 2.0, 1 << 20), dx, dy);
  // __expf as gelu_grad (-x^2/2) and the sigmoid (-x) call it; arguments below -104 underflow whatever the error
  auto half_sq = [](float x) { return -0.5f * x * x; };
  auto neg = [](float x) { return -x; };
  run(EXPF, "-x^2/2, x bf16", clip(mapped(b, half_sq), -104.f, 0.f), dx, dy);
  run(EXPF, "-x^2/2, x grid", clip(mapped(g, half_sq), -104.f, 0.f), dx, dy);
  run(EXPF, "-x, x bf16", clip(mapped(b, neg), -104.f, 89.f), dx, dy);
  run(EXPF, "-x, x grid", clip(mapped(g, neg), -104.f, 89.f), dx, dy);
  run(EXPF, "range [-104, 0]", set_range(-104.0, 0.0, 1 << 20), dx, dy);
  compare_expf("all bf16", b, dx, dy);
  compare_expf("grid", g, dx, dy);
  compare_expf("-x^2/2, x grid", mapped(g, half_sq), dx, dy);
  auto scaled = [](float x) { return x * 0.70710678118654752440f; };
  run(ERFF, "x/sqrt2, x bf16", mapped(b, scaled), dx, dy);
  run(ERFF, "x/sqrt2, x grid", mapped(g, scaled), dx, dy);
  run(TANHF, "bf16", b, dx, dy);
  run(TANHF, "grid", g, dx, dy);
  exact_cases(dx, dy);
  for (int fn = 0; fn < NFN; ++fn)
    printf("budget %-6s = %d   (largest error %.3f units, rounded up to a whole unit, plus one)\n", NAMES[fn], (int)std::ceil(worst[fn]) + 1, worst[fn]);
  hipFree(dx);
  hipFree(dy);
  return 0;
}
