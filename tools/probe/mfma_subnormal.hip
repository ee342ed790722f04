// What one v_mfma_f32_16x16x32_f16 does with fp16 SUBNORMAL operands: a single
// instruction per wave, no kernel code around it.  Every lane of a wave holds the
// same a[8g .. 8g+7] / b[8g .. 8g+7] of its k-group g, so every element of D is
// sum_k a[k] b[k] whatever the row / column layout.  Four products are non-zero:
// a normal with a full 11-bit significand and an exponent in [-6, 1], b = q 2^-24
// (subnormal, q in [1, 127]) in run 1 and the same b times 2^10 (normal) in run 2.
// All products and their sum are exact in double; cases whose sum is not an f32
// are skipped.  Printed per run: how many sums come back inexact, the largest
// error over gamma(K) sum |a b| (K = 32, u = 2^-23), over the same with b counted at
// no less than 2^-14, and in units of 2^(E - 24), E the largest sum of the
// operands' exponent FIELDS (a subnormal's field is -14).
//   hipcc --offload-arch=gfx950 -O2 -o mfma_subnormal mfma_subnormal.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__global__ __launch_bounds__(64) void one_mfma(const _Float16* a, const _Float16* b,
                                               float* out, int n) {
  const int w = blockIdx.x;
  if (w >= n) return;
  const int g = threadIdx.x >> 4;
  f16x8 va, vb;
  for (int i = 0; i < 8; ++i) {
    va[i] = a[w * 32 + g * 8 + i];
    vb[i] = b[w * 32 + g * 8 + i];
  }
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, vb, c, 0, 0, 0);
  if (threadIdx.x == 0) out[w] = c[0];
}

static int field(double v) {  // exponent field of an fp16 value (subnormal: -14)
  int e;
  frexp(fabs(v), &e);
  return e - 1 < -14 ? -14 : e - 1;
}

int main() {
  const int n = 4096, K = 32;
  std::vector<_Float16> a(n * K), b(n * K), b2(n * K);
  std::vector<double> want(n);
  srand(7);
  for (int w = 0; w < n; ++w) {
    want[w] = 0;
    for (int k = 0; k < K; ++k) a[w * K + k] = b[w * K + k] = b2[w * K + k] = (_Float16)0.f;
    for (int t = 0; t < 4; ++t) {
      const int k = (rand() % 8) * 4 + t;  // the four products in different k-groups or not
      const double av = ldexp(1024 + rand() % 1024, -10 + (rand() % 8) - 6) *
                        (rand() & 1 ? 1 : -1);
      const double bv = ldexp(1 + rand() % 127, -24) * (rand() & 1 ? 1 : -1);
      a[w * K + k] = (_Float16)av;
      b[w * K + k] = (_Float16)bv;
      b2[w * K + k] = (_Float16)(bv * 1024.0);
      want[w] += av * bv;
    }
  }
  _Float16 *da, *db;
  float* dout;
  hipMalloc(&da, n * K * 2);
  hipMalloc(&db, n * K * 2);
  hipMalloc(&dout, n * 4);
  hipMemcpy(da, a.data(), n * K * 2, hipMemcpyHostToDevice);
  std::vector<float> got(n);
  for (int run = 0; run < 2; ++run) {
    const std::vector<_Float16>& bb = run ? b2 : b;
    const double s = run ? 1024.0 : 1.0;
    hipMemcpy(db, bb.data(), n * K * 2, hipMemcpyHostToDevice);
    one_mfma<<<n, 64>>>(da, db, dout, n);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
    hipMemcpy(got.data(), dout, n * 4, hipMemcpyDeviceToHost);
    int used = 0, inexact = 0;
    double r_plain = 0, r_nom = 0, r_field = 0;
    const double gam = K * ldexp(1.0, -23) / (1 - K * ldexp(1.0, -23));
    for (int w = 0; w < n; ++w) {
      const double wv = want[w] * s;
      if ((double)(float)wv != wv) continue;
      ++used;
      double mag = 0, nom = 0;
      int E = -100;
      for (int k = 0; k < K; ++k) {
        const double av = (double)a[w * K + k], bv = (double)bb[w * K + k];
        if (av == 0 || bv == 0) continue;
        mag += fabs(av * bv);
        nom += fabs(av) * fmax(fabs(bv), ldexp(1.0, -14));
        const int e = field(av) + field(bv);
        if (e > E) E = e;
      }
      const double err = fabs((double)got[w] - wv);
      if (err > 0) ++inexact;
      r_plain = fmax(r_plain, err / (gam * mag));
      r_nom = fmax(r_nom, err / (gam * nom));
      r_field = fmax(r_field, err / ldexp(1.0, E - 24));
    }
    printf("%s b: %d sums representable in f32, %d inexact; worst error / (gamma sum|ab|) "
           "%.3g, / (gamma sum|a|max(|b|,2^-14)) %.3g, / 2^(E-24) %.3g\n",
           run ? "normal   " : "subnormal", used, inexact, r_plain, r_nom, r_field);
  }
  return 0;
}
