// Ceiling probe for v_mfma_f64_16x16x4_f64 (the loops of csrc/nearest_stretch.hip
// and csrc/van_rossum.hip): operands in registers, no loads, ACC independent
// accumulators per wave, `waves` waves per SIMD on every CU.  Prints the
// float64 matrix rate each combination sustains.
//   hipcc --offload-arch=gfx950 -O3 -o mfma_f64_probe mfma_f64_probe.hip && ./mfma_f64_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef __attribute__((ext_vector_type(4))) double f64x4;

template <int ACC>
__global__ __launch_bounds__(512) void probe(double* out, int iters) {
  const int lane = threadIdx.x & 63;
  double a = 1.0 + lane * 1e-3, b = 1.0 - lane * 1e-3;
  f64x4 acc[ACC];
#pragma unroll
  for (int i = 0; i < ACC; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < ACC; ++i)
      acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < ACC; ++i) s += acc[i][0] + acc[i][3];
  if (s == 12345.0) out[0] = s;  // (keeps the loop; never true)
}

template <int ACC>
static void run(double* out, int cus, int waves_per_simd, int iters) {
  const int threads = 64 * 4 * waves_per_simd;  // one workgroup per CU
  hipEvent_t t0, t1;
  (void)hipEventCreate(&t0);
  (void)hipEventCreate(&t1);
  float best = 1e30f;
  for (int rep = 0; rep < 5; ++rep) {
    (void)hipEventRecord(t0);
    hipLaunchKernelGGL(probe<ACC>, dim3(cus), dim3(threads), 0, 0, out, iters);
    (void)hipEventRecord(t1);
    (void)hipEventSynchronize(t1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, t0, t1);
    if (rep > 0 && ms < best) best = ms;  // (the first call loads the code)
  }
  const double flop = 2.0 * 16 * 16 * 4 * (double)ACC * iters * (threads / 64) * cus;
  printf("acc %2d  waves/SIMD %d  %8.3f ms  %7.2f TFLOP/s\n", ACC, waves_per_simd,
         best, flop / (best * 1e-3) * 1e-12);
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
  const int cus = prop.multiProcessorCount;
  double* out = nullptr;
  if (hipMalloc(&out, sizeof(double)) != hipSuccess) return 1;
  printf("%s, %d CUs, %d MFMAs per accumulator (clocks not pinned; best of 4 calls)\n",
         prop.name, cus, iters);
  for (int w = 1; w <= 2; ++w) {
    run<1>(out, cus, w, iters);
    run<2>(out, cus, w, iters);
    run<4>(out, cus, w, iters);
    run<8>(out, cus, w, iters);
  }
  (void)hipFree(out);
  return 0;
}
