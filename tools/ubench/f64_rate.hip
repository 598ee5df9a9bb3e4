// Microbenchmark: wave-instruction throughput of v_mul_f64 and v_add_f64 (gfx950), the two operations of
// k_multipath's inner loop.  Every CU runs 1, 2, 4 and 8 waves per SIMD of a loop of 16 independent chains x ITER of
// one instruction; the time of the launch gives cycles per wave instruction per SIMD at CLOCK.  One JSON line.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench/f64_rate.hip -o tools/ubench/f64_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#define ITER 2048
#define CLOCK 2.4e9
#define KERNEL(NAME, ASM)                                                                     \
  __global__ void __launch_bounds__(256) NAME(double *out, double b)                         \
  {                                                                                           \
    double r[16];                                                                             \
    for (int k = 0; k < 16; k++) r[k] = 1.0 + threadIdx.x * (k + 1) * 1e-9;                   \
    for (int i = 0; i < ITER; i++) {                                                          \
      _Pragma("unroll") for (int k = 0; k < 16; k++) asm volatile(ASM : "+v"(r[k]) : "v"(b)); \
    }                                                                                         \
    double s = 0;                                                                             \
    for (int k = 0; k < 16; k++) s += r[k];                                                   \
    if (s == 0.123456789) out[0] = s;                                                         \
  }
KERNEL(k_mul, "v_mul_f64 %0, %0, %1")
KERNEL(k_add, "v_add_f64 %0, %0, %1")
KERNEL(k_fma, "v_fma_f64 %0, %0, %1, %0")

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                  \
      return 1;                                                                \
    }                                                                          \
  } while (0)

int main()
{
  hipDeviceProp_t p;
  CK(hipGetDeviceProperties(&p, 0));
  const int cus = p.multiProcessorCount;
  double *out;
  CK(hipMalloc(&out, 8));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  struct { const char *name; void (*fn)(double *, double); } ks[] = {{"v_mul_f64", k_mul}, {"v_add_f64", k_add}, {"v_fma_f64", k_fma}};
  printf("{\"cus\": %d, \"clock\": %.1e", cus, CLOCK);
  for (auto &k : ks) {
    printf(", \"%s\": {", k.name);
    for (int w = 1; w <= 8; w *= 2) {
      // w waves per SIMD: w workgroups of 4 waves per CU
      const dim3 grid(cus * w);
      float best = 1e30f;
      for (int rep = 0; rep < 6; rep++) {
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(k.fn, grid, dim3(256), 0, 0, out, 1.0000001);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep > 0 && ms < best) best = ms;
      }
      const double cycles = best * 1e-3 * CLOCK / ((double)w * ITER * 16);
      printf("%s\"%d\": %.3f", w == 1 ? "" : ", ", w, cycles);
    }
    printf("}");
  }
  printf("}\n");
  CK(hipFree(out));
  return 0;
}
