// Microbenchmark: issue rate per SIMD of v_fmac_f64_dpp with row_newbcast:N (the only
// DPP control FP64 ALU instructions take on gfx950: lane N of each 16-lane row is
// broadcast to that row) against the plain v_fma_f64 / v_fmac_f64, in the harness of
// fp64_issue.hip: 1 and 4 waves per SIMD, 8 independent chains.  The DPP chains use a
// different N each (and all 16 over two kernels), the table registers are written once
// before the loop.  The results are checked against the plain form's bit for bit.
// hipcc -O3 --offload-arch=gfx950 -o tools/micro/fmac_dpp_issue tools/micro/fmac_dpp_issue.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

enum Op { FMA64, FMAC64, FMAC64_DPP_LO, FMAC64_DPP_HI, FMAC64_DPP_MIX };

// x = fma(lane N of h's 16-lane row, s, x)
template <int N> __device__ __forceinline__ void fmac_bcast(double &x, double h, double s) {
  asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
      : "+v"(x)
      : "v"(h), "v"(s), "n"(N));
}

template <int OP, int K> __device__ __forceinline__ void step(double *acc, const double *h,
                                                             const double *hb, double s, double a,
                                                             double b) {
  if constexpr (OP == FMA64) acc[K] = fma(acc[K], a, b);
  if constexpr (OP == FMAC64) acc[K] = fma(hb[K], s, acc[K]);
  if constexpr (OP == FMAC64_DPP_LO) fmac_bcast<K>(acc[K], h[K & 3], s);
  if constexpr (OP == FMAC64_DPP_HI) fmac_bcast<K + 8>(acc[K], h[K & 3], s);
  if constexpr (OP == FMAC64_DPP_MIX) {       // every other op through DPP
    if constexpr (K % 2 == 0) fmac_bcast<(5 * K + 3) & 15>(acc[K], h[K & 3], s);
    else acc[K] = fma(hb[K], s, acc[K]);
  }
}

template <int OP> __host__ __device__ constexpr int bcast_lane(int k) {
  return OP == FMAC64_DPP_LO ? k : OP == FMAC64_DPP_HI ? k + 8 : ((5 * k + 3) & 15);
}

template <int OP>
__global__ void chain(double *out, unsigned long long *clk, int iters, double a, double b) {
  constexpr int ILP = 8;
  double acc[ILP], h[4], hb[ILP];
  unsigned long long t0 = 0, r0 = 0;
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    t0 = __builtin_amdgcn_s_memtime();
    r0 = __builtin_amdgcn_s_memrealtime();
  }
  const int lane = threadIdx.x & 63;
  // the table: register j holds T[16 j + (lane & 15)] in every lane
#pragma unroll
  for (int j = 0; j < 4; ++j) h[j] = 1e-3 * (1 + 16 * j + (lane & 15));
#pragma unroll
  for (int k = 0; k < ILP; ++k) {
    acc[k] = lane * 1e-3 + k;
    // the plain form's operand: what chain k's broadcast delivers
    const int nb = OP == FMAC64 ? bcast_lane<FMAC64_DPP_LO>(k) : bcast_lane<OP>(k);
    hb[k] = 1e-3 * (1 + 16 * (k & 3) + nb);
  }
  const double s = 1e-3 + lane * 1e-6;
  for (int i = 0; i < iters; ++i) {
    step<OP, 0>(acc, h, hb, s, a, b);
    step<OP, 1>(acc, h, hb, s, a, b);
    step<OP, 2>(acc, h, hb, s, a, b);
    step<OP, 3>(acc, h, hb, s, a, b);
    step<OP, 4>(acc, h, hb, s, a, b);
    step<OP, 5>(acc, h, hb, s, a, b);
    step<OP, 6>(acc, h, hb, s, a, b);
    step<OP, 7>(acc, h, hb, s, a, b);
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
#pragma unroll
    for (int k = 0; k < ILP; ++k) out[k * 64 + lane] = acc[k];
  }
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    clk[0] = __builtin_amdgcn_s_memtime() - t0;
    clk[1] = __builtin_amdgcn_s_memrealtime() - r0;
  }
}

// the same chains with every DPP op replaced by the plain fma on the broadcast value
template <int OP> __global__ void chain_ref(double *out, int iters) {
  const int lane = threadIdx.x & 63;
  const double s = 1e-3 + lane * 1e-6;
  for (int k = 0; k < 8; ++k) {
    double x = lane * 1e-3 + k;
    const double hv = 1e-3 * (1 + 16 * (k & 3) + bcast_lane<OP>(k));
    for (int i = 0; i < iters; ++i) x = fma(hv, s, x);
    out[k * 64 + lane] = x;
  }
}

template <int OP> void run(const char *name, int wps, int cus) {
  double *d, *dr;
  unsigned long long *clk, hc[2];
  (void)hipMalloc(&d, 8 * 64 * 8);
  (void)hipMalloc(&dr, 8 * 64 * 8);
  (void)hipMalloc(&clk, 16);
  const int iters = 20000;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  chain<OP><<<cus, 256 * wps>>>(d, clk, 100, 0.999, 1e-3);
  (void)hipEventRecord(e0);
  chain<OP><<<cus, 256 * wps>>>(d, clk, iters, 0.999, 1e-3);
  (void)hipEventRecord(e1);
  (void)hipEventSynchronize(e1);
  float ms;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipMemcpy(hc, clk, 16, hipMemcpyDeviceToHost);
  const double ghz = (double)hc[0] / (double)hc[1] * 0.1;
  const double per_simd = (double)wps * iters * 8;            // wave-ops per SIMD
  const char *bits = "";
  if (OP == FMAC64_DPP_LO || OP == FMAC64_DPP_HI) {
    static double a[512], r[512];
    chain_ref<OP><<<1, 64>>>(dr, iters);
    (void)hipMemcpy(a, d, sizeof a, hipMemcpyDeviceToHost);
    (void)hipMemcpy(r, dr, sizeof r, hipMemcpyDeviceToHost);
    bits = memcmp(a, r, sizeof a) == 0 ? ", bits equal the plain fma's" : ", BITS DIFFER";
  }
  printf("%-14s waves/SIMD %d ILP 8: %.3f ms, clock %.2f GHz, %.2f cycles per wave-op%s\n", name,
         wps, ms, ghz, (ms * 1e-3 * ghz * 1e9) / per_simd, bits);
  (void)hipFree(d);
  (void)hipFree(dr);
  (void)hipFree(clk);
}

int main() {
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  for (int rep = 0; rep < 2; ++rep) {
    for (int wps = 1; wps <= 4; wps += 3) {
      run<FMA64>("fma64", wps, cus);
      run<FMAC64>("fmac64", wps, cus);
      run<FMAC64_DPP_LO>("fmac64_dpp0-7", wps, cus);
      run<FMAC64_DPP_HI>("fmac64_dpp8-15", wps, cus);
      run<FMAC64_DPP_MIX>("fmac64_dpp/2", wps, cus);
    }
  }
  return 0;
}
