// olpe_reduce.h -- the fixed-order block reductions of the step-3 folds and of the moments
// summary, and the stage-2 kernel two of them share.  Device code only.
//
// The tree.  T is the block size, a power of two; `red` holds T elements of LDS.  Thread t
// stores its value in red[t]; the stride o halves from T / 2 to 1 and thread t < o combines
// red[t] with red[t + o].  Every thread of the block takes part (call it outside divergent
// code) and every thread receives the result; a trailing barrier lets `red` be reused
// straight away.  The order of a double sum depends on T and on nothing else, which is what
// "bit-identical however the rows were split" rests on.  The word reductions
// are integer sum / min / max: the same whatever the order.
#pragma once
#include <hip/hip_runtime.h>

namespace olpe {

using word = unsigned long long;

struct WordSum {
  __device__ static word of(word a, word b) { return a + b; }
};
struct WordMin {
  __device__ static word of(word a, word b) { return b < a ? b : a; }
};
struct WordMax {
  __device__ static word of(word a, word b) { return b > a ? b : a; }
};

struct DoubleSum {
  __device__ static double of(double a, double b) { return a + b; }
};

template <int T, class Op, class V> __device__ V block_tree(V v, V *red) {
  static_assert(T > 0 && (T & (T - 1)) == 0, "the block size is a power of two");
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = Op::of(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  const V r = red[0];
  __syncthreads();
  return r;
}

template <int T> __device__ double block_sum(double v, double *red) {
  return block_tree<T, DoubleSum>(v, red);
}

// Op: WordSum, WordMin or WordMax
template <int T, class Op>
__device__ unsigned long long block_word(unsigned long long v, unsigned long long *red) {
  return block_tree<T, Op>(v, red);
}

// Stage 2 of a two-stage sum: workgroup j (T threads) adds the nblk partials
// part[j][0 .. nblk) -- thread t those at t, t + T, ... in order, the threads by the tree --
// into out[j].
template <int T>
static __global__ __launch_bounds__(T) void reduce_stage2_kernel(const double *__restrict__ part,
                                                                 int nblk,
                                                                 double *__restrict__ out) {
  __shared__ double red[T];
  const double *p = part + (size_t)blockIdx.x * nblk;
  double a = 0.0;
  for (int b = threadIdx.x; b < nblk; b += T) a += p[b];
  a = block_sum<T>(a, red);
  if (threadIdx.x == 0) out[blockIdx.x] = a;
}

}  // namespace olpe
