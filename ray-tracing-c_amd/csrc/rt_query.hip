// rt_query.hip — the gfx950 ray-query kernels (rt_query.h) and their launches: the one-ray-per-thread
// kernel that rt_trace_rays_async launches, and in the diagnostic build (-DRT_DIAG, RT_QUERY_NAIVE=0) the
// persistent lane-refilling kernel it was measured against.  A translation unit of
// its own: the render kernels of rt_kernel.hip are tuned to the register (rt_book1.h, rt_general.h), and
// further kernels in their module move the compiler's decisions for some of them by a register or two;
// here they cannot.  rt_kernel.hip holds the C ABI above these launches (rt_trace_rays_async).
#include <hip/hip_runtime.h>

#include "rt_query.h"

using namespace rt;

// One ray per thread, ceil(n / 256) workgroups, the preorder read through the caches: the hardware's
// workgroup dispatcher is the refill.  30 (kFeatBook1) / 65 (kFeatAll) VGPRs, no LDS: 8 / 7 waves per SIMD.
template <int F>
__global__ __launch_bounds__(qry::kBlock) void rt_query_naive_kernel(qry::QueryView V) {
  const int64_t k = (int64_t)blockIdx.x * qry::kBlock + threadIdx.x;
  if (k < V.n) qry::trace_one<F>(V, k);
}

namespace rt {
namespace qry {
void launch_naive(bool fb, hipStream_t st, const QueryView &V) {
  const dim3 g((unsigned)((V.n + kBlock - 1) / kBlock)), b(kBlock);
  if (fb) hipLaunchKernelGGL(rt_query_naive_kernel<kFeatBook1>, g, b, 0, st, V);
  else hipLaunchKernelGGL(rt_query_naive_kernel<kFeatAll>, g, b, 0, st, V);
}
}  // namespace qry
}  // namespace rt

#ifdef RT_DIAG
// Persistent ray-query kernel (rt_query.h): grid = resident workgroups, lanes take ray indices.  Two
// shapes: 256 threads with up to 32 KiB of preorder in LDS (five workgroups per CU, 5 waves per SIMD), or
// one 1024-thread workgroup per CU (4 waves per SIMD) with up to the CU's whole LDS for a larger preorder.
template <int F, int kThreads>
__global__ __launch_bounds__(kThreads, qry::kWavesPerSimd<kThreads>) void rt_query_kernel(qry::QueryView V) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  qry::query_persistent<F>(V, (float4 *)lds);
}

namespace rt {
namespace qry {

const void *kernel_fn(bool fb, bool big) {
  return big ? (fb ? (const void *)rt_query_kernel<kFeatBook1, kBigBlock> : (const void *)rt_query_kernel<kFeatAll, kBigBlock>)
             : (fb ? (const void *)rt_query_kernel<kFeatBook1, kBlock> : (const void *)rt_query_kernel<kFeatAll, kBlock>);
}

void launch(bool fb, bool big, unsigned grid, size_t lds_bytes, hipStream_t st, const QueryView &V) {
  const dim3 g(grid), b((unsigned)(big ? kBigBlock : kBlock));
  if (big && fb) hipLaunchKernelGGL((rt_query_kernel<kFeatBook1, kBigBlock>), g, b, lds_bytes, st, V);
  else if (big) hipLaunchKernelGGL((rt_query_kernel<kFeatAll, kBigBlock>), g, b, lds_bytes, st, V);
  else if (fb) hipLaunchKernelGGL((rt_query_kernel<kFeatBook1, kBlock>), g, b, lds_bytes, st, V);
  else hipLaunchKernelGGL((rt_query_kernel<kFeatAll, kBlock>), g, b, lds_bytes, st, V);
}

}  // namespace qry
}  // namespace rt
#endif
