// SFMA agent, streaming form — one workgroup of 4 or 16 wavefronts per instance, for worlds whose
// tables do not fit the LDS (1 275 ... 16 383 states; any size under COBEL_F_SFMA_STREAM).
//
// The kernel body is the general one of the LDS-resident form (cobel_sfma.h, sfma_body with BIG):
// same streams, same counters, same order of every floating-point operation.  What differs is
// where the tables lie.  Per state: the inhibition I always in LDS; the similarity rows D[cur],
// D[next] and the 2-byte successor table as far as the host-side plan (sfma.hip) finds room, else
// read from `metric` / the packed model records.  Per experience: the strengths C, the model
// records and the store stamps are read and written in the caller's arrays, Q rows likewise.  The
// priority vector of a reactivation has no home at all, so every pass rates its experiences again:
// one pass for the maximum rating, one that sums the softmax weights and takes their maximum, one
// that locates the draw — three reads of C and two exp per experience and reactivation.
//
// Thread t owns the experiences [t * chunk, (t + 1) * chunk), chunk a multiple of four: the
// cumulative sum behind the draw is an in-thread running sum, one wave scan and the totals of the
// waves before, in wave order.  A pass walks the chunk four experiences at a time (scan4): their
// strengths are two 16-byte loads, their stamps one, requested one group ahead; what else the four
// need (similarity, inhibition, successors) is requested for all four before the first is rated.
#include "cobel_sfma.h"

namespace cobel_sfma {
namespace {

__global__ __launch_bounds__(256) void k_sfma_big_4(const sfma_args A) {
  sfma_body<0, 4, false, true>(A);
}
__global__ __launch_bounds__(512) void k_sfma_big_8(const sfma_args A) {
  sfma_body<0, 8, false, true>(A);
}
__global__ __launch_bounds__(1024) void k_sfma_big_16(const sfma_args A) {
  sfma_body<0, 16, false, true>(A);
}

}  // namespace

int launch_sfma_big(const sfma_args& A, int threads, size_t lds, hipStream_t st) {
  const void* const fn = threads == 256   ? reinterpret_cast<const void*>(&k_sfma_big_4)
                         : threads == 512 ? reinterpret_cast<const void*>(&k_sfma_big_8)
                                          : reinterpret_cast<const void*>(&k_sfma_big_16);
  if (lds > 64 * 1024)
    COBEL_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (threads == 256) hipLaunchKernelGGL(k_sfma_big_4, dim3(A.r.n), dim3(256), lds, st, A);
  else if (threads == 512) hipLaunchKernelGGL(k_sfma_big_8, dim3(A.r.n), dim3(512), lds, st, A);
  else hipLaunchKernelGGL(k_sfma_big_16, dim3(A.r.n), dim3(1024), lds, st, A);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

}  // namespace cobel_sfma
