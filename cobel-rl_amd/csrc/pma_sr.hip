// PMAMemory.update_sr beyond the LDS: SR = inv(I - gamma T) in place in the instance's SR block in
// global memory, by the same in-place Gauss-Jordan without pivoting as k_pma_update_sr (pma.hip),
// blocked over panels of kB pivots (cobel_gj.h: the panel, line and tile functions, shared with the
// SFMA metrics of metric.hip).  Every element goes through the operations of that kernel in the
// same order, so the result equals the LDS kernel's bit for bit wherever both run.
// Three launches per panel, ordered by the stream (nothing waits inside a kernel): k_pma_sr_tiles,
// k_pma_sr_lines, k_pma_sr_diag — the instance is the grid's z axis.
#include "cobel_gj.h"
#include "cobel_pma.h"

namespace {

using namespace cobel_gj;

struct sr_args {
  double* M;          // [N][S][S] the SR blocks
  const double* T;    // [N][S][S]
  double gamma;
  int32_t S, k0, kb, nbr;
  uint32_t inst0;
  // per-instance parameter sets (cobel_pma_mem_x): with an index, gamma is the instance's
  const cobel_pma_param_set_t* sets;
  const uint16_t* index;
  int32_t n_sets;
};

// SETS: gamma of the instance's parameter set (the scalar launch keeps the form it had)
template <bool SETS>
__global__ __launch_bounds__(kThreads) void k_pma_sr_init(const sr_args P) {
  const int S = P.S;
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= (size_t)S * S) return;
  const uint32_t inst = P.inst0 + blockIdx.z;
  const size_t off = (size_t)inst * S * S;
  double gamma = P.gamma;
  if constexpr (SETS) {
    const int k = (int)((pma_index_ptr)P.index)[inst];
    gamma = ((pma_set_ptr)(P.sets + (k < P.n_sets ? k : P.n_sets - 1)))->gamma;
  }
  const int r = (int)(e / (size_t)S), c = (int)(e - (size_t)r * S);
  P.M[off + e] = (r == c ? 1.0 : 0.0) - gamma * P.T[off + e];
}

__global__ __launch_bounds__(kThreads) void k_pma_sr_tiles(const sr_args P) {
  extern __shared__ __attribute__((aligned(16))) double sr_lds[];
  gj_tiles(P.M + (size_t)(P.inst0 + blockIdx.z) * P.S * P.S, P.S, P.k0, P.kb, sr_lds);
}

__global__ __launch_bounds__(kThreads) void k_pma_sr_lines(const sr_args P) {
  extern __shared__ __attribute__((aligned(16))) double sr_lds[];
  gj_lines(P.M + (size_t)(P.inst0 + blockIdx.z) * P.S * P.S, P.S, P.k0, P.kb, P.nbr, sr_lds);
}

__global__ __launch_bounds__(kThreads) void k_pma_sr_diag(const sr_args P) {
  extern __shared__ __attribute__((aligned(16))) double sr_lds[];
  gj_diag(P.M + (size_t)(P.inst0 + blockIdx.z) * P.S * P.S, P.S, P.k0, P.kb, sr_lds);
}

}  // namespace

size_t cobel_pma_sr_blocked_lds() {
  return 8 * (kTileDoubles > kLineDoubles ? kTileDoubles : kLineDoubles);
}

int cobel_pma_sr_blocked(const cobel_pma_mem_x& m, hipStream_t st) {
  const int S = m.n_states;
  const unsigned nt = (unsigned)((S + kTile - 1) / kTile);
  const int nbr = (S + kThreads - 1) / kThreads;
  const unsigned init_blocks = (unsigned)(((size_t)S * S + kThreads - 1) / kThreads);
  for (uint32_t inst0 = 0; inst0 < (uint32_t)m.n; inst0 += 65535u) {
    const unsigned nz = (uint32_t)m.n - inst0 < 65535u ? (uint32_t)m.n - inst0 : 65535u;
    sr_args P;
    P.M = m.SR;
    P.T = m.T;
    P.gamma = m.gamma;
    P.sets = m.param_sets;
    P.index = m.param_index;
    P.n_sets = m.n_param_sets;
    P.S = S;
    P.k0 = 0;
    P.kb = 0;
    P.nbr = nbr;
    P.inst0 = inst0;
    COBEL_HIP_TRY(cobel_launch(P.index ? k_pma_sr_init<true> : k_pma_sr_init<false>,
                               dim3(init_blocks, 1, nz), dim3(kThreads), 0, st, P));
    for (int k0 = 0; k0 < S; k0 += kB) {
      P.k0 = k0;
      P.kb = S - k0 < kB ? S - k0 : kB;
      if (S > P.kb) {   // (else the diagonal block is the whole matrix)
        COBEL_HIP_TRY(cobel_launch(k_pma_sr_tiles, dim3(nt, nt, nz), dim3(kThreads),
                                   8 * kTileDoubles, st, P));
        COBEL_HIP_TRY(cobel_launch(k_pma_sr_lines, dim3(2u * (unsigned)nbr, 1, nz), dim3(kThreads),
                                   8 * kLineDoubles, st, P));
      }
      COBEL_HIP_TRY(cobel_launch(k_pma_sr_diag, dim3(1, 1, nz), dim3(kThreads), 8 * kDiagDoubles, st,
                                 P));
    }
  }
  return COBEL_OK;
}
