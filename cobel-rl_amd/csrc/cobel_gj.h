// In-place Gauss-Jordan without pivoting on an S x S float64 matrix in global memory, blocked over
// panels of kB pivots: the device functions pma_sr.hip (PMAMemory.update_sr beyond the LDS) and
// metric.hip (the SFMA metrics) build their kernels from.  Every element goes through the
// operations of the element-wise elimination in the same order — pivots k = 0 .. S-1 ascending; the
// pivot row scaled by 1 / pivot (the pivot's own place takes 1 / pivot); every other element
// M - col[r] * row[c] (0 - col[r] * row[k] in column k), one rounding per operation — so the result
// equals the element-wise one bit for bit.
//
// A panel K = [k0, k0 + kb) splits the matrix into the diagonal block M[K][K], the column panel
// M[r][K] (r outside K), the row panel M[K][c] (c outside K) and the rest.  Through the kb steps
//   the diagonal block depends on itself alone:         its evolution gives, per step k, 1 / pivot,
//                                                       col_k[K] and row_k[K]
//   a row r of the column panel depends on row_k[K]:    col_k[r] is its entry k before step k
//   a column c of the row panel depends on col_k[K]:    row_k[c] is its entry k / pivot at step k
//   an element of the rest takes  M - col_k[r] * row_k[c]  for k ascending
// Three launches per panel, ordered by the stream (nothing waits inside a kernel):
//   gj_tiles  one workgroup per 64 x 64 tile of the rest, so one matrix spreads over the chip: it
//             reads the OLD diagonal block and its 64 rows / 64 columns of the old panels, redoes
//             their eliminations in LDS (that gives col_k / row_k of its rows and columns; no
//             scratch memory is needed for them), then loads the tile once, applies the kb rank-1
//             updates from LDS and stores it once
//   gj_lines  one lane per row of the column panel / column of the row panel: the panels
//             themselves, in place
//   gj_diag   the diagonal block, in place (after every reader of the old one)
// The redundant panel work in gj_tiles equals the tile work at S = 1 024 (2 * 64 lines of kb^2
// operations against 64^2 * kb per tile).  All index arithmetic on M is in size_t.
#pragma once
#include "cobel_common.h"

namespace cobel_gj {

constexpr int kB = 32;          // pivots per panel
constexpr int kTile = 64;       // the rest in kTile x kTile tiles
constexpr int kThreads = 256;
constexpr int kLd = kB + 1;     // row stride of the diagonal block in LDS
// Strides of the staged panels, one past the line count: the staging loops run their lanes along a
// line (that is how memory is read in whole segments), and an even stride of 64 or 256 doubles
// would put every lane of such a store into one LDS bank.
constexpr int kTileLd = kTile + 1;
constexpr int kLineLd = kThreads + 1;

// LDS of the diagonal block's evolution: the block, then per step the column, the scaled row, 1 / pivot
struct sr_diag {
  double *D, *colk, *rowk, *inv;   // [kB][kLd] [kB][kB] [kB][kB] [kB]
};
constexpr size_t kDiagDoubles = (size_t)kB * kLd + 2 * (size_t)kB * kB + kB;
__device__ __forceinline__ sr_diag diag_carve(double* base) {
  sr_diag d;
  d.D = base;
  d.colk = d.D + kB * kLd;
  d.rowk = d.colk + kB * kB;
  d.inv = d.rowk + kB * kB;
  return d;
}

__device__ __forceinline__ void diag_load(const sr_diag& d, const double* M, int S, int k0, int kb,
                                          int t) {
  for (int e = t; e < kb * kb; e += kThreads) {
    const int i = e / kb, j = e - i * kb;
    d.D[i * kLd + j] = M[(size_t)(k0 + i) * S + k0 + j];
  }
}

// the kb steps on the diagonal block (the caller's loads into d.D need no barrier before)
__device__ __forceinline__ void diag_evolve(const sr_diag& d, int kb, int t) {
  for (int kk = 0; kk < kb; ++kk) {
    __syncthreads();
    const double inv = 1.0 / d.D[kk * kLd + kk];
    if (t < kb) {
      d.colk[kk * kB + t] = d.D[t * kLd + kk];
    } else if (t >= 64 && t - 64 < kb) {
      const int j = t - 64;
      d.rowk[kk * kB + j] = (j == kk ? 1.0 : d.D[kk * kLd + j]) * inv;
    } else if (t == 128) {
      d.inv[kk] = inv;
    }
    __syncthreads();
    for (int e = t; e < kb * kb; e += kThreads) {
      const int i = e / kb, j = e - i * kb;
      const double row = d.rowk[kk * kB + j];
      if (i == kk) d.D[i * kLd + j] = row;
      else d.D[i * kLd + j] = (j == kk ? 0.0 : d.D[i * kLd + j]) - d.colk[kk * kB + i] * row;
    }
  }
  __syncthreads();
}

// A row of the column panel, v[j * ld] = M[r][k0 + j], through the kb steps; col[kk * ldc] takes
// col_k[r] (col == nullptr: not wanted)
__device__ __forceinline__ void col_line(double* v, int ld, const double* rowk, int kb, double* col,
                                         int ldc) {
  for (int kk = 0; kk < kb; ++kk) {
    const double cv = v[kk * ld];
    if (col) col[kk * ldc] = cv;
    for (int j = 0; j < kb; ++j) {
      const double x = v[j * ld];
      v[j * ld] = (j == kk ? 0.0 : x) - cv * rowk[kk * kB + j];
    }
  }
}
// A column of the row panel, w[i * ld] = M[k0 + i][c]; row[kk * ldr] takes row_k[c]
__device__ __forceinline__ void row_line(double* w, int ld, const double* colk, const double* inv,
                                         int kb, double* row, int ldr) {
  for (int kk = 0; kk < kb; ++kk) {
    const double rv = w[kk * ld] * inv[kk];
    if (row) row[kk * ldr] = rv;
    for (int i = 0; i < kb; ++i) {
      const double x = w[i * ld];
      w[i * ld] = i == kk ? rv : x - colk[kk * kB + i] * rv;
    }
  }
}

// The bodies of the three kernels of a panel on matrix M (the caller's kernel picks its matrix by
// blockIdx.z and hands on its dynamic LDS).  gj_tiles: grid (ceil(S / kTile), ceil(S / kTile)).
constexpr size_t kTileDoubles = kDiagDoubles + (size_t)kB * kTileLd + 3 * (size_t)kB * kTile;
__device__ __forceinline__ void gj_tiles(double* const M, const int S, const int k0, const int kb,
                                         double* const lds) {
  const sr_diag d = diag_carve(lds);
  double* const As = lds + kDiagDoubles;       // [kB][kTileLd] As[j][r] = M[R0 + r][k0 + j]
  double* const Bs = As + kB * kTileLd;         // [kB][kTile] Bs[i][c] = M[k0 + i][C0 + c]
  double* const cols = Bs + kB * kTile;        // [kB][kTile] col_k[R0 + r]
  double* const rows = cols + kB * kTile;      // [kB][kTile] row_k[C0 + c]
  const int t = (int)threadIdx.x;
  const int k1 = k0 + kb;
  const int R0 = (int)blockIdx.y * kTile, C0 = (int)blockIdx.x * kTile;
  diag_load(d, M, S, k0, kb, t);
  for (int e = t; e < kTile * kb; e += kThreads) {
    const int r = e / kb, j = e - r * kb;
    As[j * kTileLd + r] = R0 + r < S ? M[(size_t)(R0 + r) * S + k0 + j] : 0.0;
  }
  for (int e = t; e < kb * kTile; e += kThreads) {
    const int i = e / kTile, c = e - i * kTile;
    Bs[i * kTile + c] = C0 + c < S ? M[(size_t)(k0 + i) * S + C0 + c] : 0.0;
  }
  diag_evolve(d, kb, t);
  if (t < kTile) {
    const int r = R0 + t;
    if (r < S && (r < k0 || r >= k1)) col_line(As + t, kTileLd, d.rowk, kb, cols + t, kTile);
    else
      for (int kk = 0; kk < kb; ++kk) cols[kk * kTile + t] = 0.0;
  } else if (t < 2 * kTile) {
    const int cl = t - kTile, c = C0 + cl;
    if (c < S && (c < k0 || c >= k1)) row_line(Bs + cl, kTile, d.colk, d.inv, kb, rows + cl, kTile);
    else
      for (int kk = 0; kk < kb; ++kk) rows[kk * kTile + cl] = 0.0;
  }
  __syncthreads();
  // the tile: lane (t / 16, t % 16) holds 4 x 4 elements
  const int tr = (t / 16) * 4, tc = (t % 16) * 4;
  double m[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = R0 + tr + i, c = C0 + tc + j;
      m[i][j] = (r < S && c < S) ? M[(size_t)r * S + c] : 0.0;
    }
  for (int kk = 0; kk < kb; ++kk) {
    double a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = cols[kk * kTile + tr + i];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = rows[kk * kTile + tc + j];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) m[i][j] = m[i][j] - a[i] * b[j];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = R0 + tr + i, c = C0 + tc + j;
      if (r < S && c < S && (r < k0 || r >= k1) && (c < k0 || c >= k1)) M[(size_t)r * S + c] = m[i][j];
    }
}

// gj_lines: grid (2 nbr), nbr = ceil(S / kThreads); blocks [0, nbr): kThreads rows of the column
// panel each; blocks [nbr, 2 nbr): columns of the row panel
constexpr size_t kLineDoubles = kDiagDoubles + (size_t)kB * kLineLd;
__device__ __forceinline__ void gj_lines(double* const M, const int S, const int k0, const int kb,
                                         const int nbr, double* const lds) {
  const sr_diag d = diag_carve(lds);
  double* const V = lds + kDiagDoubles;        // [kB][kLineLd]
  const int t = (int)threadIdx.x;
  const int k1 = k0 + kb;
  const bool is_rows = (int)blockIdx.x < nbr;
  const int base = ((int)blockIdx.x - (is_rows ? 0 : nbr)) * kThreads;
  diag_load(d, M, S, k0, kb, t);
  if (is_rows) {
    for (int e = t; e < kThreads * kb; e += kThreads) {
      const int r = e / kb, j = e - r * kb;
      V[j * kLineLd + r] = base + r < S ? M[(size_t)(base + r) * S + k0 + j] : 0.0;
    }
  } else {
    for (int e = t; e < kb * kThreads; e += kThreads) {
      const int i = e / kThreads, c = e - i * kThreads;
      V[i * kLineLd + c] = base + c < S ? M[(size_t)(k0 + i) * S + base + c] : 0.0;
    }
  }
  diag_evolve(d, kb, t);
  const int line = base + t;
  if (line < S && (line < k0 || line >= k1)) {
    if (is_rows) col_line(V + t, kLineLd, d.rowk, kb, nullptr, 0);
    else row_line(V + t, kLineLd, d.colk, d.inv, kb, nullptr, 0);
  }
  __syncthreads();
  if (is_rows) {
    for (int e = t; e < kThreads * kb; e += kThreads) {
      const int rl = e / kb, j = e - rl * kb, r = base + rl;
      if (r < S && (r < k0 || r >= k1)) M[(size_t)r * S + k0 + j] = V[j * kLineLd + rl];
    }
  } else {
    for (int e = t; e < kb * kThreads; e += kThreads) {
      const int i = e / kThreads, cl = e - i * kThreads, c = base + cl;
      if (c < S && (c < k0 || c >= k1)) M[(size_t)(k0 + i) * S + c] = V[i * kLineLd + cl];
    }
  }
}

// gj_diag: one workgroup
__device__ __forceinline__ void gj_diag(double* const M, const int S, const int k0, const int kb,
                                        double* const lds) {
  const sr_diag d = diag_carve(lds);
  const int t = (int)threadIdx.x;
  diag_load(d, M, S, k0, kb, t);
  diag_evolve(d, kb, t);
  for (int e = t; e < kb * kb; e += kThreads) {
    const int i = e / kb, j = e - i * kb;
    M[(size_t)(k0 + i) * S + k0 + j] = d.D[i * kLd + j];
  }
}

}  // namespace cobel_gj
