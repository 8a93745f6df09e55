// The spatial analysis of layer activity (analysis/network_spatial.py) for many maps at once:
//
//   cobel_activity_process   process_activity_maps (network_spatial.py:45-67) on [R][P] rows in
//                            place: x -= min, x /= max(x), x[x < threshold] = 0.  One wavefront per
//                            row; min and max are order-free and the two operations per element
//                            are IEEE, so the rows equal NumPy's bit for bit.
//   cobel_place_fields       classify_place_field with sigma = 0 (network_spatial.py:70-144) for M
//                            maps of H x W cells: one wavefront per map, the thresholded map, the
//                            labels and the bounding boxes in LDS.
//
// Labelling.  scipy.ndimage.label numbers the 4-connected components of field > 0 by their first
// cell in row-major order; here a component is named by that cell's index, the root of a union-find
// forest whose links only ever point to smaller indices:
//   1. every foreground cell points to its left neighbour if that is foreground, else to itself;
//      ceil(log2 W) rounds of pointer jumping make it point to the start of its row run;
//   2. a cell whose upper neighbour is foreground unites the two runs (atomicMin hooks the larger
//      root under the smaller) — only where the overlap of the two runs begins, i.e. not if the left
//      and the upper-left neighbour are foreground too;
//   3. every cell follows its links to the root.
// The rounds of a sweep that hands minima to neighbours grow with the length of a component (a
// serpentine through 64 x 64 cells: thousands); here a find walks at most one link per run.
// Roots are then numbered in row-major order (ballot + popcount), every cell takes its root's number,
// and three atomicMax per cell give each component its bounding box (the first row is the root's).
//
// NaN.  np.amin / np.amax / np.max propagate NaN, the device's fmin / fmax do not: reductions carry a
// flag.  A row with a NaN becomes all NaN, a constant row too (0 / 0), and NaN < threshold is false:
// they stay.  A map with a NaN has a NaN cutoff, a < NaN is false, the map stays as it is, and a NaN
// cell is background (NaN > 0 is false).
#include "cobel_common.h"

namespace {

constexpr int kMaxCells = 4096;          // H W of a map: cell indices fit 12 bits
constexpr uint32_t kBG = 0xffffffffu;    // label of a background cell
constexpr uint32_t kNumbered = 0x80000000u, kRoot = 0x40000000u, kOrd = 0xfffu;

template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T nan_of();
template <>
__device__ __forceinline__ float nan_of<float>() { return __builtin_nanf(""); }
template <>
__device__ __forceinline__ double nan_of<double>() { return __builtin_nan(""); }
template <typename T>
__device__ __forceinline__ T inf_of();
template <>
__device__ __forceinline__ float inf_of<float>() { return __builtin_inff(); }
template <>
__device__ __forceinline__ double inf_of<double>() { return __builtin_inf(); }

// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_activity_process(T* __restrict__ rows, int64_t R, int32_t P,
                                                          T threshold) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (r >= R) return;   // (whole wavefronts)
  T* const x = rows + (size_t)r * (size_t)P;
  T lo = inf_of<T>(), hi = -inf_of<T>();
  bool nan = false;
  for (int p = lane; p < P; p += 64) {
    const T v = x[p];
    nan = nan || v != v;
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  nan = __any(nan);
  // max(x - min) = fl(max - min): rounding is monotone.  An infinite minimum meets itself in the
  // row (inf - inf): NumPy's maximum of the differences is NaN then.
  T denom = hi - lo;
  if (nan || lo == inf_of<T>() || lo == -inf_of<T>()) {
    lo = nan ? nan_of<T>() : lo;
    denom = nan_of<T>();
  }
  for (int p = lane; p < P; p += 64) {
    const T v = (x[p] - lo) / denom;
    x[p] = v < threshold ? (T)0 : v;
  }
}

// ---------------------------------------------------------------------------------------------
// LDS of one map: the field [HW] T, the labels [HW] u32, three bounding-box tables [(HW + 1) / 2]
// u32 (a component has at least one cell and no two components touch: at most (HW + 1) / 2).
__host__ __device__ inline size_t pf_tables(int HW) { return (size_t)((HW + 1) / 2); }
__host__ __device__ inline size_t pf_map_bytes(int HW, int is_float64) {
  const size_t b = (size_t)HW * (is_float64 ? 8 : 4) + (size_t)HW * 4 + 3 * pf_tables(HW) * 4;
  return (b + 15) & ~(size_t)15;
}
inline int pf_maps_per_wg(int HW, int is_float64) {
  const size_t per = pf_map_bytes(HW, is_float64);
  const size_t fit = (64 * 1024) / per;
  return fit >= 4 ? 4 : fit >= 1 ? (int)fit : 1;
}

struct pf_args {
  const void* maps;
  uint8_t* has_field;
  int32_t* error;
  int32_t* features;
  int32_t* largest_area;
  void* fields;
  int64_t n_maps;
  int32_t H, W, map_bytes;
  double cutoff, size_threshold;
};

__device__ __forceinline__ uint32_t pf_find(const volatile uint32_t* parent, uint32_t a) {
  uint32_t p;
  while ((p = parent[a]) != a) a = p;
  return a;
}
// links only ever point to smaller indices, so the root of a component is its first cell
__device__ __forceinline__ void pf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  while (true) {
    a = pf_find(parent, a);
    b = pf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t s = a;
      a = b;
      b = s;
    }
    const uint32_t old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;   // (another lane hooked a first: its new parent and b are still to be united)
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_place_fields(const pf_args A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pf_lds[];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t m = (int64_t)blockIdx.x * (int64_t)(blockDim.x >> 6) + wave;
  if (m >= A.n_maps) return;   // (whole wavefronts; no workgroup barrier below)
  const int H = A.H, W = A.W, HW = H * W;
  unsigned char* const base = pf_lds + (size_t)wave * (size_t)A.map_bytes;
  T* const field = reinterpret_cast<T*>(base);
  uint32_t* const parent = reinterpret_cast<uint32_t*>(field + HW);
  const int NT = (int)pf_tables(HW);
  uint32_t* const max_r = parent + HW;
  uint32_t* const max_c = max_r + NT;
  uint32_t* const inv_c = max_c + NT;   // kMaxCells - 1 - column: its maximum is the first column
  const T* const a = (const T*)A.maps + (size_t)m * (size_t)HW;
  T* const out = (T*)A.fields + (size_t)m * (size_t)HW;

  // ---- thr = cutoff * max(a); field = a < thr ? 0 : a ------------------------------------------
  T hi = -inf_of<T>();
  bool nan = false;
  for (int c = lane; c < HW; c += 64) {
    const T v = a[c];
    field[c] = v;
    nan = nan || v != v;
    hi = v > hi ? v : hi;
  }
  hi = wave_max(hi);
  if (__any(nan)) hi = nan_of<T>();
  const T thr = (T)A.cutoff * hi;
  wsync();
  for (int c = lane; c < HW; c += 64) {
    const T v = field[c];
    field[c] = v < thr ? (T)0 : v;
  }
  wsync();

  // ---- 1. row runs -------------------------------------------------------------------------------
  for (int c = lane; c < HW; c += 64) {
    uint32_t p = kBG;
    if (field[c] > (T)0) p = (c % W != 0 && field[c - 1] > (T)0) ? (uint32_t)(c - 1) : (uint32_t)c;
    parent[c] = p;
  }
  wsync();
  for (int span = 1; span < W; span <<= 1) {
    for (int c = lane; c < HW; c += 64) {
      const uint32_t p = parent[c];
      if (p != kBG) parent[c] = parent[p];
    }
    wsync();
  }
  // ---- 2. runs that touch across rows -------------------------------------------------------------
  for (int c = lane + W; c < HW; c += 64) {
    if (parent[c] == kBG || parent[c - W] == kBG) continue;
    if (c % W != 0 && parent[c - 1] != kBG && parent[c - W - 1] != kBG) continue;
    pf_unite(parent, (uint32_t)c, (uint32_t)(c - W));
  }
  wsync();
  // ---- 3. every cell to its root ------------------------------------------------------------------
  for (int c = lane; c < HW; c += 64) {
    if (parent[c] != kBG) parent[c] = pf_find(parent, (uint32_t)c);
  }
  wsync();

  // ---- roots numbered in row-major order, every cell takes its root's number ---------------------
  int count = 0;
  for (int c0 = 0; c0 < HW; c0 += 64) {
    const int c = c0 + lane;
    const bool root = c < HW && parent[c] == (uint32_t)c;
    const unsigned long long mask = __ballot(root);
    if (root) {
      const int ord = count + __popcll(mask & ((1ull << lane) - 1ull));
      max_r[ord] = 0u;
      max_c[ord] = 0u;
      inv_c[ord] = 0u;
      parent[c] = kNumbered | kRoot | (uint32_t)ord;
    }
    count += __popcll(mask);
  }
  wsync();
  for (int c = lane; c < HW; c += 64) {
    const uint32_t p = parent[c];
    if (p != kBG && !(p & kNumbered)) parent[c] = parent[p] & ~kRoot;
  }
  wsync();

  int32_t error, best_area = HW, best_ord = -1;
  if (count > 0) {
    // ---- bounding boxes --------------------------------------------------------------------------
    for (int c = lane; c < HW; c += 64) {
      const uint32_t p = parent[c];
      if (p == kBG) continue;
      const uint32_t ord = p & kOrd, row = (uint32_t)(c / W), col = (uint32_t)(c % W);
      atomicMax(&max_r[ord], row);
      atomicMax(&max_c[ord], col);
      atomicMax(&inv_c[ord], (uint32_t)(kMaxCells - 1) - col);
    }
    wsync();
    // ---- the largest box, the first of equals: max of area << 12 | (4095 - number) ----------------
    uint32_t key = 0u;
    for (int c = lane; c < HW; c += 64) {
      const uint32_t p = parent[c];
      if (p == kBG || !(p & kRoot)) continue;
      const uint32_t ord = p & kOrd;
      const uint32_t rows = max_r[ord] - (uint32_t)(c / W) + 1u;
      const uint32_t cols = max_c[ord] - ((uint32_t)(kMaxCells - 1) - inv_c[ord]) + 1u;
      const uint32_t k = ((rows * cols) << 12) | (kOrd - ord);
      key = k > key ? k : key;
    }
    key = wave_max(key);
    best_area = (int32_t)(key >> 12);
    best_ord = (int32_t)(kOrd - (key & kOrd));
    error = count > 4 ? 2 : ((double)best_area > A.size_threshold * (double)HW ? 3 : 0);
  } else {
    error = 1;
  }
  // ---- outputs -------------------------------------------------------------------------------------
  for (int c = lane; c < HW; c += 64) {
    const uint32_t p = parent[c];
    T v = field[c];
    if (count > 0 && !(p != kBG && (int32_t)(p & kOrd) == best_ord)) v = (T)0;
    out[c] = v;
  }
  if (lane == 0) {
    A.has_field[m] = error == 0 ? 1 : 0;
    A.error[m] = error;
    A.features[m] = count;
    A.largest_area[m] = best_area;
  }
}

int pf_shape(int32_t H, int32_t W) {
  COBEL_REQUIRE(H >= 1 && W >= 1, COBEL_E_RANGE, "cobel_place_fields: maps of %d x %d cells", H, W);
  COBEL_REQUIRE((int64_t)H * (int64_t)W <= kMaxCells, COBEL_E_UNSUPPORTED,
                "cobel_place_fields: maps of at most %d cells are covered (got %d x %d)", kMaxCells,
                H, W);
  return COBEL_OK;
}

}  // namespace

extern "C" int cobel_activity_process(void* rows, int64_t n_rows, int32_t n_cols,
                                      int32_t is_float64, double threshold, void* stream) {
  COBEL_REQUIRE(rows, COBEL_E_ARG, "cobel_activity_process: NULL rows");
  COBEL_REQUIRE(n_rows >= 0 && n_cols >= 1 && (n_rows + 3) / 4 <= 0x7fffffffLL, COBEL_E_RANGE,
                "cobel_activity_process: %lld rows of %d elements", (long long)n_rows, n_cols);
  if (n_rows == 0) return COBEL_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n_rows + 3) / 4));
  if (is_float64)
    hipLaunchKernelGGL(k_activity_process<double>, grid, dim3(256), 0, st, (double*)rows, n_rows,
                       n_cols, threshold);
  else
    hipLaunchKernelGGL(k_activity_process<float>, grid, dim3(256), 0, st, (float*)rows, n_rows,
                       n_cols, (float)threshold);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

extern "C" int cobel_place_fields_plan(int32_t height, int32_t width, int32_t is_float64,
                                       int32_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_place_fields_plan: NULL out");
  if (int rc = pf_shape(height, width)) return rc;
  const int HW = height * width, f64 = is_float64 ? 1 : 0;
  const int per_wg = pf_maps_per_wg(HW, f64);
  out[0] = (int32_t)(pf_map_bytes(HW, f64) * per_wg);
  out[1] = per_wg;
  out[2] = (int32_t)pf_map_bytes(HW, f64);
  out[3] = 64 * per_wg;
  return COBEL_OK;
}

extern "C" int cobel_place_fields(const void* maps, int64_t n_maps, int32_t height, int32_t width,
                                  int32_t is_float64, double cutoff, double size_threshold,
                                  uint8_t* has_field, int32_t* error, int32_t* features,
                                  int32_t* largest_area, void* fields, void* stream) {
  COBEL_REQUIRE(maps && has_field && error && features && largest_area && fields, COBEL_E_ARG,
                "cobel_place_fields: NULL maps or outputs");
  int32_t plan[4];
  if (int rc = cobel_place_fields_plan(height, width, is_float64, plan)) return rc;
  COBEL_REQUIRE(size_threshold > 0.0 && size_threshold < 1.0, COBEL_E_ARG,
                "cobel_place_fields: The field size threshold is invalid! (%g)", size_threshold);
  COBEL_REQUIRE(cutoff > 0.0 && cutoff < 1.0, COBEL_E_ARG,
                "cobel_place_fields: The activity cutoff threshold is invalid! (%g)", cutoff);
  COBEL_REQUIRE(n_maps >= 0 && (n_maps + plan[1] - 1) / plan[1] <= 0x7fffffffLL, COBEL_E_RANGE,
                "cobel_place_fields: %lld maps", (long long)n_maps);
  if (n_maps == 0) return COBEL_OK;
  pf_args A;
  A.maps = maps;
  A.has_field = has_field;
  A.error = error;
  A.features = features;
  A.largest_area = largest_area;
  A.fields = fields;
  A.n_maps = n_maps;
  A.H = height;
  A.W = width;
  A.map_bytes = plan[2];
  A.cutoff = cutoff;
  A.size_threshold = size_threshold;
  const dim3 grid((unsigned)((n_maps + plan[1] - 1) / plan[1])), block((unsigned)plan[3]);
  if (is_float64)
    COBEL_HIP_TRY(cobel_launch(k_place_fields<double>, grid, block, (size_t)plan[0],
                               (hipStream_t)stream, A));
  else
    COBEL_HIP_TRY(cobel_launch(k_place_fields<float>, grid, block, (size_t)plan[0],
                               (hipStream_t)stream, A));
  return COBEL_OK;
}
