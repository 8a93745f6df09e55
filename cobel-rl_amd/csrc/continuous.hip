// The continuous 2D arena (interface/continuous.py of the reference): step and reset of thousands of
// instances in one launch each.  The arena is one table of directed edges a -> b with the interior
// to the left (exterior ring counter-clockwise, holes clockwise), eight float64 columns computed
// once on the host: ax ay bx by ex ey nx ny.  The kernels derive nothing else from the vertices.
//
// The layout (G lanes per instance over a staged edge table), the device functions and the launch
// planning live in cobel_c2d.h, which cobel_dqn_act_c2d (dqn_act_c2d.hip) shares.
//
// The file is compiled with -ffp-contract=off: every product and sum is rounded once, in the order
// written, as the float64 NumPy restatement in tests/c2d_common.py evaluates them.
#include "cobel_c2d.h"

using namespace cobel_c2d;

namespace {

__global__ __launch_bounds__(kBlock) void k_c2d_step(const cobel_c2d_t K, const int G,
                                                     const uint8_t* __restrict__ action,
                                                     double* __restrict__ reward_out,
                                                     uint8_t* __restrict__ done_out,
                                                     uint8_t* __restrict__ wall_out) {
  extern __shared__ double sh[];
  const int E = K.n_edges;
  stage_edges(sh, K.edges, E);
  const int j = (int)threadIdx.x & (G - 1);
  const long long inst = (long long)blockIdx.x * (kBlock / G) + (int)threadIdx.x / G;
  const bool valid = inst < (long long)K.n;
  const size_t i = valid ? (size_t)inst : 0;
  const double px = K.state[3 * i], py = K.state[3 * i + 1], th = K.state[3 * i + 2];
  const int a = action[i];
  const double m = fabs(K.buffer), half = m / 2.0, thr = half * half;
  double tx, ty, th2;
  const bool act_ok = action_target(K, px, py, th, a, tx, ty, th2);
  double cx, cy;
  group_move(sh, E, j, G, px, py, tx, ty, m, thr, cx, cy);
  if (!valid || j != 0) return;
  if (!act_ok) {   // an action the robot does not have: nothing happens
    reward_out[i] = 0.0;
    done_out[i] = 0;
    wall_out[i] = 0;
    return;
  }
  const bool hit = cx != tx || cy != ty;
  double reward;
  int end;
  step_outcome(K, cx, cy, hit, reward, end);
  K.state[3 * i] = cx;
  K.state[3 * i + 1] = cy;
  K.state[3 * i + 2] = th2;
  reward_out[i] = reward;
  done_out[i] = (uint8_t)end;
  wall_out[i] = hit ? 1 : 0;
}

// Continuous2D.reset in every instance the mask names (find_start, cobel_c2d.h)
__global__ __launch_bounds__(kBlock) void k_c2d_reset(const cobel_c2d_t K, const int G,
                                                      const uint8_t* __restrict__ mask,
                                                      int32_t* __restrict__ fallbacks) {
  extern __shared__ double sh[];
  stage_edges(sh, K.edges, K.n_edges);
  const int j = (int)threadIdx.x & (G - 1);
  const long long inst = (long long)blockIdx.x * (kBlock / G) + (int)threadIdx.x / G;
  const bool valid = inst < (long long)K.n;
  const size_t i = valid ? (size_t)inst : 0;
  const bool mine = valid && (!mask || mask[i] != 0);
  const uint32_t g = K.instance_base + (uint32_t)i;
  const uint32_t c = K.env_ctr[i];
  const double m = fabs(K.buffer), half = m / 2.0, thr = half * half;
  const start_point p = find_start(K, sh, j, G, g, c, thr, mine);
  if (!mine || j != 0) return;
  K.state[3 * i] = p.x;
  K.state[3 * i + 1] = p.y;
  K.state[3 * i + 2] = start_orientation(K, g, c, p);
  K.env_ctr[i] = c + p.adv;
  if (p.fell_back) atomicAdd(fallbacks, 1);
}

}  // namespace

extern "C" int cobel_c2d_plan(int32_t n, int32_t n_edges, int32_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_c2d_plan: NULL out");
  COBEL_REQUIRE(n >= 0, COBEL_E_RANGE, "cobel_c2d_plan: n = %d", n);
  COBEL_REQUIRE(n_edges >= 1 && n_edges <= COBEL_C2D_MAX_EDGES, COBEL_E_RANGE,
                "cobel_c2d_plan: %d edges (an arena serves 1 to %d)", n_edges,
                COBEL_C2D_MAX_EDGES);
  const int G = plan_lanes(n, n_edges);
  const long long per_block = kBlock / G;
  out[0] = G;
  out[1] = kBlock;
  out[2] = (int32_t)(kCols * n_edges * (int)sizeof(double));
  out[3] = (int32_t)((n + per_block - 1) / per_block);
  return COBEL_OK;
}

extern "C" int cobel_c2d_step(const cobel_c2d_t* c2d, const uint8_t* action, double* reward,
                              uint8_t* done, uint8_t* wall, void* stream) {
  if (int rc = check_c2d(c2d, "cobel_c2d_step")) return rc;
  COBEL_REQUIRE(action && reward && done && wall, COBEL_E_ARG, "cobel_c2d_step: NULL argument");
  COBEL_REQUIRE(((uintptr_t)reward & 7u) == 0, COBEL_E_ARG, "cobel_c2d_step: misaligned reward");
  if (c2d->n == 0) return COBEL_OK;
  const c2d_launch L = launch_shape(c2d);
  hipLaunchKernelGGL(k_c2d_step, dim3(L.grid), dim3(kBlock), L.lds, (hipStream_t)stream, *c2d,
                     L.G, action, reward, done, wall);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

extern "C" int cobel_c2d_reset(const cobel_c2d_t* c2d, const uint8_t* mask, int32_t* fallbacks,
                               void* stream) {
  if (int rc = check_c2d(c2d, "cobel_c2d_reset")) return rc;
  COBEL_REQUIRE(fallbacks && ((uintptr_t)fallbacks & 3u) == 0, COBEL_E_ARG,
                "cobel_c2d_reset: the fallback counter must be given, aligned");
  if (c2d->n == 0) return COBEL_OK;
  const c2d_launch L = launch_shape(c2d);
  hipLaunchKernelGGL(k_c2d_reset, dim3(L.grid), dim3(kBlock), L.lds, (hipStream_t)stream, *c2d,
                     L.G, mask, fallbacks);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}
