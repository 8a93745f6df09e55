// The continuous 2D arena (interface/continuous.py of the reference): step and reset of thousands of
// instances in one launch each.  The arena is one table of directed edges a -> b with the interior
// to the left (exterior ring counter-clockwise, holes clockwise), eight float64 columns computed
// once on the host: ax ay bx by ex ey nx ny.  The kernels derive nothing else from the vertices.
//
// Layout.  A workgroup of 256 lanes stages the table into LDS as eight arrays of E doubles (64 KiB
// at the cap of 1 024 edges) and serves 256 / G instances, G lanes each:
//   G = 1            every lane walks the edges in order; the 64 lanes of a wave read the same LDS
//                    address at the same time, which the LDS serves as one broadcast.
//   G = 4, 16, 64    lane j of a group takes the edges j, j + G, j + 2G ...; consecutive lanes read
//                    consecutive doubles, the groups of a wave the same ones.  The group combines
//                    the crossing parity by xor, the clearance test by "any", the first hit
//                    (t, edge) by the lexicographic minimum, through __shfl_xor butterflies.
// Nothing is summed across edges: every per-edge value is rounded by itself, a parity and an "any"
// do not depend on the order, and the minimum of (t, edge) under "smaller t, then smaller edge" is
// the minimum of a total order — the edge that wins brings its own t along.  So the results are
// the same bits for every G.
//
// The file is compiled with -ffp-contract=off: every product and sum below is rounded once, in the
// order written, as the float64 NumPy restatement in tests/c2d_common.py evaluates them.
#include "cobel_common.h"

namespace {

constexpr int kBlock = 256;
enum { AX = 0, AY, BX, BY, EX, EY, NX, NY, kCols };
constexpr int kNoEdge = 0x7fffffff;

__device__ __forceinline__ int group_xor(int v, int G) {
  for (int o = 1; o < G; o <<= 1) v ^= __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int group_or(int v, int G) {
  for (int o = 1; o < G; o <<= 1) v |= __shfl_xor(v, o);
  return v;
}

// Even-odd rule: the crossings of the ray from p towards +x that lane j of its group counts
// (edges j, j + G ...), as a parity.  `t` is a table of kCols columns of E doubles.
__device__ __forceinline__ int parity_part(const double* t, int E, int j, int G, double px,
                                           double py) {
  int par = 0;
  for (int e = j; e < E; e += G) {
    const double ax = t[AX * E + e], ay = t[AY * E + e], by = t[BY * E + e], ex = t[EX * E + e];
    const bool straddles = (ay > py) != (by > py);
    const double xi = ax + (py - ay) / (by - ay) * ex;
    par ^= (straddles && px < xi) ? 1 : 0;
  }
  return par;
}

// This lane's share of clear(p): bit 0 the crossing parity, bit 1 "some edge is nearer than m / 2"
__device__ __forceinline__ int clear_part(const double* t, int E, int j, int G, double px,
                                          double py, double thr) {
  int par = 0, near = 0;
  for (int e = j; e < E; e += G) {
    const double ax = t[AX * E + e], ay = t[AY * E + e], by = t[BY * E + e];
    const double ex = t[EX * E + e], ey = t[EY * E + e];
    const bool straddles = (ay > py) != (by > py);
    const double xi = ax + (py - ay) / (by - ay) * ex;
    par ^= (straddles && px < xi) ? 1 : 0;
    double s = ((px - ax) * ex + (py - ay) * ey) / (ex * ex + ey * ey);
    s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    const double qx = ax + s * ex, qy = ay + s * ey;
    const double d2 = (px - qx) * (px - qx) + (py - qy) * (py - qy);
    near |= !(d2 >= thr) ? 1 : 0;
  }
  return par | (near << 1);
}

// clear(p) for the whole group; to be called in wave-uniform control flow
__device__ __forceinline__ bool group_clear(const double* t, int E, int j, int G, double px,
                                            double py, double thr) {
  const int part = clear_part(t, E, j, G, px, py, thr);
  const int par = group_xor(part & 1, G), near = group_or(part >> 1, G);
  return par == 1 && near == 0;
}

// move(p, target): where the robot ends; to be called in wave-uniform control flow
__device__ __forceinline__ void group_move(const double* t, int E, int j, int G, double px,
                                           double py, double tx, double ty, double m, double thr,
                                           double& cx, double& cy) {
  const double dx = tx - px, dy = ty - py;
  double bt = __builtin_inf();
  int be = kNoEdge;
  for (int e = j; e < E; e += G) {
    const double nx = t[NX * E + e], ny = t[NY * E + e];
    const double den = dx * nx + dy * ny;
    if (!(den < 0.0)) continue;
    const double ax = t[AX * E + e], ay = t[AY * E + e];
    const double ex = t[EX * E + e], ey = t[EY * E + e];
    const double sd = (px - ax) * nx + (py - ay) * ny;
    const double tt = sd / (-den);
    if (!(tt >= 0.0 && tt <= 1.0)) continue;
    const double hx = px + tt * dx, hy = py + tt * dy;
    const double u = ((hx - ax) * ex + (hy - ay) * ey) / (ex * ex + ey * ey);
    if (!(u >= -1e-9 && u <= 1.0 + 1e-9)) continue;
    if (tt < bt) {   // (ascending e inside a lane: the lowest index keeps a tie)
      bt = tt;
      be = e;
    }
  }
  for (int o = 1; o < G; o <<= 1) {
    const double ot = __shfl_xor(bt, o);
    const int oe = __shfl_xor(be, o);
    if (ot < bt || (ot == bt && oe < be)) {
      bt = ot;
      be = oe;
    }
  }
  cx = tx;
  cy = ty;
  if (be != kNoEdge) {
    cx = (px + bt * dx) + m * t[NX * E + be];
    cy = (py + bt * dy) + m * t[NY * E + be];
  }
  if (!group_clear(t, E, j, G, cx, cy, thr)) {
    cx = px;
    cy = py;
  }
}

// a % b as NumPy evaluates it for float64 (b > 0)
__device__ __forceinline__ double py_mod(double a, double b) {
  double r = fmod(a, b);
  if (r != 0.0) {
    if (r < 0.0) r += b;
  } else {
    r = 0.0;
  }
  return r;
}

__device__ __forceinline__ void stage_edges(double* sh, const double* __restrict__ edges, int E) {
  for (int k = (int)threadIdx.x; k < kCols * E; k += kBlock) sh[k] = edges[k];
  __syncthreads();
}

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
  const double s = K.step_size;
  const double m = fabs(K.buffer), half = m / 2.0, thr = half * half;
  double tx = px, ty = py, th2 = th;
  bool act_ok;
  if (K.robot_type == COBEL_C2D_STEP) {   // continuous.py:211-219
    act_ok = a < 4;
    const double ux = a == 0 ? -1.0 : (a == 2 ? 1.0 : 0.0);
    const double uy = a == 1 ? 1.0 : (a == 3 ? -1.0 : 0.0);
    tx = px + ux * s;
    ty = py + uy * s;
  } else {                                // continuous.py:223-250
    act_ok = a < 3;
    if (a == 2) {
      tx = px + cos(th) * s;
      ty = py + sin(th) * s;
    } else {
      const double v0 = (a == 0 ? 0.0 : 1.0) * s, v1 = (a == 0 ? 1.0 : 0.0) * s;
      const double wd = K.wheel_distance;
      const double om = (v1 - v0) / wd;
      const double R = 0.5 * wd * ((v0 + v1) / (v1 - v0));
      const double sn = sin(th);
      const double iccx = px - R * sn, iccy = py + R * sn;
      const double relx = px - iccx, rely = py - iccy;
      const double co = cos(om), so = sin(om);
      tx = (co * relx - so * rely) + iccx;
      ty = (so * relx + co * rely) + iccy;
      th2 = th + th;
    }
    th2 = py_mod(th2, 2.0 * 3.141592653589793);
  }
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
  double reward = 0.0;
  int end = 0;
  int k = 0;
  for (; k < K.n_rewards; ++k) {          // continuous.py:254-259: the first row in reach
    const double rx = K.rewards[3 * k] - cx, ry = K.rewards[3 * k + 1] - cy;
    if (sqrt(rx * rx + ry * ry) <= K.body_radius * 2.0) break;
  }
  if (k < K.n_rewards) {
    reward = K.rewards[3 * k + 2];
    end = 1;
  } else if (hit && K.punish_wall) {
    reward = -10.0;
  }
  K.state[3 * i] = cx;
  K.state[3 * i + 1] = cy;
  K.state[3 * i + 2] = th2;
  reward_out[i] = reward;
  done_out[i] = (uint8_t)end;
  wall_out[i] = hit ? 1 : 0;
}

// Rejection sampling of the start (continuous.py:280-291) with a bound: 1 024 candidates, then the
// host's fallback point.  The spawn table is read in place (a reset is rare; the table stays in L2).
__global__ __launch_bounds__(kBlock) void k_c2d_reset(const cobel_c2d_t K, const int G,
                                                      const uint8_t* __restrict__ mask,
                                                      int32_t* __restrict__ fallbacks) {
  extern __shared__ double sh[];
  const int E = K.n_edges, Es = K.n_spawn_edges;
  stage_edges(sh, K.edges, E);
  const int j = (int)threadIdx.x & (G - 1);
  const long long inst = (long long)blockIdx.x * (kBlock / G) + (int)threadIdx.x / G;
  const bool valid = inst < (long long)K.n;
  const size_t i = valid ? (size_t)inst : 0;
  const bool mine = valid && (!mask || mask[i] != 0);
  const uint32_t g = K.instance_base + (uint32_t)i;
  const uint32_t c = K.env_ctr[i];
  const double m = fabs(K.buffer), half = m / 2.0, thr = half * half;
  const double lox = K.box[0], loy = K.box[1], wx = K.box[2] - K.box[0], wy = K.box[3] - K.box[1];
  bool searching = mine;
  double x = K.fallback[0], y = K.fallback[1];
  uint32_t at = 2048u, adv = 2052u;
  for (uint32_t k = 0; k < 1024u && __ballot(searching) != 0ull; ++k) {
    const double ux = cobel_draw_u01(c + 2u * k, 0u, g, COBEL_STREAM_ENV, K.seed);
    const double uy = cobel_draw_u01(c + 2u * k + 1u, 0u, g, COBEL_STREAM_ENV, K.seed);
    const double qx = lox + wx * ux, qy = loy + wy * uy;
    const int in_spawn = group_xor(parity_part(K.spawn_edges, Es, j, G, qx, qy), G);
    const bool ok = group_clear(sh, E, j, G, qx, qy, thr) && in_spawn == 1;
    if (searching && ok) {
      x = qx;
      y = qy;
      at = 2u * k + 2u;
      adv = 2u * k + 4u;
      searching = false;
    }
  }
  if (!mine || j != 0) return;
  const double u = cobel_draw_u01(c + at, 0u, g, COBEL_STREAM_ENV, K.seed);
  K.state[3 * i] = x;
  K.state[3 * i + 1] = y;
  K.state[3 * i + 2] = K.robot_type == COBEL_C2D_STEP ? 0.0 : (2.0 * 3.141592653589793) * u;
  K.env_ctr[i] = c + adv;
  if (searching) atomicAdd(fallbacks, 1);
}

bool lanes_ok(int g) { return g == 1 || g == 4 || g == 16 || g == 64; }

// The planner's choice: the largest G within a lane budget that does not exceed the next power of
// two >= E.  The budget started as the 65 536 lanes the device holds at once (256 CUs x 4 SIMDs x
// 64) and was moved on the measurement of docs/MEASUREMENTS.md §19 (75 edges): one lane per
// instance is bound by the latency of its serial walk (33 us a launch from 64 to 65 536 instances)
// and lost to four lanes at every measured count, so G = 4 and 16 take four times that budget;
// G = 64 keeps it (4 096 instances ran faster on 16 lanes than on 64).  Beyond 65 536 instances
// nothing is measured and the first rule's G = 1 stands.
int plan_lanes(int n, int n_edges) {
  int cap = 1;
  while (cap < n_edges) cap <<= 1;
  int G = 1;
  for (int g : {4, 16, 64})
    if (g <= cap && (long long)n * g <= (g == 64 ? 65536 : 262144)) G = g;
  return G;
}

int check_c2d(const cobel_c2d_t* c, const char* who) {
  COBEL_REQUIRE(c, COBEL_E_ARG, "%s: NULL arena", who);
  COBEL_REQUIRE(c->edges && c->spawn_edges && c->state && c->env_ctr, COBEL_E_ARG,
                "%s: edges, spawn_edges, state and env_ctr are required", who);
  COBEL_REQUIRE(c->n >= 0, COBEL_E_RANGE, "%s: n = %d", who, c->n);
  COBEL_REQUIRE(c->n_edges >= 1 && c->n_edges <= COBEL_C2D_MAX_EDGES && c->n_spawn_edges >= 1 &&
                    c->n_spawn_edges <= COBEL_C2D_MAX_EDGES,
                COBEL_E_RANGE, "%s: %d edges, %d spawn edges (an arena serves 1 to %d of each)",
                who, c->n_edges, c->n_spawn_edges, COBEL_C2D_MAX_EDGES);
  COBEL_REQUIRE(c->n_rewards >= 0 && c->n_rewards <= COBEL_C2D_MAX_REWARDS, COBEL_E_RANGE,
                "%s: %d reward rows (an arena serves 0 to %d)", who, c->n_rewards,
                COBEL_C2D_MAX_REWARDS);
  COBEL_REQUIRE(c->n_rewards == 0 || c->rewards, COBEL_E_ARG, "%s: NULL reward rows", who);
  COBEL_REQUIRE(c->robot_type == COBEL_C2D_STEP || c->robot_type == COBEL_C2D_WHEEL, COBEL_E_ARG,
                "%s: robot type %d", who, c->robot_type);
  COBEL_REQUIRE(c->lanes_per_instance == 0 || lanes_ok(c->lanes_per_instance), COBEL_E_ARG,
                "%s: %d lanes per instance (0: the planner's choice, or 1, 4, 16, 64)", who,
                c->lanes_per_instance);
  COBEL_REQUIRE((((uintptr_t)c->edges | (uintptr_t)c->spawn_edges | (uintptr_t)c->rewards |
                  (uintptr_t)c->state) & 7u) == 0 && ((uintptr_t)c->env_ctr & 3u) == 0,
                COBEL_E_ARG, "%s: misaligned table", who);
  return COBEL_OK;
}

struct c2d_launch {
  int G;
  unsigned grid;
  size_t lds;
};

c2d_launch launch_shape(const cobel_c2d_t* c) {
  c2d_launch L;
  L.G = c->lanes_per_instance ? c->lanes_per_instance : plan_lanes(c->n, c->n_edges);
  const long long per_block = kBlock / L.G;
  L.grid = (unsigned)((c->n + per_block - 1) / per_block);
  L.lds = (size_t)kCols * (size_t)c->n_edges * sizeof(double);
  return L;
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
