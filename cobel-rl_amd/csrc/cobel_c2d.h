// The continuous 2D arena's device functions and launch planning, shared by the stand-alone entry
// points (continuous.hip: cobel_c2d_step, cobel_c2d_reset) and the DQN act step on the arena
// (dqn_act_c2d.hip: cobel_dqn_act_c2d) — one body each for clear / move, the action's target, the
// reward scan and the candidate loop of a reset, so that both produce the same bits.
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
// The group operations are butterflies over the lanes of a wave and the candidate loop runs under
// __ballot: every lane of a wave has to walk through them, whether its instance exists, takes part
// or is still searching — callers discard the result instead of leaving early.
//
// Files that include this are compiled with -ffp-contract=off: every product and sum below is
// rounded once, in the order written, as the float64 NumPy restatement in tests/c2d_common.py
// evaluates them.
#ifndef COBEL_C2D_H
#define COBEL_C2D_H

#include "cobel_common.h"

namespace cobel_c2d {

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

// Where action a would take the robot from (px, py, th) with nothing in the way, and its new
// orientation; false for an action the robot does not have (the target is then the position).
__device__ __forceinline__ bool action_target(const cobel_c2d_t& K, double px, double py, double th,
                                              int a, double& tx, double& ty, double& th2) {
  const double s = K.step_size;
  tx = px;
  ty = py;
  th2 = th;
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
  return act_ok;
}

// What ending at (cx, cy) pays: the first reward row in reach ends the trial (continuous.py:254-259),
// else -10 for a wall hit under punish_wall.
__device__ __forceinline__ void step_outcome(const cobel_c2d_t& K, double cx, double cy, bool hit,
                                             double& reward, int& end) {
  reward = 0.0;
  end = 0;
  int k = 0;
  for (; k < K.n_rewards; ++k) {
    const double rx = K.rewards[3 * k] - cx, ry = K.rewards[3 * k + 1] - cy;
    if (sqrt(rx * rx + ry * ry) <= K.body_radius * 2.0) break;
  }
  if (k < K.n_rewards) {
    reward = K.rewards[3 * k + 2];
    end = 1;
  } else if (hit && K.punish_wall) {
    reward = -10.0;
  }
}

// A start found by rejection sampling (continuous.py:280-291) with a bound: 1 024 candidates, then
// the host's fallback point.  The spawn table is read in place (a reset is rare; the table stays in
// L2).  `at`: the offset of the orientation's draw from the counter c, `adv`: what the counter
// advances by.
struct start_point {
  double x, y;
  uint32_t at, adv;
  bool fell_back;
};
// The candidate loop, to be called by every lane of a wave (`searching`: this lane's instance wants
// a start; the others walk along and get the fallback point, which they discard).  `sh`: the staged
// arena, g: the instance's number on the streams, c: its counter.
__device__ __forceinline__ start_point find_start(const cobel_c2d_t& K, const double* sh, int j,
                                                  int G, uint32_t g, uint32_t c, double thr,
                                                  bool searching) {
  const int E = K.n_edges, Es = K.n_spawn_edges;
  const double lox = K.box[0], loy = K.box[1], wx = K.box[2] - K.box[0], wy = K.box[3] - K.box[1];
  start_point p;
  p.x = K.fallback[0];
  p.y = K.fallback[1];
  p.at = 2048u;
  p.adv = 2052u;
  for (uint32_t k = 0; k < 1024u && __ballot(searching) != 0ull; ++k) {
    const double ux = cobel_draw_u01(c + 2u * k, 0u, g, COBEL_STREAM_ENV, K.seed);
    const double uy = cobel_draw_u01(c + 2u * k + 1u, 0u, g, COBEL_STREAM_ENV, K.seed);
    const double qx = lox + wx * ux, qy = loy + wy * uy;
    const int in_spawn = group_xor(parity_part(K.spawn_edges, Es, j, G, qx, qy), G);
    const bool ok = group_clear(sh, E, j, G, qx, qy, thr) && in_spawn == 1;
    if (searching && ok) {
      p.x = qx;
      p.y = qy;
      p.at = 2u * k + 2u;
      p.adv = 2u * k + 4u;
      searching = false;
    }
  }
  p.fell_back = searching;
  return p;
}
// the orientation a reset ends with: 0 for the step robot (its draw is consumed all the same)
__device__ __forceinline__ double start_orientation(const cobel_c2d_t& K, uint32_t g, uint32_t c,
                                                    const start_point& p) {
  const double u = cobel_draw_u01(c + p.at, 0u, g, COBEL_STREAM_ENV, K.seed);
  return K.robot_type == COBEL_C2D_STEP ? 0.0 : (2.0 * 3.141592653589793) * u;
}

inline bool lanes_ok(int g) { return g == 1 || g == 4 || g == 16 || g == 64; }

// The planner's choice: the largest G within a lane budget that does not exceed the next power of
// two >= E.  The budget started as the 65 536 lanes the device holds at once (256 CUs x 4 SIMDs x
// 64) and was moved on the measurement of docs/MEASUREMENTS.md §19 (75 edges): one lane per
// instance is bound by the latency of its serial walk (33 us a launch from 64 to 65 536 instances)
// and lost to four lanes at every measured count, so G = 4 and 16 take four times that budget;
// G = 64 keeps it (4 096 instances ran faster on 16 lanes than on 64).  Beyond 65 536 instances
// nothing is measured and the first rule's G = 1 stands.
inline int plan_lanes(int n, int n_edges) {
  int cap = 1;
  while (cap < n_edges) cap <<= 1;
  int G = 1;
  for (int g : {4, 16, 64})
    if (g <= cap && (long long)n * g <= (g == 64 ? 65536 : 262144)) G = g;
  return G;
}

inline int check_c2d(const cobel_c2d_t* c, const char* who) {
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

inline c2d_launch launch_shape(const cobel_c2d_t* c) {
  c2d_launch L;
  L.G = c->lanes_per_instance ? c->lanes_per_instance : plan_lanes(c->n, c->n_edges);
  const long long per_block = kBlock / L.G;
  L.grid = (unsigned)((c->n + per_block - 1) / per_block);
  L.lds = (size_t)kCols * (size_t)c->n_edges * sizeof(double);
  return L;
}

}  // namespace cobel_c2d

#endif  // COBEL_C2D_H
