// cobel_dqn_act (dqn_act.hip) on the continuous 2D arena: everything of one lockstep DQN training
// step that is not the network —
// epsilon-greedy on the Q-values the replay kernel left behind -> Continuous2D.step -> append to the
// replay ring -> trial bookkeeping, monitors -> auto-reset by rejection sampling -> the observation
// -> draw the replay batch.  With cobel_dqn_replay a training step on the arena is two launches
// (three with the batch draw's own), where the PyTorch loop issues about 180.
//
// Reference behaviour restated (paths relative to the reference's src/cobel):
//   agent/dqn.py:170-212          train loop: retrieve_q -> select_action -> step -> store -> replay
//   policy/greedy.py:40-88        epsilon-greedy (cobel_policy.h)
//   interface/continuous.py:185-266, :268-293   step and reset (cobel_c2d.h: the bodies of
//                                 cobel_c2d_step / cobel_c2d_reset, so the same bits)
//   memory/dqn.py:103-119, :137   FIFO store, uniform sampling with replacement
//   monitor/behavior.py:82        latency = index of the last executed step
// Per instance and step the draws are: one double on the policy stream; at a restart 2k + 3 doubles
// on the env stream (k refused candidates; the counter advances by 2k + 4, cobel_c2d_reset's
// rule); `batch` bounded integers (sub = 0 .. batch-1 of ONE counter) on the memory stream — the
// same streams, counters and order as the stand-alone entry points the PyTorch loop uses.
//
// Mapping: k_c2d_step's — 256 lanes, the edge table in LDS, G lanes per instance.  Lane 0 of a group
// does the scalar work (selection, ring store, bookkeeping) and hands the action and the "restart"
// flag to its group by __shfl; the group operations (move, the candidate loop) are walked by every
// lane of the wave, whether its instance exists, is active or restarts.
#include "cobel_c2d.h"
#include "cobel_dqn_batch.h"
#include "cobel_policy.h"

using namespace cobel_c2d;

namespace {

struct c2d_act_args {
  cobel_dqn_c2d_act_t r;
  cobel_eps_consts eps;
};

// T: the network's dtype (q, the ring); WHEEL: three actions and observations (x, y, orientation)
template <typename T, bool WHEEL>
__global__ __launch_bounds__(kBlock) void k_dqn_act_c2d(const c2d_act_args A, const int G) {
  extern __shared__ double sh[];
  const cobel_dqn_c2d_act_t& R = A.r;
  const cobel_c2d_t& K = R.arena;
  const int E = K.n_edges;
  stage_edges(sh, K.edges, E);
  const int lane = (int)threadIdx.x & 63;
  const int j = (int)threadIdx.x & (G - 1), lead = lane & ~(G - 1);
  const long long inst = (long long)blockIdx.x * (kBlock / G) + (int)threadIdx.x / G;
  const bool valid = inst < (long long)K.n;
  const size_t i = valid ? (size_t)inst : 0;
  const bool live = valid && R.active[i] != 0;   // (not live: walks along, writes nothing of its own)
  const bool scalar = live && j == 0;
  const uint32_t g = K.instance_base + (uint32_t)i;
  constexpr int NA = WHEEL ? 3 : 4, D = WHEEL ? 3 : 2;

  // ---- select (policy/greedy.py:40-88), by lane 0; the group takes its action --------------------
  int a = 0;
  if (scalar) {
    const T* const q = (const T*)R.q + i * NA;
    const uint32_t pc = R.policy_ctr[i];
    const double u = cobel_draw_u01(pc, 0u, g, R.policy_stream, K.seed);
    R.policy_ctr[i] = pc + 1u;
    if (WHEEL) {   // (the split DQN._select makes: four actions by the record path, else over n)
      T qv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) qv[k] = k < NA ? q[k] : (T)0;
      a = cobel_eps_greedy_select_n<T, 8>(qv, NA, 0xffu, u, R.epsilon, nullptr);
    } else {
      a = cobel_eps_greedy_select<T>(q[0], q[1], q[2], q[3], 15u, u, A.eps);
    }
  }
  a = __shfl(a, lead);

  // ---- Continuous2D.step (k_c2d_step's body) -----------------------------------------------------
  const double px = K.state[3 * i], py = K.state[3 * i + 1], th = K.state[3 * i + 2];
  const uint32_t ec = K.env_ctr[i];
  const double m = fabs(K.buffer), half = m / 2.0, thr = half * half;
  double tx, ty, th2;
  action_target(K, px, py, th, a, tx, ty, th2);   // (a < NA: the robot has the action)
  double cx, cy;
  group_move(sh, E, j, G, px, py, tx, ty, m, thr, cx, cy);

  int restart = 0;
  bool active = true;
  if (scalar) {
    const bool hit = cx != tx || cy != ty;
    double reward;
    int end;
    step_outcome(K, cx, cy, hit, reward, end);
    const bool done = end != 0;
    if (R.reward_out) R.reward_out[i] = reward;
    if (R.done_out) R.done_out[i] = (uint8_t)end;
    if (R.wall_out) R.wall_out[i] = hit ? 1 : 0;

    // ---- store (memory/dqn.py:103-119): FIFO ring, the oldest entry goes once it is full ----------
    const int slots = R.slots;
    int size = R.ring_size[i];
    long long head = R.ring_head[i];
    const bool full = size >= slots;
    const int slot = (int)((head + (long long)size) % slots);
    const size_t row = i * slots + slot;
    T* const ds = (T*)R.ring_states + row * D;
    T* const dn = (T*)R.ring_next_states + row * D;
    ds[0] = (T)px;
    ds[1] = (T)py;
    dn[0] = (T)cx;
    dn[1] = (T)cy;
    if (WHEEL) {
      ds[2] = (T)th;
      dn[2] = (T)th2;
    }
    R.ring_actions[row] = (int64_t)a;
    ((T*)R.ring_rewards)[row] = (T)reward;
    ((T*)R.ring_nonterminal)[row] = done ? (T)0 : (T)1;
    if (full) head = (head + 1) % slots;
    else size += 1;
    R.ring_size[i] = size;
    R.ring_head[i] = head;

    // ---- trial bookkeeping (agent/dqn.py:186-212) -------------------------------------------------
    int trial = R.trial[i];
    int step = R.step[i];
    double trew = R.trial_reward[i] + reward;
    const bool over = done || (step + 1 >= R.steps_per_trial);
    if (over) {
      if (trial < R.trial_cap) {
        const size_t mi = (size_t)(i % (R.mon_stripes > 1 ? R.mon_stripes : 1)) * R.trial_cap + trial;
        if (R.lat_sum) atomicAdd((unsigned long long*)R.lat_sum + mi, (unsigned long long)step);
        if (R.lat_cnt) atomicAdd((unsigned long long*)R.lat_cnt + mi, 1ull);
        if (R.reward_sum) atomicAdd(R.reward_sum + mi, trew);
      }
      trial += 1;
      trew = 0.0;
      step = 0;
      active = trial < R.trials_target;
      restart = active ? 1 : 0;
    } else {
      step += 1;
    }
    R.trial[i] = trial;
    R.step[i] = step;
    R.trial_reward[i] = trew;
    R.active[i] = active ? 1 : 0;
    R.stepped[i] = 1;
    if (R.adam_steps) R.adam_steps[i] += 1.0;
    if (R.batch_slots) R.memory_ctr[i] += 1u;
  } else if (valid && j == 0) {
    R.stepped[i] = 0;   // finished all its trials: frozen, consumes nothing
  }

  // ---- auto-reset (k_c2d_reset's body) for the instances whose trial is over and that go on --------
  restart = __shfl(restart, lead);
  const start_point p = find_start(K, sh, j, G, g, ec, thr, restart != 0);
  if (!scalar) return;
  double ox = cx, oy = cy, oth = th2;
  if (restart) {
    ox = p.x;
    oy = p.y;
    oth = start_orientation(K, g, ec, p);
    K.env_ctr[i] = ec + p.adv;
    if (p.fell_back) atomicAdd(R.fallbacks, 1);
  }
  K.state[3 * i] = ox;
  K.state[3 * i + 1] = oy;
  K.state[3 * i + 2] = oth;
  R.obs[i * D] = ox;
  R.obs[i * D + 1] = oy;
  if (WHEEL) R.obs[i * D + 2] = oth;
}

// the replay batch of every instance that took part in this step (cobel_dqn_batch.h)
__global__ __launch_bounds__(256) void k_dqn_batch_c2d(const cobel_dqn_c2d_act_t R) {
  cobel_dqn_ring_batch(R, (long long)blockIdx.x * 256 + threadIdx.x, R.arena.n,
                       R.arena.instance_base, R.arena.seed);
}

}  // namespace

extern "C" int cobel_dqn_act_c2d(const cobel_dqn_c2d_act_t* run, void* stream) {
  COBEL_REQUIRE(run, COBEL_E_ARG, "cobel_dqn_act_c2d: NULL run");
  const cobel_dqn_c2d_act_t& r = *run;
  if (int rc = check_c2d(&r.arena, "cobel_dqn_act_c2d")) return rc;
  COBEL_REQUIRE(r.q && r.policy_ctr, COBEL_E_ARG, "cobel_dqn_act_c2d: NULL policy argument");
  COBEL_REQUIRE(r.ring_states && r.ring_next_states && r.ring_actions && r.ring_rewards &&
                    r.ring_nonterminal && r.ring_size && r.ring_head,
                COBEL_E_ARG, "cobel_dqn_act_c2d: NULL replay ring argument");
  COBEL_REQUIRE(r.trial && r.step && r.trial_reward && r.active && r.stepped, COBEL_E_ARG,
                "cobel_dqn_act_c2d: NULL bookkeeping argument");
  COBEL_REQUIRE(r.obs && r.fallbacks, COBEL_E_ARG,
                "cobel_dqn_act_c2d: obs and the fallback counter are required");
  COBEL_REQUIRE(!r.batch_slots || r.memory_ctr, COBEL_E_ARG,
                "cobel_dqn_act_c2d: batch_slots given without memory_ctr");
  COBEL_REQUIRE(r.slots > 0 && r.batch >= 0 && r.steps_per_trial > 0 && r.trial_cap >= 0,
                COBEL_E_RANGE, "cobel_dqn_act_c2d: bad sizes");
  COBEL_REQUIRE(r.epsilon >= 0.0 && r.epsilon <= 1.0, COBEL_E_ARG,
                "cobel_dqn_act_c2d: epsilon %g outside [0, 1]", r.epsilon);
  COBEL_REQUIRE((((uintptr_t)r.obs | (uintptr_t)r.reward_out | (uintptr_t)r.trial_reward |
                  (uintptr_t)r.ring_head | (uintptr_t)r.ring_actions) & 7u) == 0 &&
                    (((uintptr_t)r.fallbacks | (uintptr_t)r.policy_ctr | (uintptr_t)r.memory_ctr) & 3u) == 0,
                COBEL_E_ARG, "cobel_dqn_act_c2d: misaligned argument");
  if (r.arena.n == 0) return COBEL_OK;
  c2d_act_args A;
  A.r = r;
  A.eps = cobel_make_eps_consts(r.epsilon);
  const c2d_launch L = launch_shape(&r.arena);
  const bool wheel = r.arena.robot_type == COBEL_C2D_WHEEL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(L.grid), block(kBlock);
  if (r.is_float64 && wheel) hipLaunchKernelGGL((k_dqn_act_c2d<double, true>), grid, block, L.lds, st, A, L.G);
  else if (r.is_float64) hipLaunchKernelGGL((k_dqn_act_c2d<double, false>), grid, block, L.lds, st, A, L.G);
  else if (wheel) hipLaunchKernelGGL((k_dqn_act_c2d<float, true>), grid, block, L.lds, st, A, L.G);
  else hipLaunchKernelGGL((k_dqn_act_c2d<float, false>), grid, block, L.lds, st, A, L.G);
  COBEL_HIP_TRY(hipGetLastError());
  if (r.batch > 0 && r.batch_slots) {
    const dim3 bgrid((unsigned)(((long long)r.arena.n * r.batch + 255) / 256));
    hipLaunchKernelGGL(k_dqn_batch_c2d, bgrid, dim3(256), 0, st, r);
    COBEL_HIP_TRY(hipGetLastError());
  }
  return COBEL_OK;
}
