/*
 * cobel_hip.h — C ABI of libcobel_hip.so, the MI355X (gfx950) hot path of the
 * vectorised navigation-RL loop.
 *
 * The reference (sencheng/CoBeL-RL) is pure Python and has no FFI layer; its
 * boundary for this path is the duck-typed Python API.  Each entry point below
 * names the reference interface it replaces (paths relative to
 * /root/reference/src/cobel).  The binding a maintainer would add is a ctypes
 * stub; see INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; every pointer marked [dev] is DEVICE memory owned by the
 *     caller (e.g. a torch tensor's data_ptr()), [host] is host memory;
 *   - every call returns 0 on success or a negative COBEL_E_* code and never
 *     throws; cobel_last_error() returns a thread-local message;
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and calls return without synchronising;
 *   - the library keeps no global mutable state besides the last-error string; a
 *     world handle changes only through cobel_world_set_transitions (once, before its first
 *     use) and cobel_world_update / cobel_world_update_transitions (in stream order, see
 *     there) and may be shared by any number of runs on its device.
 */
#ifndef COBEL_HIP_H
#define COBEL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COBEL_API __attribute__((visibility("default")))

#define COBEL_OK 0
#define COBEL_E_ARG (-1)         /* NULL / malformed argument            (reference: AssertionError) */
#define COBEL_E_RANGE (-2)       /* index or size out of range            (reference: IndexError)     */
#define COBEL_E_HIP (-3)         /* HIP runtime failure (message has hipGetErrorString)               */
#define COBEL_E_UNSUPPORTED (-4) /* valid request this build cannot serve (e.g. table exceeds LDS)   */

#define COBEL_ACTIONS 4 /* gridworld / 4-neighbour topology action count (gridworld.py:86) */
#define COBEL_MAX_ACTIONS 32 /* largest action count of cobel_world_create_n (hexagonal topology: 6).
                               Action masks (bit a = action a allowed, policy/greedy.py:79-81) are
                               one byte per row in worlds of up to eight actions and one 32-bit
                               word per row (4-byte aligned) in worlds of nine to 32 */
/* 64-bit words per entry of a QAgent's replay log (cobel_tab_run_t.replay_log) in a world of A
 * actions and S states: ONE packed word while states and action fit beside the reward, TWO where
 * they do not — the reference's memory (agent/q.py:213) is a list of tuples of any size. */
#define COBEL_LOG_WORDS(A, S) ((((A) > 8 && (S) > 8192) || (S) > 16384) ? 2 : 1)

/* Random streams: Philox-4x32-10, key = (seed lo, seed hi), ctr = (block, sub, instance, stream).
 * Each stream is consumed through a per-instance draw counter c:
 *   bounded integer c = mulhi32(word (c & 3) of block (c >> 2), n)
 *   uniform double  c = 53-bit double from words 2(c & 1), 2(c & 1) + 1 of block (c >> 1)      */
#define COBEL_STREAM_ENV 0u    /* c = resets so far                (gridworld.py:142)     */
#define COBEL_STREAM_POLICY 1u /* c = select_action calls          (greedy.py:58)         */
#define COBEL_STREAM_MEMORY 2u /* c = replay batches, sub = j      (memory/dyna_q.py:137) */
#define COBEL_STREAM_POLICY_TEST 3u
#define COBEL_STREAM_AGENT 4u  /* c = draws of the agent's own generator (agent/sfma.py:312) */
/* A generator that mixes integer and double draws (SFMAMemory.rng) takes its doubles from
 * sub = 1 + j (j = position in a vector draw): integer and double draws never share a block. */
#define COBEL_SUB_DOUBLE 1u

COBEL_API const char* cobel_last_error(void);
/* ABI version of this header: major * 1000 + minor. */
COBEL_API int cobel_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Raw stream access (used by the host facade for single calls of Policy.select_action /
 * Interface.reset, and by the parity tests of the generator itself).
 *   uniform: out[i]    = double draw number index[i] (sub 0) of instance instance_base + i
 *   bounded: out[i][j] = integer draw number index[i], sub j, j < per_instance
 * If advance != 0, index[i] += 1 afterwards.
 * ------------------------------------------------------------------------------------------ */
COBEL_API int cobel_rng_uniform(uint32_t* index /* [dev] [N] */, uint64_t seed, uint32_t stream,
                                uint32_t instance_base, double* out /* [dev] [N] */, int32_t n,
                                int32_t advance, void* stream_handle);
COBEL_API int cobel_rng_bounded(uint32_t* index /* [dev] [N] */, uint64_t seed, uint32_t stream,
                                uint32_t instance_base, uint32_t bound,
                                int32_t* out /* [dev] [N][per_instance] */, int32_t n,
                                int32_t per_instance, int32_t advance, void* stream_handle);
/* Same with one bound per instance (replay memories of different fill); a bound of 0 yields 0
 * and leaves that instance's counter untouched. */
COBEL_API int cobel_rng_bounded_each(uint32_t* index /* [dev] [N] */, uint64_t seed,
                                     uint32_t stream, uint32_t instance_base,
                                     const uint32_t* bounds /* [dev] [N] */,
                                     int32_t* out /* [dev] [N][per_instance] */, int32_t n,
                                     int32_t per_instance, int32_t advance, void* stream_handle);

/* ------------------------------------------------------------------------------------------
 * World tables.  Replaces WorldDict (interface/gridworld.py:17-30) as produced by
 * make_gridworld (misc/gridworld_tools.py:10-136) and Topology's node dict
 * (interface/topology.py:21-26): the dense one-hot sas[S,4,S] becomes next[S,4].
 * n_worlds distinct worlds of the same state count can live in one handle; instance g uses
 * world (g % n_worlds).
 * ------------------------------------------------------------------------------------------ */
typedef struct cobel_world cobel_world_t;

COBEL_API int cobel_world_create(const uint16_t* next /* [host] [n_worlds][S][4] */,
                       const float* reward /* [host] [n_worlds][S] reward on ENTERING the state */,
                       const uint8_t* terminal /* [host] [n_worlds][S] */,
                       const uint16_t* starts /* [host] concatenated start lists */,
                       const int32_t* start_offsets /* [host] [n_worlds + 1] into starts */,
                       int32_t n_states, int32_t n_worlds, int32_t device, cobel_world_t** out);
/* Worlds whose action count is not four: a Topology's action space is the neighbour count of its
 * start node (interface/topology.py:110-112), six on the hexagonal graphs of
 * misc/topology_tools.py:175-272.  next is [n_worlds][S][n_actions]; n_actions = 4 is
 * cobel_world_create.  Such a world is served by cobel_env_step / cobel_env_reset, and by
 * cobel_tab_run (Q rows of n_actions entries: QAgent on the wavefront kernel of
 * csrc/tabular_nact.hip while the tables fit, else the general kernel); the entry points built
 * around four actions (cobel_sr_run, cobel_sfma_run; cobel_dqn_act beyond eight) refuse it with
 * COBEL_E_UNSUPPORTED. */
COBEL_API int cobel_world_create_n(const uint16_t* next /* [host] [n_worlds][S][n_actions] */,
                       const float* reward /* [host] [n_worlds][S] */,
                       const uint8_t* terminal /* [host] [n_worlds][S] */,
                       const uint16_t* starts, const int32_t* start_offsets, int32_t n_states,
                       int32_t n_worlds, int32_t n_actions /* 1..COBEL_MAX_ACTIONS */,
                       int32_t device, cobel_world_t** out);
COBEL_API int cobel_world_actions(const cobel_world_t* world, int32_t* n_actions);
COBEL_API int cobel_world_destroy(cobel_world_t* world);
COBEL_API int cobel_world_info(const cobel_world_t* world, int32_t* n_states, int32_t* n_worlds,
                     int32_t* device);
/* Transition rows that are DISTRIBUTIONS.  The reference's Gridworld.step reads
 * p = world['sas'][s][a] and, when world['deterministic'] is off, draws the successor with
 * rng.choice(arange(S), p=p) (interface/gridworld.py:115-123).  Every builder writes one-hot rows;
 * a world whose dense sas was edited (slippery floors, ...) is handed over here in list form: for
 * pair p = (world * S + s) * n_actions + a the possible successors succ_state[succ_off[p] ..
 * succ_off[p + 1]) in ascending state order and the normalised cumulative sum of their
 * probabilities (cumsum(p) / cumsum(p)[-1], as Generator.choice forms it; the last entry of a row
 * is 1).  Afterwards cobel_env_step_draw steps the world and cobel_tab_run, cobel_sr_run and
 * cobel_sfma_run draw the successor inside their kernels (cobel_tab_run: the generic wavefront
 * kernel for runs with replayed updates, the general kernel otherwise; cobel_sr_run: the wavefront
 * kernel for plain runs, the row-streaming one with occupancy counters; per-instance parameter
 * sets together with drawn successors are refused there): every step draws one double of
 * COBEL_STREAM_ENV (sub-stream 1) at the instance's env counter, which trial starts share (they
 * draw integers, sub-stream 0).  cobel_env_step and cobel_dqn_act refuse such a world
 * (COBEL_E_UNSUPPORTED); the table given to cobel_world_create (most likely successors) stays in
 * place for them to see. */
COBEL_API int cobel_world_set_transitions(cobel_world_t* world,
                       const uint32_t* succ_off /* [host] [n_worlds * S * n_actions + 1] */,
                       const uint16_t* succ_state /* [host] [nnz] */,
                       const double* succ_cdf /* [host] [nnz] */, int64_t nnz);

/* Live worlds.  The reference reads world['sas'] / ['rewards'] / ['terminals'] /
 * ['starting_states'] anew on every step and reset (interface/gridworld.py:115-126, :142;
 * interface/topology.py:126-172 reads the node dictionary), so a caller may move a reward, a
 * start box or a wall between two runs.  cobel_world_update rewrites the tables of a handle IN
 * STREAM ORDER: arrays as cobel_world_create_n takes them, for the handle's own n_states /
 * n_worlds / n_actions (those never change).  Everything cobel_world_create* checks is checked
 * first; a refused update (COBEL_E_ARG, COBEL_E_RANGE) leaves the handle exactly as it was.  Every
 * derived field follows: the packed records (or next / reward / terminal tables), the start lists
 * (which may change length), the rewarded states and their pairwise order, and their largest
 * count, by which cobel_sr_run picks its kernel form.
 *   - launches enqueued on `stream` BEFORE the call see the old world, launches enqueued AFTER it
 *     the new one; the call enqueues one small kernel and returns, it never waits for the device;
 *   - the caller's arrays are free again on return (they are staged in pinned memory of the
 *     handle's own); buffers an update outgrows are kept until cobel_world_destroy.  A staging
 *     area is reused once the kernel that reads it has finished (asked, never waited for); an
 *     update made while every area is still in flight allocates another one (the size of the
 *     tables, about 1 MB for 64 worlds of 1 024 states), all held until cobel_world_destroy: a
 *     caller that issues many updates without letting the stream progress pays that memory.  The
 *     first update of a handle also pays the allocation of its staging area and one event;
 *   - the host-side fields (start-list length, rewarded-state count, whether rows are
 *     distributions) take effect at call time: while an update is made the handle must not be in
 *     use on ANOTHER stream, and launches on other streams must be ordered behind `stream` by the
 *     caller to see the new world.
 * cobel_world_update_transitions replaces the distribution rows the same way, with the checks of
 * cobel_world_set_transitions; succ_off == NULL returns to plain table rows (the table of
 * cobel_world_create / cobel_world_update: update it as well when the most likely successors
 * changed).  cobel_world_set_transitions keeps its meaning, refusal of a second call included. */
COBEL_API int cobel_world_update(cobel_world_t* world,
                       const uint16_t* next /* [host] [n_worlds][S][n_actions] */,
                       const float* reward /* [host] [n_worlds][S] */,
                       const uint8_t* terminal /* [host] [n_worlds][S] */,
                       const uint16_t* starts /* [host] concatenated start lists */,
                       const int32_t* start_offsets /* [host] [n_worlds + 1] */, void* stream);
COBEL_API int cobel_world_update_transitions(cobel_world_t* world,
                       const uint32_t* succ_off /* [host] [n_worlds * S * n_actions + 1], or NULL */,
                       const uint16_t* succ_state /* [host] [nnz] */,
                       const double* succ_cdf /* [host] [nnz] */, int64_t nnz, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stand-alone vectorised environment.  Replaces Gridworld.step / Gridworld.reset
 * (interface/gridworld.py:92-129, :131-145) and Topology.step / reset
 * (interface/topology.py:126-172) for N instances at once.
 *   step : ns = next[s][a]; reward_out = reward[ns]; done_out = terminal[ns]; state <- ns
 *   reset: where reset_mask[i] != 0 (or reset_mask == NULL):
 *          state[i] = starts[bounded draw number env_ctr[i] of COBEL_STREAM_ENV, n = n_starts];
 *          env_ctr[i] += 1
 * ------------------------------------------------------------------------------------------ */
COBEL_API int cobel_env_step(const cobel_world_t* world, int32_t* state /* [dev] [N] in/out */,
                   const uint8_t* action /* [dev] [N] */, float* reward_out /* [dev] [N] */,
                   uint8_t* done_out /* [dev] [N] */, int32_t n, uint32_t instance_base,
                   void* stream);
/* step of a world with distribution rows (cobel_world_set_transitions): u = double draw number
 * env_ctr[i] of COBEL_STREAM_ENV, sub-stream 1; ns = first successor of (s, a) whose cumulative
 * probability exceeds u; env_ctr[i] += 1.  Worlds without such rows step as cobel_env_step does
 * and leave the counters alone. */
COBEL_API int cobel_env_step_draw(const cobel_world_t* world, int32_t* state /* [dev] [N] in/out */,
                   const uint8_t* action /* [dev] [N] */, float* reward_out /* [dev] [N] */,
                   uint8_t* done_out /* [dev] [N] */, uint32_t* env_ctr /* [dev] [N] in/out */,
                   uint64_t seed, int32_t n, uint32_t instance_base, void* stream);
COBEL_API int cobel_env_reset(const cobel_world_t* world, int32_t* state /* [dev] [N] */,
                    const uint8_t* reset_mask /* [dev] [N] or NULL */,
                    uint32_t* env_ctr /* [dev] [N] in/out */, uint64_t seed, int32_t n,
                    uint32_t instance_base, void* stream);

/* Observation lookup: out[i][0..width) = table[index[i]][0..width) (float64 rows).  Replaces
 * Topology.get_observation for pose observations (interface/topology.py:174-193) and the
 * coordinate lookup of Gridworld.get_position (interface/gridworld.py:147-156). */
COBEL_API int cobel_gather_rows(const double* table /* [dev] [rows][width] */,
                                const int32_t* index /* [dev] [N] */,
                                double* out /* [dev] [N][width] */, int32_t n, int32_t width,
                                int32_t rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Epsilon-greedy.  Replaces EpsilonGreedy.get_action_probs / select_action
 * (policy/greedy.py:40-88) incl. the Generator.choice draw
 * searchsorted(cumsum(p) / cumsum(p)[-1], u, 'right').
 *
 * Probabilities are float64 as in the reference (probs = np.zeros(v.shape)); ties are
 * detected with exact equality on the float32 values.
 * cobel_eps_greedy selects actions for N rows of 4 values with injected uniforms (KAT entry
 * point; the fused run kernels draw u from COBEL_STREAM_POLICY instead) and optionally
 * returns get_action_probs().
 * ------------------------------------------------------------------------------------------ */
COBEL_API int cobel_eps_greedy(const float* values /* [dev] [N][4], 16-byte aligned */,
                               const uint8_t* mask /* [dev] [N] 4-bit masks, or NULL = all */,
                               const double* u /* [dev] [N] in [0,1) */, double epsilon,
                               uint8_t* action_out /* [dev] [N] */,
                               double* probs_out /* [dev] [N][4] or NULL */, int32_t n,
                               void* stream);

/* Same for float64 value rows (network outputs of the DQN path, which the reference keeps in
 * float64): ties are exact equality on the float64 values. */
COBEL_API int cobel_eps_greedy_f64(const double* values /* [dev] [N][4] */,
                                   const uint8_t* mask /* [dev] [N] or NULL */,
                                   const double* u /* [dev] [N] */, double epsilon,
                                   uint8_t* action_out /* [dev] [N] */,
                                   double* probs_out /* [dev] [N][4] or NULL */, int32_t n,
                                   void* stream);

/* The same selection over rows of n_actions values (1..COBEL_MAX_ACTIONS; mask bit a = action a
 * allowed: bytes up to eight actions, 32-bit words beyond): action spaces other than four, e.g. the
 * six neighbours of a hexagonal Topology. */
COBEL_API int cobel_eps_greedy_n(const float* values /* [dev] [N][n_actions] */,
                                 const uint8_t* mask /* [dev] [N] bytes (n_actions <= 8) or
                                                        32-bit words, or NULL */,
                                 const double* u /* [dev] [N] */, double epsilon,
                                 uint8_t* action_out /* [dev] [N] */,
                                 double* probs_out /* [dev] [N][n_actions] or NULL */, int32_t n,
                                 int32_t n_actions, void* stream);
COBEL_API int cobel_eps_greedy_n_f64(const double* values /* [dev] [N][n_actions] */,
                                     const uint8_t* mask, const double* u, double epsilon,
                                     uint8_t* action_out, double* probs_out, int32_t n,
                                     int32_t n_actions, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused tabular agents.  One call advances every instance through
 *   select -> env.step -> [model store] -> TD update -> [B planning / replay TD updates]
 * with per-instance auto-reset at trial ends, entirely on device.
 *
 * Replaces the loops DynaQ.train / DynaQ.test (agent/dyna_q.py:140-273) with update_q
 * (:275-301), replay (:319-330), DynaQMemory.store / retrieve_batch (memory/dyna_q.py:77-96,
 * :122-157); QAgent.train / update_q / replay (agent/q.py:160-228, :289-315, :344-354); and
 * the on_trial_end monitors EscapeLatencyMonitor / RewardMonitor (monitor/behavior.py:73-97,
 * :111-) plus the visit counts behind get_occupancy_map (analysis/behavior_spatial.py:9-73).
 *
 * Numerics ("f32 tables"): tables are float32; the arithmetic follows what the reference
 * itself computes when its tables are cast to float32 under NumPy >= 2 promotion — online TD
 * and QAgent replay in float32, Dyna-Q planning TD in float64 rounded once on store, model
 * reward update in float32 — so results are bit-exact against that run of the reference.
 * ------------------------------------------------------------------------------------------ */

/* Per-instance scalar state: 12 x 32-bit words, caller-owned [dev] [N][12]. */
enum {
  COBEL_I_STATE = 0,      /* int32  current env state                                        */
  COBEL_I_STEP = 1,       /* int32  steps taken in the running trial                         */
  COBEL_I_TRIAL = 2,      /* int32  trials finished (agent.current_trial, agent.py:58)       */
  COBEL_I_CTR_ENV = 3,    /* uint32 next index on COBEL_STREAM_ENV                           */
  COBEL_I_CTR_POLICY = 4, /* uint32 next index on the policy stream                          */
  COBEL_I_CTR_MEMORY = 5, /* uint32 next index on COBEL_STREAM_MEMORY                        */
  COBEL_I_LOG_LEN = 6,    /* uint32 QAgent: experiences logged so far                        */
  COBEL_I_FLAGS = 7,      /* bit 0: a trial is in progress                                   */
  COBEL_I_REWARD_LO = 8,  /* float64 reward collected in the running trial (2 words)         */
  COBEL_I_REWARD_HI = 9,
  COBEL_I_STEPS_LO = 10,  /* uint64 env steps executed over the instance's lifetime (2 words) */
  COBEL_I_STEPS_HI = 11,
  COBEL_I_WORDS = 12
};

enum { COBEL_AGENT_Q = 0, COBEL_AGENT_DYNAQ = 1 };

#define COBEL_F_LEARN 1u          /* 0 = Agent.test(): act only                              */
#define COBEL_F_NO_REPLAY 2u      /* DynaQ.train(no_replay=True)                             */
#define COBEL_F_EPISODIC 4u       /* DynaQ.episodic_replay: one batch per trial              */
#define COBEL_F_MASK_ACTIONS 8u   /* agent.mask_actions                                      */
#define COBEL_F_TEST_STREAM 16u   /* draw u from COBEL_STREAM_POLICY_TEST (separate policy)  */
#define COBEL_F_FORCE_WAVE 32u    /* always use the wave-per-instance kernel (testing); SFMA: always
                                     use the general kernel instead of a specialised one      */
#define COBEL_F_FORCE_LDS_MODEL 64u /* ignore model_index, keep the model digest in LDS (testing) */
#define COBEL_F_NO_PREFETCH 128u   /* SR: load value rows at the top of each step (testing)        */
#define COBEL_F_TAB_GENERAL 512u   /* cobel_tab_run: always take the general kernel (testing)          */
#define COBEL_F_NO_PWG 1024u       /* Dyna-Q: never take the persistent-workgroup kernel (testing,
                                      A/B measurements): k_tab_wpi, one workgroup per instance      */
#define COBEL_F_PWG_GLOBAL 2048u   /* ... its wavefronts ALL work on Q in global memory (testing)          */
#define COBEL_F_SFMA_STREAM 4096u   /* cobel_sfma_run: always take the streaming form (testing)           */
#define COBEL_F_REPLAY_LANE 8192u   /* cobel_dynaq_replay: always take the lane form (testing)           */
#define COBEL_F_SR_STREAM_ROWS 256u /* SR: always take the row-streaming kernel, also where the
                                      sparse-reward kernel applies (testing, A/B measurements)    */

/* Per-instance hyper-parameters.  The reference explores hyper-parameters by running one
 * simulation per combination (optimizer/grid_search.py:173-262: `simulation(task, parameters)`
 * for every entry of `parameter_combinations`, nb_runs times); here the combinations ride on the
 * instance axis of ONE launch: instance i uses param_sets[param_index[i]].  A set carries the
 * agent's learning rate and discount (agent/dyna_q.py:112-113, q.py:121-122, sr.py:115-116), the
 * policy's epsilon (policy/greedy.py:35) and the world model's learning rate
 * (memory/dyna_q.py:66), plus the constants derived from them on the host in float64 — fill it
 * with cobel_param_set_fill, never by hand.  512 bytes. */
typedef struct {
  double alpha, gamma, epsilon, model_lr;
  float alpha_f, gamma_f, model_lr_f, reserved_;
  double eps_base[5];      /* eps / n,        n = 1..4 (index 0 unused)                       */
  double eps_bonus[5];     /* (1 - eps) / t,  t = 1..4                                        */
  uint64_t eps_thr[16][3]; /* per tie pattern: ceil(cdf_k * 2^53) of the unmasked CDF         */
} cobel_param_set_t;
COBEL_API int cobel_param_set_fill(double alpha, double gamma, double epsilon, double model_lr,
                                   cobel_param_set_t* out /* [host] */);

typedef struct {
  /* tables, all caller-owned device memory */
  float* q;              /* [N][S][4] float32 Q.  The replayed updates of a step use the bit
                            patterns 0xffffffc0 .. 0xffffffff inside the table as lane tags while
                            a batch runs (NaNs of a payload no arithmetic produces: the reference's
                            tables never hold them).  A table that holds such a pattern — e.g.
                            uninitialised memory — is garbage in, garbage out (the cell may be
                            taken for a tag); every batch still ends.                           */
  uint64_t* model;       /* DYNAQ: [N][S][4] packed {f32 R; u16 NS; u8 nonterminal; u8 0}    */
  uint16_t* model_index; /* DYNAQ, optional: [N][S][4] 16-bit digest of `model`
                            (next | nonterminal << 14 | (R != +0) << 15, cobel_model_index_build),
                            kept in sync by the kernel.  When present the planning kernel reads
                            it from HBM/L2 instead of holding a copy in LDS: nine instances per
                            CU instead of six.  8-byte aligned, as `model` and `replay_log` are
                            (a state's four entries are read as one 64-bit word): COBEL_E_ARG
                            otherwise.                                                         */
  uint64_t* replay_log;  /* Q: [N][log_cap][COBEL_LOG_WORDS(actions, states)] experiences
                            (q.py:213), or NULL (needed for batch > 0).  Every learning step
                            appends one while there is room, also at batch 0 (the reference's
                            memory grows whether it replays or not).  One word per entry:
                            lo = f32 reward, hi = s | ns << 14 | action << 28 | nonterminal << 30
                            (worlds of five to eight actions: nonterminal << 31; of nine to 32
                            actions, at most 8 192 states: s | ns << 13 | action << 26 |
                            nonterminal << 31).  Two words per entry (more than 16 384 states, or
                            more than eight actions and more than 8 192 states): word 0 lo = f32
                            reward, hi = action | nonterminal << 8; word 1 lo = s, hi = ns      */
  int32_t* inst;         /* [N][COBEL_I_WORDS]                                               */
  const uint8_t* action_mask; /* [S] masks (bit a = action a) shared by all instances, or NULL:
                                 bytes in worlds of up to eight actions, 32-bit words beyond */
  /* monitors (any may be NULL) */
  unsigned long long* lat_sum;  /* [trial_cap] sum over instances of logs['steps']           */
  unsigned long long* lat_cnt;  /* [trial_cap] instances that finished that trial            */
  double* reward_sum;           /* [trial_cap] sum of trial rewards                          */
  unsigned long long* resp_cnt; /* [trial_cap] instances whose trial reward was > 0: the default
                                   response of ResponseMonitor (monitor/behavior.py:286-289)    */
  int32_t* lat_trace;           /* [N][trial_cap] per-instance logs['steps'], or NULL        */
  unsigned long long* occupancy;/* [n_worlds][S] visits of next_state                        */
  unsigned long long* steps_done; /* [1] env steps executed by this call (added)             */
  int32_t* last_exp;     /* [N][6] last experience {s, a, ns, nonterminal, f32 r, f32 td} for
                            per-step host callbacks (use with step_budget = 1), or NULL       */
  /* sizes */
  int32_t n;             /* instances on this device                                         */
  int32_t log_cap;       /* entries per instance in replay_log                               */
  int32_t trial_cap;     /* length of the monitor arrays                                     */
  uint32_t instance_base;/* global id of local instance 0 (sharding; keeps draws G-independent) */
  /* run parameters */
  int32_t agent;         /* COBEL_AGENT_*                                                    */
  uint32_t flags;        /* COBEL_F_*                                                        */
  int32_t trials_target; /* stop an instance when inst[TRIAL] reaches this                   */
  int32_t steps_per_trial;
  int32_t step_budget;   /* max env steps per instance in this call; <= 0 = unlimited        */
  int32_t batch;         /* B: planning / replay updates per step (0..COBEL_MAX_BATCH)       */
  double alpha, gamma, epsilon, model_lr;
  uint64_t seed;
  /* optional per-instance hyper-parameters: with param_index != NULL instance i uses
     param_sets[param_index[i]] (index < n_param_sets) and the four scalars above are ignored */
  const cobel_param_set_t* param_sets; /* [dev] [n_param_sets]                               */
  const uint16_t* param_index;         /* [dev] [N]                                          */
  int32_t n_param_sets;
  int32_t mon_stripes;   /* > 1: lat_sum / lat_cnt / reward_sum / resp_cnt are [mon_stripes][trial_cap]
                            and workgroup b adds into copy b % mon_stripes (spreads the atomics of
                            many instances finishing the same trials over L2 channels); the caller
                            sums the copies.  0 or 1: one copy.                                 */
  unsigned long long* batches_done; /* [1] or NULL: planning / replay batches EVALUATED by this call
                            (added).  A Dyna-Q batch is drawn in every learning step but evaluated
                            only if it can change a table: not while the instance's Q and the
                            reward estimates of its model are all +0.0f (every update of such a
                            batch is 0 + alpha (0 + gamma nt 0 - 0) = 0).  steps_done minus this is
                            the number of batches skipped that way (episodic replay: per trial).  */
  void* scratch;         /* optional [dev] work area of the call, caller-owned (the library allocates
                            nothing in a run): COBEL_TAB_SCRATCH_BYTES(n) bytes, zeroed once by the
                            caller after allocating it, contents otherwise undefined between
                            calls, never shared by two calls in flight.  The
                            persistent-workgroup Dyna-Q kernel keeps its ticket counters and the
                            rings of its ready slices there; with it a launch of few instances
                            per GPU (a shard of a split batch) is handed out in slices of an
                            instance's steps instead of whole instances, so that the last round of
                            work fills the chip.  NULL: whole instances,
                            counters in a buffer of the world handle (one call in flight per
                            handle).                                                           */
  int64_t scratch_bytes;
} cobel_tab_run_t;
#define COBEL_TAB_SCRATCH_BYTES(n) ((256 + 7 * ((int64_t)(n) + 8)) * 4)
/* Word (uint32) of the scratch area a sliced launch raises when one of its wavefronts gave up
 * waiting for a ring entry that never came (a producer wavefront that faulted or was killed: the
 * wait is bounded — seconds — so that the grid drains instead of hanging the GPU).  Valid from the
 * end of a call to the start of the next one on the same area; read by cobel_tab_scratch_check.
 * What slicing relies on, for a maintainer: (1) the hand-off of an instance from the wavefront that
 * ran slice k to the one that runs slice k + 1 goes through ONE XCD's L2 — a queue of tickets is
 * served by the workgroups of a single XCD (HW_REG_XCC_ID, claimed through the `owner` words), the
 * producer waits for its stores (vmcnt(0), a workgroup-scope release) before it publishes the
 * entry, the consumer drops its CU's L1 (agent-scope acquire) before it reads; the per-XCD L2s are
 * not written back per hand-off; (2) every ticket that exists is held by a resident wavefront that
 * finishes (one persistent workgroup per CU, grid <= CU count), so a waiting wavefront waits for
 * work in progress, never for work not yet scheduled. */
#define COBEL_TAB_SCRATCH_ABORT_WORD 255

/* Largest batch the wavefront kernels plan in one pass (one lane per update).  Larger batches —
 * the reference has no limit (agent/dyna_q.py:319-330, memory/dyna_q.py:137) — are planned by
 * Dyna-Q and QAgent in ceil(batch / 62) passes per step (the passes run one after the other, so
 * the sequential order of the reference's loop is kept).  The general kernel — one lane per
 * instance, every update in the reference's sequential order, tables in HBM / L2 — is taken where
 * no wavefront kernel covers a world with an action
 * count other than four (Q is then [N][S][n_actions], replay records carry the action in bits 28-30
 * and the nonterminal flag in bit 31 of the high word; QAgent runs one wavefront per instance on
 * 1 .. 32 actions) and for state counts whose tables
 * exceed the LDS. */
#define COBEL_MAX_BATCH 62

/* 0 = this (S, agent, batch) combination is supported; fills *lds_bytes with the LDS per instance. */
COBEL_API int cobel_tab_query(int32_t n_states, int32_t agent, int32_t batch, int32_t* lds_bytes,
                    int32_t* instances_per_block);
COBEL_API int cobel_tab_run(const cobel_world_t* world, const cobel_tab_run_t* run, void* stream);
/* SURVEY.md section 8b names the two agents' entry points separately; they are cobel_tab_run with
 * run->agent checked: COBEL_E_ARG unless it is COBEL_AGENT_DYNAQ (agent/dyna_q.py:140-330) /
 * COBEL_AGENT_Q (agent/q.py:115-354).  Same arguments, same kernels, same results. */
COBEL_API int cobel_dynaq_run(const cobel_world_t* world, const cobel_tab_run_t* run, void* stream);
COBEL_API int cobel_q_run(const cobel_world_t* world, const cobel_tab_run_t* run, void* stream);
/* Which kernel cobel_tab_run would take for this run, without launching anything (same argument
 * checks): out[0] = COBEL_TAB_KERNEL_*, out[1] = LDS bytes per workgroup, out[2] = workgroups a CU
 * can hold by LDS (1 280-byte blocks, 128 per CU), out[3] = instances per workgroup.  For tests
 * and benchmark reports; all zero for n = 0. */
enum {
  COBEL_TAB_KERNEL_LPI = 0,       /* one lane per instance (runs without planning)              */
  COBEL_TAB_KERNEL_WPI = 1,       /* one wavefront per instance, every run-time switch          */
  COBEL_TAB_KERNEL_WPI_FAST = 2,  /* ... plain Dyna-Q training, model digest in LDS             */
  COBEL_TAB_KERNEL_WPI_INDEX = 3, /* ... plain Dyna-Q training, model digest in HBM (model_index) */
  COBEL_TAB_KERNEL_PWG = 5,       /* plain Dyna-Q training on worlds of 257 .. 1 024 states, one
                                     persistent workgroup per CU: as many wavefronts as Q tables fit
                                     its LDS (ten at 32 x 32); wavefronts that work on Q in global
                                     memory only with COBEL_F_PWG_GLOBAL and forced mixes; out[1] =
                                     LDS of the workgroup, out[2] = 1, out[3] = its wavefronts      */
  COBEL_TAB_KERNEL_WQN = 6,       /* Q-learning on worlds of 1..32 (not four) actions whose tables fit
                                     the LDS: one wavefront per instance, Q rows padded to 8, 16 or
                                     32 values; out[3] = instances per workgroup                   */
  COBEL_TAB_KERNEL_GENERAL = 4    /* one lane per instance, tables in HBM: any action count, batch
                                     size and state count                                        */
};
COBEL_API int cobel_tab_describe(const cobel_world_t* world, const cobel_tab_run_t* run,
                                 int32_t* out /* [host] [4] */);

/* After a cobel_tab_run call that was given a scratch area: waits for `stream`, reads the area's
 * abort word and returns COBEL_OK, or COBEL_E_HIP when a sliced launch gave up (the tables of the
 * call are then incomplete and must be discarded).  The word is STICKY: a launch zeroes its
 * counters and rings but never this word (only the caller does, by zeroing the area it owns), so
 * the check may be made once after any number of launches and reports an abort in ANY of them.  scratch NULL or smaller than
 * COBEL_TAB_SCRATCH_BYTES(1): COBEL_OK (nothing was sliced).  The reference has no counterpart:
 * its loop cannot lose a producer (agent/dyna_q.py:140-215 is one thread). */
COBEL_API int cobel_tab_scratch_check(const void* scratch /* [dev] */, int64_t scratch_bytes,
                                      void* stream);

/* ------------------------------------------------------------------------------------------
 * QAgent and Dyna-Q with the reference's other discrete policies: Softmax (policy/softmax.py),
 * ExclusiveEpsilonGreedy (policy/greedy.py:91-147) and RandomDiscrete (policy/random.py:13-75).
 * A kernel and an entry point of their own (csrc/tabular_policy.hip, one wavefront per instance,
 * tables in LDS); EpsilonGreedy runs take cobel_tab_run as before.  `run` is a cobel_tab_run_t as
 * cobel_tab_run takes it — the same q, model, replay_log, inst, monitor, last_exp and counter
 * formats, the same Philox streams and order of effects as its general kernel, so sessions on
 * either entry point interleave on the same tables — with run.epsilon and the epsilon tables of the
 * parameter sets ignored.  Served: worlds of 1 .. 8 actions and up to 1 024 states whose transition
 * rows are tables; COBEL_AGENT_Q and COBEL_AGENT_DYNAQ (model [N][S][n_actions]); batch 0 ..
 * COBEL_MAX_BATCH; the flags COBEL_F_LEARN, NO_REPLAY, MASK_ACTIONS and TEST_STREAM.
 * batches_done counts every batch drawn from a non-empty source (as the general kernel counts).
 *
 * Selection is float64 whatever the table dtype and consumes exactly ONE draw of the policy stream:
 *   Softmax    e_a = exp((v_a - max) * beta) over the allowed actions, summed in action order,
 *              p_a = e_a / sum
 *   Exclusive  ties by exact equality; p_a = ((1 - eps) * tie_a) / n_ties, then
 *              p_a += (eps * !tie_a) / max(n_allowed - n_ties, 1)
 *              (eps = 1 with every allowed value tied: every probability is 0, as in the
 *              reference, whose Generator.choice then raises; the action here is 0)
 *   both      the action is Generator.choice's: sequential cumulative sum, division by the last
 *              entry, the count of entries <= u (u: the double draw of the counter)
 *   Random     int(rng.integers(n_actions)): the bounded integer draw of the counter, as
 *              cobel_rng_bounded; values and mask are ignored, as the reference ignores them
 * policy_param is beta (Softmax) or epsilon (Exclusive).  With run.param_index instance i uses
 * policy_params[run.param_index[i]] beside alpha, gamma and model_lr of its parameter set; without
 * policy_params the launch-wide policy_param applies to every instance.
 *
 * COBEL_E_ARG, before any launch: a NULL table, an unknown policy, beta <= 0 or epsilon outside
 * [0, 1] (policy_param, or an entry of policy_params), an action mask with a row that allows no
 * action, policy_params without run.param_index.  COBEL_E_UNSUPPORTED, with the limit in the
 * message: more than 8 actions, more than 1 024 states, batch above COBEL_MAX_BATCH,
 * COBEL_F_EPISODIC, worlds whose rows are distributions, a log of two words per entry.  (The mask
 * and policy_params are device memory: checking them copies them to the host and waits for the
 * stream.) */
enum { COBEL_POLICY_SOFTMAX = 1, COBEL_POLICY_EXCLUSIVE = 2, COBEL_POLICY_RANDOM = 3 };
typedef struct {
  cobel_tab_run_t run;
  int32_t policy;              /* COBEL_POLICY_*                                              */
  int32_t reserved_;
  double policy_param;         /* beta / epsilon of every instance (policy_params == NULL)    */
  const double* policy_params; /* [dev] [run.n_param_sets] or NULL                            */
} cobel_tab_policy_run_t;
COBEL_API int cobel_tab_policy_run(const cobel_world_t* world, const cobel_tab_policy_run_t* run,
                                   void* stream);
/* What cobel_tab_policy_run would launch (same checks but the ones that read device memory):
 * out = {LDS bytes per workgroup, its threads, instances per workgroup, workgroups}; zeros for
 * n = 0 and where the run is refused. */
COBEL_API int cobel_tab_policy_plan(const cobel_world_t* world, const cobel_tab_policy_run_t* run,
                                    int32_t* out /* [host] [4] */);
/* The three policies as a single call on n rows v[n][A] (float64; A = 1 .. 8; the host classes
 * round the values to float32 first where the reference's ties are float32 ties), by the device
 * routine of the run kernel, one group of eight lanes per row; stands beside cobel_softmax_n.
 * mask_bits: [n] bytes (bit a = action a allowed) or NULL.  Softmax / Exclusive: u[n] the uniform
 * draws, param[n_param] (n_param = 1 or n) beta / epsilon; k is not read.  Random: k[n] holds the
 * 32-bit word of each bounded draw in its low half, action = (word * A) >> 32; v, mask_bits, u
 * and param are not read.  act[n] and probs[n][A] may each be NULL.  Every pointer is device
 * memory; param and mask_bits are copied back and checked as above before the launch. */
COBEL_API int cobel_policy_select_n(int32_t policy, const double* v, const uint8_t* mask_bits,
                                    const double* u_or_null, const uint64_t* k_or_null,
                                    const double* param, int32_t n_param, uint8_t* act,
                                    double* probs, int32_t n, int32_t A, void* stream);

/* The additions NumPy's pairwise summation (np.sum over a contiguous float32 vector, agent/sr.py:
 * 302-306 `np.sum(SR[j] * rewards)`) performs on a vector of n elements of which only the k <= 32 at
 * `pos` (ascending) are not zero: step t is value[dst[t]] += value[src[t]] on slots 0..k-1, k - 1
 * steps (fewer never: every non-zero element is added once), *root = the slot holding the sum (-1
 * for k = 0).  Pure host function: the SR kernel's sparse-reward form takes its order from it. */
COBEL_API int cobel_pairwise_order(int32_t n, const int32_t* pos, int32_t k, uint8_t* dst /* [31] */,
                                   uint8_t* src /* [31] */, int32_t* root);

/* Host helpers for the packed 8-byte records (so bindings never re-derive the layout). */
COBEL_API uint64_t cobel_pack_model(float reward, uint16_t next_state, uint8_t nonterminal);
COBEL_API void cobel_unpack_model(uint64_t rec, float* reward, uint16_t* next_state, uint8_t* nonterminal);
/* Initialise a model table the way DynaQMemory.__init__ does (memory/dyna_q.py:72-75):
 * R = 0, NS[s][a] = s, nonterminal = 0. */
COBEL_API int cobel_model_init(uint64_t* model /* [dev] [N][S][4] */, int32_t n, int32_t n_states,
                     void* stream);
/* (Re)build the 16-bit digest of a model table — after cobel_model_init or whenever the caller
 * has edited `model` by hand. */
COBEL_API int cobel_model_index_build(const uint64_t* model /* [dev] [N][S][4] */,
                                      uint16_t* index /* [dev] [N][S][4] */, int32_t n,
                                      int32_t n_states, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dyna-Q between sessions.  The reference's DynaQ is a loop over three public calls —
 * M.store(experience), update_q(experience), replay(batch_size) (agent/dyna_q.py:193-211) — which
 * users also call themselves, to plan between trials or between sessions.  These are those calls
 * for N instances on the tables cobel_tab_run keeps (same run struct), in stream order with it.
 * ------------------------------------------------------------------------------------------ */
/* One experience per instance, 24 bytes.  state < 0: the instance has none (left untouched). */
typedef struct {
  int32_t state, action, next_state;
  int32_t nonterminal;    /* experience['terminal'] (the reference stores 1 - end_trial there)  */
  float reward;           /* float32, as the tables are                                         */
  int32_t reserved_;
} cobel_tab_exp_t;

enum { COBEL_REPLAY_WAVE = 0, COBEL_REPLAY_LANE = 1 };
enum { COBEL_UPDATE_ONLINE = 0, COBEL_UPDATE_PLANNING = 1 };

/* DynaQ.replay (agent/dyna_q.py:319-330) with DynaQMemory.retrieve_batch (memory/dyna_q.py:
 * 122-157), n_batches times in one launch: per batch, run->batch pairs in one vector draw of
 * COBEL_STREAM_MEMORY at the instance's counter inst[COBEL_I_CTR_MEMORY] (element j from
 * sub-stream j, what a planning step of cobel_tab_run consumes), their model records, the updates
 * in the reference's order in the planning arithmetic (float64 TD, one rounding into the float32
 * Q), the counter advanced by one.  n_batches calls of one batch and one call of n_batches leave
 * the same bits.  Uses q, model, inst, batch (>= 1, no upper limit), alpha / gamma or the parameter
 * sets, seed, instance_base, n and flags (COBEL_F_REPLAY_LANE) of the run; monitors, scratch and
 * model_index are ignored (planning never writes the model).  Two forms, same results:
 * COBEL_REPLAY_WAVE — one wavefront per instance, Q in LDS — while a Q table fits the LDS,
 * COBEL_REPLAY_LANE — one lane per instance, Q in place — beyond, and under the flag.
 * COBEL_E_RANGE for n_batches < 0 or batch < 1, COBEL_E_ARG for a misaligned or missing table or an
 * agent other than COBEL_AGENT_DYNAQ, COBEL_E_UNSUPPORTED for worlds of other than four actions. */
COBEL_API int cobel_dynaq_replay(const cobel_world_t* world, const cobel_tab_run_t* run,
                                 int32_t n_batches, void* stream);
/* What cobel_dynaq_replay would launch, without launching (same checks): out = {COBEL_REPLAY_*,
 * LDS bytes per workgroup, threads per workgroup, instances per workgroup}. */
COBEL_API int cobel_dynaq_replay_plan(const cobel_world_t* world, const cobel_tab_run_t* run,
                                      int32_t n_batches, int32_t out[4]);
/* DynaQ.update_q (agent/dyna_q.py:275-301): one given experience per instance, td [dev] [N]
 * float64 (0 for an instance without one).  form COBEL_UPDATE_ONLINE: float32, gamma * nt first,
 * one rounding per operation — the step of cobel_tab_run, what the reference computes on float32
 * tables from Python scalars; COBEL_UPDATE_PLANNING: the arithmetic of cobel_dynaq_replay, what it
 * computes from the NumPy scalars its memory hands out.  Uses q, alpha / gamma or the parameter
 * sets and n of the run.  An experience that names a pair outside the tables is skipped. */
COBEL_API int cobel_dynaq_update(const cobel_world_t* world, const cobel_tab_run_t* run,
                                 const cobel_tab_exp_t* exps /* [dev] [N] */, uint32_t form,
                                 double* td /* [dev] [N] */, void* stream);
/* DynaQMemory.store (memory/dyna_q.py:77-96) in every instance: R += lr * (r - R) in float32
 * (d = r - R; R + lr * d, as the step of cobel_tab_run), next state and flag replaced; the digest
 * entry follows when model_index is given (NULL: none is kept). */
COBEL_API int cobel_model_store(uint64_t* model /* [dev] [N][S][4] */,
                                uint16_t* model_index /* [dev] [N][S][4] or NULL */, int32_t n,
                                int32_t n_states, const cobel_tab_exp_t* exps /* [dev] [N] */,
                                double model_lr, void* stream);

/* ------------------------------------------------------------------------------------------
 * A test session that records.  The reference's TrajectoryMonitor (monitor/behavior.py:304-385)
 * appends env.get_position() at every on_step_end; step hooks cannot fire inside a launch, so
 * vectorised test runs report sums only.  cobel_tab_rollout is the test session of cobel_tab_run
 * (COBEL_F_LEARN clear: select with the test policy, step, count — agent/dyna_q.py:217-273,
 * agent/q.py:230-287) for QAgent and Dyna-Q on worlds of 1..32 actions, with every draw, counter,
 * monitor and inst word as cobel_tab_run leaves them, that also keeps what each instance did:
 * for instance i and session trial t (t = trial index - (run.trials_target - trials)),
 *   start  [i][t]      the state after the reset
 *   states [i][t][k]   the state entered by step k
 *   actions[i][t][k]   the action of step k
 *   length [i][t]      steps executed (logs['steps'] + 1)
 * and 0xffff / 0xff (-1 / 255) in states / actions at k >= length: the call fills both arrays
 * with 0xff bytes in stream order before its one kernel launch.  Q is read, never written; model,
 * replay_log, scratch, last_exp, batch and batches_done of the run are ignored.  Every instance
 * is expected at a trial boundary (inst[COBEL_I_FLAGS] bit 0 clear) of trial trials_target -
 * trials; a trial outside the session's range runs and counts but leaves no record.
 * One lane per instance (k_tab_rollout, rollout.hip), Q rows read from device memory.
 * ------------------------------------------------------------------------------------------ */
#define COBEL_ROLLOUT_ELEMENT_STORES 1u /* record_flags: store every record entry on its own (2- and
                                           1-byte stores) instead of four steps at a time as one 8-byte
                                           and one 4-byte store (testing, A/B measurements)          */
typedef struct {
  cobel_tab_run_t run;   /* the session, as cobel_tab_run takes it                              */
  int16_t* start;        /* [N][trials]          2-byte aligned                                 */
  int16_t* states;       /* [N][trials][steps]   8-byte aligned                                 */
  uint8_t* actions;      /* [N][trials][steps]   4-byte aligned                                 */
  int32_t* length;       /* [N][trials]          4-byte aligned                                 */
  int32_t trials;        /* trials of this session (>= 1)                                       */
  int32_t steps;         /* steps per trial (>= 1): run.steps_per_trial must equal it           */
  uint32_t record_flags; /* COBEL_ROLLOUT_*                                                     */
  int32_t reserved_;
} cobel_tab_rollout_t;
/* COBEL_E_ARG: a NULL argument, record array or q; COBEL_F_LEARN set; step_budget != 0; a
 * misaligned q (16 bytes in four-action worlds, else 4), inst or record array; steps_per_trial !=
 * steps.  COBEL_E_RANGE: trials < 1, steps < 1, n < 0, trials_target < trials, trial_cap <
 * trials_target.  COBEL_E_UNSUPPORTED: more than COBEL_MAX_ACTIONS actions.  All before any launch. */
COBEL_API int cobel_tab_rollout(const cobel_world_t* world, const cobel_tab_rollout_t* rollout,
                                void* stream);
/* The same checks without a launch: out = {LDS bytes per workgroup (0), threads per workgroup,
 * instances per workgroup, workgroups}; all zero for n = 0. */
COBEL_API int cobel_tab_rollout_plan(const cobel_world_t* world,
                                     const cobel_tab_rollout_t* rollout, int32_t out[4]);
/* Visit counts of a record: counts[w][s] += entries of `states` equal to s among the instances of
 * world w = (instance_base + i) % n_worlds (what cobel_tab_run adds to `occupancy` over the same
 * session).  Entries outside 0 .. n_states - 1 (the padding) are skipped. */
COBEL_API int cobel_rollout_visits(const int16_t* states /* [dev] [N][per_instance] */, int32_t n,
                                   int64_t per_instance, int32_t n_states, int32_t n_worlds,
                                   uint32_t instance_base,
                                   unsigned long long* counts /* [dev] [n_worlds][n_states] */,
                                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Successor-representation agent.  Replaces SR.train / SR.update / SR.retrieve_q
 * (agent/sr.py:142-197, :255-286, :288-308).  Tables: SR f32 [N][S][S] (= eye at init),
 * agent transition table T u16 [N][S][4] (= s at init, sr.py:131-135), reward estimate
 * f32 [N][S].  The row TD error is evaluated in float64 and rounded once on store, as the
 * reference does with a float32 SR (np.eye is float64, sr.py:276-284).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  float* sr;          /* [N][S][S] */
  uint16_t* trans;    /* [N][S][4], 8-byte aligned (a state's row is read as one 64-bit word;
                         COBEL_E_ARG otherwise; sr: 16-byte, inst: 8-byte aligned)            */
  float* rewards;     /* [N][S]    */
  int32_t* inst;      /* [N][COBEL_I_WORDS] */
  const uint8_t* action_mask;
  unsigned long long* lat_sum;
  unsigned long long* lat_cnt;
  double* reward_sum;
  unsigned long long* resp_cnt;
  int32_t* lat_trace;
  unsigned long long* occupancy;
  unsigned long long* steps_done;
  int32_t* last_exp;  /* [N][6] {s, a, ns, nonterminal, f32 r, 0} or NULL */
  int32_t n, trial_cap;
  uint32_t instance_base;
  uint32_t flags;
  int32_t trials_target, steps_per_trial, step_budget;
  double alpha, gamma, epsilon;
  uint64_t seed;
  const cobel_param_set_t* param_sets; /* as in cobel_tab_run_t (model_lr unused)            */
  const uint16_t* param_index;
  int32_t n_param_sets;
  int32_t mon_stripes;   /* as in cobel_tab_run_t                                             */
  /* optional [dev] [4] counters the sparse-reward kernel adds to: SR rows read, SR rows
     written, 4-byte value gathers, instances that fell back to full row sums (NULL: not counted;
     untouched by the row-streaming kernel) */
  unsigned long long* traffic;
} cobel_sr_run_t;

COBEL_API int cobel_sr_init(float* sr, uint16_t* trans, float* rewards, int32_t n, int32_t n_states,
                  void* stream);
COBEL_API int cobel_sr_run(const cobel_world_t* world, const cobel_sr_run_t* run, void* stream);
/* q[i][a] = V[T[s_i][a]], V[j] = sum_k SR[j][k] * rewards[k] (sr.py:302-306) for given states. */
COBEL_API int cobel_sr_retrieve_q(const float* sr, const uint16_t* trans, const float* rewards,
                        const int32_t* states /* [dev] [N] */, float* q_out /* [dev] [N][4] */,
                        int32_t n, int32_t n_states, void* stream);

/* ------------------------------------------------------------------------------------------
 * SFMA agent: Dyna-Q whose replay is driven by Spatial structure and Frequency-weighted Memory
 * Access.  Replaces SFMA.train / test / replay / update_q (agent/sfma.py:233-458) and
 * SFMAMemory.store / replay / softmax / retrieve_random_batch (memory/sfma.py:195-416) for N
 * instances; the similarity metric (memory/utils/metrics.py) comes in as a matrix.
 *
 * Per trial: online steps (select -> env.step -> store -> TD), then — unless NO_REPLAY —
 * nb_replays replays of `batch` reactivations.  One reactivation ranks all 4S experiences
 * j = a * S + s by R = C * D * (1 - I) [* T] (strength x similarity x (1 - inhibition) [x
 * recency]), thresholds, normalises, and draws one from softmax(R) = exp(beta R) - 1
 * (memory/sfma.py:280-333); the drawn experience is applied with a TD update at once (the batch
 * the reference builds first does not depend on Q, so the order of effects is the same).
 *
 * Numerics: Q and the model's reward estimates are float32 and follow the reference run with
 * float32 tables (online TD float32, replayed TD float64 rounded once on store, |TD| sum float32
 * until the first replayed TD after a reset); strengths, inhibition, recency, similarities and
 * priorities are float64 as in the reference.  The drawn index is
 * #{k : cumsum(w)_k / cumsum(w)_last <= u}: the reference normalises w three times before the same
 * count and sums sequentially, here the sum is a wave scan and exp() is the device's — equal up
 * to a few ulp of the CDF, so a draw differs from the reference's only if u falls within ~1e-14
 * of a CDF edge.
 * ------------------------------------------------------------------------------------------ */
enum {
  COBEL_SFMA_DEFAULT = 0, COBEL_SFMA_REVERSE = 1, COBEL_SFMA_FORWARD = 2,
  COBEL_SFMA_BLEND_FORWARD = 3, COBEL_SFMA_BLEND_REVERSE = 4, COBEL_SFMA_INTERPOLATE = 5,
  COBEL_SFMA_SWEEPING = 6, COBEL_SFMA_MODES = 7
};

#define COBEL_SF_RANDOM 1u            /* agent.random: uniform batches (memory/sfma.py:374-416) */
#define COBEL_SF_DYNAMIC 2u           /* agent.dynamic: reverse/default drawn from the |TD| sum  */
#define COBEL_SF_START_REPLAY 4u      /* agent.start_replay: a replay (without TD) at trial start */
#define COBEL_SF_DETERMINISTIC 8u     /* M.deterministic: argmax instead of the softmax draw      */
#define COBEL_SF_RECENCY 16u          /* M.recency                                                */
#define COBEL_SF_C_NORMALIZE 32u      /* M.C_normalize                                            */
#define COBEL_SF_D_NORMALIZE 64u      /* M.D_normalize                                            */
#define COBEL_SF_R_NORMALIZE 128u     /* M.R_normalize (default on)                               */
#define COBEL_SF_REWARD_MOD_LOCAL 256u/* M.reward_mod_local                                       */
#define COBEL_SF_REWARD_MOD 512u      /* M.reward_mod                                             */
#define COBEL_SF_STATE_MOD 1024u      /* M.state_mod                                              */

/* Per-instance SFMA state: 8 x 32-bit words, caller-owned [dev] [N][8]. */
enum {
  COBEL_SI_CLOCK = 0,     /* uint32 experiences stored so far (the recency clock)              */
  COBEL_SI_EPOCH = 1,     /* uint32 clock at the last T.fill(0) (agent/sfma.py:325)            */
  COBEL_SI_MODE = 2,      /* int32  M.mode (COBEL_SFMA_*); rewritten in dynamic mode           */
  COBEL_SI_FLAGS = 3,     /* bit 0: the |TD| sum currently has float32 type                    */
  COBEL_SI_TD_LO = 4,     /* float64 agent.td, the |TD| sum (2 words)                          */
  COBEL_SI_TD_HI = 5,
  COBEL_SI_CTR_AGENT = 6, /* uint32 next index on COBEL_STREAM_AGENT                           */
  COBEL_SI_RESERVED = 7,
  COBEL_SI_WORDS = 8
};

/* One replayed experience (logs['replay'], agent/sfma.py:273,322), 24 bytes. */
typedef struct {
  uint32_t sa;     /* state | action << 16 | nonterminal << 24 | kind << 25 (1 = trial start)  */
  uint32_t next;   /* next state                                                               */
  float reward;    /* M.rewards[s][a] at replay time                                           */
  int32_t trial;   /* agent.current_trial of the trial the replay belongs to                   */
  double td;       /* TD error of the update (NaN for start-of-trial replays)                  */
} cobel_sfma_event_t;

/* Per-instance SFMA parameters: the agent's set (cobel_param_set_t: learning rate, discount,
 * the policy's epsilon with its derived selection constants, M.learning_rate as model_lr) and the
 * ten parameters of the memory a sweep varies (memory/sfma.py:40-72).  The reference runs one
 * simulation per combination; here instance i of ONE launch uses param_sets[param_index[i]] — in
 * every kernel of cobel_sfma_run except the plain-training one, whose conditions (decay_strength
 * == 1, 0 <= beta <= 700, r_threshold >= 0) are facts of a set the launcher cannot see: a launch
 * with an index takes the two-experiences-per-lane kernel that serves every value instead.  The
 * replay mode is per instance already (sfma_inst[COBEL_SI_MODE]); the switches (COBEL_SF_*),
 * nb_replays, the recency decay and the replay length stay launch-wide.  Fill a set with
 * cobel_sfma_param_set_fill, never by hand.  592 bytes, a multiple of 16 as it stands. */
typedef struct {
  cobel_param_set_t agent;
  double decay_inhibition, decay_strength;       /* M.decay_inhibition, M.decay_strength      */
  double c_step, i_step, r_threshold, beta;      /* M.C_step, M.I_step, M.R_threshold, M.beta */
  double reward_modulation, blend, interp_fwd, interp_rev;
} cobel_sfma_param_set_t;
/* Host only.  The agent part is cobel_param_set_fill(alpha, gamma, epsilon, model_lr) — epsilon
 * outside [0, 1] is refused (COBEL_E_ARG), as cobel_sfma_run refuses it; memory[10] in the order
 * of the members above, taken verbatim. */
COBEL_API int cobel_sfma_param_set_fill(double alpha, double gamma, double epsilon, double model_lr,
                                        const double memory[10],
                                        cobel_sfma_param_set_t* out /* [host] */);

typedef struct {
  /* tables, caller-owned device memory */
  float* q;               /* [N][S][4] float32 Q                                              */
  uint64_t* model;        /* [N][S][4] packed records as in cobel_tab_run_t (cobel_model_init) */
  double* strength;       /* [N][4S]  M.C, index a * S + s                                    */
  uint32_t* stamp;        /* [N][4S]  clock value at which (s, a) was last stored; M.T[j] =
                             recency_tab[clock - stamp[j]] if stamp[j] > epoch else 0         */
  int32_t* inst;          /* [N][COBEL_I_WORDS]                                               */
  int32_t* sfma_inst;     /* [N][COBEL_SI_WORDS]                                              */
  const double* metric;   /* [n_worlds][S][S] similarity matrix metric.D of each world        */
  const double* recency_tab; /* [recency_len] 1, d, fl(d*d), ... by repeated multiplication
                             (M.T *= decay_recency per store); ages beyond the end use the last */
  const double* random_cdf;  /* [4S] RANDOM: cumsum(p) / cumsum(p)[-1] of the masked uniform p */
  const uint8_t* action_mask; /* [S] 4-bit masks or NULL                                       */
  /* monitors (any may be NULL), as in cobel_tab_run_t */
  unsigned long long* lat_sum;
  unsigned long long* lat_cnt;
  double* reward_sum;
  unsigned long long* resp_cnt;
  int32_t* lat_trace;
  unsigned long long* occupancy;
  unsigned long long* steps_done;
  unsigned long long* replays_done; /* [1] experiences reactivated by this call (added)       */
  int32_t* last_exp;      /* [N][6] as in cobel_tab_run_t                                     */
  cobel_sfma_event_t* replay_trace; /* [N][trace_cap] or NULL                                 */
  int32_t* trace_len;     /* [N] in/out: events appended so far (counts past trace_cap too)   */
  /* sizes */
  int32_t n, trial_cap, trace_cap, recency_len;
  uint32_t instance_base;
  /* run parameters */
  uint32_t flags;         /* COBEL_F_LEARN | NO_REPLAY | MASK_ACTIONS | TEST_STREAM           */
  uint32_t sfma_flags;    /* COBEL_SF_*                                                       */
  int32_t trials_target, steps_per_trial, step_budget;
  int32_t batch;          /* replay length                                                    */
  int32_t nb_replays;     /* agent.nb_replays                                                 */
  int32_t mon_stripes;    /* as in cobel_tab_run_t                                            */
  double alpha, gamma, epsilon, model_lr;        /* agent lr, discount, policy eps, M.learning_rate */
  double decay_inhibition, decay_strength;       /* M.decay_inhibition, M.decay_strength      */
  double c_step, i_step, r_threshold, beta;      /* M.C_step, M.I_step, M.R_threshold, M.beta */
  double reward_modulation, blend, interp_fwd, interp_rev;
  uint64_t seed;
  /* optional per-instance parameter sets, as in cobel_tab_run_t: with param_index != NULL
     instance i uses param_sets[param_index[i]] (index < n_param_sets, 1 .. 65 535 sets) and the
     fourteen scalars above are ignored; with param_index == NULL the launch is the scalar launch */
  const cobel_sfma_param_set_t* param_sets; /* [dev] [n_param_sets], 16-byte aligned          */
  const uint16_t* param_index;              /* [dev] [N]                                      */
  int32_t n_param_sets;
} cobel_sfma_run_t;

/* The LDS-resident form: 0 = it serves n_states; fills *lds_bytes with the LDS one instance needs. */
COBEL_API int cobel_sfma_query(int32_t n_states, int32_t* lds_bytes);
/* What cobel_sfma_run launches for a world of n_states under `flags` (COBEL_F_*; the ones that
 * matter are COBEL_F_SFMA_STREAM and COBEL_F_NO_PREFETCH): out = {form (0 LDS-resident, up to
 * 1 274 states; 1 streaming, tables read where the caller keeps them), LDS bytes per workgroup,
 * threads per instance, bytes of caller-owned scratch (0: neither form takes any)}.
 * COBEL_E_RANGE for n_states < 1; COBEL_E_UNSUPPORTED beyond 16 383 states, the largest index the
 * 15-bit successor field of an experience (NS | flag << 15) holds. */
COBEL_API int cobel_sfma_plan(int32_t n_states, uint32_t flags, int32_t out[4]);
COBEL_API int cobel_sfma_run(const cobel_world_t* world, const cobel_sfma_run_t* run, void* stream);
/* For tests: exp(x[i]) by the routine the plain-training SFMA kernel uses for its softmax weights
 * (arguments in [0, 700], memory/sfma.py:349-372) and by the device library's exp, which every
 * other instantiation calls; the two must agree bit for bit on that range.  With `divisor`: x[i] /
 * divisor[i] through the reciprocal the kernels share over a reactivation's experiences, and by
 * the division it replaces (the normalisation R / max R, memory/sfma.py:319-321).  Device pointers. */
COBEL_API int cobel_sfma_exp_check(const double* x, double* in_range, double* library,
                                   const double* divisor, double* quotient_by_reciprocal,
                                   double* quotient, int32_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * SFMAMemory on its own: store / replay / retrieve_random_batch (memory/sfma.py:195-416) as calls
 * on the tables cobel_sfma_run keeps, for N instances, without an agent.  The kernels are the
 * store and the replay of cobel_sfma_run (the same code, in its general form), so a store writes
 * the bits the agent's kernel writes and a replay reactivates what the agent's replay would.
 *
 * Draws.  The memory stream is the one cobel_sfma_run uses: COBEL_STREAM_MEMORY of instance
 * instance_base + i at index counter[i], integers on sub-stream 0, doubles on sub-stream 1 (a
 * NumPy Generator stand-in TapeRNG(seed, g, STREAM_MEMORY, start = counter, double_sub = 1)).
 *   - a single replay (n_replays = 1, no COBEL_SFM_STRIDED) consumes what the reference consumes —
 *     one integer unless the action is given, one double if the state is drawn, one double per
 *     reactivation unless deterministic — and advances counter[i] by that many;
 *   - COBEL_SFM_STRIDED: replay k starts at counter[i] + k * (replay_length + 2), the most one replay
 *     can consume, and the call advances counter[i] by n_replays * (replay_length + 2): replay k is
 *     what a reference memory in the same state produces with its generator positioned there;
 *   - a random batch of any size is one vector draw: doubles at index counter[i], sub-streams
 *     1, 2, ...; counter[i] advances by one.
 * ------------------------------------------------------------------------------------------ */
#define COBEL_SFM_ERROR_MOD_LOCAL 1u  /* M.error_mod_local: C[j] += |td|                             */
#define COBEL_SFM_ERROR_MOD 2u        /* M.error_mod: C += |td| * tile(D[next_state])                */
#define COBEL_SFM_STRIDED 4u          /* cobel_sfma_replay: one stride of the stream per replay      */

/* One experience handed to cobel_sfma_store, 32 bytes. */
typedef struct {
  int32_t state, action, next_state;
  int32_t nonterminal;    /* experience['terminal'] (the reference stores 1 - end_trial there)  */
  double reward;          /* rounded to float32 for the model's estimate, as given for C        */
  double td;              /* read under COBEL_SFM_ERROR_MOD_LOCAL / COBEL_SFM_ERROR_MOD only    */
} cobel_sfma_exp_t;

typedef struct {
  /* tables, caller-owned device memory, as in cobel_sfma_run_t */
  uint64_t* model;        /* [N][S][4]                                                        */
  double* strength;       /* [N][4S]                                                          */
  uint32_t* stamp;        /* [N][4S]                                                          */
  int32_t* sfma_inst;     /* [N][COBEL_SI_WORDS]: clock, epoch and mode are used              */
  const double* metric;   /* [n_worlds][S][S]; instance g uses world g % n_worlds             */
  const double* recency_tab; /* [recency_len], needed under COBEL_SF_RECENCY                  */
  uint32_t* counter;      /* [N] next index on the memory stream, in/out                      */
  int32_t n, n_states, n_worlds, recency_len;
  uint32_t instance_base;
  uint32_t flags;         /* COBEL_F_SFMA_STREAM | COBEL_F_FORCE_WAVE | COBEL_F_NO_PREFETCH, as
                             cobel_sfma_plan reads them                                        */
  uint32_t sfma_flags;    /* COBEL_SF_*: the switches of the memory                            */
  uint32_t mem_flags;     /* COBEL_SFM_*                                                       */
  double model_lr;        /* M.learning_rate                                                   */
  double decay_inhibition, decay_strength;
  double c_step, i_step, r_threshold, beta;
  double reward_modulation, blend, interp_fwd, interp_rev;
  uint64_t seed;
  /* optional per-instance parameter sets, as in cobel_sfma_run_t: instance i — every one of its
     replays in a strided call — uses param_sets[param_index[i]]; of the agent part a store reads
     model_lr, the rest is unused here */
  const cobel_sfma_param_set_t* param_sets; /* [dev] [n_param_sets], 16-byte aligned          */
  const uint16_t* param_index;              /* [dev] [N]                                      */
  int32_t n_param_sets;
} cobel_sfma_mem_t;

/* What the memory's calls launch for n_states under `flags`: out = {form (0 LDS-resident, 1
 * streaming), LDS bytes per workgroup, threads per workgroup, what the streaming form keeps in
 * LDS besides I (bit 0 the successor table, bit 1 the two similarity rows)}.  The form, the LDS
 * and its tiers are cobel_sfma_plan's; a workgroup is one instance (store) or one replay. */
COBEL_API int cobel_sfma_mem_plan(int32_t n_states, uint32_t flags, int32_t out[4]);
/* M.store(experiences[i]) in every instance i: model record, C *= decay_strength, C[j] += C_step,
 * stamp and clock, reward / error / state modulation.  experiences: [dev] [N]. */
COBEL_API int cobel_sfma_store(const cobel_sfma_mem_t* mem, const cobel_sfma_exp_t* experiences,
                               void* stream);
/* n_replays independent replays of replay_length reactivations in every instance, side by side.
 * Reads the memory only (strengths, stamps, model records); writes counter (see above) and
 *   events     [dev] [N][n_replays][replay_length], td = NaN, trial = 0, kind = 0
 *   lengths    [dev] [N][n_replays] reactivations before the ratings ran out
 *   inhibition [dev] [N][S] or NULL: M.I as replay 0 of each instance leaves it
 * start_state / start_action: [dev] [N] or NULL; an entry < 0 (or NULL) means None: the start is
 * drawn from the clipped strengths, the action is drawn. */
COBEL_API int cobel_sfma_replay(const cobel_sfma_mem_t* mem, int32_t n_replays,
                                int32_t replay_length, const int32_t* start_state,
                                const int32_t* start_action, cobel_sfma_event_t* events,
                                int32_t* lengths, double* inhibition, void* stream);
/* M.retrieve_random_batch: n_experiences draws per instance through random_cdf ([dev] [4S],
 * cumsum(p) / cumsum(p)[-1] of the masked uniform p as in cobel_sfma_run_t); events [dev]
 * [N][n_experiences] as above. */
COBEL_API int cobel_sfma_random_batch(const cobel_sfma_mem_t* mem, int32_t n_experiences,
                                      const double* random_cdf, cobel_sfma_event_t* events,
                                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused Adam step for network parameters stacked over instances (the DQN path keeps one network
 * per agent-env instance, parameters [N][...] per tensor).  Replaces optimizer.step() behind
 * TorchNetwork.train_on_batch (network/network_torch.py:160-167) for torch.optim.Adam without
 * amsgrad: one pass over param / grad / exp_avg / exp_avg_sq instead of ~10 elementwise kernels.
 *   steps[i]  : Adam step count of instance i INCLUDING this step (bias corrections 1 - beta^step)
 *   active[i] : 0 = instance i keeps parameters and optimizer state untouched; NULL = all step
 * Elements [i * per_instance, (i + 1) * per_instance) of every tensor belong to instance i.
 * ------------------------------------------------------------------------------------------ */
COBEL_API int cobel_adam_step(void* param /* [dev] [N][per_instance] */,
                              const void* grad /* [dev] */, void* exp_avg /* [dev] */,
                              void* exp_avg_sq /* [dev] */, const double* steps /* [dev] [N] */,
                              const uint8_t* active /* [dev] [N] or NULL */, int64_t n_instances,
                              int64_t per_instance, int32_t is_float64, double lr, double beta1,
                              double beta2, double eps, double weight_decay,
                              void* target /* [dev] same shape, or NULL: target[e] += tau *
                                              (param_new[e] - target[e]) for stepping instances
                                              (the DQN target blend, agent/dqn.py:366-371) */,
                              double tau, void* stream);

/* ------------------------------------------------------------------------------------------
 * One DQN replay step per instance in ONE kernel, for networks of the shape the reference's DQN
 * demos and tests use — Linear(D, 64) - ReLU - Linear(64, 64) - ReLU - Linear(64, A), D <= 32,
 * A = 4 (1 .. 8 on the streaming form: the six neighbours of a hexagonal Topology),
 * batches of 32, float64 or float32, MSE loss, torch.optim.Adam without amsgrad:
 *   targets = Q_online(s); targets[a] = r + gamma * nt * max_a' Q_target(s')   (agent/dqn.py:346-364;
 *             ddqn != 0: a' = argmax Q_online(s'), :352-355; a sample with nt == 0 does not look at
 *             Q_target: its target is r even where the target network holds NaN or infinity — the
 *             package's PyTorch paths, agent/dqn.py and agent/dyna_dqn.py, do the same)
 *   loss = mean((Q_online(s) - targets)^2); backward; Adam step   (network/network_torch.py:160-167)
 *   w_target += tau * (w_online - w_target)                       (agent/dqn.py:366-371; tau 0 = none)
 * Parameters are torch.nn.Linear tensors stacked over instances: w[l] [N][out][in], b[l] [N][out]
 * for the online network, *_target for the target network, m_* / v_* Adam's exp_avg / exp_avg_sq
 * of the online network.  steps / active as for cobel_adam_step.  The batch is given gathered:
 * states / next_states [N][32][D], actions int64 [N][32], rewards and the non-terminal flags
 * (1 - end_trial, agent/dqn.py:191) [N][32] in the network's dtype.  All device memory, caller-owned.
 * `activation` swaps both ReLUs for tanh.
 * ------------------------------------------------------------------------------------------ */
enum { COBEL_ACT_RELU = 0, COBEL_ACT_TANH = 1 };
typedef struct {
  void* w[3];
  void* b[3];
  void* w_target[3];
  void* b_target[3];
  void* m_w[3];
  void* m_b[3];
  void* v_w[3];
  void* v_b[3];
  const double* steps;      /* [N] Adam step count INCLUDING this step                          */
  const uint8_t* active;    /* [N] or NULL                                                      */
  const void* states;       /* [N][batch][n_inputs]                                             */
  const void* next_states;
  const int64_t* actions;   /* [N][batch]                                                       */
  const void* rewards;      /* [N][batch]                                                       */
  const void* nonterminal;  /* [N][batch]                                                       */
  int32_t n, n_inputs, n_hidden1, n_hidden2, n_actions, batch;
  int32_t is_float64, ddqn;
  double gamma, lr, beta1, beta2, eps, weight_decay, tau;
  /* optional: the kernel gathers the batch from the replay rings itself.  With batch_slots != NULL
     states / next_states / actions / rewards / nonterminal are the rings [N][ring_slots][..] and
     sample s of instance i is row batch_slots[i][s] (as written by cobel_dqn_act). */
  const int32_t* batch_slots; /* [N][batch] or NULL                                             */
  int32_t ring_slots;
  /* the activation of both hidden layers: COBEL_ACT_RELU (0, what a zeroed struct asks for) or
     COBEL_ACT_TANH — the network of the reference's Continuous2D demo (demo/continuous/demo_2d.py:
     torch.tanh after both hidden layers).  Forward h = tanh(pre) in the network's dtype, backward
     delta_l = (delta_{l+1} W_{l+1}) * (1 - h_l * h_l) in that order (torch's tanh_backward).  tanh
     runs on the streaming form at every width; any other value is COBEL_E_ARG. */
  int32_t activation;
  /* optional: Q-values of each instance's NEXT observation, computed with the updated online
     network at the end of the step (what the next action selection needs, agent/dqn.py:174):
     observation of instance i = row obs_index[i] of obs_table.  Instances outside `active` are
     left alone. */
  const int32_t* obs_index;   /* [N]                                                            */
  const double* obs_table;    /* [rows][n_inputs] float64                                       */
  void* q_out;                /* [N][n_actions] network dtype, or NULL                          */
  /* optional: the batch's observations as rows of obs_table (DynaDQN: the model is indexed by
     integer states, agent/dyna_q.py:333-708).  With state_index != NULL states / next_states are
     not read; actions / rewards / nonterminal are the gathered [N][batch] arrays. */
  const int32_t* state_index; /* [N][batch] or NULL                                             */
  const int32_t* next_index;  /* [N][batch]                                                     */
} cobel_dqn_replay_t;
/* 0 = the fused step covers this network / batch shape; fills *lds_bytes (per instance). */
COBEL_API int cobel_dqn_replay_query(int32_t n_inputs, int32_t n_hidden1, int32_t n_hidden2,
                                     int32_t n_actions, int32_t batch, int32_t is_float64,
                                     int32_t* lds_bytes);
COBEL_API int cobel_dqn_replay(const cobel_dqn_replay_t* run, void* stream);

/* ------------------------------------------------------------------------------------------
 * TorchNetwork.train_on_batch / predict_on_batch for STACKS of small networks — Linear(D <= 32,
 * 64)-ReLU-Linear(64, 64)-ReLU-Linear(64, O <= 32), batches of 32, float64 or float32 — one
 * kernel each (network/network_torch.py:110-167).  They carry DynaDSR.replay
 * (agent/dyna_q.py:1042-1150): per agent four online + four target successor networks
 * (D -> 64 -> 64 -> D) and one reward network (D -> 64 -> 64 -> 1).
 *
 * cobel_mlp_forward: out[j] = net[j / net_div](inputs of instance j), 32 rows per instance; the
 *   inputs are rows in_table[in_index[j / in_div][s]] of a float64 table or a dense block
 *   in_dense[j][32][D] in the network's dtype.  active[j / act_div] == 0: out[j] is not written.
 *   Every array that a divisor indexes (in_index, active, the parameters by net_div; in
 *   cobel_mlp_fit also targets by tgt_div and ep_index by ep_div) has ceil(n / divisor) entries:
 *   n need not be a multiple of any of them.
 * cobel_mlp_fit: network j takes ONE optimisation step towards targets[j / tgt_div][32][O] on its
 *   32 input rows: loss = mean over the samples marked in sample_mask[j] (NULL: all) and the O
 *   outputs of (out - target)^2, torch.optim.Adam with the network's own step count steps[j]
 *   (incremented here), then w_target += tau * (w - w_target).  The divisor of the mean is
 *   max(number of marked samples, 1) * O: a network that trains with NOTHING marked (train NULL or
 *   train[j] != 0 and an all-zero mask row) takes an Adam step on a zero gradient — its moments
 *   decay, its parameters move by what is left of them, its step count goes up.
 *   train[j] == 0: no optimiser step (parameters, moments and step count untouched, whatever the
 *   mask says) but the blend still happens, as the reference
 *   blends every network pair every step (agent/dyna_q.py:1134-1143).  active[j / act_div] == 0:
 *   nothing at all (ep_out[j] included).  Afterwards ep_out[j][ep_rows][O] receives the (updated)
 *   network's outputs — also of a network with train[j] == 0 — for ep_rows <= 4 extra rows: ONE
 *   row ep_table[ep_index[j / ep_div]] (ep_rows == 1) or ep_dense[j][ep_rows][D]; that is what the
 *   next action selection needs.  ep_rows == 0 or ep_out NULL: no extra rows, ep_out is not written.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* w[3];        /* [M][out][in], network dtype; M = ceil(n / net_div) */
  const void* b[3];        /* [M][out]                    */
  const uint8_t* active;   /* [ceil(n / act_div)] or NULL */
  const double* in_table;  /* [rows][D] float64, or NULL  */
  const int32_t* in_index; /* [ceil(n / in_div)][32]      */
  const void* in_dense;    /* [n][32][D], network dtype   */
  void* out;               /* [n][32][O]                  */
  int32_t n, n_inputs, n_outputs, is_float64;
  int32_t net_div, in_div, act_div, reserved_;
} cobel_mlp_forward_t;

typedef struct {
  void* w[3];              /* [n][out][in] */
  void* b[3];
  void* w_target[3];       /* blend targets, or NULL with tau == 0 */
  void* b_target[3];
  void* m_w[3];            /* Adam exp_avg / exp_avg_sq */
  void* m_b[3];
  void* v_w[3];
  void* v_b[3];
  double* steps;           /* [n] Adam step counts, += 1 for every network that trains            */
  const uint8_t* train;    /* [n] or NULL (= all)                                                 */
  const uint8_t* active;   /* [ceil(n / act_div)] or NULL                                         */
  const double* in_table;  /* inputs as for cobel_mlp_forward                                     */
  const int32_t* in_index;
  const void* in_dense;
  const void* targets;     /* [ceil(n / tgt_div)][32][O], network dtype                           */
  const uint8_t* sample_mask; /* [n][32] or NULL                                                  */
  const double* ep_table;  /* extra rows: one row of a float64 table ...                          */
  const int32_t* ep_index; /* ... [ceil(n / ep_div)]                                              */
  const void* ep_dense;    /* ... or [n][ep_rows][D], network dtype                               */
  void* ep_out;            /* [n][ep_rows][O] or NULL                                             */
  int32_t n, n_inputs, n_outputs, is_float64;
  int32_t in_div, tgt_div, act_div, ep_div, ep_rows;
  int32_t debug_stage;     /* 0; k = 1..4: return after the forward pass / the output layer / the
                              second layer's gradient / delta1 (phase timings, scripts/exp_mlp_fit.py) */
  double lr, beta1, beta2, eps, weight_decay, tau;
} cobel_mlp_fit_t;
/* 0 = this shape is covered; fills *lds_bytes (per workgroup). */
COBEL_API int cobel_mlp_query(int32_t n_inputs, int32_t n_hidden1, int32_t n_hidden2,
                              int32_t n_outputs, int32_t batch, int32_t is_float64,
                              int32_t* lds_bytes);
COBEL_API int cobel_mlp_forward(const cobel_mlp_forward_t* run, void* stream);
COBEL_API int cobel_mlp_fit(const cobel_mlp_fit_t* run, void* stream);

/* ------------------------------------------------------------------------------------------
 * TorchNetwork.get_layer_activity (network/network_torch.py:331-388) for a STACK of the networks
 * cobel_mlp_forward serves: the activity of one layer of every network on n_probes probe rows,
 * written units-major, out[j][k][p] = apply(Linear_layer(...)(probe p))[units[k]] — the reference's
 * (units, batch) orientation.  A forward hook on an nn.Linear sees the layer's pre-activation and
 * the reference then applies activations[layer]: `apply` is that function (COBEL_APPLY_*), while
 * `hidden_activation` (COBEL_ACT_*) is what the network itself applies between its layers.
 * layer 0 / 1 have 64 units, layer 2 has n_outputs.  units NULL: all of them in order; else
 * n_units numbers in any order, repeats allowed (they are read back and checked before the launch:
 * the call then waits for the stream).  n_probes is any positive number: the rows go through in
 * tiles of 32 with the network's weights held in registers.  probes_per_instance 0: one [P][D]
 * block for every network; 1: [n][P][D].  ReLU is pre > 0 ? pre : 0, as in the other kernels: a NaN
 * pre-activation gives 0 where torch.relu gives NaN.
 * COBEL_E_UNSUPPORTED for other shapes than cobel_mlp_forward's, COBEL_E_ARG for NULL tensors, an
 * unknown hidden_activation or misaligned 64-wide matrices, COBEL_E_RANGE for layer, apply, sizes
 * or a unit number out of range.  n == 0 returns COBEL_OK.
 * ------------------------------------------------------------------------------------------ */
enum { COBEL_APPLY_NONE = 0, COBEL_APPLY_RELU = 1, COBEL_APPLY_TANH = 2 };
typedef struct {
  const void* w[3];        /* [n][out][in], network dtype                          */
  const void* b[3];        /* [n][out]                                             */
  const void* probes;      /* [P][D] or [n][P][D], network dtype                   */
  const int32_t* units;    /* [dev] [n_units] or NULL                              */
  void* out;               /* [n][n_units or U][P], network dtype                  */
  int32_t n, n_probes, n_inputs, n_outputs, is_float64;
  int32_t layer;           /* 0, 1 or 2: which Linear                              */
  int32_t hidden_activation; /* COBEL_ACT_RELU / COBEL_ACT_TANH                    */
  int32_t apply;           /* COBEL_APPLY_*: on the chosen layer's Linear output   */
  int32_t n_units, probes_per_instance;
} cobel_mlp_activity_t;
COBEL_API int cobel_mlp_activity(const cobel_mlp_activity_t* run, void* stream);

/* process_activity_maps (analysis/network_spatial.py:45-67) on rows [n_rows][n_cols] in place, in
 * the rows' dtype: x -= min(x); x /= max(x); x[x < (T)threshold] = 0, each row equal to NumPy's bit
 * for bit.  NaN as NumPy: a row that holds one becomes all NaN, a constant row too (0 / 0). */
COBEL_API int cobel_activity_process(void* rows /* [dev] */, int64_t n_rows, int32_t n_cols,
                                     int32_t is_float64, double threshold, void* stream);

/* classify_place_field with sigma = 0 (analysis/network_spatial.py:70-144) for n_maps maps of
 * height x width cells (height width <= 4096) in one launch, one wavefront per map:
 *   thr = (T)cutoff * max(a) (NaN propagates);  field = a < thr ? 0 : a
 *   4-connected components of field > 0, ordered by their first cell in row-major order
 *   (scipy.ndimage.label's numbering); largest = the first component of maximal BOUNDING-BOX area
 *   error = 1 without a component, else 2 with more than 4, else 3 if
 *           (double)area[largest] > size_threshold * (double)(height * width), else 0
 * has_field[m] = error == 0; features[m] = the number of components; largest_area[m] = the box
 * area of the largest (height * width without a component); fields[m] = field where the cell
 * belongs to the largest component, else 0 — without a component the thresholded field itself, as
 * the reference returns it.  COBEL_E_ARG for NULL tensors or cutoff / size_threshold outside
 * (0, 1) (the reference's asserts), COBEL_E_RANGE for sizes < 1, COBEL_E_UNSUPPORTED beyond 4096
 * cells.  cobel_place_fields_plan: out = {LDS bytes per workgroup, maps per workgroup, LDS bytes
 * per map, threads per workgroup}. */
COBEL_API int cobel_place_fields_plan(int32_t height, int32_t width, int32_t is_float64,
                                      int32_t out[4]);
COBEL_API int cobel_place_fields(const void* maps /* [dev] [n_maps][height * width] */,
                                 int64_t n_maps, int32_t height, int32_t width, int32_t is_float64,
                                 double cutoff, double size_threshold,
                                 uint8_t* has_field /* [dev] [n_maps] */,
                                 int32_t* error /* [dev] [n_maps] */,
                                 int32_t* features /* [dev] [n_maps] */,
                                 int32_t* largest_area /* [dev] [n_maps] */,
                                 void* fields /* [dev] [n_maps][height * width] */, void* stream);

/* The regression targets of DynaDSR.replay (agent/dyna_q.py:1079-1131) for all samples of all
 * agents in ONE launch — what sits between the two forward passes and the two fits of a step:
 *   best[s]   = argmax_a value[a][s]   (first maximum)      | use_dr: the mean over the actions
 *   boot_sr   = successor[best[s]][s][:]                     |         of successor[a][s][:]
 *   nt        = nonterminal[s] != 0
 *   boot      = next_obs * ((1 - follow_up)(1 - ignore)) * (1 - nt) + boot_sr * min(nt + ignore, 1)
 *   targets[s][:] = (follow_up ? next_obs : obs) + gamma * boot
 *   took[a][s] = actions[s] == a;  train[a] = any_s took[a][s]
 * with obs / next_obs = rows state_index[s] / next_index[s] of the float64 observation table
 * converted to the network dtype.  Operation order as in the reference's expressions (and in the
 * PyTorch path of cobel_amd.agent.DynaDSR), element for element. */
typedef struct {
  const void* successor;      /* [n][A][32][O] network dtype: target networks on the next states  */
  const void* value;          /* [n][A][32]    network dtype: reward network on those             */
  const double* table;        /* [rows][O] float64 observation table                              */
  const int32_t* state_index; /* [n][32]                                                          */
  const int32_t* next_index;  /* [n][32]                                                          */
  const int64_t* actions;     /* [n][32]                                                          */
  const void* nonterminal;    /* [n][32] network dtype                                            */
  void* targets;              /* out [n][32][O] network dtype                                     */
  uint8_t* took;              /* out [n * A][32]                                                  */
  uint8_t* train;             /* out [n * A]                                                      */
  int32_t n, n_actions, n_outputs, is_float64;
  int32_t use_dr, follow_up, ignore_terminality, reserved_;
  double gamma;
} cobel_dsr_targets_t;
COBEL_API int cobel_dsr_targets(const cobel_dsr_targets_t* run, void* stream);

/* ------------------------------------------------------------------------------------------
 * Everything of one lockstep DQN training step that is not the network: per instance
 *   epsilon-greedy on the given Q-values (policy/greedy.py:40-88) -> env.step
 *   (interface/topology.py:146-157, gridworld.py:115-126) -> append the experience to the replay
 *   ring (memory/dqn.py:103-119; FIFO at capacity) -> trial bookkeeping and monitors
 *   (agent/dqn.py:186-212, monitor/behavior.py:73-97) with auto-reset (topology.py:170) ->
 *   draw the replay batch (memory/dqn.py:137: uniform over the stored entries, with replacement).
 * One lane per instance; instances whose `active` flag is 0 are left untouched (they consume no
 * draws).  Observations are rows of obs_table indexed by the env state (Topology poses, one-hot
 * rows for a Gridworld).  Outputs for cobel_dqn_replay: `stepped` (1 = the instance took part
 * in this step; its Adam step count adam_steps[i] has been incremented) and `batch_slots`.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  /* environment */
  int32_t* state;           /* [N] in/out                                                       */
  uint32_t* env_ctr;        /* [N] next index on COBEL_STREAM_ENV                               */
  const double* obs_table;  /* [S][n_obs] float64                                               */
  /* policy */
  const void* q;            /* [N][A] Q-values of the current observations, network dtype; A =
                               the world's action count: four, or 1 .. 8 on a world of
                               cobel_world_create_n (replay ring only, one-hot rows)            */
  uint32_t* policy_ctr;     /* [N] next index on the policy stream                              */
  uint32_t policy_stream;   /* COBEL_STREAM_POLICY or COBEL_STREAM_POLICY_TEST                  */
  int32_t is_float64;       /* dtype of q and of the ring's floating-point arrays               */
  double epsilon;
  /* replay ring, [N][slots][..] */
  void* ring_states;
  void* ring_next_states;
  int64_t* ring_actions;
  void* ring_rewards;
  void* ring_nonterminal;
  int32_t* ring_size;       /* [N] stored entries                                               */
  int64_t* ring_head;       /* [N] slot of the oldest entry                                     */
  uint32_t* memory_ctr;     /* [N] next index on COBEL_STREAM_MEMORY                            */
  /* trial bookkeeping */
  int32_t* trial;           /* [N] trials finished                                              */
  int32_t* step;            /* [N] steps taken in the running trial                             */
  double* trial_reward;     /* [N]                                                              */
  uint8_t* active;          /* [N] in/out: 0 once trial == trials_target                        */
  double* adam_steps;       /* [N] += 1 for every instance that steps                           */
  long long* lat_sum;       /* [mon_stripes][trial_cap] (instance i adds into copy i % mon_stripes) */
  long long* lat_cnt;
  double* reward_sum;
  /* outputs */
  uint8_t* stepped;         /* [N]                                                              */
  int32_t* batch_slots;     /* [N][batch]                                                       */
  /* sizes and parameters */
  int32_t n, n_obs, slots, batch;
  int32_t steps_per_trial, trials_target, trial_cap, mon_stripes;
  uint32_t instance_base;
  uint32_t reserved_;
  uint64_t seed;
  /* optional, instead of the replay ring (ring_* may then be NULL): the tabular world model of
     DynaDQN (memory/dyna_q.py:62-157 in float64, as the reference keeps it): store = running
     reward estimate + successor + non-terminal flag of (state, action); the batch = `batch` pairs
     drawn uniformly from ALL n_states x 4 pairs, written out gathered. */
  double* model_rewards;        /* [N][n_states * 4]                                            */
  int64_t* model_states;        /* [N][n_states * 4]                                            */
  double* model_nonterminal;    /* [N][n_states * 4]                                            */
  double model_lr;
  int32_t n_states;
  int32_t reserved2_;
  int32_t* batch_state_index;   /* [N][batch] out: state of each drawn pair                     */
  int32_t* batch_next_index;    /* [N][batch] out: its modelled successor                       */
  int64_t* batch_actions;       /* [N][batch] out                                               */
  void* batch_rewards;          /* [N][batch] out, network dtype                                */
  void* batch_nonterminal;      /* [N][batch] out, network dtype                                */
} cobel_dqn_act_t;
COBEL_API int cobel_dqn_act(const cobel_world_t* world, const cobel_dqn_act_t* run, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prioritized Memory Access (Mattar & Daw 2018).  Replaces PMAMemory.replay / store / update_sr
 * (memory/pma.py:168-267, :148-166, :413-415) and the trial loop of PMA.train / PMA.test
 * (agent/pma.py:167-317).  Every table is float64, as the reference's are: the gain is a
 * difference of nearly equal sums clipped at min_gain and the selection an exact-equality tie
 * test.  Worlds of up to COBEL_PMA_MAX_STATES states and COBEL_PMA_MAX_ACTIONS actions; with
 * COBEL_PMA_WIDE in cobel_pma_mem_t.flags the wide form, up to COBEL_PMA_WIDE_MAX_STATES states
 * (10-bit states in the replay records, 16-bit successors, up to 160 KiB of LDS per instance, and
 * update_sr by blocked kernels on the SR block in global memory).  The wide form is opt-in: T and
 * SR cost 8 * S * S bytes each per instance, 8 MiB each at 1 024 states.
 * Tables per instance: Q, rewards f64 [S][A]; states, terminals i32 [S][A]; T, SR f64 [S][S];
 * update_mask u8 [A * S], experience index a * S + s as in the reference.
 * Draws: the memory's generator is COBEL_STREAM_PMA_MEMORY at mem_ctr[i] — one double (sub-stream
 * COBEL_SUB_DOUBLE) per round for the tie draw, one bounded integer (sub-stream 0) for force_first;
 * the memory's policy object is pol_stream (COBEL_STREAM_PMA_POLICY unless it is the agent's own
 * policy object) at pol_ctr[i] — one double per extension action (policy/greedy.py:58).
 * ------------------------------------------------------------------------------------------ */
#define COBEL_STREAM_PMA_MEMORY 5u /* c = draws of PMAMemory.rng          (memory/pma.py:252, :258) */
#define COBEL_STREAM_PMA_POLICY 6u /* c = select_action calls of PMAMemory.policy (memory/pma.py:232) */
#define COBEL_PMA_MAX_STATES 128
#define COBEL_PMA_MAX_ACTIONS 8
#define COBEL_PMA_WIDE_MAX_STATES 1024
#define COBEL_PMA_EQUAL_NEED 1u        /* PMAMemory.equal_need                                   */
#define COBEL_PMA_EQUAL_GAIN 2u        /* PMAMemory.equal_gain                                   */
#define COBEL_PMA_IGNORE_BARRIERS 4u   /* PMAMemory.ignore_barriers (default on)                 */
#define COBEL_PMA_ALLOW_LOOPS 8u       /* PMAMemory.allow_loops                                  */
#define COBEL_PMA_GAIN_ORIGINAL 16u    /* PMAMemory.min_gain_mode == 'original'                  */
#define COBEL_PMA_SHARED_POLICY 32u    /* cobel_pma_trial: the memory's policy IS the agent's: its
                                          extension draws continue inst[COBEL_I_CTR_POLICY]         */
#define COBEL_PMA_SETS 128u            /* cobel_pma_mem_t.flags: the struct is the head of a
                                          cobel_pma_mem_sets_t, whose tail the call reads           */
#define COBEL_PMA_WIDE 64u             /* cobel_pma_mem_t.flags: the wide form (cobel_pma_plan_wide
                                          says what it serves); clear: every call behaves and
                                          refuses as the narrow form does                           */

/* Per-instance PMA parameters: the seven doubles of the memory a sweep varies (memory/pma.py:
 * 121-137) and the agent's three (agent/pma.py:158-159 and the acting policy's epsilon).  The reference
 * runs one simulation per combination; here instance i of ONE launch uses
 * param_sets[param_index[i]] in every entry point that reads a parameter.  The switches
 * (COBEL_PMA_*) and the replay length stay launch-wide.  Fill a set with
 * cobel_pma_param_set_fill, never by hand.  80 bytes, a multiple of 16 as it stands. */
typedef struct {
  double learning_rate, learning_rate_q, learning_rate_T; /* PMAMemory's                        */
  double gamma, gamma_q, min_gain;
  double epsilon;             /* of the memory's policy                                         */
  double alpha;               /* PMA.learning_rate                                              */
  double agent_gamma;         /* PMA.gamma (= PMA.gamma ** 1, cobel_pma_run_t.gamma_pow1)       */
  double agent_epsilon;       /* of the acting policy                                           */
} cobel_pma_param_set_t;
/* Host only.  memory[7] in the order of the first seven members, taken verbatim but for the
 * ranges the kernels rest on: an epsilon (memory[6], agent_epsilon) outside [0, 1] is refused
 * (COBEL_E_ARG, the value in the message) as the scalar launches refuse it, and so is a memory
 * gamma (memory[3]) outside [0, 1): update_sr eliminates without pivoting, which rests on
 * I - gamma T being strictly diagonally dominant.  Nothing else has a range. */
COBEL_API int cobel_pma_param_set_fill(const double memory[7], double alpha, double agent_gamma,
                                       double agent_epsilon,
                                       cobel_pma_param_set_t* out /* [host] */);

typedef struct {
  double* q;                  /* [N][S][A] the Q-function the replay updates                    */
  double* rewards;            /* [N][S][A]                                                      */
  int32_t* states;            /* [N][S][A]                                                      */
  int32_t* terminals;         /* [N][S][A] experience['terminal'] = 1 - end_trial               */
  double* T;                  /* [N][S][S]                                                      */
  double* SR;                 /* [N][S][S]                                                      */
  uint8_t* update_mask;       /* [N][A * S]                                                     */
  const uint8_t* action_mask; /* [S] bit a = action a allowed, or NULL                          */
  uint32_t* mem_ctr;          /* [N] next index on COBEL_STREAM_PMA_MEMORY                      */
  uint32_t* pol_ctr;          /* [N] next index on pol_stream                                   */
  const double* gamma_pow;    /* [pow_len] gamma ** k, filled by the host; with parameter sets
                                 [n_param_sets][pow_len], row k holding set k's powers          */
  const double* gamma_q_pow;  /* [pow_len] gamma_q ** k; with sets [n_param_sets][pow_len]      */
  int32_t n, n_states, n_actions, pow_len;
  uint32_t instance_base, flags /* COBEL_PMA_* */, pol_stream, reserved_;
  double learning_rate, learning_rate_q, learning_rate_T, gamma, gamma_q, min_gain, epsilon;
  uint64_t seed;
} cobel_pma_mem_t;

/* cobel_pma_mem_t with the optional per-instance parameter sets behind it.  cobel_pma_mem_t itself
 * keeps its 192 bytes: a caller that has sets builds THIS struct, sets COBEL_PMA_SETS in mem.flags
 * and hands &x.mem to the entry points, which read the tail only under that flag (without it the
 * memory behind the 192 bytes is never looked at).  A zeroed tail is the scalar launch.  With
 * param_index != NULL instance i uses param_sets[param_index[i]] and row param_index[i] of the two
 * power tables (an index >= n_param_sets is clamped to the last set); the seven scalars of mem —
 * and alpha, gamma_pow1 and epsilon of cobel_pma_run_t — are ignored.  1 .. 65 535 sets.
 * Refused before any launch (COBEL_E_ARG): an index without sets, n_param_sets < 1, param_sets
 * not 16-byte or param_index not 2-byte aligned, pow_len not above the replay length.
 * cobel_pma_stationary* and cobel_pma_action_probs read no parameter and do not look here. */
typedef struct {
  cobel_pma_mem_t mem;
  const cobel_pma_param_set_t* param_sets; /* [dev] [n_param_sets], 16-byte aligned             */
  const uint16_t* param_index;             /* [dev] [N]                                         */
  int32_t n_param_sets, reserved_;
} cobel_pma_mem_sets_t;

/* One performed update (memory/pma.py:263), 24 bytes. */
typedef struct {
  int32_t state, action, next_state, terminal;
  double reward;
} cobel_pma_rec_t;
/* One experience per instance (memory/pma.py:148-166), 24 bytes.  state < 0: none. */
typedef cobel_pma_rec_t cobel_pma_exp_t;

typedef struct {
  int32_t* inst;              /* [N][COBEL_I_WORDS]                                             */
  unsigned long long* lat_sum; /* monitors as in cobel_tab_run_t; each may be NULL              */
  unsigned long long* lat_cnt;
  double* reward_sum;
  unsigned long long* resp_cnt;
  int32_t* lat_trace;         /* [N][trial_cap] or NULL                                         */
  unsigned long long* occupancy;
  unsigned long long* steps_done;
  int32_t* last;              /* [N] out: the terminal state the trial reached, or -1           */
  cobel_pma_rec_t* replay_out; /* [N][batch] out: the start-of-trial replay                     */
  int32_t trial_cap, mon_stripes, steps_per_trial, batch;
  uint32_t flags;             /* COBEL_F_LEARN | COBEL_F_NO_REPLAY | COBEL_F_MASK_ACTIONS |
                                 COBEL_F_TEST_STREAM, and COBEL_PMA_SHARED_POLICY << 16          */
  uint32_t reserved_;
  double alpha;               /* PMA.learning_rate                                              */
  double gamma_pow1;          /* PMA.gamma ** 1, from the host                                  */
  double epsilon;             /* of the acting policy                                           */
} cobel_pma_run_t;

/* Launch shapes: out = {LDS bytes of a replay / trial workgroup (one wavefront per instance),
 * its threads, LDS bytes of an update_sr workgroup (one per instance), its threads}.
 * COBEL_E_UNSUPPORTED beyond COBEL_PMA_MAX_STATES / COBEL_PMA_MAX_ACTIONS, or where the sequence
 * of a replay of that length no longer fits 64 KiB of LDS beside the tables. */
COBEL_API int cobel_pma_plan(int32_t n_states, int32_t n_actions, int32_t replay_length,
                             int32_t out[4]);
/* The same for the wide form (COBEL_PMA_WIDE): COBEL_E_UNSUPPORTED beyond
 * COBEL_PMA_WIDE_MAX_STATES / COBEL_PMA_MAX_ACTIONS, or where the tables and the sequence do not
 * fit 160 KiB of LDS (1 024 states with 8 actions do not; the message gives the byte counts).
 * out[2] / out[3] are those of the blocked update_sr kernels beyond COBEL_PMA_MAX_STATES states. */
COBEL_API int cobel_pma_plan_wide(int32_t n_states, int32_t n_actions, int32_t replay_length,
                                  int32_t out[4]);
/* PMAMemory.replay (memory/pma.py:168-267) once per instance on mem->q: replay_length rounds of
 * compute_gain_batch (:333-386) / compute_gain (:269-331) for the extended sequence, utility =
 * gain * need * update_mask, the draw among exact ties (:251-254), force_first (:256-259), the
 * n-step update_q (:452-496).  current_state [dev] [N] (entry >= 0: need = SR[state], :411) or
 * NULL; an entry < 0 — or NULL — takes the instance's row of need [dev] [N][S] (compute_need(None),
 * :403-408, evaluated by the caller).  force_first [dev] [N] (entry < 0: none) or NULL.  records
 * [dev] [N][replay_length] out. */
COBEL_API int cobel_pma_replay(const cobel_pma_mem_t* mem, int32_t replay_length,
                               const int32_t* current_state, const double* need,
                               const int32_t* force_first, cobel_pma_rec_t* records, void* stream);
/* One trial of PMA.train (agent/pma.py:192-245; COBEL_F_LEARN) or PMA.test (:274-314) in every
 * instance: reset, the start-of-trial replay of run->batch rounds with need = SR[start state],
 * then up to steps_per_trial steps of select_action -> env.step -> the agent's 1-step update_q
 * (:319-353, alpha / gamma_pow1) -> PMAMemory.store.  The end-of-trial update_sr and replay are
 * calls of their own (cobel_pma_update_sr, cobel_pma_replay). */
COBEL_API int cobel_pma_trial(const cobel_world_t* world, const cobel_pma_mem_t* mem,
                              const cobel_pma_run_t* run, void* stream);
/* PMAMemory.store (memory/pma.py:148-166) in every instance. */
COBEL_API int cobel_pma_store(const cobel_pma_mem_t* mem, const cobel_pma_exp_t* experiences,
                              void* stream);
/* PMAMemory.update_sr (memory/pma.py:413-415): SR = inv(I - gamma T) per instance, in-place
 * Gauss-Jordan without pivoting (I - gamma T is strictly diagonally dominant by rows): in LDS up
 * to COBEL_PMA_MAX_STATES states, beyond (wide form) blocked over panels of 32 pivots on the SR
 * block in global memory, the same operations per element in the same order. */
COBEL_API int cobel_pma_update_sr(const cobel_pma_mem_t* mem, void* stream);
/* PMAMemory.compute_need(None) (memory/pma.py:403-408) per instance: |v| for the unit-2-norm
 * left eigenvector v of mem->T for the eigenvalue 1, i.e. the stationary distribution of T
 * divided by its 2-norm.  select [dev][N] or NULL: an instance whose entry is >= 0 is skipped
 * (its row of need and its status are not written); NULL selects all.  need [dev][N][S] out,
 * status [dev][N] out (0 ok, 1 degenerate).  Reads mem->T, n, n_states (and the form in flags)
 * only.  So cobel_pma_replay's current_state serves as select, and need as its need.
 * Method: T is row-stochastic, so the vector solves (I - T + (1/S) 1 1^T)^T x = (1/S) 1; one
 * float64 Gaussian elimination with partial pivoting per instance in LDS (one workgroup each),
 * |x| divided by its 2-norm, every operation in a fixed order — no iteration, and the same bits
 * from the same T whatever the batch.  Every T with a simple eigenvalue 1 is served, transient
 * states included.  Degenerate (status 1): a pivot is exactly zero or the result is not finite;
 * need is then 1 / sqrt(S) in every component.  With a multiple eigenvalue 1 the reference
 * returns whichever vector of the eigenspace LAPACK's iteration ends on; this call returns that
 * defined one, or, where rounding hides the singularity, some finite vector with status 0.
 * COBEL_E_UNSUPPORTED beyond COBEL_PMA_MAX_STATES states and for the wide form (COBEL_PMA_WIDE:
 * T and SR leave no S x S workspace in LDS; cobel_pma_stationary_wide below serves it);
 * COBEL_E_RANGE for n < 1. */
COBEL_API int cobel_pma_stationary(const cobel_pma_mem_t* mem, const int32_t* select,
                                   double* need, int32_t* status, void* stream);
/* Launch shape of cobel_pma_stationary: out = {LDS bytes of a workgroup (one per instance): the
 * S x (S + 1) augmented matrix at a row stride of the next odd count past S, the multipliers,
 * pivots and solution; its threads}.  COBEL_E_UNSUPPORTED beyond COBEL_PMA_MAX_STATES. */
COBEL_API int cobel_pma_plan_need(int32_t n_states, int32_t out[2]);
/* The same vectors beyond the LDS: 1 .. COBEL_PMA_WIDE_MAX_STATES states, the elimination on a
 * caller-owned workspace in device memory.  select, need and status as in cobel_pma_stationary;
 * reads mem->T, n and n_states only (COBEL_PMA_WIDE in flags is not looked at).  The same
 * operations per element in the same order as the LDS kernel, so the same bits wherever both run.
 * Workspace per instance, in bytes (cobel_pma_plan_need_wide's out[0]):
 *     8 * S * (S + 1) + 4 * (S + 1), rounded up to a multiple of 16
 * — the augmented matrix, the pivot rows and one mark word; 8 MiB at 1 024 states.  work [dev],
 * 8-byte aligned, holds work_bytes / that many instances (at least one); the n instances are taken
 * in groups of that size, one group after the other in the stream, and the result does not depend
 * on the group size.  The workspace holds nothing of value between calls.
 * Method: a right-looking LU with partial pivoting, blocked over panels of 16 pivots; per panel
 * three launches ordered by the stream — the panel with pivoting (one workgroup per instance, the
 * whole remaining height in LDS), the panel's swaps and its rows of U in the columns to the right,
 * the rank-16 update of the rest over 64 x 64 tiles (one instance uses the whole chip) — then one
 * workgroup per instance for the back substitution and the norm.  No kernel waits for another
 * workgroup and nothing is read back; a degenerate instance is marked in its workspace and skipped
 * by the later launches.
 * COBEL_E_ARG: NULL mem, T, need, status or work, a misaligned pointer, or a workspace smaller
 * than one instance's (the message names the bytes needed); COBEL_E_RANGE: n < 1;
 * COBEL_E_UNSUPPORTED: n_states outside 1 .. COBEL_PMA_WIDE_MAX_STATES.  Every refusal comes before
 * any launch. */
COBEL_API int cobel_pma_stationary_wide(const cobel_pma_mem_t* mem, const int32_t* select,
                                        double* need, int32_t* status, void* work,
                                        int64_t work_bytes, void* stream);
/* out = {workspace bytes per instance, LDS bytes of the largest workgroup (the panel kernel's
 * S x 17 doubles from 241 states on, the back substitution's below), its threads, the panel width}.
 * COBEL_E_UNSUPPORTED outside 1 .. COBEL_PMA_WIDE_MAX_STATES, with out zeroed. */
COBEL_API int cobel_pma_plan_need_wide(int32_t n_states, int64_t out[4]);

/* The observables of the memory as calls of their own (csrc/pma_gain.hip): the gain map, the gain
 * of given n-step updates, the action probabilities of a table and the n-step update_q.  The same
 * expressions, operation for operation, as cobel_pma_replay evaluates every round.  All four read
 * their tables in place from device memory, so one form serves 1 .. COBEL_PMA_WIDE_MAX_STATES
 * states and 1 .. COBEL_PMA_MAX_ACTIONS actions (COBEL_PMA_WIDE in flags is not looked at), draw
 * no number and move no counter.  Every refusal comes before any launch: COBEL_E_ARG for a NULL
 * or misaligned argument, a stride that is none of those named, an epsilon outside [0, 1] or power
 * tables of pow_len <= the longest sequence; COBEL_E_UNSUPPORTED for a state or action count
 * outside the range and a max_len outside 1 .. COBEL_PMA_MAX_SEQ; COBEL_E_RANGE for n, n_seq or
 * rows < 0 and a length outside 1 .. max_len.
 * A sequence is cobel_pma_rec_t[max_len], valid up to its length; states, actions and successors
 * outside the world are clamped into it.  lengths is [host]: it is checked by the call and
 * travels to the device in the stream (the call waits for that copy where the array is not
 * pinned). */
#define COBEL_PMA_MAX_SEQ 256          /* steps of one sequence of cobel_pma_gain_seq / _update_q */
/* PMAMemory.compute_gain_batch (memory/pma.py:333-386) per instance: the gain of every one-step
 * backup, clipped at min_gain.  q [dev] [N][S][A] with q_stride = S * A, or one [S][A] table for
 * every instance with q_stride = 0; gain [dev] [N][A * S] out, index a * S + s.  Reads
 * mem->rewards, states, terminals, action_mask, learning_rate_q, gamma_q, min_gain and epsilon;
 * mem->q and COBEL_PMA_EQUAL_GAIN are not looked at (the reference applies equal_gain in replay). */
COBEL_API int cobel_pma_gain_batch(const cobel_pma_mem_t* mem, const double* q, int64_t q_stride,
                                   double* gain, void* stream);
/* PMAMemory.compute_gain (memory/pma.py:269-331) for n_seq n-step updates per instance.  steps
 * [dev] [n_seq][max_len] and lengths [host] [n_seq] with inst_stride = 0 (every instance scores the
 * same list), or [N][n_seq][max_len] and [N][n_seq] with inst_stride = n_seq * max_len; gain [dev]
 * [N][n_seq] out.  As in the reference the rewards are discounted by mem->gamma_pow (gamma ** k)
 * and the bootstrap — the unmasked row maximum times the last step's terminal — by
 * mem->gamma_q_pow (gamma_q ** (n - j)), the policies are not normalised, a step gain is clipped at
 * min_gain only under COBEL_PMA_GAIN_ORIGINAL, the sum (step 0 first) always. */
COBEL_API int cobel_pma_gain_seq(const cobel_pma_mem_t* mem, const double* q, int64_t q_stride,
                                 const cobel_pma_rec_t* steps, const int32_t* lengths,
                                 int32_t n_seq, int32_t max_len, int64_t inst_stride, double* gain,
                                 void* stream);
/* PMAMemory.action_probs_batch (memory/pma.py:423-450): the epsilon-greedy probabilities
 * (policy/greedy.py:77-86) of every row, divided by the row's sum.  q, probs [dev] [rows][A];
 * mask_bits [dev] [rows] (bit a = action a allowed) or NULL.  Any row count: the reference calls
 * it with the tiled [A * S][A] table. */
COBEL_API int cobel_pma_action_probs(const double* q, const uint8_t* mask_bits, int64_t rows,
                                     int32_t n_actions, double epsilon, double* probs, void* stream);
/* The n-step update_q of PMAMemory (memory/pma.py:452-496: learning_rate_q, gamma_q ** k) and of
 * the PMA agent (agent/pma.py:319-353: learning_rate, gamma ** k), in place on q [dev] [N][S][A]:
 * one sequence per instance, steps [dev] [N][max_len] and lengths [host] [N] with inst_stride =
 * max_len, or one for all with inst_stride = 0.  The bootstrap value is read before any write, the
 * steps are applied in order (a repeated (s, a) sees the earlier write), and a sequence of more
 * than one step that holds a terminal == 0 changes nothing (:476-489).  pow_table [dev] [pow_len].
 * Reads mem->n, n_states and n_actions only. */
COBEL_API int cobel_pma_update_q(const cobel_pma_mem_t* mem, double* q,
                                 const cobel_pma_rec_t* steps, const int32_t* lengths,
                                 int32_t max_len, int64_t inst_stride, double learning_rate,
                                 const double* pow_table, int32_t pow_len, void* stream);
/* The same update with the learning rate and the powers of each instance's parameter set
 * (mem->param_index is required).  which = COBEL_PMA_Q_MEMORY: learning_rate_q and the instance's
 * row of mem->gamma_q_pow (PMAMemory.update_q); COBEL_PMA_Q_AGENT: alpha and the instance's row of
 * agent_pow [dev] [n_param_sets][mem->pow_len], row k holding set k's agent_gamma ** j (PMA.update_q)
 * — a pointer argument, so cobel_pma_mem_t carries the memory's two tables only; it is not looked
 * at under COBEL_PMA_Q_MEMORY.  Reads mem->n, n_states, n_actions, pow_len and the sets. */
#define COBEL_PMA_Q_MEMORY 0
#define COBEL_PMA_Q_AGENT 1
COBEL_API int cobel_pma_update_q_sets(const cobel_pma_mem_t* mem, double* q,
                                      const cobel_pma_rec_t* steps, const int32_t* lengths,
                                      int32_t max_len, int64_t inst_stride, int32_t which,
                                      const double* agent_pow, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The similarity metrics of SFMA (memory/utils/metrics.py:66-268) for stacks of four-action worlds
 * given by their compact successor tables: SR.D = inv(I - gamma T) (:66-105) and DR.D, the same
 * inverse of the default world corrected by the Woodbury identity (:107-268).  Everything is
 * float64, one rounding per operation, every sum in ascending index order (no MFMA), so a matrix
 * depends on its own world alone and equals the NumPy restatement of tests/metric_common.py bit
 * for bit.  Neither call has a status word; every refusal comes before any launch.
 * --------------------------------------------------------------------------------------------- */
#define COBEL_METRIC_MAX_STATES 16383  /* what cobel_sfma_run serves                              */
#define COBEL_METRIC_MAX_RANK 128      /* affected states per world: the k x k block of the
                                        * Woodbury correction at a row stride of k + 1 doubles and
                                        * its bookkeeping (pivots, the rows of delta, the pivot
                                        * search) take 152 064 of a workgroup's 163 840 bytes of LDS */
#define COBEL_METRIC_MAX_WORLDS 65535  /* worlds of one call (the grid's z axis)                  */
/* SR(sas, gamma).D (metrics.py:66-105) of n_worlds worlds: next [dev] [n_worlds][S][4] successor
 * of (state, action); D [dev] [n_worlds][S][S] out.  L = I - gamma T is written straight from the
 * table (T[s][c] = count / 4; 1.0 - gamma t on the diagonal, 0.0 - gamma t elsewhere; no dense T is
 * formed), then inverted in place by Gauss-Jordan without pivoting (L is strictly diagonally
 * dominant by rows for gamma < 1): pivots ascending, the pivot row scaled by 1 / pivot (the pivot's
 * place takes 1 / pivot), every other element M - col[r] * row[c] (0 - col[r] * row[k] in column
 * k); blocked over panels of 32 pivots as cobel_pma_update_sr's wide form, 1 + 3 ceil(S / 32)
 * launches ordered by the stream.
 * COBEL_E_ARG: a NULL or misaligned pointer, n_worlds < 1, gamma outside [0, 1);
 * COBEL_E_UNSUPPORTED: n_states outside 1 .. COBEL_METRIC_MAX_STATES, more than
 * COBEL_METRIC_MAX_WORLDS worlds. */
COBEL_API int cobel_metric_sr(const int32_t* next, int32_t n_worlds, int32_t n_states, double gamma,
                              double* D, void* stream);
/* DR.update_transitions (metrics.py:107-268): D_w = D0 - (D0[:, J_w] alpha_w) (delta_w D0) per
 * world.  D0 [dev] [S][S] is the metric of the default world, shared by all worlds (cobel_metric_sr
 * on next_default); next [dev] [n_worlds][S][4]; next_default [dev] [S][4]; J [HOST]
 * [n_worlds][max_rank], row w holding rank[w] affected states in strictly ascending order
 * (np.unique of the first members of invalid_transitions); rank [HOST] [n_worlds]; D [dev]
 * [n_worlds][S][S] out, not D0.  J and rank are copied into the workspace in stream order; they
 * must stay valid until the stream has passed the call.
 *   delta  rows (I - gamma T_new)[J] - (I - gamma T_default)[J], those very expressions on the at
 *          most nine columns where either table has an entry (the state, four successors each)
 *   A      I_k + delta D0[:, J]
 *   alpha  A^-1 by in-place Gauss-Jordan with partial pivoting in LDS, one workgroup per world
 *          (pivot: largest magnitude in the column, lowest row on ties)
 *   D      X = delta D0, Y = D0[:, J] alpha, D = D0 - Y X over 64 x 64 tiles (D0 and D touched
 *          once); terms of delta that are exactly zero are skipped (they change no bit)
 * A world of rank 0 gets a copy of D0.  Four launches (one with max_rank 0).
 * work [dev], 16-byte aligned, of at least
 *     (4 * n_worlds * (1 + max_rank), rounded up to 16) + n_worlds * cobel_metric_plan's out[3]
 * bytes for (n_states, max_rank); it holds nothing of value between calls.
 * COBEL_E_ARG: a NULL or misaligned pointer, D == D0, n_worlds < 1, gamma outside [0, 1), a rank
 * outside 0 .. max_rank, J unsorted or out of range, a workspace too small (the message names the
 * bytes); COBEL_E_UNSUPPORTED: n_states outside 1 .. COBEL_METRIC_MAX_STATES, a rank above
 * COBEL_METRIC_MAX_RANK, more than COBEL_METRIC_MAX_WORLDS worlds. */
COBEL_API int cobel_metric_dr(const double* D0, const int32_t* next, const int32_t* next_default,
                              const int32_t* J, const int32_t* rank, int32_t max_rank,
                              int32_t n_worlds, int32_t n_states, double gamma, double* D,
                              void* work, int64_t work_bytes, void* stream);
/* out = {form of cobel_metric_sr (0: the matrix is one diagonal block, up to 32 states; 1:
 * blocked), LDS bytes of the largest workgroup of cobel_metric_sr and — rank > 0 — cobel_metric_dr
 * at that rank, its threads, workspace bytes per world of cobel_metric_dr at max_rank = rank}.
 * COBEL_E_UNSUPPORTED outside 1 .. COBEL_METRIC_MAX_STATES states or 0 .. COBEL_METRIC_MAX_RANK,
 * with out zeroed. */
COBEL_API int cobel_metric_plan(int32_t n_states, int32_t rank, int64_t out[4]);

/* ---------------------------------------------------------------------------------------------
 * Model-Free Episodic Control (Blundell et al. 2016).  Replaces ActionBuffer / QEC
 * (agent/mfec.py:28-237: find_state, find_neighbors, add, replace, estimate, update,
 * update_episode) and the trial loops of MFEC.train / MFEC.test / predict_on_batch
 * (agent/mfec.py:423-559).  Everything is float64, as in the reference.
 *
 * The observation of a tabular world is a function of the node, so the buffers hold node ids and
 * the k-d tree's arithmetic is done once per world: cobel_mfec_pairs turns the feature table
 * F[S][D] (row = process_observation of that node's observation, agent/mfec.py:362-403) into the
 * S x S table of reduced distances (scikit-learn's euclidean_rdist: sum over d of (x - y)^2,
 * sequential, multiply and add rounded separately) and the S x S table of find_state's
 * np.allclose(stored, query, rtol=1e-4, atol=1e-6) (agent/mfec.py:76; not symmetric).  A query
 * follows a KDTree of one leaf: every entry in index order onto a max-heap of k (sklearn/utils/
 * _heap.pyx), then simultaneous_sort (sklearn/utils/_sorting.pyx) — the order among equidistant
 * entries, and so the float64 sum of estimate (agent/mfec.py:195-200), is the tree's.  Time stamps
 * are a per-instance counter that advances by one per training step (the reference stamps
 * time.time(), of which only the order matters). */
#define COBEL_MFEC_MAX_STATES 1024
#define COBEL_MFEC_MAX_ACTIONS 8
#define COBEL_MFEC_MAX_CAPACITY 2048
#define COBEL_MFEC_MAX_K 32
#define COBEL_MFEC_MAX_FEATURES 65536

typedef struct {
  const double* rdist;        /* [S][S] reduced distances (cobel_mfec_pairs)                    */
  const uint8_t* same;        /* [S][S] same[q * S + j] = allclose(F[j], F[q]): 0 / 1           */
  int32_t* ids;               /* [N][A][capacity] node ids (ActionBuffer.states)                */
  double* values;             /* [N][A][capacity] ActionBuffer.values                           */
  int32_t* times;             /* [N][A][capacity] ActionBuffer.times                            */
  int32_t* len;               /* [N][A] len(ActionBuffer)                                       */
  int32_t* clock;             /* [N] the stamp of the last training step                        */
  int32_t n, n_states, n_actions, capacity, k, reserved_;
} cobel_mfec_mem_t;

typedef struct {
  int32_t* inst;              /* [N][COBEL_I_WORDS]; COBEL_I_FLAGS bit 0: a trial is under way  */
  unsigned long long* lat_sum; /* monitors as in cobel_tab_run_t; each may be NULL              */
  unsigned long long* lat_cnt;
  double* reward_sum;
  unsigned long long* resp_cnt;
  int32_t* lat_trace;         /* [N][trial_cap] or NULL                                         */
  unsigned long long* occupancy;
  unsigned long long* steps_done;
  int32_t* last_exp;          /* [N][6] as in cobel_tab_run_t (td = 0), or NULL                 */
  int32_t* ep_sa;             /* [N][steps_per_trial] scratch: the episode, state | action << 16 */
  double* ep_value;           /* [N][steps_per_trial] scratch: its rewards, then its returns    */
  double* trace;              /* [N][trace_cap][4 + A] or NULL: state, action, reward, end and the
                                 estimates handed to the policy, of every step                 */
  int32_t* trace_len;         /* [N] rows of trace written so far (NULL iff trace is)           */
  int32_t n, trial_cap, mon_stripes, trace_cap;
  uint32_t instance_base, flags; /* COBEL_F_LEARN (train: episodes are written back) |
                                    COBEL_F_TEST_STREAM                                         */
  int32_t trials_target, steps_per_trial, step_budget, reserved_;
  double gamma;               /* MFEC.gamma                                                     */
  double epsilon;             /* of the acting policy                                           */
  uint64_t seed;
} cobel_mfec_run_t;

/* The two S x S tables of a world from its features [dev] [S][D]; rdist [dev] [S][S] and same
 * [dev] [S][S] out.  COBEL_E_UNSUPPORTED beyond COBEL_MFEC_MAX_STATES / COBEL_MFEC_MAX_FEATURES. */
COBEL_API int cobel_mfec_pairs(const double* features, int32_t n_states, int32_t n_features,
                               double* rdist, uint8_t* same, void* stream);
/* MFEC.train (agent/mfec.py:423-484; COBEL_F_LEARN) or MFEC.test (:486-532) in every instance, one
 * wavefront each, until trials_target trials are done or step_budget (> 0) steps: reset, then per
 * step retrieve_q (:405-421, QEC.estimate :173-200 per action) -> select_action -> env.step -> the
 * episode row; at a terminal step the discounted returns backward through the episode (:472-476)
 * and QEC.update_episode (:202-236) event by event.  A trial that times out leaves the memory as it
 * was.  The world must be a single one (the tables of mem are its).  COBEL_E_UNSUPPORTED beyond
 * COBEL_MFEC_MAX_STATES / _ACTIONS / _CAPACITY / _K. */
COBEL_API int cobel_mfec_run(const cobel_world_t* world, const cobel_mfec_mem_t* mem,
                             const cobel_mfec_run_t* run, void* stream);
/* MFEC.predict_on_batch (agent/mfec.py:534-559) on frozen buffers: nodes [dev] [B], out [dev]
 * [N][B][A]. */
COBEL_API int cobel_mfec_estimate(const cobel_mfec_mem_t* mem, const int32_t* nodes,
                                  int32_t n_nodes, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Associative learning: the Sequence environment (interface/sequence.py:25-215), the scalar
 * policies Proportional / Threshold / Sigmoid (policy/scalar.py:13-300) and the agents
 * RescorlaWagner / BinaryRescorlaWagner (agent/rw.py:15-376).  Everything is float64.
 *
 * A Sequence is compiled once into tables shared by all instances: the observation table (row 0 is
 * the zero observation of zero_current(), sequence.py:115-127), per schedule step the index of its
 * observation, its reward row with the flag "the reward is one float" (sequence.py:159), its forced
 * action (-1: None), and per schedule the offsets of its trials.  An instance follows one schedule;
 * its position (current_trial, current_step) lives on the device.
 *
 * An instance takes a group of G lanes, G = dim rounded up to a power of two, one lane per weight.
 * W @ state is the balanced binary tree over G leaves W[j] * state[j] (each rounded; leaves beyond
 * dim are +0.0), adjacent leaves first. */
#define COBEL_RW_MAX_DIM 64
#define COBEL_RW_POLICY_NONE 0          /* RescorlaWagner: the value itself is the action        */
#define COBEL_RW_POLICY_PROPORTIONAL 1  /* policy/scalar.py:52-68, one double draw per step      */
#define COBEL_RW_POLICY_THRESHOLD 2     /* :151-172, one bounded draw per step inside the window */
#define COBEL_RW_POLICY_SIGMOID 3       /* :256-274, one double draw per step                    */

typedef struct {
  const double* obs_table;    /* [n_obs][dim]; row 0 is all zero                                */
  const int32_t* step_obs;    /* [n_steps] row of obs_table                                     */
  const int32_t* step_action; /* [n_steps] TrialStep['action'], -1 for None                     */
  const uint8_t* step_scalar; /* [n_steps] 1: the reward is one float (column 0 of its row)     */
  const double* step_reward;  /* [n_steps][n_actions]                                           */
  const int32_t* trial_off;   /* [n_schedules][n_trials + 1] first step of every trial          */
  const int32_t* schedule_of; /* [n] schedule of every instance, or NULL: schedule 0            */
  int32_t* cur_trial;         /* [n] Sequence.current_trial                                     */
  int32_t* cur_step;          /* [n] Sequence.current_step                                      */
  int32_t n, dim, n_obs, n_actions, n_schedules, n_trials, n_steps, overwrite;
} cobel_seq_t;

typedef struct {
  double* W;                  /* [n][dim] the weights                                           */
  const double* lr;           /* [lr_rows][dim] learning rates                                  */
  const double* pol;          /* [pol_rows][4] threshold, window / 2, scale, value_max; or NULL */
  uint32_t* pol_ctr;          /* [n] draws taken from the policy's stream so far; or NULL       */
  const uint32_t* instance_ids; /* [n] stream instance numbers, or NULL: instance_base + i      */
  int32_t* mid;               /* [n] 1: a trial is under way (step_budget ran out inside it)    */
  double* trew;               /* [n] its reward so far                                          */
  double* trial_reward;       /* [n][trial_cap] logs['trial_reward'] of every trial, or NULL    */
  int32_t* trial_steps;       /* [n][trial_cap] logs['steps'] (index of its last step), or NULL */
  int32_t* trial_action;      /* [n][trial_cap] logs['action'] (its last action), or NULL       */
  double* trace;              /* [n][trace_cap][4] value, action, reward, end of every step, or
                                 NULL                                                           */
  int32_t* trace_len;         /* [n] rows of trace written so far (NULL iff trace is)           */
  unsigned long long* steps_done; /* env steps executed, added to; or NULL                      */
  int32_t n, trial_cap, trace_cap, lr_rows, pol_rows, policy, code_reverse, reserved_;
  uint32_t instance_base, flags;  /* COBEL_F_LEARN: train (the weights are updated)             */
  uint32_t pol_stream, reserved2_;
  int32_t trial_first;        /* row of the per-trial traces the session's first trial takes    */
  int32_t trials;             /* trials to run                                                  */
  int32_t steps_per_trial;    /* the cap of train(interface, trials, steps)                     */
  int32_t step_budget;        /* > 0: stop after that many steps (launch per step)              */
  uint64_t seed;
} cobel_rw_run_t;

/* Launch shape of cobel_rw_run for n instances of dim weights: out = {lanes per instance,
 * instances per wavefront, instances per workgroup, workgroups}.  COBEL_E_UNSUPPORTED beyond
 * COBEL_RW_MAX_DIM. */
COBEL_API int cobel_rw_plan(int32_t dim, int32_t n, int32_t out[4]);
/* RescorlaWagner.train / test (agent/rw.py:76-174) or BinaryRescorlaWagner.train / test
 * (:267-376) with Sequence.reset / step and the policy's select_action inside, `trials` trials in
 * every instance in one launch.  A trial cut by steps_per_trial is replayed from its first step.
 * The caller guarantees that no instance runs past its last trial (the position depends on the
 * schedule and the caps alone). */
COBEL_API int cobel_rw_run(const cobel_seq_t* seq, const cobel_rw_run_t* run, void* stream);
/* RescorlaWagner.predict_on_batch (agent/rw.py:176-192): out [dev] [n][n_batch] = W [dev] [n][dim]
 * times batch [dev] [n_batch][dim], row by row in the summation order of cobel_rw_run. */
COBEL_API int cobel_rw_predict(const double* W, int32_t n, int32_t dim, const double* batch,
                               int32_t n_batch, double* out, void* stream);
/* Sequence.step (interface/sequence.py:129-186) in every instance: action [dev] [n] in; obs [dev]
 * [n][dim], reward [dev] [n], end [dev] [n] and info [dev] [n][2] = {'action', 'step_action'}
 * (-1: None) out. */
COBEL_API int cobel_seq_step(const cobel_seq_t* seq, const int32_t* action, double* obs,
                             double* reward, uint8_t* end, int32_t* info, void* stream);
/* Sequence.reset (interface/sequence.py:188-204) in every instance: obs [dev] [n][dim] out. */
COBEL_API int cobel_seq_reset(const cobel_seq_t* seq, double* obs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * AssociativeNetwork (agent/anet.py:15-374, Donoso et al. 2021) on a Sequence: excitatory and
 * inhibitory weights [dim][n_actions - 1] with saturation, noisy outputs, an epsilon-greedy choice
 * among the n_actions - 1 outputs.  Everything is float64.
 *
 * Packing and summation order are cobel_rw_run's: an instance takes a group of G lanes, lane j
 * holds row j of both matrices; each of the 2 (n_actions - 1) dot products is the balanced tree
 * over G leaves w[j][a] * state[j].  q[a] = (state @ We - state @ Wi)[a] + noise * u[a], the u[a]
 * being n_actions - 1 consecutive double draws of COBEL_STREAM_AGENT at the instance's agent_ctr
 * (anet.py:325-333); the selection is one double draw of pol_stream at pol_ctr (policy/greedy.py:
 * 56-58, also where there is one output only). */
#define COBEL_ANET_MAX_ACTIONS 9   /* n_actions 2 .. 9: one to eight outputs */

typedef struct {
  double* We;                 /* [n][dim][n_actions - 1] weights['excitatory']                  */
  double* Wi;                 /* [n][dim][n_actions - 1] weights['inhibitory']                  */
  const double* sat_e;        /* [sat_rows][dim][n_actions - 1] saturation['excitatory']        */
  const double* sat_i;        /* ... ['inhibitory']                                             */
  const double* lr_e;         /* [lr_rows][dim][n_actions - 1] learning_rate['excitatory']      */
  const double* lr_i;         /* ... ['inhibitory']                                             */
  const double* eps;          /* [eps_rows] epsilon of the policy                               */
  uint32_t* pol_ctr;          /* [n] draws taken from the policy's stream so far                */
  uint32_t* agent_ctr;        /* [n] draws taken from COBEL_STREAM_AGENT so far                 */
  const uint32_t* instance_ids; /* [n] stream instance numbers, or NULL: instance_base + i      */
  int32_t* mid;               /* [n] 1: a trial is under way (step_budget ran out inside it)    */
  double* trew;               /* [n] its reward so far                                          */
  double* trial_reward;       /* [n][trial_cap] logs['trial_reward'] of every trial, or NULL    */
  int32_t* trial_steps;       /* [n][trial_cap] logs['steps'] (index of its last step), or NULL */
  int32_t* trial_action;      /* [n][trial_cap] logs['action'] (its last action), or NULL       */
  double* trace;              /* [n][trace_cap][3 + n_actions - 1] action, reward, end, q[0] ..
                                 of every step, or NULL                                         */
  int32_t* trace_len;         /* [n] rows of trace written so far (NULL iff trace is)           */
  unsigned long long* steps_done; /* env steps executed, added to; or NULL                      */
  int32_t n, n_actions;       /* n_actions: action_space.n of the agent (not the Sequence's)    */
  int32_t trial_cap, trace_cap, sat_rows, lr_rows, eps_rows;
  int32_t linear_update;      /* 1: delta.fill(1.0) (anet.py:354-355)                           */
  uint32_t instance_base, flags;  /* COBEL_F_LEARN: train (update_q after every step)           */
  uint32_t pol_stream, reserved_;
  int32_t trial_first;        /* row of the per-trial traces the session's first trial takes    */
  int32_t trials;             /* trials to run                                                  */
  int32_t steps_per_trial;    /* the cap of train(interface, trials, steps)                     */
  int32_t step_budget;        /* > 0: stop after that many steps (launch per step)              */
  double alpha;               /* anet.py:353                                                    */
  double noise;               /* noise_amplitude, anet.py:325                                   */
  uint64_t seed;
} cobel_anet_run_t;

/* Launch shape of cobel_anet_run for n instances of dim observation components: out = {lanes per
 * instance, instances per wavefront, instances per workgroup, workgroups}.  COBEL_E_UNSUPPORTED
 * beyond COBEL_RW_MAX_DIM components or outside 2 .. COBEL_ANET_MAX_ACTIONS actions.  (No line of the
 * reference corresponds: the launch shape is this library's.) */
COBEL_API int cobel_anet_plan(int32_t dim, int32_t n_actions, int32_t n, int32_t out[4]);
/* AssociativeNetwork.train / test (agent/anet.py:181-296) with Sequence.reset / step, retrieve_q
 * (:311-333), EpsilonGreedy.select_action and, under COBEL_F_LEARN, update_q (:335-356) inside:
 * `trials` trials in every instance in one launch.  A trial cut by steps_per_trial is replayed from
 * its first step.  The caller guarantees that no instance runs past its last trial. */
COBEL_API int cobel_anet_run(const cobel_seq_t* seq, const cobel_anet_run_t* run, void* stream);
/* AssociativeNetwork.retrieve_q / predict_on_batch (agent/anet.py:311-333, 358-374): out [dev]
 * [n][n_batch][n_actions - 1] for batch [dev] [n_batch][dim], the same rows for every instance.
 * Row b of instance i takes the draws agent_ctr[i] + b (n_actions - 1) + a of COBEL_STREAM_AGENT;
 * agent_ctr[i] advances by n_batch (n_actions - 1).  Of run: We, Wi, agent_ctr, instance_ids, n,
 * n_actions, instance_base, noise and seed are read. */
COBEL_API int cobel_anet_predict(const cobel_anet_run_t* run, int32_t dim, const double* batch,
                                 int32_t n_batch, double* out, void* stream);
/* AssociativeNetwork.update_q (agent/anet.py:335-356), one experience per instance: state [dev]
 * [n][dim], action [dev] [n] (outside 0 .. n_actions - 2: nothing changes, as the reference's
 * action_vector is all zero then), reward [dev] [n].  Of run: We, Wi, sat_*, lr_*, sat_rows,
 * lr_rows, n, n_actions, linear_update and alpha are read. */
COBEL_API int cobel_anet_update(const cobel_anet_run_t* run, int32_t dim, const double* state,
                                const int32_t* action, const double* reward, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ADQN (agent/adqn.py:18-279) and ADQNMemory (memory/adqn.py:29-198) on a Sequence: a network
 * predicts one value per observation, the value IS the action, every experience is kept, and every
 * step replays a batch drawn with recency-decayed prediction-error priorities.
 *
 * The memory of instance j is rows [j][0 .. count[j]) of caller-owned arrays of capacity `cap`; it
 * only ever grows.  One wavefront serves one instance.  The cumulative distribution of a draw is
 * formed in ONE fixed order: the count[j] entries are cut into 64
 * consecutive chunks of c = ceil(count / 64) entries, lane l holding [l c, min((l + 1) c, count));
 *   prob_sum = balanced tree (adjacent lanes first) over the lanes' sequential chunk sums of the
 *              priorities;
 *   p_i      = priority_i / prob_sum, or 1.0 / count each where prob_sum == 0;
 *   cdf_i    = (sum of the chunk totals of p of the lanes before, as a Hillis-Steele inclusive scan
 *               over the lanes hands it to the next lane) + (the sequential sum of p inside the
 *               chunk up to and including i);
 *   index    = min(#{i : cdf_i / cdf_last <= u}, count - 1)
 * for each of the `batch` draws u, draw b being the double at (counter draw_ctr[j], sub b) of
 * COBEL_STREAM_ADQN_MEMORY: what Generator.choice(n, p=probs, size=batch) consumes as ONE call.
 * Non-finite rewards or values are outside the contract: NumPy's choice raises on NaN
 * probabilities, these kernels do not look. */
#define COBEL_STREAM_ADQN_MEMORY 7u /* c = sample_batch calls, sub = position in the batch
                                       (memory/adqn.py:160)                                    */
#define COBEL_ADQN_RPE 1u           /* ADQNMemory.rpe: priority |error| instead of 1            */

typedef struct {
  double* states;             /* [n][cap][dim] ADQNMemory.states                                */
  double* reinforcements;     /* [n][cap]                                                       */
  double* errors;             /* [n][cap] action - reward                                       */
  double* priorities;         /* [n][cap]                                                       */
  int32_t* count;             /* [n] experiences held, <= cap                                   */
  uint32_t* draw_ctr;         /* [n] sample_batch calls so far (store: not read)                */
  const uint32_t* instance_ids; /* [n] stream instance numbers, or NULL: instance_base + i      */
  double* scratch;            /* [n][cap] the cdf of a draw (cobel_adqn_plan; store: not read)  */
  int32_t n, dim, cap;
  int32_t count_min, count_max; /* the host's bounds on count[]: they decide the refusals       */
  uint32_t instance_base, flags;  /* COBEL_ADQN_RPE                                             */
  uint32_t reserved_;
  double decay;               /* ADQNMemory.decay, 0 .. 1                                       */
  uint64_t seed;
} cobel_adqn_mem_t;

typedef struct {
  const void* value;          /* [n] the network's value of the current observation = the action,
                                 in the network's dtype (widened exactly, as float() does)      */
  int32_t* in_index;          /* [n][batch] out: row j cap + index of states viewed [n cap][dim] */
  void* targets;              /* [n][batch] out: reinforcements[index], network dtype           */
  int32_t* idx;               /* [n][batch] out: the drawn indices, or NULL                     */
  int32_t* ep_index;          /* [n] out: the observation-table row the instance sees next      */
  uint8_t* active;            /* [n] out: 1 = the instance stored (and drew) in this step       */
  uint8_t* alive;             /* [n] out: 1 = the instance has steps of this session left       */
  int32_t* done;              /* [n] trials finished in this session (the caller zeroes it)     */
  int32_t* mid;               /* [n] 1: a trial is under way                                    */
  double* trew;               /* [n] its reward so far                                          */
  double* trial_reward;       /* [n][trial_cap] logs['trial_reward'] of every trial, or NULL    */
  int32_t* trial_steps;       /* [n][trial_cap] logs['steps'] (index of its last step), or NULL */
  double* step_rec;           /* [n][4] value, reward, end_trial, terminal of this step, or NULL */
  double* trace;              /* [n][trace_cap][3] value, reward, end of every step, or NULL    */
  int32_t* idx_trace;         /* [n][trace_cap][batch] the drawn indices of every step, or NULL */
  int32_t* trace_len;         /* [n] rows of trace written so far (NULL iff trace is)           */
  unsigned long long* steps_done; /* env steps executed, added to; or NULL                      */
  int32_t n, batch, is_float64, trial_cap, trace_cap;
  uint32_t flags;             /* COBEL_F_LEARN: train (store and draw); 0: test                 */
  int32_t trial_first;        /* row of the per-trial traces the session's first trial takes    */
  int32_t trials;             /* trials of the session                                          */
  int32_t steps_per_trial;    /* the cap of train(interface, trials, steps)                     */
  int32_t reserved_;
} cobel_adqn_step_t;

/* Launch shape and scratch of the three entry points below for n instances of capacity cap: out =
 * {instances per workgroup, workgroups, bytes of cobel_adqn_mem_t.scratch, lanes per instance}.
 * COBEL_E_UNSUPPORTED beyond COBEL_RW_MAX_DIM components, COBEL_E_RANGE unless n cap < 2^31.  (No
 * line of the reference corresponds: the launch shape is this library's.) */
COBEL_API int cobel_adqn_plan(int32_t dim, int32_t n, int32_t cap, int64_t out[4]);
/* ADQNMemory.store (memory/adqn.py:119-138), k experiences per instance one after the other: states
 * [dev] [n][k][dim], actions [dev] [n][k], rewards [dev] [n][k].  Per experience: append state,
 * reward and action - reward; multiply every stored priority by decay (one rounded multiplication
 * per entry per store, the reference's repeated *=); append |error| ** int(rpe).  COBEL_E_RANGE if
 * count_max + k > cap; the kernel itself never writes past cap either. */
COBEL_API int cobel_adqn_store(const cobel_adqn_mem_t* mem, int32_t k, const double* states,
                               const double* actions, const double* rewards, void* stream);
/* ADQNMemory.sample_batch (memory/adqn.py:140-164): idx [dev] [n][batch] (or NULL), in_index [dev]
 * [n][batch] and targets [dev] [n][batch] (float64, or float32 with is_float64 == 0) as in
 * cobel_adqn_step_t; draw_ctr[j] += 1.  batch >= 1.  COBEL_E_RANGE if count_min == 0: an empty
 * memory has nothing to draw, the reference's choice raises. */
COBEL_API int cobel_adqn_sample(const cobel_adqn_mem_t* mem, int32_t batch, int32_t is_float64,
                                int32_t* idx, int32_t* in_index, void* targets, void* stream);
/* One lockstep step of ADQN.train / test (agent/adqn.py:128-156, :187-212) without the network: in
 * every instance with trials of the session left, Sequence.reset where a trial begins, Sequence.step
 * (interface/sequence.py:129-186; rewards one float per step, or array rewards under overwrite),
 * under COBEL_F_LEARN memory.store of (observation, value, reward) and the draw of
 * memory.sample_batch, then the trial bookkeeping and ep_index.  The caller then hands in_index,
 * targets, active and ep_index to cobel_mlp_fit nb_replays times (agent/adqn.py:234-236); its
 * ep_out is the next step's value.  COBEL_E_RANGE if a store could pass cap (count_max + 1 > cap). */
COBEL_API int cobel_adqn_step(const cobel_seq_t* seq, const cobel_adqn_mem_t* mem,
                              const cobel_adqn_step_t* run, void* stream);

/* ---------------------------------------------------------------------------------------------
 * QAgent (agent/q.py:26-354) on a Sequence, with a Softmax (policy/softmax.py:11-88) or an
 * EpsilonGreedy policy.  Everything is float64, every operation rounded by itself.
 *
 * Keys.  The reference keys Q by tuple(observation.flatten()): observation rows of equal values
 * share a Q row, and the zero observation a trial ends in (row 0 of obs_table) is a key too.  The
 * host deduplicates the rows of obs_table by value into key_of_row [n_obs]; the kernel sees key
 * indices only.  Q is [n][n_keys][n_actions].
 *
 * Log.  One 16-byte record per experience (QAgent.M): the reward and meta = state key |
 * next key << 8 | action << 16 | non-terminal << 24.  log_len[i] persists between launches.
 *
 * Draws.  The policy takes one double per selection from pol_stream at pol_ctr[i]; a replay takes
 * its batch_size indices as ONE integers(0, len(M), batch_size) of COBEL_STREAM_MEMORY at
 * mem_ctr[i] (element j from sub-stream j; the counter moves by one per learning step, at
 * batch_size 0 too, as TapeRNG.integers(size=0) does).
 *
 * Softmax selection (policy/softmax.py:77-86 and Generator.choice): e_a = exp((v_a - max v) beta),
 * p_a = e_a / (((e_0 + e_1) + e_2) + ...), the cumulative sums in the same order, action =
 * #{a < A - 1 : cum_a / cum_{A-1} <= u}.  Epsilon-greedy is cobel_eps_greedy_n_f64's.
 *
 * An instance takes a group of eight lanes, lane a holding the column of action a; its Q table
 * stays in LDS for the launch.
 * --------------------------------------------------------------------------------------------- */
#define COBEL_QSEQ_MAX_ACTIONS 8
#define COBEL_QSEQ_MAX_KEYS 64
#define COBEL_QSEQ_POLICY_SOFTMAX 0     /* par[.][2] is beta                                      */
#define COBEL_QSEQ_POLICY_EPS_GREEDY 1  /* par[.][2] is epsilon                                   */
#define COBEL_QSEQ_ROW 6  /* doubles of a trace row: state key, action, reward, next key,
                             non-terminal, td (0 without COBEL_F_LEARN; the td of the last update
                             of the step's own experience, a replay in its batch included)        */

typedef struct {
  double reward;
  uint32_t meta;              /* state key | next key << 8 | action << 16 | non-terminal << 24  */
  uint32_t reserved_;
} cobel_qseq_rec_t;

typedef struct {
  double* Q;                  /* [n][n_keys][n_actions]                                         */
  const int32_t* key_of_row;  /* [seq->n_obs] key of every row of obs_table                     */
  const double* par;          /* [par_rows][4] learning rate, gamma, beta or epsilon, unused    */
  uint32_t* pol_ctr;          /* [n] draws taken from the policy's stream so far                */
  uint32_t* mem_ctr;          /* [n] replay() calls so far (COBEL_STREAM_MEMORY); NULL allowed
                                 without COBEL_F_LEARN                                          */
  cobel_qseq_rec_t* log;      /* [n][log_cap]; NULL allowed without COBEL_F_LEARN               */
  int32_t* log_len;           /* [n] records of the log; NULL iff log is                        */
  const uint32_t* instance_ids; /* [n] stream instance numbers, or NULL: instance_base + i      */
  int32_t* mid;               /* [n] 1: a trial is under way (step_budget ran out inside it)    */
  double* trew;               /* [n] its reward so far                                          */
  double* trial_reward;       /* [n][trial_cap] logs['trial_reward'] of every trial, or NULL    */
  int32_t* trial_steps;       /* [n][trial_cap] logs['steps'] (index of its last step), or NULL */
  int32_t* trial_action;      /* [n][trial_cap] its last action, or NULL                        */
  double* trace;              /* [n][trace_cap][COBEL_QSEQ_ROW] every step, or NULL             */
  int32_t* trace_len;         /* [n] rows of trace written so far (NULL iff trace is)           */
  double* last;               /* [n][COBEL_QSEQ_ROW] the row of the launch's last step, or NULL */
  unsigned long long* steps_done; /* env steps executed, added to; or NULL                      */
  int32_t n, n_keys, n_actions, log_cap, trial_cap, trace_cap, par_rows, policy;
  int32_t batch_size, reserved_;
  uint32_t instance_base, flags;  /* COBEL_F_LEARN: train (update, log and replay)              */
  uint32_t pol_stream, reserved2_;
  int32_t trial_first;        /* row of the per-trial traces the session's first trial takes    */
  int32_t trials;             /* trials to run                                                  */
  int32_t steps_per_trial;    /* the cap of train(interface, trials, steps)                     */
  int32_t step_budget;        /* > 0: stop after that many steps (launch per step)              */
  uint64_t seed;
} cobel_qseq_run_t;

/* Launch shape of cobel_qseq_run: out = {lanes per instance, instances per wavefront, instances
 * per workgroup, workgroups}.  COBEL_E_UNSUPPORTED outside 1 .. COBEL_QSEQ_MAX_ACTIONS actions or
 * 1 .. COBEL_QSEQ_MAX_KEYS keys. */
COBEL_API int cobel_qseq_plan(int32_t n_keys, int32_t n_actions, int32_t n, int32_t out[4]);
/* QAgent.train (agent/q.py:160-228; COBEL_F_LEARN) or QAgent.test (:230-287) with Sequence.reset /
 * step and the policy's select_action inside, `trials` trials in every instance in one launch.  Per
 * step: select from Q[key(state)]; the Sequence step (under overwrite the forced action picks the
 * reward, the experience keeps the agent's); append the experience (q.py:213); update_q
 * (:304-313); replay(batch_size) (:344-354), the updates one after the other.  A trial cut by
 * steps_per_trial is replayed from its first step.  The caller guarantees that no instance runs
 * past its last trial and that the log has room (a full log takes no record).
 * COBEL_E_UNSUPPORTED outside the limits above, before any launch. */
COBEL_API int cobel_qseq_run(const cobel_seq_t* seq, const cobel_qseq_run_t* run, void* stream);
/* Softmax.get_action_probs / select_action on N rows of n_actions float64 values with injected
 * uniforms, in the arithmetic of cobel_qseq_run: values [dev] [N][n_actions], mask [dev] [N] bytes
 * (bit a: action a allowed) or NULL, u [dev] [N], beta [dev] [beta_rows] (beta_rows 1 or N),
 * action_out [dev] [N] or NULL, probs_out [dev] [N][n_actions] or NULL. */
COBEL_API int cobel_softmax_n(const double* values, const uint8_t* mask, const double* u,
                              const double* beta, int32_t beta_rows, uint8_t* action_out,
                              double* probs_out, int32_t n, int32_t n_actions, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The continuous 2D arena (interface/continuous.py:21-438): a "step" robot that moves in the four
 * cardinal directions or a differential-wheel robot, inside one exterior ring with hole rings
 * (room, obstacles).  Everything is float64, every operation rounded by itself.
 *
 * The arena is a table of directed edges a -> b with the interior to the left (exterior
 * counter-clockwise, holes clockwise), eight columns of n_edges doubles computed on the host:
 * ax, ay, bx, by, ex = bx - ax, ey = by - ay, nx = -ey / L, ny = ex / L (L = sqrt(ex ex + ey ey)).
 * With m = |buffer|:
 *   inside(p)  even-odd rule: an edge toggles when (ay > py) != (by > py) and
 *              px < ax + (py - ay) / (by - ay) * ex
 *   clear(p)   inside(p), and every edge is at least m / 2 away (squared distance to the point at
 *              s = ((px - ax) ex + (py - ay) ey) / (ex ex + ey ey) clamped to [0, 1])
 *   move(p, target), d = target - p: among the edges with den = dx nx + dy ny < 0,
 *              t = ((px - ax) nx + (py - ay) ny) / (-den) in [0, 1] and the hit point h = p + t d at
 *              u = ((hx - ax) ex + (hy - ay) ey) / (ex ex + ey ey) in [-1e-9, 1 + 1e-9], take the
 *              least t (the lowest edge on ties): the robot ends at h + m n of that edge, at the
 *              target itself (bit for bit) with no hit, and stays at p where that point is not
 *              clear.  wall_hit: the end differs from the target.
 * This replaces shapely's polygon / line-string intersection and buffered-polygon projection
 * (continuous.py:311-329): the robot lands m inside the wall instead of on it.
 *
 * An instance takes G = 1, 4, 16 or 64 lanes, which split the edges; the results are the same bits
 * for every G. */
#define COBEL_C2D_MAX_EDGES 1024
#define COBEL_C2D_MAX_REWARDS 32
#define COBEL_C2D_STEP 0   /* 4 actions: -x, +y, +x, -y by step_size (continuous.py:211-219)   */
#define COBEL_C2D_WHEEL 1  /* 3 actions: turn on either wheel, straight (continuous.py:220-251) */

typedef struct {
  const double* edges;        /* [dev] [8][n_edges] the arena                                    */
  const double* spawn_edges;  /* [dev] [8][n_spawn_edges] the rings of the spawn area            */
  const double* rewards;      /* [dev] [n_rewards][3] x, y, magnitude; NULL with none            */
  double* state;              /* [dev] [n][3] x, y, orientation                                  */
  uint32_t* env_ctr;          /* [dev] [n] next index on COBEL_STREAM_ENV (kept even)            */
  double box[4];              /* lo_x, lo_y, hi_x, hi_y of the candidates of a reset             */
  double fallback[2];         /* the start where 1 024 candidates were all refused               */
  double step_size, body_radius, wheel_distance, buffer;
  uint64_t seed;
  int32_t n, n_edges, n_spawn_edges, n_rewards;
  int32_t robot_type;         /* COBEL_C2D_STEP / COBEL_C2D_WHEEL                                */
  int32_t punish_wall;        /* reward -10 for a step that hit a wall                           */
  int32_t lanes_per_instance; /* 0: the planner's choice; 1, 4, 16, 64                           */
  uint32_t instance_base;
} cobel_c2d_t;

/* Launch shape for n instances in an arena of n_edges edges: out = {lanes per instance, lanes per
 * workgroup, bytes of LDS per workgroup, workgroups}.  The largest G of 1, 4, 16, 64 within the
 * lane budget (n G <= 262 144 for G = 4 and 16, <= 65 536 for G = 64; docs/MEASUREMENTS.md §19)
 * and with G <= the next power of two >= n_edges.  COBEL_E_RANGE outside 1 .. COBEL_C2D_MAX_EDGES
 * edges. */
COBEL_API int cobel_c2d_plan(int32_t n, int32_t n_edges, int32_t out[4]);
/* Continuous2D.step (continuous.py:185-266, clip_movement :295-329) in every instance: action
 * [dev] [n] in; the state is updated in place; reward [dev] [n], done [dev] [n] (end_trial) and
 * wall [dev] [n] (wall_hit) out.  The first reward row within 2 body_radius pays and ends the
 * trial; else -10 for a wall hit under punish_wall.  An action the robot does not have leaves the
 * instance where it is: reward 0, not done, no wall hit.  COBEL_E_ARG / COBEL_E_RANGE for a
 * malformed arena, before any HIP call. */
COBEL_API int cobel_c2d_step(const cobel_c2d_t* c2d, const uint8_t* action, double* reward,
                             uint8_t* done, uint8_t* wall, void* stream);
/* Continuous2D.reset (continuous.py:268-293) in every instance whose mask byte is set (mask NULL:
 * all): candidate k = box.lo + (box.hi - box.lo) * (draws c + 2k, c + 2k + 1 of COBEL_STREAM_ENV,
 * c = env_ctr[i]); the first of k = 0 .. 1023 inside the spawn rings and clear in the arena is the
 * start, the orientation 2 pi times draw c + 2k + 2 (0 for the step robot, the draw is consumed),
 * env_ctr += 2k + 4.  Where none is accepted: the fallback point, the draw c + 2048,
 * env_ctr += 2052 and *fallbacks += 1.  This bounds the reference's `while` loop (:282-283). */
COBEL_API int cobel_c2d_reset(const cobel_c2d_t* c2d, const uint8_t* mask, int32_t* fallbacks,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * cobel_dqn_act on the arena: everything of one lockstep DQN training step that is not the
 * network, for the agent the reference runs on Continuous2D (demo/continuous/demo_2d.py,
 * agent/dqn.py:170-212).  Per instance, in this order:
 *   epsilon-greedy on q (policy/greedy.py:40-88; four actions for the step robot, three for the
 *     wheel robot), one double of the policy stream
 *   Continuous2D.step (continuous.py:185-266), exactly cobel_c2d_step
 *   append (observation, action, reward, observation after the step and BEFORE any reset,
 *     1 - end_trial) to the replay ring in the network's dtype (memory/dqn.py:103-119); the
 *     observation is (x, y) for the step robot and (x, y, orientation) for the wheel robot
 *   trial bookkeeping and monitors (agent/dqn.py:186-212, monitor/behavior.py:82)
 *   where the trial is over and the instance goes on: Continuous2D.reset (continuous.py:268-293),
 *     exactly cobel_c2d_reset with a mask of that instance, env_ctr advanced as it advances it
 *   obs = the observation the next selection looks at
 *   the replay batch (memory/dqn.py:137), sub-streams 0 .. batch - 1 of one memory counter
 * — the same streams, counters and order as cobel_rng_uniform + cobel_eps_greedy[_n][_f64],
 * cobel_c2d_step, cobel_c2d_reset and cobel_rng_bounded_each, bit for bit, for every lane count.
 * An instance whose `active` flag is 0 consumes no draw, has nothing of its own written and gets
 * stepped = 0.  The fields shared with cobel_dqn_act_t carry its names and meanings.  arena.n,
 * arena.seed and arena.instance_base count for the policy and memory streams as well; the scalar
 * fields of the arena are read at the call (a recorded launch keeps them).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  cobel_c2d_t arena;        /* state [n][3] and env_ctr [n] in/out                              */
  /* policy */
  const void* q;            /* [n][A] Q-values of the current observations, network dtype; A = 4
                               (step robot) or 3 (wheel robot)                                  */
  uint32_t* policy_ctr;     /* [n] next index on the policy stream                              */
  uint32_t policy_stream;   /* COBEL_STREAM_POLICY or COBEL_STREAM_POLICY_TEST                  */
  int32_t is_float64;       /* dtype of q and of the ring's floating-point arrays               */
  double epsilon;
  /* replay ring, [n][slots][..]; observations of n_obs = 2 (step robot) or 3 numbers            */
  void* ring_states;
  void* ring_next_states;
  int64_t* ring_actions;
  void* ring_rewards;
  void* ring_nonterminal;
  int32_t* ring_size;
  int64_t* ring_head;
  uint32_t* memory_ctr;
  /* trial bookkeeping */
  int32_t* trial;
  int32_t* step;
  double* trial_reward;
  uint8_t* active;
  double* adam_steps;       /* or NULL                                                          */
  long long* lat_sum;       /* [mon_stripes][trial_cap], or NULL                                */
  long long* lat_cnt;
  double* reward_sum;
  /* outputs */
  uint8_t* stepped;         /* [n]                                                              */
  int32_t* batch_slots;     /* [n][batch], or NULL: no batch is drawn                           */
  double* obs;              /* [n][n_obs] float64: after the step and after any reset           */
  double* reward_out;       /* [n] what cobel_c2d_step would have written, or NULL              */
  uint8_t* done_out;        /* [n] or NULL                                                      */
  uint8_t* wall_out;        /* [n] or NULL                                                      */
  int32_t* fallbacks;       /* the counter cobel_c2d_reset adds into                            */
  /* sizes and parameters */
  int32_t slots, batch;
  int32_t steps_per_trial, trials_target, trial_cap, mon_stripes;
} cobel_dqn_c2d_act_t;
COBEL_API int cobel_dqn_act_c2d(const cobel_dqn_c2d_act_t* run, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COBEL_HIP_H */
