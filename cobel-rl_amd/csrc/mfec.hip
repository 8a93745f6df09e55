// Model-Free Episodic Control (agent/mfec.py of the reference): the per-action episodic memories,
// the k-nearest-neighbour value lookup and the trial loops, one wavefront per instance, the whole
// session in one launch.
//
// The buffers hold node ids; what the reference's KDTree computes from D-long vectors comes from two
// S x S tables built once per world (k_mfec_pairs): the reduced distance and find_state's allclose
// bit.  A query walks the buffer in index order, 64 entries at a time: the lanes gather their
// distances from the table row of the queried node, a ballot finds the entries that beat the heap's
// root, and lane 0 pushes those — in index order, re-testing each against the root as it stands —
// onto the max-heap of sklearn/utils/_heap.pyx kept in LDS.  Pushing only those is exact: heap_push
// starts by rejecting val >= root and the root never grows.  Lane 0 then runs simultaneous_sort
// (sklearn/utils/_sorting.pyx, an unstable quicksort) and sums the values in the order it leaves:
// the order among equidistant entries — duplicates of a buffer's first node are normal, see
// QEC.update's `if state_index:` — is the tree's, and with it the last bit of the float64 sum.
//
// Buffers live in global memory and are written by lane 0 (the episode write-back is sequential
// by definition); gsync() makes those writes visible to the gathers of the other lanes.
#include "cobel_common.h"
#include "cobel_policy.h"

namespace {

constexpr int kMaxA = COBEL_MFEC_MAX_ACTIONS;
constexpr int kMaxK = COBEL_MFEC_MAX_K;
constexpr double kRtol = 1e-04, kAtol = 1e-06;   // agent/mfec.py:76

struct mfec_lds {
  double hv[kMaxK];      // the heap's distances
  int hi[kMaxK];         // ... and buffer indices
  int stack[2 * kMaxK];  // simultaneous_sort's pending (offset, size) pairs
  int len[kMaxA];
  double result;
};

// Orders lane 0's global stores before the other lanes' loads (one wavefront per workgroup).
__device__ __forceinline__ void gsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// sklearn/utils/_heap.pyx: heap_push (one lane).
__device__ __forceinline__ void heap_push(double* values, int* indices, int size, double val,
                                          int val_idx) {
  if (val >= values[0]) return;
  values[0] = val;
  indices[0] = val_idx;
  int cur = 0;
  while (true) {
    const int left = 2 * cur + 1, right = left + 1;
    int swap;
    if (left >= size) {
      break;
    } else if (right >= size) {
      if (values[left] > val) swap = left; else break;
    } else if (values[left] >= values[right]) {
      if (val < values[left]) swap = left; else break;
    } else {
      if (val < values[right]) swap = right; else break;
    }
    values[cur] = values[swap];
    indices[cur] = indices[swap];
    cur = swap;
  }
  values[cur] = val;
  indices[cur] = val_idx;
}

__device__ __forceinline__ void dual_swap(double* v, int* x, int a, int b) {
  const double d = v[a];
  v[a] = v[b];
  v[b] = d;
  const int t = x[a];
  x[a] = x[b];
  x[b] = t;
}

// sklearn/utils/_sorting.pyx: simultaneous_sort (one lane); the two recursive calls work on
// disjoint parts, so they are taken from a stack in any order.
__device__ __forceinline__ void simultaneous_sort(double* values, int* indices, int size,
                                                  int* stack) {
  int top = 0;
  stack[0] = 0;
  stack[1] = size;
  top = 1;
  while (top > 0) {
    --top;
    double* v = values + stack[2 * top];
    int* x = indices + stack[2 * top];
    const int base = stack[2 * top];
    const int n = stack[2 * top + 1];
    if (n <= 1) {
    } else if (n == 2) {
      if (v[0] > v[1]) dual_swap(v, x, 0, 1);
    } else if (n == 3) {
      if (v[0] > v[1]) dual_swap(v, x, 0, 1);
      if (v[1] > v[2]) {
        dual_swap(v, x, 1, 2);
        if (v[0] > v[1]) dual_swap(v, x, 0, 1);
      }
    } else {
      int pivot = n / 2;
      if (v[0] > v[n - 1]) dual_swap(v, x, 0, n - 1);
      if (v[n - 1] > v[pivot]) {
        dual_swap(v, x, n - 1, pivot);
        if (v[0] > v[n - 1]) dual_swap(v, x, 0, n - 1);
      }
      const double pivot_val = v[n - 1];
      int store = 0;
      for (int i = 0; i < n - 1; ++i) {
        if (v[i] < pivot_val) {
          dual_swap(v, x, i, store);
          ++store;
        }
      }
      dual_swap(v, x, store, n - 1);
      pivot = store;
      if (pivot > 1) {
        stack[2 * top] = base;
        stack[2 * top + 1] = pivot;
        ++top;
      }
      if (pivot + 2 < n) {
        stack[2 * top] = base + pivot + 1;
        stack[2 * top + 1] = n - pivot - 1;
        ++top;
      }
    }
  }
}

// KDTree.query(k=1) on a single leaf: the lowest index among the smallest distances (n >= 1).
__device__ __forceinline__ int nearest(const double* __restrict__ drow, const int32_t* ids, int n,
                                       int S, int lane) {
  double bd = __builtin_huge_val();
  int bi = 0x7fffffff;
  for (int j = lane; j < n; j += 64) {
    int id = ids[j];
    id = (unsigned)id < (unsigned)S ? id : S - 1;
    const double d = drow[id];
    if (d < bd) {
      bd = d;
      bi = j;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double od = __shfl_xor(bd, o);
    const int oi = __shfl_xor(bi, o);
    if (od < bd || (od == bd && oi < bi)) {
      bd = od;
      bi = oi;
    }
  }
  return bi < n ? bi : 0;   // (no finite distance: still an entry of the buffer)
}

// First minimum of the time stamps (np.argmin, agent/mfec.py:119; n >= 1).
__device__ __forceinline__ int oldest(const int32_t* times, int n, int lane) {
  int bt = 0x7fffffff, bi = 0x7fffffff;
  for (int j = lane; j < n; j += 64) {
    const int t = times[j];
    if (t < bt) {
      bt = t;
      bi = j;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int ot = __shfl_xor(bt, o);
    const int oi = __shfl_xor(bi, o);
    if (ot < bt || (ot == bt && oi < bi)) {
      bt = ot;
      bi = oi;
    }
  }
  return bi < n ? bi : 0;
}

// ActionBuffer.find_state (agent/mfec.py:60-79): index of the hit, or -1.
__device__ __forceinline__ int find_state(const cobel_mfec_mem_t& m, const int32_t* ids, int n,
                                          int s, int lane) {
  if (n <= 0) return -1;
  const int S = m.n_states;
  const int bi = nearest(m.rdist + (size_t)s * S, ids, n, S, lane);
  int id = ids[bi];
  id = (unsigned)id < (unsigned)S ? id : S - 1;
  return m.same[(size_t)s * S + id] ? bi : -1;
}

// QEC.estimate (agent/mfec.py:173-200) of node s on one buffer; wave-uniform.
__device__ __forceinline__ double estimate(const cobel_mfec_mem_t& m, mfec_lds* l,
                                           const int32_t* ids, const double* values, int n, int s,
                                           int lane) {
  const int hit = find_state(m, ids, n, s, lane);
  if (hit >= 0) return values[hit];
  const int k = m.k;
  if (n <= k) return 0.0;
  const int S = m.n_states;
  const double* const drow = m.rdist + (size_t)s * S;
  if (lane < k) {
    l->hv[lane] = __builtin_huge_val();
    l->hi[lane] = 0;
  }
  wsync();
  for (int base = 0; base < n; base += 64) {
    const int j = base + lane;
    double d = __builtin_huge_val();
    if (j < n) {
      int id = ids[j];
      id = (unsigned)id < (unsigned)S ? id : S - 1;
      d = drow[id];
    }
    unsigned long long todo = __ballot(d < l->hv[0]);
    while (todo) {
      const int b = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const double db = __shfl(d, b);
      if (lane == 0) heap_push(l->hv, l->hi, k, db, base + b);
      wsync();
    }
  }
  if (lane == 0) {
    simultaneous_sort(l->hv, l->hi, k, l->stack);
    double value = 0.0;
    for (int t = 0; t < k; ++t) value += values[l->hi[t]];
    l->result = value / (double)k;
  }
  wsync();
  const double out = l->result;
  wsync();
  return out;
}

struct mfec_run_args {
  cobel_mfec_mem_t m;
  cobel_mfec_run_t r;
  const cobel_wrec* rec;
  const uint16_t* next_n;
  const float* reward_s;
  const uint8_t* terminal_s;
  const uint16_t* starts;
  const int32_t* start_off;
  const uint32_t* succ_off;
  const uint16_t* succ_state;
  const double* succ_cdf;
};

__global__ __launch_bounds__(64) void k_mfec_run(const mfec_run_args G) {
  __shared__ mfec_lds l;
  const int lane = (int)threadIdx.x;
  const int i = (int)blockIdx.x;
  const cobel_mfec_mem_t& m = G.m;
  const cobel_mfec_run_t& R = G.r;
  const int S = m.n_states, A = m.n_actions, cap = m.capacity;
  const bool learn = R.flags & COBEL_F_LEARN;
  const uint32_t act_stream =
      (R.flags & COBEL_F_TEST_STREAM) ? COBEL_STREAM_POLICY_TEST : COBEL_STREAM_POLICY;
  const uint32_t g = R.instance_base + (uint32_t)i;
  int32_t* const inst = R.inst + (size_t)i * COBEL_I_WORDS;
  int32_t* const ids = m.ids + (size_t)i * A * cap;
  double* const values = m.values + (size_t)i * A * cap;
  int32_t* const times = m.times + (size_t)i * A * cap;
  int32_t* const ep_sa = R.ep_sa + (size_t)i * R.steps_per_trial;
  double* const ep_value = R.ep_value + (size_t)i * R.steps_per_trial;
  if (lane < A) {
    int n = m.len[(size_t)i * A + lane];
    l.len[lane] = n < 0 ? 0 : (n > cap ? cap : n);
  }
  wsync();
  uint32_t ce = (uint32_t)inst[COBEL_I_CTR_ENV];
  uint32_t cp = (uint32_t)inst[COBEL_I_CTR_POLICY];
  int trial = inst[COBEL_I_TRIAL];
  int state = inst[COBEL_I_STATE];
  int step = inst[COBEL_I_STEP];
  bool mid = inst[COBEL_I_FLAGS] & 1;
  double trew = mid ? *reinterpret_cast<const double*>(inst + COBEL_I_REWARD_LO) : 0.0;
  int clock = m.clock[i];
  long long budget = R.step_budget > 0 ? (long long)R.step_budget : 0x7fffffffffffffffll;
  unsigned long long executed = 0;
  const int start_lo = G.start_off[0];
  const uint32_t start_cnt = (uint32_t)(G.start_off[1] - start_lo);
  if (state < 0 || state >= S) state = 0;
  if (step < 0 || step >= R.steps_per_trial) {
    step = 0;
    mid = false;
  }

  while (trial < R.trials_target && budget > 0) {
    if (!mid) {   // reset (interface/topology.py:159-172)
      state = (int)G.starts[start_lo + (int)cobel_draw_bounded(ce, 0u, g, COBEL_STREAM_ENV, R.seed,
                                                               start_cnt)];
      ce += 1u;
      if (state >= S) state = S - 1;
      step = 0;
      trew = 0.0;
      mid = true;
    }
    bool done = false;
    int latency = 0;
    while (step < R.steps_per_trial && budget > 0) {
      // retrieve_q (agent/mfec.py:405-421)
      double q[kMaxA];
#pragma unroll
      for (int a = 0; a < kMaxA; ++a) {
        q[a] = 0.0;
        if (a < A)
          q[a] = estimate(m, &l, ids + (size_t)a * cap, values + (size_t)a * cap, l.len[a], state,
                          lane);
      }
      const double u = cobel_draw_u01(cp, 0u, g, act_stream, R.seed);
      cp += 1u;
      const int a = cobel_eps_greedy_select_n<double, kMaxA>(q, A, 0xffffffffu, u, R.epsilon,
                                                             nullptr);
      int ns;
      if (G.succ_off) {
        const double ue = cobel_draw_u01(ce, COBEL_SUB_DOUBLE, g, COBEL_STREAM_ENV, R.seed);
        ce += 1u;
        ns = cobel_draw_successor(G.succ_off, G.succ_state, G.succ_cdf, (size_t)state * A + a, ue);
      } else {
        ns = G.rec ? (int)G.rec[state].next[a] : (int)G.next_n[(size_t)state * A + a];
      }
      if (ns >= S) ns = S - 1;
      const double r = (double)(G.rec ? G.rec[ns].reward : G.reward_s[ns]);
      const uint32_t end = G.rec ? G.rec[ns].terminal : (uint32_t)G.terminal_s[ns];
      if (lane == 0) {
        if (learn) {   // the episode row (agent/mfec.py:458-466)
          ep_sa[step] = state | (a << 16);
          ep_value[step] = r;
        }
        if (R.last_exp) {
          int32_t* const e = R.last_exp + (size_t)i * 6;
          e[0] = state;
          e[1] = a;
          e[2] = ns;
          e[3] = end ? 0 : 1;
          e[4] = (int32_t)fbits((float)r);
          e[5] = 0;
        }
        if (R.trace) {
          const int row = R.trace_len[i];
          if (row < R.trace_cap) {
            double* const t = R.trace + ((size_t)i * R.trace_cap + row) * (size_t)(4 + A);
            t[0] = (double)state;
            t[1] = (double)a;
            t[2] = r;
            t[3] = end ? 1.0 : 0.0;
            for (int b = 0; b < A; ++b) t[4 + b] = q[b];
            R.trace_len[i] = row + 1;
          }
        }
        if (R.occupancy) atomicAdd(R.occupancy + ns, 1ull);
      }
      if (learn) clock += 1;
      trew += r;
      executed += 1ull;
      budget -= 1;
      state = ns;
      if (end) {
        if (learn) {
          const int nev = step + 1;
          // the returns, backward through the episode (agent/mfec.py:472-476)
          if (lane == 0) {
            double ret = 0.0;
            for (int e = nev - 1; e >= 0; --e) {
              ret = R.gamma * ret + ep_value[e];
              ep_value[e] = ret;
            }
          }
          gsync();
          // QEC.update_episode (agent/mfec.py:202-236), event by event
          for (int e = 0; e < nev; ++e) {
            const int sa = ep_sa[e];
            int es = sa & 0xffff, ea = sa >> 16;
            es = es < S ? es : S - 1;
            ea = ea < A ? ea : A - 1;
            const double ev = ep_value[e];
            const int et = clock - (nev - 1 - e);
            int32_t* const bi = ids + (size_t)ea * cap;
            double* const bv = values + (size_t)ea * cap;
            int32_t* const bt = times + (size_t)ea * cap;
            const int n = l.len[ea];
            const int hit = find_state(m, bi, n, es, lane);
            if (hit > 0) {   // `if state_index:` — a hit at index 0 counts as a miss
              if (lane == 0) {
                const double old = bv[hit];
                bv[hit] = old > ev ? old : ev;      // max(buffer.values[i], value)
                const int ot = bt[hit];
                bt[hit] = ot > et ? ot : et;
                bi[hit] = es;
              }
            } else if (n < cap) {   // ActionBuffer.add (agent/mfec.py:101-122)
              if (lane == 0) {
                bi[n] = es;
                bv[n] = ev;
                bt[n] = et;
                l.len[ea] = n + 1;
              }
            } else if (n > 0) {
              const int old = oldest(bt, n, lane);
              if (lane == 0 && et > bt[old]) {
                bi[old] = es;
                bv[old] = ev;
                bt[old] = et;
              }
            }
            gsync();
          }
        }
        done = true;
        latency = step;
        break;
      }
      ++step;
    }
    if (!done && step >= R.steps_per_trial) {   // timed out: the memory stays as it was
      done = true;
      latency = R.steps_per_trial - 1;
    }
    if (!done) break;   // the step budget ran out inside the trial
    if (lane == 0 && trial >= 0 && trial < R.trial_cap) {
      const size_t mo = cobel_mon_offset(R.mon_stripes, R.trial_cap) + (size_t)trial;
      if (R.lat_sum) atomicAdd(R.lat_sum + mo, (unsigned long long)latency);
      if (R.lat_cnt) atomicAdd(R.lat_cnt + mo, 1ull);
      if (R.reward_sum) atomicAdd(R.reward_sum + mo, trew);
      if (R.resp_cnt && trew > 0.0) atomicAdd(R.resp_cnt + mo, 1ull);
      if (R.lat_trace) R.lat_trace[(size_t)i * R.trial_cap + trial] = latency;
    }
    step = latency;
    trial += 1;
    mid = false;
  }
  wsync();
  if (lane < A) m.len[(size_t)i * A + lane] = l.len[lane];
  if (lane == 0) {
    inst[COBEL_I_STATE] = state;
    inst[COBEL_I_STEP] = step;
    inst[COBEL_I_TRIAL] = trial;
    inst[COBEL_I_CTR_ENV] = (int32_t)ce;
    inst[COBEL_I_CTR_POLICY] = (int32_t)cp;
    inst[COBEL_I_FLAGS] = mid ? 1 : 0;
    *reinterpret_cast<double*>(inst + COBEL_I_REWARD_LO) = trew;
    *reinterpret_cast<unsigned long long*>(inst + COBEL_I_STEPS_LO) += executed;
    if (R.steps_done && executed) atomicAdd(R.steps_done, executed);
    m.clock[i] = clock;
  }
}

// predict_on_batch: one wavefront per (instance, node)
__global__ __launch_bounds__(64) void k_mfec_estimate(const cobel_mfec_mem_t m,
                                                      const int32_t* __restrict__ nodes, int B,
                                                      double* __restrict__ out) {
  __shared__ mfec_lds l;
  const int lane = (int)threadIdx.x;
  const int i = (int)(blockIdx.x / (unsigned)B), b = (int)(blockIdx.x % (unsigned)B);
  const int A = m.n_actions, cap = m.capacity;
  int s = nodes[b];
  s = s < 0 ? 0 : (s >= m.n_states ? m.n_states - 1 : s);
  for (int a = 0; a < A; ++a) {
    int n = m.len[(size_t)i * A + a];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const size_t off = ((size_t)i * A + a) * cap;
    const double q = estimate(m, &l, m.ids + off, m.values + off, n, s, lane);
    if (lane == 0) out[((size_t)i * B + b) * A + a] = q;
  }
}

// The pair tables: one thread per (query q, stored j).
__global__ __launch_bounds__(256) void k_mfec_pairs(const double* __restrict__ F, int S, int D,
                                                    double* __restrict__ rdist,
                                                    uint8_t* __restrict__ same) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)S * S) return;
  const int q = (int)(p / (size_t)S), j = (int)(p % (size_t)S);
  const double* const x = F + (size_t)q * D;
  const double* const y = F + (size_t)j * D;
  double acc = 0.0;
  bool close = true;
  for (int d = 0; d < D; ++d) {
    // euclidean_rdist: tmp = x1[d] - x2[d]; d += tmp * tmp   (-ffp-contract=off: no fma)
    const double t = x[d] - y[d];
    acc = acc + t * t;
    // np.allclose(stored, query): |stored - query| <= atol + rtol * |query|
    close = close && (fabs(y[d] - x[d]) <= kAtol + kRtol * fabs(x[d]));
  }
  rdist[p] = acc;
  same[p] = close ? 1 : 0;
}

int check_mem(const cobel_mfec_mem_t* m, const char* who) {
  COBEL_REQUIRE(m, COBEL_E_ARG, "%s: NULL mem", who);
  COBEL_REQUIRE(m->n_states >= 1 && m->n_states <= COBEL_MFEC_MAX_STATES, COBEL_E_UNSUPPORTED,
                "%s: %d states (MFEC serves up to %d states)", who, m->n_states,
                COBEL_MFEC_MAX_STATES);
  COBEL_REQUIRE(m->n_actions >= 1 && m->n_actions <= COBEL_MFEC_MAX_ACTIONS, COBEL_E_UNSUPPORTED,
                "%s: %d actions (MFEC serves 1 to %d actions)", who, m->n_actions,
                COBEL_MFEC_MAX_ACTIONS);
  COBEL_REQUIRE(m->capacity >= 1 && m->capacity <= COBEL_MFEC_MAX_CAPACITY, COBEL_E_UNSUPPORTED,
                "%s: capacity %d (MFEC serves a capacity of 1 to %d)", who, m->capacity,
                COBEL_MFEC_MAX_CAPACITY);
  COBEL_REQUIRE(m->k >= 1 && m->k <= COBEL_MFEC_MAX_K, COBEL_E_UNSUPPORTED,
                "%s: k = %d (MFEC serves k of 1 to %d)", who, m->k, COBEL_MFEC_MAX_K);
  COBEL_REQUIRE(m->n >= 0, COBEL_E_RANGE, "%s: n = %d", who, m->n);
  COBEL_REQUIRE(m->rdist && m->same && m->ids && m->values && m->times && m->len && m->clock,
                COBEL_E_ARG, "%s: NULL table", who);
  COBEL_REQUIRE((((uintptr_t)m->rdist | (uintptr_t)m->values) & 7u) == 0 &&
                    (((uintptr_t)m->ids | (uintptr_t)m->times | (uintptr_t)m->len |
                      (uintptr_t)m->clock) & 3u) == 0,
                COBEL_E_ARG, "%s: misaligned table", who);
  return COBEL_OK;
}

}  // namespace

extern "C" int cobel_mfec_pairs(const double* features, int32_t n_states, int32_t n_features,
                                double* rdist, uint8_t* same, void* stream) {
  COBEL_REQUIRE(features && rdist && same, COBEL_E_ARG, "cobel_mfec_pairs: NULL argument");
  COBEL_REQUIRE(n_states >= 1 && n_states <= COBEL_MFEC_MAX_STATES, COBEL_E_UNSUPPORTED,
                "cobel_mfec_pairs: %d states (MFEC serves up to %d states)", n_states,
                COBEL_MFEC_MAX_STATES);
  COBEL_REQUIRE(n_features >= 1 && n_features <= COBEL_MFEC_MAX_FEATURES, COBEL_E_UNSUPPORTED,
                "cobel_mfec_pairs: %d features (MFEC serves 1 to %d features)", n_features,
                COBEL_MFEC_MAX_FEATURES);
  COBEL_REQUIRE((((uintptr_t)features | (uintptr_t)rdist) & 7u) == 0, COBEL_E_ARG,
                "cobel_mfec_pairs: misaligned argument");
  const size_t pairs = (size_t)n_states * n_states;
  hipLaunchKernelGGL(k_mfec_pairs, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, features, n_states, n_features, rdist, same);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

extern "C" int cobel_mfec_run(const cobel_world_t* world, const cobel_mfec_mem_t* mem,
                              const cobel_mfec_run_t* run, void* stream) {
  if (int rc = cobel_world_check(world, "cobel_mfec_run")) return rc;
  if (int rc = check_mem(mem, "cobel_mfec_run")) return rc;
  COBEL_REQUIRE(run && run->inst, COBEL_E_ARG, "cobel_mfec_run: run and run->inst are required");
  COBEL_REQUIRE(world->n_worlds == 1, COBEL_E_UNSUPPORTED,
                "cobel_mfec_run: %d worlds in the handle (the pair tables are one world's)",
                world->n_worlds);
  COBEL_REQUIRE(world->n_states == mem->n_states && world->n_actions == mem->n_actions,
                COBEL_E_ARG,
                "cobel_mfec_run: the world has %d states and %d actions, the memory %d and %d",
                world->n_states, world->n_actions, mem->n_states, mem->n_actions);
  COBEL_REQUIRE(run->n == mem->n, COBEL_E_ARG, "cobel_mfec_run: run->n = %d, mem->n = %d", run->n,
                mem->n);
  COBEL_REQUIRE(run->steps_per_trial >= 1 && run->steps_per_trial <= 65536 * 16, COBEL_E_RANGE,
                "cobel_mfec_run: steps_per_trial = %d", run->steps_per_trial);
  COBEL_REQUIRE(run->ep_sa && run->ep_value, COBEL_E_ARG,
                "cobel_mfec_run: the episode scratch (ep_sa, ep_value) is required");
  COBEL_REQUIRE((run->trace == nullptr) == (run->trace_len == nullptr) &&
                    (!run->trace || run->trace_cap >= 0),
                COBEL_E_ARG, "cobel_mfec_run: trace and trace_len go together");
  COBEL_REQUIRE((((uintptr_t)run->inst | (uintptr_t)run->ep_value | (uintptr_t)run->trace) & 7u) ==
                    0,
                COBEL_E_ARG, "cobel_mfec_run: misaligned inst / ep_value / trace");
  if (mem->n == 0) return COBEL_OK;
  mfec_run_args G;
  G.m = *mem;
  G.r = *run;
  G.rec = world->rec;
  G.next_n = world->next_n;
  G.reward_s = world->reward_s;
  G.terminal_s = world->terminal_s;
  G.starts = world->starts;
  G.start_off = world->start_off;
  G.succ_off = world->succ_off;
  G.succ_state = world->succ_state;
  G.succ_cdf = world->succ_cdf;
  COBEL_HIP_TRY(cobel_launch(k_mfec_run, dim3((unsigned)mem->n), dim3(64), 0, (hipStream_t)stream,
                             G));
  return COBEL_OK;
}

extern "C" int cobel_mfec_estimate(const cobel_mfec_mem_t* mem, const int32_t* nodes,
                                   int32_t n_nodes, double* out, void* stream) {
  if (int rc = check_mem(mem, "cobel_mfec_estimate")) return rc;
  COBEL_REQUIRE(n_nodes >= 0, COBEL_E_RANGE, "cobel_mfec_estimate: n_nodes = %d", n_nodes);
  if (mem->n == 0 || n_nodes == 0) return COBEL_OK;
  COBEL_REQUIRE(nodes && out && ((uintptr_t)out & 7u) == 0 && ((uintptr_t)nodes & 3u) == 0,
                COBEL_E_ARG, "cobel_mfec_estimate: nodes and out must be given, aligned");
  COBEL_REQUIRE((long long)mem->n * n_nodes <= 0x7fffffffll, COBEL_E_RANGE,
                "cobel_mfec_estimate: %d instances x %d nodes", mem->n, n_nodes);
  hipLaunchKernelGGL(k_mfec_estimate, dim3((unsigned)(mem->n * n_nodes)), dim3(64), 0,
                     (hipStream_t)stream, *mem, nodes, n_nodes, out);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}
