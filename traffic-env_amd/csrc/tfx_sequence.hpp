// tfx_sequence.hpp - the ONE launch sequence of the per-tick kernels, for plain tfx_step calls and agent steps alike
// (host side; included by tfx_hip.hip):
//   pair       the launches of two ticks - the only place that names their order
//   single     the launches of one tick
//   run_ticks  the loop over a call's ticks: pairs, then the odd tick; the env range in two halves on two streams
//   agent_sequence  what a decision launches around its ticks (tfx_step's counterpart, step_body, is in tfx_hip.hip)
// Where an agent step (tfx_agent_step, `if done: break`) differs from a plain call it says `agent`:
//   k_risk     ahead of the pass of an agent step's pair, unless a k_tail before it evaluated the bound; never in a plain call
//   the pass   a plain call's reads the road state words of the k_tail before it (rsw) from its second pair on; never an agent's
//   k_tail     agent: TAIL_RISK_NEXT while another pair follows; plain: TAIL_SYNC on the call's last pair; both: TAIL_LAST
//   no k_tail  agent: the restricted one-tick pass (the envs k_risk sorted out) between the edge and the second advance
//   timing     tfx_profile times plain calls only (TickTimer)
//   counters   tfx_tail_ticks counts plain calls only; pair, split and fused ticks count for both
// A sequence only enqueues: on the caller's stream, on the handle's second stream, or into a stream capture.  Every grid
// it launches with was sized by size_grids at the API entry (tfx_launch.hpp), for the whole env range; the ticks it
// enqueues are added to the handle's counters as their pair is enqueued - a call that fails midway keeps those of the
// pairs it had enqueued (a capture takes them back and adds them per replay: run_captured, tfx_hip.hip).
#pragma once
#include "tfx_clone.hpp"
#include "tfx_launch.hpp"

namespace {

// The masked restart of a decision from the attached pool (tfx_set_episode_pool): what tfx_clone_envs(h, pool, src, 0)
// does with src[env] = the slot of rule 3 for the marked envs and -1 for the others, the source picked in the kernel
// (k_clone<true>, which also leaves the `last` flags behind) - the pool as it is when the launch runs
int launch_pool_restart(tfx_handle h, hipStream_t st) {
  const tfx_handle pool = h->pool;
  CloneOpt o{};
  o.d_ep = h->ep;
  if (h->d.greedy_act && pool->d.greedy_act) {
    o.d_greedy = h->d.greedy_act;
    o.s_greedy = pool->d.greedy_act;
  }
  hipLaunchKernelGGL(k_clone<true>, dim3((unsigned)tile_grid(h)), dim3(256), 0, st, h->d, pool->d, (const int *)nullptr, o);
  HIPCHK(hipGetLastError());
  return TFX_OK;
}

// the second stream of a split call and the events that fork it from / join it to the caller's stream.
// The second stream must not share a hardware queue with the caller's: HIP hands its hardware queues (4 per priority
// level by default) to streams as they are created and shares them from then on, and two streams on one queue run
// their kernels in order - no overlap.  Measured at cfg2 in a process that had initialised RCCL before the handle's
// first split call (as every rank of `bench.py --gpus N` does): a plain second stream 4.43-4.47e11 vehicle-updates/s
// against 5.1-5.2e11 without RCCL; a second stream of ANOTHER priority level - its own pool of queues - 5.10-5.11e11
// either way (low priority: 4.91e11; a CU-masked stream: 4.43e11 either way).
int ensure_split(tfx_handle h, hipStream_t caller) {
  int lo = 0, hi = 0, cp = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));  // (numerically: hi <= 0 <= lo)
  if (hipStreamGetPriority(caller, &cp) != hipSuccess) cp = 0;
  const int want = (cp == hi) ? lo : hi;   // high priority; low if high is the caller's own level
  if (h->split_stream && h->split_prio == want) return TFX_OK;
  if (h->split_stream) {
    HIPCHK(hipStreamSynchronize(h->split_stream));
    HIPCHK(hipStreamDestroy(h->split_stream));
    h->split_stream = nullptr;
  }
  HIPCHK(hipStreamCreateWithPriority(&h->split_stream, hipStreamNonBlocking, want));
  h->split_prio = want;
  if (h->split_fork) return TFX_OK;
  HIPCHK(hipEventCreateWithFlags(&h->split_fork, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&h->split_join, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&h->split_stagger, hipEventDisableTiming));
  return TFX_OK;
}

// Whatever a launch sequence changes in the handle while it enqueues - the device block (agent mode, reward
// accumulation, the sub-range of one half), the half being enqueued - is put back on EVERY exit, and a second stream
// that was forked is joined back into the caller's stream, so that work already enqueued there stays ordered before
// whatever the caller enqueues next: an error in the middle of a sequence leaves a handle the next call can use.
struct SeqGuard {
  tfx_handle h;
  Dev keep;
  hipStream_t user = nullptr;
  bool forked = false;
  explicit SeqGuard(tfx_handle hh) : h(hh), keep(hh->d) {}
  int fork(hipStream_t st) {
    user = st;
    HIPCHK(hipEventRecord(h->split_fork, st));
    HIPCHK(hipStreamWaitEvent(h->split_stream, h->split_fork, 0));
    forked = true;
    return TFX_OK;
  }
  int join() {
    if (!forked) return TFX_OK;
    forked = false;
    HIPCHK(hipEventRecord(h->split_join, h->split_stream));
    HIPCHK(hipStreamWaitEvent(user, h->split_join, 0));
    return TFX_OK;
  }
  ~SeqGuard() {
    h->d = keep;
    h->split_half = -1;
    h->split_first = false;
    if (forked) {  // (an error exit: best effort, the error being reported is the first one)
      const std::string first = g_err;
      (void)join();
      g_err = first;
    }
  }
};

// Per-kernel timing of plain calls (tfx_profile): three events per timed entry - ahead of the mover, behind it, behind
// the entry's last launch - and the ticks the entry covers.  Active while the handle times and has entries left when
// begin() is asked; does nothing otherwise.
struct TickTimer {
  tfx_handle h;
  hipEvent_t *e = nullptr;
  explicit TickTimer(tfx_handle hh) : h(hh) {}
  int begin(hipStream_t st) {
    if (!h->prof || h->ev_used >= h->ev_ticks) return TFX_OK;
    e = &h->ev[(size_t)h->ev_used * 3];
    HIPCHK(hipEventRecord(e[0], st));
    return TFX_OK;
  }
  int mid(hipStream_t st) {
    if (e) HIPCHK(hipEventRecord(e[1], st));
    return TFX_OK;
  }
  int end(hipStream_t st, int weight) {
    if (!e) return TFX_OK;
    HIPCHK(hipEventRecord(e[2], st));
    h->ev_weight[h->ev_used] = weight;
    ++h->ev_used;
    return TFX_OK;
  }
};

// Ticks t and t + 1 of a call (a chunk) of n_ticks ticks, of the envs h->d describes (the whole handle, or one half of
// it), on st: a two-tick pass (tfx_move_tt.hpp) and the rest of the pair.
int pair(tfx_handle h, int t, int n_ticks, hipStream_t st, bool agent) {
  const bool tail = tail_usable(h);
  TickTimer timer(h);
  if (int rc = launch_inputs(h, st)) return rc;
  // agent steps: envs in which the first tick of a pair could overflow take the pair one tick at a time (k_risk; k_tail
  // evaluates the bound for the pair that follows it: only the first pair pays a launch of its own)
  if (agent && !(tail && t > 0)) {
    if (int rc = launch_risk(h, t, st)) return rc;
  }
  if (!agent) {
    if (int rc = timer.begin(st)) return rc;
  }
  // (plain calls: from a call's second pair on the pass reads the road state words the k_tail before it left; the last
  // k_tail of the call stores leading / lastcar / hb themselves)
  if (int rc = launch_move_tt(h, true, agent, t, st, 0, tail, agent ? false : t > 0)) return rc;
  if (int rc = timer.mid(st)) return rc;
  if (tail) {
    // the rest of the pair in one launch (agent: the envs k_risk sorted out get their second tick inside it)
    const int flags = (t + 2 >= n_ticks ? TAIL_LAST : 0) |
                      (agent ? (t + 3 < n_ticks ? TAIL_RISK_NEXT : 0) : (t + 3 >= n_ticks ? TAIL_SYNC : 0));
    if (int rc = launch_tail(h, t, st, agent, flags)) return rc;
    if (!agent) h->tail_ticks += 2;
  } else {
    if (int rc = launch_advance(h, t, st)) return rc;
    if (int rc = launch_inputs(h, st)) return rc;
    if (int rc = launch_edge(h, agent, t + 1, st)) return rc;
    if (agent) {
      if (int rc = launch_move_tt(h, false, true, t + 1, st, /*only_risky=*/1)) return rc;
    }
    if (int rc = launch_advance(h, t + 1, st)) return rc;
  }
  if (int rc = timer.end(st, 2)) return rc;
  h->pair_ticks += 2;
  return TFX_OK;
}

// Tick t alone.  A handle that runs its calls as pairs takes the one-tick form of the pass, or k_move_ts where the
// launch is small enough for it (single_tick_ts)
int single(tfx_handle h, int t, hipStream_t st, bool agent) {
  TickTimer timer(h);
  if (int rc = launch_inputs(h, st)) return rc;
  if (!agent) {
    if (int rc = timer.begin(st)) return rc;
  }
  if (int rc = (pairs_usable(h) && !single_tick_ts(h)) ? launch_move_tt(h, false, agent, t, st) : launch_move(h, t, st)) return rc;
  if (int rc = timer.mid(st)) return rc;
  if (int rc = launch_advance(h, t, st)) return rc;
  return timer.end(st, 1);
}

// The ticks of a call (of one chunk of a tfx_step call) on the per-tick kernels, on st: pairs, then the odd tick.
// split (split_usable; ensure_split has run): the env range in two halves, the handle's own stream takes the second
// half of the envs, the caller's stream the first - launched eagerly: a batch big enough to split is not bound by its
// launches.
int run_ticks(tfx_handle h, int n_ticks, hipStream_t st, bool agent, bool split) {
  SeqGuard guard(h);
  const Dev whole = h->d;
  Dev halves[2] = {whole, whole};
  if (split) {
    // (the second half's clock is copied on the CALLER's stream, ahead of the fork: copied on the second stream it
    // raced with the first half's kernels, which move the clock on - a new stream's first launch can take longer to
    // start than a small batch's whole pair)
    hipLaunchKernelGGL(k_clock_copy, dim3(1), dim3(1), 0, st, whole.tickA, whole.tickB, h->misc->clock2);
    HIPCHK(hipGetLastError());
    if (int rc = guard.fork(st)) return rc;
    const int n0 = whole.E / 2;
    halves[0] = sub_dev(whole, 0, n0, nullptr);
    halves[1] = sub_dev(whole, n0, whole.E - n0, h->misc->clock2);
  }
  // The two halves' launches are submitted pair by pair, alternately.  (Submitted half after half - all of the first
  // half's launches, then the second's - the second stream's first launch reached the device only after the host had
  // queued the whole first half: under rocprofv3 the first half ran FIVE pairs alone at the start of a 50-tick call
  // and the second five alone at its end, each at 0.47 ms per half pair instead of the 0.39 of two halves side by
  // side; profiles/r04_split_submission_order.txt.)  One range: all its ticks in one turn.
  const long long pair0 = h->pair_ticks, tail0 = h->tail_ticks;
  const int turn = split ? 2 : n_ticks;
  int rc = TFX_OK;
  for (int t0 = 0; t0 < n_ticks && rc == TFX_OK; t0 += turn) {
    for (int half = 0; half < (split ? 2 : 1) && rc == TFX_OK; ++half) {
      if (split) {
        h->d = halves[half];
        h->split_half = half;
        h->split_first = t0 == 0;
      }
      const hipStream_t hs = half == 0 ? st : h->split_stream;
      const int t_hi = t0 + turn < n_ticks ? t0 + turn : n_ticks;
      int t = t0;
      if (pairs_usable(h))
        for (; t + 1 < t_hi && rc == TFX_OK; t += 2) rc = pair(h, t, n_ticks, hs, agent);
      for (; t < t_hi && rc == TFX_OK; ++t) rc = single(h, t, hs, agent);
    }
  }
  if (!split) return rc;
  h->d = whole;
  h->split_half = -1;
  h->pair_ticks = pair0 + (h->pair_ticks - pair0) / 2;  // (both halves counted them)
  h->tail_ticks = tail0 + (h->tail_ticks - tail0) / 2;
  if (rc != TFX_OK) return rc;  // (the guard joins the second stream)
  h->split_ticks += n_ticks;
  return guard.join();
}

// the launches of one agent step, in order, on `st`: the episode restart, then k_res with the decision's tail inside, or
// the per-tick kernels between k_agent_begin and k_agent_tail
int agent_sequence(tfx_handle h, int n_ticks, int remi, float *aobs, float *areward, uint8_t *adone,
                   hipStream_t st, bool split) {
  Dev &d = h->d;
  SeqGuard guard(h);
  if (h->ep.on) {
    // episodes (tfx_set_episodes): the envs whose last decision ended their episode restart, ahead of the ticks and
    // of any fork - the one launch the feature adds; the accounting rides in the decision's tail
    TFX_INJECT(h);
    if (h->pool) {
      // ... as clones of envs of the attached pool (tfx_set_episode_pool), in that same one launch
      if (int rc = launch_pool_restart(h, st)) return rc;
    } else {
      hipLaunchKernelGGL(k_episode_begin, dim3(grid_for(h, (long)d.E * d.R)), dim3(256), 0, st, d, h->ep);
      HIPCHK(hipGetLastError());
    }
  }
  if (h->stream.upfront()) {
    // demand profiles (tfx_set_demand): the decision's rows up front, from the device clock on - exact because rule 4
    // is stateless: an env that overflows simply does not consume the rows of the ticks it skips.  From here on the
    // decision runs as it does for a bound per-tick count buffer.
    if (int rc = launch_stream(h, n_ticks, st)) return rc;
  }
  if (res_usable(h, n_ticks)) {
    // every tick of the decision AND its tail (remi, observation, rewards, done flags) in one launch
    d.agent_mode = 1;
    d.accum_rewards = remi ? 0 : 1;
    const int rc = launch_res(h, n_ticks, st, 1, remi, aobs, areward, adone);
    if (rc == TFX_OK) h->fused_ticks += n_ticks;
    return rc;
  }
  hipLaunchKernelGGL(k_agent_begin, dim3(1), dim3(1), 0, st, d, const_cast<int *>(d.agent_first));
  HIPCHK(hipGetLastError());
  if (int rc = launch_greedy(h, st)) return rc;
  d.agent_mode = 1;
  d.accum_rewards = remi ? 0 : 1;
  if (int rc = run_ticks(h, n_ticks, st, true, split)) return rc;
  d.agent_mode = guard.keep.agent_mode;  // the tail kernel below runs outside the step's tick loop
  d.accum_rewards = guard.keep.accum_rewards;
  if (remi || aobs || areward || adone || h->ep.on) {
    hipLaunchKernelGGL(k_agent_tail, dim3(grid_for(h, (long)d.E * (2 * d.r + d.I))), dim3(256), 0, st, d, remi, aobs,
                       areward, adone, d.agent_first, h->ep);
    HIPCHK(hipGetLastError());
  }
  return TFX_OK;
}

}  // namespace
