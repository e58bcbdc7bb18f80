/* include/kinova_rollout.h -- C ABI of the batched rollout / replay kernels in libkinova_sim.so.
 *
 * The reference drives ONE env from Python and keeps its replay in Python lists; for N envs in lock step the same
 * bookkeeping is a handful of per-env elementwise rules.  Each entry point below is one kernel launch that replaces
 * the loop body named beside it (reference root /root/reference/gym-kinova-gripper):
 *
 *   kr_select_action    main_DDPGfD.py:425-451  check_grasp latch (expert_data.py:559-593), exploration noise,
 *                                               clip, scripted lift action
 *   kr_controller_select expert_data.py:610-671, 746-804 / main_DDPGfD.py:418-439 (--mode naive / combined)  the scripted
 *                                               demonstrators' get_action with the loop's own lift rule, in place of the actor
 *   kr_store_transition main_DDPGfD.py:443-471  replay_buffer.add (utils.py:34-64) for envs that are not lifting,
 *                                               replace (utils.py:309-343) when an episode ends during the lift,
 *                                               per-episode counters; decides which episodes are kept (len-n > 1)
 *   kr_rank_episodes    utils.py:66-90          FIFO slot of every kept episode (env order)
 *   kr_commit_episodes  utils.py:66-90          copy the kept open episodes into the episode ring
 *   kr_advance_ring     utils.py:66-90          ring head / count, open-episode lengths of finished envs
 *   kr_sample_windows   utils.py:240-306        sample_batch_nstep: per sampled episode, ceiling-1 uniform window
 *                                               starts + the final window, as ONE fixed-shape padded batch
 *   kr_commit_classes / kr_sample_windows_balanced   (none: main_DDPGfD.py balances objects while collecting)  the same batch with
 *                                               every episode drawn from one class of its ring, the classes in cyclic rotation
 *
 * Conventions: all pointers are DEVICE pointers owned by the caller (PyTorch tensors); bool arrays are one byte per
 * element; counters are int64; float data is fp32, row-major; every call is asynchronous on `stream` (hipStream_t
 * as void*) and does no host synchronisation, so sequences of them can be captured in a HIP graph.
 * Return value: 0, or a negative ks_status (kinova_sim.h).
 */
#ifndef KINOVA_ROLLOUT_H
#define KINOVA_ROLLOUT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KR_STATE_DIM 82
#define KR_ACTION_DIM 4

/* action selection for n envs.  obs/prev_obs [n,82], has_prev/ready/lifting bool [n], t int64 [n] (steps taken in
 * the episode), actor_out [n,4] = pi(obs), noise [n,4] ~ N(0,1).  ready is updated in place (latched),
 * action [n,4], action_t [4,n] (the layout ks_step takes) and lifting (= ready at the time of the action) are written. */
int kr_select_action(int32_t n, const float *obs, const float *prev_obs, const uint8_t *has_prev, const int64_t *t, uint8_t *ready,
                     const float *actor_out, const float *noise, float sigma, float max_action, int32_t skip_steps,
                     float *action, float *action_t, uint8_t *lifting, void *stream);

/* The scripted demonstrators (expert_data.py:318-671) in kr_select_action's place: no actor output, no noise, no max_action clip.
 * mode: KS_CONTROLLER_NAIVE / _POSITION_DEPENDENT / _COMBINED (1, 2, 3), lift_rule: KS_LIFT_RULE_TRAIN (0: ready |= check_grasp &&
 * has_prev && t + 1 >= skip_steps, lifting = ready; main_DDPGfD.py:418-439) or KS_LIFT_RULE_EXPERT (1: ready |= check_grasp && has_prev
 * && t >= 2, lifting = ready && t > 10; expert_data.py:746-804) - kinova_sim.h; other values: KS_ERR_INVALID.  init float [2, n]
 * (in/out, caller-owned): the episode's (obs[21], obs[81]), written for envs at t == 0, read otherwise.  Per env the arithmetic of
 * kinovagrasping_amd.demonstrators.controller_action on fp32 tensors, operation for operation (csrc/ks_controller.h).  One launch, no
 * LDS, capturable. */
int kr_controller_select(int32_t n, int32_t mode, int32_t lift_rule, const float *obs, const float *prev_obs, const uint8_t *has_prev,
                         const int64_t *t, uint8_t *ready, float *init, int32_t skip_steps, float *action, float *action_t,
                         uint8_t *lifting, void *stream);

/* replay write + bookkeeping after ks_step.  sim_obs/sim_final_obs [n,82], sim_reward [n], sim_done uint8 [n]
 * (non-zero = finished), auto_reset as in ks_config.  Engine state (in/out): obs (the state the action was taken
 * in; becomes the new observation), prev_obs, has_prev, t, ready; lifting/action from kr_select_action.
 * Open episodes (in/out): cur_state/cur_next [n,H,82], cur_action [n,H,4], cur_reward/cur_not_done [n,H],
 * cur_len int64 [n].  Outputs: reward_out [n], done_out bool [n], keep bool [n] (finished AND len - n_steps > 1). */
int kr_store_transition(int32_t n, int32_t horizon, int32_t n_steps, int32_t auto_reset, int32_t with_replay,
                        const float *sim_obs, const float *sim_final_obs, const float *sim_reward, const uint8_t *sim_done,
                        float *obs, float *prev_obs, uint8_t *has_prev, int64_t *t, uint8_t *ready, const uint8_t *lifting,
                        const float *action, float *cur_state, float *cur_next, float *cur_action, float *cur_reward,
                        float *cur_not_done, int64_t *cur_len, float *reward_out, uint8_t *done_out, uint8_t *keep, void *stream);

/* rank [n] int64: number of kept episodes among envs 0..i (inclusive); total int64 [1] */
int kr_rank_episodes(int32_t n, const uint8_t *keep, int64_t *rank, int64_t *total, void *stream);
/* Stream-side pacing for the free-running rollout (no reference counterpart: main_DDPGfD.py:424-486 alternates acting and learning on one
 * thread): a one-wave, LDS-free kernel on `stream` that returns when min_i values[i] >= target (ks_rollout_args.steps_total: every env has
 * done that many env-steps of the persistent rollout launch) or after timeout_s of wall clock - whatever follows on the stream (the
 * learner's next update, the commit of published episodes) then stays within a bounded distance of the SLOWEST env however long the launch is.
 * timeout_s <= 0 waits for ever (like a library collective: only for values that are certain to arrive).  kr_wait_min_counted also adds 1
 * to *timeouts (device int64, may be NULL) when the wait ended on the clock instead of the target, so that a paced run that degrades - e.g.
 * more stepping workgroups than resident slots, whose second round only starts when the first has finished its whole launch - is visible. */
int kr_wait_min(const int64_t *values, int32_t n, int64_t target, double timeout_s, void *stream);
int kr_wait_min_counted(const int64_t *values, int32_t n, int64_t target, double timeout_s, int64_t *timeouts, void *stream);

/* ring rows ep_* [capacity(+), H, ...], ep_len int64; kept env i goes to slot (head + rank[i] - 1) % capacity */
int kr_commit_episodes(int32_t n, int32_t horizon, int32_t capacity, const uint8_t *keep, const int64_t *rank, const int64_t *head,
                       const float *cur_state, const float *cur_next, const float *cur_action, const float *cur_reward,
                       const float *cur_not_done, const int64_t *cur_len, float *ep_state, float *ep_next, float *ep_action,
                       float *ep_reward, float *ep_not_done, int64_t *ep_len, void *stream);

/* head = (head + total) % capacity, count = min(capacity, count + total), cur_len[i] = 0 where ended[i] */
int kr_advance_ring(int32_t n, int32_t capacity, const int64_t *total, int64_t *head, int64_t *count, const uint8_t *ended,
                    int64_t *cur_len, void *stream);

/* n-step window batch: B episodes x W = horizon - n_steps rows.  u_ep [B], u_start [B,W] uniform in [0,1).
 * Episode b is the floor(u_ep[b] * (count - 1))-th OLDEST of the ring (slot head - count + k mod capacity): the newest
 * episode is never sampled (np.random.randint(replay_ep_num - 1), utils.py:259), before and after the ring wraps.
 * Outputs state/next_state [B*W,n_steps,82], action [B*W,n_steps,4], reward/not_done [B*W,n_steps], weight [B*W]
 * (1 for real windows, 0 for padding rows; all 0 while the ring holds fewer than two episodes). */
int kr_sample_windows(int32_t batch, int32_t horizon, int32_t n_steps, const int64_t *count, const int64_t *head, int32_t capacity,
                      const int64_t *ep_len, const float *u_ep, const float *u_start, const float *ep_state, const float *ep_next, const float *ep_action, const float *ep_reward,
                      const float *ep_not_done, float *state, float *action, float *next_state, float *reward, float *not_done,
                      float *weight, void *stream);

/* The same batch with the uniforms drawn in the kernel: Philox4x32-10 keyed by `seed`, counter (draw[0], episode b | row) -
 * `draw` is a device counter that is constant while the kernel runs and differs from call to call (the learner's update
 * count).  No host-side generator, so a captured graph needs no generator-state launches.  next_ends (optional) [2 B W, 82]:
 * next_state[:, 0] followed by next_state[:, n_steps - 1], the rows the target networks evaluate (DDPGfD.py:256-275). */
int kr_sample_windows_draw(int32_t batch, int32_t horizon, int32_t n_steps, const int64_t *count, const int64_t *head, int32_t capacity,
                           const int64_t *ep_len, uint64_t seed, const int64_t *draw, const float *ep_state, const float *ep_next,
                           const float *ep_action, const float *ep_reward, const float *ep_not_done, float *state, float *action,
                           float *next_state, float *reward, float *not_done, float *weight, float *next_ends, void *stream);

/* DDPGfD's demonstration mix (DDPGfD.train_batch, DDPGfD.py:232-254: agent_batch_size = int(batch_size * (1 - prob)) episodes from
 * the agent's replay, the other batch_size - agent_batch_size from the expert replay, concatenated agent first) as ONE launch:
 * episodes b < batch_agent of the batch are drawn from ring `agent`, the others from ring `expert`, each with the rule of
 * kr_sample_windows on its own ring (k-th oldest of count - 1; a ring with fewer than two episodes yields weight-0 rows).
 * Both rings have row shape [*, horizon, ...].  Uniforms: u_ep [batch] + u_start [batch, W] when given (tests), else drawn in the
 * kernel exactly as kr_sample_windows_draw does (Philox keyed by seed, draw[0], b | row).  next_ends optional as there. */
typedef struct {
    const int64_t *count, *head;      /* device scalars: committed episodes, next slot */
    int32_t capacity;
    const int64_t *ep_len;            /* [capacity(+)] */
    const float *ep_state, *ep_next, *ep_action, *ep_reward, *ep_not_done;
} kr_ring;
int kr_sample_windows_mixed(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring *agent, const kr_ring *expert,
                            const float *u_ep, const float *u_start, uint64_t seed, const int64_t *draw, float *state, float *action,
                            float *next_state, float *reward, float *not_done, float *weight, float *next_ends, void *stream);

/* kr_sample_windows_mixed's batch as EPISODE TABLES: the same draws (uniforms given or Philox keyed by seed / draw[0], the same episode and
 * window-start rule), but each batch episode's `horizon` ring rows are written once and a window row is the index of its first state.  The
 * batch * W * n_steps window states of a batch (W = horizon - n_steps) are rows of batch * horizon distinct ones: a learner that works on
 * the tables evaluates each state once (learner_native: NativeDDPGfDUpdate.phase_*_tables).
 *   table_state, table_next  [batch * horizon, 82]  row b * horizon + t = row t of the ring slot batch slot b drew, as the ring holds it
 *   table_action             [batch * horizon, 4]   the same rows' actions (no update reads them beyond action0: they make the batch whole)
 *   row_table  int32 [batch * W]   b * horizon + start of window row (b, w), padding rows included
 *   slot_weight  [batch]           the weight every real window row of slot b carries (1; the prioritized forms: the episode's importance weight)
 *   state0 [R, 82], action0 [R, 4], reward [R, n_steps], not_done [R, n_steps], weight [R]   (R = batch * W) the window rows' first state and
 *                                  action and their columns of kr_sample_windows_mixed's batch: what the critic phase reads
 * so that kr_sample_windows_mixed's state[r][k] = table_state[row_table[r] + k], next_state[r][k] = table_next[row_table[r] + k], action[r][k] = table_action[row_table[r] + k], in every
 * bit.  next_ends (optional) [2 R, 82] as kr_sample_windows_mixed writes it.  KS_ERR_INVALID, nothing launched or written: what
 * kr_sample_windows_mixed refuses, or a NULL output other than next_ends. */
int kr_sample_tables_mixed(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring *agent, const kr_ring *expert,
                           const float *u_ep, const float *u_start, uint64_t seed, const int64_t *draw, float *table_state, float *table_next,
                           float *table_action, int32_t *row_table, float *slot_weight, float *state0, float *action0, float *reward, float *not_done, float *weight,
                           float *next_ends, void *stream);
/* The table form behind the other picks: kr_sample_windows_balanced's, _prioritized's and _balanced_prioritized's arguments and pick launch,
 * kr_sample_tables_mixed's outputs (the table gather as second launch) and `picked` int32 [batch], which is required here.  The prioritized
 * forms write the episode's importance weight to slot_weight[b] and to its real rows in `weight`.  Each equals its window sampler's batch
 * in every bit, as kr_sample_tables_mixed equals kr_sample_windows_mixed's.  KS_ERR_INVALID, nothing launched or written: what the window
 * entry refuses, a NULL output other than next_ends, a NULL picked. */
int kr_sample_tables_balanced(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring *agent, const kr_ring *expert,
                              const int32_t *agent_class, const int32_t *expert_class, int32_t n_classes, int32_t rotation, const float *u_ep,
                              const float *u_start, uint64_t seed, const int64_t *draw, float *table_state, float *table_next, float *table_action,
                              int32_t *row_table, float *slot_weight, float *state0, float *action0, float *reward, float *not_done, float *weight,
                              float *next_ends, int32_t *picked, void *stream);
int kr_sample_tables_prioritized(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring *agent, const kr_ring *expert,
                                 const uint32_t *agent_prio, const uint32_t *expert_prio, const float *beta, const float *u_ep, const float *u_start,
                                 uint64_t seed, const int64_t *draw, float *table_state, float *table_next, float *table_action, int32_t *row_table,
                                 float *slot_weight, float *state0, float *action0, float *reward, float *not_done, float *weight, float *next_ends,
                                 int32_t *picked, void *stream);
int kr_sample_tables_balanced_prioritized(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring *agent,
                                          const kr_ring *expert, const int32_t *agent_class, const int32_t *expert_class, int32_t n_classes,
                                          int32_t rotation, const uint32_t *agent_prio, const uint32_t *expert_prio, const float *beta,
                                          const float *u_ep, const float *u_start, uint64_t seed, const int64_t *draw, float *table_state,
                                          float *table_next, float *table_action, int32_t *row_table, float *slot_weight, float *state0,
                                          float *action0, float *reward, float *not_done, float *weight, float *next_ends, int32_t *picked,
                                          void *stream);

/* ---- replay batches balanced over the episodes' classes (no reference counterpart as a sampler: main_DDPGfD.py takes the stage's objects
 * in Latin-square order while COLLECTING, so that every object contributes the same number of episodes; a free-running or time-budgeted
 * rollout fills the ring at each object's own pace instead, and the balance is restored where the batch is drawn).
 *
 * kr_commit_classes: the per-episode class column of a ring.  keep uint8 [n], rank int64 [n] (kr_rank_episodes), head int64 [1], env_class
 * int32 [n] (the class of whatever env i collects), ep_class int32 [capacity (+ trash row)]: for every env i with keep[i] != 0
 *     ep_class[(head[0] + rank[i] - 1) % capacity] = env_class[i]
 * - kr_commit_episodes' slot rule; issued between kr_rank_episodes and kr_advance_ring.  Nothing else is written. */
int kr_commit_classes(int32_t n, int32_t capacity, const uint8_t *keep, const int64_t *rank, const int64_t *head, const int32_t *env_class,
                      int32_t *ep_class, void *stream);

/* kr_sample_windows_mixed with the episode of every batch slot drawn from ONE class of its ring.  agent_class / expert_class int32: one tag
 * per slot of that ring (expert_class may be NULL only when batch_agent == batch, agent_class only when batch_agent == 0); n_classes in
 * 1 .. 64; picked (optional, may be NULL) int32 [batch]: the ring slot each batch episode was read from.
 * Per ring segment of the batch - agent: slots [0, batch_agent), expert: [batch_agent, batch); b0 its first slot:
 *   eligible   the count - 1 oldest episodes of the ring, age a = 0 .. count - 2 in slot (head - count + a) mod capacity (the newest is
 *              never sampled, as in kr_sample_windows);
 *   m_c        the eligible episodes whose tag is c; a tag outside [0, n_classes) - -1: unknown - counts for no class;
 *   slot b     wants class c = (b - b0 + rotation + (draw ? draw[0] : 0)) mod n_classes (non-negative), and takes the j-th OLDEST eligible
 *              episode of that class, j = (long)(ue * (float)m_c) capped at m_c - 1; where m_c == 0 it falls back to kr_sample_windows'
 *              rule, k = (long)(ue * (float)hi) capped at hi - 1 over all eligible episodes.
 * A ring with fewer than two episodes: as kr_sample_windows (weight-0 rows).  Window starts, the final window, weights, the output layout
 * and next_ends are kr_sample_windows'; the uniforms are the caller's u_ep / u_start or Philox with kr_sample_windows_draw's key, counters
 * and tags.  Hence: with n_classes == 1 and every tag 0 the batch equals kr_sample_windows_mixed's in every bit; within a segment the
 * classes' slot counts differ by at most one, and over n_classes consecutive values of draw[0] every class gets exactly the segment's
 * length in slots.
 * Two launches of one-wave, LDS-free workgroups: the pick (`batch` waves, each walks its ring's tag table twice - count, locate - and
 * touches no episode data) and the gather (batch * W waves, kr_sample_windows' rows with the episode supplied).  Without `picked` the
 * slots travel between the two in `weight`, which needs no more than the [batch * W] floats it has.
 * KS_ERR_INVALID, nothing launched or written: what kr_sample_windows_mixed refuses; n_classes < 1 or > 64; a NULL class array for a ring
 * that has batch slots. */
int kr_sample_windows_balanced(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring *agent, const kr_ring *expert,
                               const int32_t *agent_class, const int32_t *expert_class, int32_t n_classes, int32_t rotation, const float *u_ep,
                               const float *u_start, uint64_t seed, const int64_t *draw, float *state, float *action, float *next_state,
                               float *reward, float *not_done, float *weight, float *next_ends, int32_t *picked, void *stream);

/* ---- prioritized episode replay (DDPGfD's sampling, Vecerik et al. 2017, per episode: an episode is drawn in proportion to the last TD error
 * seen on it, demonstrations carry a priority bonus so that they stay sampled, and importance weights correct the bias).  The reference
 * samples uniformly (utils.py:259); this is an option beside it, not a restatement.
 *
 * A ring may carry ep_prio uint32 [capacity (+ trash row)], one priority per slot in units of 1 / 65536 (65536 is priority 1.0; a committed
 * slot holds 1 .. 2^32 - 1, a stored 0 is read as 1 everywhere), and prio_max uint32 [1], the largest priority any update has written to
 * the ring (initialised to 65536 by the caller).  Priorities are integers, their sums 64-bit and the draw an integer comparison: which
 * episode a uniform takes is exact and independent of any order of evaluation.  The two powf calls below are the only inexact steps.
 * All kernels: one wave per workgroup, no LDS, vector loads / stores and one vector atomic (they run on the learner's stream beside a
 * stepping kernel that holds the CUs' LDS).
 *
 * kr_commit_priorities: keep uint8 [n], rank int64 [n] (kr_rank_episodes), head int64 [1]: for every env i with keep[i] != 0
 *     ep_prio[(head[0] + rank[i] - 1) % capacity] = max(prio_max[0], 1)
 * - kr_commit_episodes' slot rule; a new episode enters at the largest priority seen so far, so it is sampled soon.  Issued between
 * kr_rank_episodes and kr_advance_ring, where kr_commit_classes is.  Nothing else is written. */
int kr_commit_priorities(int32_t n, int32_t capacity, const uint8_t *keep, const int64_t *rank, const int64_t *head, const uint32_t *prio_max,
                         uint32_t *ep_prio, void *stream);

/* kr_sample_windows_mixed with the episode of every batch slot drawn in proportion to its priority within its ring.  agent_prio / expert_prio:
 * the rings' ep_prio (expert_prio may be NULL only when batch_agent == batch, agent_prio only when batch_agent == 0); beta: a device float
 * (a captured graph is annealed by a fill between replays); picked (optional, may be NULL) int32 [batch]: the ring slot each batch episode
 * was read from.  Per ring segment of the batch - agent: slots [0, batch_agent), expert: [batch_agent, batch):
 *   eligible   the count - 1 oldest episodes of the ring, age a = 0 .. count - 2 in slot (head - count + a) mod capacity (the newest is never
 *              sampled, as in kr_sample_windows); p_a = max(ep_prio[slot], 1);
 *   T, p_min   the sum (uint64) and the minimum of the p_a;
 *   slot b     with its episode uniform ue:  t = min(T - 1, (uint64)((double)ue * (double)T))  - one IEEE double product, (double)T exact
 *              because T < 2^52 -, and it takes the episode at the SMALLEST age whose inclusive prefix sum p_0 + .. + p_a exceeds t;
 *   weight     every real window row of the episode gets  w_b = powf((float)p_min / (float)p_b, beta[0])  - the usual (N P(b))^-beta over
 *              its maximum over the ring - in (0, 1]; padding rows get 0.
 * A ring with fewer than two episodes: as kr_sample_windows (slot head - count, weight-0 rows).  Window starts, the final window, the output
 * layout and next_ends are kr_sample_windows'; the uniforms are the caller's u_ep / u_start or Philox with kr_sample_windows_draw's key,
 * counters and tags.  Hence with equal priorities slot b takes age min(count - 2, floor((double)ue * (count - 1))) and every weight is 1.
 * Two launches: the pick (`batch` waves; each walks its ring's one or two contiguous pieces of the table twice - sum and minimum, then
 * locate - with 16-byte loads where aligned, per-element loads at the pieces' ends, nothing outside them read; touches no episode data)
 * and the gather (batch * W waves, kr_sample_windows' rows with the episode supplied).  Between the two w_b travels in `weight`, one copy
 * per row, and without `picked` the slot travels in the first reward of each row: the gather wave of a row reads both before it writes
 * the row.
 * KS_ERR_INVALID, nothing launched or written: what kr_sample_windows_mixed refuses; a NULL beta; for a ring that has batch slots, a NULL
 * priority table or capacity > 2^20. */
int kr_sample_windows_prioritized(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring *agent, const kr_ring *expert,
                                  const uint32_t *agent_prio, const uint32_t *expert_prio, const float *beta, const float *u_ep,
                                  const float *u_start, uint64_t seed, const int64_t *draw, float *state, float *action, float *next_state,
                                  float *reward, float *not_done, float *weight, float *next_ends, int32_t *picked, void *stream);

/* kr_sample_windows_balanced and kr_sample_windows_prioritized combined: the class of every batch slot by the balanced rule, the episode within
 * that class by priority.  The rings carry both columns; agent_class / expert_class, n_classes, rotation as in kr_sample_windows_balanced,
 * agent_prio / expert_prio, beta and picked as in kr_sample_windows_prioritized (a table of a ring without batch slots may be NULL).  Per
 * ring segment of the batch, whose first slot is b0:
 *   eligible   the count - 1 oldest episodes of the ring, age a = 0 .. count - 2 in slot (head - count + a) mod capacity;
 *              p_a = max(ep_prio[slot], 1);
 *   slot b     wants class c = (b - b0 + rotation + (draw ? draw[0] : 0)) mod n_classes (non-negative);
 *   q_a        p_a where the tag of age a is c, else 0; a tag outside [0, n_classes) belongs to no class.  m_c the number of eligible episodes
 *              of the class, T_c the sum (uint64) of the q_a, pmin_c the least p_a of the class;
 *   m_c > 0    with the slot's episode uniform ue:  t = min(T_c - 1, (uint64)((double)ue * (double)T_c))  - one IEEE double product -, and
 *              the slot takes the episode at the SMALLEST age whose inclusive prefix sum q_0 + .. + q_a exceeds t: an episode of class c.
 *              Every real window row of it gets  w_b = powf((float)pmin_c / (float)p_b, beta[0]),  padding rows 0: the importance weight that
 *              corrects the draw back to kr_sample_windows_balanced's distribution, uniform within the class, (T_c / (m_c p_b))^beta, over
 *              its maximum over the class - as kr_sample_windows_prioritized normalises each ring on its own;
 *   m_c == 0   kr_sample_windows_prioritized's rule and weight over all eligible episodes of the ring (kr_sample_windows_balanced falls
 *              back to the uniform rule in the same case).
 * A ring with fewer than two episodes, window starts, the final window, the output layout, next_ends, picked and the uniforms - the caller's
 * or Philox with kr_sample_windows_draw's key, counters and tags -: as the two samplers.  Hence:
 *   - with n_classes == 1 and every tag 0, or with no eligible tag inside [0, n_classes), the batch equals kr_sample_windows_prioritized's;
 *   - with every priority 65536 the slot takes the floor((double)ue * m_c)-th oldest episode of its class and every real weight is exactly 1.
 * Two launches: the pick (`batch` waves; each walks its ring's one or two contiguous pieces of BOTH tables twice - sum and minimum of the
 * class, then locate -, 16-byte loads of the priorities where aligned and of the tags where the two tables sit alike relative to a 16-byte
 * boundary, which they need not, per-element loads otherwise and at the pieces' ends, nothing outside them read, no atomics, no LDS) and
 * kr_sample_windows_prioritized's gather, w_b and the slot travelling the same way.
 * KS_ERR_INVALID, nothing launched or written: what kr_sample_windows_mixed refuses; n_classes < 1 or > 64; a NULL beta; for a ring that has
 * batch slots, a NULL class or priority table or capacity > 2^20. */
int kr_sample_windows_balanced_prioritized(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring *agent,
                                           const kr_ring *expert, const int32_t *agent_class, const int32_t *expert_class, int32_t n_classes,
                                           int32_t rotation, const uint32_t *agent_prio, const uint32_t *expert_prio, const float *beta,
                                           const float *u_ep, const float *u_start, uint64_t seed, const int64_t *draw, float *state,
                                           float *action, float *next_state, float *reward, float *not_done, float *weight, float *next_ends,
                                           int32_t *picked, void *stream);

/* The priorities of the episodes a batch was read from, from the critic's errors on it: issued after kr_critic_grad on the same q, tq1
 * [batch * W], reward [batch * W, n_steps], weight [batch * W] and on the sampler's picked [batch]; W = horizon - n_steps.
 *   real row   r = b W + w is real iff weight[r] > 0;
 *   e_r        |q[r] - (reward[r n_steps] + discount * tq1[r])|, kr_critic_grad's own target_Q, fp32 without contraction;
 *   delta_b    the maximum of e_r over the real rows of batch episode b; NaN if one of them is NaN; -1 without a real row;
 *   v_b        clamp(floor(powf(delta_b + eps, alpha) * 65536), 1, 2^32 - 1) in fp32, the conversion saturating; eps = eps_agent for
 *              b < batch_agent, eps_expert otherwise (eps_expert > eps_agent is the demonstration bonus);
 *   table      for every slot s that a segment picked:  ep_prio[s] = max{ v_b : b in the segment, picked[b] == s, delta_b finite and >= 0 }
 *              - the same episode picked twice has two sets of rows; the maximum is taken inside one wave, no result depends on which wave
 *              runs last -, and the ring's prio_max[0] = max(prio_max[0], that value) (an atomic maximum).  A slot none of whose batch
 *              episodes has a finite delta >= 0 stays as it is: a diverged critic does not reach the table.
 * delta_out (optional) float [batch] receives delta_b (tests, logging).  picked[b] < 0 is skipped; the call has no capacity to check the
 * slots against - they are the sampler's.  Nothing else is written.
 * KS_ERR_INVALID, nothing launched or written: batch <= 0, batch_agent outside [0, batch], horizon <= n_steps, n_steps <= 0; a NULL q, tq1,
 * reward, weight or picked; alpha, eps_agent or eps_expert negative or NaN, discount NaN; for a segment that has batch slots, a NULL table
 * or prio_max. */
int kr_update_priorities(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const float *q, const float *tq1,
                         const float *reward, const float *weight, float discount, const int32_t *picked, float alpha, float eps_agent,
                         float eps_expert, uint32_t *agent_prio, uint32_t *expert_prio, uint32_t *agent_prio_max, uint32_t *expert_prio_max,
                         float *delta_out, void *stream);

/* ---- learner glue (DDPGfD.train_batch, DDPGfD.py:219-367): the elementwise steps between the GEMMs, one launch each
 *
 *   kr_critic_grad   targets + dLoss/dQ of the critic loss L1 + 0.5 LN with masked row means (DDPGfD.py:256-330):
 *                      target_Q  = r[:,0] + discount * tq1,   target_QN = sum_i discount^i r[:,i] + discount^n * tqn
 *                      dq = w / sum(w) * (2 (q - target_Q) + 0.5 * 2 (q - target_QN));  losses[0..2] = (loss, L1, LN)
 *   kr_relu_backward g = (z > 0) ? g : 0 in place (z = the ReLU OUTPUT of the layer)
 *   kr_sigmoid_scale_backward  g *= a (1 - a / max_action)  for a = max_action * sigmoid(z)   (DDPGfD.py:32)
 *   kr_adam_step     torch.optim.Adam (lr, betas, eps, weight_decay as L2 added to the gradient) on a flat parameter buffer;
 *                      step is a device counter that the caller has already incremented
 *   kr_soft_update   target = tau * p + (1 - tau) * target on every `freq`-th value of the device counter `it`
 *                      (DDPGfD.py:360-366), else unchanged
 */
int kr_critic_grad(int32_t rows, int32_t n_steps, const float *q, const float *tq1, const float *tqn, const float *reward,
                   const float *weight, const float *weight_sum, float discount, float *dq, float *losses, void *stream);
/* start of an update (one launch): weight_sum[0] = max(sum(weight), 1) (weight NULL = all ones), dq_actor[rows * n_steps] =
 * -weight[row] / (weight_sum * n_steps) (dLoss/dQ of the actor loss -mean Q(s, pi(s)), DDPGfD.py:341), it[0] += 1 (the update
 * counter Adam and the soft update read), and with pipelined != 0 it_head[0] = it[0]: this update's actor step will be applied by
 * the head of the next one (learner_native.phase_head). */
int kr_update_prologue(int32_t rows, int32_t n_steps, const float *weight, float *weight_sum, float *dq_actor, int64_t *it, int64_t *it_head,
                       int32_t pipelined, void *stream);
/* kr_update_prologue for an update on episode tables (kr_sample_tables_mixed; rows = batch * W): weight_sum, it and it_head as there, and
 *   dq_table [batch * horizon]    slot_weight[b] * (-1 / (weight_sum * n_steps)) for the rows of slot b - kr_update_prologue's own
 *                                 expression, hence dq_actor's bits for every state of a real window row
 *   row_index int32 [rows * n_steps]   the table row of window state (r, k): row_table[r] + k, or -1 where weight[r] == 0
 * (what kr_weight_grad_indexed takes).  KS_ERR_INVALID, nothing launched or written: a NULL pointer or a non-positive size. */
int kr_update_prologue_tables(int32_t rows, int32_t n_steps, int32_t batch, int32_t horizon, const float *weight, const float *slot_weight,
                              const int32_t *row_table, float *weight_sum, float *dq_table, int32_t *row_index, int64_t *it, int64_t *it_head,
                              int32_t pipelined, void *stream);
/* the target critic's Q on the table rows (table_next) -> the [2 * rows] layout kr_critic_grad* take:
 * tq[r] = tq_table[row_table[r]], tq[rows + r] = tq_table[row_table[r] + n_steps - 1].  KS_ERR_INVALID as above. */
int kr_gather_table_q(int32_t rows, int32_t n_steps, const int32_t *row_table, const float *tq_table, float *tq, void *stream);
int kr_relu_backward(int64_t count, const float *act, float *grad, void *stream);
int kr_sigmoid_scale_backward(int64_t count, const float *a, float max_action, float *grad, void *stream);
int kr_adam_step(int64_t count, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const int64_t *step, float lr,
                 float beta1, float beta2, float eps, float weight_decay, void *stream);
int kr_soft_update(int64_t count, const float *param, float *target, float tau, const int64_t *it, int32_t freq, void *stream);

/* ---- TD3fD (ddpgfd.TD3fD; Fujimoto et al. 2018 on the n-step / demonstration update above): twin critics, smoothed target actions, a
 * delayed actor.  One launch each, fp32 without contraction, no LDS.
 *
 *   kr_target_smooth     the target actor's output action [rows, 4] (16-byte aligned), in place, per element:
 *                          e = sigma * z;   e = e < -clip ? -clip : (e > clip ? clip : e);
 *                          s = action + e;  action = s < 0 ? 0 : (s > max_action ? max_action : s)
 *                        - two roundings and two exact clamps; a NaN in action or z fails every comparison and reaches the output.
 *                        z: exactly one of `noise` ([rows, 4] N(0,1) draws, 16-byte aligned) and `draw` (a device counter, as
 *                        kr_actor_select's) is given.  With draw, the four z of row r are ONE Philox4x32-10 call with counter
 *                        (r, draw[0] low word, draw[0] high word, 0x5433) and key (seed low word, seed high word), bits -> uniforms ->
 *                        Box-Muller exactly as kr_actor_select's exploration noise (whose tag is 0x4b52; the samplers' are 0x5a4d /
 *                        0x5a4e): a stream of its own under the same seed and update counter.  One thread per row, grid-stride.
 *                        KS_ERR_INVALID, nothing launched or written: rows <= 0; a NULL or misaligned action; both or neither of noise
 *                        and draw; a misaligned noise; sigma or clip negative or NaN; max_action <= 0 or NaN.
 *   kr_twin_critic_grad  kr_critic_grad for two critics q1, q2 [rows] on the minimum of two target critics:
 *                          m1 = min(tq1_a, tq1_b),  mn = min(tqn_a, tqn_b)   - NaN if either operand is NaN -;
 *                          tmin[r] = m1,  tmin[rows + r] = mn   (exact);
 *                          target_Q, target_QN from m1, mn by kr_critic_grad's expressions in its order;
 *                          dq_k = w / sum(w) * (2 (q_k - target_Q) + 0.5 * 2 (q_k - target_QN));
 *                          losses[0..2] = (loss, L1, LN) of critic 1, losses[3..5] of critic 2.
 *                        One wave, butterfly sums; weight NULL = all ones; weight_sum[0] = 0 gives all-zero dq and losses (tmin is
 *                        written all the same).  With q2 = q1, tq1_b = tq1_a, tqn_b = tqn_a: kr_critic_grad's bits, twice.
 *                        KS_ERR_INVALID, nothing launched or written: rows <= 0, n_steps <= 0, a NULL q1, q2, tq1_a, tq1_b, tqn_a, tqn_b,
 *                        reward, weight_sum, dq1, dq2, tmin or losses.
 *   kr_adam_step_every   the delayed actor's optimizer: acts only if step[0] > 0 and step[0] % every == 0, and then is kr_adam_step as
 *                        step number step[0] / every; otherwise param, grad, exp_avg and exp_avg_sq are untouched.  every = 1 is
 *                        kr_adam_step.  KS_ERR_INVALID, nothing launched or written: what kr_adam_step refuses (count <= 0, a NULL
 *                        pointer); every <= 0.
 */
int kr_target_smooth(int32_t rows, float *action, const float *noise, uint64_t seed, const int64_t *draw, float sigma, float clip,
                     float max_action, void *stream);
int kr_twin_critic_grad(int32_t rows, int32_t n_steps, const float *q1, const float *q2, const float *tq1_a, const float *tq1_b,
                        const float *tqn_a, const float *tqn_b, const float *reward, const float *weight, const float *weight_sum,
                        float discount, float *dq1, float *dq2, float *tmin, float *losses, void *stream);
int kr_adam_step_every(int64_t count, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const int64_t *step, int32_t every,
                       float lr, float beta1, float beta2, float eps, float weight_decay, void *stream);

/* ---- the bounded critic update (ddpgfd.DDPGfD / TD3fD with q_bounds, huber_delta, max_grad_norm): a clamp on the bootstrapped value, a
 * Huber-shaped TD loss, a global gradient-norm clip per network.  One launch each, fp32 without contraction (the norm: fp64), no LDS, no
 * scratch, vector loads and stores only.
 *
 *   kr_critic_grad_bounded  kr_critic_grad (q2, tq1_b, tqn_b and dq2 all NULL: one critic, losses[0..2]) or kr_twin_critic_grad (all four
 *                        given: two critics, losses[0..5]) on a clamped bootstrap and with the loss rho in place of the square.  Per row:
 *                          m1 = tq1_a, or min(tq1_a, tq1_b) - NaN if either operand is NaN - for two critics;  mn likewise from tqn;
 *                          b1 = m1 < q_lo ? q_lo : (m1 > q_hi ? q_hi : m1),  bn likewise from mn   - a NaN passes through -;
 *                          tboot[r] = b1,  tboot[rows + r] = bn   (exact): the bootstrap the update used, which kr_update_priorities reads;
 *                          target_Q, target_QN from b1, bn by kr_critic_grad's expressions in its order;
 *                          e1 = q_k - target_Q,  en = q_k - target_QN;
 *                          c(e)   = e where not |e| > huber_delta, else huber_delta with e's sign;
 *                          rho(e) = e^2 where not |e| > huber_delta, else huber_delta (2 |e| - huber_delta)   - twice the usual Huber
 *                                   function, so that huber_delta = +inf is the square and not half of it; a NaN e takes the square branch -;
 *                          dq_k = w / sum(w) * (2 c(e1) + 0.5 * 2 c(en));
 *                          L1, LN = sum_r w rho(e1), sum_r w rho(en) over sum(w), the terms in fp32 (the square branch is fl(fl(w e) e), as
 *                                   kr_critic_grad's), lane sums and a butterfly;  losses[0] = fl(losses[1] + fl(0.5 losses[2])), and
 *                                   likewise losses[3..5] for critic 2.
 *                        One wave, butterfly sums; weight NULL = all ones; weight_sum[0] = 0 gives all-zero dq and losses (tboot is written
 *                        all the same).  With q_lo = -inf, q_hi = +inf, huber_delta = +inf every output bit is kr_critic_grad's (one
 *                        critic; tboot = (tq1, tqn)) or kr_twin_critic_grad's (two; tboot = tmin).
 *                        KS_ERR_INVALID, nothing launched or written: rows <= 0, n_steps <= 0; a NULL q1, tq1_a, tqn_a, reward, weight_sum,
 *                        dq1, tboot or losses; some but not all of q2, tq1_b, tqn_b, dq2 NULL; q_lo or q_hi NaN, q_lo > q_hi;
 *                        huber_delta <= 0 or NaN.
 *   kr_grad_sqnorm       the squared L2 norm of grad [count] (4-byte aligned: the flat gradient buffers are sliced) as KR_NORM_PARTS fp64
 *                        partial sums: workgroup b (one wave), lane l adds (double)grad[i] * (double)grad[i] - the widening and the square
 *                        are exact - over i = 64 b + l + 4096 k, k = 0, 1, ... in that order, then the 64 lanes' sums are combined by an
 *                        xor butterfly (offsets 32, 16, ..., 1) into partials[b].  The result is a function of (grad, count) alone: no
 *                        atomics, no dependence on the schedule or the grid.  grad is not written.
 *                        KS_ERR_INVALID, nothing launched or written: count <= 0, a NULL grad or partials.
 *   kr_adam_step_clipped kr_adam_step_every behind torch.nn.utils.clip_grad_norm_(params, max_norm): every wave loads the KR_NORM_PARTS
 *                        partials, one per lane, and adds them by the same fp64 butterfly (so all waves hold the same bits); then in fp32
 *                          norm = sqrtf((float)total);  coef = max_norm / (norm + 1e-6f);  coef = coef > 1 ? 1 : coef   (a NaN stays NaN)
 *                        and the step is kr_adam_step_every's with grad[i] * coef in place of grad[i] (scaled before the weight-decay
 *                        term); grad itself is not written.  The gate on step and every is kr_adam_step_every's.  clip_out (optional,
 *                        float [2]) receives (norm, coef) from one lane, also when the gate is closed.  max_norm = +inf with finite
 *                        gradients: kr_adam_step_every's four buffers in every bit.
 *                        KS_ERR_INVALID, nothing launched or written: what kr_adam_step_every refuses (count <= 0, a NULL param, grad,
 *                        exp_avg, exp_avg_sq or step, every <= 0); a NULL partials; max_norm <= 0 or NaN.
 */
#define KR_NORM_PARTS 64
int kr_critic_grad_bounded(int32_t rows, int32_t n_steps, const float *q1, const float *q2, const float *tq1_a, const float *tq1_b,
                           const float *tqn_a, const float *tqn_b, const float *reward, const float *weight, const float *weight_sum,
                           float discount, float q_lo, float q_hi, float huber_delta, float *dq1, float *dq2, float *tboot, float *losses,
                           void *stream);
int kr_grad_sqnorm(int64_t count, const float *grad, double *partials, void *stream);
int kr_adam_step_clipped(int64_t count, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const int64_t *step, int32_t every,
                         const double *partials, float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                         float *clip_out, void *stream);

/* ---- the behaviour-cloning term of the actor loss with its Q-filter (ddpgfd.DDPGfD / TD3fD with bc_weight, q_filter; Nair et al. 2018,
 * "Overcoming Exploration in Reinforcement Learning with Demonstrations"): on the demonstration rows of a batch the actor loss gains
 * bc_weight * sum_r w_r sum_k f_rk |pi(s_rk) - a_rk|^2 / (sum(w) n), whose coefficient per row is -dq[r] for the dq of kr_update_prologue
 * (dq_actor) or kr_update_prologue_tables (dq_table).  One launch, fp32 without contraction, no LDS, no scratch, no atomics, vector loads
 * and stores only (16 bytes per row of a [rows, 4] buffer); one thread per row, grid-stride.
 *
 *   kr_bc_actor_grad     adds the term's gradient to dz3 [rows, 4], dLoss/d(actor pre-activation), in place.  pi [rows, 4] the actor's
 *                        output max_action * sigmoid(z), demo [rows, 4] the batch's actions, q_demo / q_pi [rows] the critic's Q(s, a) and
 *                        Q(s, pi(s)) (both NULL: no filter), dq [rows].  Rows r < demo_from are agent rows.  Per row r >= demo_from:
 *                          f       = 1 without the filter, else 1 where q_demo[r] > q_pi[r] and 0 otherwise - strict, on the floats as given;
 *                                    a NaN on either side gives 0;
 *                          pass[r] = f   (exact);
 *                          d_j     = fl(pi_j - demo_j),  j = 0 .. 3;
 *                          sq[r]   = fl(fl(fl(fl(d_0 d_0) + fl(d_1 d_1)) + fl(d_2 d_2)) + fl(d_3 d_3))  where f = 1, +0 where f = 0;
 *                          and where f = 1, dq[r] != 0 (a NaN is not 0) and bc_weight != 0:
 *                          c       = fl((2 bc_weight) * (-dq[r]))   - 2 bc_weight is exact -;
 *                          s_j     = fl(pi_j * fl(1 - fl(pi_j / max_action)))   - kr_sigmoid_scale_backward's factor in its order -;
 *                          dz3_j   = fl(dz3_j + fl(fl(c d_j) s_j)).
 *                        Rows r < demo_from: sq[r] = pass[r] = +0.  A dz3 row that receives nothing - an agent row, f = 0, dq[r] = 0 (a
 *                        padding row), bc_weight = 0 - is not stored and keeps every bit (a -0.0 and a NaN too); a row with f = 0 does
 *                        not read pi, demo or dz3, so a NaN in pi reaches its own row only, and only where f = 1.  demo_from = rows: dz3 is
 *                        untouched, sq and pass are all +0.  pi, demo, q_demo, q_pi and dq are not written.
 *                        KS_ERR_INVALID, nothing launched or written: rows <= 0; demo_from outside [0, rows]; a NULL pi, demo, dq, dz3, sq
 *                        or pass; a pi, demo or dz3 that is not 16-byte aligned; exactly one of q_demo / q_pi NULL; bc_weight negative or
 *                        NaN; max_action <= 0 or NaN.
 */
int kr_bc_actor_grad(int32_t rows, int32_t demo_from, const float *pi, const float *demo, const float *q_demo, const float *q_pi, const float *dq,
                     float bc_weight, float max_action, float *dz3, float *sq, float *pass, void *stream);

/* ---- running observation normalisation (ddpgfd.DDPGfD / TD3fD with obs_norm): a running mean and standard deviation per observation
 * component, as the HER / DDPG baselines behind Nair et al. 2018 keep them, without clipping - so the map is affine and folds into the
 * actor's first layer, and the rollout kernels act with the folded copy unchanged.  Three launches, no LDS, no scratch, no atomics, fixed
 * reduction order (the results are a function of the inputs alone), stream-ordered and capturable.  fp32 and fp64 without contraction.
 *
 *   kr_obs_stats_update  the statistics (count, mean [dim], m2 [dim]; fp64) take the rows of x [rows, >= dim] (row stride lda floats)
 *                        whose weight [rows] is not 0 (NULL: every row), and mean32 / inv32 [dim] are derived.  With nb such rows:
 *                          mb_c    = (sum_r x_rc) / nb,  q_c = sum_r (x_rc - mb_c)^2      in fp64, two passes; per column PH = 64 / ceil(dim / 4)
 *                                    lanes of one wave add the rows p, p + PH, ... each in ascending order, and their sums are added in ascending p;
 *                          n       = count + nb,  delta = mb_c - mean_c;
 *                          mean_c  = mean_c + delta * (nb / n);
 *                          m2_c    = (m2_c + q_c) + (delta * delta) * (count * (nb / n));
 *                          count   = n;
 *                          mean32_c = fp32(mean_c),  inv32_c = fp32(1 / max(sqrt(m2_c / n), eps)).
 *                        A row with weight 0 is not read into any sum (a NaN in it changes nothing).  nb = 0, or it != NULL and freeze_after
 *                        > 0 and it[0] >= freeze_after (the device's update count: a captured launch keeps its gate): every output keeps
 *                        every bit.  One workgroup of 256 lanes.  KS_ERR_INVALID, nothing launched or written: rows <= 0, dim <= 0, dim > 256,
 *                        lda < dim, a NULL x, count, mean, m2, mean32 or inv32, eps not finite or <= 0, freeze_after < 0.
 *   kr_obs_normalize     x_rc = fl(fl(x_rc - mean32_c) * inv32_c) in place for c < dim; the columns c >= dim of a wider row (lda > dim) are
 *                        neither read nor written.  KS_ERR_INVALID: rows <= 0, dim <= 0, lda < dim, a NULL pointer.
 *   kr_fold_obs_norm     the first layer W1 [h1, in_dim], b1 [h1] that takes raw inputs:  W1_out_jk = fl(W1_jk * inv32_k) for k < norm_dim,
 *                        W1_jk bit for bit for k >= norm_dim (a critic's action columns);  b1_out_j = fp32(b1_j - sum_k W1_out_jk * mean32_k),
 *                        the products exact in fp64, the sum in fp64 in ascending k, the difference rounded to fp64 and then to fp32.
 *                        KS_ERR_INVALID, nothing launched or written: h1 <= 0, in_dim <= 0, norm_dim outside [0, in_dim], a NULL pointer,
 *                        or an output that overlaps an input or the other output. */
int kr_obs_stats_update(int32_t rows, int32_t dim, const float *x, int32_t lda, const float *weight, const int64_t *it, int64_t freeze_after,
                        double *count, double *mean, double *m2, float *mean32, float *inv32, double eps, void *stream);
int kr_obs_normalize(int32_t rows, int32_t dim, float *x, int32_t lda, const float *mean32, const float *inv32, void *stream);
int kr_fold_obs_norm(int32_t h1, int32_t in_dim, int32_t norm_dim, const float *W1, const float *b1, const float *mean32, const float *inv32,
                     float *W1_out, float *b1_out, void *stream);

/* ---- fused 3-layer MLP forward on the matrix cores (fp32 MFMA): Actor.forward (DDPGfD.py:29-32) and
 * Critic.forward (DDPGfD.py:47-50) as ONE launch each:
 *     out[n,out_dim] = f(W3 relu(W2 relu(W1 x + b1) + b2) + b3),   f = identity (KR_ACT_NONE) or scale * sigmoid
 * x = the first in_a columns from xa ([n, >= in_a], row stride lda) followed by in_b columns from xb (row stride ldb;
 * in_b = 0: xb unused) - the critic's cat([state, action], 1) without materialising it.  Weights in torch.nn.Linear
 * layout (W [out][in] row-major, b [out]).  Limits: in_a + in_b <= 96, out_dim <= 4.  Hidden widths: any pair whose tile
 * counts (ceil(h1/16), ceil(h2/16)) are those of an instantiation - (16,16) for 256-256 (BASELINE), (25,19) for 400-300
 * (reference), (8,8) for 128-128, (4,4) for 64-64 - so partial last tiles such as 250-250, 390-290, 120-116 or 60-52 run
 * too (h % 4 != 0 takes the scalar weight loads); any other tile pair returns KS_ERR_INVALID and the caller keeps its GEMM
 * path.  h1_out [n,h1] / h2_out [n,h2] (optional, NULL to skip): the hidden activations (after the ReLU), which the
 * backward pass of a training step needs; they require h % 4 == 0 and 16-byte aligned buffers. */
#define KR_ACT_NONE 0
#define KR_ACT_SIGMOID 1
int kr_mlp3_forward(int32_t n, int32_t in_a, int32_t in_b, int32_t h1, int32_t h2, int32_t out_dim, const float *xa, int32_t lda,
                    const float *xb, int32_t ldb, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                    const float *b3, int32_t act, float scale, float *out, float *h1_out, float *h2_out, void *stream);

/* The same forward WITHOUT LDS (one wavefront per 16 rows, everything in registers, <= 168 registers per lane): its
 * waves can be resident beside a kernel that holds a CU's whole LDS (k_env_step), so a learner's forward-only passes
 * run in that kernel's shadow instead of behind it.  Widths 256-256, 128-128, 64-64 (whole 16-wide tiles only: h % 16 == 0);
 * otherwise KS_ERR_INVALID. */
int kr_mlp3_forward_shadow(int32_t n, int32_t in_a, int32_t in_b, int32_t h1, int32_t h2, int32_t out_dim, const float *xa, int32_t lda,
                           const float *xb, int32_t ldb, const float *W1, const float *b1, const float *W2, const float *b2,
                           const float *W3, const float *b3, int32_t act, float scale, float *out, float *h1_out, float *h2_out,
                           void *stream);

/* Backward of the same MLP, LDS-free like kr_mlp3_forward_shadow (DDPGfD.train_batch's loss.backward(), DDPGfD.py:330-356):
 *   kr_mlp3_backward_shadow   data gradients  dz2 = (dz3 W3) * [h2 > 0],  dz1 = (dz2 W2) * [h1 > 0]  ([n,h2], [n,h1];
 *                             either may be NULL) and optionally  dx = dz1 W1[:, col0 : col0 + ncol]  ([n,ncol], ncol <= 4:
 *                             dQ/da through the critic's first layer), followed - when act_out [n,ncol] is given - by the
 *                             backward of a = scale * sigmoid(z):  dx *= a (1 - a / scale).  dz3 [n,out_dim], h1 / h2 the
 *                             activations kr_mlp3_forward* stored.  Widths 256-256, 128-128, 64-64.
 *   kr_weight_grad_shadow     dW [M,N] = dz^T [ha | hb]  and  db [M] = column sums of dz, dz [n,M], ha [n,>=Na] (row stride
 *                             lda), hb [n,>=Nb] (ldb; Nb = 0: unused); the batch rows are split into `chunks` partial sums
 *                             in `workspace` (chunks * (M*N + M) floats) that a second launch adds up in chunk order.
 *                             Each chunk covers a multiple of 16 rows: chunks beyond ceil(n / that) are not used. */
/* kr_mlp3_forward_shadow with the tiles of each layer split over `waves` (2 or 4) wavefronts of a workgroup: the same LDS-free
 * launch at ~1/waves of the latency (one wave per 16 rows is a serial chain of ~1400 MFMAs: 87 us whatever the batch).  The
 * waves exchange layer 1's output through global memory: h1_out when the caller keeps it, else `scratch`; scratch_floats >=
 * (h1_out ? 0 : ceil(n/16)*16*h1) + ceil(n/16)*waves*64.  Layers 1 and 2 are bitwise those of kr_mlp3_forward_shadow, layer 3's
 * sum is associated per wave (deterministic). */
int kr_mlp3_forward_split(int32_t n, int32_t in_a, int32_t in_b, int32_t h1, int32_t h2, int32_t out_dim, const float *xa, int32_t lda,
                          const float *xb, int32_t ldb, const float *W1, const float *b1, const float *W2, const float *b2,
                          const float *W3, const float *b3, int32_t act, float scale, float *out, float *h1_out, float *h2_out,
                          float *scratch, int64_t scratch_floats, int32_t waves, void *stream);

int kr_mlp3_backward_shadow(int32_t n, int32_t in_dim, int32_t h1, int32_t h2, int32_t out_dim, const float *dz3, const float *W3,
                            const float *h2a, const float *W2, const float *h1a, float *dz2_out, float *dz1_out, const float *W1,
                            int32_t col0, int32_t ncol, const float *act_out, float scale, float *dx_out, void *stream);

/* kr_mlp3_backward_shadow with the dz1 tiles split over `waves` (2 or 4) wavefronts of a workgroup (as kr_mlp3_forward_split);
 * scratch (only used for dx_out: >= ceil(n/16) * waves * 64 floats) holds the waves' partial sums of dx, added in wave order. */
int kr_mlp3_backward_split(int32_t n, int32_t in_dim, int32_t h1, int32_t h2, int32_t out_dim, const float *dz3, const float *W3,
                           const float *h2a, const float *W2, const float *h1a, float *dz2_out, float *dz1_out, const float *W1, int32_t col0,
                           int32_t ncol, const float *act_out, float scale, float *dx_out, float *scratch, int64_t scratch_floats,
                           int32_t waves, void *stream);
int kr_weight_grad_shadow(int32_t n, int32_t M, int32_t Na, int32_t Nb, const float *dz, const float *ha, int32_t lda, const float *hb,
                          int32_t ldb, int32_t chunks, float *workspace, float *dW, float *db, void *stream);
/* kr_weight_grad_shadow over n TERMS read through an index: term r is row idx[r] of dz / ha / hb, which hold `rows` rows; an idx[r]
 * outside [0, rows) reads as zeros.  Terms, order, chunks and rounds are kr_weight_grad_shadow's: the result is bit for bit what it
 * gives on the gathered rows.  KS_ERR_INVALID, nothing launched: what kr_weight_grad_shadow refuses, a NULL idx, rows < 1, a row
 * stride below its width, or rows * max(M, lda, ldb) * 4 >= 2^31. */
int kr_weight_grad_indexed(int32_t n, int32_t rows, int32_t M, int32_t Na, int32_t Nb, const float *dz, const float *ha, int32_t lda,
                           const float *hb, int32_t ldb, const int32_t *idx, int32_t chunks, float *workspace, float *dW, float *db,
                           void *stream);

/* The LEAN LDS-free forward and backward: kr_mlp3_forward_shadow / kr_mlp3_backward_shadow (same operand layouts, optional
 * outputs, act / scale handling and dx epilogue with the sigmoid backward) for the tile pair the one-wave kernels cannot take:
 * (ceil(h1/16), ceil(h2/16)) == (25, 19) - the reference's 400-300 and partial last tiles in either layer, e.g. 392-292.
 * Why they exist: the free-running rollout kernel at that width (k_rollout<25,19>) holds 416 of the 512 registers of every SIMD
 * lane for a whole launch, so a learner wave is resident beside it only within the remaining 96.  Both kernels are capped at
 * 96 registers per lane in the source (amdgpu_waves_per_eu(5, 5)) and use no scratch memory; tools/learner_budget.py reads the
 * compiler's figures and fails when a pairing exceeds 512.  They keep no hidden layer in registers: the first product's output
 * (h1 / dz2) goes through global memory - the caller's h1_out / dz2_out when given, else `scratch` - and is streamed back, with
 * the weights, as the operands of the second product.
 * Refused with KS_ERR_INVALID, nothing written: any other tile pair; h1 % 4 or h2 % 4 != 0; in_a + in_b > 96; out_dim > 4;
 * W2, W3, h1_out, h2_out / h1a, h2a, dz1_out, dz2_out or scratch not 16-byte aligned; a NULL or short scratch when it is needed:
 *   forward   scratch_floats >= (h1_out  ? 0 : ceil(n/16) * 16 * h1)
 *   backward  scratch_floats >= (dz2_out ? 0 : ceil(n/16) * 16 * h2)
 * (scratch may be NULL when that is 0); ceil(n/16) * 16 * max(h1, h2) * 4 bytes, n * lda * 4 and n * ldb * 4 must stay below 2^31.
 * Elements at or beyond h1 / h2 of a partial last tile contribute zero to every reduction and are neither read nor stored. */
int kr_mlp3_forward_lean(int32_t n, int32_t in_a, int32_t in_b, int32_t h1, int32_t h2, int32_t out_dim, const float *xa, int32_t lda,
                         const float *xb, int32_t ldb, const float *W1, const float *b1, const float *W2, const float *b2,
                         const float *W3, const float *b3, int32_t act, float scale, float *out, float *h1_out, float *h2_out,
                         float *scratch, int64_t scratch_floats, void *stream);
int kr_mlp3_backward_lean(int32_t n, int32_t in_dim, int32_t h1, int32_t h2, int32_t out_dim, const float *dz3, const float *W3,
                          const float *h2a, const float *W2, const float *h1a, float *dz2_out, float *dz1_out, const float *W1, int32_t col0,
                          int32_t ncol, const float *act_out, float scale, float *dx_out, float *scratch, int64_t scratch_floats,
                          void *stream);

/* Actor forward + exploration noise + kr_select_action in ONE launch (main_DDPGfD.py:424-451): the epilogue of the
 * fused MLP applies the selection rule to its own output.  obs .. ready and action .. lifting as in kr_select_action;
 * W1 .. b3 the actor (82 -> h1 -> h2 -> 4; any hidden widths kr_mlp3_forward accepts, partial last tiles included).
 * Noise: either `noise` [n,4] ~ N(0,1) (then rng_state = NULL), or noise = NULL and rng_state = int64[2] on the device, zero-initialised by the caller: the kernel draws
 * Philox4x32-10 / Box-Muller normals keyed by (seed, rng_state[0], env) and advances rng_state[0] by one per launch
 * (rng_state[1] is its scratch word) - no host-side generator state, so the launch replays from a HIP graph.
 * actor_out [n,4] (optional, may be NULL) receives pi(obs). */
int kr_actor_select(int32_t n, int32_t h1, int32_t h2, const float *obs, const float *prev_obs, const uint8_t *has_prev, const int64_t *t,
                    uint8_t *ready, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3, const float *b3,
                    const float *noise, uint64_t seed, int64_t *rng_state, float sigma, float max_action, int32_t skip_steps,
                    float *actor_out, float *action, float *action_t, uint8_t *lifting, void *stream);

/* ---- the learner's one exchange step (gradient mean over the env-shard ranks; the reference is single-process,
 * its multi-GPU form is DDPGfD.train_batch on every rank + an all-reduce of the gradients, DDPGfD.py:330-356).
 * An LDS-free all-reduce over peer-mapped device memory (csrc/ks_xchg.hip): it runs beside ks_step's stepping kernel, which
 * holds every CU's LDS; a library (RCCL) collective would wait for it.  One process per GPU:
 *   kr_xchg_create   allocates this rank's exchange block for buffers of up to max_count floats and returns its
 *                    KR_XCHG_HANDLE_BYTES-byte inter-process handle (hipIpcGetMemHandle);
 *   kr_xchg_connect  takes the handles of ALL ranks (world x KR_XCHG_HANDLE_BYTES, rank order; gathered by the caller, e.g.
 *                    torch.distributed.all_gather_object) and maps the peers' blocks;
 *   kr_xchg_allreduce_mean  grad[i] <- mean over ranks of grad[i], in place, asynchronous on `stream`; every rank must make
 *                    the same sequence of calls (same counts).  The sum runs in rank order on every rank: bitwise identical
 *                    results everywhere.  grad must be 16-byte aligned;
 *   kr_xchg_status   failed_epoch = 0, or the number of the first call in which a peer did not arrive within ~4 s (the call
 *                    then leaves grad unreduced instead of hanging the GPU). */
#define KR_XCHG_MAX_RANKS 8
#define KR_XCHG_HANDLE_BYTES 64
typedef struct kr_xchg kr_xchg;
int kr_xchg_create(kr_xchg **out, int32_t world, int32_t rank, int64_t max_count, uint8_t *handle_out);
int kr_xchg_connect(kr_xchg *x, const uint8_t *handles);
int kr_xchg_allreduce_mean(kr_xchg *x, float *grad, int64_t count, void *stream);
int kr_xchg_status(kr_xchg *x, uint32_t *failed_epoch);
void kr_xchg_destroy(kr_xchg *x);

#ifdef __cplusplus
}
#endif
#endif
