// ks_rollout.hip -- batched rollout / replay bookkeeping kernels (C ABI: include/kinova_rollout.h).
//
// Every kernel is HBM-streaming elementwise work on struct-of-rows tensors owned by PyTorch: one wavefront per
// env (or per sampled window row), lanes across the 82 observation columns, so that row reads/writes are
// coalesced 256-byte bursts.  No LDS, no atomics; the only cross-env step (FIFO ranks of the kept episodes) is a
// single-block scan.  The torch implementations in rollout.py / replay.py are the checkers of these kernels.
#include <hip/hip_runtime.h>

#include "../../include/kinova_rollout.h"
#include "../../include/kinova_sim.h"
#include "ks_select.h"

namespace {

constexpr int WAVE = 64;
constexpr int S = KR_STATE_DIM, A = KR_ACTION_DIM;

__global__ __launch_bounds__(256) void k_select_action(int n, const float* __restrict__ obs, const float* __restrict__ prev_obs,
                                                       const uint8_t* __restrict__ has_prev, const int64_t* __restrict__ t, uint8_t* ready,
                                                       const float* __restrict__ actor_out, const float* __restrict__ noise, float sigma,
                                                       float max_action, int skip_steps, float* __restrict__ action,
                                                       float* __restrict__ action_t, uint8_t* __restrict__ lifting) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float pi[A], nz[A];
#pragma unroll
    for (int k = 0; k < A; k++) { pi[k] = actor_out[(long)i * A + k]; nz[k] = noise[(long)i * A + k]; }
    krsel::select_one(i, n, pi, nz, obs, prev_obs, has_prev, t, ready, sigma, max_action, skip_steps, action, action_t, lifting);
}

// the scripted demonstrators in k_select_action's place (ks_controller.h): one env per lane
__global__ __launch_bounds__(256) void k_controller_select(int n, int mode, int lift_rule, const float* __restrict__ obs,
                                                           const float* __restrict__ prev_obs, const uint8_t* __restrict__ has_prev,
                                                           const int64_t* __restrict__ t, uint8_t* ready, float* init, int skip_steps,
                                                           float* __restrict__ action, float* __restrict__ action_t, uint8_t* __restrict__ lifting) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    krsel::controller_one(i, n, mode, lift_rule, obs, prev_obs, has_prev, t, ready, init, skip_steps, action, action_t, lifting);
}

// one wave per env
__global__ __launch_bounds__(WAVE) void k_store_transition(int n, int H, int n_steps, int auto_reset, int with_replay,
                                                           const float* __restrict__ sim_obs, const float* __restrict__ sim_final,
                                                           const float* __restrict__ sim_reward, const uint8_t* __restrict__ sim_done,
                                                           float* obs, float* prev_obs, uint8_t* has_prev, int64_t* t, uint8_t* ready,
                                                           const uint8_t* __restrict__ lifting, const float* __restrict__ action,
                                                           float* cur_state, float* cur_next, float* cur_action, float* cur_reward,
                                                           float* cur_not_done, int64_t* cur_len, float* reward_out, uint8_t* done_out,
                                                           uint8_t* keep) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const bool done = sim_done[i] != 0, lift = lifting[i] != 0;
    const float rew = sim_reward[i];
    const bool store = with_replay && !lift;
    const long len0 = with_replay ? cur_len[i] : 0;
    const long tt = len0 < H - 1 ? len0 : H - 1;
    const long row = ((long)i * H + tt);
    for (int c = lane; c < S; c += WAVE) {
        const float so = sim_obs[(long)i * S + c];
        const float st = obs[(long)i * S + c];
        const float nx = (done && auto_reset) ? sim_final[(long)i * S + c] : so;
        if (store) { cur_state[row * S + c] = st; cur_next[row * S + c] = nx; }
        prev_obs[(long)i * S + c] = done ? so : st;
        obs[(long)i * S + c] = so;
    }
    if (store && lane < A) cur_action[row * A + lane] = action[(long)i * A + lane];
    if (lane == 0) {
        long len1 = len0;
        if (store) {
            cur_reward[row] = rew;
            cur_not_done[row] = done ? 0.0f : 1.0f;
            len1 = tt + 1;
        }
        if (with_replay) {
            // the episode ended during the scripted lift: the last stored transition carries the outcome
            if (done && lift && len1 > 0) {
                cur_reward[(long)i * H + len1 - 1] = rew;
                cur_not_done[(long)i * H + len1 - 1] = 0.0f;
            }
            cur_len[i] = len1;
            keep[i] = done && (len1 - n_steps > 1);
        }
        has_prev[i] = !done;
        t[i] = done ? 0 : t[i] + 1;
        ready[i] = (ready[i] != 0) && !done;
        reward_out[i] = rew;
        done_out[i] = done;
    }
}

// One wavefront, no LDS (so that the launch can run while the stepping kernel holds the CUs' LDS): every lane counts a
// contiguous slice of the flags, the lane totals are scanned with shuffles, the ranks written back per slice.
__global__ __launch_bounds__(WAVE) void k_rank_episodes(int n, const uint8_t* __restrict__ keep, int64_t* __restrict__ rank, int64_t* total) {
    const int lane = threadIdx.x;
    const int per = (n + WAVE - 1) / WAVE, i0 = min(lane * per, n), i1 = min(i0 + per, n);
    int local = 0;
    for (int i = i0; i < i1; i++) local += keep[i] != 0;
    int incl = local;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    int before = incl - local;
    for (int i = i0; i < i1; i++) {
        before += keep[i] != 0;
        rank[i] = before;
    }
    if (lane == WAVE - 1) total[0] = incl;
}

// one wave per env; only kept envs move data
__global__ __launch_bounds__(WAVE) void k_commit_episodes(int n, int H, int capacity, const uint8_t* __restrict__ keep,
                                                          const int64_t* __restrict__ rank, const int64_t* __restrict__ head,
                                                          const float* __restrict__ cur_state, const float* __restrict__ cur_next,
                                                          const float* __restrict__ cur_action, const float* __restrict__ cur_reward,
                                                          const float* __restrict__ cur_not_done, const int64_t* __restrict__ cur_len,
                                                          float* ep_state, float* ep_next, float* ep_action, float* ep_reward,
                                                          float* ep_not_done, int64_t* ep_len) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n || keep[i] == 0) return;
    const long slot = (head[0] + rank[i] - 1) % capacity;
    const long src = (long)i * H, dst = slot * H;
    // 16-byte copies where the episode blocks are 16-byte aligned (H * 82 floats: even H), several loads in flight: at an
    // episode boundary all 4096 envs commit (84 MB) while the rollout waits - float by float this took 0.4 ms
    if ((H * S) % 4 == 0) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f* s0 = (const v4f*)(cur_state + src * S); const v4f* s1 = (const v4f*)(cur_next + src * S);
        v4f* d0 = (v4f*)(ep_state + dst * S); v4f* d1 = (v4f*)(ep_next + dst * S);
        const int n4 = H * S / 4;
        int k = lane;
        for (; k + WAVE < n4; k += 2 * WAVE) {
            const v4f a = s0[k], b = s0[k + WAVE], c = s1[k], d = s1[k + WAVE];
            d0[k] = a; d0[k + WAVE] = b; d1[k] = c; d1[k + WAVE] = d;
        }
        for (; k < n4; k += WAVE) { d0[k] = s0[k]; d1[k] = s1[k]; }
    } else {
        for (int k = lane; k < H * S; k += WAVE) {
            ep_state[dst * S + k] = cur_state[src * S + k];
            ep_next[dst * S + k] = cur_next[src * S + k];
        }
    }
    for (int k = lane; k < H * A; k += WAVE) ep_action[dst * A + k] = cur_action[src * A + k];
    for (int k = lane; k < H; k += WAVE) {
        ep_reward[dst + k] = cur_reward[src + k];
        ep_not_done[dst + k] = cur_not_done[src + k];
    }
    if (lane == 0) ep_len[slot] = cur_len[i];
}

__global__ __launch_bounds__(256) void k_advance_ring(int n, int capacity, const int64_t* __restrict__ total, int64_t* head, int64_t* count,
                                                      const uint8_t* __restrict__ ended, int64_t* cur_len) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        const long k = total[0];
        head[0] = (head[0] + k) % capacity;
        const long c = count[0] + k;
        count[0] = c < capacity ? c : capacity;
    }
    if (i < n && ended[i] != 0) cur_len[i] = 0;
}

struct Ring {                      // one episode ring of DeviceEpisodeReplay (kr_ring of the C ABI)
    const int64_t* count;
    const int64_t* head;
    int capacity;
    const int64_t* ep_len;
    const float *ep_state, *ep_next, *ep_action, *ep_reward, *ep_not_done;
};

// the sampler's uniforms: the caller's, or (u == nullptr) Philox4x32-10 keyed by the seed at counter (draw[0], index, tag) - `draw` is a
// device counter that does not change while the kernel runs (the learner's update count).  tag 0x5a4d with the batch episode b: which
// episode; tag 0x5a4e with the row r: where its window starts.
__device__ __forceinline__ float sample_uniform(const float* __restrict__ u, long index, uint32_t tag, unsigned long long seed,
                                                const int64_t* __restrict__ draw) {
    if (u != nullptr) return u[index];
    const unsigned long long d = (unsigned long long)draw[0];
    uint32_t r4[4];
    krsel::philox4x32((uint32_t)index, (uint32_t)d, (uint32_t)(d >> 32), tag, (uint32_t)seed, (uint32_t)(seed >> 32), r4);
    return (float)(r4[0] >> 8) * (1.0f / 16777216.0f);
}

// np.random.randint(replay_ep_num - 1): the k-th OLDEST episode, k in [0, count - 1) - the newest one is never sampled
// (utils.py:259).  In the ring the oldest episode sits at head - count, so after the first wrap the excluded slot is
// head - 1, wherever that is.  (Fewer than two episodes: slot head - count, and every row of it gets weight 0.)
__device__ __forceinline__ long uniform_episode(float ue, long cnt, long head, int capacity) {
    long hi = cnt - 1;
    hi = hi > 1 ? hi : 1;
    long k = (long)(ue * (float)hi);
    k = k < hi - 1 ? k : hi - 1;
    long ep = (head - cnt + k) % capacity;
    return ep < 0 ? ep + capacity : ep;
}

// where window w of the episode in ring slot `ep` starts (utils.py:283-301), and the episode's number of real windows: the one rule of
// the window form (window_row) and of the table form (k_sample_tables)
__device__ __forceinline__ long window_start(const Ring& g, long ep, float us, int H, int n_steps, int w, long& ceiling) {
    ceiling = g.ep_len[ep] - n_steps;
    ceiling = ceiling > 1 ? ceiling : 1;
    long start = (long)(us * (float)ceiling);
    start = start < H - n_steps ? start : H - n_steps;
    if (w == ceiling - 1) start = ceiling;     // the final window of the episode
    return start < H - n_steps ? start : H - n_steps;
}

// window row r = (b, w) of the batch, read from ring slot `ep`: the body k_sample_windows and k_gather_windows share
__device__ __forceinline__ void window_row(const Ring& g, long ep, float us, bool none, int B, int H, int n_steps, int r, int w, int lane,
                                           float* __restrict__ next_ends, float* __restrict__ state, float* __restrict__ action,
                                           float* __restrict__ next_state, float* __restrict__ reward, float* __restrict__ not_done,
                                           float* weight, float real_weight = 1.0f) {
    const int W = H - n_steps;
    const float *ep_state = g.ep_state, *ep_next = g.ep_next, *ep_action = g.ep_action, *ep_reward = g.ep_reward, *ep_not_done = g.ep_not_done;
    long ceiling;
    const long start = window_start(g, ep, us, H, n_steps, w, ceiling);
    const long src = ep * H + start, dst = (long)r * n_steps;
    for (int k = lane; k < n_steps * S; k += WAVE) {
        state[dst * S + k] = ep_state[src * S + k];
        next_state[dst * S + k] = ep_next[src * S + k];
    }
    // the rows the target networks evaluate (DDPGfD.py:256-275: next_state[:, 0] and next_state[:, -1]) as one [2 B W, 82] block
    if (next_ends != nullptr) {
        for (int k = lane; k < S; k += WAVE) {
            next_ends[(long)r * S + k] = ep_next[src * S + k];
            next_ends[((long)B * W + r) * S + k] = ep_next[(src + n_steps - 1) * S + k];
        }
    }
    for (int k = lane; k < n_steps * A; k += WAVE) action[dst * A + k] = ep_action[src * A + k];
    if (lane < n_steps) {
        reward[dst + lane] = ep_reward[src + lane];
        not_done[dst + lane] = ep_not_done[src + lane];
    }
    if (lane == 0) weight[r] = (!none && w < ceiling) ? real_weight : 0.0f;
}

// one wave per window row (b, w); episodes b < B_agent are drawn from ring `ra`, the others from ring `re` (the expert
// demonstrations DDPGfD mixes into every batch, DDPGfD.py:232-254; B_agent = B: one ring)
__global__ __launch_bounds__(WAVE) void k_sample_windows(int B, int B_agent, int H, int n_steps, Ring ra, Ring re, const float* __restrict__ u_ep,
                                                         const float* __restrict__ u_start, unsigned long long seed,
                                                         const int64_t* __restrict__ draw, float* __restrict__ next_ends,
                                                         float* __restrict__ state, float* __restrict__ action, float* __restrict__ next_state,
                                                         float* __restrict__ reward, float* __restrict__ not_done, float* __restrict__ weight) {
    const int W = H - n_steps;
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= B * W) return;
    const int b = r / W, w = r % W;
    const Ring& g = b < B_agent ? ra : re;
    const long cnt = g.count[0];
    const float ue = sample_uniform(u_ep, b, 0x5a4du, seed, draw);
    const float us = sample_uniform(u_start, r, 0x5a4eu, seed, draw);
    const long ep = uniform_episode(ue, cnt, g.head[0], g.capacity);
    window_row(g, ep, us, cnt < 2, B, H, n_steps, r, w, lane, next_ends, state, action, next_state, reward, not_done, weight);
}

// The batch as episode tables (kr_sample_tables_*): the window samplers' draws - the same uniforms, picks and window_start - but each batch
// episode's H ring rows are copied ONCE (table_state / table_next [B * H, S], table_action [B * H, A], rows b * H + t) and a window row is
// its first table row (row_table [B * W]).  A batch's B * W * n window states are drawn from these B * H rows, so what the learner computes
// per state it computes once per table row.  Per window row only what the critic phase reads at R = B * W rows is written: state0, action0,
// reward, not_done, weight; slot_weight [B] is the weight a real window row of slot b carries (real_weight: 1, or the episode's importance
// weight).  Wave (b, w) copies the table rows w, w + W, ... of its episode.  table_row: window row r = (b, w) read from ring slot `ep`, the
// body k_sample_tables and k_gather_tables share.
struct Tables {
    float *table_state, *table_next, *table_action;
    int* row_table;
    float *slot_weight, *state0, *action0, *reward, *not_done, *weight, *next_ends;
};

__device__ __forceinline__ void table_row(const Ring& g, long ep, float us, bool none, int B, int H, int n_steps, int r, int b, int w, int lane,
                                          float real_weight, const Tables& o) {
    const int W = H - n_steps;
    long ceiling;
    const long start = window_start(g, ep, us, H, n_steps, w, ceiling);
    for (int t = w; t < H; t += W) {
        const long src = (ep * H + t) * S, dst = ((long)b * H + t) * S;
        for (int k = lane; k < S; k += WAVE) {
            o.table_state[dst + k] = g.ep_state[src + k];
            o.table_next[dst + k] = g.ep_next[src + k];
        }
        if (lane < A) o.table_action[((long)b * H + t) * A + lane] = g.ep_action[(ep * H + t) * A + lane];
    }
    const long src = ep * H + start;
    for (int k = lane; k < S; k += WAVE) o.state0[(long)r * S + k] = g.ep_state[src * S + k];
    // (a TD3fD learner's target pass keeps the window form's [2 B W, S] rows: its smoothing noise is keyed by the row)
    if (o.next_ends != nullptr) {
        for (int k = lane; k < S; k += WAVE) {
            o.next_ends[(long)r * S + k] = g.ep_next[src * S + k];
            o.next_ends[((long)B * W + r) * S + k] = g.ep_next[(src + n_steps - 1) * S + k];
        }
    }
    if (lane < A) o.action0[(long)r * A + lane] = g.ep_action[src * A + lane];
    if (lane < n_steps) {
        o.reward[(long)r * n_steps + lane] = g.ep_reward[src + lane];
        o.not_done[(long)r * n_steps + lane] = g.ep_not_done[src + lane];
    }
    if (lane == 0) {
        o.weight[r] = (!none && w < ceiling) ? real_weight : 0.0f;
        o.row_table[r] = b * H + (int)start;
        if (w == 0) o.slot_weight[b] = real_weight;
    }
}

__global__ __launch_bounds__(WAVE) void k_sample_tables(int B, int B_agent, int H, int n_steps, Ring ra, Ring re, const float* __restrict__ u_ep,
                                                        const float* __restrict__ u_start, unsigned long long seed,
                                                        const int64_t* __restrict__ draw, Tables o) {
    const int W = H - n_steps;
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= B * W) return;
    const int b = r / W, w = r % W;
    const Ring& g = b < B_agent ? ra : re;
    const long cnt = g.count[0];
    const float ue = sample_uniform(u_ep, b, 0x5a4du, seed, draw);
    const float us = sample_uniform(u_start, r, 0x5a4eu, seed, draw);
    const long ep = uniform_episode(ue, cnt, g.head[0], g.capacity);
    table_row(g, ep, us, cnt < 2, B, H, n_steps, r, b, w, lane, 1.0f, o);
}

// The table gather behind a pick (kr_sample_tables_balanced, _prioritized, _balanced_prioritized): k_gather_windows' part with the episode
// in picked[b].  with_weight: the pick left the episode's importance weight in every row of o.weight; each wave reads its own element
// before it writes the row's weight there and touches no other.
__global__ __launch_bounds__(WAVE) void k_gather_tables(int B, int B_agent, int H, int n_steps, Ring ra, Ring re, const int* __restrict__ picked,
                                                        int with_weight, const float* __restrict__ u_start, unsigned long long seed,
                                                        const int64_t* __restrict__ draw, Tables o) {
    const int W = H - n_steps;
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= B * W) return;
    const int b = r / W, w = r % W;
    const Ring& g = b < B_agent ? ra : re;
    long ep = picked[b];
    ep = ep < 0 ? 0 : (ep < g.capacity ? ep : g.capacity - 1);      // (the pick launch wrote a slot of this ring)
    const float real_weight = with_weight ? o.weight[r] : 1.0f;
    const float us = sample_uniform(u_start, r, 0x5a4eu, seed, draw);
    table_row(g, ep, us, g.count[0] < 2, B, H, n_steps, r, b, w, lane, real_weight, o);
}

// ---- replay batches balanced over the episodes' classes (kr_sample_windows_balanced): the pick and the gather.
// One wave per workgroup and no LDS, as everything on the learner's stream (see wave_sum below).
//
// scan_tags walks tags[s0, s1) - one contiguous piece of a ring's eligible range, in age order - for the tag `c`.  A trip is 64 lanes x 4
// consecutive tags, one 16-byte load per lane where the four lie inside the piece (the first and last vector of a piece, and a table that
// is not 16-byte aligned, are covered by per-tag loads of the elements inside it: nothing outside [s0, s1) is read); the match flags become
// counts through four 64-bit ballots per trip.  The loads of the next SCAN_TRIPS trips are issued before the ballots of the current
// ones: a table of 16 384 tags is 64 KB in L2, what costs is the number of dependent round trips - 8 for it.
//   LOCATE = false: returns how many tags equal c.
//   LOCATE = true:  returns the index of the target-th (0-based, age order) tag that equals c, -1 if there are not that many.
// The result is the same in every lane.
constexpr int SCAN_TRIPS = 8;
typedef int v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4i load_tags(const int* __restrict__ tags, long q, long mis, long s0, long s1, long q1) {
    v4i v = {-1, -1, -1, -1};                        // (-1 equals no wanted class: 0 <= c)
    if (q >= q1) return v;
    const long e0 = 4 * q - mis;
    if (e0 >= s0 && e0 + 4 <= s1) return *(const v4i*)(tags + e0);
    if (e0 + 0 >= s0 && e0 + 0 < s1) v.x = tags[e0 + 0];
    if (e0 + 1 >= s0 && e0 + 1 < s1) v.y = tags[e0 + 1];
    if (e0 + 2 >= s0 && e0 + 2 < s1) v.z = tags[e0 + 2];
    if (e0 + 3 >= s0 && e0 + 3 < s1) v.w = tags[e0 + 3];
    return v;
}

template <bool LOCATE>
__device__ __forceinline__ long scan_tags(const int* __restrict__ tags, long s0, long s1, int c, long target, int lane) {
    if (s1 <= s0) return LOCATE ? -1 : 0;
    const long mis = (long)(((uintptr_t)tags >> 2) & 3);            // tags + e is 16-byte aligned where (e + mis) % 4 == 0
    const long q0 = (s0 + mis) >> 2, q1 = (s1 + mis + 3) >> 2;      // the 16-byte vectors [q0, q1) cover the piece
    constexpr long GROUP = (long)SCAN_TRIPS * WAVE;
    v4i cur[SCAN_TRIPS], nxt[SCAN_TRIPS];
#pragma unroll
    for (int u = 0; u < SCAN_TRIPS; u++) cur[u] = load_tags(tags, q0 + u * WAVE + lane, mis, s0, s1, q1);
    long seen = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long g0 = q0; g0 < q1; g0 += GROUP) {
        const bool more = g0 + GROUP < q1;
        if (more) {
#pragma unroll
            for (int u = 0; u < SCAN_TRIPS; u++) nxt[u] = load_tags(tags, g0 + GROUP + u * WAVE + lane, mis, s0, s1, q1);
        }
#pragma unroll
        for (int u = 0; u < SCAN_TRIPS; u++) {
            const bool m0 = cur[u].x == c, m1 = cur[u].y == c, m2 = cur[u].z == c, m3 = cur[u].w == c;
            const unsigned long long b0 = __ballot(m0), b1 = __ballot(m1), b2 = __ballot(m2), b3 = __ballot(m3);
            const long tot = __popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3);
            if (LOCATE && target < seen + tot) {
                // age order within a trip: lane by lane, the lane's four tags in turn
                long rest = target - seen - (__popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below) + __popcll(b3 & below));
                const int mine = (int)m0 + (int)m1 + (int)m2 + (int)m3;
                const bool owner = rest >= 0 && rest < mine;
                int k = 0;
                if (owner) {
                    if (m0) { if (rest == 0) k = 0; rest--; }
                    if (m1) { if (rest == 0) k = 1; rest--; }
                    if (m2) { if (rest == 0) k = 2; rest--; }
                    if (m3) { if (rest == 0) k = 3; rest--; }
                }
                const int at = (int)(4 * (g0 + u * WAVE + lane) - mis) + k;
                const unsigned long long who = __ballot(owner);          // exactly one lane
                return (long)__shfl(at, __ffsll((long long)who) - 1);
            }
            seen += tot;
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < SCAN_TRIPS; u++) cur[u] = nxt[u];
        }
    }
    return LOCATE ? -1 : seen;
}

// The pick: one wave per batch episode b.  Its class is c = (i + rotation + draw) mod n_classes for its index i within its ring's segment
// of the batch (the Latin square's cyclic rotation, moved from collection to sampling); among the m_c eligible episodes of that class -
// the count - 1 oldest of the ring, ages 0 .. count - 2 in slots head - count + age mod capacity: one or two contiguous pieces of the tag
// table - it takes the floor(ue * m_c)-th oldest, and where the class has none the slot k_sample_windows would take.  Writes the slot
// to picked[b] (row_major == 0) or to picked[b * W + w] for every row w of the episode (row_major != 0: the scratch form, see
// kr_sample_windows_balanced); never touches episode data.
__global__ __launch_bounds__(WAVE) void k_pick_balanced(int B, int B_agent, int W, Ring ra, Ring re, const int* __restrict__ agent_class,
                                                        const int* __restrict__ expert_class, int n_classes, int rotation,
                                                        const float* __restrict__ u_ep, unsigned long long seed,
                                                        const int64_t* __restrict__ draw, int* __restrict__ picked, int row_major) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const bool is_agent = b < B_agent;
    const Ring& g = is_agent ? ra : re;
    const int* tags = is_agent ? agent_class : expert_class;
    const long cnt = g.count[0], head = g.head[0];
    const int capacity = g.capacity;
    const float ue = sample_uniform(u_ep, b, 0x5a4du, seed, draw);
    long want = (long)(b - (is_agent ? 0 : B_agent)) + rotation + (draw != nullptr ? draw[0] : 0);
    want %= n_classes;
    const int c = (int)(want < 0 ? want + n_classes : want);
    long first = (head - cnt) % capacity;
    first = first < 0 ? first + capacity : first;
    const long eligible = cnt - 1 > 0 ? cnt - 1 : 0;                            // <= capacity - 1
    const long end_a = first + eligible < capacity ? first + eligible : capacity;   // piece A: slots [first, end_a), the older ones
    const long end_b = first + eligible - end_a;                                // piece B: slots [0, end_b) behind the wrap
    const long m_a = scan_tags<false>(tags, first, end_a, c, 0, lane);
    const long m_c = m_a + scan_tags<false>(tags, 0, end_b, c, 0, lane);
    long ep;
    if (m_c > 0) {
        long j = (long)(ue * (float)m_c);
        j = j < m_c - 1 ? j : m_c - 1;
        ep = j < m_a ? scan_tags<true>(tags, first, end_a, c, j, lane) : scan_tags<true>(tags, 0, end_b, c, j - m_a, lane);
    } else {
        ep = uniform_episode(ue, cnt, head, capacity);
    }
    if (row_major == 0) {
        if (lane == 0) picked[b] = (int)ep;
    } else {
        for (int w = lane; w < W; w += WAVE) picked[(long)b * W + w] = (int)ep;
    }
}

// The gather: k_sample_windows' rows with the episode supplied - picked[b], or (row_major != 0) picked[r * row_major], which may lie in
// an output of the call itself - the weight column (row_major 1) or, for the prioritized sampler, the first reward of the row (row_major
// n_steps): every wave reads its own element before it writes it and touches no other (hence no __restrict__ on these).  row_weight (NULL:
// 1, the other samplers' path) holds, per window row, the weight a real row gets; it may be the weight column itself, read the same way.
__global__ __launch_bounds__(WAVE) void k_gather_windows(int B, int B_agent, int H, int n_steps, Ring ra, Ring re, const int* picked,
                                                         int row_major, const float* __restrict__ u_start, unsigned long long seed,
                                                         const int64_t* __restrict__ draw, float* __restrict__ next_ends,
                                                         float* __restrict__ state, float* __restrict__ action, float* __restrict__ next_state,
                                                         float* reward, float* __restrict__ not_done, float* weight, const float* row_weight) {
    const int W = H - n_steps;
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= B * W) return;
    const int b = r / W, w = r % W;
    const Ring& g = b < B_agent ? ra : re;
    long ep = picked[row_major != 0 ? (long)r * row_major : (long)b];
    ep = ep < 0 ? 0 : (ep < g.capacity ? ep : g.capacity - 1);      // (the pick launch wrote a slot of this ring)
    const float real_weight = row_weight != nullptr ? row_weight[r] : 1.0f;
    const float us = sample_uniform(u_start, r, 0x5a4eu, seed, draw);
    window_row(g, ep, us, g.count[0] < 2, B, H, n_steps, r, w, lane, next_ends, state, action, next_state, reward, not_done, weight, real_weight);
}

// kr_commit_classes: the class tag of every kept env into kr_commit_episodes' slot
__global__ __launch_bounds__(WAVE) void k_commit_classes(int n, int capacity, const uint8_t* __restrict__ keep, const int64_t* __restrict__ rank,
                                                         const int64_t* __restrict__ head, const int* __restrict__ env_class,
                                                         int* __restrict__ ep_class) {
    const int i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n || keep[i] == 0) return;
    ep_class[(head[0] + rank[i] - 1) % capacity] = env_class[i];
}

// ---- prioritized episode replay (kr_commit_priorities, kr_sample_windows_prioritized, kr_update_priorities).  One wave per workgroup, no
// LDS, vector loads / stores and one vector atomic only, as everything on the learner's stream (see wave_sum below).  A priority is a
// uint32 in units of 1 / 65536; a stored 0 reads as 1, so every eligible episode has a positive share and sums of at most 2^20 of them
// stay below 2^52: exact as uint64 and as double.
//
// The table walk has scan_tags' shape with the ragged ends taken out of the loop.  A piece [s0, s1) of the table is a head of up to three
// priorities in front of the first 16-byte boundary, whole 16-byte vectors, and a tail of up to three; head and tail are read element
// by element, the same elements in every lane.  A trip is 64 lanes x one vector, a group PRIO_TRIPS trips (1536 priorities); the loads of
// the next group are issued before the current one is reduced.  Six trips, not scan_tags' eight: two groups of vectors, their addresses and
// the 64-bit sums fit the 96 registers a learner wave has beside the 400-300 rollout kernel, with eight they do not.  Nothing outside the
// piece is read.  Indices are ints: a table has at most 2^20 slots.
constexpr int PRIO_TRIPS = 6;
typedef unsigned int v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t at_least_one(uint32_t p) { return p > 1u ? p : 1u; }

struct PrioPiece { int s0, ha, hb, s1, qa, qb, mis; };      // head [s0, ha), vectors [qa, qb) = elements [ha, hb), tail [hb, s1)

__device__ __forceinline__ PrioPiece prio_piece(const uint32_t* tab, int s0, int s1) {
    PrioPiece p;
    p.mis = (int)(((uintptr_t)tab >> 2) & 3);                       // tab + e is 16-byte aligned where (e + mis) % 4 == 0
    p.s0 = s0; p.s1 = s1;
    p.qa = (s0 + p.mis + 3) >> 2; p.qb = (s1 + p.mis) >> 2;
    p.ha = min(s1, 4 * p.qa - p.mis);
    p.hb = max(p.ha, 4 * p.qb - p.mis);
    p.qb = max(p.qa, p.qb);
    return p;
}

// element e if it lies in [lo, hi), else 0 (a priority inside reads as at least 1)
__device__ __forceinline__ uint32_t prio_at(const uint32_t* __restrict__ tab, int e, int lo, int hi) {
    return e >= lo && e < hi ? at_least_one(tab[e]) : 0u;
}

// vector q of a piece that has one (qa < qb), in two steps so that a group's loads can be issued back to back: the load itself is
// unconditional - beyond the piece's last vector, of that one - and what it brought is put right afterwards, 0 beyond the last vector
__device__ __forceinline__ uint32_t prio_first(int q, const PrioPiece& p) {
    return (uint32_t)(4 * (q < p.qb ? q : p.qb - 1) - p.mis);                  // (>= s0 >= 0; unsigned: a 32-bit offset to a uniform base)
}

__device__ __forceinline__ v4u prio_raw(const uint32_t* __restrict__ tab, int q, const PrioPiece& p) {
    return *(const v4u*)(tab + prio_first(q, p));
}

__device__ __forceinline__ v4u prio_fix(v4u v, int q, const PrioPiece& p) {
    const bool inside = q < p.qb;
    v.x = inside ? at_least_one(v.x) : 0u; v.y = inside ? at_least_one(v.y) : 0u;
    v.z = inside ? at_least_one(v.z) : 0u; v.w = inside ? at_least_one(v.w) : 0u;
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long x) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

__device__ __forceinline__ unsigned long long sum4(v4u v) {
    return (unsigned long long)v.x + (unsigned long long)v.y + (unsigned long long)v.z + (unsigned long long)v.w;
}

__device__ __forceinline__ uint32_t min_inside(uint32_t m, uint32_t p) { return p != 0u && p < m ? p : m; }

// The walk under a class mask (MASKED, kr_sample_windows_balanced_prioritized): an episode whose tag is not `c` counts with priority 0 - it adds
// nothing to the sum, is no candidate for the minimum and is never located; with `all` set every episode counts, the unmasked walk's
// results.  The tags of a vector's four episodes come with one 16-byte load where the two tables sit alike relative to a 16-byte boundary
// (`aligned`), else with four loads of the same elements: the vectors are the priority table's, and nothing outside the piece is read of
// either table.  MASKED_TRIPS trips to a group: two groups of vectors of BOTH tables in the registers PRIO_TRIPS trips of one table take.
constexpr int MASKED_TRIPS = 3;
struct ClassMask { const int* tags; int c; bool all, aligned; };

__device__ __forceinline__ ClassMask class_mask(const int* tags, const uint32_t* tab, int c, bool all) {
    return ClassMask{tags, c, all, ((((uintptr_t)tags ^ (uintptr_t)tab) >> 2) & 3) == 0};
}

__device__ __forceinline__ v4i tags_raw(int q, const PrioPiece& p, const ClassMask& m) {
    const int* at = m.tags + prio_first(q, p);
    if (m.aligned) return *(const v4i*)at;
    return v4i{at[0], at[1], at[2], at[3]};
}

__device__ __forceinline__ v4u prio_masked(v4u v, v4i t, const ClassMask& m) {
    v.x = m.all || t.x == m.c ? v.x : 0u; v.y = m.all || t.y == m.c ? v.y : 0u;
    v.z = m.all || t.z == m.c ? v.z : 0u; v.w = m.all || t.w == m.c ? v.w : 0u;
    return v;
}

// prio_at under the mask
template <bool MASKED>
__device__ __forceinline__ uint32_t prio_edge(const uint32_t* __restrict__ tab, int e, int lo, int hi, const ClassMask& m) {
    uint32_t x = prio_at(tab, e, lo, hi);
    if constexpr (MASKED) {
        if (x != 0u && !m.all && m.tags[e] != m.c) x = 0u;                      // (x != 0: e lies inside)
    }
    return x;
}

// prio_fix under the mask, t the vector's tags
template <bool MASKED>
__device__ __forceinline__ v4u prio_value(v4u v, v4i t, int q, const PrioPiece& p, const ClassMask& m) {
    v = prio_fix(v, q, p);
    if constexpr (MASKED) v = prio_masked(v, t, m);
    return v;
}

// the sum and the minimum of the piece's priorities (MASKED: of those the mask m lets through): lane partials only (integers: exact in any
// order), the caller reduces over the wave
template <int TRIPS = PRIO_TRIPS, bool MASKED = false>
__device__ __forceinline__ void prio_total(const uint32_t* __restrict__ tab, int s0, int s1, int lane, unsigned long long& sum, uint32_t& least,
                                           const ClassMask& m = ClassMask{}) {
    if (s1 <= s0) return;
    const PrioPiece p = prio_piece(tab, s0, s1);
    const uint32_t edge = lane < 3 ? prio_edge<MASKED>(tab, p.s0 + lane, p.s0, p.ha, m)
                                   : (lane < 6 ? prio_edge<MASKED>(tab, p.hb + lane - 3, p.hb, p.s1, m) : 0u);
    sum += edge;
    least = min_inside(least, edge);
    if (p.qa >= p.qb) return;
    constexpr int GROUP = TRIPS * WAVE;
    v4u cur[TRIPS], nxt[TRIPS];
    v4i tcur[TRIPS] = {}, tnxt[TRIPS] = {};                                     // (the tags: MASKED only)
#pragma unroll
    for (int u = 0; u < TRIPS; u++) {
        cur[u] = prio_raw(tab, p.qa + u * WAVE + lane, p);
        if constexpr (MASKED) tcur[u] = tags_raw(p.qa + u * WAVE + lane, p, m);
    }
    for (int g0 = p.qa; g0 < p.qb; g0 += GROUP) {
#pragma unroll
        for (int u = 0; u < TRIPS; u++) {
            nxt[u] = prio_raw(tab, g0 + GROUP + u * WAVE + lane, p);
            if constexpr (MASKED) tnxt[u] = tags_raw(g0 + GROUP + u * WAVE + lane, p, m);
        }
#pragma unroll
        for (int u = 0; u < TRIPS; u++) {
            const v4u v = prio_value<MASKED>(cur[u], tcur[u], g0 + u * WAVE + lane, p, m);
            sum += sum4(v);
            least = min_inside(min_inside(min_inside(min_inside(least, v.x), v.y), v.z), v.w);
        }
#pragma unroll
        for (int u = 0; u < TRIPS; u++) { cur[u] = nxt[u]; tcur[u] = tnxt[u]; }
    }
}

// the index, within the table, of the piece's first element - age order: the head, then trip by trip, lane by lane, the lane's four in turn,
// then the tail - whose inclusive prefix sum over the piece exceeds `target` (< the piece's sum, so there is one; -1 otherwise), and its
// priority.  One wave sum per group; the group that holds the target is then read once more and taken apart trip by trip, and its one trip
// lane by lane.  The same in every lane.  MASKED: the priorities as the mask m leaves them; an episode it hides is never the one named.
template <int TRIPS = PRIO_TRIPS, bool MASKED = false>
__device__ __forceinline__ int prio_locate(const uint32_t* __restrict__ tab, int s0, int s1, unsigned long long target, int lane, uint32_t& prio,
                                           const ClassMask& m = ClassMask{}) {
    if (s1 <= s0) return -1;
    const PrioPiece p = prio_piece(tab, s0, s1);
    unsigned long long seen = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const uint32_t x = prio_edge<MASKED>(tab, p.s0 + i, p.s0, p.ha, m);
        if (x != 0u && target < seen + x) { prio = x; return p.s0 + i; }
        seen += x;
    }
    constexpr int GROUP = TRIPS * WAVE;
    int hit_group = -1;
    if (p.qa < p.qb) {
        v4u cur[TRIPS], nxt[TRIPS];
        v4i tcur[TRIPS] = {}, tnxt[TRIPS] = {};
#pragma unroll
        for (int u = 0; u < TRIPS; u++) {
            cur[u] = prio_raw(tab, p.qa + u * WAVE + lane, p);
            if constexpr (MASKED) tcur[u] = tags_raw(p.qa + u * WAVE + lane, p, m);
        }
        for (int g0 = p.qa; g0 < p.qb; g0 += GROUP) {
#pragma unroll
            for (int u = 0; u < TRIPS; u++) {
                nxt[u] = prio_raw(tab, g0 + GROUP + u * WAVE + lane, p);
                if constexpr (MASKED) tnxt[u] = tags_raw(g0 + GROUP + u * WAVE + lane, p, m);
            }
            unsigned long long mine = 0;
#pragma unroll
            for (int u = 0; u < TRIPS; u++) mine += sum4(prio_value<MASKED>(cur[u], tcur[u], g0 + u * WAVE + lane, p, m));
            const unsigned long long group = wave_sum_u64(mine);
            if (target < seen + group) { hit_group = g0; break; }             // (wave-uniform)
            seen += group;
#pragma unroll
            for (int u = 0; u < TRIPS; u++) { cur[u] = nxt[u]; tcur[u] = tnxt[u]; }
        }
    }
    if (hit_group >= 0) {
        v4u grp[TRIPS];
        v4i tgrp[TRIPS] = {};
#pragma unroll
        for (int u = 0; u < TRIPS; u++) {
            grp[u] = prio_raw(tab, hit_group + u * WAVE + lane, p);
            if constexpr (MASKED) tgrp[u] = tags_raw(hit_group + u * WAVE + lane, p, m);
        }
        v4u hit = {0u, 0u, 0u, 0u};
        int trip = 0;
        bool found = false;
#pragma unroll
        for (int u = 0; u < TRIPS; u++) {
            const v4u v = prio_value<MASKED>(grp[u], tgrp[u], hit_group + u * WAVE + lane, p, m);
            const unsigned long long tot = wave_sum_u64(sum4(v));
            if (!found && target < seen + tot) { hit = v; trip = hit_group + u * WAVE; found = true; }
            if (!found) seen += tot;
        }
        const unsigned long long own = sum4(hit);
        unsigned long long incl = own;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        unsigned long long rest = target - seen;                         // < the trip's sum
        const bool owner = rest >= incl - own && rest < incl;             // exactly one lane
        rest -= incl - own;
        int k = 3;
        if (owner) {
            if (rest < hit.x) k = 0;
            else if (rest < (unsigned long long)hit.x + hit.y) k = 1;
            else if (rest < (unsigned long long)hit.x + hit.y + hit.z) k = 2;
        }
        const uint32_t x = k == 0 ? hit.x : (k == 1 ? hit.y : (k == 2 ? hit.z : hit.w));
        const int at = 4 * (trip + lane) - p.mis + k;
        const int src = __ffsll((long long)__ballot(owner)) - 1;
        prio = (uint32_t)__shfl((int)x, src);
        return __shfl(at, src);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const uint32_t x = prio_edge<MASKED>(tab, p.hb + i, p.hb, p.s1, m);
        if (x != 0u && target < seen + x) { prio = x; return p.hb + i; }
        seen += x;
    }
    return -1;
}

// The pick: one wave per batch episode b.  Over the eligible episodes of its ring - the count - 1 oldest, one or two contiguous pieces of the
// priority table in age order - T is the sum of the priorities and the target t = min(T - 1, (uint64)((double)ue * (double)T)); the episode
// taken is the one at the smallest age whose inclusive prefix sum exceeds t.  Its importance weight powf(p_min / p_b, beta) goes to EVERY
// row of the episode in `weight`, where the gather finds it; the slot to picked[b], or (picked NULL) into the first reward of every row of
// the episode, as an int.  Never touches episode data.
__global__ __launch_bounds__(WAVE) void k_pick_prioritized(int B, int B_agent, int W, int n_steps, Ring ra, Ring re, const uint32_t* __restrict__ agent_prio,
                                                           const uint32_t* __restrict__ expert_prio, const float* __restrict__ beta,
                                                           const float* __restrict__ u_ep, unsigned long long seed,
                                                           const int64_t* __restrict__ draw, int* __restrict__ picked, float* __restrict__ reward,
                                                           float* __restrict__ weight) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const bool is_agent = b < B_agent;
    const Ring& g = is_agent ? ra : re;
    const uint32_t* tab = is_agent ? agent_prio : expert_prio;
    const long cnt = g.count[0], head = g.head[0];
    const int capacity = g.capacity;
    const float ue = sample_uniform(u_ep, b, 0x5a4du, seed, draw);
    long first = (head - cnt) % capacity;
    first = first < 0 ? first + capacity : first;
    long eligible = cnt - 1 > 0 ? cnt - 1 : 0;
    eligible = eligible < capacity ? eligible : capacity - 1;                   // (count <= capacity)
    const long end_a = first + eligible < capacity ? first + eligible : capacity;   // piece A: slots [first, end_a), the older ones
    const long end_b = first + eligible - end_a;                                // piece B: slots [0, end_b) behind the wrap
    long ep = -1;
    float wb = 1.0f;
    if (eligible > 0) {
        unsigned long long sa = 0, sb = 0;
        uint32_t least = 0xffffffffu;
#pragma nounroll
        for (int piece = 0; piece < 2; piece++) {                                   // (one copy of the walk's code and of its registers)
            unsigned long long sum = 0;
            prio_total(tab, piece ? 0 : (int)first, (int)(piece ? end_b : end_a), lane, sum, least);
            if (piece) sb = sum; else sa = sum;
        }
        const unsigned long long t_a = wave_sum_u64(sa), total = t_a + wave_sum_u64(sb);
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)least, o);
            least = other < least ? other : least;
        }
        unsigned long long t = (unsigned long long)__dmul_rn((double)ue, (double)total);
        t = t < total - 1 ? t : total - 1;
        uint32_t p = least;
        const bool older = t < t_a;
        ep = prio_locate(tab, older ? (int)first : 0, (int)(older ? end_a : end_b), older ? t : t - t_a, lane, p);
        wb = powf((float)least / (float)p, beta[0]);
    }
    if (ep < 0) ep = uniform_episode(ue, cnt, head, capacity);
    for (int w = lane; w < W; w += WAVE) {
        weight[(long)b * W + w] = wb;
        if (picked == nullptr) ((int*)reward)[((long)b * W + w) * n_steps] = (int)ep;
    }
    if (picked != nullptr && lane == 0) picked[b] = (int)ep;
}

// The pick of kr_sample_windows_balanced_prioritized: k_pick_balanced's class c for the slot, then k_pick_prioritized's rule over the eligible
// episodes tagged c alone - their sum T_c, their minimum, the episode at the smallest age whose inclusive prefix sum of the masked priorities
// exceeds t, the weight powf(pmin_c / p_b, beta).  Where no eligible episode is tagged c (T_c == 0: a priority reads as at least 1) the walk is
// made once more over all of them, which is k_pick_prioritized itself.  Both tables are walked twice, the priority table's vectors setting
// the pace (ClassMask).  Outputs as k_pick_prioritized.
__global__ __launch_bounds__(WAVE) void k_pick_balanced_prioritized(int B, int B_agent, int W, int n_steps, Ring ra, Ring re,
                                                                    const int* __restrict__ agent_class, const int* __restrict__ expert_class,
                                                                    int n_classes, int rotation, const uint32_t* __restrict__ agent_prio,
                                                                    const uint32_t* __restrict__ expert_prio, const float* __restrict__ beta,
                                                                    const float* __restrict__ u_ep, unsigned long long seed,
                                                                    const int64_t* __restrict__ draw, int* __restrict__ picked,
                                                                    float* __restrict__ reward, float* __restrict__ weight) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const bool is_agent = b < B_agent;
    const Ring& g = is_agent ? ra : re;
    const uint32_t* tab = is_agent ? agent_prio : expert_prio;
    const int* tags = is_agent ? agent_class : expert_class;
    const long cnt = g.count[0], head = g.head[0];
    const int capacity = g.capacity;
    const float ue = sample_uniform(u_ep, b, 0x5a4du, seed, draw);
    long want = (long)(b - (is_agent ? 0 : B_agent)) + rotation + (draw != nullptr ? draw[0] : 0);
    want %= n_classes;
    const int c = (int)(want < 0 ? want + n_classes : want);
    long first = (head - cnt) % capacity;
    first = first < 0 ? first + capacity : first;
    long eligible = cnt - 1 > 0 ? cnt - 1 : 0;
    eligible = eligible < capacity ? eligible : capacity - 1;                   // (count <= capacity)
    const long end_a = first + eligible < capacity ? first + eligible : capacity;   // piece A: slots [first, end_a), the older ones
    const long end_b = first + eligible - end_a;                                // piece B: slots [0, end_b) behind the wrap
    long ep = -1;
    float wb = 1.0f;
    if (eligible > 0) {
        unsigned long long t_a = 0, total = 0;
        uint32_t least = 0xffffffffu;
        ClassMask m = class_mask(tags, tab, c, false);
#pragma nounroll
        for (int pass = 0; pass < 4 && (pass < 2 || total == 0); pass++) {          // (passes 0, 1: the class's pieces A, B; 2, 3: everybody's)
            const int piece = pass & 1;
            m.all = pass >= 2;
            unsigned long long sum = 0;
            prio_total<MASKED_TRIPS, true>(tab, piece ? 0 : (int)first, (int)(piece ? end_b : end_a), lane, sum, least, m);
            sum = wave_sum_u64(sum);
            if (!piece) t_a = sum;
            total = piece ? t_a + sum : 0;
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)least, o);
            least = other < least ? other : least;
        }
        unsigned long long t = (unsigned long long)__dmul_rn((double)ue, (double)total);
        t = t < total - 1 ? t : total - 1;
        uint32_t p = least;
        const bool older = t < t_a;
        ep = prio_locate<MASKED_TRIPS, true>(tab, older ? (int)first : 0, (int)(older ? end_a : end_b), older ? t : t - t_a, lane, p, m);
        wb = powf((float)least / (float)p, beta[0]);
    }
    if (ep < 0) ep = uniform_episode(ue, cnt, head, capacity);
    for (int w = lane; w < W; w += WAVE) {
        weight[(long)b * W + w] = wb;
        if (picked == nullptr) ((int*)reward)[((long)b * W + w) * n_steps] = (int)ep;
    }
    if (picked != nullptr && lane == 0) picked[b] = (int)ep;
}

// kr_commit_priorities: a new episode enters its slot at the largest priority any update has written
__global__ __launch_bounds__(WAVE) void k_commit_priorities(int n, int capacity, const uint8_t* __restrict__ keep, const int64_t* __restrict__ rank,
                                                            const int64_t* __restrict__ head, const uint32_t* __restrict__ prio_max,
                                                            uint32_t* __restrict__ ep_prio) {
    const int i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n || keep[i] == 0) return;
    ep_prio[(head[0] + rank[i] - 1) % capacity] = at_least_one(prio_max[0]);
}

// delta_b of kr_update_priorities: the largest 1-step TD error over the real rows of batch episode b (k_critic_grad's t1 and e1), -1 without
// a real row, NaN where a real row's error is NaN.  The same in every lane.
__device__ __forceinline__ float episode_delta(int b, int W, int n, const float* __restrict__ q, const float* __restrict__ tq1,
                                               const float* __restrict__ reward, const float* __restrict__ weight, float discount, int lane) {
#pragma clang fp contract(off)
    float m = -1.0f;
    bool bad = false;
    for (int w = lane; w < W; w += WAVE) {
        const long r = (long)b * W + w;
        if (weight[r] > 0.0f) {
            const float t1 = reward[r * n] + discount * tq1[r];
            const float e = fabsf(q[r] - t1);
            if (e != e) bad = true;
            else m = e > m ? e : m;
        }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const float other = __shfl_xor(m, o);
        m = other > m ? other : m;
    }
    return __ballot(bad) != 0ull ? __builtin_nanf("") : m;
}

// clamp(floor(powf(delta + eps, alpha) * 65536), 1, 2^32 - 1) in fp32, the conversion saturating
__device__ __forceinline__ uint32_t quantise_priority(float delta, float eps, float alpha) {
#pragma clang fp contract(off)
    const float x = floorf(powf(delta + eps, alpha) * 65536.0f);
    return !(x >= 1.0f) ? 1u : (x >= 4294967296.0f ? 0xffffffffu : (uint32_t)x);
}

// One wave per batch episode b: its delta to delta_out; then, unless an earlier batch episode of the segment was read from the same slot
// (that wave writes for both), the largest quantised priority over b and the later batch episodes of the segment with b's slot - their
// deltas recomputed here, duplicates are few - is stored to the slot and offered to the ring's prio_max.  Every slot has one writer and one
// value: nothing depends on the order the waves run in.
__global__ __launch_bounds__(WAVE) void k_update_priorities(int B, int B_agent, int W, int n, const float* __restrict__ q, const float* __restrict__ tq1,
                                                            const float* __restrict__ reward, const float* __restrict__ weight, float discount,
                                                            const int* __restrict__ picked, float alpha, float eps_agent, float eps_expert,
                                                            uint32_t* __restrict__ agent_prio, uint32_t* __restrict__ expert_prio,
                                                            uint32_t* agent_max, uint32_t* expert_max, float* __restrict__ delta_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const bool is_agent = b < B_agent;
    const int b0 = is_agent ? 0 : B_agent, b1 = is_agent ? B_agent : B;
    uint32_t* tab = is_agent ? agent_prio : expert_prio;
    uint32_t* top = is_agent ? agent_max : expert_max;
    const float eps = is_agent ? eps_agent : eps_expert;
    const float d = episode_delta(b, W, n, q, tq1, reward, weight, discount, lane);
    if (delta_out != nullptr && lane == 0) delta_out[b] = d;
    const int s = picked[b];
    if (s < 0) return;
    for (int j0 = b0; j0 < b; j0 += WAVE) {
        const int j = j0 + lane;
        if (__ballot(j < b && picked[j] == s) != 0ull) return;
    }
    uint32_t v = (d >= 0.0f && d < __builtin_inff()) ? quantise_priority(d, eps, alpha) : 0u;       // 0: nothing to write
    for (int j0 = b + 1; j0 < b1; j0 += WAVE) {
        const int j = j0 + lane;
        unsigned long long same = __ballot(j < b1 && picked[j] == s);
        while (same != 0ull) {
            const int k = __ffsll((long long)same) - 1;
            same &= same - 1ull;
            const float dj = episode_delta(j0 + k, W, n, q, tq1, reward, weight, discount, lane);
            if (dj >= 0.0f && dj < __builtin_inff()) {
                const uint32_t vj = quantise_priority(dj, eps, alpha);
                v = vj > v ? vj : v;
            }
        }
    }
    if (v != 0u && lane == 0) {
        tab[s] = v;
        atomicMax(top, v);
    }
}

// ---- learner glue: plain grid-stride elementwise kernels, no fma contraction where the torch expression has none
// (ONE wave, no LDS: the update's body must be able to start beside a stepping kernel that holds ALL of a CU's LDS - with the larger hull
// tables of a mixed-object context not even the 1 KB of a block reduction is left, and a learner whose first kernel waits for LDS only
// runs when persistent workgroups exit: the episodes published meanwhile were dropped, round 4.  The sums are wave butterflies.)
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// TD3's clipped double-Q minimum; NaN if either operand is NaN (a diverged critic stays visible)
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }

// The bounded critic update: the bootstrapped value clamped to [lo, hi] - a NaN fails both comparisons and passes - and the loss shaped as
// twice the Huber function: rho(e) = e^2 where not |e| > d, d (2 |e| - d) otherwise, whose derivative is 2 clamp(e, -d, d).  The square
// branch is the unbounded term in its order, so infinite bounds and an infinite d give the unbounded update's bits.
__device__ __forceinline__ float bound_q(float m, float lo, float hi) { return m < lo ? lo : (m > hi ? hi : m); }
__device__ __forceinline__ float huber_clip(float e, float d) { return fabsf(e) > d ? (e < 0.0f ? -d : d) : e; }
__device__ __forceinline__ float huber_term(float w, float e, float d) {
#pragma clang fp contract(off)
    const float a = fabsf(e);
    return a > d ? w * (d * (2.0f * a - d)) : w * e * e;
}

// one critic's share of a row: its 1-step and n-step errors into the loss sums; returns dLoss/dQ of L1 + 0.5 LN
template <bool BOUNDED>
__device__ __forceinline__ float td_row(float q, float t1, float tn, float w, float inv, float d, float& l1, float& ln) {
#pragma clang fp contract(off)
    const float e1 = q - t1, en = q - tn;
    if constexpr (BOUNDED) {
        l1 += huber_term(w, e1, d);
        ln += huber_term(w, en, d);
        return w * inv * (2.0f * huber_clip(e1, d) + 0.5f * 2.0f * huber_clip(en, d));
    } else {
        l1 += w * e1 * e1;
        ln += w * en * en;
        return w * inv * (2.0f * e1 + 0.5f * 2.0f * en);
    }
}

// (critic loss, L1, LN) of one critic from its summed terms
__device__ __forceinline__ void loss_triple(float l1, float ln, float inv, float* out) {
#pragma clang fp contract(off)
    out[1] = l1 * inv; out[2] = ln * inv; out[0] = l1 * inv + 0.5f * (ln * inv);
}

// Targets and critic loss gradient, the one body of kr_critic_grad <false, false>, kr_twin_critic_grad <true, false> and
// kr_critic_grad_bounded <TWIN, true>.  Per row: the bootstrap pair (1-step, n-step) is the target critic's, with TWIN the nan_min of the
// two target critics', with BOUNDED then clamped, and where it is not simply tq1_a / tqn_a it is written to tboot [2R] for the priorities;
// t1 and tn from it; each critic's td_row.  Unused with TWIN = false: q2, tq1_b, tqn_b, dq2, losses[3..5]; with BOUNDED = false: lo, hi,
// delta; with neither: tboot.  A single wave: the batch is a few thousand rows; the masked means are wave reductions.
template <bool TWIN, bool BOUNDED>
__global__ __launch_bounds__(WAVE) void k_critic_grad(int R, int n, const float* __restrict__ q1, const float* __restrict__ q2,
                                                      const float* __restrict__ tq1_a, const float* __restrict__ tq1_b,
                                                      const float* __restrict__ tqn_a, const float* __restrict__ tqn_b,
                                                      const float* __restrict__ reward, const float* __restrict__ weight,
                                                      const float* __restrict__ wsum, float discount, float lo, float hi, float delta,
                                                      float* __restrict__ dq1, float* __restrict__ dq2, float* __restrict__ tboot,
                                                      float* losses) {
#pragma clang fp contract(off)
    const float inv = wsum[0] > 0.0f ? 1.0f / wsum[0] : 0.0f;     // an all-padding batch (empty replay) has zero loss and gradient
    float l1a = 0, lna = 0, l1b = 0, lnb = 0;
    for (int r = threadIdx.x; r < R; r += WAVE) {
        float b1 = tq1_a[r], bn = tqn_a[r];
        if constexpr (TWIN) { b1 = nan_min(b1, tq1_b[r]); bn = nan_min(bn, tqn_b[r]); }
        if constexpr (BOUNDED) { b1 = bound_q(b1, lo, hi); bn = bound_q(bn, lo, hi); }
        if constexpr (TWIN || BOUNDED) { tboot[r] = b1; tboot[(long)R + r] = bn; }
        const float t1 = reward[(long)r * n] + discount * b1;
        float ret = 0, g = 1.0f;
        for (int i = 0; i < n; i++) { ret += g * reward[(long)r * n + i]; g *= discount; }
        const float tn = ret + g * bn;
        const float w = weight ? weight[r] : 1.0f;
        dq1[r] = td_row<BOUNDED>(q1[r], t1, tn, w, inv, delta, l1a, lna);
        if constexpr (TWIN) dq2[r] = td_row<BOUNDED>(q2[r], t1, tn, w, inv, delta, l1b, lnb);
    }
    l1a = wave_sum(l1a);
    lna = wave_sum(lna);
    if constexpr (TWIN) { l1b = wave_sum(l1b); lnb = wave_sum(lnb); }
    if (threadIdx.x == 0) {
        loss_triple(l1a, lna, inv, losses);
        if constexpr (TWIN) loss_triple(l1b, lnb, inv, losses + 3);
    }
}

// TD3's target policy smoothing on the target actor's [rows, 4] output, in place: one thread per row, the row as one 16-byte load / store
__global__ __launch_bounds__(256) void k_target_smooth(int rows, float* __restrict__ action, const float* __restrict__ noise,
                                                       unsigned long long seed, const int64_t* __restrict__ draw, float sigma, float clip,
                                                       float max_action) {
#pragma clang fp contract(off)
    static_assert(A == 4, "one float4 per row");
    const unsigned long long d = draw ? (unsigned long long)draw[0] : 0ull;
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
        const float4 a4 = reinterpret_cast<const float4*>(action)[r];
        float a[A] = {a4.x, a4.y, a4.z, a4.w}, z[A];
        if (noise) {
            const float4 z4 = reinterpret_cast<const float4*>(noise)[r];
            z[0] = z4.x; z[1] = z4.y; z[2] = z4.z; z[3] = z4.w;
        } else {
            krsel::normal4_tagged(seed, d, (uint32_t)r, krsel::TAG_TARGET_SMOOTH, z);
        }
#pragma unroll
        for (int k = 0; k < A; k++) {
            // (a NaN fails every comparison and passes through)
            float e = sigma * z[k];
            e = e < -clip ? -clip : (e > clip ? clip : e);
            const float s = a[k] + e;
            a[k] = s < 0.0f ? 0.0f : (s > max_action ? max_action : s);
        }
        reinterpret_cast<float4*>(action)[r] = make_float4(a[0], a[1], a[2], a[3]);
    }
}

// start of an update's body: what used to be eight tiny library launches (sum, clamp, mul, div, copy, add, fill, copy).  The part
// k_update_prologue and k_update_prologue_tables share: the sum of the weights, the counters; returns dLoss/dQ of the actor loss per unit
// of weight.
__device__ __forceinline__ float prologue_scale(int R, int n, const float* __restrict__ weight, float* __restrict__ wsum, int64_t* it,
                                                int64_t* it_head, int pipelined) {
#pragma clang fp contract(off)
    float s = 0;
    for (int r = threadIdx.x; r < R; r += WAVE) s += weight ? weight[r] : 1.0f;
    s = wave_sum(s);                                  // (0 / 1 weights: exact in any order; every lane holds the total)
    const float total = s > 1.0f ? s : 1.0f;          // exact unless the batch is all padding
    if (threadIdx.x == 0) {
        wsum[0] = total;
        it[0] += 1;                                   // this update's number (Adam bias correction, soft-update phase)
        if (pipelined) it_head[0] = it[0];            // its actor step is applied by the NEXT update's head
    }
    return -1.0f / (total * (float)n);                // d(-sum_r w_r sum_k Q_rk / (sum(w) n)) / dQ_rk
}

__global__ __launch_bounds__(WAVE) void k_update_prologue(int R, int n, const float* __restrict__ weight, float* __restrict__ wsum,
                                                          float* __restrict__ dq_actor, int64_t* it, int64_t* it_head, int pipelined) {
#pragma clang fp contract(off)
    const float scale = prologue_scale(R, n, weight, wsum, it, it_head, pipelined);
    for (int i = threadIdx.x; i < R * n; i += WAVE) dq_actor[i] = (weight ? weight[i / n] : 1.0f) * scale;
}

// The prologue of an update on episode tables (k_sample_tables): dLoss/dQ per TABLE row - every real window row of batch slot b carries
// slot_weight[b], so state (b, t) has the dq of k_update_prologue in every window that holds it - and the table row of each of the R * n
// window states, -1 for the states of a weight-0 (padding) row, whose terms the window form adds as exact zeros.
__global__ __launch_bounds__(WAVE) void k_update_prologue_tables(int R, int n, int B, int H, const float* __restrict__ weight,
                                                                 const float* __restrict__ slot_weight, const int* __restrict__ row_table,
                                                                 float* __restrict__ wsum, float* __restrict__ dq_table,
                                                                 int* __restrict__ row_index, int64_t* it, int64_t* it_head, int pipelined) {
#pragma clang fp contract(off)
    const float scale = prologue_scale(R, n, weight, wsum, it, it_head, pipelined);
    for (int i = threadIdx.x; i < B * H; i += WAVE) dq_table[i] = slot_weight[i / H] * scale;
    for (int r = threadIdx.x; r < R; r += WAVE) {         // (by window row: no division per window state)
        const bool real = weight[r] != 0.0f;
        const int first = row_table[r];
        for (int k = 0; k < n; k++) row_index[(long)r * n + k] = real ? first + k : -1;
    }
}

// the target critic's Q of the table rows -> the [2R] layout the loss-gradient kernels take: the 1-step rows (the window's first next
// state), then the n-step rows (its last)
__global__ __launch_bounds__(WAVE) void k_gather_table_q(int R, int n, const int* __restrict__ row_table, const float* __restrict__ tq_table,
                                                         float* __restrict__ tq) {
    const int r = blockIdx.x * WAVE + threadIdx.x;
    if (r >= R) return;
    tq[r] = tq_table[row_table[r]];
    tq[(long)R + r] = tq_table[row_table[r] + n - 1];
}

__global__ __launch_bounds__(256) void k_relu_backward(long count, const float* __restrict__ act, float* __restrict__ grad) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) grad[i] = act[i] > 0.0f ? grad[i] : 0.0f;
}

__global__ __launch_bounds__(256) void k_sigmoid_scale_backward(long count, const float* __restrict__ a, float max_action, float* __restrict__ grad) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) grad[i] *= a[i] * (1.0f - a[i] / max_action);
}

// The behaviour-cloning term of the actor loss (Nair et al. 2018) added to dLoss/d(actor pre-activation), with its Q-filter: one thread per
// row, the row of each [rows, 4] buffer as one 16-byte load / store.  A row below demo_from, a row the filter rejects and a row whose dq is
// 0 (padding) add nothing, and their dz3 is not stored: it keeps every bit (a -0.0 too, which dz3 + 0 would not).  The order of the
// operations is the contract of include/kinova_rollout.h.
__global__ __launch_bounds__(256) void k_bc_actor_grad(int rows, int demo_from, const float* __restrict__ pi, const float* __restrict__ demo,
                                                       const float* __restrict__ q_demo, const float* __restrict__ q_pi,
                                                       const float* __restrict__ dq, float bc_weight, float max_action, float* __restrict__ dz3,
                                                       float* __restrict__ sq, float* __restrict__ pass) {
#pragma clang fp contract(off)
    static_assert(A == 4, "one float4 per row");
    const float two_w = 2.0f * bc_weight;
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
        if (r < demo_from) { sq[r] = 0.0f; pass[r] = 0.0f; continue; }
        const bool f = q_demo ? q_demo[r] > q_pi[r] : true;          // (strict; a NaN on either side fails the comparison)
        pass[r] = f ? 1.0f : 0.0f;
        if (!f) { sq[r] = 0.0f; continue; }
        const float4 p4 = reinterpret_cast<const float4*>(pi)[r], a4 = reinterpret_cast<const float4*>(demo)[r];
        const float p[A] = {p4.x, p4.y, p4.z, p4.w};
        const float d[A] = {p4.x - a4.x, p4.y - a4.y, p4.z - a4.z, p4.w - a4.w};
        sq[r] = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3];
        const float g = dq[r];
        if (!(g != 0.0f) || !(bc_weight != 0.0f)) continue;          // (a NaN dq is not 0: it reaches the row)
        const float c = two_w * -g;                                  // d(bc term) / d(pi_j) = c * d_j
        const float4 z4 = reinterpret_cast<const float4*>(dz3)[r];
        float z[A] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
        for (int j = 0; j < A; j++) z[j] += (c * d[j]) * (p[j] * (1.0f - p[j] / max_action));
        reinterpret_cast<float4*>(dz3)[r] = make_float4(z[0], z[1], z[2], z[3]);
    }
}

// torch.optim.Adam, single-tensor formulation, as step number t (bias corrections)
// (CLIP: the gradient is g * coef, scaled before the weight-decay term as torch.nn.utils.clip_grad_norm_ does; g itself is not written)
template <bool CLIP = false>
__device__ __forceinline__ void adam_apply(long count, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, float t, float lr, float b1, float b2, float eps, float wd, float coef = 1.0f) {
#pragma clang fp contract(off)
    const float bc1 = 1.0f - powf(b1, t), bc2 = 1.0f - powf(b2, t);
    const float step_size = lr / bc1, bc2s = sqrtf(bc2);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) {
        float gi = g[i];
        if (CLIP) gi = gi * coef;
        if (wd != 0.0f) gi = gi + wd * p[i];
        const float mi = m[i] + (gi - m[i]) * (1.0f - b1);            // exp_avg.lerp_(grad, 1 - beta1)
        const float vi = v[i] * b2 + (1.0f - b2) * gi * gi;           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2s + eps;
        p[i] = p[i] - step_size * (mi / denom);
    }
}

__global__ __launch_bounds__(256) void k_adam_step(long count, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, const int64_t* __restrict__ step, float lr, float b1, float b2,
                                                   float eps, float wd) {
    // bias corrections from the (already incremented) device step
    if (step[0] <= 0) return;                 // no update has produced gradients yet
    adam_apply(count, p, g, m, v, (float)step[0], lr, b1, b2, eps, wd);
}

// TD3's delayed actor: the step of every `every`-th update, numbered step / every; nothing is touched on the others
template <bool CLIP = false>
__device__ __forceinline__ void adam_apply_every(long count, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, const int64_t* __restrict__ step, int every, float lr, float b1,
                                                 float b2, float eps, float wd, float coef = 1.0f) {
    const int64_t s = step[0];
    if (s <= 0 || s % every != 0) return;
    adam_apply<CLIP>(count, p, g, m, v, (float)(s / every), lr, b1, b2, eps, wd, coef);
}

__global__ __launch_bounds__(256) void k_adam_step_every(long count, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, const int64_t* __restrict__ step, int every, float lr, float b1,
                                                         float b2, float eps, float wd) {
    adam_apply_every(count, p, g, m, v, step, every, lr, b1, b2, eps, wd);
}

// Global gradient-norm clip (torch.nn.utils.clip_grad_norm_), two launches.  The squared norm: KR_NORM_PARTS workgroups of one wave, lane l of
// workgroup b sums the exact fp64 squares of g[b 64 + l + 4096 k], k = 0, 1, ... in that order, an xor butterfly gives partials[b]: a function
// of (g, count) alone, whatever the schedule, and no float atomics.  4-byte loads: the flat buffers are sliced.
constexpr int NORM_PARTS = KR_NORM_PARTS;
static_assert(NORM_PARTS == WAVE, "k_adam_step_clipped loads one partial per lane");

__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

__global__ __launch_bounds__(WAVE) void k_grad_sqnorm(long count, const float* __restrict__ g, double* __restrict__ partials) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (long i = (long)blockIdx.x * WAVE + threadIdx.x; i < count; i += (long)NORM_PARTS * WAVE) {
        const double gi = (double)g[i];
        s += gi * gi;
    }
    s = wave_sum_f64(s);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// k_adam_step_every on g * coef, coef = min(max_norm / (norm + 1e-6), 1): every wave sums the same 64 partials by the same butterfly, so all
// hold the same bits.  clip_out (optional) = (norm, coef), written whatever the gate says.
__global__ __launch_bounds__(256) void k_adam_step_clipped(long count, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, const int64_t* __restrict__ step, int every,
                                                           const double* __restrict__ partials, float max_norm, float lr, float b1, float b2,
                                                           float eps, float wd, float* __restrict__ clip_out) {
#pragma clang fp contract(off)
    const double total = wave_sum_f64(partials[threadIdx.x & (WAVE - 1)]);
    const float norm = sqrtf((float)total);
    float coef = max_norm / (norm + 1e-6f);
    coef = coef > 1.0f ? 1.0f : coef;                     // (a NaN stays NaN, as with torch.clamp(max=1))
    if (clip_out && blockIdx.x == 0 && threadIdx.x == 0) { clip_out[0] = norm; clip_out[1] = coef; }
    adam_apply_every<true>(count, p, g, m, v, step, every, lr, b1, b2, eps, wd, coef);
}

__global__ __launch_bounds__(256) void k_soft_update(long count, const float* __restrict__ p, float* __restrict__ tp, float tau,
                                                     const int64_t* __restrict__ it, int freq) {
#pragma clang fp contract(off)
    if (it[0] <= 0 || it[0] % freq != 0) return;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) tp[i] = tau * p[i] + (1.0f - tau) * tp[i];
}

// Running observation normalisation (ddpgfd: obs_norm), three launches of the learner's stream; the arithmetic is the contract of
// include/kinova_rollout.h.  The statistics: ONE workgroup of four waves - every wave reads the scalar count before one of them replaces it,
// which a barrier orders and a second workgroup could not -, one wave per SIMD, so the workgroup is resident within what k_rollout<25,19>
// leaves.  Wave w owns the CW = ceil(dim / 4) adjacent columns from w CW on; its lanes are PH = 64 / CW row phases of CW columns each, so
// that one load covers PH rows of CW adjacent floats (a few cache lines, not one per lane).  Lane (p, c) adds its rows p, p + PH, ... in fp64
// in ascending order; the phases' sums are added in ascending p (the same in every lane); the lanes of phase 0 merge their columns: a
// function of the inputs alone.
constexpr int OBS_WAVES = 4;
constexpr int OBS_MAX_DIM = OBS_WAVES * WAVE;

__device__ __forceinline__ double obs_phase_sum(double x, int cw, int ph, int col) {
#pragma clang fp contract(off)
    double t = 0.0;
    for (int p = 0; p < ph; p++) t += __shfl(x, p * cw + col);        // (uniform trip count; every lane of a column gets the same bits)
    return t;
}

// one lane's pass over its rows p, p + ph, ...: the sum of x (SQ false) or of (x - mb)^2 (SQ true) over the counted rows, in ascending order.
// The loads of OBS_BATCH rows are issued together - every row of the buffer may be read, only what is added depends on the weight -, so a
// pass is rows / (ph OBS_BATCH) memory round trips and not one per row.
constexpr int OBS_BATCH = 16;

template <bool SQ>
__device__ __forceinline__ double obs_column_pass(const float* __restrict__ xc, int lda, const float* __restrict__ weight, int rows, int phase,
                                                  int ph, double mb) {
#pragma clang fp contract(off)
    double acc = 0.0;
    int r = phase;
    for (; r + (OBS_BATCH - 1) * ph < rows; r += OBS_BATCH * ph) {
        float v[OBS_BATCH], w[OBS_BATCH];
#pragma unroll
        for (int u = 0; u < OBS_BATCH; u++) {
            v[u] = xc[(long)(r + u * ph) * lda];
            w[u] = weight ? weight[r + u * ph] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < OBS_BATCH; u++) {
            const double d = SQ ? (double)v[u] - mb : (double)v[u];
            acc += w[u] != 0.0f ? (SQ ? d * d : d) : 0.0;                             // (a padding row's value is never added, a NaN neither)
        }
    }
    for (; r < rows; r += ph) {
        const float v = xc[(long)r * lda];
        const bool on = !weight || weight[r] != 0.0f;
        const double d = SQ ? (double)v - mb : (double)v;
        acc += on ? (SQ ? d * d : d) : 0.0;
    }
    return acc;
}

__global__ __launch_bounds__(OBS_WAVES * WAVE) void k_obs_stats_update(int rows, int dim, const float* __restrict__ x, int lda,
                                                                       const float* __restrict__ weight, const int64_t* __restrict__ it,
                                                                       int64_t freeze_after, double* count, double* __restrict__ mean,
                                                                       double* __restrict__ m2, float* __restrict__ mean32,
                                                                       float* __restrict__ inv32, double eps) {
#pragma clang fp contract(off)
    if (it && freeze_after > 0 && it[0] >= freeze_after) return;                     // frozen: nothing is touched (uniform)
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    double nb = 0.0;                                                                 // counted rows: exact
    for (int r = lane; r < rows; r += WAVE) nb += (!weight || weight[r] != 0.0f) ? 1.0 : 0.0;
    nb = wave_sum_f64(nb);
    const double na = __hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // every wave, before the barrier
    __syncthreads();
    if (!(nb > 0.0)) return;                                                         // all padding: nothing is touched (uniform)
    const double n = na + nb;
    const int cw = (dim + OBS_WAVES - 1) / OBS_WAVES, ph = WAVE / cw;                 // 1 <= cw <= 64
    const int phase = lane / cw, col = lane - phase * cw, c = wave * cw + col;
    const bool mine = phase < ph && c < dim;                                         // (lanes beyond ph * cw, columns beyond dim: idle)
    const float* __restrict__ xc = x + (mine ? c : 0);
    const double s = mine ? obs_column_pass<false>(xc, lda, weight, rows, phase, ph, 0.0) : 0.0;
    const double mb = obs_phase_sum(s, cw, ph, col) / nb;
    double q = mine ? obs_column_pass<true>(xc, lda, weight, rows, phase, ph, mb) : 0.0;
    q = obs_phase_sum(q, cw, ph, col);
    if (mine && phase == 0) {
        // Chan et al.: (na, mean, m2) + (nb, mb, q)
        const double ma = mean[c], delta = mb - ma;
        const double mn = ma + delta * (nb / n);
        const double qn = (m2[c] + q) + (delta * delta) * (na * (nb / n));
        mean[c] = mn;
        m2[c] = qn;
        mean32[c] = (float)mn;
        const double sd = sqrt(qn / n);
        inv32[c] = (float)(1.0 / (sd > eps ? sd : eps));
    }
    if (threadIdx.x == 0) count[0] = n;
}

// in place on the first `dim` columns of every row: one subtract, one multiply (no contraction: the two fp32 operations of the host)
__global__ __launch_bounds__(256) void k_obs_normalize(long rows, int dim, float* __restrict__ x, int lda, const float* __restrict__ mean32,
                                                       const float* __restrict__ inv32) {
#pragma clang fp contract(off)
    const long count = rows * dim;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) {
        const long r = i / dim;
        const int c = (int)(i - r * dim);
        float* p = x + r * lda + c;
        *p = (*p - mean32[c]) * inv32[c];
    }
}

// W1 (x - mean) * inv = (W1 * inv) x + (b1 - (W1 * inv) mean): a thread per output row, the bias sum in fp64 in ascending k, rounded once
__global__ __launch_bounds__(256) void k_fold_obs_norm(int h1, int in_dim, int norm_dim, const float* __restrict__ W1, const float* __restrict__ b1,
                                                       const float* __restrict__ mean32, const float* __restrict__ inv32,
                                                       float* __restrict__ W1_out, float* __restrict__ b1_out) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= h1) return;
    const float* __restrict__ w = W1 + (long)j * in_dim;
    float* __restrict__ wo = W1_out + (long)j * in_dim;
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < norm_dim; k++) {
        const float f = w[k] * inv32[k];
        wo[k] = f;
        acc += (double)f * (double)mean32[k];
    }
    for (int k = norm_dim; k < in_dim; k++) wo[k] = w[k];
    b1_out[j] = (float)((double)b1[j] - acc);
}

// one wave, no LDS: every lane scans its share of the values (agent-scope loads: the writers' stores are device-visible), the wave takes
// the minimum with shuffles; the launch ends when it has reached the target or the wall clock runs out
__global__ __launch_bounds__(64) void k_wait_min(const int64_t* __restrict__ values, int n, int64_t target, long long ticks, int64_t* timeouts) {
    const long long t0 = wall_clock64();
    for (;;) {
        long long m = 0x7fffffffffffffffll;
        for (int i = threadIdx.x; i < n; i += 64) {
            const long long v = __hip_atomic_load(values + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            m = v < m ? v : m;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const long long other = __shfl_xor(m, o);
            m = other < m ? other : m;
        }
        if (m >= target) break;                                                    // (wave-uniform)
        if (ticks > 0 && wall_clock64() - t0 > ticks) {
            if (timeouts && threadIdx.x == 0) atomicAdd((unsigned long long*)timeouts, 1ull);   // a time-out is never silent
            break;
        }
        __builtin_amdgcn_s_sleep(64);
    }
}

inline int grid_for(long count) { long b = (count + 255) / 256; return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b)); }

inline int launched() { return hipGetLastError() == hipSuccess ? KS_OK : KS_ERR_HIP; }

}  // namespace

extern "C" {

int kr_select_action(int32_t n, const float* obs, const float* prev_obs, const uint8_t* has_prev, const int64_t* t, uint8_t* ready,
                     const float* actor_out, const float* noise, float sigma, float max_action, int32_t skip_steps, float* action,
                     float* action_t, uint8_t* lifting, void* stream) {
    if (n <= 0 || !obs || !prev_obs || !has_prev || !t || !ready || !actor_out || !noise || !action || !action_t || !lifting) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_select_action, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, obs, prev_obs, has_prev, t, ready, actor_out,
                       noise, sigma, max_action, skip_steps, action, action_t, lifting);
    return launched();
}

int kr_controller_select(int32_t n, int32_t mode, int32_t lift_rule, const float* obs, const float* prev_obs, const uint8_t* has_prev, const int64_t* t,
                         uint8_t* ready, float* init, int32_t skip_steps, float* action, float* action_t, uint8_t* lifting, void* stream) {
    if (n <= 0 || !krsel::controller_args_ok(mode, lift_rule) || !obs || !prev_obs || !has_prev || !t || !ready || !init || !action || !action_t || !lifting)
        return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_controller_select, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, mode, lift_rule, obs, prev_obs, has_prev, t, ready,
                       init, skip_steps, action, action_t, lifting);
    return launched();
}

int kr_store_transition(int32_t n, int32_t horizon, int32_t n_steps, int32_t auto_reset, int32_t with_replay, const float* sim_obs,
                        const float* sim_final_obs, const float* sim_reward, const uint8_t* sim_done, float* obs, float* prev_obs,
                        uint8_t* has_prev, int64_t* t, uint8_t* ready, const uint8_t* lifting, const float* action, float* cur_state,
                        float* cur_next, float* cur_action, float* cur_reward, float* cur_not_done, int64_t* cur_len, float* reward_out,
                        uint8_t* done_out, uint8_t* keep, void* stream) {
    if (n <= 0 || !sim_obs || !sim_reward || !sim_done || !obs || !prev_obs || !has_prev || !t || !ready || !lifting || !reward_out || !done_out)
        return KS_ERR_INVALID;
    if (auto_reset && !sim_final_obs) return KS_ERR_INVALID;
    if (with_replay && (!action || !cur_state || !cur_next || !cur_action || !cur_reward || !cur_not_done || !cur_len || !keep)) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_store_transition, dim3(n), dim3(WAVE), 0, (hipStream_t)stream, n, horizon, n_steps, auto_reset, with_replay, sim_obs,
                       sim_final_obs, sim_reward, sim_done, obs, prev_obs, has_prev, t, ready, lifting, action, cur_state, cur_next, cur_action,
                       cur_reward, cur_not_done, cur_len, reward_out, done_out, keep);
    return launched();
}

int kr_wait_min_counted(const int64_t* values, int32_t n, int64_t target, double timeout_s, int64_t* timeouts, void* stream) {
    if (!values || n <= 0) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_wait_min, dim3(1), dim3(64), 0, (hipStream_t)stream, values, n, target, (long long)(timeout_s * 1e8), timeouts);   // wall_clock64: 100 MHz
    return launched();
}

int kr_wait_min(const int64_t* values, int32_t n, int64_t target, double timeout_s, void* stream) {
    return kr_wait_min_counted(values, n, target, timeout_s, nullptr, stream);
}

int kr_rank_episodes(int32_t n, const uint8_t* keep, int64_t* rank, int64_t* total, void* stream) {
    if (n <= 0 || !keep || !rank || !total) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_rank_episodes, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, n, keep, rank, total);
    return launched();
}

int kr_commit_episodes(int32_t n, int32_t horizon, int32_t capacity, const uint8_t* keep, const int64_t* rank, const int64_t* head,
                       const float* cur_state, const float* cur_next, const float* cur_action, const float* cur_reward,
                       const float* cur_not_done, const int64_t* cur_len, float* ep_state, float* ep_next, float* ep_action, float* ep_reward,
                       float* ep_not_done, int64_t* ep_len, void* stream) {
    if (n <= 0 || capacity <= 0 || !keep || !rank || !head || !cur_state || !cur_next || !cur_action || !cur_reward || !cur_not_done || !cur_len ||
        !ep_state || !ep_next || !ep_action || !ep_reward || !ep_not_done || !ep_len)
        return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_commit_episodes, dim3(n), dim3(WAVE), 0, (hipStream_t)stream, n, horizon, capacity, keep, rank, head, cur_state, cur_next,
                       cur_action, cur_reward, cur_not_done, cur_len, ep_state, ep_next, ep_action, ep_reward, ep_not_done, ep_len);
    return launched();
}

int kr_advance_ring(int32_t n, int32_t capacity, const int64_t* total, int64_t* head, int64_t* count, const uint8_t* ended, int64_t* cur_len,
                    void* stream) {
    if (n <= 0 || capacity <= 0 || !total || !head || !count || !ended || !cur_len) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_advance_ring, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, capacity, total, head, count, ended, cur_len);
    return launched();
}

static bool ring_ok(const kr_ring* r) {
    return r && r->count && r->head && r->capacity > 0 && r->ep_len && r->ep_state && r->ep_next && r->ep_action && r->ep_reward && r->ep_not_done;
}

static Ring to_ring(const kr_ring* r) {
    return Ring{r->count, r->head, r->capacity, r->ep_len, r->ep_state, r->ep_next, r->ep_action, r->ep_reward, r->ep_not_done};
}

// what kr_sample_windows_mixed requires of its arguments; _balanced and _prioritized require it too and add their own terms behind it
static bool sample_args_ok(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring* agent, const kr_ring* expert,
                           const float* u_ep, const float* u_start, const int64_t* draw, const float* state, const float* action,
                           const float* next_state, const float* reward, const float* not_done, const float* weight) {
    return batch > 0 && batch_agent >= 0 && batch_agent <= batch && horizon > n_steps && n_steps > 0 && n_steps <= WAVE && ring_ok(agent) && ring_ok(expert) &&
           ((u_ep == nullptr) == (u_start == nullptr)) && (u_ep || draw) && state && action && next_state && reward && not_done && weight;
}

// the gather behind a pick (kr_sample_windows_balanced, _prioritized): kr_sample_windows' rows with the episode supplied
static int gather_windows(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring* agent, const kr_ring* expert,
                          const int* slots, int row_major, const float* u_start, uint64_t seed, const int64_t* draw, float* next_ends, float* state,
                          float* action, float* next_state, float* reward, float* not_done, float* weight, const float* row_weight, void* stream) {
    hipLaunchKernelGGL(k_gather_windows, dim3(batch * (horizon - n_steps)), dim3(WAVE), 0, (hipStream_t)stream, batch, batch_agent, horizon, n_steps,
                       to_ring(agent), to_ring(expert), slots, row_major, u_start, (unsigned long long)seed, draw, next_ends, state, action, next_state,
                       reward, not_done, weight, row_weight);
    return launched();
}

int kr_sample_windows(int32_t batch, int32_t horizon, int32_t n_steps, const int64_t* count, const int64_t* head, int32_t capacity,
                      const int64_t* ep_len, const float* u_ep, const float* u_start, const float* ep_state, const float* ep_next, const float* ep_action, const float* ep_reward,
                      const float* ep_not_done, float* state, float* action, float* next_state, float* reward, float* not_done, float* weight,
                      void* stream) {
    if (!u_ep || !u_start) return KS_ERR_INVALID;
    const kr_ring g{count, head, capacity, ep_len, ep_state, ep_next, ep_action, ep_reward, ep_not_done};
    return kr_sample_windows_mixed(batch, batch, horizon, n_steps, &g, &g, u_ep, u_start, 0, nullptr, state, action, next_state, reward, not_done, weight,
                                   nullptr, stream);
}

int kr_sample_windows_draw(int32_t batch, int32_t horizon, int32_t n_steps, const int64_t* count, const int64_t* head, int32_t capacity,
                           const int64_t* ep_len, uint64_t seed, const int64_t* draw, const float* ep_state, const float* ep_next,
                           const float* ep_action, const float* ep_reward, const float* ep_not_done, float* state, float* action, float* next_state,
                           float* reward, float* not_done, float* weight, float* next_ends, void* stream) {
    if (!draw) return KS_ERR_INVALID;
    const kr_ring g{count, head, capacity, ep_len, ep_state, ep_next, ep_action, ep_reward, ep_not_done};
    return kr_sample_windows_mixed(batch, batch, horizon, n_steps, &g, &g, nullptr, nullptr, seed, draw, state, action, next_state, reward, not_done, weight,
                                   next_ends, stream);
}

int kr_sample_windows_mixed(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring* agent, const kr_ring* expert,
                            const float* u_ep, const float* u_start, uint64_t seed, const int64_t* draw, float* state, float* action,
                            float* next_state, float* reward, float* not_done, float* weight, float* next_ends, void* stream) {
    if (!sample_args_ok(batch, batch_agent, horizon, n_steps, agent, expert, u_ep, u_start, draw, state, action, next_state, reward, not_done, weight))
        return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_sample_windows, dim3(batch * (horizon - n_steps)), dim3(WAVE), 0, (hipStream_t)stream, batch, batch_agent, horizon, n_steps,
                       to_ring(agent), to_ring(expert), u_ep, u_start, (unsigned long long)seed, draw, next_ends, state, action, next_state, reward, not_done,
                       weight);
    return launched();
}

// what every kr_sample_tables_* entry requires beyond sample_args_ok's terms, and its outputs as the kernels take them
static bool tables_ok(const float* table_state, const float* table_next, const float* table_action, const int32_t* row_table, const float* slot_weight,
                      const float* state0, const float* action0, const float* reward, const float* not_done, const float* weight) {
    return table_state && table_next && table_action && row_table && slot_weight && state0 && action0 && reward && not_done && weight;
}
#define KR_TABLE_PARAMS float *table_state, float *table_next, float *table_action, int32_t *row_table, float *slot_weight, float *state0, float *action0, \
                        float *reward, float *not_done, float *weight, float *next_ends
#define KR_TABLE_ARGS table_state, table_next, table_action, row_table, slot_weight, state0, action0, reward, not_done, weight
#define KR_TABLES Tables{table_state, table_next, table_action, row_table, slot_weight, state0, action0, reward, not_done, weight, next_ends}

static int gather_tables(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring* agent, const kr_ring* expert,
                         const int* picked, int with_weight, const float* u_start, uint64_t seed, const int64_t* draw, const Tables& o, void* stream) {
    hipLaunchKernelGGL(k_gather_tables, dim3(batch * (horizon - n_steps)), dim3(WAVE), 0, (hipStream_t)stream, batch, batch_agent, horizon, n_steps,
                       to_ring(agent), to_ring(expert), picked, with_weight, u_start, (unsigned long long)seed, draw, o);
    return launched();
}

int kr_sample_tables_mixed(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring* agent, const kr_ring* expert,
                           const float* u_ep, const float* u_start, uint64_t seed, const int64_t* draw, KR_TABLE_PARAMS, void* stream) {
    if (!tables_ok(KR_TABLE_ARGS) ||
        !sample_args_ok(batch, batch_agent, horizon, n_steps, agent, expert, u_ep, u_start, draw, table_state, action0, table_next, reward, not_done, weight))
        return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_sample_tables, dim3(batch * (horizon - n_steps)), dim3(WAVE), 0, (hipStream_t)stream, batch, batch_agent, horizon, n_steps,
                       to_ring(agent), to_ring(expert), u_ep, u_start, (unsigned long long)seed, draw, KR_TABLES);
    return launched();
}

int kr_sample_tables_balanced(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring* agent, const kr_ring* expert,
                              const int32_t* agent_class, const int32_t* expert_class, int32_t n_classes, int32_t rotation, const float* u_ep,
                              const float* u_start, uint64_t seed, const int64_t* draw, KR_TABLE_PARAMS, int32_t* picked, void* stream) {
    if (!picked || !tables_ok(KR_TABLE_ARGS) ||
        !sample_args_ok(batch, batch_agent, horizon, n_steps, agent, expert, u_ep, u_start, draw, table_state, action0, table_next, reward, not_done, weight) ||
        n_classes < 1 || n_classes > 64 || (batch_agent > 0 && !agent_class) || (batch_agent < batch && !expert_class))
        return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_pick_balanced, dim3(batch), dim3(WAVE), 0, (hipStream_t)stream, batch, batch_agent, horizon - n_steps, to_ring(agent),
                       to_ring(expert), agent_class, expert_class, n_classes, rotation, u_ep, (unsigned long long)seed, draw, picked, 0);
    if (launched() != KS_OK) return KS_ERR_HIP;
    return gather_tables(batch, batch_agent, horizon, n_steps, agent, expert, picked, 0, u_start, seed, draw, KR_TABLES, stream);
}

int kr_sample_tables_prioritized(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring* agent, const kr_ring* expert,
                                 const uint32_t* agent_prio, const uint32_t* expert_prio, const float* beta, const float* u_ep, const float* u_start,
                                 uint64_t seed, const int64_t* draw, KR_TABLE_PARAMS, int32_t* picked, void* stream) {
    if (!picked || !tables_ok(KR_TABLE_ARGS) ||
        !sample_args_ok(batch, batch_agent, horizon, n_steps, agent, expert, u_ep, u_start, draw, table_state, action0, table_next, reward, not_done, weight) ||
        !beta || (batch_agent > 0 && (!agent_prio || agent->capacity > (1 << 20))) || (batch_agent < batch && (!expert_prio || expert->capacity > (1 << 20))))
        return KS_ERR_INVALID;
    // the pick hands every row its episode's importance weight in the weight output, where the gather wave of the row finds it
    hipLaunchKernelGGL(k_pick_prioritized, dim3(batch), dim3(WAVE), 0, (hipStream_t)stream, batch, batch_agent, horizon - n_steps, n_steps, to_ring(agent),
                       to_ring(expert), agent_prio, expert_prio, beta, u_ep, (unsigned long long)seed, draw, picked, reward, weight);
    if (launched() != KS_OK) return KS_ERR_HIP;
    return gather_tables(batch, batch_agent, horizon, n_steps, agent, expert, picked, 1, u_start, seed, draw, KR_TABLES, stream);
}

int kr_sample_tables_balanced_prioritized(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring* agent,
                                          const kr_ring* expert, const int32_t* agent_class, const int32_t* expert_class, int32_t n_classes,
                                          int32_t rotation, const uint32_t* agent_prio, const uint32_t* expert_prio, const float* beta,
                                          const float* u_ep, const float* u_start, uint64_t seed, const int64_t* draw, KR_TABLE_PARAMS,
                                          int32_t* picked, void* stream) {
    if (!picked || !tables_ok(KR_TABLE_ARGS) ||
        !sample_args_ok(batch, batch_agent, horizon, n_steps, agent, expert, u_ep, u_start, draw, table_state, action0, table_next, reward, not_done, weight) ||
        n_classes < 1 || n_classes > 64 || !beta ||
        (batch_agent > 0 && (!agent_class || !agent_prio || agent->capacity > (1 << 20))) ||
        (batch_agent < batch && (!expert_class || !expert_prio || expert->capacity > (1 << 20))))
        return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_pick_balanced_prioritized, dim3(batch), dim3(WAVE), 0, (hipStream_t)stream, batch, batch_agent, horizon - n_steps, n_steps,
                       to_ring(agent), to_ring(expert), agent_class, expert_class, n_classes, rotation, agent_prio, expert_prio, beta, u_ep,
                       (unsigned long long)seed, draw, picked, reward, weight);
    if (launched() != KS_OK) return KS_ERR_HIP;
    return gather_tables(batch, batch_agent, horizon, n_steps, agent, expert, picked, 1, u_start, seed, draw, KR_TABLES, stream);
}

int kr_commit_classes(int32_t n, int32_t capacity, const uint8_t* keep, const int64_t* rank, const int64_t* head, const int32_t* env_class,
                      int32_t* ep_class, void* stream) {
    if (n <= 0 || capacity <= 0 || !keep || !rank || !head || !env_class || !ep_class) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_commit_classes, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, (hipStream_t)stream, n, capacity, keep, rank, head, env_class,
                       ep_class);
    return launched();
}

int kr_sample_windows_balanced(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring* agent, const kr_ring* expert,
                               const int32_t* agent_class, const int32_t* expert_class, int32_t n_classes, int32_t rotation, const float* u_ep,
                               const float* u_start, uint64_t seed, const int64_t* draw, float* state, float* action, float* next_state,
                               float* reward, float* not_done, float* weight, float* next_ends, int32_t* picked, void* stream) {
    if (!sample_args_ok(batch, batch_agent, horizon, n_steps, agent, expert, u_ep, u_start, draw, state, action, next_state, reward, not_done, weight) ||
        n_classes < 1 || n_classes > 64 || (batch_agent > 0 && !agent_class) || (batch_agent < batch && !expert_class))
        return KS_ERR_INVALID;
    // without `picked` the slots travel from the pick to the gather in the weight output, one copy per window row: the gather wave of a row
    // reads its own element and then writes its weight there - no scratch buffer to own, nothing allocated on a captured stream
    const int row_major = picked == nullptr;
    int* slots = picked != nullptr ? picked : (int*)weight;
    hipLaunchKernelGGL(k_pick_balanced, dim3(batch), dim3(WAVE), 0, (hipStream_t)stream, batch, batch_agent, horizon - n_steps, to_ring(agent),
                       to_ring(expert), agent_class, expert_class, n_classes, rotation, u_ep, (unsigned long long)seed, draw, slots, row_major);
    if (launched() != KS_OK) return KS_ERR_HIP;
    return gather_windows(batch, batch_agent, horizon, n_steps, agent, expert, slots, row_major, u_start, seed, draw, next_ends, state, action, next_state,
                          reward, not_done, weight, nullptr, stream);
}

int kr_commit_priorities(int32_t n, int32_t capacity, const uint8_t* keep, const int64_t* rank, const int64_t* head, const uint32_t* prio_max,
                         uint32_t* ep_prio, void* stream) {
    if (n <= 0 || capacity <= 0 || !keep || !rank || !head || !prio_max || !ep_prio) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_commit_priorities, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, (hipStream_t)stream, n, capacity, keep, rank, head, prio_max,
                       ep_prio);
    return launched();
}

int kr_sample_windows_prioritized(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring* agent, const kr_ring* expert,
                                  const uint32_t* agent_prio, const uint32_t* expert_prio, const float* beta, const float* u_ep, const float* u_start,
                                  uint64_t seed, const int64_t* draw, float* state, float* action, float* next_state, float* reward, float* not_done,
                                  float* weight, float* next_ends, int32_t* picked, void* stream) {
    if (!sample_args_ok(batch, batch_agent, horizon, n_steps, agent, expert, u_ep, u_start, draw, state, action, next_state, reward, not_done, weight) ||
        !beta || (batch_agent > 0 && (!agent_prio || agent->capacity > (1 << 20))) || (batch_agent < batch && (!expert_prio || expert->capacity > (1 << 20))))
        return KS_ERR_INVALID;
    // the pick hands every row its episode's importance weight in the weight output and, without `picked`, the slot in the row's first reward:
    // the gather wave of a row reads its own two elements and then writes the row there - no scratch buffer, nothing allocated on a captured stream
    const int row_major = picked == nullptr ? n_steps : 0;
    const int* slots = picked != nullptr ? picked : (const int*)reward;
    hipLaunchKernelGGL(k_pick_prioritized, dim3(batch), dim3(WAVE), 0, (hipStream_t)stream, batch, batch_agent, horizon - n_steps, n_steps, to_ring(agent),
                       to_ring(expert), agent_prio, expert_prio, beta, u_ep, (unsigned long long)seed, draw, picked, reward, weight);
    if (launched() != KS_OK) return KS_ERR_HIP;
    return gather_windows(batch, batch_agent, horizon, n_steps, agent, expert, slots, row_major, u_start, seed, draw, next_ends, state, action, next_state,
                          reward, not_done, weight, weight, stream);
}

int kr_sample_windows_balanced_prioritized(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const kr_ring* agent,
                                           const kr_ring* expert, const int32_t* agent_class, const int32_t* expert_class, int32_t n_classes,
                                           int32_t rotation, const uint32_t* agent_prio, const uint32_t* expert_prio, const float* beta,
                                           const float* u_ep, const float* u_start, uint64_t seed, const int64_t* draw, float* state, float* action,
                                           float* next_state, float* reward, float* not_done, float* weight, float* next_ends, int32_t* picked,
                                           void* stream) {
    if (!sample_args_ok(batch, batch_agent, horizon, n_steps, agent, expert, u_ep, u_start, draw, state, action, next_state, reward, not_done, weight) ||
        n_classes < 1 || n_classes > 64 || !beta ||
        (batch_agent > 0 && (!agent_class || !agent_prio || agent->capacity > (1 << 20))) ||
        (batch_agent < batch && (!expert_class || !expert_prio || expert->capacity > (1 << 20))))
        return KS_ERR_INVALID;
    // the weight and, without `picked`, the slot travel to the gather as in kr_sample_windows_prioritized
    const int row_major = picked == nullptr ? n_steps : 0;
    const int* slots = picked != nullptr ? picked : (const int*)reward;
    hipLaunchKernelGGL(k_pick_balanced_prioritized, dim3(batch), dim3(WAVE), 0, (hipStream_t)stream, batch, batch_agent, horizon - n_steps, n_steps,
                       to_ring(agent), to_ring(expert), agent_class, expert_class, n_classes, rotation, agent_prio, expert_prio, beta, u_ep,
                       (unsigned long long)seed, draw, picked, reward, weight);
    if (launched() != KS_OK) return KS_ERR_HIP;
    return gather_windows(batch, batch_agent, horizon, n_steps, agent, expert, slots, row_major, u_start, seed, draw, next_ends, state, action, next_state,
                          reward, not_done, weight, weight, stream);
}

int kr_update_priorities(int32_t batch, int32_t batch_agent, int32_t horizon, int32_t n_steps, const float* q, const float* tq1, const float* reward,
                         const float* weight, float discount, const int32_t* picked, float alpha, float eps_agent, float eps_expert, uint32_t* agent_prio,
                         uint32_t* expert_prio, uint32_t* agent_prio_max, uint32_t* expert_prio_max, float* delta_out, void* stream) {
    if (batch <= 0 || batch_agent < 0 || batch_agent > batch || horizon <= n_steps || n_steps <= 0 || !q || !tq1 || !reward || !weight || !picked ||
        !(alpha >= 0.0f) || !(eps_agent >= 0.0f) || !(eps_expert >= 0.0f) || !(discount == discount) ||
        (batch_agent > 0 && (!agent_prio || !agent_prio_max)) || (batch_agent < batch && (!expert_prio || !expert_prio_max)))
        return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_update_priorities, dim3(batch), dim3(WAVE), 0, (hipStream_t)stream, batch, batch_agent, horizon - n_steps, n_steps, q, tq1, reward,
                       weight, discount, picked, alpha, eps_agent, eps_expert, agent_prio, expert_prio, agent_prio_max, expert_prio_max, delta_out);
    return launched();
}

// The one launch path of kr_critic_grad / kr_twin_critic_grad / kr_critic_grad_bounded.  twin: two critics on two target critics - q2, tq1_b,
// tqn_b and dq2 are all there or all absent; tboot [2R] is there exactly when the kernel writes it (twin or bounded).
static int critic_grad_launch(bool twin, bool bounded, int32_t rows, int32_t n_steps, const float* q1, const float* q2, const float* tq1_a,
                              const float* tq1_b, const float* tqn_a, const float* tqn_b, const float* reward, const float* weight,
                              const float* weight_sum, float discount, float q_lo, float q_hi, float huber_delta, float* dq1, float* dq2,
                              float* tboot, float* losses, void* stream) {
    if (rows <= 0 || n_steps <= 0 || !q1 || !tq1_a || !tqn_a || !reward || !weight_sum || !dq1 || !losses) return KS_ERR_INVALID;
    if ((q2 != nullptr) != twin || (dq2 != nullptr) != twin || (tq1_b != nullptr) != twin || (tqn_b != nullptr) != twin) return KS_ERR_INVALID;
    if ((tboot != nullptr) != (twin || bounded)) return KS_ERR_INVALID;
    if (bounded && (!(q_lo <= q_hi) || !(huber_delta > 0.0f))) return KS_ERR_INVALID;          // (a NaN fails either comparison)
    const auto kernel = twin ? (bounded ? k_critic_grad<true, true> : k_critic_grad<true, false>)
                             : (bounded ? k_critic_grad<false, true> : k_critic_grad<false, false>);
    hipLaunchKernelGGL(kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, rows, n_steps, q1, q2, tq1_a, tq1_b, tqn_a, tqn_b, reward, weight, weight_sum,
                       discount, q_lo, q_hi, huber_delta, dq1, dq2, tboot, losses);
    return launched();
}

// ... and of kr_adam_step / kr_adam_step_every / kr_adam_step_clipped (every and partials / max_norm / clip_out: of the forms that have them)
enum AdamForm { ADAM_PLAIN, ADAM_EVERY, ADAM_CLIPPED };
static int adam_launch(AdamForm form, int64_t count, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int64_t* step,
                       int32_t every, const double* partials, float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                       float* clip_out, void* stream) {
    if (count <= 0 || every <= 0 || !param || !grad || !exp_avg || !exp_avg_sq || !step) return KS_ERR_INVALID;
    if (form == ADAM_CLIPPED && (!partials || !(max_norm > 0.0f))) return KS_ERR_INVALID;
    const dim3 grid(grid_for(count)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    const long n = (long)count;
    if (form == ADAM_PLAIN)
        hipLaunchKernelGGL(k_adam_step, grid, block, 0, st, n, param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay);
    else if (form == ADAM_EVERY)
        hipLaunchKernelGGL(k_adam_step_every, grid, block, 0, st, n, param, grad, exp_avg, exp_avg_sq, step, every, lr, beta1, beta2, eps, weight_decay);
    else
        hipLaunchKernelGGL(k_adam_step_clipped, grid, block, 0, st, n, param, grad, exp_avg, exp_avg_sq, step, every, partials, max_norm, lr, beta1, beta2,
                           eps, weight_decay, clip_out);
    return launched();
}

int kr_critic_grad(int32_t rows, int32_t n_steps, const float* q, const float* tq1, const float* tqn, const float* reward, const float* weight,
                   const float* weight_sum, float discount, float* dq, float* losses, void* stream) {
    return critic_grad_launch(false, false, rows, n_steps, q, nullptr, tq1, nullptr, tqn, nullptr, reward, weight, weight_sum, discount, 0.0f, 0.0f, 0.0f,
                              dq, nullptr, nullptr, losses, stream);
}

int kr_update_prologue(int32_t rows, int32_t n_steps, const float* weight, float* weight_sum, float* dq_actor, int64_t* it, int64_t* it_head,
                       int32_t pipelined, void* stream) {
    if (rows <= 0 || n_steps <= 0 || !weight_sum || !dq_actor || !it || !it_head) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_update_prologue, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, rows, n_steps, weight, weight_sum, dq_actor, it, it_head, pipelined);
    return launched();
}

int kr_update_prologue_tables(int32_t rows, int32_t n_steps, int32_t batch, int32_t horizon, const float* weight, const float* slot_weight,
                              const int32_t* row_table, float* weight_sum, float* dq_table, int32_t* row_index, int64_t* it, int64_t* it_head,
                              int32_t pipelined, void* stream) {
    if (rows <= 0 || n_steps <= 0 || batch <= 0 || horizon < n_steps || !weight || !slot_weight || !row_table || !weight_sum || !dq_table ||
        !row_index || !it || !it_head)
        return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_update_prologue_tables, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, rows, n_steps, batch, horizon, weight, slot_weight,
                       row_table, weight_sum, dq_table, row_index, it, it_head, pipelined);
    return launched();
}

int kr_gather_table_q(int32_t rows, int32_t n_steps, const int32_t* row_table, const float* tq_table, float* tq, void* stream) {
    if (rows <= 0 || n_steps <= 0 || !row_table || !tq_table || !tq) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_gather_table_q, dim3((rows + WAVE - 1) / WAVE), dim3(WAVE), 0, (hipStream_t)stream, rows, n_steps, row_table, tq_table, tq);
    return launched();
}

int kr_relu_backward(int64_t count, const float* act, float* grad, void* stream) {
    if (count <= 0 || !act || !grad) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_relu_backward, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, (long)count, act, grad);
    return launched();
}

int kr_sigmoid_scale_backward(int64_t count, const float* a, float max_action, float* grad, void* stream) {
    if (count <= 0 || !a || !grad) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_sigmoid_scale_backward, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, (long)count, a, max_action, grad);
    return launched();
}

int kr_adam_step(int64_t count, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int64_t* step, float lr, float beta1,
                 float beta2, float eps, float weight_decay, void* stream) {
    return adam_launch(ADAM_PLAIN, count, param, grad, exp_avg, exp_avg_sq, step, 1, nullptr, 0.0f, lr, beta1, beta2, eps, weight_decay, nullptr, stream);
}

int kr_adam_step_every(int64_t count, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int64_t* step, int32_t every,
                       float lr, float beta1, float beta2, float eps, float weight_decay, void* stream) {
    return adam_launch(ADAM_EVERY, count, param, grad, exp_avg, exp_avg_sq, step, every, nullptr, 0.0f, lr, beta1, beta2, eps, weight_decay, nullptr, stream);
}

int kr_twin_critic_grad(int32_t rows, int32_t n_steps, const float* q1, const float* q2, const float* tq1_a, const float* tq1_b, const float* tqn_a,
                        const float* tqn_b, const float* reward, const float* weight, const float* weight_sum, float discount, float* dq1, float* dq2,
                        float* tmin, float* losses, void* stream) {
    return critic_grad_launch(true, false, rows, n_steps, q1, q2, tq1_a, tq1_b, tqn_a, tqn_b, reward, weight, weight_sum, discount, 0.0f, 0.0f, 0.0f, dq1,
                              dq2, tmin, losses, stream);
}

int kr_target_smooth(int32_t rows, float* action, const float* noise, uint64_t seed, const int64_t* draw, float sigma, float clip, float max_action,
                     void* stream) {
    if (rows <= 0 || !action || (noise != nullptr) == (draw != nullptr) || !(sigma >= 0.0f) || !(clip >= 0.0f) || !(max_action > 0.0f) ||
        ((uintptr_t)action & 15) != 0 || ((uintptr_t)noise & 15) != 0)
        return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_target_smooth, dim3(grid_for(rows)), dim3(256), 0, (hipStream_t)stream, rows, action, noise, (unsigned long long)seed, draw, sigma,
                       clip, max_action);
    return launched();
}

int kr_critic_grad_bounded(int32_t rows, int32_t n_steps, const float* q1, const float* q2, const float* tq1_a, const float* tq1_b, const float* tqn_a,
                           const float* tqn_b, const float* reward, const float* weight, const float* weight_sum, float discount, float q_lo, float q_hi,
                           float huber_delta, float* dq1, float* dq2, float* tboot, float* losses, void* stream) {
    return critic_grad_launch(q2 != nullptr, true, rows, n_steps, q1, q2, tq1_a, tq1_b, tqn_a, tqn_b, reward, weight, weight_sum, discount, q_lo, q_hi,
                              huber_delta, dq1, dq2, tboot, losses, stream);
}

int kr_grad_sqnorm(int64_t count, const float* grad, double* partials, void* stream) {
    if (count <= 0 || !grad || !partials) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_grad_sqnorm, dim3(NORM_PARTS), dim3(WAVE), 0, (hipStream_t)stream, (long)count, grad, partials);
    return launched();
}

int kr_adam_step_clipped(int64_t count, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int64_t* step, int32_t every,
                         const double* partials, float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, float* clip_out,
                         void* stream) {
    return adam_launch(ADAM_CLIPPED, count, param, grad, exp_avg, exp_avg_sq, step, every, partials, max_norm, lr, beta1, beta2, eps, weight_decay,
                       clip_out, stream);
}

int kr_bc_actor_grad(int32_t rows, int32_t demo_from, const float* pi, const float* demo, const float* q_demo, const float* q_pi, const float* dq,
                     float bc_weight, float max_action, float* dz3, float* sq, float* pass, void* stream) {
    if (rows <= 0 || demo_from < 0 || demo_from > rows || !pi || !demo || !dq || !dz3 || !sq || !pass || (q_demo != nullptr) != (q_pi != nullptr) ||
        !(bc_weight >= 0.0f) || !(max_action > 0.0f) || (((uintptr_t)pi | (uintptr_t)demo | (uintptr_t)dz3) & 15) != 0)
        return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_bc_actor_grad, dim3(grid_for(rows)), dim3(256), 0, (hipStream_t)stream, rows, demo_from, pi, demo, q_demo, q_pi, dq, bc_weight,
                       max_action, dz3, sq, pass);
    return launched();
}

int kr_obs_stats_update(int32_t rows, int32_t dim, const float* x, int32_t lda, const float* weight, const int64_t* it, int64_t freeze_after,
                        double* count, double* mean, double* m2, float* mean32, float* inv32, double eps, void* stream) {
    if (rows <= 0 || dim <= 0 || dim > OBS_MAX_DIM || lda < dim || !x || !count || !mean || !m2 || !mean32 || !inv32 || !(eps > 0.0) || !(eps < INFINITY) || freeze_after < 0)
        return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_obs_stats_update, dim3(1), dim3(OBS_WAVES * WAVE), 0, (hipStream_t)stream, rows, dim, x, lda, weight, it, freeze_after, count,
                       mean, m2, mean32, inv32, eps);
    return launched();
}

int kr_obs_normalize(int32_t rows, int32_t dim, float* x, int32_t lda, const float* mean32, const float* inv32, void* stream) {
    if (rows <= 0 || dim <= 0 || lda < dim || !x || !mean32 || !inv32) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_obs_normalize, dim3(grid_for((long)rows * dim)), dim3(256), 0, (hipStream_t)stream, (long)rows, dim, x, lda, mean32, inv32);
    return launched();
}

int kr_fold_obs_norm(int32_t h1, int32_t in_dim, int32_t norm_dim, const float* W1, const float* b1, const float* mean32, const float* inv32,
                     float* W1_out, float* b1_out, void* stream) {
    if (h1 <= 0 || in_dim <= 0 || norm_dim < 0 || norm_dim > in_dim || !W1 || !b1 || !mean32 || !inv32 || !W1_out || !b1_out) return KS_ERR_INVALID;
    // the outputs may not overlap an input (the kernel's pointers are restrict, and a row's bias reads what its weights wrote)
    const size_t wb = (size_t)h1 * in_dim * sizeof(float), bb = (size_t)h1 * sizeof(float), nb = (size_t)norm_dim * sizeof(float);
    const auto overlap = [](const void* a, size_t na, const void* b, size_t nb_) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return x < y + nb_ && y < x + na;
    };
    const void* outs[2] = {W1_out, b1_out};
    const size_t out_bytes[2] = {wb, bb};
    for (int o = 0; o < 2; o++)
        if (overlap(outs[o], out_bytes[o], W1, wb) || overlap(outs[o], out_bytes[o], b1, bb) || overlap(outs[o], out_bytes[o], mean32, nb) ||
            overlap(outs[o], out_bytes[o], inv32, nb))
            return KS_ERR_INVALID;
    if (overlap(W1_out, wb, b1_out, bb)) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_fold_obs_norm, dim3((h1 + 255) / 256), dim3(256), 0, (hipStream_t)stream, h1, in_dim, norm_dim, W1, b1, mean32, inv32, W1_out,
                       b1_out);
    return launched();
}

int kr_soft_update(int64_t count, const float* param, float* target, float tau, const int64_t* it, int32_t freq, void* stream) {
    if (count <= 0 || freq <= 0 || !param || !target || !it) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k_soft_update, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, (long)count, param, target, tau, it, freq);
    return launched();
}

}  // extern "C"
