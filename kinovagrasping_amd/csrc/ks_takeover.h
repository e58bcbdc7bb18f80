// ks_takeover.h -- the hand-over protocol of k_rollout's free-running waves (ks_api.hip): a wave that has done its env-steps of the
// launch takes over half the envs of the least-advanced wave of its own workgroup, within the exact step count (every env still
// does n_iter env-steps, one after the other, by one wave at a time).
//
// A wave's RUN is (off, cnt, left): it steps the envs of slots group * epw + off .. + cnt - 1 `left` more times.  The four waves of a
// workgroup share 4 x 3 words of LDS:
//   REQ[w]    0, or h + 1: wave h asks wave w for envs            (CAS 0 -> h + 1 by the helper; CAS -> 0 by w to claim, by h to withdraw)
//   PROG[w]   left << 3 | cnt of wave w's run                     (written by w only)
//   GRANT[h]  0, DECLINED, or GRANT_BIT | the run handed to h     (written by the wave that claimed h's request; cleared by h)
// A WORKER (left > 0) looks at REQ[me] before every env-step: a request it can serve (cnt >= 2, left >= MIN_LEFT) is claimed with ONE
// CAS and answered with the upper cnt / 2 envs of its run (release fence first: the envs' state travels through global memory), any
// other one is claimed and DECLINED.  A worker never waits and never retries: a CAS that fails (the helper has withdrawn) means no
// grant in this step.  A HELPER (left == 0, or no envs) picks the sibling with the largest left (then larger cnt, then lower index)
// among those with cnt >= 2, left > MIN_LEFT and no pending request, CASes its REQ word and polls its own GRANT word until the answer
// is there, the target has finished (left == 0) or the clock says DEADLINE; then it withdraws (CAS back to 0) - and if THAT fails the
// target has claimed the request and the answer is on its way: the helper takes it.  A sibling that qualifies but for a pending request
// is polled again (somebody else's request is answered within one env-step); the wave leaves when no sibling has envs to give.
//
// Host/device: the state machine below does ONE access to the shared words per call of advance(), through a memory policy M - LDS
// atomics in the kernel, a plain array under a deterministic scheduler in tests/native/ks_takeover_host.cpp, which interleaves the
// four waves' calls in every order.  Everything else (the run, the state, the scan's best candidate) is the wave's own.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KTK_HD __host__ __device__ __forceinline__
#else
#define KTK_HD inline
#endif
#include <stdint.h>

#ifndef KS_TAKEOVER_MIN_LEFT
#define KS_TAKEOVER_MIN_LEFT 2
#endif

namespace kstk {

constexpr int WAVES = 4, MIN_LEFT = KS_TAKEOVER_MIN_LEFT;
constexpr int REQ = 0, PROG = WAVES, GRANT = 2 * WAVES, WORDS = 3 * WAVES;
constexpr int LEFT_MAX = (1 << 22) - 1;                                   // a packed run: left << 7 | off << 3 | cnt (never 0: cnt >= 1)
constexpr uint32_t GRANT_BIT = 0x80000000u, DECLINED = 0x40000000u, FROM_PAIR = 0x20000000u;      // FROM_PAIR: the granting run had two envs

KTK_HD uint32_t pack_prog(int left, int cnt) { return (uint32_t)left << 3 | (uint32_t)cnt; }
KTK_HD uint32_t pack_run(int off, int cnt, int left) { return (uint32_t)left << 7 | (uint32_t)off << 3 | (uint32_t)cnt; }
KTK_HD int run_cnt(uint32_t r) { return (int)(r & 7u); }
KTK_HD int run_off(uint32_t r) { return (int)(r >> 3 & 15u); }
KTK_HD int run_left(uint32_t r) { return (int)(r >> 7 & (uint32_t)LEFT_MAX); }

enum State : int {
    W_ITER_DONE, W_CHECK, W_CLAIM, W_ANSWER, W_PUBLISH,                   // worker
    H_START, H_SCAN, H_REQUEST, H_WAIT, H_WAIT_TARGET, H_WITHDRAW, H_WAIT_ANSWER, H_TAKE, EXITED
};
enum Event : int { NONE, STEP, EXIT };                                    // STEP: run one env-step of the run now, then call again

// What a wave keeps to itself.  Between two env-steps only (off, cnt, left) matter (state W_ITER_DONE): the kernel carries them as one
// packed word and rebuilds the rest.
struct Wave {
    int me, state;
    int off, cnt, left;
    int q;                       // worker: the request word it has seen
    int target, k;               // helper: whom it asks; position of the scan (6 loads: PROG and REQ of the three siblings)
    int best, best_left, best_cnt, blocked;      // the scan's best qualified sibling so far; a sibling qualifies but for a pending request
    uint32_t got, prog;          // the answer taken from GRANT[me]; the PROG word of the sibling being scanned
    int64_t deadline;
    int expired;                 // the wait ended on the clock
    int idle;                    // set when a poll found nothing new: the kernel sleeps before the next call
    int grants, grants_from_pairs, expiries;     // counted for the caller: runs taken (of them: from a run of two envs), waits that expired
};

// The wave has run the env-step that advance() asked for with STEP.  A launch begins with resume(me, pack_run(off, cnt, n_iter + 1)): the first
// W_ITER_DONE then publishes the initial run, and a wave without envs becomes a helper at once.
KTK_HD Wave resume(int me, uint32_t run) {
    Wave w{};
    w.me = me; w.off = run_off(run); w.cnt = run_cnt(run); w.left = run_left(run);
    w.state = W_ITER_DONE;
    return w;
}
// the envs of wave w in a group of epw (the last group of an object may be partly filled), and what the shared words hold before the
// first wave looks at them: no request, no answer, every wave's initial run (a wave without envs must not find its siblings at left 0)
KTK_HD int initial_cnt(int w, int epw) { return epw - 4 * w < 4 ? (epw - 4 * w < 0 ? 0 : epw - 4 * w) : 4; }
KTK_HD uint32_t initial_word(int word, int epw, int n_iter) {
    return (word >= PROG && word < PROG + WAVES) ? pack_prog(n_iter, initial_cnt(word - PROG, epw)) : 0u;
}

// M: uint32_t load(int word); void store(int word, uint32_t v); bool cas(int word, uint32_t expect, uint32_t v) - relaxed, on the
// workgroup's WORDS words; void release() / acquire(): the fences around a grant (agent scope in the kernel); int64_t deadline_ticks().
template <class M>
KTK_HD Event advance(Wave& w, M& mem, int64_t now) {
    switch (w.state) {
    // ---- worker
    case W_ITER_DONE:
        w.left--;
        mem.store(PROG + w.me, pack_prog(w.left, w.cnt));
        w.state = (w.left > 0 && w.cnt > 0) ? W_CHECK : H_START;
        return NONE;
    case W_CHECK:
        w.q = (int)mem.load(REQ + w.me);
        if (w.q == 0) { w.state = W_ITER_DONE; return STEP; }
        w.state = W_CLAIM;
        return NONE;
    case W_CLAIM:
        if (!mem.cas(REQ + w.me, (uint32_t)w.q, 0u)) { w.state = W_ITER_DONE; return STEP; }      // withdrawn meanwhile: no grant in this step
        w.state = W_ANSWER;
        return NONE;
    case W_ANSWER:
        if (w.cnt >= 2 && w.left >= MIN_LEFT) {
            const int give = w.cnt / 2;
            mem.release();                                                // the envs' state as the last env-step left it
            mem.store(GRANT + w.q - 1, GRANT_BIT | pack_run(w.off + w.cnt - give, give, w.left) | (w.cnt == 2 ? FROM_PAIR : 0u));
            w.cnt -= give;
            w.state = W_PUBLISH;
            return NONE;
        }
        mem.store(GRANT + w.q - 1, DECLINED);
        w.state = W_ITER_DONE;
        return STEP;
    case W_PUBLISH:
        mem.store(PROG + w.me, pack_prog(w.left, w.cnt));
        w.state = W_ITER_DONE;
        return STEP;
    // ---- helper
    case H_START:
        w.deadline = now + mem.deadline_ticks();
        w.k = 0; w.best = -1; w.blocked = 0;
        w.state = H_SCAN;
        return NONE;
    case H_SCAN: {
        const int s = (w.me + 1 + w.k / 2) % WAVES;                      // sibling k / 2: first its PROG word, then its REQ word
        if ((w.k & 1) == 0) w.prog = mem.load(PROG + s);
        else {
            const int left = (int)(w.prog >> 3), cnt = (int)(w.prog & 7u);
            const bool pending = mem.load(REQ + s) != 0u;
            if (cnt >= 2 && left > MIN_LEFT) {
                if (pending) w.blocked = 1;
                else if (w.best < 0 || left > w.best_left || (left == w.best_left && (cnt > w.best_cnt || (cnt == w.best_cnt && s < w.best)))) {
                    w.best = s; w.best_left = left; w.best_cnt = cnt;
                }
            }
        }
        if (++w.k < 2 * (WAVES - 1)) return NONE;
        if (w.best >= 0) { w.target = w.best; w.state = H_REQUEST; return NONE; }
        if (w.blocked && now < w.deadline) { w.k = 0; w.blocked = 0; w.idle = 1; return NONE; }      // (scan again: the kernel sleeps in between)
        w.state = EXITED;
        return EXIT;
    }
    case H_REQUEST:
        if (mem.cas(REQ + w.target, 0u, (uint32_t)w.me + 1u)) { w.deadline = now + mem.deadline_ticks(); w.expired = 0; w.state = H_WAIT; }
        else if (now < w.deadline) { w.k = 0; w.best = -1; w.blocked = 0; w.state = H_SCAN; }      // somebody else asked first: look again
        else { w.state = EXITED; return EXIT; }
        return NONE;
    case H_WAIT:
        w.got = mem.load(GRANT + w.me);
        w.state = w.got != 0u ? H_TAKE : H_WAIT_TARGET;
        return NONE;
    case H_WAIT_TARGET:
        if ((mem.load(PROG + w.target) >> 3) == 0u) w.state = H_WITHDRAW;
        else if (now >= w.deadline) { w.expired = 1; w.state = H_WITHDRAW; }
        else { w.idle = 1; w.state = H_WAIT; }
        return NONE;
    case H_WITHDRAW:
        if (mem.cas(REQ + w.target, (uint32_t)w.me + 1u, 0u)) {          // withdrawn: nobody will answer this request
            if (w.expired) { w.expiries++; w.state = EXITED; return EXIT; }
            w.state = H_START;
        } else w.state = H_WAIT_ANSWER;                                   // claimed by the target: its answer is a store away
        return NONE;
    case H_WAIT_ANSWER:
        w.got = mem.load(GRANT + w.me);
        if (w.got != 0u) w.state = H_TAKE;
        else w.idle = 1;
        return NONE;
    case H_TAKE:
        mem.store(GRANT + w.me, 0u);
        if (w.got & GRANT_BIT) {
            mem.acquire();
            w.off = run_off(w.got); w.cnt = run_cnt(w.got); w.left = run_left(w.got);
            w.grants++;
            if (w.got & FROM_PAIR) w.grants_from_pairs++;
            w.state = W_PUBLISH;                                          // a worker again: publish the run, then step it
        } else w.state = H_START;                                         // declined (the target's run had shrunk meanwhile)
        return NONE;
    default:
        return EXIT;
    }
}

}  // namespace kstk
