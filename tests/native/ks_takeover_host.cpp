// Host model of csrc/ks_takeover.h (the hand-over protocol of k_rollout's free-running waves) for tests/test_takeover_cpu.py:
//   g++ -O2 -std=c++17 -o ks_takeover_host ks_takeover_host.cpp        (stand-alone; may also be built with -fsanitize=address,undefined)
// The header is the code the kernel compiles.  Here four model waves share twelve plain words; a deterministic scheduler picks, tick by
// tick, which wave makes its next call of kstk::advance() - ONE access to the shared words - or spends a tick of the env-step it is in.
// Schedules: every interleaving of the first `depth` ticks (then round-robin), and seeded random ones with random env-step durations
// and deadlines short enough to expire.  Checked in every run:
//   - every env is stepped exactly n_iter times, in order (a wave steps env e for the k-th time only when e has done k - 1 steps);
//   - an env is never in two waves' runs during the same step;
//   - every wave terminates;
//   - a request that its helper has withdrawn is never answered (and every answer goes to the helper whose request was claimed).
// usage: ks_takeover_host [depth [random_schedules]]; prints one summary line, exit status 1 on the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../kinovagrasping_amd/csrc/ks_takeover.h"

namespace {

using namespace kstk;

struct Violation { const char* what; };

struct Mem {
    uint32_t w[WORDS];
    int64_t dl;
    int cur = 0;                        // the wave whose call this is
    int asked[WAVES];                   // helper h: 1 + the wave it has an open request with, 0 none
    bool claimed[WAVES];                // ... and that wave has claimed it
    long ops = 0, fences = 0;
    bool released[WAVES] = {};          // wave w: a release fence since its last answer
    void fail(const char* what) { throw Violation{what}; }
    uint32_t load(int i) { ops++; return w[i]; }
    void store(int i, uint32_t v) {
        ops++;
        if (i >= GRANT) {
            const int h = i - GRANT;
            if (v == 0u) {
                if (cur != h) fail("an answer word cleared by another wave than its helper");
                asked[h] = 0; claimed[h] = false;
            } else {
                if (asked[h] != cur + 1) fail("a request that is not open (withdrawn, or never made) was answered");
                if (!claimed[h]) fail("a request was answered without having been claimed");
                if (w[i] != 0u) fail("an answer overwrote an answer that had not been taken");
                if ((v & GRANT_BIT) && !released[cur]) fail("a grant without a release fence in front of it");
                released[cur] = false;
            }
        } else if (i >= PROG) {
            if (i - PROG != cur) fail("a progress word written by another wave");
        } else fail("a request word written without CAS");
        w[i] = v;
    }
    bool cas(int i, uint32_t expect, uint32_t v) {
        ops++;
        if (i >= PROG) fail("CAS on a word that is no request word");
        if (w[i] != expect) return false;
        const int t = i - REQ;
        if (expect == 0u) {                                  // a helper asks
            if ((int)v != cur + 1 || asked[cur] != 0) fail("a helper with two open requests, or asking in another's name");
            asked[cur] = t + 1; claimed[cur] = false;
        } else if (t == cur) {                               // the asked wave claims
            claimed[expect - 1] = true;
        } else {                                             // the helper withdraws
            if ((int)expect != cur + 1 || asked[cur] != t + 1) fail("a request withdrawn by another wave than its helper");
            asked[cur] = 0;
        }
        w[i] = v;
        return true;
    }
    void release() { fences++; released[cur] = true; }
    void acquire() { fences++; }
    int64_t deadline_ticks() const { return dl; }
};

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

struct Totals { long runs = 0, grants = 0, from_pairs = 0, expiries = 0, declines = 0, ops = 0, max_ticks = 0; };

// One launch of a workgroup.  prefix[0 .. depth): the scheduler's choices (0..3) of the first ticks, round-robin after them; rng != nullptr: random
// choices and env-step durations 0 .. max_dur ticks instead.
void run_one(const int* cnt0, int n_iter, int64_t deadline, const int* prefix, int depth, int fixed_dur, Rng* rng, int max_dur, Totals& tot) {
    Mem mem;
    memset(mem.w, 0, sizeof mem.w);
    memset(mem.asked, 0, sizeof mem.asked);
    memset(mem.claimed, 0, sizeof mem.claimed);
    mem.dl = deadline;
    Wave wv[WAVES];
    int busy[4 * WAVES] = {}, steps[4 * WAVES] = {}, dur[WAVES] = {};
    bool exited[WAVES] = {}, stepping[WAVES] = {};
    for (int w = 0; w < WAVES; w++) {
        mem.w[PROG + w] = pack_prog(n_iter, cnt0[w]);
        wv[w] = resume(w, pack_run(4 * w, cnt0[w], n_iter + 1));
    }
    int alive = WAVES, rr = 0;
    long tick = 0;
    const long tick_limit = 4000L + 400L * n_iter * (1 + (rng ? max_dur : fixed_dur)) + 40 * deadline;
    for (; alive > 0; tick++) {
        if (tick > tick_limit) throw Violation{"a wave does not terminate"};
        int c = tick < depth ? prefix[tick] : (rng ? rng->below(WAVES) : rr++ % WAVES);
        while (exited[c]) c = (c + 1) % WAVES;
        if (dur[c] > 0) { dur[c]--; continue; }              // in the middle of its env-step
        Wave& w = wv[c];
        if (stepping[c]) {                                   // the env-step is over: as the kernel does, the wave comes back with its packed run only
            for (int e = 0; e < 4 * WAVES; e++)
                if (busy[e] == c + 1) { busy[e] = 0; steps[e]++; }
            stepping[c] = false;
            const Wave keep = w;
            w = resume(c, pack_run(keep.off, keep.cnt, keep.left));
            w.grants = keep.grants; w.grants_from_pairs = keep.grants_from_pairs; w.expiries = keep.expiries;
        }
        mem.cur = c;
        w.idle = 0;
        const uint32_t had = mem.w[GRANT + c];
        const Event ev = advance(w, mem, (int64_t)tick);
        if (had == DECLINED && mem.w[GRANT + c] == 0u) tot.declines++;
        if (ev == STEP) {
            if (w.cnt < 1 || w.cnt > 4 || w.off < 0 || w.off + w.cnt > 4 * WAVES || w.left < 1 || w.left > n_iter) throw Violation{"a run out of range"};
            for (int e = w.off; e < w.off + w.cnt; e++) {
                if (busy[e]) throw Violation{"an env in two waves' runs during the same step"};
                if (steps[e] != n_iter - w.left) throw Violation{"an env stepped out of order (a step skipped or repeated)"};
                busy[e] = c + 1;
            }
            stepping[c] = true;
            dur[c] = rng ? rng->below(max_dur + 1) : fixed_dur;
        } else if (ev == EXIT) {
            if (mem.asked[c] != 0) throw Violation{"a wave left with an open request"};
            if (mem.w[GRANT + c] != 0u) throw Violation{"a wave left with an answer it had not taken"};
            exited[c] = true;
            alive--;
            tot.grants += w.grants; tot.from_pairs += w.grants_from_pairs; tot.expiries += w.expiries;
        }
    }
    for (int w = 0; w < WAVES; w++)
        for (int j = 0; j < 4; j++) {
            const int e = 4 * w + j, want = j < cnt0[w] ? n_iter : 0;
            if (steps[e] != want) throw Violation{"an env was not stepped exactly n_iter times"};
        }
    tot.runs++;
    tot.ops += mem.ops;
    if (tick > tot.max_ticks) tot.max_ticks = tick;
}

}  // namespace

int main(int argc, char** argv) {
    const int depth = argc > 1 ? atoi(argv[1]) : 8, n_random = argc > 2 ? atoi(argv[2]) : 4000;
    static const int starts[4][WAVES] = {{4, 4, 4, 4}, {4, 1, 0, 0}, {2, 0, 0, 0}, {3, 4, 0, 4}};
    static const int iters[4] = {1, 2, 3, 9};
    if (depth < 0 || depth > 12) { fprintf(stderr, "depth 0..12\n"); return 2; }
    Totals tot;
    int prefix[12] = {};
    const int* cnt0 = nullptr;
    int n_iter = 0;
    try {
        for (int s = 0; s < 4; s++)
            for (int k = 0; k < 4; k++) {
                cnt0 = starts[s]; n_iter = iters[k];
                // every interleaving of the first `depth` ticks; env-steps that take no tick at all (the protocol's calls back to back) or two,
                // a deadline that never comes or one of three ticks
                for (int variant = 0; variant < 4; variant++) {
                    const long total = 1L << (2 * depth);
                    for (long code = 0; code < total; code++) {
                        for (int d = 0; d < depth; d++) prefix[d] = (int)(code >> (2 * d) & 3);
                        run_one(cnt0, n_iter, (variant & 1) ? 3 : 1000000, prefix, depth, (variant & 2) ? 2 : 0, nullptr, 0, tot);
                    }
                }
                for (int r = 0; r < n_random; r++) {
                    Rng rng{0x9E3779B97F4A7C15ull * (uint64_t)(r + 1) + (uint64_t)(s * 4 + k)};
                    const int max_dur = 1 + rng.below(40);
                    const int64_t deadline = (r & 1) ? 1 + rng.below(60) : 1000000;
                    run_one(cnt0, n_iter, deadline, prefix, 0, 0, &rng, max_dur, tot);
                }
            }
    } catch (const Violation& v) {
        printf("VIOLATION: %s (start %d %d %d %d, n_iter %d, after %ld clean runs)\n", v.what, cnt0[0], cnt0[1], cnt0[2], cnt0[3], n_iter, tot.runs);
        return 1;
    }
    printf("ok: %ld schedules (depth %d, %d random per case), %ld grants taken (%ld from runs of two), %ld declined, %ld expired waits, %ld shared accesses, longest %ld ticks\n",
           tot.runs, depth, n_random, tot.grants, tot.from_pairs, tot.declines, tot.expiries, tot.ops, tot.max_ticks);
    return 0;
}
