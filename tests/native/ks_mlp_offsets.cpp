// tests/native/ks_mlp_offsets.cpp -- TEST-ONLY host walk of the actor forward's operand addressing (csrc/ks_mlp_tile.h: quad_off, tail_off,
// tail_here, x_off, tile_soff).  For every matrix of a network it plays every load the two tile bodies issue - every lane, every tile
// including the prefetches behind the last one, every k-step - against a copy of the matrix that has NaN on both sides, with the
// hardware's rule (a lane offset of OOR returns +0.0f and touches nothing), and checks
//   * that every lane offset other than OOR lies wholly inside the matrix: lane offset + size <= bytes (what the hardware checks) and
//     scalar offset + lane offset + size <= bytes (the address itself), both multiples of 4;
//   * that the operand the MFMA then gets - the quad, or the tail words where tail_here says so - is W[row][k .. k + 3] with exactly
//     +0.0f for every element at or beyond nrow / K (bit for bit: what load_w4 of the parent revision returned).
// Prints the number of loads walked; exit status 0 = every check held.  Built with -fsanitize=address,undefined by its test.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kinovagrasping_amd/csrc/ks_mlp_tile.h"

using namespace kmlp;

static long n_loads = 0, n_oor = 0, n_fail = 0;

#define CHECK(c, ...)                                                                  \
    do {                                                                               \
        if (!(c)) {                                                                    \
            if (n_fail++ < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                              \
    } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// a matrix of `count` floats between two guards of NaN
struct Guarded {
    static constexpr int G = 64;
    std::vector<float> buf;
    long count;
    explicit Guarded(long n) : buf((size_t)(n + 2 * G), std::nanf("")), count(n) {
        for (long i = 0; i < n; i++) buf[(size_t)(G + i)] = (float)(i % 8191 + 1) * ((i & 1) ? -1.f : 1.f);
    }
    uint32_t bytes() const { return (uint32_t)count * 4u; }
    float at(long i) const { return buf[(size_t)(G + i)]; }
    // the load of `words` floats at scalar offset soff + lane offset voff, as the hardware does it
    void load(uint32_t voff, uint32_t soff, int words, float* out, const char* what) const {
        n_loads++;
        for (int i = 0; i < words; i++) out[i] = 0.f;
        if (voff == OOR) { n_oor++; return; }
        const uint64_t end_lane = (uint64_t)voff + 4u * words, end = (uint64_t)soff + end_lane;
        CHECK(voff % 4 == 0 && soff % 4 == 0, "%s: voff %u soff %u", what, voff, soff);
        CHECK(end_lane <= bytes(), "%s: lane offset %u + %d > %u bytes", what, voff, 4 * words, bytes());
        CHECK(end <= bytes(), "%s: address %u + %u + %d > %u bytes", what, soff, voff, 4 * words, bytes());
        if (end > bytes() || (voff | soff) % 4) return;
        for (int i = 0; i < words; i++) out[i] = at((long)((soff + voff) / 4) + i);
    }
};

// what the MFMA must get for W[row][k .. k + 3], W = [nrow][K]
static void expect_quad(const Guarded& W, int row, int nrow, int k, int K, const float* got, const char* what) {
    for (int i = 0; i < 4; i++) {
        const bool exists = row >= 0 && row < nrow && k + i < K;
        const float want = exists ? W.at((long)row * K + k + i) : 0.f;
        CHECK(bits(got[i]) == bits(want), "%s row %d/%d k %d/%d: got %a, want %a", what, row, nrow, k + i, K, (double)got[i], (double)want);
    }
}

// Tile<NS, TAIL>::issue + quad / bias for tile row0 of W = [nrow][K] with bias B = [nrow]
static void walk_tile(const Guarded& W, const Guarded& B, int row0, int nrow, int K, int NS, bool TAIL, const char* what) {
    for (int lane = 0; lane < 64; lane++) {
        const int nn = lane & 15, q = lane >> 4;
        float wt[3] = {0, 0, 0}, bt[3] = {0, 0, 0}, bq[4];
        if (TAIL)
            for (int j = 0; j < 3; j++) {
                W.load(tail_off(nn, row0, nrow, K, j), tile_soff(row0, 0, K), 1, &wt[j], what);
                B.load(tail_off(0, 0, 1, nrow, j), 0, 1, &bt[j], what);
            }
        for (int s = 0; s < NS; s++) {
            float w[4];
            W.load(quad_off(nn, q, row0, nrow, 16 * s, K), tile_soff(row0, 16 * s, K), 4, w, what);
            if (TAIL && tail_here(q, 16 * s, K)) { w[0] = wt[0]; w[1] = wt[1]; w[2] = wt[2]; w[3] = 0.f; }
            expect_quad(W, row0 + nn, nrow, 16 * s + 4 * q, K, w, what);
        }
        B.load(quad_off(0, q, 0, 1, row0, nrow), tile_soff(0, row0, nrow), 4, bq, what);
        if (TAIL && tail_here(q, row0, nrow)) { bq[0] = bt[0]; bq[1] = bt[1]; bq[2] = bt[2]; bq[3] = 0.f; }
        expect_quad(B, 0, 1, row0 + 4 * q, nrow, bq, "bias");
    }
}

// every tile a body of `nw` waves issues for a layer of `nrow` outputs: tiles wave + nw i, and the two prefetches behind the last
static void walk_layer(const Guarded& W, const Guarded& B, int nrow, int K, int NS, bool TAIL, int nw, const char* what) {
    const int NT = (nrow + 15) / 16;
    for (int t = 0; t < NT + 2 * nw; t++) walk_tile(W, B, 16 * t, nrow, K, NS, TAIL, what);
}

// layer 3's quads of W3 = [out_dim][h2] over k-steps 0 .. NT2 - 1 (+ one step behind, as a partial wave split issues)
static void walk_w3(const Guarded& W3, int out_dim, int h2, bool TAIL, int nw) {
    const int NT2 = (h2 + 15) / 16;
    for (int lane = 0; lane < 64; lane++) {
        const int nn = lane & 15, q = lane >> 4;
        float wt[3] = {0, 0, 0};
        if (TAIL)
            for (int j = 0; j < 3; j++) W3.load(tail_off(nn, 0, out_dim, h2, j), 0, 1, &wt[j], "W3 tail");
        for (int s = 0; s < NT2 + nw; s++) {
            float w[4];
            W3.load(quad_off(nn, q, 0, out_dim, 16 * s, h2), tile_soff(0, 16 * s, h2), 4, w, "W3");
            if (TAIL && tail_here(q, 16 * s, h2)) { w[0] = wt[0]; w[1] = wt[1]; w[2] = wt[2]; w[3] = 0.f; }
            expect_quad(W3, nn, out_dim, 16 * s + 4 * q, h2, w, "W3");
        }
    }
}

// the input rows: `rows` rows exist; lanes name row nn - shift (so some are < 0) or no row; xa holds columns [0, in_a), xb [in_a, in_a + in_b)
static void walk_x(int rows, int in_a, int in_b, int lda, int ldb, int nr) {
    const Guarded Xa((long)(rows - 1) * lda + in_a), Xb(in_b ? (long)(rows - 1) * ldb + in_b : 0);
    CHECK(x_bytes(rows, 0, in_a, lda) == Xa.bytes(), "x_bytes a");
    CHECK(x_bytes(rows, in_a, in_a + in_b, ldb) == (in_b ? Xb.bytes() : 0u) || !in_b, "x_bytes b");
    for (int shift = 0; shift <= 2; shift++)
        for (int lane = 0; lane < 64; lane++) {
            const int nn = lane & 15, q = lane >> 4;
            long row = (long)nn - shift;                        // shift > 0: lanes 0 .. shift - 1 have row < 0
            if (nn >= nr || row >= rows) row = -1;              // the wave form's columns >= NR, a partial last tile
            for (int s = 0; s < KS_IN_MAX; s++)
                for (int j = 0; j < 4; j++) {
                    const int k = 16 * s + 4 * q + j;
                    float fa, fb = 0.f;
                    Xa.load(x_off(row, k, 0, in_a, lda), 0, 1, &fa, "xa");
                    if (in_b) Xb.load(x_off(row, k, in_a, in_a + in_b, ldb), 0, 1, &fb, "xb");
                    const float got = k < in_a ? fa : fb;
                    float want = 0.f;
                    if (row >= 0 && k < in_a) want = Xa.at(row * lda + k);
                    else if (row >= 0 && k < in_a + in_b) want = Xb.at(row * ldb + (k - in_a));
                    CHECK(bits(got) == bits(want), "x row %ld k %d: got %a want %a", row, k, (double)got, (double)want);
                }
        }
}

int main() {
    const int widths[][2] = {{64, 64}, {60, 52}, {128, 128}, {120, 116}, {256, 256}, {244, 244}, {250, 250}, {400, 300}, {392, 292}};
    const int in_dims[] = {82, 86, 96, 5};
    const int forms[] = {1, 4};                     // waves that split a layer's tiles: the wave form (and a 1-wave build), the 4-wave form
    for (const auto& hw : widths) {
        const int h1 = hw[0], h2 = hw[1];
        const bool tail = (h1 % 4) || (h2 % 4);     // the VEC = false instantiation
        const Guarded B1(h1), B2(h2), W2((long)h2 * h1);
        for (int nw : forms) {
            for (int in_dim : in_dims) {
                const Guarded W1((long)h1 * in_dim);
                walk_layer(W1, B1, h1, in_dim, KS_IN_MAX, true, nw, "W1");
            }
            walk_layer(W2, B2, h2, h1, (h1 + 15) / 16, tail, nw, "W2");
            if (!tail) walk_layer(W2, B2, h2, h1, (h1 + 15) / 16, true, nw, "W2 (tail loads on whole quads)");
            for (int out_dim = 1; out_dim <= 4; out_dim++) {
                const Guarded W3((long)out_dim * h2);
                walk_w3(W3, out_dim, h2, tail, nw);
            }
        }
    }
    for (int nr : {4, 16}) {                        // the wave form's NR = 4 rows, the 16-row form
        walk_x(21, 82, 0, 82, 0, nr);
        walk_x(3, 82, 4, 82, 4, nr);
        walk_x(17, 82, 4, 90, 7, nr);
        walk_x(16, 96, 0, 96, 0, nr);
        walk_x(2, 5, 0, 5, 0, nr);
        walk_x(1, 3, 2, 3, 2, nr);
    }
    std::printf("%ld loads walked, %ld of them out of range, %ld checks failed\n", n_loads, n_oor, n_fail);
    return n_fail ? 1 : 0;
}
