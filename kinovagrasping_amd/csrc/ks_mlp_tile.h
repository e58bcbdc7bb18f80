// ks_mlp_tile.h -- the 3-layer MLP forward of ONE 16-row tile on the matrix cores, as a device function: the body of k_mlp3
// (ks_mlp.hip: kr_mlp3_forward / kr_actor_select) and of the in-kernel actor of the free-running rollout kernel (ks_api.hip:
// k_rollout), so that both are the same k-ordered fp32 fma chains bit for bit.  See ks_mlp.hip for the layout.
// Two forms: mlp3_rows16 (a workgroup of NW waves, 16 batch rows, v_mfma_f32_16x16x4_f32) and mlp3_rows_wave (ONE wave, its own
// <= 4 batch rows, v_mfma_f32_4x4x1_16B_f32: no zero columns) - the second spells out, one k per instruction, the chains of the first.
//
// How the operands arrive.  Every matrix, bias vector and input block is read through a raw buffer resource of exactly its own
// bytes, with the addressing rule of the section below: the tile and k steps go into the (wave-uniform) scalar offset, the lane
// adds its row and quarter, and a lane whose element does not exist - a row of a partial last tile, the prefetch behind the last
// tile, a k beyond the row, a batch row that is not there - gets the out-of-range lane offset OOR instead: the hardware returns
// +0.0f for it and touches no memory.  No load sits in a branch, so all loads of a tile (its weight quads, the words of a row's
// tail when rows are no multiple of 4 floats, its bias quad) leave as ONE batch, the batch of the next tile before the MFMAs of
// the current one, and the first wait on them is the next tile's first MFMA: the two register sets take turns (Tile a / b below),
// nothing is copied.  sched_barrier(0) behind every batch keeps the scheduler from pulling it apart.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KS_MLP_HD __host__ __device__
#else
#define KS_MLP_HD
#endif

namespace kmlp {

constexpr int ROWS = 16;        // batch rows per workgroup (the N of the MFMA)
constexpr int KS_IN_MAX = 6;    // input k-steps: in_dim <= 96

// ---- the addressing rule (host / device, no intrinsics: tests/native/ks_mlp_offsets.cpp walks it over every lane, tile and k-step).
// A load's byte address is  base + scalar offset + lane offset;  the hardware's range check covers the LANE offset only (lane offset
// + size of the load <= bytes of the resource, else the load returns 0), so every guard is in the lane offset.
constexpr uint32_t OOR = 0x7ffffff0u;          // beyond every resource (whose sizes are < 2^31)

// scalar offset of tile row row0, k-step k0 of a row-major [.][K] float matrix
KS_MLP_HD inline uint32_t tile_soff(int row0, int k0, int K) { return (uint32_t)(row0 * K + k0) * 4u; }
// lane offset of the 16-byte load of W[row0 + nn][k0 + 4 q .. + 3], W = [nrow][K]: the row must exist and the quad lie in it as a whole
KS_MLP_HD inline uint32_t quad_off(int nn, int q, int row0, int nrow, int k0, int K) {
    const int row = row0 + nn, k = k0 + 4 * q;
    return (row >= 0 && row < nrow && k + 3 < K) ? (uint32_t)(nn * K + 4 * q) * 4u : OOR;
}
// A row of K % 4 != 0 floats ends in a tail of K % 4 words at k = tail_k(K), which no 16-byte load may touch (its last words are the
// next row's, or lie behind the matrix).  The tail's words j = 0 .. 2 are 4-byte loads of the tile's batch - lane offset tail_off
// beside the scalar offset tile_soff(row0, 0, K) - and replace the quad of the k-step and quarter that tail_here names.
KS_MLP_HD inline int tail_k(int K) { return K & ~3; }
KS_MLP_HD inline uint32_t tail_off(int nn, int row0, int nrow, int K, int j) {
    const int row = row0 + nn;
    return (row >= 0 && row < nrow && j < (K & 3)) ? (uint32_t)(nn * K + tail_k(K) + j) * 4u : OOR;
}
KS_MLP_HD inline bool tail_here(int q, int k0, int K) { return k0 + 4 * q == tail_k(K); }
// lane offset (scalar offset 0) of word k of batch row `row` of an input block x[.][ld] that holds the columns lo <= k < hi
KS_MLP_HD inline uint32_t x_off(long row, int k, int lo, int hi, int ld) {
    return (row >= 0 && k >= lo && k < hi) ? (uint32_t)(row * ld + (k - lo)) * 4u : OOR;
}
// bytes of such a block of `rows` rows (the last row ends with its own columns, not with the stride)
KS_MLP_HD inline uint32_t x_bytes(long rows, int lo, int hi, int ld) { return rows > 0 ? (uint32_t)((rows - 1) * ld + (hi - lo)) * 4u : 0u; }

}  // namespace kmlp

#if defined(__HIPCC__)
namespace kmlp {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

#ifndef KS_MLP_WAVES
#define KS_MLP_WAVES 4
#endif
constexpr int NW = KS_MLP_WAVES;   // waves per workgroup

// A wave-uniform value into scalar registers.  What a resource or a scalar offset is made of must be there: an out-of-line device function gets
// its arguments in vector registers, and a resource the compiler takes for divergent is loaded through in a loop over its distinct values.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ const float* uni(const float* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (const float*)(((unsigned long long)hi << 32) | lo);
}
// a resource over `bytes` bytes at p (both the same in all lanes); 4- and 16-byte loads through it (any 4-byte-aligned address)
__device__ __forceinline__ rsrc_t rsrc(const float* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(uni(p)), 0, uni((int)bytes), 0x00020000);
}
__device__ __forceinline__ float ldf(rsrc_t r, uint32_t voff, uint32_t soff) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0)); }
__device__ __forceinline__ f32x4 ldq(rsrc_t r, uint32_t voff, uint32_t soff) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0)); }

// The operands of one output tile - rows row0 .. row0 + 15 of W = [nrow][K] over NS k-steps, and the tile's bias quad - as ONE batch of
// loads (issue) whose values are touched only by quad() / bias(), at the MFMAs.  TAIL: K % 4 may be nonzero (W1 always; W2 / W3 and the
// biases in the VEC = false instantiation); without it a row is whole quads.
template <int NS, bool TAIL> struct Tile {
    f32x4 w[NS], bq;
    float wt[3], bt[3];
    __device__ __forceinline__ void issue(rsrc_t rW, rsrc_t rB, int nn, int q, int row0, int nrow, int K) {
#pragma unroll
        for (int s = 0; s < NS; s++) w[s] = ldq(rW, quad_off(nn, q, row0, nrow, 16 * s, K), tile_soff(row0, 16 * s, K));
        bq = ldq(rB, quad_off(0, q, 0, 1, row0, nrow), tile_soff(0, row0, nrow));
        if (TAIL) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                wt[j] = ldf(rW, tail_off(nn, row0, nrow, K, j), tile_soff(row0, 0, K));
                bt[j] = ldf(rB, tail_off(0, 0, 1, nrow, j), 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ f32x4 quad(int s, int q, int K) const {
        if (TAIL && tail_here(q, 16 * s, K)) return f32x4{wt[0], wt[1], wt[2], 0.f};
        return w[s];
    }
    __device__ __forceinline__ f32x4 bias(int q, int row0, int nrow) const {
        if (TAIL && tail_here(q, row0, nrow)) return f32x4{bt[0], bt[1], bt[2], 0.f};
        return bq;
    }
};

__device__ __forceinline__ f32x4 mfma4(f32x4 a, f32x4 b, f32x4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
    return c;
}

// bias + ReLU on an output quad (features f .. f+3, zero beyond nfeat), the biases read where they are used (the learner's kernels)
__device__ __forceinline__ f32x4 bias_relu(f32x4 acc, const float* __restrict__ bias, int f, int nfeat) {
    f32x4 r;
    r.x = f < nfeat ? fmaxf(acc.x + bias[f], 0.f) : 0.f;
    r.y = f + 1 < nfeat ? fmaxf(acc.y + bias[f + 1], 0.f) : 0.f;
    r.z = f + 2 < nfeat ? fmaxf(acc.z + bias[f + 2], 0.f) : 0.f;
    r.w = f + 3 < nfeat ? fmaxf(acc.w + bias[f + 3], 0.f) : 0.f;
    return r;
}

// the same with the bias quad in registers (features f .. f+3 with their bias quad b, zero beyond nfeat)
__device__ __forceinline__ f32x4 bias_relu(f32x4 acc, f32x4 b, int f, int nfeat) {
    f32x4 r;
    r.x = f < nfeat ? fmaxf(acc.x + b.x, 0.f) : 0.f;
    r.y = f + 1 < nfeat ? fmaxf(acc.y + b.y, 0.f) : 0.f;
    r.z = f + 2 < nfeat ? fmaxf(acc.z + b.z, 0.f) : 0.f;
    r.w = f + 3 < nfeat ? fmaxf(acc.w + b.w, 0.f) : 0.f;
    return r;
}

// All three layers for the 16 rows of a workgroup of NW waves (every thread of the workgroup must call this: two barriers inside).
// `row` = this lane's batch row (lane & 15 selects it; the same in all waves), < 0: no such row.  xa / xb: the input blocks,
// xa_bytes / xb_bytes what x_bytes() gives for the rows `row` can name (xb == nullptr: none); all pointers wave-uniform.  H1 / H2 / P:
// workgroup-shared scratch, [NT1 * 4][ROWS], [NT2 * 4][ROWS], [NW][ROWS] float4.  Returns true on the lanes that hold a row's layer-3
// sums z4 (wave 0, first quarter, row valid): the caller adds b3 and applies the output activation.
template <int NT1, int NT2, bool VEC>
__device__ __forceinline__ bool mlp3_rows16(const int wave_id, const int lane, const long row, int in_a, int in_b, int h1, int h2, int out_dim,
                                            const float* __restrict__ xa, int lda, uint32_t xa_bytes, const float* __restrict__ xb, int ldb,
                                            uint32_t xb_bytes, const float* __restrict__ W1, const float* __restrict__ b1,
                                            const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ W3,
                                            float* __restrict__ h1_out, float* __restrict__ h2_out, f32x4 (*H1)[ROWS], f32x4 (*H2)[ROWS],
                                            f32x4 (*P)[ROWS], f32x4& z4) {
    const int nn = lane & 15, q = lane >> 4;
    const int wave = uni(wave_id);          // (threadIdx.x >> 6 is the same in all lanes, but the compiler does not know: it goes into scalar offsets)
    const bool row_ok = row >= 0;
    in_a = uni(in_a), in_b = uni(in_b), h1 = uni(h1), h2 = uni(h2), out_dim = uni(out_dim), lda = uni(lda), ldb = uni(ldb);
    const int in_dim = in_a + in_b;
    const rsrc_t rW1 = rsrc(W1, (uint32_t)(h1 * in_dim) * 4u), rB1 = rsrc(b1, (uint32_t)h1 * 4u), rW2 = rsrc(W2, (uint32_t)(h2 * h1) * 4u),
                 rB2 = rsrc(b2, (uint32_t)h2 * 4u), rW3 = rsrc(W3, (uint32_t)(out_dim * h2) * 4u);
    // the first batch: the wave's copy of the 16 input rows as B operands of layer 1 (k = 16 s + 4 q + j), its first tile of W1, and its
    // first tile of W2, which arrives while layer 1 computes
    f32x4 bx[KS_IN_MAX];
    {
        const rsrc_t rXa = rsrc(xa, xa_bytes);
        float fa[KS_IN_MAX][4];
#pragma unroll
        for (int s = 0; s < KS_IN_MAX; s++)
#pragma unroll
            for (int j = 0; j < 4; j++) fa[s][j] = ldf(rXa, x_off(row, 16 * s + 4 * q + j, 0, in_a, lda), 0);
        if (xb) {       // (the same for the whole launch; nullptr at compile time in the rollout kernels)
            const rsrc_t rXb = rsrc(xb, xb_bytes);
#pragma unroll
            for (int s = 0; s < KS_IN_MAX; s++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float fb = ldf(rXb, x_off(row, 16 * s + 4 * q + j, in_a, in_dim, ldb), 0);
                    fa[s][j] = 16 * s + 4 * q + j < in_a ? fa[s][j] : fb;
                }
        }
#pragma unroll
        for (int s = 0; s < KS_IN_MAX; s++) bx[s] = f32x4{fa[s][0], fa[s][1], fa[s][2], fa[s][3]};
    }
    Tile<NT1, !VEC> a2, b2t;
    {
        Tile<KS_IN_MAX, true> a1, b1t;
        a1.issue(rW1, rB1, nn, q, 16 * wave, h1, in_dim);
        a2.issue(rW2, rB2, nn, q, 16 * wave, h2, h1);
        // one output tile of layer 1 (two chains: the MFMA's dependent latency is 40 cycles, its issue 32)
        auto tile1 = [&](const Tile<KS_IN_MAX, true>& w, int t) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS_IN_MAX; s++) {       // k beyond in_dim: both operands are zero
                if (s & 1) acc1 = mfma4(w.quad(s, q, in_dim), bx[s], acc1);
                else acc0 = mfma4(w.quad(s, q, in_dim), bx[s], acc0);
            }
            const f32x4 hq = bias_relu(acc0 + acc1, w.bias(q, 16 * t, h1), t * 16 + 4 * q, h1);
            H1[t * 4 + q][nn] = hq;
            if (h1_out && row_ok && t * 16 + 4 * q < h1) *(f32x4*)(h1_out + (long)row * h1 + t * 16 + 4 * q) = hq;   // h1 % 4 == 0 (checked by the host)
        };
#pragma unroll 1
        for (int t = wave; t < NT1; t += 2 * NW) {
            if (NT1 > NW) b1t.issue(rW1, rB1, nn, q, 16 * (t + NW), h1, in_dim);          // (a wave with one tile, or two: no batch for a tile nobody has)
            tile1(a1, t);
            if (NT1 > 2 * NW) a1.issue(rW1, rB1, nn, q, 16 * (t + 2 * NW), h1, in_dim);
            if (NT1 > NW && t + NW < NT1) tile1(b1t, t + NW);
        }
    }
    __syncthreads();

    // layer 2: K = h1, one k-step per tile of H1.  The wave's quads of W3 leave ahead of the loop and are used behind it.
    constexpr int NJ = (NT2 + NW - 1) / NW;
    f32x4 w3[NJ];
    float w3t[3];
#pragma unroll
    for (int j = 0; j < NJ; j++) w3[j] = ldq(rW3, quad_off(nn, q, 0, out_dim, 16 * (wave + NW * j), h2), tile_soff(0, 16 * (wave + NW * j), h2));
    if (!VEC) {
#pragma unroll
        for (int j = 0; j < 3; j++) w3t[j] = ldf(rW3, tail_off(nn, 0, out_dim, h2, j), 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    auto tile2 = [&](const Tile<NT1, !VEC>& w, int t) {
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NT1; s++) {
            if (s & 1) acc1 = mfma4(w.quad(s, q, h1), H1[s * 4 + q][nn], acc1);
            else acc0 = mfma4(w.quad(s, q, h1), H1[s * 4 + q][nn], acc0);
        }
        const f32x4 hq = bias_relu(acc0 + acc1, w.bias(q, 16 * t, h2), t * 16 + 4 * q, h2);
        H2[t * 4 + q][nn] = hq;
        if (h2_out && row_ok && t * 16 + 4 * q < h2) *(f32x4*)(h2_out + (long)row * h2 + t * 16 + 4 * q) = hq;
    };
#pragma unroll 1
    for (int t = wave; t < NT2; t += 2 * NW) {
        if (NT2 > NW) b2t.issue(rW2, rB2, nn, q, 16 * (t + NW), h2, h1);
        tile2(a2, t);
        if (NT2 > 2 * NW) a2.issue(rW2, rB2, nn, q, 16 * (t + 2 * NW), h2, h1);
        if (NT2 > NW && t + NW < NT2) tile2(b2t, t + NW);
    }
    __syncthreads();

    // layer 3: out_dim <= 4 outputs = rows 0..3 of ONE tile (quarter q = 0); the waves split the k-steps
    {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; j++)
            if (wave + NW * j < NT2) {
                const f32x4 wq = (!VEC && tail_here(q, 16 * (wave + NW * j), h2)) ? f32x4{w3t[0], w3t[1], w3t[2], 0.f} : w3[j];
                acc = mfma4(wq, H2[(wave + NW * j) * 4 + q][nn], acc);
            }
        if (q == 0) P[wave][nn] = acc;
    }
    __syncthreads();
    if (wave == 0 && q == 0 && row_ok) {
        z4 = P[0][nn];
#pragma unroll
        for (int w = 1; w < NW; w++) z4 += P[w][nn];
        return true;
    }
    return false;
}

// ---- the 4-row form: the same three layers by ONE wave for its own NR <= 4 batch rows (the free-running rollout kernel's waves each own
// four envs and never meet a barrier), on v_mfma_f32_4x4x1_16B_f32: 16 blocks of (4 x 1)(1 x 4), i.e. per instruction ONE k of 64 output
// features x 4 batch rows.  Transposed as above: A = the weight of the lane's own feature (lane l is feature o0 + l of a 64-feature
// group), B = the activation of batch row l % 4 (all 16 blocks read the same four), D = the features 4 (l / 4) .. + 3 of row l % 4 in the
// lane's four registers - after bias + ReLU again ONE float4 to LDS at [feature quad][row], which the next layer reads back as its B
// quads (one ds_read_b128 per four k).  One such MFMA is one fma per output, so every output element is spelled out as the chain the
// 16-row tile runs for it (mlp3_rows16): two accumulators per output, even 16-wide k-steps s into the first and odd s into the second;
// within a k-step k = 16 s + 4 q + x with x = 0..3 outer and q = 0..3 inner (the order in which mfma4 feeds the quads' components to the
// 16x16x4 instruction, whose four k are q); (acc0 + acc1) + bias, ReLU; layer 3 as NW partial sums over the k-steps w, w + NW, ..,
// added in wave order.  A row's result is the 4-wave kernel's bit for bit.
//
// The stream.  A batch is ONE k-step of G <= 4 feature groups (4 G quads per lane: 64 bytes of the lane's own row per group), so a pass
// over K runs G independent accumulator chains at a time; two register sets take turns as above.  The weights do not depend on the
// activations, so the batches run across pass and layer boundaries: the last two k-steps of a pass issue the first two batches of the
// next pass or layer (W3 behind layer 2), and nothing but the input rows is waited for with nothing to compute.
__device__ __forceinline__ f32x4 mfma1(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0); }

struct Rows4Set {
    f32x4 w[16];        // [group][quarter] of a k-step (layer 3: the lane's quads in k order)
};

// one batch: k-step s of the G groups of 64 rows at row0 (W = [nrow][K]); lane = row within the group
template <int G>
__device__ __forceinline__ void rows4_issue(Rows4Set& t, rsrc_t rW, int lane, int row0, int nrow, int s, int K) {
    __builtin_amdgcn_sched_barrier(0);          // (behind the MFMAs that read the set: the batch takes their registers, not new ones)
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (int q = 0; q < 4; q++) t.w[4 * g + q] = ldq(rW, quad_off(lane, q, row0 + 64 * g, nrow, 16 * s, K), tile_soff(row0 + 64 * g, 16 * s, K));
    __builtin_amdgcn_sched_barrier(0);
}
// the words of the rows' tails (wt: [G][3]), once per pass: they leave with the pass's second batch
template <int G>
__device__ __forceinline__ void rows4_tails(float* wt, rsrc_t rW, int lane, int row0, int nrow, int K) {
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (int j = 0; j < 3; j++) wt[3 * g + j] = ldf(rW, tail_off(lane, row0 + 64 * g, nrow, K, j), tile_soff(row0 + 64 * g, 0, K));
    __builtin_amdgcn_sched_barrier(0);
}

// the 16 G MFMAs of k-step s: B = the quads 4 s .. 4 s + 3 of the lane's batch row in Bsrc ([k quad][NR])
template <int G, bool TAIL, int NR>
__device__ __forceinline__ void rows4_kstep(const Rows4Set& t, const float* wt, f32x4 (&acc)[G], const f32x4 (*Bsrc)[NR], int lane, int s, int K) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const bool col_ok = (lane & 3) < NR;
    f32x4 b[4], a[G][4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        b[q] = col_ok ? Bsrc[4 * s + q][col_ok ? lane & 3 : 0] : zero;
#pragma unroll
        for (int g = 0; g < G; g++)
            a[g][q] = (TAIL && tail_here(q, 16 * s, K)) ? f32x4{wt[3 * g], wt[3 * g + 1], wt[3 * g + 2], 0.f} : t.w[4 * g + q];
    }
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int g = 0; g < G; g++) acc[g] = mfma1(a[g][q][x], b[q][x], acc[g]);
}

// One hidden layer: NP passes of G groups over the NS k-steps of K.  On entry the sets a / b hold (in flight) the k-steps 0 / 1 of the
// first pass and wt its tail words (TAILW); next_a / next_b issue the first two batches of whatever follows the layer.  Hout: [NQ][NR], feature quads of this layer.
template <int G, int NP, int NS, bool TAILW, bool TAILB, int NR, int NQ, class FA, class FB>
__device__ __forceinline__ void rows4_layer(rsrc_t rW, rsrc_t rB, int lane, int nfeat, int K, const f32x4 (*Bsrc)[NR], f32x4 (*Hout)[NR], Rows4Set& a,
                                            Rows4Set& b, float* wt, FA next_a, FB next_b) {
    constexpr int NSE = (NS + 1) & ~1;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int fq = lane >> 2;
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int o0 = 64 * G * p;
        f32x4 acc0[G], acc1[G];
#pragma unroll
        for (int g = 0; g < G; g++) acc0[g] = acc1[g] = zero;
#pragma unroll 1
        for (int s = 0; s + 2 < NSE; s += 2) {
            rows4_kstep<G, TAILW, NR>(a, wt, acc0, Bsrc, lane, s, K);
            rows4_issue<G>(a, rW, lane, o0, nfeat, s + 2, K);
            rows4_kstep<G, TAILW, NR>(b, wt, acc1, Bsrc, lane, s + 1, K);
            rows4_issue<G>(b, rW, lane, o0, nfeat, s + 3, K);           // (s + 3 == NS, NS odd: beyond K, nothing is read)
        }
        // the pass's bias quads, then its last two k-steps, each followed by a batch of what comes next
        f32x4 bq[G];
        float bt[3];
#pragma unroll
        for (int g = 0; g < G; g++) bq[g] = ldq(rB, quad_off(0, fq, 0, 1, o0 + 64 * g, nfeat), tile_soff(0, o0 + 64 * g, nfeat));
        if (TAILB) {
#pragma unroll
            for (int j = 0; j < 3; j++) bt[j] = ldf(rB, tail_off(0, 0, 1, nfeat, j), 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        rows4_kstep<G, TAILW, NR>(a, wt, acc0, Bsrc, lane, NSE - 2, K);
        if (p + 1 < NP) rows4_issue<G>(a, rW, lane, o0 + 64 * G, nfeat, 0, K);
        else next_a();
        if (NSE - 1 < NS) rows4_kstep<G, TAILW, NR>(b, wt, acc1, Bsrc, lane, NSE - 1, K);
        if (p + 1 < NP) {
            rows4_issue<G>(b, rW, lane, o0 + 64 * G, nfeat, 1, K);
            if (TAILW) rows4_tails<G>(wt, rW, lane, o0 + 64 * G, nfeat, K);
        } else next_b();
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int f = o0 + 64 * g + 4 * fq;
            const f32x4 bias = (TAILB && tail_here(fq, o0 + 64 * g, nfeat)) ? f32x4{bt[0], bt[1], bt[2], 0.f} : bq[g];
            const f32x4 hq = bias_relu(acc0[g] + acc1[g], bias, f, nfeat);
            if ((lane & 3) < NR && (f >> 2) < NQ) Hout[f >> 2][lane & 3] = hq;
        }
    }
}

__device__ __forceinline__ void rows4_join() {       // the wave's own LDS stores before its own LDS loads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// groups of 64 features per pass and passes of a layer of NT 16-feature tiles (256: 4 x 1, 400: 4 x 2, 300: 3 x 2, 128: 2 x 1, 64: 1 x 1)
constexpr int rows4_passes(int NT) { return ((NT + 3) / 4 + 3) / 4; }
constexpr int rows4_groups(int NT) { return ((NT + 3) / 4 + rows4_passes(NT) - 1) / rows4_passes(NT); }

// `row` = the batch row of lane l < NR (< 0: no such row; the other lanes' are ignored).  xa: [.][lda] rows of in_dim columns, xa_bytes
// as x_bytes() gives them.  X / H1 / H2: the wave's own scratch, [KS_IN_MAX * 4][NR], [NT1 * 4][NR], [NT2 * 4][NR] float4.  Returns true on
// the lanes that hold a row's layer-3 sums z4 (lane < NR, row valid).
template <int NT1, int NT2, bool VEC, int NR>
__device__ __forceinline__ bool mlp3_rows_wave(const int lane, const long row, int in_dim, int h1, int h2, int out_dim, const float* __restrict__ xa, int lda,
                                               uint32_t xa_bytes, const float* __restrict__ W1, const float* __restrict__ b1,
                                               const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ W3,
                                               f32x4 (*X)[NR], f32x4 (*H1)[NR], f32x4 (*H2)[NR], f32x4& z4) {
    static_assert(NR >= 1 && NR <= 4, "one MFMA block holds four batch rows");
    constexpr int G1 = rows4_groups(NT1), NP1 = rows4_passes(NT1), G2 = rows4_groups(NT2), NP2 = rows4_passes(NT2);
    constexpr int NJ = (NT2 + NW - 1) / NW, NQ3 = 4 * NJ;          // layer 3: k-steps and quads per partial sum
    static_assert(NQ3 <= 32, "layer 3's quads fill at most the two register sets");
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    in_dim = uni(in_dim), h1 = uni(h1), h2 = uni(h2), out_dim = uni(out_dim), lda = uni(lda);
    const rsrc_t rW1 = rsrc(W1, (uint32_t)(h1 * in_dim) * 4u), rB1 = rsrc(b1, (uint32_t)h1 * 4u), rW2 = rsrc(W2, (uint32_t)(h2 * h1) * 4u),
                 rB2 = rsrc(b2, (uint32_t)h2 * 4u), rW3 = rsrc(W3, (uint32_t)(out_dim * h2) * 4u);
    // the first batch: the NR input rows word by word (word i of the [NR][16 KS_IN_MAX] block goes to lane i % 64), and W1's first two k-steps
    constexpr int XW = 16 * KS_IN_MAX, XN = (NR * XW + 63) / 64;
    float xv[XN];
    {
        const rsrc_t rXa = rsrc(xa, xa_bytes);
#pragma unroll
        for (int j = 0; j < XN; j++) {
            const int i = lane + 64 * j, r = i / XW;
            const int rowr = __shfl((int)row, r < NR ? r : 0);
            xv[j] = ldf(rXa, x_off(r < NR ? (long)rowr : -1L, i % XW, 0, in_dim, lda), 0);
        }
    }
    Rows4Set a, b;
    float wt[12], wt3[3];
    rows4_issue<G1>(a, rW1, lane, 0, h1, 0, in_dim);
    rows4_issue<G1>(b, rW1, lane, 0, h1, 1, in_dim);
    rows4_tails<G1>(wt, rW1, lane, 0, h1, in_dim);
#pragma unroll
    for (int j = 0; j < XN; j++) {
        const int i = lane + 64 * j, r = i / XW, k = i % XW;
        if (r < NR) ((float*)X)[((k >> 2) * NR + r) * 4 + (k & 3)] = xv[j];
    }
    rows4_join();
    rows4_layer<G1, NP1, KS_IN_MAX, true, !VEC, NR, NT1 * 4>(
        rW1, rB1, lane, h1, in_dim, X, H1, a, b, wt, [&] { rows4_issue<G2>(a, rW2, lane, 0, h2, 0, h1); },
        [&] {
            rows4_issue<G2>(b, rW2, lane, 0, h2, 1, h1);
            if (!VEC) rows4_tails<G2>(wt, rW2, lane, 0, h2, h1);
        });
    rows4_join();

    // layer 3 puts its NW partial sums side by side: block w = lane / 4 of the MFMA runs the chain of the k-steps w, w + NW, .. with
    // A = W3's row lane % 4 (the output) and B = H2 of batch row lane % 4; the blocks w >= NW compute on zeros and are discarded.
    // The lane's NQ3 quads of W3, in the order of its chain, are the last two batches of the stream.
    const int w3 = lane >> 2, r3 = w3 < NW ? lane & 3 : -1;
    const auto issue3 = [&](Rows4Set& t, int i0) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = i0; i < NQ3 && i < i0 + 16; i++) t.w[i - i0] = ldq(rW3, quad_off(r3, 4 * (w3 + NW * (i >> 2)) + (i & 3), 0, out_dim, 0, h2), 0);
        if (!VEC && i0 == 0) {
#pragma unroll
            for (int j = 0; j < 3; j++) wt3[j] = ldf(rW3, tail_off(r3, 0, out_dim, h2, j), 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    rows4_layer<G2, NP2, NT1, !VEC, !VEC, NR, NT2 * 4>(rW2, rB2, lane, h2, h1, H1, H2, a, b, wt, [&] { issue3(a, 0); }, [&] { issue3(b, 16); });
    rows4_join();

    f32x4 acc = zero;
    const bool col_ok = (lane & 3) < NR;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int s = w3 + NW * j;
        const bool ok = w3 < NW && s < NT2;             // (a partial sum without this k-step keeps its value: the 4-wave kernel skips it)
        f32x4 hq[4], wq[4], n = acc;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            hq[q] = (ok && col_ok) ? H2[(ok ? s : 0) * 4 + q][col_ok ? lane & 3 : 0] : zero;
            const int i = 4 * j + q;
            wq[q] = i < 16 ? a.w[i < 16 ? i : 0] : b.w[i < 16 ? 0 : i - 16];
            if (!VEC) wq[q] = tail_here(4 * s + q, 0, h2) ? f32x4{wt3[0], wt3[1], wt3[2], 0.f} : wq[q];
        }
#pragma unroll
        for (int x = 0; x < 4; x++)
#pragma unroll
            for (int q = 0; q < 4; q++) n = mfma1(wq[q][x], hq[q][x], n);
        acc = (NT2 % NW == 0 || j + 1 < NJ || ok) ? n : acc;
    }
    // lane 4 w + r holds partial sum w of batch row r (its four registers: the outputs); the rows' lanes add them in wave order
    f32x4 z = acc;
#pragma unroll
    for (int w = 1; w < NW; w++) {
        const int src = 4 * w + (lane & 3);
        z += f32x4{__shfl(acc.x, src), __shfl(acc.y, src), __shfl(acc.z, src), __shfl(acc.w, src)};
    }
    if (lane < NR && row >= 0) {
        z4 = z;
        return true;
    }
    return false;
}

}  // namespace kmlp
#endif  // __HIPCC__
