// ks_mlp.hip -- fused 3-layer MLP forward on the matrix cores (C ABI: include/kinova_rollout.h, kr_mlp3_forward).
//
// The reference's actor and critic (DDPGfD.py:17-50) are  out = f(W3 relu(W2 relu(W1 x + b1) + b2) + b3)  with
// 82 / 86 inputs, two hidden layers (256-256 in BASELINE, 400-300 in the reference) and 4 / 1 outputs.  As three
// library GEMMs + bias/activation kernels that is 8-11 launches of a few microseconds each, on the critical path of
// every env-step (the action of step t+1 needs the observation of step t).  Here it is ONE launch:
//
//   * a workgroup (4 waves, one per SIMD) owns 16 batch rows and computes all three layers for them; the activations
//     never leave the CU (LDS), the weights (<= 0.7 MB, L2 resident) stream through the MFMA A operand;
//   * exact fp32 on v_mfma_f32_16x16x4_f32, in the TRANSPOSED orientation  H^T = W X^T : A = W (16 output features x
//     4 k), B = X^T (4 k x 16 batch rows), D = 16 features x 16 rows.  A lane of D holds features 4q..4q+3 (q = lane>>4)
//     of batch row n = lane&15 - exactly the 4 k-values the same lane must supply as the B operand of the next
//     layer's four MFMAs of a 16-wide k-step.  So a layer's output quad is stored as one float4 at [tile*4 + q][n] and
//     read back from the same slot: no transposes, no bank conflicts (16 consecutive float4 per quarter wave);
//   * the waves split the output tiles of layers 1 and 2 and the k-steps of layer 3 (partial sums through LDS).
//
// Arithmetic: every output is a k-ordered fp32 fma chain (MFMA f32 is bitwise an fmaf chain), so results differ
// from the library GEMMs only by summation order (~1e-7 relative); tests/test_gpu_parity.py checks against torch.
// Pinned on dense random data: the free-running waves run the same chains ONE k per instruction on v_mfma_f32_4x4x1_16B_f32
// (ks_mlp_tile.h: mlp3_rows_wave) and equal this kernel bit for bit at six widths (tests/test_gpu_actor_wave_rows4.py) - so the
// 16x16x4 instruction is, per output, the fma chain of its four k in the order k = 0, 1, 2, 3.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/kinova_rollout.h"
#include "../../include/kinova_sim.h"
#include "ks_mlp_tile.h"
#include "ks_select.h"

namespace {

using namespace kmlp;

// occupancy target of the 2- / 4-wave split learner kernels: 3 waves per SIMD = up to 168 registers (156 used, no spills); the
// experiment switch 4 caps them at 128 (140 B of scratch per lane) so that they fit beside k_rollout's 368
#ifndef KS_SPLIT_WAVES_PER_EU
#define KS_SPLIT_WAVES_PER_EU 3
#endif

// Epilogue of the fused actor + action-selection launch (kr_actor_select): everything k_select_action takes, plus the
// noise source (a tensor of N(0,1) draws, or the in-kernel counter-based generator keyed by (seed, rng_state[0], env))
struct SelectArgs {
    const float* obs; const float* prev_obs; const uint8_t* has_prev; const int64_t* t; uint8_t* ready;
    const float* noise; unsigned long long seed; int64_t* rng_state;
    float sigma, max_action; int skip_steps;
    float* action; float* action_t; uint8_t* lifting;
};

// NT1 / NT2: 16-feature tiles of the two hidden layers.  x is [n][ldx] with the first in_a columns from xa and, when
// xb != nullptr, the next in_b columns from xb ([n][ldb]) - the critic's cat([state, action]) without materialising it.
template <int NT1, int NT2, bool VEC, bool SEL>
__global__ __launch_bounds__(64 * NW) void k_mlp3(int n, int in_a, int in_b, int h1, int h2, int out_dim, const float* __restrict__ xa, int lda,
                                              const float* __restrict__ xb, int ldb, const float* __restrict__ W1, const float* __restrict__ b1,
                                              const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ W3,
                                              const float* __restrict__ b3, int act, float scale, float* __restrict__ out, float* __restrict__ h1_out,
                                              float* __restrict__ h2_out, SelectArgs sel) {
    __shared__ f32x4 H1[NT1 * 4][ROWS];
    __shared__ f32x4 H2[NT2 * 4][ROWS];
    __shared__ f32x4 P[NW][ROWS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nn = lane & 15;
    const int row = blockIdx.x * ROWS + nn;
    const bool row_ok = row < n;
    unsigned long long rng_step = 0;
    if (SEL && sel.rng_state) rng_step = (unsigned long long)sel.rng_state[0];      // read by every workgroup before any of them finishes
    f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    // (the tile body addresses the workgroup's own rows 0 .. 15 of blocks that begin at its first row: 32-bit offsets at any n)
    const long r0 = (long)blockIdx.x * ROWS;
    const long nr = n - r0 < ROWS ? n - r0 : ROWS;
    if (mlp3_rows16<NT1, NT2, VEC>(wave, lane, row_ok ? (long)nn : -1L, in_a, in_b, h1, h2, out_dim, xa + r0 * lda, lda, x_bytes(nr, 0, in_a, lda),
                                   xb ? xb + r0 * ldb : nullptr, ldb, x_bytes(nr, in_a, in_a + in_b, ldb), W1, b1, W2, b2, W3,
                                   h1_out ? h1_out + r0 * h1 : nullptr, h2_out ? h2_out + r0 * h2 : nullptr, H1, H2, P, z4)) {
        const float z[4] = {z4.x, z4.y, z4.z, z4.w};
        float y[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < out_dim; i++) {
            y[i] = z[i] + b3[i];
            if (act == KR_ACT_SIGMOID) y[i] = scale / (1.f + __expf(-y[i]));
            if (out) out[(long)row * out_dim + i] = y[i];
        }
        if (SEL) {
            float nz[4];
            if (sel.noise) {
#pragma unroll
                for (int k = 0; k < 4; k++) nz[k] = sel.noise[(long)row * 4 + k];
            } else {
                krsel::normal4(sel.seed, rng_step, (uint32_t)row, nz);
            }
            krsel::select_one(row, n, y, nz, sel.obs, sel.prev_obs, sel.has_prev, sel.t, sel.ready, sel.sigma, sel.max_action, sel.skip_steps,
                              sel.action, sel.action_t, sel.lifting);
        }
    }
    if (SEL && sel.rng_state) {
        // the LAST workgroup to finish advances the step counter: every workgroup has read it by then
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence();
            const unsigned ticket = atomicAdd((unsigned*)(sel.rng_state + 1), 1u);
            if (ticket == gridDim.x - 1) {
                sel.rng_state[1] = 0;
                sel.rng_state[0] = (int64_t)(rng_step + 1);
            }
        }
    }
}

// ---- the LDS-FREE forms of the same network (the learner's passes, which run in the shadow of the stepping kernel) and what
// they share.  One wave = 16 batch rows with all layers in registers (k_mlp3_wave / k_mlp3_bwd_wave), the tiles of a layer split
// over 2 / 4 waves of a workgroup (k_mlp3_split / k_mlp3_bwd_split), or no layer in registers at all (k_mlp3_lean /
// k_mlp3_bwd_lean).  The helpers from here to k_mlp3_wave are the one copy of the blocks the forms have in common; a block that stays
// written out in a kernel does so because the compiler allocates or schedules that kernel worse through a helper (profiles/mlp_front_end.txt).
//
// All operand reads are raw buffer loads (kmlp::rsrc / ldf / ldq): ONE 32-bit lane offset per matrix, the tile / k-step advance
// in the wave-uniform scalar offset, out-of-range reads return 0 in hardware.  The flat-load version spent 5 VALU + 7 SALU
// instructions (address arithmetic, bounds branches) per MFMA - issue slots these kernels share with the stepping kernel's wave
// on the same SIMD.  The range check covers the LANE offset only, not the scalar offset: an element that does not exist gets the
// out-of-range lane offset OOR instead of relying on the sum (the rule of ks_mlp_tile.h).

// a 16-byte load that sees what another lane or wave of this workgroup stored behind a fence (glc)
__device__ __forceinline__ f32x4 ldq_glc(rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 1));
}

// B operands of layer 1: the 16 input rows, k = 16 s + 4 q + j, columns < in_a from xa and the rest from xb.  A row beyond n gets OOR (0).
__device__ __forceinline__ void input_quads(f32x4 (&bx)[KS_IN_MAX], int n, int row, int q, int in_a, int in_b, const float* __restrict__ xa, int lda,
                                            const float* __restrict__ xb, int ldb) {
    const bool row_ok = row < n;
    const int in_dim = in_a + in_b;
    const rsrc_t rXa = rsrc(xa, ((n - 1) * lda + in_a) * 4), rXb = rsrc(xb ? xb : xa, xb ? ((n - 1) * ldb + in_b) * 4 : 0);
    const int oa = row * lda * 4 + 16 * q, ob = (row * ldb + 4 * q - in_a) * 4;
#pragma unroll
    for (int s = 0; s < KS_IN_MAX; s++) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = 16 * s + 4 * q + j;
            const float fa = ldf(rXa, (row_ok && k < in_a) ? oa : OOR, (16 * s + j) * 4);
            const float fb = ldf(rXb, (row_ok && k >= in_a && k < in_dim) ? ob + (16 * s + j) * 4 : OOR, 0);
            v[j] = k < in_a ? fa : fb;
        }
        bx[s] = f32x4{v[0], v[1], v[2], v[3]};
    }
}

// output epilogue of a lane that holds a row's layer-3 sums: z + b3, the optional scale * sigmoid, store
__device__ __forceinline__ void store_out(f32x4 z4, const float* __restrict__ b3, int act, float scale, float* __restrict__ out, int row, int out_dim) {
    const float z[4] = {z4.x, z4.y, z4.z, z4.w};
    for (int i = 0; i < out_dim; i++) {
        float y = z[i] + b3[i];
        if (act == KR_ACT_SIGMOID) y = scale / (1.f + __expf(-y));
        out[(long)row * out_dim + i] = y;
    }
}

// backward of ReLU on a quad: the gradient passes where the forward activation hv was positive
__device__ __forceinline__ f32x4 relu_mask(f32x4 hv, f32x4 acc) {
    f32x4 dz;
    dz.x = hv.x > 0.f ? acc.x : 0.f; dz.y = hv.y > 0.f ? acc.y : 0.f; dz.z = hv.z > 0.f ? acc.z : 0.f; dz.w = hv.w > 0.f ? acc.w : 0.f;
    return dz;
}

// dx epilogue of a lane that holds a row's <= 4 input gradients, with the optional backward of  a = scale * sigmoid(z):  dz = dx * a (1 - a / scale)
__device__ __forceinline__ void store_dx(f32x4 accx, int ncol, const float* __restrict__ act_out, float scale, float* __restrict__ dx_out, int row) {
    const float g[4] = {accx.x, accx.y, accx.z, accx.w};
    for (int i = 0; i < ncol; i++) {
        float v = g[i];
        if (act_out) { const float a = act_out[(long)row * ncol + i]; v *= a * (1.f - a / scale); }
        dx_out[(long)row * ncol + i] = v;
    }
}

// The partial sums of a workgroup's NWS waves (lanes q == 0 hold the <= 4 sums of row nn) meet in scratch, `partial` =
// [block][wave][64]: on the lanes `lead` (wave 0's lanes q == 0, which the caller tests for its epilogue anyway) the return value is
// their sum in wave order (deterministic), elsewhere acc itself.  Every thread of the workgroup must call this (a barrier inside).
template <int NWS>
__device__ __forceinline__ f32x4 wave_sum(f32x4 acc, float* __restrict__ partial, int wave, int nn, int q, bool lead) {
    float* pw = partial + ((long)blockIdx.x * NWS + wave) * 64;
    if (q == 0) *(f32x4*)(pw + 4 * nn) = acc;
    __threadfence_block();
    __syncthreads();
    if (lead) {
        const rsrc_t rP = rsrc(partial + (long)blockIdx.x * NWS * 64, NWS * 64 * 4);
#pragma unroll
        for (int w = 1; w < NWS; w++) acc += ldq_glc(rP, (w * 64 + 4 * nn) * 4, 0);
    }
    return acc;
}

// ---- ONE WAVE = 16 batch rows, all layers in registers.  Layer 1's output quads (NT1 float4 registers) are the B operands of
// layer 2; every layer-2 output quad feeds layer 3's MFMAs right away, so h2 is never stored.  The kernel is capped at 168 registers per lane (3 waves per SIMD): k_env_step holds all of a
// CU's LDS and 344 of the 512 registers of every SIMD lane, so these waves can be resident BESIDE it and use the
// matrix pipes and issue slots the stepping kernel leaves idle - the learner's forward-only passes run in its shadow
// instead of waiting for its workgroups to retire.  Slower per wave than the LDS kernel (no split of the tiles over
// four waves), which does not matter there.  (The host checks h1 % 16 == h2 % 16 == 0 for this form.)
template <int NT1, int NT2>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_mlp3_wave(
    int n, int in_a, int in_b, int h1, int h2, int out_dim, const float* __restrict__ xa, int lda, const float* __restrict__ xb, int ldb,
    const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
    const float* __restrict__ W3, const float* __restrict__ b3, int act, float scale, float* __restrict__ out, float* __restrict__ h1_out,
    float* __restrict__ h2_out) {
    const int lane = threadIdx.x & 63, nn = lane & 15, q = lane >> 4;
    const int row = blockIdx.x * ROWS + nn;
    const bool row_ok = row < n;
    const int in_dim = in_a + in_b;
    const rsrc_t rW1 = rsrc(W1, h1 * in_dim * 4), rW2 = rsrc(W2, h2 * h1 * 4), rW3 = rsrc(W3, out_dim * h2 * 4);
    f32x4 h1r[NT1];
    {
        f32x4 bx[KS_IN_MAX];
        input_quads(bx, n, row, q, in_a, in_b, xa, lda, xb, ldb);
        // A operands: W1[16 t + nn][16 s + 4 q + j], zero beyond in_dim
        const int o1 = (nn * in_dim + 4 * q) * 4;
#pragma unroll
        for (int t = 0; t < NT1; t++) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS_IN_MAX; s++) {
                const int so = (16 * t * in_dim + 16 * s) * 4, k0 = 16 * s + 4 * q;
                const f32x4 w = {ldf(rW1, k0 < in_dim ? o1 : OOR, so), ldf(rW1, k0 + 1 < in_dim ? o1 : OOR, so + 4),
                                 ldf(rW1, k0 + 2 < in_dim ? o1 : OOR, so + 8), ldf(rW1, k0 + 3 < in_dim ? o1 : OOR, so + 12)};
                if (s & 1) acc1 = mfma4(w, bx[s], acc1);
                else acc0 = mfma4(w, bx[s], acc0);
            }
            h1r[t] = bias_relu(acc0 + acc1, b1, t * 16 + 4 * q, h1);
            if (h1_out && row_ok) *(f32x4*)(h1_out + (long)row * h1 + t * 16 + 4 * q) = h1r[t];
        }
    }
    f32x4 acc3 = {0.f, 0.f, 0.f, 0.f};
    const int o2 = (nn * h1 + 4 * q) * 4;                       // W2[16 t + nn][16 s + 4 q ..]: 16-byte reads (h1 % 4 == 0)
    const int o3 = (nn * h2 + 4 * q) * 4;                       // W3[nn][16 t + 4 q ..]: rows >= out_dim do not exist
#pragma unroll 1
    for (int t = 0; t < NT2; t ++) {
        f32x4 w[NT1];
#pragma unroll
        for (int s = 0; s < NT1; s++) w[s] = ldq(rW2, o2, (16 * t * h1 + 16 * s) * 4);
        const f32x4 w3 = ldq(rW3, nn < out_dim ? o3 : OOR, 16 * t * 4);
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NT1; s++) {
            if (s & 1) acc1 = mfma4(w[s], h1r[s], acc1);
            else acc0 = mfma4(w[s], h1r[s], acc0);
        }
        const f32x4 hq = bias_relu(acc0 + acc1, b2, t * 16 + 4 * q, h2);
        if (h2_out && row_ok) *(f32x4*)(h2_out + (long)row * h2 + t * 16 + 4 * q) = hq;
        acc3 = mfma4(w3, hq, acc3);
    }
    if (q == 0 && row_ok) store_out(acc3, b3, act, scale, out, row, out_dim);
}

// ---- the tiles of a layer SPLIT over NWS waves of one workgroup (still 16 batch rows per workgroup).
// One wave per 16 rows is a serial chain of ~1400 MFMAs fed by ~1400 weight loads: 87 us whatever the batch, and the learner's
// five forward passes are more than half of an update that - early in training - is what an env-step waits for.  Here wave w
// computes the layer-1 tiles t = w (mod NWS), the waves exchange their output quads through global memory (the caller's
// h1_out, or scratch; L2 resident, read back with glc loads) across a workgroup barrier - no LDS, so the kernel still runs
// beside the stepping kernel - then wave w computes the layer-2 tiles t = w (mod NWS) and its share of layer 3, whose partial
// sums meet in scratch (wave_sum).  Per output element the layer-1 / layer-2 fma chains are those of k_mlp3_wave; only layer
// 3's sum is associated differently.
template <int NT1, int NT2, int NWS>
__global__ __launch_bounds__(64 * NWS) __attribute__((amdgpu_waves_per_eu(KS_SPLIT_WAVES_PER_EU, KS_SPLIT_WAVES_PER_EU))) void k_mlp3_split(
    int n, int in_a, int in_b, int h1, int h2, int out_dim, const float* __restrict__ xa, int lda, const float* __restrict__ xb, int ldb,
    const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
    const float* __restrict__ W3, const float* __restrict__ b3, int act, float scale, float* __restrict__ out, float* __restrict__ h1buf,
    int h1_rows, float* __restrict__ h2_out, float* __restrict__ partial) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nn = lane & 15, q = lane >> 4;
    const int row = blockIdx.x * ROWS + nn;
    const bool row_ok = row < n;
    const int in_dim = in_a + in_b;
    const rsrc_t rW1 = rsrc(W1, h1 * in_dim * 4), rW2 = rsrc(W2, h2 * h1 * 4), rW3 = rsrc(W3, out_dim * h2 * 4), rH1 = rsrc(h1buf, h1_rows * h1 * 4);
    {
        f32x4 bx[KS_IN_MAX];
        input_quads(bx, n, row, q, in_a, in_b, xa, lda, xb, ldb);
        const int o1 = (nn * in_dim + 4 * q) * 4;                 // (the tiles of k_mlp3_wave, this wave's share)
#pragma unroll 1
        for (int t = wave; t < NT1; t += NWS) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS_IN_MAX; s++) {
                const int so = (16 * t * in_dim + 16 * s) * 4, k0 = 16 * s + 4 * q;
                const f32x4 w = {ldf(rW1, k0 < in_dim ? o1 : OOR, so), ldf(rW1, k0 + 1 < in_dim ? o1 : OOR, so + 4),
                                 ldf(rW1, k0 + 2 < in_dim ? o1 : OOR, so + 8), ldf(rW1, k0 + 3 < in_dim ? o1 : OOR, so + 12)};
                if (s & 1) acc1 = mfma4(w, bx[s], acc1);
                else acc0 = mfma4(w, bx[s], acc0);
            }
            const f32x4 hq = bias_relu(acc0 + acc1, b1, t * 16 + 4 * q, h1);
            if (row < h1_rows) *(f32x4*)(h1buf + (long)row * h1 + t * 16 + 4 * q) = hq;
        }
    }
    __threadfence_block();
    __syncthreads();
    // every wave takes the whole layer-1 output of its 16 rows as B operands (glc: written by the other waves of this workgroup)
    f32x4 h1r[NT1];
    {
        const int oh = row < h1_rows ? (row * h1 + 4 * q) * 4 : OOR;
#pragma unroll
        for (int s = 0; s < NT1; s++) h1r[s] = ldq_glc(rH1, oh, 16 * s * 4);
    }
    f32x4 acc3 = {0.f, 0.f, 0.f, 0.f};
    const int o2 = (nn * h1 + 4 * q) * 4, o3 = (nn * h2 + 4 * q) * 4;
#pragma unroll 1
    for (int t = wave; t < NT2; t += NWS) {                     // (the layer-2 / layer-3 tile loop of k_mlp3_wave, this wave's share)
        f32x4 w[NT1];
#pragma unroll
        for (int s = 0; s < NT1; s++) w[s] = ldq(rW2, o2, (16 * t * h1 + 16 * s) * 4);
        const f32x4 w3 = ldq(rW3, nn < out_dim ? o3 : OOR, 16 * t * 4);
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NT1; s++) {
            if (s & 1) acc1 = mfma4(w[s], h1r[s], acc1);
            else acc0 = mfma4(w[s], h1r[s], acc0);
        }
        const f32x4 hq = bias_relu(acc0 + acc1, b2, t * 16 + 4 * q, h2);
        if (h2_out && row_ok) *(f32x4*)(h2_out + (long)row * h2 + t * 16 + 4 * q) = hq;
        acc3 = mfma4(w3, hq, acc3);
    }
    const f32x4 z4 = wave_sum<NWS>(acc3, partial, wave, nn, q, wave == 0 && q == 0);
    if (wave == 0 && q == 0 && row_ok) store_out(z4, b3, act, scale, out, row, out_dim);
}

// ---- backward of the same network, also without LDS: one wave = 16 batch rows (NWS = 1, k_mlp3_bwd_wave), or the tiles of dz1
// split over the NWS waves of a workgroup as in k_mlp3_split (k_mlp3_bwd_split).
// Data gradients: with dz3 = dLoss/d(output pre-activation) [n, out_dim],
//     dz2 = (dz3 W3) * [h2 > 0],   dz1 = (dz2 W2) * [h1 > 0],   dx = dz1 W1[:, col0 : col0 + ncol]   (optional)
// again in the transposed orientation: dh^T = W^T dz^T, A = W^T (16 features of the layer below x 4 k), B = dz^T
// (4 k x 16 rows); the masked output quads are the next product's B operands, exactly as in the forward kernel.
// dx (<= 4 columns: the action inputs of the critic, DDPGfD.py:345-349) can be followed in the epilogue by the
// backward of  a = scale * sigmoid(z)  (store_dx; kr_sigmoid_scale_backward), which makes it the dz3 of the actor.
// dz2_out / dz1_out may be NULL when only dx is wanted.  Every wave computes dz2 itself (one MFMA per tile), wave w the dz1
// tiles t = w (mod NWS); the partial sums of dx meet in scratch (wave_sum), which NWS = 1 does without.
template <int NT1, int NT2, int NWS>
__device__ __forceinline__ void mlp3_bwd_rows16(int n, int in_dim, int h1, int h2, int out_dim, const float* __restrict__ dz3, const float* __restrict__ W3,
                                                const float* __restrict__ h2a, const float* __restrict__ W2, const float* __restrict__ h1a,
                                                float* __restrict__ dz2_out, float* __restrict__ dz1_out, const float* __restrict__ W1, int col0, int ncol,
                                                const float* __restrict__ act_out, float scale, float* __restrict__ dx_out, float* __restrict__ partial) {
    const int wave = NWS == 1 ? 0 : threadIdx.x >> 6, lane = threadIdx.x & 63, nn = lane & 15, q = lane >> 4;
    const int row = blockIdx.x * ROWS + nn;
    const bool row_ok = row < n;
    // B operand of the first product: dz3^T, k = output index = q
    const float b3 = (row_ok && q < out_dim) ? dz3[(long)row * out_dim + q] : 0.f;
    f32x4 dz2r[NT2];
#pragma unroll
    for (int t = 0; t < NT2; t++) {
        const int f = t * 16 + nn;                                          // A: W3^T[f][k = q] = W3[q][f]
        const float a3 = (q < out_dim && f < h2) ? W3[(long)q * h2 + f] : 0.f;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, b3, acc, 0, 0, 0);
        const int f4 = t * 16 + 4 * q;
        f32x4 hv = {0.f, 0.f, 0.f, 0.f};
        if (row_ok && f4 < h2) hv = *(const f32x4*)(h2a + (long)row * h2 + f4);
        const f32x4 dz = relu_mask(hv, acc);
        dz2r[t] = dz;
        if (dz2_out && row_ok && f4 < h2 && (NWS == 1 || t % NWS == wave)) *(f32x4*)(dz2_out + (long)row * h2 + f4) = dz;
    }
    f32x4 accx = {0.f, 0.f, 0.f, 0.f};
    const rsrc_t rW2 = rsrc(W2, h1 * h2 * 4);
#pragma unroll 1
    for (int t = wave; t < NT1; t += NWS) {
        // A: W2^T[f][k] = W2[k][f], k = 16 s + 4 q + j (rows of W2, stride h1), f = 16 t + nn
        const int f = t * 16 + nn;
        // (host checks h1 % 16 == h2 % 16 == 0: every row / column of the tile exists).  Buffer loads: ONE 32-bit lane
        // offset for the whole tile, the row steps (16 s + j) * h1 are wave-uniform and go in the scalar offset - flat
        // loads would hold a 64-bit address per load in flight and spill at this register budget.  (The load builtin as it
        // stands: through kmlp::ldf the split instantiations at 64-64 and 128-128 allocate 1 - 3 more registers.)
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const int voff = (4 * q * h1 + f) * 4;
        constexpr int HALF = (NT2 + 1) / 2;
#pragma unroll
        for (int half = 0; half < 2; half++) {
            f32x4 w[HALF];
#pragma unroll
            for (int u = 0; u < HALF; u++) {
                const int s = half * HALF + u;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (s < NT2) {
                    v.x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rW2, voff, (16 * s + 0) * h1 * 4, 0));
                    v.y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rW2, voff, (16 * s + 1) * h1 * 4, 0));
                    v.z = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rW2, voff, (16 * s + 2) * h1 * 4, 0));
                    v.w = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rW2, voff, (16 * s + 3) * h1 * 4, 0));
                }
                w[u] = v;
            }
#pragma unroll
            for (int u = 0; u < HALF; u++) {
                const int s = half * HALF + u;
                if (s < NT2) {
                    if (s & 1) acc1 = mfma4(w[u], dz2r[s], acc1);
                    else acc0 = mfma4(w[u], dz2r[s], acc0);
                }
            }
        }
        const f32x4 acc = acc0 + acc1;
        const int f4 = t * 16 + 4 * q;
        f32x4 hv = {0.f, 0.f, 0.f, 0.f};
        if (row_ok && f4 < h1) hv = *(const f32x4*)(h1a + (long)row * h1 + f4);
        const f32x4 dz = relu_mask(hv, acc);
        if (dz1_out && row_ok && f4 < h1) *(f32x4*)(dz1_out + (long)row * h1 + f4) = dz;
        if (dx_out) {
            // A: W1[:, col0 + m]^T: [m][k] = W1[k][col0 + m], k = 16 t + 4 q + j (rows of W1, stride in_dim), m = nn < ncol
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (nn < ncol) {
                const int k = 16 * t + 4 * q;
                const float* p = W1 + (long)k * in_dim + col0 + nn;
                if (k < h1) v.x = p[0];
                if (k + 1 < h1) v.y = p[in_dim];
                if (k + 2 < h1) v.z = p[2 * (long)in_dim];
                if (k + 3 < h1) v.w = p[3 * (long)in_dim];
            }
            accx = mfma4(v, dz, accx);
        }
    }
    if constexpr (NWS > 1) {
        if (dx_out) accx = wave_sum<NWS>(accx, partial, wave, nn, q, wave == 0 && q == 0);
    }
    if (dx_out && wave == 0 && q == 0 && row_ok) store_dx(accx, ncol, act_out, scale, dx_out, row);
}

template <int NT1, int NT2>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_mlp3_bwd_wave(
    int n, int in_dim, int h1, int h2, int out_dim, const float* __restrict__ dz3, const float* __restrict__ W3, const float* __restrict__ h2a,
    const float* __restrict__ W2, const float* __restrict__ h1a, float* __restrict__ dz2_out, float* __restrict__ dz1_out,
    const float* __restrict__ W1, int col0, int ncol, const float* __restrict__ act_out, float scale, float* __restrict__ dx_out) {
    mlp3_bwd_rows16<NT1, NT2, 1>(n, in_dim, h1, h2, out_dim, dz3, W3, h2a, W2, h1a, dz2_out, dz1_out, W1, col0, ncol, act_out, scale, dx_out, nullptr);
}

template <int NT1, int NT2, int NWS>
__global__ __launch_bounds__(64 * NWS) __attribute__((amdgpu_waves_per_eu(KS_SPLIT_WAVES_PER_EU, KS_SPLIT_WAVES_PER_EU))) void k_mlp3_bwd_split(
    int n, int in_dim, int h1, int h2, int out_dim, const float* __restrict__ dz3, const float* __restrict__ W3, const float* __restrict__ h2a,
    const float* __restrict__ W2, const float* __restrict__ h1a, float* __restrict__ dz2_out, float* __restrict__ dz1_out,
    const float* __restrict__ W1, int col0, int ncol, const float* __restrict__ act_out, float scale, float* __restrict__ dx_out,
    float* __restrict__ partial) {
    mlp3_bwd_rows16<NT1, NT2, NWS>(n, in_dim, h1, h2, out_dim, dz3, W3, h2a, W2, h1a, dz2_out, dz1_out, W1, col0, ncol, act_out, scale, dx_out, partial);
}

// ---- the LEAN kernels: the same forward and backward for tile pairs too wide for k_mlp3_wave / k_mlp3_bwd_wave, which keep
// a whole hidden layer in registers (at 25 tiles that alone is 100).  The free-running rollout kernel at the reference's 400-300
// (k_rollout<25,19>) holds 416 of the 512 registers of every SIMD lane for a whole launch: a learner wave is resident beside it
// only at <= 96, and these two kernels are capped there (amdgpu_waves_per_eu(5, 5): 512 / 5, rounded down to the allocation
// granule of 8, is 96; tools/learner_budget.py checks the sums).  Data flow: one wave = 16 batch rows as before, but NO layer stays
// in registers.  The first product's output quads go to global memory (the caller's h1_out / dz2_out, or scratch) and come back
// as the B operands of the second product's k-loop, LEAN_KC k-steps per round, together with the weight quads; every quad is read
// back by the lane that wrote it (the D layout of one MFMA is the B layout of the next), behind a fence and with glc loads.
// A round's loads serve TWO output tiles (one B quad, two A quads per k-step: 12 registers instead of 16), which halves the
// number of dependent load rounds - the kernels are bound by those, not by the matrix pipe.
// Partial last tiles are right by construction: every element at or beyond h1 / h2 - a row of the A tile or a k of the
// reduction - gets an out-of-range LANE offset, so it is read as zero and never touches memory (the tile and k steps sit in the
// scalar offset, which the hardware's range check does not cover: the end of the buffer protects nothing), and is never stored.
constexpr int LEAN_KC = 5;                   // k-steps per load round: 3 quads x 5 = 60 registers of operands in flight
#define KS_LEAN_ATTR __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5)))
// all loads of a round are issued before its first MFMA: left alone, the scheduler interleaves them and waits for each in turn
#define KS_LEAN_LOADS_FIRST() __builtin_amdgcn_sched_barrier(0)

template <int NT1, int NT2>
__global__ KS_LEAN_ATTR void k_mlp3_lean(
    int n, int in_a, int in_b, int h1, int h2, int out_dim, const float* __restrict__ xa, int lda, const float* __restrict__ xb, int ldb,
    const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
    const float* __restrict__ W3, const float* __restrict__ b3, int act, float scale, float* __restrict__ out, float* __restrict__ h1buf,
    int h1_rows, float* __restrict__ h2_out) {
    const int lane = threadIdx.x & 63, nn = lane & 15, q = lane >> 4;
    const int row = blockIdx.x * ROWS + nn;
    const bool row_ok = row < n;
    const int in_dim = in_a + in_b;
    const auto rW1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W1), 0, h1 * in_dim * 4, 0x00020000);
    const auto rW2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W2), 0, h2 * h1 * 4, 0x00020000);
    const auto rW3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W3), 0, out_dim * h2 * 4, 0x00020000);
    const auto rH1 = __builtin_amdgcn_make_buffer_rsrc(h1buf, 0, h1_rows * h1 * 4, 0x00020000);
    {
        f32x4 bx[KS_IN_MAX];
        const auto rXa = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xa), 0, ((n - 1) * lda + in_a) * 4, 0x00020000);
        const auto rXb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb ? xb : xa), 0, xb ? ((n - 1) * ldb + in_b) * 4 : 0, 0x00020000);
        // B operands of layer 1: input_quads written out, as are this kernel's resources and its output epilogue - through the helpers
        // the compiler schedules its load rounds 1 - 3 % slower (profiles/mlp_front_end.txt)
        const int oa = row * lda * 4 + 16 * q, ob = (row * ldb + 4 * q - in_a) * 4;
#pragma unroll
        for (int s = 0; s < KS_IN_MAX; s++) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int k = 16 * s + 4 * q + j;
                const float fa = ldf(rXa, (row_ok && k < in_a) ? oa : OOR, (16 * s + j) * 4);
                const float fb = ldf(rXb, (row_ok && k >= in_a && k < in_dim) ? ob + (16 * s + j) * 4 : OOR, 0);
                v[j] = k < in_a ? fa : fb;
            }
            bx[s] = f32x4{v[0], v[1], v[2], v[3]};
        }
        // layer 1, one tile per round: A = W1[16 t + nn][16 s + 4 q + j], zero beyond h1 rows / in_dim columns
        const int o1 = (nn * in_dim + 4 * q) * 4;
#pragma unroll 1
        for (int t = 0; t < NT1; t++) {
            const bool rok = 16 * t + nn < h1;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            f32x4 w[KS_IN_MAX];
#pragma unroll
            for (int s = 0; s < KS_IN_MAX; s++) {
                const int so = (16 * t * in_dim + 16 * s) * 4, k0 = 16 * s + 4 * q;
                w[s] = f32x4{ldf(rW1, (rok && k0 < in_dim) ? o1 : OOR, so), ldf(rW1, (rok && k0 + 1 < in_dim) ? o1 : OOR, so + 4),
                             ldf(rW1, (rok && k0 + 2 < in_dim) ? o1 : OOR, so + 8), ldf(rW1, (rok && k0 + 3 < in_dim) ? o1 : OOR, so + 12)};
            }
            KS_LEAN_LOADS_FIRST();
#pragma unroll
            for (int s = 0; s < KS_IN_MAX; s++) {
                if (s & 1) acc1 = mfma4(w[s], bx[s], acc1);
                else acc0 = mfma4(w[s], bx[s], acc0);
            }
            const int f4 = t * 16 + 4 * q;
            const f32x4 hq = bias_relu(acc0 + acc1, b1, f4, h1);
            if (f4 < h1 && row < h1_rows) *(f32x4*)(h1buf + (long)row * h1 + f4) = hq;
        }
    }
    __threadfence_block();          // the quads above are read back below, each by the lane that stored it (glc loads)
    f32x4 acc3 = {0.f, 0.f, 0.f, 0.f};
    const int o2 = (nn * h1 + 4 * q) * 4;                       // W2[16 t + nn][16 s + 4 q ..]: 16-byte reads (h1 % 4 == 0)
    const int o3 = (nn * h2 + 4 * q) * 4;                       // W3[nn][16 t + 4 q ..]
    const int oh = row < h1_rows ? (row * h1 + 4 * q) * 4 : OOR;
    constexpr int NC = (NT1 + LEAN_KC - 1) / LEAN_KC;
#pragma unroll 1
    for (int t = 0; t < NT2; t += 2) {                          // tiles t and t + 1 (a tile at or beyond NT2: every row masked)
        f32x4 acca = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
        const int oa = 16 * t + nn < h2 ? o2 : OOR, ob = 16 * (t + 1) + nn < h2 ? o2 : OOR;
#pragma unroll 1
        for (int c = 0; c < NC; c++) {
            f32x4 wa[LEAN_KC], wb[LEAN_KC], hb[LEAN_KC];
#pragma unroll
            for (int u = 0; u < LEAN_KC; u++) {
                const int s = c * LEAN_KC + u;
                const bool kok = (NT1 % LEAN_KC == 0 || s < NT1) && 16 * s + 4 * q < h1;
                hb[u] = ldq_glc(rH1, kok ? oh : OOR, 16 * s * 4);
                wa[u] = ldq(rW2, kok ? oa : OOR, (16 * t * h1 + 16 * s) * 4);
                wb[u] = ldq(rW2, kok ? ob : OOR, (16 * (t + 1) * h1 + 16 * s) * 4);
            }
            KS_LEAN_LOADS_FIRST();
#pragma unroll
            for (int u = 0; u < LEAN_KC; u++) {
                acca = mfma4(wa[u], hb[u], acca);
                accb = mfma4(wb[u], hb[u], accb);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int f4 = (t + u) * 16 + 4 * q;
            const f32x4 hq = bias_relu(u ? accb : acca, b2, f4, h2);
            if (h2_out && row_ok && f4 < h2) *(f32x4*)(h2_out + (long)row * h2 + f4) = hq;
            const f32x4 w3 = ldq(rW3, (nn < out_dim && f4 < h2) ? o3 : OOR, 16 * (t + u) * 4);
            acc3 = mfma4(w3, hq, acc3);
        }
    }
    if (q == 0 && row_ok) {
        const float z[4] = {acc3.x, acc3.y, acc3.z, acc3.w};
        for (int i = 0; i < out_dim; i++) {
            float y = z[i] + b3[i];
            if (act == KR_ACT_SIGMOID) y = scale / (1.f + __expf(-y));
            out[(long)row * out_dim + i] = y;
        }
    }
}

// backward (the arithmetic of k_mlp3_bwd_wave): the masked dz2 quads (one MFMA each) go to dz2buf, then every pair of dz1 tiles
// streams them back with the W2^T quads; dx accumulates in four registers.
template <int NT1, int NT2>
__global__ KS_LEAN_ATTR void k_mlp3_bwd_lean(
    int n, int in_dim, int h1, int h2, int out_dim, const float* __restrict__ dz3, const float* __restrict__ W3, const float* __restrict__ h2a,
    const float* __restrict__ W2, const float* __restrict__ h1a, float* __restrict__ dz2buf, float* __restrict__ dz1_out,
    const float* __restrict__ W1, int col0, int ncol, const float* __restrict__ act_out, float scale, float* __restrict__ dx_out, int dz2_rows) {
    const int lane = threadIdx.x & 63, nn = lane & 15, q = lane >> 4;
    const int row = blockIdx.x * ROWS + nn;
    const bool row_ok = row < n;
    const rsrc_t rW3 = rsrc(W3, out_dim * h2 * 4), rW2 = rsrc(W2, h2 * h1 * 4), rH2 = rsrc(h2a, n * h2 * 4), rH1 = rsrc(h1a, n * h1 * 4),
                 rD2 = rsrc(dz2buf, dz2_rows * h2 * 4);
    // B operand of the first product: dz3^T, k = output index = q
    const float b3 = (row_ok && q < out_dim) ? dz3[(long)row * out_dim + q] : 0.f;
    {
        const int o3 = (q * h2 + nn) * 4;                                   // A: W3^T[f][k = q] = W3[q][f], f = 16 t + nn
        const int oh2 = row_ok ? (row * h2 + 4 * q) * 4 : OOR;
#pragma unroll 1
        for (int t0 = 0; t0 < NT2; t0 += 4) {
            float a3[4];
            f32x4 hv[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int t = t0 + u;
                a3[u] = ldf(rW3, (q < out_dim && 16 * t + nn < h2) ? o3 : OOR, 16 * t * 4);
                hv[u] = ldq(rH2, 16 * t + 4 * q < h2 ? oh2 : OOR, 16 * t * 4);
            }
            KS_LEAN_LOADS_FIRST();
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int f4 = (t0 + u) * 16 + 4 * q;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a3[u], b3, acc, 0, 0, 0);
                const f32x4 dz = relu_mask(hv[u], acc);
                if (f4 < h2 && row < dz2_rows) *(f32x4*)(dz2buf + (long)row * h2 + f4) = dz;
            }
        }
    }
    __threadfence_block();          // read back below by the lane that stored them (glc loads)
    f32x4 accx = {0.f, 0.f, 0.f, 0.f};
    const rsrc_t rW1 = rsrc(W1 ? W1 : W2, W1 ? h1 * in_dim * 4 : 0);
    const int od = row < dz2_rows ? (row * h2 + 4 * q) * 4 : OOR;
    const int oh1 = row_ok ? (row * h1 + 4 * q) * 4 : OOR;
    constexpr int NC = (NT2 + LEAN_KC - 1) / LEAN_KC;
#pragma unroll 1
    for (int t = 0; t < NT1; t += 2) {                          // tiles t and t + 1 (a tile at or beyond NT1: every row masked)
        // A: W2^T[f][k] = W2[k][f], k = 16 s + 4 q + j (rows of W2, stride h1: the steps (16 s + j) h1 are scalar), f = 16 t + nn
        f32x4 acca = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
        const int va = 16 * t + nn < h1 ? (4 * q * h1 + 16 * t + nn) * 4 : OOR, vb = 16 * (t + 1) + nn < h1 ? (4 * q * h1 + 16 * (t + 1) + nn) * 4 : OOR;
#pragma unroll 1
        for (int c = 0; c < NC; c++) {
            f32x4 wa[LEAN_KC], wb[LEAN_KC], db[LEAN_KC];
#pragma unroll
            for (int u = 0; u < LEAN_KC; u++) {
                const int s = c * LEAN_KC + u;
                const bool kok = (NT2 % LEAN_KC == 0 || s < NT2) && 16 * s + 4 * q < h2;       // h2 % 4 == 0: a quad exists as a whole
                const int ka = kok ? va : OOR, kb = kok ? vb : OOR;
                db[u] = ldq_glc(rD2, kok ? od : OOR, 16 * s * 4);
                wa[u] = f32x4{ldf(rW2, ka, (16 * s + 0) * h1 * 4), ldf(rW2, ka, (16 * s + 1) * h1 * 4), ldf(rW2, ka, (16 * s + 2) * h1 * 4),
                              ldf(rW2, ka, (16 * s + 3) * h1 * 4)};
                wb[u] = f32x4{ldf(rW2, kb, (16 * s + 0) * h1 * 4), ldf(rW2, kb, (16 * s + 1) * h1 * 4), ldf(rW2, kb, (16 * s + 2) * h1 * 4),
                              ldf(rW2, kb, (16 * s + 3) * h1 * 4)};
            }
            KS_LEAN_LOADS_FIRST();
#pragma unroll
            for (int u = 0; u < LEAN_KC; u++) {
                acca = mfma4(wa[u], db[u], acca);
                accb = mfma4(wb[u], db[u], accb);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int f4 = (t + u) * 16 + 4 * q;
            const f32x4 hv = ldq(rH1, f4 < h1 ? oh1 : OOR, 16 * (t + u) * 4);
            const f32x4 dz = relu_mask(hv, u ? accb : acca);
            if (dz1_out && row_ok && f4 < h1) *(f32x4*)(dz1_out + (long)row * h1 + f4) = dz;
            if (dx_out) {
                // A: W1[:, col0 + m]^T: [m][k] = W1[k][col0 + m], k = 16 t + 4 q + j (rows of W1, stride in_dim), m = nn < ncol
                const int vx = (nn < ncol && f4 < h1) ? ((4 * q * in_dim) + col0 + nn) * 4 : OOR;
                const int sx = 16 * (t + u) * in_dim * 4;
                const f32x4 v = {ldf(rW1, vx, sx), ldf(rW1, vx, sx + in_dim * 4), ldf(rW1, vx, sx + 2 * in_dim * 4), ldf(rW1, vx, sx + 3 * in_dim * 4)};
                accx = mfma4(v, dz, accx);
            }
        }
    }
    if (dx_out && q == 0 && row_ok) store_dx(accx, ncol, act_out, scale, dx_out, row);
}
#undef KS_LEAN_LOADS_FIRST

// Weight gradients  dW[M][N] = dz^T h  (dz [n][M], h = [ha | hb] [n][N]) and the bias gradient  db[M] = column sums of dz,
// without LDS: a wave owns one 16-row tile of dW and TN 16-column tiles, and one chunk of the batch rows; A = dz^T
// (lane: feature m, row k), B = h (lane: row k, column).  The chunk partials go to a workspace [chunk][M * N + M] that
// k_wgrad_reduce sums in chunk order (deterministic, unlike atomics).
//
// INDEXED (kr_weight_grad_indexed): term r of the sums is row idx[r] of dz / ha / hb, which then hold `rows` rows - the learner's episode
// tables, every state evaluated once and read by each of the ~4 window rows that hold it.  The n terms, their order, the chunks and the
// rounds are those of the plain form, so the sums are its bits on the gathered rows; a term with idx[r] outside [0, rows) reads as
// zeros.  The row advance moves from the scalar offset into the lane offset; the indices of round k + 1 are loaded ahead of round k's
// operands.
constexpr int WG_TN = 4;
template <bool INDEXED>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_wgrad_wave(
    int n, int rows, int M, int Na, int Nb, int rows_per_chunk, const float* __restrict__ dz, const float* __restrict__ ha, int lda,
    const float* __restrict__ hb, int ldb, const int* __restrict__ idx, float* __restrict__ ws) {
    const int lane = threadIdx.x & 63, nn = lane & 15, q = lane >> 4;
    const int N = Na + Nb, n_blocks = (N + 16 * WG_TN - 1) / (16 * WG_TN);
    const int mt = blockIdx.x / n_blocks, nb = blockIdx.x % n_blocks, chunk = blockIdx.y;
    const int r0 = chunk * rows_per_chunk, r1 = min(n, r0 + rows_per_chunk);
    const int m = mt * 16 + nn;
    // Raw buffer loads (as in k_mlp3_wave): per matrix ONE lane offset (row q of a 4-row group, this lane's column), the row
    // advance in the wave-uniform scalar offset; an element that does not exist gets an out-of-range lane offset (-> 0).
    // The flat-load version spent ~10 VALU + ~20 SALU instructions per MFMA on addresses and bounds branches.
    const auto rZ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dz), 0, rows * M * 4, 0x00020000);
    const auto rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ha), 0, ((rows - 1) * lda + Na) * 4, 0x00020000);
    const auto rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(hb ? hb : ha), 0, hb ? ((rows - 1) * ldb + Nb) * 4 : 0, 0x00020000);
    const auto rI = __builtin_amdgcn_make_buffer_rsrc(const_cast<int*>(INDEXED ? idx : nullptr), 0, INDEXED ? n * 4 : 0, 0x00020000);
    const int row_q = INDEXED ? 0 : q;            // (indexed: the lane's row comes with its index)
    const int vz = m < M ? (row_q * M + m) * 4 : OOR;
    int va[WG_TN], vb[WG_TN];
#pragma unroll
    for (int u = 0; u < WG_TN; u++) {
        const int c = (nb * WG_TN + u) * 16 + nn;
        va[u] = c < Na ? (row_q * lda + c) * 4 : OOR;
        vb[u] = (c >= Na && c < N) ? (row_q * ldb + c - Na) * 4 : OOR;
    }
    f32x4 acc[WG_TN];
#pragma unroll
    for (int u = 0; u < WG_TN; u++) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    float colsum = 0.f;
    // four k-steps (16 rows) per round, all loads first; only the last round of a chunk can hold rows that do not exist
    // (id: INDEXED, the table rows of this lane's four terms of the round)
    auto round = [&](int k0, const int* id, auto guard, auto hasb) {
        constexpr bool GUARD = decltype(guard)::value, HASB = decltype(hasb)::value;
        float a[4], b[4][WG_TN];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int rj = k0 + 4 * j;                                 // wave-uniform; this lane's row is rj + q
            bool ok = !GUARD || rj + q < r1;
            if constexpr (INDEXED) {
                // the row's byte offset joins the lane offset; a term that is no row gets OOR there, and OOR plus a column offset - or
                // plus another OOR - is still beyond every resource as the unsigned 32-bit offset the hardware compares
                ok = ok && (unsigned)id[j] < (unsigned)rows;
                const uint32_t oz = ok ? (uint32_t)(id[j] * M * 4) : OOR, oa = ok ? (uint32_t)(id[j] * lda * 4) : OOR;
                a[j] = ldf(rZ, (uint32_t)vz + oz, 0);
#pragma unroll
                for (int u = 0; u < WG_TN; u++) {
                    float v = ldf(rA, (uint32_t)va[u] + oa, 0);
                    if (HASB) v += ldf(rB, (uint32_t)vb[u] + (ok ? (uint32_t)(id[j] * ldb * 4) : OOR), 0);
                    b[j][u] = v;
                }
                continue;
            }
            a[j] = ldf(rZ, ok ? vz : OOR, rj * M * 4);
#pragma unroll
            for (int u = 0; u < WG_TN; u++) {
                float v = ldf(rA, ok ? va[u] : OOR, rj * lda * 4);
                if (HASB) v += ldf(rB, ok ? vb[u] : OOR, rj * ldb * 4);      // at most one of the two exists
                b[j][u] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            colsum += a[j];
#pragma unroll
            for (int u = 0; u < WG_TN; u++) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j][u], acc[u], 0, 0, 0);
        }
    };
    const int full_end = r0 + ((r1 - r0) >> 4 << 4);
    // the rounds of the chunk; INDEXED: the next round's indices are in flight before this round's operands are asked for (the row is in the
    // lane offset, which the range check covers: an index at or past n is not read at all and comes back as 0; it is never used - the
    // guarded round masks it, or the loop has ended)
    auto rounds = [&](auto hasb) {
        if constexpr (INDEXED) {
            int cur[4], nxt[4];
#pragma unroll
            for (int j = 0; j < 4; j++) cur[j] = __builtin_amdgcn_raw_buffer_load_b32(rI, (r0 + 4 * j + q) * 4, 0, 0);
            for (int k0 = r0; k0 < r1; k0 += 16) {
#pragma unroll
                for (int j = 0; j < 4; j++) nxt[j] = __builtin_amdgcn_raw_buffer_load_b32(rI, (k0 + 16 + 4 * j + q) * 4, 0, 0);
                if (k0 < full_end) round(k0, cur, std::false_type{}, hasb);
                else round(k0, cur, std::true_type{}, hasb);
#pragma unroll
                for (int j = 0; j < 4; j++) cur[j] = nxt[j];
            }
        } else {
            for (int k0 = r0; k0 < full_end; k0 += 16) round(k0, nullptr, std::false_type{}, hasb);
            if (full_end < r1) round(full_end, nullptr, std::true_type{}, hasb);
        }
    };
    if (Nb > 0) rounds(std::true_type{});
    else rounds(std::false_type{});
    float* out = ws + (long)chunk * ((long)M * N + M);
#pragma unroll
    for (int u = 0; u < WG_TN; u++) {
        const int c = (nb * WG_TN + u) * 16 + nn;
        const float v[4] = {acc[u].x, acc[u].y, acc[u].z, acc[u].w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int mr = mt * 16 + 4 * q + i;
            if (mr < M && c < N) out[(long)mr * N + c] = v[i];
        }
    }
    if (nb == 0) {
        colsum += __shfl_xor(colsum, 16);
        colsum += __shfl_xor(colsum, 32);
        if (q == 0 && m < M) out[(long)M * N + m] = colsum;
    }
}

__global__ __launch_bounds__(256) void k_wgrad_reduce(long count_w, long count_b, int chunks, const float* __restrict__ ws, float* __restrict__ dW,
                                                      float* __restrict__ db) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x, total = count_w + count_b;
    if (i >= total) return;
    float s = 0.f;
    for (int c = 0; c < chunks; c++) s += ws[(long)c * total + i];
    if (i < count_w) dW[i] = s;
    else db[i - count_w] = s;
}

// ---- host front end.  The arguments the forward entry points share, and those of the backward ones, as kinova_rollout.h names them.
struct Fwd {
    int n, in_a, in_b, h1, h2, out_dim;
    const float* xa; int lda; const float* xb; int ldb;
    const float *W1, *b1, *W2, *b2, *W3, *b3;
    int act; float scale;
    float *out, *h1_out, *h2_out;
};
struct Bwd {
    int n, in_dim, h1, h2, out_dim;
    const float *dz3, *W3, *h2a, *W2, *h1a;
    float *dz2_out, *dz1_out;
    const float* W1; int col0, ncol;
    const float* act_out; float scale;
    float* dx_out;
};

// what every forward form refuses; each entry point adds the conditions of its own form
bool fwd_args_ok(const Fwd& a) {
    if ((a.h1_out && (a.h1 % 4 || (uintptr_t)a.h1_out % 16)) || (a.h2_out && (a.h2 % 4 || (uintptr_t)a.h2_out % 16))) return false;
    if (!a.xa || !a.W1 || !a.b1 || !a.W2 || !a.b2 || !a.W3 || !a.b3 || !a.out || a.in_a <= 0 || a.in_b < 0 || (a.in_b > 0 && !a.xb)) return false;
    if (a.in_a + a.in_b > 16 * KS_IN_MAX || a.out_dim < 1 || a.out_dim > 4 || a.h1 < 1 || a.h2 < 1) return false;
    return a.act == KR_ACT_NONE || a.act == KR_ACT_SIGMOID;
}
// ... and every backward form (the hidden widths are each form's own)
bool bwd_args_ok(const Bwd& a) {
    if (!a.dz3 || !a.W3 || !a.h2a || !a.W2 || !a.h1a || a.out_dim < 1 || a.out_dim > 4) return false;
    if (a.dx_out && (!a.W1 || a.ncol < 1 || a.ncol > 4 || a.col0 < 0 || a.col0 + a.ncol > a.in_dim)) return false;
    return !((uintptr_t)a.h1a % 16 || (uintptr_t)a.h2a % 16 || (a.dz1_out && (uintptr_t)a.dz1_out % 16) || (a.dz2_out && (uintptr_t)a.dz2_out % 16));
}
// whole tiles, and 16-byte loads of W2 / W3 rows: the one-wave and split forms
bool whole_tiles(int h1, int h2) { return h1 >= 16 && h2 >= 16 && h1 % 16 == 0 && h2 % 16 == 0; }
bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// Tile pairs (NT1, NT2) with an instantiation, one list per form (mlp.py: SUPPORTED_TILES, SHADOW_TILES, LEAN_TILES).
// LIST(KR_PICK, kernel [, further template arguments]) leaves in `k` the kernel's instantiation for (nt1, nt2), if the list has the pair.
#define KR_MLP_PAIRS(CASE, ...)                                                                                                      \
    CASE(16, 16, __VA_ARGS__)    /* 256-256 (BASELINE) */                                                                            \
    CASE(25, 19, __VA_ARGS__)    /* 400-300 (reference, DDPGfD.py:19-23) */                                                          \
    CASE(8, 8, __VA_ARGS__)      /* 128-128 */                                                                                       \
    CASE(4, 4, __VA_ARGS__)      /* 64-64 (tests) */
// the one-wave and split forms: wider first layers do not fit the register budget
#define KR_SHADOW_PAIRS(CASE, ...) CASE(16, 16, __VA_ARGS__) CASE(8, 8, __VA_ARGS__) CASE(4, 4, __VA_ARGS__)
// the lean form: 400-300 and its partial tiles, e.g. 392-292; every lane offset is a 32-bit byte offset: rows * width * 4 must stay below OOR
#define KR_LEAN_PAIRS(CASE, ...) CASE(25, 19, __VA_ARGS__)
#define KR_PICK(A, B, K, ...) if (nt1 == A && nt2 == B) k = K<A, B, ##__VA_ARGS__>;

// one workgroup of `threads` per 16 rows; no instantiation (k == nullptr): these widths are not supported
template <typename... P, typename... A>
int launch(void (*k)(P...), int n, int threads, hipStream_t s, A... a) {
    if (!k) return KS_ERR_INVALID;
    hipLaunchKernelGGL(k, dim3((n + ROWS - 1) / ROWS), dim3(threads), 0, s, (P)a...);
    return hipGetLastError() == hipSuccess ? KS_OK : KS_ERR_HIP;
}
// ... of a forward kernel (every one takes the shared arguments up to `out`, then `tail`), of a backward kernel (dz2: where dz2 goes)
template <typename K, typename... T>
int launch_fwd(K k, int threads, void* stream, const Fwd& a, T... tail) {
    return launch(k, a.n, threads, (hipStream_t)stream, a.n, a.in_a, a.in_b, a.h1, a.h2, a.out_dim, a.xa, a.lda, a.xb, a.ldb, a.W1, a.b1, a.W2, a.b2, a.W3, a.b3,
                  a.act, a.scale, a.out, tail...);
}
template <typename K, typename... T>
int launch_bwd(K k, int threads, void* stream, const Bwd& a, float* dz2, T... tail) {
    return launch(k, a.n, threads, (hipStream_t)stream, a.n, a.in_dim, a.h1, a.h2, a.out_dim, a.dz3, a.W3, a.h2a, a.W2, a.h1a, dz2, a.dz1_out, a.W1, a.col0, a.ncol,
                  a.act_out, a.scale, a.dx_out, tail...);
}

// Where the split and lean forms pass a layer's output quads ([rows][width]) and the split forms' partial sums through global
// memory: the quads in the caller's own tensor `keep` ([n][width]) or, without one, in scratch for whole blocks of 16 rows;
// behind them in scratch 64 partial sums per block and wave.  False when scratch is needed and missing, misaligned or too small.
struct Exchange { float* buf; int rows; float* partial; };
bool exchange(Exchange& x, int n, int width, float* keep, int partial_waves, float* scratch, int64_t scratch_floats) {
    const int64_t blocks = (n + ROWS - 1) / ROWS;
    const int64_t quads = keep ? 0 : blocks * ROWS * width, need = quads + blocks * partial_waves * 64;
    if (need && (!scratch || !aligned16(scratch) || scratch_floats < need)) return false;
    x = Exchange{keep ? keep : scratch, keep ? n : (int)blocks * ROWS, scratch + quads};
    return true;
}

bool lean_widths_ok(int h1, int h2) {
    if (h1 < 1 || h2 < 1 || h1 % 4 || h2 % 4) return false;
    const int nt1 = (h1 + 15) / 16, nt2 = (h2 + 15) / 16;
#define KR_LEAN_IS(A, B, ...) || (nt1 == A && nt2 == B)
    return false KR_LEAN_PAIRS(KR_LEAN_IS);
#undef KR_LEAN_IS
}
bool lean_fits32(int64_t rows, int64_t width) { return rows * width * 4 < (int64_t)OOR; }

// k_mlp3 (the LDS form, any widths of its tile pairs): kr_mlp3_forward, and with the selection epilogue kr_actor_select
template <bool SEL>
int dispatch(const Fwd& a, const SelectArgs& sel, void* stream) {
    const int nt1 = (a.h1 + 15) / 16, nt2 = (a.h2 + 15) / 16;
    const bool vec = (a.h1 % 4 == 0) && (a.h2 % 4 == 0) && aligned16(a.W2) && aligned16(a.W3);
    decltype(&k_mlp3<4, 4, true, SEL>) k = nullptr;      // other widths: the caller keeps its GEMM path
    if (vec) { KR_MLP_PAIRS(KR_PICK, k_mlp3, true, SEL) } else { KR_MLP_PAIRS(KR_PICK, k_mlp3, false, SEL) }
    return launch_fwd(k, 64 * NW, stream, a, a.h1_out, a.h2_out, sel);
}

}  // namespace

extern "C" {

int kr_mlp3_forward(int32_t n, int32_t in_a, int32_t in_b, int32_t h1, int32_t h2, int32_t out_dim, const float* xa, int32_t lda,
                    const float* xb, int32_t ldb, const float* W1, const float* b1, const float* W2, const float* b2,
                    const float* W3, const float* b3, int32_t act, float scale, float* out, float* h1_out, float* h2_out, void* stream) {
    if (n <= 0) return KS_OK;
    const Fwd a{n, in_a, in_b, h1, h2, out_dim, xa, lda, xb, ldb, W1, b1, W2, b2, W3, b3, act, scale, out, h1_out, h2_out};
    if (!fwd_args_ok(a)) return KS_ERR_INVALID;
    return dispatch<false>(a, SelectArgs{}, stream);
}

int kr_mlp3_forward_shadow(int32_t n, int32_t in_a, int32_t in_b, int32_t h1, int32_t h2, int32_t out_dim, const float* xa, int32_t lda,
                           const float* xb, int32_t ldb, const float* W1, const float* b1, const float* W2, const float* b2,
                           const float* W3, const float* b3, int32_t act, float scale, float* out, float* h1_out, float* h2_out, void* stream) {
    if (n <= 0) return KS_OK;
    const Fwd a{n, in_a, in_b, h1, h2, out_dim, xa, lda, xb, ldb, W1, b1, W2, b2, W3, b3, act, scale, out, h1_out, h2_out};
    if (!fwd_args_ok(a) || !whole_tiles(h1, h2) || !aligned16(W2) || !aligned16(W3)) return KS_ERR_INVALID;
    const int nt1 = h1 / 16, nt2 = h2 / 16;
    decltype(&k_mlp3_wave<4, 4>) k = nullptr;
    KR_SHADOW_PAIRS(KR_PICK, k_mlp3_wave)
    return launch_fwd(k, 64, stream, a, h1_out, h2_out);
}

int kr_mlp3_forward_split(int32_t n, int32_t in_a, int32_t in_b, int32_t h1, int32_t h2, int32_t out_dim, const float* xa, int32_t lda,
                          const float* xb, int32_t ldb, const float* W1, const float* b1, const float* W2, const float* b2,
                          const float* W3, const float* b3, int32_t act, float scale, float* out, float* h1_out, float* h2_out,
                          float* scratch, int64_t scratch_floats, int32_t waves, void* stream) {
    if (n <= 0) return KS_OK;
    const Fwd a{n, in_a, in_b, h1, h2, out_dim, xa, lda, xb, ldb, W1, b1, W2, b2, W3, b3, act, scale, out, h1_out, h2_out};
    if (!fwd_args_ok(a) || !whole_tiles(h1, h2) || !aligned16(W2) || !aligned16(W3) || (waves != 2 && waves != 4)) return KS_ERR_INVALID;
    Exchange x;      // the layer-1 exchange and the layer-3 partial sums
    if (!exchange(x, n, h1, h1_out, waves, scratch, scratch_floats)) return KS_ERR_INVALID;
    const int nt1 = h1 / 16, nt2 = h2 / 16;
    decltype(&k_mlp3_split<4, 4, 2>) k = nullptr;
    if (waves == 4) { KR_SHADOW_PAIRS(KR_PICK, k_mlp3_split, 4) } else { KR_SHADOW_PAIRS(KR_PICK, k_mlp3_split, 2) }
    return launch_fwd(k, 64 * waves, stream, a, x.buf, x.rows, h2_out, x.partial);
}

int kr_mlp3_backward_shadow(int32_t n, int32_t in_dim, int32_t h1, int32_t h2, int32_t out_dim, const float* dz3, const float* W3,
                            const float* h2a, const float* W2, const float* h1a, float* dz2_out, float* dz1_out, const float* W1, int32_t col0,
                            int32_t ncol, const float* act_out, float scale, float* dx_out, void* stream) {
    if (n <= 0) return KS_OK;
    const Bwd a{n, in_dim, h1, h2, out_dim, dz3, W3, h2a, W2, h1a, dz2_out, dz1_out, W1, col0, ncol, act_out, scale, dx_out};
    if (!bwd_args_ok(a) || !whole_tiles(h1, h2)) return KS_ERR_INVALID;
    const int nt1 = h1 / 16, nt2 = h2 / 16;
    decltype(&k_mlp3_bwd_wave<4, 4>) k = nullptr;
    KR_SHADOW_PAIRS(KR_PICK, k_mlp3_bwd_wave)
    return launch_bwd(k, 64, stream, a, dz2_out);
}

int kr_mlp3_backward_split(int32_t n, int32_t in_dim, int32_t h1, int32_t h2, int32_t out_dim, const float* dz3, const float* W3,
                            const float* h2a, const float* W2, const float* h1a, float* dz2_out, float* dz1_out, const float* W1, int32_t col0,
                            int32_t ncol, const float* act_out, float scale, float* dx_out, float* scratch, int64_t scratch_floats, int32_t waves, void* stream) {
    if (n <= 0) return KS_OK;
    const Bwd a{n, in_dim, h1, h2, out_dim, dz3, W3, h2a, W2, h1a, dz2_out, dz1_out, W1, col0, ncol, act_out, scale, dx_out};
    if (!bwd_args_ok(a) || !whole_tiles(h1, h2) || (waves != 2 && waves != 4)) return KS_ERR_INVALID;
    Exchange x;      // only the partial sums of dx
    if (!exchange(x, n, 0, nullptr, dx_out ? waves : 0, scratch, scratch_floats)) return KS_ERR_INVALID;
    const int nt1 = h1 / 16, nt2 = h2 / 16;
    decltype(&k_mlp3_bwd_split<4, 4, 2>) k = nullptr;
    if (waves == 4) { KR_SHADOW_PAIRS(KR_PICK, k_mlp3_bwd_split, 4) } else { KR_SHADOW_PAIRS(KR_PICK, k_mlp3_bwd_split, 2) }
    return launch_bwd(k, 64 * waves, stream, a, dz2_out, x.partial);
}

int kr_mlp3_forward_lean(int32_t n, int32_t in_a, int32_t in_b, int32_t h1, int32_t h2, int32_t out_dim, const float* xa, int32_t lda,
                         const float* xb, int32_t ldb, const float* W1, const float* b1, const float* W2, const float* b2,
                         const float* W3, const float* b3, int32_t act, float scale, float* out, float* h1_out, float* h2_out,
                         float* scratch, int64_t scratch_floats, void* stream) {
    if (n <= 0) return KS_OK;
    const Fwd a{n, in_a, in_b, h1, h2, out_dim, xa, lda, xb, ldb, W1, b1, W2, b2, W3, b3, act, scale, out, h1_out, h2_out};
    if (!fwd_args_ok(a) || !lean_widths_ok(h1, h2) || !aligned16(W2) || !aligned16(W3)) return KS_ERR_INVALID;
    if (lda < in_a || (in_b > 0 && ldb < in_b)) return KS_ERR_INVALID;
    Exchange x;      // layer 1's output quads
    if (!exchange(x, n, h1, h1_out, 0, scratch, scratch_floats)) return KS_ERR_INVALID;
    if (!lean_fits32((n + ROWS - 1) / ROWS * ROWS, h1 > h2 ? h1 : h2) || !lean_fits32(n, lda) || !lean_fits32(n, in_b > 0 ? ldb : 1)) return KS_ERR_INVALID;
    const int nt1 = (h1 + 15) / 16, nt2 = (h2 + 15) / 16;
    decltype(&k_mlp3_lean<25, 19>) k = nullptr;
    KR_LEAN_PAIRS(KR_PICK, k_mlp3_lean)
    return launch_fwd(k, 64, stream, a, x.buf, x.rows, h2_out);
}

int kr_mlp3_backward_lean(int32_t n, int32_t in_dim, int32_t h1, int32_t h2, int32_t out_dim, const float* dz3, const float* W3,
                          const float* h2a, const float* W2, const float* h1a, float* dz2_out, float* dz1_out, const float* W1, int32_t col0,
                          int32_t ncol, const float* act_out, float scale, float* dx_out, float* scratch, int64_t scratch_floats, void* stream) {
    if (n <= 0) return KS_OK;
    const Bwd a{n, in_dim, h1, h2, out_dim, dz3, W3, h2a, W2, h1a, dz2_out, dz1_out, W1, col0, ncol, act_out, scale, dx_out};
    if (!bwd_args_ok(a) || !lean_widths_ok(h1, h2)) return KS_ERR_INVALID;
    Exchange x;      // the masked dz2 quads
    if (!exchange(x, n, h2, dz2_out, 0, scratch, scratch_floats)) return KS_ERR_INVALID;
    if (!lean_fits32((n + ROWS - 1) / ROWS * ROWS, h1 > h2 ? h1 : h2) || (dx_out && !lean_fits32(h1, in_dim))) return KS_ERR_INVALID;
    const int nt1 = (h1 + 15) / 16, nt2 = (h2 + 15) / 16;
    decltype(&k_mlp3_bwd_lean<25, 19>) k = nullptr;
    KR_LEAN_PAIRS(KR_PICK, k_mlp3_bwd_lean)
    return launch_bwd(k, 64, stream, a, x.buf, x.rows);
}

// the two launches behind kr_weight_grad_shadow (idx == nullptr: the n terms are the rows themselves) and kr_weight_grad_indexed
static int weight_grad(int32_t n, int32_t rows, int32_t M, int32_t Na, int32_t Nb, const float* dz, const float* ha, int32_t lda, const float* hb,
                       int32_t ldb, const int32_t* idx, int32_t chunks, float* workspace, float* dW, float* db, void* stream) {
    if (n <= 0 || M < 1 || Na < 1 || Nb < 0 || chunks < 1 || !dz || !ha || (Nb > 0 && !hb) || !workspace || !dW || !db) return KS_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int N = Na + Nb, n_blocks = (N + 16 * WG_TN - 1) / (16 * WG_TN), m_tiles = (M + 15) / 16;
    int rows_per_chunk = (n + chunks - 1) / chunks;
    rows_per_chunk = (rows_per_chunk + 15) / 16 * 16;
    // the rounding can leave trailing chunks that start at or past n: launch (and reduce) only the chunks that hold rows.  A chunk
    // with r0 > n would otherwise take full_end = r0 - 16 in k_wgrad_wave and add rows the previous chunk already counted.
    chunks = (n + rows_per_chunk - 1) / rows_per_chunk;
    const dim3 grid(m_tiles * n_blocks, chunks);
    if (idx != nullptr)
        hipLaunchKernelGGL(k_wgrad_wave<true>, grid, dim3(64), 0, s, n, rows, M, Na, Nb, rows_per_chunk, dz, ha, lda, hb, ldb, idx, workspace);
    else
        hipLaunchKernelGGL(k_wgrad_wave<false>, grid, dim3(64), 0, s, n, n, M, Na, Nb, rows_per_chunk, dz, ha, lda, hb, ldb, idx, workspace);
    const long total = (long)M * N + M;
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (long)M * N, (long)M, chunks, workspace, dW, db);
    return hipGetLastError() == hipSuccess ? KS_OK : KS_ERR_HIP;
}

int kr_weight_grad_shadow(int32_t n, int32_t M, int32_t Na, int32_t Nb, const float* dz, const float* ha, int32_t lda, const float* hb, int32_t ldb,
                          int32_t chunks, float* workspace, float* dW, float* db, void* stream) {
    return weight_grad(n, n, M, Na, Nb, dz, ha, lda, hb, ldb, nullptr, chunks, workspace, dW, db, stream);
}

int kr_weight_grad_indexed(int32_t n, int32_t rows, int32_t M, int32_t Na, int32_t Nb, const float* dz, const float* ha, int32_t lda, const float* hb,
                           int32_t ldb, const int32_t* idx, int32_t chunks, float* workspace, float* dW, float* db, void* stream) {
    // (the lane offsets row * ld * 4 are 32-bit)
    if (!idx || rows < 1 || M < 1 || lda < Na || (Nb > 0 && ldb < Nb) || (int64_t)rows * (M > lda ? (M > ldb ? M : ldb) : (lda > ldb ? lda : ldb)) * 4 >= (int64_t)OOR)
        return KS_ERR_INVALID;
    return weight_grad(n, rows, M, Na, Nb, dz, ha, lda, hb, ldb, idx, chunks, workspace, dW, db, stream);
}

int kr_actor_select(int32_t n, int32_t h1, int32_t h2, const float* obs, const float* prev_obs, const uint8_t* has_prev, const int64_t* t,
                    uint8_t* ready, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                    const float* noise, uint64_t seed, int64_t* rng_state, float sigma, float max_action, int32_t skip_steps, float* actor_out,
                    float* action, float* action_t, uint8_t* lifting, void* stream) {
    if (n <= 0) return KS_OK;
    if (!obs || !prev_obs || !has_prev || !t || !ready || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !action || !action_t || !lifting) return KS_ERR_INVALID;
    if ((noise == nullptr) == (rng_state == nullptr) || h1 < 1 || h2 < 1) return KS_ERR_INVALID;     // exactly one noise source
    SelectArgs sel{obs, prev_obs, has_prev, t, ready, noise, (unsigned long long)seed, rng_state, sigma, max_action, skip_steps, action, action_t, lifting};
    const Fwd a{n, KR_STATE_DIM, 0, h1, h2, KR_ACTION_DIM, obs, KR_STATE_DIM, nullptr, 0, W1, b1, W2, b2, W3, b3, KR_ACT_SIGMOID, max_action, actor_out, nullptr, nullptr};
    return dispatch<true>(a, sel, stream);
}

}  // extern "C"
