// ks_controller.h -- the scripted demonstrators as a per-env rule beside krsel::select_one (ks_select.h): the reference's naive,
// position-dependent and combined controllers (expert_data.py:318-671) with the two lift rules its loops use (expert_data.py:746-804,
// main_DDPGfD.py:418-439).  One env per call, fp32, no fma contraction, every operation in the order of the torch expressions in
// kinovagrasping_amd/demonstrators.py (controller_action, run_controller_episodes): bit-identical to them on fp32 tensors.
// (A divisor that is a Python scalar is divided by here, as the expressions are written and as torch divides on the CPU; torch's GPU
// kernel multiplies by the reciprocal instead, which can differ in the last bit.  It shows in one place only, pid_vel above the
// 0.5 floor of check_vel_in_range, i.e. obs[81] < -0.95.)
// Host/device: the same source compiles with a C++ compiler for tests/native/ks_controller_host.cpp.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KRC_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define KRC_HD inline
#endif
#include <stdint.h>

namespace krsel {

// VELOCITIES of demonstrators.py (expert_data.py:617)
constexpr float C_CONSTANT_VELOCITY = 0.5f, C_MIN_VELOCITY = 0.5f, C_MAX_VELOCITY = 0.8f, C_FINGER_LIFT_VELOCITY = 0.5f, C_WRIST_LIFT_VELOCITY = 0.6f;
constexpr int C_OBS = 82, C_ACT = 4;
constexpr int C_MODE_NAIVE = 1, C_MODE_POSITION_DEPENDENT = 2, C_MODE_COMBINED = 3;      // KS_CONTROLLER_* of include/kinova_sim.h
constexpr int C_LIFT_TRAIN = 0, C_LIFT_EXPERT = 1;                                      // KS_LIFT_RULE_*
constexpr int C_MIN_LIFT_TIMESTEPS = 10;                                                // expert_data.py:762

KRC_HD bool controller_args_ok(int mode, int lift_rule) {
    return mode >= C_MODE_NAIVE && mode <= C_MODE_COMBINED && (lift_rule == C_LIFT_TRAIN || lift_rule == C_LIFT_EXPERT);
}

// torch.clamp(x, lo, hi): a NaN passes through
KRC_HD float controller_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// pd_controller_action: o = the env's observation row, (init_x, init_dot) = (obs[21], obs[81]) at the start of the episode -> a[4]
KRC_HD void pd_controller_action(const float* o, float init_x, float init_dot, bool lift, float* a) {
#pragma clang fp contract(off)
    const float dot = o[81], d78 = o[78], d79 = o[79];
    const float k = (float)(1.0 + 1.0 / 15.0);                      // kp + kd / sampling_time
    float pid_vel = (1.0f - dot) * k / 1.25f * 0.3f;
    pid_vel = pid_vel < 0.05f ? 0.05f : pid_vel;                    // clamp(min=0.05)
    const float touch1 = (dot - d78) * k, touch2 = (dot - d79) * k;
    const float full = C_CONSTANT_VELOCITY, lift_f = C_FINGER_LIFT_VELOCITY;
    const float moved_by = fabsf(dot - init_dot);
    const bool moved = moved_by > 0.01f, pre = moved_by < 0.01f, far = fabsf(1.0f - dot) > 0.01f;
    float f1, f23;
    if (fabsf(init_x) <= 0.03f) {                                   // centre
        f1 = lift ? lift_f / 2 : full;
        f23 = lift ? lift_f : (moved ? full / 2 : full);
    } else if (init_x > 0.0f) {                                     // right: fingers 2, 3 push first
        f1 = pre ? 0.0f : (lift ? lift_f / 2 : (far ? C_MIN_VELOCITY : touch1));
        f23 = pre ? touch2 : (lift ? lift_f : (far ? pid_vel : 0.0f));
    } else {                                                        // left: finger 1 pushes first
        f1 = pre ? touch1 : (lift ? lift_f / 2 : (far ? pid_vel : 0.0f));
        f23 = pre ? 0.0f : (lift ? lift_f : (far ? C_MIN_VELOCITY : touch2));
    }
    a[0] = lift ? C_WRIST_LIFT_VELOCITY : 0.0f;
    a[1] = controller_clamp(f1, C_MIN_VELOCITY, C_MAX_VELOCITY);    // check_vel_in_range (expert_data.py:540-551)
    a[2] = a[3] = controller_clamp(f23, C_MIN_VELOCITY, C_MAX_VELOCITY);
}

// controller_action of demonstrators.py (expert_data.get_action): no noise, no max_action clip
KRC_HD void controller_action(int mode, const float* o, float init_x, float init_dot, bool lift, float* a) {
    if (mode == C_MODE_NAIVE) {
        a[0] = lift ? C_WRIST_LIFT_VELOCITY : 0.0f;
        a[1] = a[2] = a[3] = lift ? C_FINGER_LIFT_VELOCITY : C_CONSTANT_VELOCITY;
        return;
    }
    pd_controller_action(o, init_x, init_dot, lift, a);
    if (mode == C_MODE_POSITION_DEPENDENT) return;
    // combined: chosen on the CURRENT palm-frame x
    const float x = o[21];
    const bool outer = x < -0.04f || x > 0.04f;
    const bool band = (x >= -0.04f && x <= -0.02f) || (x >= 0.02f && x <= 0.04f);
    if (outer) return;
    if (band) { a[1] = a[3] = a[2]; return; }                       // np.interp right of its sample points: the PD controller's finger 2
    a[1] = a[2] = a[3] = lift ? C_FINGER_LIFT_VELOCITY : C_CONSTANT_VELOCITY;
}

// check_grasp on obs[9:17] (expert_data.py:559-593), as select_one has it
KRC_HD bool controller_check_grasp(const float* o, const float* p) {
#pragma clang fp contract(off)
    float d = fabsf(p[9] - o[9]) / 15.0f;
    d += fabsf(p[12] - o[12]) / 15.0f;
    d += fabsf(p[15] - o[15]) / 15.0f;
    return d < 0.0002f;
}

// the lift rule: latches `ready`, returns the lift flag of this step
KRC_HD bool controller_lift(int lift_rule, bool chk, bool has_prev, int64_t t, int skip_steps, bool& ready) {
    if (lift_rule == C_LIFT_EXPERT) {                               // expert_data.py:746-804
        ready = ready || (chk && has_prev && t >= 2);
        return ready && t > C_MIN_LIFT_TIMESTEPS;
    }
    ready = ready || (chk && has_prev && t + 1 >= skip_steps);      // main_DDPGfD.py:418-439
    return ready;
}

// env i: latches init[2][n] = (obs[21], obs[81]) at t == 0 and `ready`; writes action / action_t / lifting
KRC_HD void controller_one(int i, int n, int mode, int lift_rule, const float* obs, const float* prev_obs, const uint8_t* has_prev, const int64_t* t,
                           uint8_t* ready, float* init, int skip_steps, float* action, float* action_t, uint8_t* lifting) {
    const float* o = obs + (long)i * C_OBS;
    const float* p = prev_obs + (long)i * C_OBS;
    const int64_t ti = t[i];
    if (ti == 0) { init[i] = o[21]; init[(long)n + i] = o[81]; }
    const float init_x = init[i], init_dot = init[(long)n + i];
    bool rdy = ready[i] != 0;
    const bool lift = controller_lift(lift_rule, controller_check_grasp(o, p), has_prev[i] != 0, ti, skip_steps, rdy);
    ready[i] = rdy;
    lifting[i] = lift;
    float a[C_ACT];
    controller_action(mode, o, init_x, init_dot, lift, a);
    for (int k = 0; k < C_ACT; k++) {
        action[(long)i * C_ACT + k] = a[k];
        action_t[(long)k * n + i] = a[k];
    }
}

}  // namespace krsel
