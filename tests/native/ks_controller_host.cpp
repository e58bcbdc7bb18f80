// Host build of csrc/ks_controller.h (the scripted demonstrators' per-env rule) for tests/test_controller_cpu.py:
//   g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared
// The header is the code the kernels compile (k_controller_select, rollout_controller); here its functions run one env after another.
#include "../../kinovagrasping_amd/csrc/ks_controller.h"

extern "C" {

// controller_action for n cases: obs [n, 82], init_x / init_dot [n], lift uint8 [n] -> action [n, 4]
void kc_action(int n, int mode, const float* obs, const float* init_x, const float* init_dot, const uint8_t* lift, float* action) {
    for (int i = 0; i < n; i++) krsel::controller_action(mode, obs + (long)i * krsel::C_OBS, init_x[i], init_dot[i], lift[i] != 0, action + (long)i * krsel::C_ACT);
}

// the lift rule for one env: returns lifting, *ready is latched
int kc_lift(int lift_rule, int chk, int has_prev, long long t, int skip_steps, uint8_t* ready) {
    bool r = *ready != 0;
    const bool lifting = krsel::controller_lift(lift_rule, chk != 0, has_prev != 0, (int64_t)t, skip_steps, r);
    *ready = r;
    return lifting;
}

int kc_check_grasp(const float* obs_row, const float* prev_row) { return krsel::controller_check_grasp(obs_row, prev_row); }

int kc_args_ok(int mode, int lift_rule) { return krsel::controller_args_ok(mode, lift_rule); }

// controller_one for every env of a batch, as k_controller_select runs it
void kc_select(int n, int mode, int lift_rule, const float* obs, const float* prev_obs, const uint8_t* has_prev, const int64_t* t, uint8_t* ready,
               float* init, int skip_steps, float* action, float* action_t, uint8_t* lifting) {
    for (int i = 0; i < n; i++) krsel::controller_one(i, n, mode, lift_rule, obs, prev_obs, has_prev, t, ready, init, skip_steps, action, action_t, lifting);
}

}  // extern "C"
