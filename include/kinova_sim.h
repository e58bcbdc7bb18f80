/* include/kinova_sim.h -- C ABI of libkinova_sim.so, the MI355X-native batched replacement for the
 * mujoco-py engine object that KinovaGripper_Env drives one env at a time.
 *
 * Reference interface each entry point replaces (reference root = /root/reference/, file
 * gym-kinova-gripper/gym_kinova_gripper/envs/kinova_gripper_env.py, "ENV"):
 *
 *   ks_create / ks_destroy   <- MjSim(model) construction / garbage collection      ENV:102, 879, 1003
 *   ks_load_model            <- mujoco_py.load_model_from_path(xml)                 ENV:62, 878, 1002
 *                               (the MJCF+STL compile happens offline: model_compiler.py -> .ksm)
 *   ks_load_models /
 *   ks_reset_objects         <- the per-episode object choice: select_object + load of another XML   ENV:986-1005, 1180-1222
 *   ks_reset                 <- KinovaGripper_Env.reset: write_xml (hand euler) + _set_state
 *                               + sim.forward() + _get_obs()                        ENV:1310-1410, 851-881, 692-703
 *   ks_set_start_pool        <- the NEW start every reset() draws (orientation class, coordinate-table row, hand euler), for the
 *                               resets that happen inside ks_step / ks_rollout                       ENV:1310-1410
 *   ks_set_episode_log /
 *   ks_get_episode_log       <- the per-episode outcome eval_policy collects: success / fail start coordinates per orientation,
 *                               main_DDPGfD.py:130-272, 310-330 - for the episodes that end inside ks_step / ks_rollout
 *   ks_set_rollout_controller<- the scripted demonstrators that act instead of the actor: expert_data.py:318-671 (get_action) with the
 *                               lift rule of expert_data.py:746-804 or main_DDPGfD.py:418-439 - inside ks_rollout
 *   ks_step                  <- KinovaGripper_Env.step: action->ctrl, 15 x sim.step(),
 *                               _get_obs(), _get_reward()                           ENV:1495-1552
 *                               + gym TimeLimit (max_episode_steps)                 gym_kinova_gripper/__init__.py:3-7, main_DDPGfD.py:384
 *   ks_set_env_params        <- (none: the reference edits geom mass / pair friction in the XML; config-5 extension)
 *   ks_set_param_ranges /
 *   ks_get_env_params        <- (none: config-5 extension, per episode)
 *   ks_obs_from_snapshot     <- _get_obs() + _get_reward() on a given engine state          ENV:438-534, 631-687
 *   ks_get_state/ks_set_state<- sim.data.qpos / qvel / qacc_warmstart, sim.data.ncon,
 *                               contact forces (parity taps)                        ENV:109, 347-353
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless the name ends in _host.  The caller (PyTorch) owns
 *     every buffer; the library owns only its context and scratch.  Pointers are borrowed for the
 *     duration of the stream operation.
 *   - Real-valued buffers have the context precision: float for precision 32 (the product), double
 *     for precision 64 (the exact mode: parity checks, and rollout / training through ks_rollout).
 *   - Batched arrays are struct-of-arrays, field-major: x[k * n_envs + env].  The observation may be
 *     requested env-major (obs[env * 82 + k]) with obs_env_major = 1.
 *   - Every call is asynchronous on `stream` (a hipStream_t passed as void*); no hidden host syncs.
 *   - One context per GPU per process; a context is not thread safe.
 *   - Return value: 0 on success, negative ks_status otherwise; ks_last_error gives a message.
 *   - There is NO CPU path: ks_create fails when no HIP device is available.
 *   - Two builds of this ABI exist.  libkinova_sim.so: the reference's fixed topology (ground, 7 hand geoms, ONE object geom) - every
 *     single-geom object, the fast path.  libkinova_sim_mg.so: the same sources with the capacities of the multi-geom objects (the
 *     Bottle / TBottle / Bowl / RBowl models, `object` + welded child bodies: kinova_description/j2s7s300_end_effector_v1_sbottle.xml
 *     :158-186, shape keys ENV:189-208); it also loads single-geom models (a curriculum stage mixes both), more slowly.  A caller binds
 *     the library its models need: ks_load_model of libkinova_sim.so refuses a multi-geom blob with a message that says so.
 */
#ifndef KINOVA_SIM_H
#define KINOVA_SIM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KS_NQ 16
#define KS_NV 15
#define KS_NACT 4
#define KS_NOBS 82
#define KS_NINFO 3
#define KS_NCON_MAX 24      /* libkinova_sim.so; the multi-geom build (libkinova_sim_mg.so) keeps KS_NCON_MAX_MG */
#define KS_NCON_MAX_MG 40
#define KS_CONTACT_STRIDE 20

typedef enum {
    KS_OK = 0,
    KS_ERR_INVALID = -1,  /* bad argument */
    KS_ERR_NO_DEVICE = -2,
    KS_ERR_HIP = -3,      /* a HIP runtime call failed */
    KS_ERR_MODEL = -4,    /* malformed or unsupported model blob */
    KS_ERR_STATE = -5     /* call sequence error (e.g. step before load_model) */
} ks_status;

typedef struct {
    int32_t n_envs;
    int32_t frame_skip;         /* 15 (ENV:51) */
    int32_t horizon;            /* episode time limit in env steps, 30 (main_DDPGfD.py:384); <= 0 disables */
    int32_t solver_iterations;  /* Newton iterations per substep */
    int32_t precision;          /* 32 or 64 */
    int32_t auto_reset;         /* 1: envs that finish are reset inside ks_step: to their stored initial state, or - with a start
                                   pool, ks_set_start_pool - to a start drawn from the env's pool */
    int32_t obs_env_major;      /* 0: obs[k*N+env], 1: obs[env*82+k] */
    int32_t envs_per_wave;      /* envs per stepping workgroup (256 threads = 16 lanes per env): 0 = automatic (16,
                                   or fewer when the model's hull tables leave less LDS); else 1..16 */
    int32_t contact_tap;        /* 1: keep the per-contact records of the last substep for ks_get_state (parity) */
    int32_t pair_memory;        /* 1 (default): every env carries what its hull pairs remember of their last narrow-phase
                                   queries (support hints and the closest-feature simplex: vertex ids only) from one
                                   ks_step to the next, so no substep starts its queries cold; 0: cold start at every
                                   ks_step.  Same contacts to the queries' 1e-6 tolerance either way. */
    int32_t reserved[2];
} ks_config;

typedef struct ks_ctx ks_ctx;

void ks_default_config(ks_config *cfg);
int ks_create(const ks_config *cfg, int device, ks_ctx **out);
void ks_destroy(ks_ctx *ctx);
const char *ks_last_error(const ks_ctx *ctx);   /* ctx may be NULL: last creation error */

/* blob_host: KSMB model blob in HOST memory (copied; may be freed after the call).  A context loads its model(s) once. */
int ks_load_model(ks_ctx *ctx, const void *blob_host, size_t nbytes);

/* Mixed-object batches (BASELINE config 5; the reference swaps the object by loading another MJCF per episode,
 * ENV:986-1005): n_models (<= 32) blobs of the SAME hand with different objects; object k of ks_reset_objects is
 * blobs_host[k].  One context, one stepping launch: envs are grouped by object inside the library (every stepping
 * workgroup stages one object's hull tables), the hand's meshes are kept once. */
int ks_load_models(ks_ctx *ctx, int32_t n_models, const void *const *blobs_host, const size_t *nbytes);

/* Reset `n` envs.  env_ids: device int32[n] or NULL for envs 0..n-1 (then n must be n_envs).
 * qpos0: [16, n] start configuration (3 slides, 6 finger joints, object xyz + quat wxyz),
 * hand_quat: [4, n] orientation of j2s7s300_link_7 (the euler the reference patches into the XML).
 * Both are stored as the env's initial state for auto-reset.  obs (optional): observation buffer of
 * the WHOLE batch (layout per cfg); only the rows of the reset envs are written. */
int ks_reset(ks_ctx *ctx, const int32_t *env_ids, int32_t n, const void *qpos0, const void *hand_quat, void *obs, void *stream);

/* ks_reset that also chooses every reset env's object and (optionally) its randomised parameters - the reference's
 * reset(): select_object (ENV:986-1005) + select_orienation (ENV:1180-1222) + _set_state (ENV:692-703).
 * env_ids must not name an env twice in one call (each entry is stored by its own thread: which of two would win is not defined).
 * object_id: device int32 [n], index into the blobs of ks_load_models, or NULL (objects stay);
 * A call with object_id CLEARS the context's start pool (ks_set_start_pool): a pool entry is a start of the object the env held.
 * An env whose object CHANGES also forgets what its lanes remember of its hull pairs' last queries (the pair memory of fp32 contexts names vertices of
 * the object it held) and continues like an env of a new context of its new object.
 * mass_friction: device [2, n] (row 0 object mass in kg - the inertia scales with it -, row 1 friction of the seven
 * object-hand pairs), or NULL: an env whose object is (re)assigned takes that object's compiled mass / friction, other
 * envs keep theirs.  (Mass / friction randomisation is an extension: the reference fixes 0.1 kg, XML:153, and mu 1,
 * XML:160-166.)  With object_id in a context of several models the call regroups the stepping kernels' work list and - round 6, unless the
 * stream is being captured - WAITS for the stream once to read back how many 16-env groups hold envs (what ks_rollout schedules: ks_rollout_plan). */
int ks_reset_objects(ks_ctx *ctx, const int32_t *env_ids, int32_t n, const void *qpos0, const void *hand_quat, const int32_t *object_id,
                     const void *mass_friction, void *obs, void *stream);

/* Start pool: k prepared starts per env, one of which every AUTO-RESET of the env draws inside the stepping kernels (ks_step and
 * ks_rollout, both precisions, both libraries) - instead of replaying the one stored initial state for as long as the context lives.
 * qpos0: [k][16][N], hand_quat: [k][4][N] (entry j of env e: qpos0[(j * 16 + i) * N + e]), as ks_reset takes them.
 * The call behaves like a ks_reset of ALL envs:
 *   - it copies the pool (context precision) into storage the context owns - (16 + 4 + 82) * k * N values, 107 MB for k = 64,
 *     N = 4096 in fp32; grown on demand, kept until ks_destroy; when it cannot be allocated: KS_ERR_HIP, the message states the size;
 *   - it computes the observation of every one of the k * N starts once, with ks_reset's own kernels and therefore its bits: the
 *     reset pass (state <- start, kinematics, rays, observation) is looped over the k entries, all envs per pass, reading the entry
 *     in the pool and writing into the pool and into preparation buffers of the context's - no env's live state is touched;
 *   - it zeroes every env's episode counter, resets every env to its draw for episode 0 and writes `obs` (optional, as ks_reset).
 * The draw, for callers that want to reproduce it:
 *     r = Philox4x32-10(counter = (env, episode low word, episode high word, 0x5350), key = (seed low word, seed high word))
 *     index = (uint64(r[0]) * k) >> 32
 * where `episode` counts the auto-resets the env has done since the pool was set (episode 0: the call's own reset).  On an auto-reset
 * the kernel bumps the counter, draws, copies the entry (start, hand orientation, cached observation) over the env's stored
 * initial state and restarts the env from it exactly as without a pool: a copy and forward kinematics, no rays.
 * ks_reset of some envs keeps the pool: those envs run the caller's start until their next auto-reset draws again.
 * ks_reset_objects with object_id clears the pool.  (An object per episode is not part of this: it regroups the work list.)
 * k = 0 clears the pool (qpos0 / hand_quat / obs ignored, no reset): every env keeps the start of its running episode as its stored
 * initial state, as if ks_reset had set it.  1 <= k <= 1024 otherwise.
 * No host synchronisation, like ks_reset - except that a call which has to allocate (the first, or a larger k) allocates, and
 * waits for the device before it gives a smaller storage back.  Not for stream capture. */
int ks_set_start_pool(ks_ctx *ctx, int32_t k, const void *qpos0, const void *hand_quat, uint64_t seed, void *obs, void *stream);
/* index: int32 [N], the pool entry every env's running episode started from (an env that was ks_reset since: its last draw);
 * episode: int64 [N], its auto-resets since the pool was set.  Either may be NULL.  KS_ERR_STATE without a pool. */
int ks_get_start_index(ks_ctx *ctx, int32_t *index, int64_t *episode, void *stream);

/* Episode log: one fixed-size record per episode that ENDS and restarts inside the stepping kernels (ks_step and ks_rollout, both
 * precisions, both libraries) - which env, object and start it was and how it ended; what the four totals of ks_rollout_args.counters
 * cannot say.  The record is written where the auto-reset happens, just before the next start is drawn (ks_set_start_pool), into a
 * ring in device memory that the context owns.  32 bytes, 8 little-endian 32-bit words:
 *   word 0     env          int32  env id
 *   word 1     object       int32  the env's object (index into the blobs of ks_load_models; 0 in a one-model context)
 *   word 2     start_index  int32  pool entry the finished episode started from (what ks_get_start_index gave while it ran); -1 without a pool
 *   word 3     steps        int32  env-steps of the episode
 *   word 4     done         int32  done bits of its last step (1 lifted, 2 time limit)
 *   word 5, 6  start_x, _y  float  obs[21], obs[22] of the episode's first observation: the object's start position in the palm frame
 *                                  (what eval_policy keeps per episode, main_DDPGfD.py:130-272).  fp64 contexts: rounded to float once.
 *   word 7     episode      int32  ordinal of this episode among the env's logged episodes since the log was set: 0, 1, ...
 * Every record takes a ticket (a device int64 counter, `written`: records since the log was set, never wraps) and goes to slot
 * ticket % capacity: the ring overwrites its oldest records, and a reader that knows `written` knows which tickets the slots hold.
 * Tickets are taken in the order the hardware runs the envs: within one ks_step the order of the envs is not defined, the records of
 * ONE env are always in ticket order.
 * ks_set_episode_log: n_envs <= capacity <= KS_EPISODE_LOG_CAPACITY_MAX records (2^24: 512 MB), KS_ERR_INVALID otherwise.  At least one
 * record per env, so that the records of one LOCK-STEP launch (ks_step: at most one per env) never share a slot.  That guarantee is
 * ks_step's only: a ks_rollout launch in which the envs finish more than `capacity` episodes wraps the ring while it runs, and a writer
 * that is held up between taking its ticket and storing its record may then store over, or into, the record of the ticket `capacity`
 * later.  A ring that wraps inside one free-running launch is best effort; size it for the launch (steps / shortest episode records per
 * env) where every record counts.  Allocates the ring - grown on demand, kept until ks_destroy; when it
 * cannot be allocated: KS_ERR_HIP, the message states the size -, zeroes it, `written` and every env's ordinal.  capacity = 0 clears
 * the log.  KS_ERR_STATE on a context without auto_reset (nothing would ever be written) or before ks_load_model.  No host
 * synchronisation - except that a call which has to allocate allocates, and waits for the device before it gives a smaller ring back.
 * Not for stream capture; but the log's descriptor lives in device memory and is written by the stream, so a ks_step / ks_rollout
 * captured BEFORE the call logs when it is replayed after it.
 * The log is untouched by ks_reset and ks_reset_objects (an episode that a host reset cuts off is not logged: it did not end), by
 * ks_set_start_pool (set or cleared) and by budget_ticks launches.  A context that never sets a log computes what it always did.
 * ks_get_episode_log: device-to-device copies of the whole ring (ring_out: `capacity` records) and of `written` (written_out: device
 * int64 [1]), asynchronous on `stream`, no host synchronisation; either pointer may be NULL.  KS_ERR_STATE without a log.  Defined for
 * reads that are stream-ordered after the launches whose episodes they want; reading beside a running launch is not (a slot may be
 * half written, `written` may be ahead of the slots). */
#define KS_EPISODE_LOG_CAPACITY_MAX (1 << 24)
typedef struct {
    int32_t env, object, start_index, steps, done;
    float start_x, start_y;
    int32_t episode;
} ks_episode_record;
int ks_set_episode_log(ks_ctx *ctx, int32_t capacity, void *stream);
int ks_get_episode_log(ks_ctx *ctx, ks_episode_record *ring_out, int64_t *written_out, void *stream);

/* One env.step() for every env.  action: [4, N] (wrist, finger1..3), obs: N x 82, reward: [N],
 * done: uint8 [N] (bit0 lifted, bit1 time limit), info: [3, N] (finger, grasp, lift reward).
 * final_obs (optional): with auto_reset, rows of envs that finished hold their terminal
 * observation while `obs` already holds the observation after the reset.
 * Stream capture: ks_step / ks_rollout may be recorded into a HIP graph.  The library then records a host-to-device copy
 * of the call's output-pointer record from pinned memory it owns for the life of the context (one record per captured call,
 * never recycled), so any number of captured graphs with different output buffers can be replayed in any order; the
 * buffers themselves are borrowed for as long as the graph may be replayed.  Eager calls may be mixed with replays: once a context
 * holds a captured call, every eager ks_step re-sends its own output record (the "same pointers as the last call" shortcut is off). */
int ks_step(ks_ctx *ctx, const void *action, void *obs, void *reward, uint8_t *done, void *info, void *final_obs, void *stream);

/* Parity taps; any pointer may be NULL.  contact: [KS_NCON_MAX*KS_CONTACT_STRIDE, N] (libkinova_sim_mg.so: KS_NCON_MAX_MG) records of the
 * last substep (pos3 normal3 dist mu bodies+pair (b1 + 16 b2 + 256 pair index) R aref4 force3(normal,t1,t2) active-row-mask D spare; needs cfg.contact_tap), ncon: int32 [N],
 * status: int32 [N] sticky bit flags (1 contact overflow, 2 non-finite state, 4 the env's rays were not delivered in time by the
 * stepping launch's ray pool - a wait ran out; never seen in practice, reported instead of hanging; 8 a substep's Newton iteration
 * ended at cfg.solver_iterations before its stop rule fired: that substep used a truncated iterate). */
int ks_get_state(ks_ctx *ctx, void *qpos, void *qvel, void *qacc_warmstart, void *contact, int32_t *ncon, int32_t *status, void *stream);
int ks_set_state(ks_ctx *ctx, const void *qpos, const void *qvel, const void *qacc_warmstart, void *stream);

/* Per-env domain randomisation (BASELINE config 5; an extension: the reference fixes the object's mass at 0.1 kg,
 * XML:153, and the object-hand friction at 1, XML:160-166).  obj_mass [N] (kg; the inertia scales with it), obj_mu [N]
 * (friction of the seven object-hand pairs); either pointer may be NULL = leave as is.  Defaults are the model's. */
int ks_set_env_params(ks_ctx *ctx, const void *obj_mass, const void *obj_mu, void *stream);

/* Per-EPISODE domain randomisation: ranges from which every AUTO-RESET of an env draws its object's mass and its object-hand friction
 * inside the stepping kernels (ks_step and ks_rollout, both precisions, both libraries) - instead of keeping the one pair the host wrote
 * for as long as the context lives.
 * ranges: device [4][N], context precision: mass_lo, mass_hi, mu_lo, mu_hi per env (ranges[k * N + env]); copied into storage the context
 * owns.  NULL clears the ranges (seed ignored): every env keeps the values of its running episode.
 * The draw, for callers that want to reproduce any episode's parameters from (seed, env, episode) alone:
 *     r    = Philox4x32-10(counter = (env, episode low word, episode high word, 0x4d46), key = (seed low word, seed high word))
 *     mass = T( mass_lo + (mass_hi - mass_lo) * (r[0] * 2^-32) )        mu = T( mu_lo + (mu_hi - mu_lo) * (r[1] * 2^-32) )
 * evaluated in fp64 - the bounds converted exactly, difference, product and sum each rounded to nearest (never contracted into a fused
 * multiply-add) - and rounded ONCE to the context precision T: float64 arithmetic followed by one conversion (numpy: .astype)
 * reproduces it bit for bit in both precisions; kinovagrasping_amd.scenarios.param_draw_reference does.  lo == hi gives the constant;
 * every result lies in [lo, hi].  `episode` counts the env's auto-resets since the ranges were set (episode 0: the call's own draw) -
 * with an episode log set at the same boundary it is the `episode` ordinal of the log's records.
 * The call zeroes every env's counter, draws episode 0 and writes the pair of all N envs where the env-steps read them (what
 * ks_set_env_params writes).  It resets nothing: it is meant for an episode boundary, behind ks_reset or ks_set_start_pool.  On an
 * auto-reset the kernel bumps the env's counter, draws and stores the pair; the env-step that follows loads it.  With or without a
 * start pool, with or without an episode log.
 * ks_set_env_params after the call overrides the values of the running episodes until an env's next auto-reset draws again; ks_reset
 * keeps the ranges; ks_reset_objects with object_id CLEARS them (a range belonged to the object the env held), with mass_friction only
 * it behaves like ks_set_env_params.
 * The record the kernels read lives in device memory and is written by the stream, so a ks_step / ks_rollout captured BEFORE the call
 * draws when it is replayed after it.  Storage ([4][N] values, [N] int64 counters) is allocated by the first call that sets ranges and
 * kept until ks_destroy; no host synchronisation otherwise.  Not for stream capture itself.
 * KS_ERR_STATE on a context without auto_reset (nothing would ever be drawn) or before ks_load_model.  The library cannot see device
 * values without a synchronisation: the CALLER is responsible for mass_lo > 0 and lo <= hi in every env (the Python layer checks host
 * inputs).  A context that never sets ranges computes what it always did. */
int ks_set_param_ranges(ks_ctx *ctx, const void *ranges, uint64_t seed, void *stream);
/* mass, mu: [N], context precision - the object mass and object-hand friction every env's running episode uses (drawn, or written by
 * ks_set_env_params / ks_reset_objects, or the model's); episode: int64 [N], the env's draws since the ranges were set (0 in a context
 * that never set ranges).  Asynchronous copies on `stream`; any pointer may be NULL.  KS_ERR_STATE before ks_load_model. */
int ks_get_env_params(ks_ctx *ctx, void *mass, void *mu, int64_t *episode, void *stream);

/* Advance by ONE mj_step with explicit controls ctrl [9, N] (no observation); parity testing. */
int ks_substep(ks_ctx *ctx, const void *ctrl, void *stream);

/* Observation / reward / termination of caller-provided kinematic snapshots: snap [105, N] = world poses of bodies 2..9
 * (j2s7s300_link_7, finger 1 proximal, distal, finger 2 ..., object; 12 values each: rotation row-major 9, position 3)
 * followed by the 9 jointpos sensors (slides, proximal 1-3, distal 1-3); rays [17, N] = the rangefinder distances
 * (-1 = no hit).  Replaces _get_obs() + _get_reward() on a given mujoco-py state (ENV:438-534, 631-687) without any
 * stepping: done bit0 = lifted; no step counter, no time limit, no auto-reset.  Overwrites the context's snapshot and ray
 * buffers (call ks_reset afterwards to continue an episode).  Parity hook: the reference-generated env-layer golden
 * vectors go through the HIP observation kernel this way. */
int ks_obs_from_snapshot(ks_ctx *ctx, const void *snap, const void *rays, void *obs, void *reward, uint8_t *done, void *info, void *stream);

/* Free-running rollout: n_iter env-steps of EVERY env in ONE launch, every stepping workgroup (16 envs, one CU) running its own
 * loop with no synchronisation between workgroups -
 *     actor forward of its envs (3-layer MLP on the matrix cores, newest published weights) + exploration noise + the
 *     check_grasp / scripted-lift rule  ->  15 substeps  ->  rangefinder rays  ->  observation / reward / done / auto-reset
 *     ->  replay write (open-episode buffers) + episode hand-over
 * i.e. what kr_actor_select + ks_step + kr_store_transition do per env-step (main_DDPGfD.py:424-464 around ENV:1495-1552), fused.
 * A lock-step launch lasts as long as its slowest wave; here a wave (round 6: with one 16-env group per
 * workgroup the four waves of a workgroup never meet inside a launch; otherwise a workgroup) starts its next env-step the
 * moment it has finished the last.  Per env the arithmetic, the noise stream (Philox keyed by seed, the env's own step count,
 * env) and therefore the trajectory are those of the lock-step calls for the same weights.
 * A context with more 16-env groups than the GPU has compute units (8192 envs; many objects: one partly filled group per object)
 * keeps one persistent workgroup per compute unit; the groups are taken from a ready queue - a workgroup steps the group at its
 * head once and puts it back behind the others - so that no workgroup idles while a group is ready and every env still does
 * exactly n_iter env-steps per launch (environment variable KS_ROLLOUT_DEAL=static / rr: fixed deals instead; the multi-geom
 * build keeps the round-robin deal; the exact mode below always deals them).
 *
 * Actor weights: `actor_pub` holds 3 parameter buffers of `actor_stride` floats (layout: offsets off_*, torch.nn.Linear
 * layout); `actor_ver` is a device counter that the learner increments AFTER it has completely written buffer
 * (ver % 3): a workgroup reads the counter at the start of every env-step and uses that buffer (and repeats the forward in the
 * unlikely case that two more versions were published meanwhile).
 * Episodes: two open-episode buffers per env, cur_* [2][n][horizon][...]; a finished episode that is kept (len - n_steps > 1,
 * main_DDPGfD.py:469-471) is handed over by setting pub_len[buf][env] = len (release) and switching to the other buffer; the
 * consumer (the learner's stream: kr_rank / kr_commit / kr_advance_ring on buffer `buf` with cur_len = pub_len + buf * n) clears
 * it.  If the other buffer has not been consumed yet the finished episode is dropped and counted in `dropped`.
 * Contexts: env-major observations and auto_reset; one model or many.
 *   precision 32: observations in the stepping kernel (the default).
 *   precision 64, the exact mode (libkinova_sim.so only; libkinova_sim_mg.so refuses it): the physics state, contacts, rays,
 *     observation, reward and done are fp64, with the arithmetic of ks_step on that context, and go to the fp64 sim_* buffers.
 *     The policy and the replay stay fp32: the actor reads the fp32 rounding of the fp64 observation (obs / prev_obs), the replay
 *     rows are that same rounding, the reward is rounded once.  So per env the trajectory equals the lock-step
 *     kr_actor_select -> ks_step -> (sim outputs rounded to fp32) -> kr_store_transition, bit for bit.  One persistent workgroup
 *     per compute unit steps its 16-env groups in turn, barrier-joined (KS_PLAN_WORKGROUPS, or KS_PLAN_RUNS / KS_PLAN_ROUND_ROBIN
 *     with more groups than workgroups); no ready queue, no time budget (budget_ticks != 0: KS_ERR_STATE).
 * Scripted demonstrators (ks_set_rollout_controller below): with a controller set, the policy phase of every env-step is the
 * controller's rule instead of the actor forward and the check_grasp / scripted-lift rule - in every scheduling form, both
 * precisions (the exact mode feeds it the fp32 rounding of the fp64 observation, as it feeds the actor), both libraries.  actor_pub,
 * actor_ver, actor_stride, the offsets, h1 / h2, sigma and max_action are then ignored and the pointers may be NULL.  Everything behind
 * the action is unchanged - lift steps are not stored, an episode that ends during the lift writes its outcome into the last stored
 * transition (the demonstration loop's own storage rule, expert_data.py:789-793), the hand-over, the keep rule, counters, log and
 * pool - so per env trajectory and stored transitions are those of kr_controller_select -> ks_step -> kr_store_transition. */
typedef struct {
    const float *actor_pub;
    const int64_t *actor_ver;
    int64_t actor_stride;
    int64_t off_w1, off_b1, off_w2, off_b2, off_w3, off_b3;
    int32_t h1, h2;                  /* hidden widths: 256-256, 400-300, 128-128 or 64-64 */
    float sigma, max_action;         /* exploration noise std (max_action * expl_noise), action bound */
    int32_t skip_steps;              /* check_grasp from this step of an episode on (6, main_DDPGfD.py:418) */
    int32_t with_replay;
    uint64_t seed;
    /* engine state (kinovagrasping_amd.rollout.RolloutEngine) */
    float *obs, *prev_obs;           /* [n, 82] */
    uint8_t *has_prev, *ready, *lifting;
    int64_t *t, *steps_total;        /* [n] steps in the episode / since the start (the noise counter; stored device-visibly: kr_wait_min paces the learner's stream on it) */
    float *action, *action_t;        /* [n, 4], [4, n] */
    float *reward_out; uint8_t *done_out;
    /* ks_step's outputs (as passed to ks_step): sim_obs, sim_reward, sim_info and sim_final_obs have the context's precision */
    void *sim_obs, *sim_reward; uint8_t *sim_done; void *sim_info, *sim_final_obs;
    /* open episodes */
    int32_t horizon, n_steps;
    float *cur_state, *cur_next, *cur_action, *cur_reward, *cur_not_done;
    int64_t *cur_len;                /* [2][n] */
    uint8_t *cur_sel;                /* [n] */
    int64_t *pub_len;                /* [2][n] */
    int64_t *counters;               /* [4]: episodes finished, lifted, kept, dropped (a -DKS_ROLLOUT_STAMP diagnostic build writes [8 + 4 * 512 + 8]) */
    /* Round 6, opt-in: 0 = every env does exactly n_iter env-steps (the default and what every parity test runs).  > 0: a TIME budget in ticks of the
     * 100 MHz device clock - a wave starts no further env-step of its four envs once that long has passed since it entered the launch, so envs advance
     * by time: between 1 and n_iter env-steps each, steps_total[] says how many.  Per env the trajectory is still the lock-step one (same arithmetic, noise
     * keyed by the env's own step count).  For contexts whose objects differ widely in cost (a curriculum stage holding bowls and cubes: the slowest
     * object otherwise paces every env) - at the price of an uneven object mix in what is collected.  Needs the wave form (ks_rollout_plan:
     * KS_PLAN_WAVES), KS_ERR_STATE otherwise. */
    int64_t budget_ticks;
    /* Optional (NULL = not counted): int64 [1], incremented once per actor forward that was repeated because the version counter had
     * advanced by two or more while the forward read buffer (ver % 3) - once per deciding workgroup (KS_PLAN_WORKGROUPS / queue / deals)
     * or per wave (KS_PLAN_WAVES).  Diagnostic of the weight hand-off above; every word of counters[] is taken. */
    int64_t *repeats;
    /* Optional (NULL = not counted): int64 [3], KS_PLAN_WAVES only - [0] runs of envs that a wave which had done its env-steps of the launch took
     * over from a slower wave of its workgroup, [1] waits for such a hand-over that ended on the clock (50 ms), [2] of [0]: taken from a run of two
     * envs (a second split).  Every env still does exactly n_iter env-steps on its lock-step trajectory; KS_ROLLOUT_TAKEOVER=0 (read when the
     * context is created) or a time budget switches the hand-overs off. */
    int64_t *takeovers;
} ks_rollout_args;
int ks_rollout(ks_ctx *ctx, int32_t n_iter, const ks_rollout_args *args_host, void *stream);

/* The scripted demonstrators on the free-running path: the reference's naive, position-dependent and combined controllers
 * (expert_data.py:318-671; main_DDPGfD.py --mode naive / combined) act in ks_rollout instead of the actor.  The context owns a small
 * record in device memory (mode, lift rule, and a context-owned float [2][N] holding every env's (obs[21], obs[81]) of its episode's
 * start) that `stream` writes - like the start pool's and the episode log's - so a ks_rollout captured BEFORE this call acts by the
 * controller when the graph is replayed after it.  (The reverse needs care: a ks_rollout issued with NULL actor pointers must not
 * run once the controller has been cleared.)  The call zeroes the [2][N] buffer: it is meant for episode boundaries - an env that is
 * mid-episode (t > 0) when the controller is set uses (0, 0) as its start values until its next episode begins.
 * lift_rule: KS_LIFT_RULE_TRAIN (ready |= check_grasp && has_prev && t + 1 >= skip_steps; lifting = ready) or KS_LIFT_RULE_EXPERT
 * (ready |= check_grasp && has_prev && t >= 2; lifting = ready && t > 10) - kinova_rollout.h, kr_controller_select.
 * KS_CONTROLLER_NONE clears the record: the actor path again (lift_rule is then ignored).  KS_ERR_STATE before ks_load_model,
 * KS_ERR_INVALID for values out of range.  No host synchronisation.  Both precisions, both libraries.
 * ks_get_rollout_controller: *mode / *lift_rule (host) as last set, and a device-to-device copy of the start values (init: device float
 * [2, N]), asynchronous on `stream`; any pointer may be NULL.  KS_ERR_STATE before ks_load_model. */
enum { KS_CONTROLLER_NONE = 0, KS_CONTROLLER_NAIVE = 1, KS_CONTROLLER_POSITION_DEPENDENT = 2, KS_CONTROLLER_COMBINED = 3 };
enum { KS_LIFT_RULE_TRAIN = 0, KS_LIFT_RULE_EXPERT = 1 };
int ks_set_rollout_controller(ks_ctx *ctx, int32_t mode, int32_t lift_rule, void *stream);
int ks_get_rollout_controller(ks_ctx *ctx, int32_t *mode, int32_t *lift_rule, float *init, void *stream);

/* How ks_rollout would schedule this context's env groups (16 envs sharing one object's hull tables) on the device it runs on - the library's
 * own decision, for callers that report or warn about it (bench.py, pipeline.AsyncTrainer; ADVICE r5: they used to re-derive it from environment
 * variables).  *mode: KS_PLAN_WAVES one group per persistent workgroup, its four waves run free (no barrier inside a launch);
 * KS_PLAN_WORKGROUPS one group per workgroup, the waves joined by barriers at every phase (KS_ROLLOUT_WAVES=0, or a context the wave form cannot
 * hold); KS_PLAN_QUEUE more groups than resident workgroups, taken from a ready queue; KS_PLAN_RUNS / KS_PLAN_ROUND_ROBIN more groups than
 * workgroups in a fixed deal (contiguous runs / round-robin: KS_ROLLOUT_DEAL=static / rr, and the multi-geom library's default) - a launch then
 * runs at the pace of the workgroup with the most groups.  *groups: 16-env groups incl. the partly filled one of every object;
 * *workgroups: persistent workgroups of a launch.  After ks_load_model(s). */
enum { KS_PLAN_WAVES = 0, KS_PLAN_WORKGROUPS = 1, KS_PLAN_QUEUE = 2, KS_PLAN_RUNS = 3, KS_PLAN_ROUND_ROBIN = 4 };
int ks_rollout_plan(ks_ctx *ctx, int32_t *mode, int32_t *groups, int32_t *workgroups);

/* HIP event timing of the dominant kernel: average duration (ms) of the env-step kernel launches
 * since the last call with reset != 0, measured with hipEvents on the launch stream - every 4th launch is sampled (the two
 * event records cost ~8 us of stream time per sampled launch; KS_EVENT_STRIDE=1 samples all of them).  Host sync.
 * (fp32 contexts: that kernel is the 15 substeps of every env plus the rangefinder rays of the workgroup's own envs.) */
int ks_kernel_time(ks_ctx *ctx, int reset, double *avg_ms_host, int64_t *launches_host);

int ks_version(void);

#ifdef __cplusplus
}
#endif
#endif
