/*
 * ppo_hip.h -- C ABI of libppo_hip.so, the MI355X (gfx950) engine behind the
 * ProximalPolicyOptimization.jl rollout-and-update path.
 *
 * The reference has NO FFI: its boundary is Julia multiple dispatch on the generic functions of
 * module ProximalPolicyOptimization (src/ProximalPolicyOptimization.jl:16-30).  Each entry point
 * below names the reference function it stands in for; the Julia-side binding (ccall methods for
 * HipVecEnv / HipPolicy / HipRollouts) is in julia/ProximalPolicyOptimizationHIP.jl and
 * INTEGRATION.md.  The Python mirror used by the tests is proximalpolicyoptimization.jl_amd/.
 *
 * Conventions
 *  - every function returns int32 status: 0 = ok, <0 = error; ppo_last_error() gives the text.
 *    (reference: ErrorException / AssertionError, SURVEY.md 8(b) "Errors")
 *  - every pointer is a HOST pointer owned by the caller unless the name ends in _dev;
 *    getters copy into caller buffers; handles own all device memory.
 *  - action indices crossing this ABI are 0-based int32 (Julia shim adds/subtracts 1).
 *  - layouts: rollout columns are time-major [T,N]; states are int8 [.,H,F] (row = half-edge,
 *    F = 72 features: 36 template scores then 36 template degrees); the action mask travels as
 *    the active-quad bit mask (bit q set = quad q active; entries a with quad a/16 inactive are
 *    -Inf in the reference, test/quad_game_utilities.jl:39-44).
 *  - policy parameters are one flat float32 vector in Flux order (W1,b1, the num_hidden_layers-1 hidden->hidden
 *    (W,b) pairs, W_out,b_out), W stored [out,in] column-major, so Flux.params(policy) round-trips (test/policy.jl:9-19).
 *  - one engine per HOST THREAD: the device (ppo_device_init), the stream (ppo_set_stream), the kernel timers, the RCCL
 *    communicator and the error text are thread-local, so a process may run several engines side by side (one thread per
 *    GPU); a handle belongs to the thread that created it and is not re-entrant.  The ppo_set_* tuning knobs are
 *    process-wide.  Each starts at its PPO_* environment variable, read once at load, else at its built-in default;
 *    passing -1 to its setter restores that starting value.
 */
#ifndef PPO_HIP_H
#define PPO_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ppo_env_s* ppo_env_t;
typedef struct ppo_policy_s* ppo_policy_t;
typedef struct ppo_adam_s* ppo_adam_t;
typedef struct ppo_rollouts_s* ppo_rollouts_t;

#define PPO_OK 0
#define PPO_ERR_ARG (-1)        /* bad argument / failed @assert-equivalent            */
#define PPO_ERR_HIP (-2)        /* HIP runtime error                                   */
#define PPO_ERR_DEVICE_FLAG (-3)/* device-side error flag (zero-prob action sampled,   */
                                /* invalid action index, stepping a terminated env)    */
#define PPO_ERR_UNSUPPORTED (-4)

/* advantage plugin modes (batch_advantage, src/ProximalPolicyOptimization.jl:29; no
 * implementation exists in the reference, old scripts use raw returns) */
#define PPO_ADV_RETURNS 0            /* advantage = returns (what the reference's old scripts do)            */
#define PPO_ADV_RETURNS_NORMALISED 1 /* (R - mean) / (std + 1e-8) over the minibatch (population std, fp64 stats) */
#define PPO_ADV_GAE 2                /* the GAE(gamma, lambda) column of ppo_rollouts_compute_gae (host-supplied state values) or _gae_critic */
#define PPO_ADV_GAE_NORMALISED 3     /* the same, normalised over the minibatch like mode 1 */

/* ---------------------------------------------------------------- library / device */
int32_t ppo_version(void);
int32_t ppo_last_error(char* buf, int64_t cap);
int32_t ppo_device_init(int32_t device_ordinal);          /* hipSetDevice + private stream     */
int32_t ppo_set_stream(void* hip_stream);                 /* run on an external hipStream_t     */
int32_t ppo_device_synchronize(void);
int32_t ppo_device_count(int32_t* out);
/* rollout execution: 0 = three launches per step (observe, policy forward + sample, step!), 1 = ONE launch for the
 * whole T-step rollout wherever the shape is covered (envs are independent: each wavefront walks its envs through all
 * steps with the env state in LDS), -1 = the value at load (PPO_ROLLOUT_PERSISTENT, else automatic: one launch for
 * Q = 8 envs, per-step launches otherwise).  Same results bit for bit; per-step launches are always used while a disk
 * sink is attached. */
int32_t ppo_set_rollout_persistent(int32_t mode);
/* state storage of engine-collected rollouts (R4, src/rollout_buffer.jl:1-22: the reference boxes every state):
 * 0 = expanded observation rows [H][F] int8 per transition (2304 B for Q = 8), 1 = compact: the env snapshot the rows
 * are derived from (score[V] + degree[V] int8 = 64 B for Q = 8, plus the active-quad word) -- the train forward
 * re-derives the rows exactly as state(env) does, the getters expand on demand; -1 = the value at load
 * (PPO_ROLLOUT_COMPACT, else automatic: compact when the expanded rollout would exceed 32 GiB (PPO_COMPACT_AUTO_BYTES;
 * below that the rows are kept because re-deriving them costs the train forward 3 % in fp32 and 17 % in bf16 mode) or
 * while a disk sink is attached (the streamed record shrinks 28x)).  Same results bit for bit.  Host-supplied rollouts (ppo_rollouts_set) are always expanded. */
int32_t ppo_set_rollout_compact(int32_t mode);

/* ---------------------------------------------------------------- standalone ops (parity entry points) */
/* compute_returns(rewards, terminal, discount)            src/collect_rollouts.jl:26-42
 * flat concatenated-episodes semantics; discount_is_f32=0 reproduces the Float64 running value */
int32_t ppo_compute_returns(const float* rewards, const uint8_t* terminal, int64_t n,
                            double discount, int32_t discount_is_f32, float* out);
/* same scan on time-major [T,N] columns (v=0 at each column tail) -- the engine's hot layout */
int32_t ppo_compute_returns_tn(const float* rewards, const uint8_t* done, int64_t T, int64_t N,
                               double discount, int32_t discount_is_f32, float* out);
/* GAE(gamma,lambda) extension (values [T+1,N]); lambda=1, V=0 == ppo_compute_returns_tn */
int32_t ppo_gae_tn(const float* rewards, const uint8_t* done, const float* values, int64_t T,
                   int64_t N, double gamma, double lambda, float* adv_out, float* ret_out);
/* the same scan with a bootstrap column boot [T,N] (no reference op): a done row takes V[t+1] := boot[t] instead of 0 while
 * the trace is still cut there.  boot = the value of the state a time-limit truncation cut the episode in, exactly 0.0f at
 * real terminals and at rows that are not done; boot == 0 everywhere gives ppo_gae_tn's numbers */
int32_t ppo_gae_boot_tn(const float* rewards, const uint8_t* done, const float* values, const float* boot, int64_t T,
                        int64_t N, double gamma, double lambda, float* adv_out, float* ret_out);
/* rand(Categorical(p)) for B rows of A probabilities given B uniforms   src/collect_rollouts.jl:6-7
 * actions 0-based; err[b]=1 when the sampled entry has p==0 (the reference's @assert) */
int32_t ppo_categorical_sample(const float* probs, const float* u, int64_t B, int64_t A,
                               int32_t* actions, float* p_sel, int32_t* err);
/* get_linear_action_index (1-based in, 1-based out)        src/train.jl:48-52 */
int32_t ppo_linear_action_index(const int64_t* actions1, int64_t B, int64_t A, int64_t* out);
/* ppo_loss_with_entropy on given probs [A,B] (column-major), 1-based linear indices
 *                                                          src/train.jl:21-26,35-46 */
int32_t ppo_loss_with_entropy(const float* probs, const int64_t* lin_idx1, const float* p_old,
                              const float* adv, int64_t B, int64_t A, double epsilon,
                              double* ppoloss, double* entropyloss);
/* counter RNG exposed for tests: Philox4x32-10 */
int32_t ppo_philox4x32_10(const uint32_t* ctr4, const uint32_t* key2, int64_t n, uint32_t* out4);

/* ---------------------------------------------------------------- env plugin (batched) */
/* PPO.state / reward / is_terminal / reset! / step!        src/ProximalPolicyOptimization.jl:16-20
 * kind 0 = synthetic rand-poly-shaped env (Q quad slots, H=4Q half-edges, A=16Q actions) */
int32_t ppo_env_create(int32_t kind, int64_t num_envs, int64_t global_env_offset, int32_t Q,
                       int32_t max_actions, float no_action_reward, uint64_t seed, ppo_env_t* out);
int32_t ppo_env_destroy(ppo_env_t env);
int32_t ppo_env_dims(ppo_env_t env, int64_t* N, int32_t* H, int32_t* F, int32_t* A);
int32_t ppo_env_reset(ppo_env_t env);                                   /* reset!      :19 */
int32_t ppo_env_step(ppo_env_t env, const int32_t* actions0);           /* step!       :20 */
int32_t ppo_env_get_state(ppo_env_t env, int8_t* obs, uint32_t* active);/* state       :16 */
int32_t ppo_env_get_reward(ppo_env_t env, float* out);                  /* reward      :17 */
int32_t ppo_env_get_terminal(ppo_env_t env, uint8_t* out);              /* is_terminal :18 */
int32_t ppo_env_get_internal(ppo_env_t env, int8_t* score, int8_t* degree, int32_t* steps,
                             uint32_t* episode, uint32_t* tick);
/* Caller-supplied env states: score and degree [N][V] (V = 4Q), active [N] active-quad words.  Leaves every env as reset!
 * would, with these arrays in place of the Philox draw: steps = 0, reward = 0, done = 0; the episode and tick counters are
 * untouched.  Checked on the host before anything is uploaded (PPO_ERR_ARG): active != 0, no bit at or above Q, every entry
 * of an inactive quad 0 in both arrays. */
int32_t ppo_env_set_internal(ppo_env_t env, const int8_t* score, const int8_t* degree, const uint32_t* active);
int32_t ppo_env_get_active(ppo_env_t env, uint32_t* active);
int32_t ppo_env_check_errors(ppo_env_t env, int32_t* flags_or_null);
/* rand(Categorical(ap)) walks the CDF sequentially; when the fp32 sum of ap stops short of u (u within 2^-24 of 1) the
 * walk ends on the LAST action, and if that action is masked the reference's `@assert ap[a] > 0.0` throws
 * (src/collect_rollouts.jl:7) -- about 3 in 10^8 samples.  Default (strict = 0): the residue goes to the last action
 * with ap > 0 and flag bit 32 records it.  strict = 1: the rollout call fails with PPO_ERR_DEVICE_FLAG like the
 * reference's AssertionError. */
int32_t ppo_env_set_strict_sampling(ppo_env_t env, int32_t strict);

/* ---------------------------------------------------------------- policy plugin */
/* SimplePolicy.Policy(in, hidden, num_hidden_layers, out)  test/policy.jl:9-19
 * in = 72 or 216 features, hidden = 1..256 (widths other than 128 / 256 run zero-padded on the next wider kernel, exact),
 * num_hidden_layers = 1..4 (2: the fused kernels; 1, 3, 4: the layer-looped forms of the same kernels, fp32 only),
 * out = 4 (the quad game's actions per edge, test/quad_game_utilities.jl:95).  Anything else: PPO_ERR_UNSUPPORTED. */
int32_t ppo_policy_create(int32_t F, int32_t hidden, int32_t num_hidden_layers,
                          int32_t out_per_edge, ppo_policy_t* out);
/* arithmetic type of the policy MLP (BASELINE config 5: "bf16 MLP on MFMA + fp32 GAE").  PPO_DTYPE_F32 (default):
 * exact fp32 MFMA.  PPO_DTYPE_BF16: weights and layer inputs rounded to bfloat16 (RNE), fp32 accumulation, bias,
 * leakyrelu, softmax, sampling, loss and Adam (fp32 master parameters) unchanged; saved activations and the
 * gradient signals dZ are bf16.  Call before training; the reference has no counterpart (Flux Float32 only). */
#define PPO_DTYPE_F32 0
#define PPO_DTYPE_BF16 1
int32_t ppo_policy_set_dtype(ppo_policy_t pol, int32_t dtype);
int32_t ppo_policy_get_dtype(ppo_policy_t pol, int32_t* dtype);
int32_t ppo_policy_destroy(ppo_policy_t pol);
int32_t ppo_policy_num_params(ppo_policy_t pol, int64_t* n);
int32_t ppo_policy_set_params(ppo_policy_t pol, const float* flat);     /* Flux.params order */
int32_t ppo_policy_get_params(ppo_policy_t pol, float* flat);
/* batch_action_probabilities(policy, state) -> probs [A,B] column-major (B=1: action_probabilities)
 *                                                          test/quad_game_utilities.jl:65-79 */
int32_t ppo_policy_forward(ppo_policy_t pol, const int8_t* states, const uint32_t* active,
                           int64_t B, int32_t H, float* probs);
/* flat gradient of the last ppo_forward_backward (Flux order) */
int32_t ppo_policy_get_grad(ppo_policy_t pol, float* flat);
/* device pointer to the flat gradient buffer [num_params + 2] (grad, ppo-sum, entropy-sum):
 * the hand-off point for the data-parallel all-reduce (RCCL through torch.distributed) */
int32_t ppo_policy_grad_buffer_dev(ppo_policy_t pol, void** dev_ptr, int64_t* n_floats);

/* ---------------------------------------------------------------- optimiser */
/* Flux.Optimiser(Adam(eta,(beta1,beta2),eps)) + Flux.update!            src/train.jl:81,155-158 */
int32_t ppo_adam_create(ppo_policy_t pol, double eta, double beta1, double beta2, double eps,
                        ppo_adam_t* out);
int32_t ppo_adam_destroy(ppo_adam_t opt);
int32_t ppo_adam_get_lr(ppo_adam_t opt, double* eta);                    /* get_optimizer_learning_rate */
int32_t ppo_adam_set_lr(ppo_adam_t opt, double eta);
int32_t ppo_adam_get_state(ppo_adam_t opt, float* m, float* v, double* beta_pow2);
int32_t ppo_adam_set_state(ppo_adam_t opt, const float* m, const float* v, const double* beta_pow2);
/* number of epochs this optimiser has trained through ppo_train.  Together with the caller's seed it keys the device
 * minibatch permutation (the stand-in for randperm, src/train.jl:93), so there is no hidden process-global state: the
 * same seed with a fresh optimiser reproduces a run, and a checkpointed optimiser (m, v, beta powers, epoch count)
 * resumes one. */
int32_t ppo_adam_get_epoch_count(ppo_adam_t opt, int64_t* epochs);
int32_t ppo_adam_set_epoch_count(ppo_adam_t opt, int64_t epochs);

/* Flux.Optimiser chain (Flux 0.13 legacy Flux.Optimise) of 1..4 members, each kind at most once, in any order: the
 * members whose `eta` get_optimizer_learning_rate multiplies (src/train.jl:155-158).  Flux.update! (src/train.jl:81)
 * then does, per parameter: D = grad (f32); D = apply!(member, x, D) for each member in chain order; x -= D.
 * Float64 hyper-parameters against Float32 arrays: each member's arithmetic is float64 where a float64 operand enters,
 * and its output D (and every state array it stores) is rounded to float32:
 *   Adam      exactly ppo_adam_create's update (m, v, float64 beta powers)
 *   ExpDecay  D = f32(D * eta_n); at its n-th update! (n counts them, this one included) first
 *             eta = max(eta * decay, clip) when n > start && n % decay_step == 0 && (decay_step > 1 || n == start + 1)
 *             (Flux counts the arrays already at step n: with decay_step == 1 it decays exactly once)
 *   Descent   D = f32(D * eta)
 *   Momentum  v = f32(rho v - eta D); D = -v
 *   Nesterov  d = rho*rho v - ((1 + rho) eta) D (old v, float64); v = f32(rho v - eta D); D = f32(-d)
 *   RMSProp   acc = f32(rho acc + ((1 - rho) D) D); D = f32(D (eta / (sqrt_f32(acc) + epsilon)))
 * Members without an eta (x: the float32 parameter before this step's update; "array": one of the 2L + 2 arrays of
 * Flux.params, in order W1, b1, (W, b) per hidden->hidden layer, W3, b3):
 *   ClipValue    D = f32(clamp(D, -thresh, thresh)); NaN stays NaN
 *   ClipNorm     per array: S = the float64 sum of D_i^2 over the array, rounded once from the exact sum (the squares of
 *                float32 values are exact in float64); nrm = f32(sqrt(S)); if nrm > thresh: D_i = f32(D_i (thresh / nrm)).
 *                Julia takes norm() of a Vector{Float32} through BLAS snrm2, which is not correctly rounded: this is the
 *                deterministic, correctly rounded definition (a fixed-order double-double sum on the device)
 *   WeightDecay  D = f32(D + wd x)
 *   InvDecay     at its n-th update! (n counts them, this one included): D = f32(D (1 / (1 + gamma n)))
 * Flux.AdamW(eta, beta, decay) is Optimiser(Adam(1, beta), WeightDecay(decay), Descent(eta)).
 * hyper: n rows of 5 doubles, unused trailing entries ignored:
 *   Adam (eta, beta1, beta2, epsilon)   ExpDecay (eta, decay, decay_step, clip, start)   Descent (eta)
 *   Momentum (eta, rho)   Nesterov (eta, rho)   RMSProp (eta, rho, epsilon)
 *   ClipValue (thresh)   ClipNorm (thresh)   WeightDecay (wd)   InvDecay (gamma)
 * The handle is a ppo_adam_t: ppo_train / ppo_step_batch / ppo_adam_apply take it unchanged; ppo_train's lr history is
 * the left-to-right product of the etas of the members that have one, after each epoch (the reference's ppo_train!
 * fails on a member without eta; the engine goes beyond it here).  ppo_adam_create makes the chain of Adam alone, and
 * such a chain runs the Adam kernels however it was made.  ppo_adam_get_lr returns that product on any chain;
 * ppo_adam_set_lr / _get_state / _set_state are the member-0 calls below and need a chain of Adam alone.
 * Unknown kind: PPO_ERR_UNSUPPORTED; bad n, duplicate kind, a NaN or negative thresh: PPO_ERR_ARG. */
#define PPO_OPT_ADAM 1
#define PPO_OPT_EXPDECAY 2
#define PPO_OPT_DESCENT 3
#define PPO_OPT_MOMENTUM 4
#define PPO_OPT_NESTEROV 5
#define PPO_OPT_RMSPROP 6
#define PPO_OPT_CLIPVALUE 7
#define PPO_OPT_CLIPNORM 8
#define PPO_OPT_WEIGHTDECAY 9
#define PPO_OPT_INVDECAY 10
int32_t ppo_optimiser_create(ppo_policy_t pol, int32_t n, const int32_t* kinds, const double* hyper, ppo_adam_t* out);
/* member: 0-based chain position; a member without eta (ClipValue .. InvDecay): PPO_ERR_ARG */
int32_t ppo_optimiser_get_eta(ppo_adam_t opt, int32_t member, double* eta);
int32_t ppo_optimiser_set_eta(ppo_adam_t opt, int32_t member, double eta);
/* the member's hyper row (5 doubles, as in ppo_optimiser_create): a caller may change thresh / wd / gamma (or any other
 * hyper-parameter) between calls, as Flux allows; set_hyper validates like ppo_optimiser_create */
int32_t ppo_optimiser_get_hyper(ppo_adam_t opt, int32_t member, double* hyper5);
int32_t ppo_optimiser_set_hyper(ppo_adam_t opt, int32_t member, const double* hyper5);
/* member state, Flux layout (any argument may be NULL): Adam s0 = m, s1 = v, scalars = beta powers [2];
 * Momentum / Nesterov s0 = velocity; RMSProp s0 = acc; ExpDecay / InvDecay count = update! calls seen (ExpDecay's eta:
 * _get_eta). */
int32_t ppo_optimiser_get_state(ppo_adam_t opt, int32_t member, float* s0, float* s1, double* scalars2, int64_t* count);
int32_t ppo_optimiser_set_state(ppo_adam_t opt, int32_t member, const float* s0, const float* s1,
                                const double* scalars2, const int64_t* count);

/* ---------------------------------------------------------------- rollout buffer */
/* BufferRollouts()                                          src/rollout_buffer.jl:1-22 */
int32_t ppo_rollouts_create(ppo_env_t env, int64_t capacity_T, ppo_rollouts_t* out);
/* the same for states that do not come from the built-in env (a user env's state(env) converted by the host, e.g. the
 * reference's 216-feature level-4 template, test/output/catmull-clark-policy-l4.bson): N columns of [H][F] int8 rows,
 * H = 32 or 128, F a multiple of 8 the policy was created for; filled with ppo_rollouts_set */
int32_t ppo_rollouts_create_shape(int64_t num_envs, int32_t H, int32_t F, int64_t capacity_T, ppo_rollouts_t* out);
int32_t ppo_rollouts_destroy(ppo_rollouts_t ro);
int32_t ppo_rollouts_len(ppo_rollouts_t ro, int64_t* n);                 /* Base.length :40-48 */
int32_t ppo_rollouts_dims(ppo_rollouts_t ro, int64_t* T, int64_t* N);
/* collect_rollouts!(rollouts, env, policy, ., discount)     src/rollout_buffer.jl:66-79
 * fixed-T vectorised form: T steps of all N envs with auto-reset, then compute_state_value!
 * (returns overwrite rewards, :55-64).  record_probs!=0 additionally keeps the full [T,N,A]
 * probabilities (tests only). */
int32_t ppo_collect_rollouts(ppo_rollouts_t ro, ppo_env_t env, ppo_policy_t pol, int64_t T,
                             double discount, int32_t discount_is_f32, int32_t record_probs);
/* num_episodes form (the reference's own signature): EXACTLY num_episodes whole episodes enter the buffer
 * (src/rollout_buffer.jl:73-77).  The N resident envs play them in parallel, episode e on env e mod N (env n plays
 * ceil((num_episodes - n) / N) episodes, reset! before each; envs beyond num_episodes stay idle).  Dataset order =
 * env-major concatenation of the whole episodes; length = number of valid transitions. */
int32_t ppo_collect_rollouts_episodes(ppo_rollouts_t ro, ppo_env_t env, ppo_policy_t pol,
                                      int64_t num_episodes, double discount,
                                      int32_t discount_is_f32);
/* column getters, time-major [T,N] (dataset getindex, src/rollout_buffer.jl:103-133) */
int32_t ppo_rollouts_get_states(ppo_rollouts_t ro, int8_t* states, uint32_t* active);
int32_t ppo_rollouts_get_actions(ppo_rollouts_t ro, int32_t* actions0);
int32_t ppo_rollouts_get_probs(ppo_rollouts_t ro, float* p_sel);
int32_t ppo_rollouts_get_returns(ppo_rollouts_t ro, float* returns);     /* "rewards" after :55-64 */
int32_t ppo_rollouts_get_raw_rewards(ppo_rollouts_t ro, float* rewards);
int32_t ppo_rollouts_get_terminal(ppo_rollouts_t ro, uint8_t* terminal);
int32_t ppo_rollouts_get_valid(ppo_rollouts_t ro, uint8_t* valid);
int32_t ppo_rollouts_get_full_probs(ppo_rollouts_t ro, float* probs);   /* [T,N,A], record_probs only */
/* dataset order: flat index list of the valid transitions (t*N+n), length = ppo_rollouts_len */
int32_t ppo_rollouts_get_index(ppo_rollouts_t ro, int64_t* idx);
/* batch_advantage as GAE(gamma, lambda) (north_star "GAE advantage reverse scan"; the reference declares the plugin at
 * src/ProximalPolicyOptimization.jl:29 and implements nothing).  values: [T+1][N] state values from the caller's critic
 * (row T = bootstrap value behind the last step; the reference has no value head).  Runs the LDS-tiled fp64 scan over
 * the buffer's raw rewards / terminal flags and keeps the advantage column on the device for adv_mode PPO_ADV_GAE*;
 * optional host copies of the advantages and of the lambda-returns adv + V.  lambda = 1 and V = 0 reproduce
 * compute_returns (src/collect_rollouts.jl:26-42) bit for bit. */
int32_t ppo_rollouts_compute_gae(ppo_rollouts_t ro, const float* values, double gamma, double lambda,
                                 float* adv_out_or_null, float* lambda_returns_out_or_null);
/* ppo_rollouts_compute_gae with the bootstrap column of ppo_gae_boot_tn, boot [T][N] from the host (a user's critic on
 * the final states of ppo_rollouts_truncated, or of the user's own env).  Works on any buffer.  The column stays in the
 * buffer (ppo_rollouts_get_boot) */
int32_t ppo_rollouts_compute_gae_boot(ppo_rollouts_t ro, const float* values, const float* boot, double gamma, double lambda,
                                      float* adv_out_or_null, float* lambda_returns_out_or_null);
/* Time-limit truncations of a buffer collected from the built-in env (no reference op).  The env ends an episode at its
 * optimum (a terminal) or after max_actions steps (a truncation) and records both as `done`; which one it was is
 * re-derived on the device by replaying the stored action on the stored state: terminated = (sum |score| == |sum score|
 * over the active quads behind the step).  truncated_out [T][N]: 1 at done && valid transitions that did not reach the
 * optimum, 0 everywhere else.  count_out: their number K.  final_states_out [K][H][F] / final_active_out [K]: the
 * observation and the active word of the state each of them was cut in, in ascending transition id t*N + n; asked for
 * with capacity < K: PPO_ERR_ARG (call once with null outputs for K).  A buffer without an env template
 * (ppo_rollouts_create_shape): PPO_ERR_UNSUPPORTED */
int32_t ppo_rollouts_truncated(ppo_rollouts_t ro, uint8_t* truncated_out_or_null, int8_t* final_states_out_or_null,
                               uint32_t* final_active_out_or_null, int64_t capacity, int64_t* count_out);
/* the boot column [T][N] the latest ppo_rollouts_compute_gae_boot / _gae_critic_boot on these rollouts left in the
 * buffer (none since the latest collection: PPO_ERR_ARG) */
int32_t ppo_rollouts_get_boot(ppo_rollouts_t ro, float* boot_out);
/* load columns from host (tests / generic host-side envs) */
int32_t ppo_rollouts_set(ppo_rollouts_t ro, int64_t T, const int8_t* states, const uint32_t* active,
                         const int32_t* actions0, const float* p_sel, const float* returns,
                         const uint8_t* terminal);

/* ---------------------------------------------------------------- training */
/* forward + loss + backward of one minibatch given dataset positions `sample_idx` (0-based
 * positions into the dataset order).  Leaves the flat gradient (mean over B_global) in the
 * policy's gradient buffer.  B_global = minibatch size across all data-parallel ranks.
 *                                                          src/train.jl:35-46,65-79 */
int32_t ppo_forward_backward(ppo_policy_t pol, ppo_rollouts_t ro, const int64_t* sample_idx,
                             int64_t B, int64_t B_global, double epsilon, double entropy_weight,
                             int32_t adv_mode);
/* Which backward kernel a minibatch takes (same gradient, different reduction tree: results agree to fp32 rounding):
 * up to `tiles` 32-row tiles the three-product form (dZ kernel + output-stationary split-K weight-gradient kernel: no
 * per-workgroup gradient slabs, the fixed cost that dominates a small optimiser step), above it the fused kernel that
 * keeps every weight gradient resident in MFMA accumulators.  Default PPO_BWD_SMALL_MAX_TILES, else 384 (-1 restores
 * it), 0 = always fused.  While the
 * split-fp32 training pass is on (ppo_set_bwd_split_bf16, the default) its fused backward is faster at every size and the
 * threshold that applies is PPO_BWD_SMALL_MAX_TILES_SPLIT (default 0). */
int32_t ppo_set_bwd_small_max_tiles(int64_t tiles);
/* fp32 policies, fused backward (Policy(72, h, 2, 4)): 1 = its three big products (dH1 = dZ2 W2, dW2 += dZ2^T H1,
 * dW1 += dZ1^T X) run on the bf16 matrix pipe as SPLIT-fp32 products -- every fp32 operand is the exact sum of three
 * bfloat16 pieces, six piece products (fp32 accumulation) carry a product to one fp32 rounding -- instead of on the 16x
 * slower fp32 matrix instructions; 0 = the pure fp32-MFMA kernel; -1 = the default (environment PPO_BWD_SPLIT_BF16, else
 * on).  The same switch selects the split-fp32 train forward for minibatches up to PPO_FWD_SPLIT_MAX_TILES states.  Same inputs, same gradient slab; gradients agree with the other form to fp32 rounding and meet the same 2e-5 max|g|
 * bar against the float64 restatement. */
int32_t ppo_set_bwd_split_bf16(int32_t mode);
/* Small minibatches (the per-GPU shard of a strong-scaling run): up to `tiles` 32-row tiles the train forward, the loss and
 * the backward-data pass of a tile run in ONE workgroup (k_policy_train_tile: nothing but the operands of the weight-
 * gradient products leaves the CU) followed by the split-K weight-gradient kernel, instead of the separate forward and
 * backward launches.  Same gradient to fp32 rounding (the layer-3 partial sums are added in another order), bitwise
 * reproducible.  Default PPO_TRAIN_TILE_MAX_TILES, else 0 (-1 restores it), 0 = never. */
int32_t ppo_set_train_tile_max_tiles(int64_t tiles);
/* Likewise for the train forward: minibatches of up to `states` states (H = 32) give every state to 2 or 4 waves instead
 * of one, so a minibatch smaller than the chip's 1024 SIMDs still fills it (logits agree with the one-wave kernel to
 * fp32 rounding: the layer-3 partial sums are added in a different order).  Default PPO_FWD_SPLIT_MAX_STATES, else 512
 * (-1 restores it), 0 = never. */
int32_t ppo_set_fwd_split_max_states(int64_t states);
/* The split-fp32 train forward (ppo_set_bwd_split_bf16) of an H = 32 minibatch at kernel width `hid` (128 or 256) takes
 * its two-tiles-per-pass form from `tiles` 32-row tiles on.  Default PPO_FWD_SPLIT_T2_MIN_TILES_128 / PPO_FWD_SPLIT_T2_MIN_TILES,
 * else 1024 / 1536 (-1 restores it), 0 = never.  Same results bit for bit. */
int32_t ppo_set_fwd_split_t2_min_tiles(int32_t hid, int64_t tiles);
/* And for the one-launch rollout: up to `envs` resident envs (Q = 8, fp32) every env is walked by 2 or 4 waves instead of
 * one.  Unlike the train forward this split is BIT-EXACT (the layer-3 fmaf chain is handed from wave to wave in tile
 * order), so it changes nothing but the time.  Default PPO_ROLLOUT_SPLIT_MAX_ENVS, else 512 (-1 restores it), 0 = never. */
int32_t ppo_set_rollout_split_max_envs(int64_t envs);
/* Flux.update!(optimizer, weights, grad)                    src/train.jl:81 */
int32_t ppo_adam_apply(ppo_adam_t opt, ppo_policy_t pol);
/* losses of the last forward_backward (after any all-reduce): (ppoloss, entropy_weight*entropyloss)
 *                                                          src/train.jl:83 */
int32_t ppo_last_losses(ppo_policy_t pol, double* ppoloss, double* entropyloss);
/* step_batch!                                               src/train.jl:54-84 */
int32_t ppo_step_batch(ppo_policy_t pol, ppo_adam_t opt, ppo_rollouts_t ro,
                       const int64_t* sample_idx, int64_t B, double epsilon, double entropy_weight,
                       int32_t adv_mode, double* ppoloss, double* entropyloss);
/* all-reduce hook: called once per optimiser step between backward and Adam with the device
 * gradient buffer (sum over ranks expected on return, enqueued on / ordered with the stream).
 * Contract: the hook must reduce EXACTLY the buffer it is handed on each call -- `grad_dev`, `n_floats` floats -- and it
 * must SUM (not average): ppo_train also calls it on two small non-gradient buffers at its start (the shard-length
 * exchange, 2 * world floats, and a 1-float status agreement), so a hook that ignores the pointer / count and reduces a
 * cached gradient tensor, or one that divides by the world size, breaks the exchange (ppo_train then fails on every
 * rank alike with "shard-length exchange is inconsistent").  Return 0 on success. */
typedef int32_t (*ppo_allreduce_fn)(void* ctx, void* grad_dev, int64_t n_floats);
/* ppo_train!(policy, optimizer, dataset, epsilon, batch_size, num_epochs, entropy_weight)
 *                                                          src/train.jl:86-153
 * perm: NULL -> device Feistel permutation keyed by (seed, ppo_adam_get_epoch_count), else num_epochs
 * explicit 0-based permutations of length len (randperm, :93).  hist arrays have num_epochs
 * entries: mean per-batch losses and the learning rate (:127,144-150).
 * Data parallel: rank / world = this process's place among the ranks that each hold an env shard (1 process: 0 / 1).
 * The minibatch of a step is the union of `batch_size` samples per rank.  Shards may differ in length: the ranks
 * exchange their dataset lengths once per call (through the hook), all run max_r ceil(len_r / batch_size) steps per
 * epoch, each step's gradient is the exact mean over the samples all ranks contributed to it, and a rank whose shard
 * is exhausted contributes zeros -- so every rank issues the same sequence of collectives.  batch_size must not
 * exceed the shortest shard (the reference's @assert, on every rank alike). */
int32_t ppo_train(ppo_policy_t pol, ppo_adam_t opt, ppo_rollouts_t ro, double epsilon, int64_t batch_size,
                  int32_t num_epochs, double entropy_weight, int32_t adv_mode, const int64_t* perm, uint64_t seed,
                  int32_t rank, int32_t world, ppo_allreduce_fn allreduce, void* allreduce_ctx, double* ppo_hist,
                  double* entropy_hist, double* lr_hist);

/* ---------------------------------------------------------------- behaviour cloning (imitation) on a rollout buffer
 * No reference op.  Supervised learning on the buffer's stored actions -- the action paths of a search collected by
 * ppo_collect_paths, or recorded action histories: the policy minimises
 *     -(1 / B_global) sum_i w_i log pi(a_i | s_i)  +  entropy_weight * (the entropy term of ppo_loss_with_entropy)
 * with log pi formed as a log-softmax over the actions of active quads, (l[a] - max l) - log sum exp(l - max l), so that an
 * action the current policy gives a probability that underflows to 0 still has a finite loss and gradient; the gradient is
 * (w / B_global)(p_k - [k == a]) per logit.  Every stored action must lie on an active quad (as for ppo_forward_backward).
 * weight_mode: PPO_IMITATE_UNIFORM, w = 1 (behaviour cloning); PPO_IMITATE_POSITIVE_ADVANTAGE, w = max(adv, 0) with adv the
 * column adv_mode names (self-imitation learning): PPO_ADV_RETURNS or PPO_ADV_GAE -- the latter needs a GAE call on these
 * rollouts first (PPO_ERR_ARG); the two normalised modes and an unknown weight mode are PPO_ERR_UNSUPPORTED.  adv_mode is
 * checked in both weight modes and read in the weighted one.  p_old is not read; no probability ratio is stored.
 * fp32 dtype only (a bf16-dtype policy: PPO_ERR_UNSUPPORTED), any fp32 policy shape ppo_forward_backward takes. */
#define PPO_IMITATE_UNIFORM 0
#define PPO_IMITATE_POSITIVE_ADVANTAGE 1
/* gradient only, like ppo_forward_backward (same argument checks); the two loss columns through ppo_last_losses: the
 * cross-entropy and entropy_weight * entropy loss */
int32_t ppo_imitate_forward_backward(ppo_policy_t pol, ppo_rollouts_t ro, const int64_t* sample_idx, int64_t B,
                                     int64_t B_global, double entropy_weight, int32_t weight_mode, int32_t adv_mode);
/* ppo_train's epoch loop on that objective: perm / seed / rank / world / allreduce / allreduce_ctx and the three history
 * arrays as there (ce_hist: per-epoch mean of the per-batch cross-entropies).  The policy's target_kl is not read: the
 * call never stops early, stores no ratios and leaves ppo_policy_last_train_stats what the latest ppo_train left. */
int32_t ppo_imitate_train(ppo_policy_t pol, ppo_adam_t opt, ppo_rollouts_t ro, int64_t batch_size, int32_t num_epochs,
                          double entropy_weight, int32_t weight_mode, int32_t adv_mode, const int64_t* perm, uint64_t seed,
                          int32_t rank, int32_t world, ppo_allreduce_fn allreduce, void* allreduce_ctx, double* ce_hist,
                          double* entropy_hist, double* lr_hist);

/* ---------------------------------------------------------------- policy distillation (soft targets) on a rollout buffer
 * No reference op.  Training towards a DISTRIBUTION over actions per stored state -- a wider or deeper teacher's, the behaviour
 * policy's recorded one, or rows made on the host (label smoothing): the policy minimises
 *     -(1 / B_global) sum_i w_i sum_k q'_ik log pi(k | s_i)  +  entropy_weight * (the entropy term of ppo_loss_with_entropy)
 * q' = the state's target row q on the actions of active quads and 0 elsewhere (mass on an inactive quad is ignored, never an
 * error), log pi the log-softmax of imitation above, a term with q'_k == 0 contributing exactly 0.  The gradient per logit is
 * (w / B_global)(p_k Qs - q'_k) with Qs = sum_k q'_k used as it is: rows need not sum to 1, an all-zero row leaves the entropy
 * term alone, a one-hot row is ppo_imitate_forward_backward.  Nothing divides by a probability.  The loss is the cross-entropy,
 * not the KL divergence: its floor is the targets' entropy, which the device does not compute.
 * The target column: [T][N][A] floats in ppo_rollouts_get_full_probs' layout, indexed by transition id, allocated on first use;
 * every call that writes new transitions into the buffer (the collectors, ppo_rollouts_set, a disk load) marks it not filled.
 * ppo_rollouts_fill_targets: the teacher's action probabilities (ppo_policy_forward's bits) of all T*N stored states, on the
 *   device.  Any teacher ppo_policy_forward takes on the buffer's states, bf16 dtype included; on a compact buffer (env
 *   snapshots) fp32 teachers only (a bf16 one: PPO_ERR_UNSUPPORTED).  teacher F != the buffer's F: PPO_ERR_ARG.
 * ppo_rollouts_set_targets / _get_targets: upload (every entry finite and >= 0, else PPO_ERR_ARG) and read back.
 * A buffer with a disk sink attached: PPO_ERR_UNSUPPORTED from every call of this section. */
int32_t ppo_rollouts_fill_targets(ppo_policy_t teacher, ppo_rollouts_t ro);
int32_t ppo_rollouts_set_targets(ppo_rollouts_t ro, const float* targets);
int32_t ppo_rollouts_get_targets(ppo_rollouts_t ro, float* targets_out);
/* target_source: PPO_TARGETS_COLUMN, the column above; PPO_TARGETS_RECORDED, the behaviour policy's distributions a collector
 * recorded (record_probs).  A source that is not filled / not recorded for these rollouts: PPO_ERR_ARG; an unknown one:
 * PPO_ERR_UNSUPPORTED.  weight_mode / adv_mode: as for ppo_imitate_forward_backward.  fp32 students only (a bf16-dtype policy:
 * PPO_ERR_UNSUPPORTED). */
#define PPO_TARGETS_COLUMN 0
#define PPO_TARGETS_RECORDED 1
/* gradient only, like ppo_imitate_forward_backward; the two loss columns through ppo_last_losses */
int32_t ppo_distill_forward_backward(ppo_policy_t pol, ppo_rollouts_t ro, const int64_t* sample_idx, int64_t B,
                                     int64_t B_global, double entropy_weight, int32_t weight_mode, int32_t adv_mode,
                                     int32_t target_source);
/* ppo_imitate_train's epoch loop on that objective, same permutation, rank and hook arguments and histories; never stops
 * early, stores no ratios, leaves ppo_policy_last_train_stats and ppo_policy_last_value_stats alone */
int32_t ppo_distill_train(ppo_policy_t pol, ppo_adam_t opt, ppo_rollouts_t ro, int64_t batch_size, int32_t num_epochs,
                          double entropy_weight, int32_t weight_mode, int32_t adv_mode, int32_t target_source,
                          const int64_t* perm, uint64_t seed, int32_t rank, int32_t world, ppo_allreduce_fn allreduce,
                          void* allreduce_ctx, double* ce_hist, double* entropy_hist, double* lr_hist);

/* ---------------------------------------------------------------- update statistics and target-KL early stopping
 * No reference op: the reference reports the two losses and the learning rate.  While a target_kl is set on the policy
 * handle (below; +inf = record only), every train forward stores the probability ratio r = p_new(a|s) / p_old(a|s) of
 * each state (the quotient its surrogate forms); ppo_train reduces an epoch's ratios once, in fp64 and in a fixed order,
 * and keeps per epoch
 *     approx_kl     = mean((r - 1) - log r)      (the estimator Stable-Baselines3 and CleanRL report under that name)
 *     old_approx_kl = mean(-log r)
 *     clip_fraction = mean(|r - 1| > epsilon)
 * Each transition enters with the parameters its own minibatch saw, i.e. before that minibatch's update, like there.
 * Read them with ppo_policy_last_train_stats.  With target_kl == 0 (off, the default) nothing is stored or reduced -- the
 * store costs the train forward a measurable 0.2 % -- and the three statistics read NaN; epochs_run is kept either way.
 * target_kl (a property of the policy handle): when > 0, ppo_train ends after the first epoch whose
 * approx_kl is not <= target_kl (so Inf and NaN end it); that epoch's updates stay applied, no epoch is cut short.  The
 * epoch count of the optimiser (permutation key), the ExpDecay / InvDecay counters and the history arrays advance for
 * the epochs that ran only; history entries behind them are left untouched.  +inf records without ever stopping.
 * Data parallel: with world > 1 and target_kl > 0 the four sums behind the statistics are exchanged through the hook once
 * per epoch (one more call, 12 * world floats), so every rank holds the same GLOBAL statistics and takes the same
 * decision; target_kl must then be the same on every rank, like num_epochs.  With target_kl == 0 no call is added. */
/* no reference op.  0 off; > 0 or +inf on; < 0 / NaN: PPO_ERR_ARG */
int32_t ppo_policy_set_target_kl(ppo_policy_t pol, double target_kl);
/* no reference op */
int32_t ppo_policy_get_target_kl(ppo_policy_t pol, double* target_kl);
/* no reference op.  Of the latest ppo_train on this policy: epochs_run, stopped_early (1: fewer epochs ran than were
 * asked for), and the first min(cap, epochs_run) entries of each per-epoch array (NaN for a call that ran with
 * target_kl == 0); every output may be NULL */
int32_t ppo_policy_last_train_stats(ppo_policy_t pol, int32_t cap, int32_t* epochs_run, int32_t* stopped_early,
                                    double* approx_kl, double* old_approx_kl, double* clip_fraction);

/* ---------------------------------------------------------------- KL-anchored PPO: a penalty towards target distributions
 * No reference op.  While a KL anchor is set on the policy handle, ppo_train, ppo_forward_backward and ppo_step_batch
 * (signatures unchanged) minimise
 *     ppo_loss_with_entropy  +  coef * -(1 / B_global) sum_i sum_k q'_ik log pi(k | s_i)
 * the clipped surrogate and entropy term as they are plus coef times the soft-target cross-entropy of the distillation section
 * above (q', log pi, Qs and the gradient (coef / B_global)(p_k Qs - q'_k) as stated there): the gradient of
 * coef * KL(q' || pi), whose value differs from the cross-entropy by the targets' entropy only.  q: the frozen cloned or
 * teacher policy (kickstarting / RL from a prior; source PPO_TARGETS_COLUMN, filled by ppo_rollouts_fill_targets), or the
 * behaviour policy's whole distribution at collection time (PPO's penalty form, Schulman et al. 2017, section 4; source
 * PPO_TARGETS_RECORDED).  Loss column 0 (ppo_last_losses, ppo_train's ppo_hist) is then the minimised sum, surrogate plus
 * coef * cross-entropy.  The per-state divergence kl_i = sum over q'_ik > 0 of q'_ik (log q'_ik - log pi(k | s_i)) is formed in
 * fp32 beside it; ppo_train reduces an epoch's column once (fp64, fixed order) to the mean anchor KL, every state with the
 * parameters its own minibatch saw.  coef == 0 records the divergence and leaves the gradient alone.
 * target == 0: the coefficient is fixed.  target = d > 0: behind every epoch of ppo_train whose mean anchor KL exceeds 1.5 d
 * coef doubles, below d / 1.5 it halves; the adapted value stays on the handle across calls (ppo_policy_get_kl_anchor).
 * Data parallel: the sums behind the mean are exchanged through the hook once per epoch (6 * world floats), so every rank
 * holds the global mean and the same coefficient; the anchor must be the same on every rank.
 * Errors, before anything is launched: a source not filled / not recorded for these rollouts PPO_ERR_ARG; a bf16-dtype
 * policy or a buffer with a disk sink attached PPO_ERR_UNSUPPORTED.  The fp32-MFMA train forward alone has the anchored tail:
 * while an anchor is set every minibatch size takes it.  The target_kl statistics and stop work as without an anchor. */
#define PPO_ANCHOR_OFF (-1)
/* source: PPO_ANCHOR_OFF (the default; coef and target are then ignored and read back 0), PPO_TARGETS_COLUMN or
 * PPO_TARGETS_RECORDED (another value: PPO_ERR_UNSUPPORTED); coef >= 0 and finite, target >= 0 and finite, else PPO_ERR_ARG */
int32_t ppo_policy_set_kl_anchor(ppo_policy_t pol, double coef, int32_t source, double target);
/* every output may be NULL */
int32_t ppo_policy_get_kl_anchor(ppo_policy_t pol, double* coef, int32_t* source, double* target);
/* Of the latest ppo_train on this policy that ran with an anchor: n = its epochs that ran, and the first min(cap, n) entries
 * of kl (mean anchor KL of the epoch) and coef (the coefficient the epoch ran with); every output may be NULL.  A ppo_train
 * without an anchor leaves n = 0 */
int32_t ppo_policy_last_anchor_stats(ppo_policy_t pol, int32_t cap, int32_t* n, double* kl, double* coef);

/* ---------------------------------------------------------------- critic (device state values)
 * A critic is an ordinary ppo_policy_t made by ppo_policy_create(F, hidden, L, 4) and read as a state value: the mean of
 * the 4 outputs of every half-edge row that belongs to an ACTIVE quad,
 *     V(s) = (sum over active rows r, outputs i of y[r][i]) / (4 * number of active rows),   0 when no quad is active,
 * trained with Flux.mse(V, target).  Parameters, gradient, optimiser chains and checkpoints are the policy's.  fp32 dtype
 * only (PPO_ERR_UNSUPPORTED for a bf16 critic, and for one whose F differs from the buffer's).  Data parallel through
 * ppo_value_train_dp and ppo_rollouts_value_moments_shifts; the other entry points are local to their rank. */
#define PPO_VTARGET_RETURNS 0         /* regress on the buffer's returns column                                     */
#define PPO_VTARGET_LAMBDA_RETURNS 1  /* ... on the lambda-returns adv + V of the latest GAE call on these rollouts */
/* values[b] = V(states[b]): host arrays in and out like ppo_policy_forward */
int32_t ppo_value_forward(ppo_policy_t critic, const int8_t* states, const uint32_t* active, int64_t B, int32_t H,
                          float* values);
/* fills the buffer's device values [T+1][N]: rows 0 .. T-1 are the stored states, row T the state every env is in now
 * (behind the last step).  env may be NULL -- e.g. for a buffer made by ppo_rollouts_create_shape -- and row T is then
 * all zeros: the caller bootstraps from 0.  Optional host copy. */
int32_t ppo_rollouts_compute_values(ppo_rollouts_t ro, ppo_env_t env_or_null, ppo_policy_t critic, float* values_out_or_null);
/* ppo_rollouts_compute_values + the scan of ppo_rollouts_compute_gae, nothing crossing to the host unless an output is
 * asked for; ppo_train(..., PPO_ADV_GAE*) works after it */
int32_t ppo_rollouts_compute_gae_critic(ppo_rollouts_t ro, ppo_env_t env_or_null, ppo_policy_t critic, double gamma,
                                        double lambda, float* adv_out_or_null, float* lambda_returns_out_or_null);
/* the same with time-limit truncations bootstrapped: ppo_rollouts_compute_values, then ppo_rollouts_truncated's replay,
 * one critic forward over the K final states, their values scattered into the boot column, and the scan of
 * ppo_gae_boot_tn.  One 8-byte count (K, also to n_truncated_out) crosses to the host; no state or value column does
 * unless an output is asked for.  The returns column (PPO_VTARGET_RETURNS) is not bootstrapped.  A buffer without an env
 * template: PPO_ERR_UNSUPPORTED (use ppo_rollouts_compute_gae_boot with final values of your own) */
int32_t ppo_rollouts_compute_gae_critic_boot(ppo_rollouts_t ro, ppo_env_t env_or_null, ppo_policy_t critic, double gamma,
                                             double lambda, float* adv_out_or_null, float* lambda_returns_out_or_null,
                                             int64_t* n_truncated_out_or_null);
/* forward + mse + backward of one minibatch (sample_idx as in ppo_forward_backward): the flat gradient of
 * sum_b (V(s_b) - target_b)^2 / B_global goes to the critic's gradient buffer (ppo_policy_get_grad), that loss to
 * loss_out (optional).  target: PPO_VTARGET_*; lambda-returns need a GAE call on these rollouts first (PPO_ERR_ARG). */
int32_t ppo_value_forward_backward(ppo_policy_t critic, ppo_rollouts_t ro, const int64_t* sample_idx, int64_t B,
                                   int64_t B_global, int32_t target, double* loss_out_or_null);
/* the epoch loop of ppo_train for the critic: perm / seed, slices of batch_size with a short last one, mse_hist[ep] =
 * unweighted mean of the per-batch losses, lr_hist from the chain.  opt: any optimiser made for `critic`. */
int32_t ppo_value_train(ppo_policy_t critic, ppo_adam_t opt, ppo_rollouts_t ro, int64_t batch_size, int32_t num_epochs,
                        int32_t target, const int64_t* perm, uint64_t seed, double* mse_hist, double* lr_hist);
/* ppo_value_train across data-parallel ranks: rank / world / allreduce / allreduce_ctx as in ppo_train, with the same
 * shard-length exchange, union minibatches, zero gradient from an exhausted shard and batch_size held against the
 * shortest shard on every rank alike.  Every rank keeps a replica of the critic and of its optimiser; after the call the
 * replicas are bit-identical and mse_hist is the GLOBAL history (each step's loss is the mean over the samples all ranks
 * contributed to it).  ppo_value_train is this call with (0, 1, NULL, NULL).  While a value_clip is set and world > 1,
 * the three sums behind the value-clip statistics are exchanged through the hook once per epoch (one more call,
 * 9 * world floats) and added in rank order, so ppo_policy_last_value_stats is the same on every rank; value_clip must
 * then be the same on every rank, like target_kl and num_epochs. */
int32_t ppo_value_train_dp(ppo_policy_t critic, ppo_adam_t opt, ppo_rollouts_t ro, int64_t batch_size, int32_t num_epochs,
                           int32_t target, const int64_t* perm, uint64_t seed, int32_t rank, int32_t world,
                           ppo_allreduce_fn allreduce, void* allreduce_ctx, double* mse_hist, double* lr_hist);
/* no reference op.  The sums behind the critic's explained variance, over the valid transitions of the buffer, with V =
 * rows 0 .. T-1 of the buffer's device values (ppo_rollouts_compute_values / _gae / _gae_critic first: PPO_ERR_ARG
 * otherwise) and t = the PPO_VTARGET_* column: sums5 = n, sum x, sum x^2, sum y, sum y^2 in fp64 and a fixed order, where
 * x = t - t0 and y = (t - V) - (t0 - V0) are taken relative to the first transition of the dataset (ppo_rollouts_get_index)
 * so that a variance is not a difference of large numbers.  Explained variance = 1 - Var(y) / Var(x) with
 * Var(z) = sum z^2 / n - (sum z / n)^2, NaN when Var(x) == 0. */
int32_t ppo_rollouts_value_moments(ppo_rollouts_t ro, int32_t target, double* sums5);
/* no reference op.  ppo_rollouts_value_moments plus the two shifts its sums are relative to: shifts2 = t0, t0 - V0 (each
 * from the two floats the reduction read).  Sums of different buffers have different shifts and cannot be added; with the
 * shifts each buffer gives its own n, mean and sum of squared deviations of t and of t - V, which merge exactly
 * (data-parallel shards: explained_variance_from_shards in the Python package). */
int32_t ppo_rollouts_value_moments_shifts(ppo_rollouts_t ro, int32_t target, double* sums5, double* shifts2);

/* ---------------------------------------------------------------- critic: PPO-clipped value loss
 * No reference op: the value half of PPO's trust region (PPO2, CleanRL, Stable-Baselines3 clip_range_vf).  While a
 * value_clip c is set on the critic handle, ppo_value_forward_backward and ppo_value_train minimise, instead of the mse,
 *     sum_b max((V_b - t_b)^2, (Vclip_b - t_b)^2) / B_global,    Vclip = Vold + clamp(V - Vold, -c, c)
 * (no factor 1/2: it continues Flux.mse), where Vold is the buffer's device value of that transition -- rows 0 .. T-1 of
 * what ppo_rollouts_compute_values / _gae / _gae_critic left there, i.e. the values the critic had before the update.
 * In fp32, with c = (float)value_clip: delta = V - Vold; a state is inside when |delta| <= c (decided on delta itself);
 * outside, Vclip = Vold + copysign(c, delta), and the unclipped square is kept when |V - t| >= |Vclip - t| (a tie keeps it).
 * A state whose clipped square is the larger one contributes (Vclip - t)^2 to the loss and exactly 0 to the gradient.
 * value_clip: 0 = off (the default: gradients, losses and parameters are bit for bit those of the mse; nothing is
 * allocated, stored, launched or copied), > 0 on, +inf = record the statistics and never clip (every state is inside: the
 * mse bit for bit); negative or NaN: PPO_ERR_ARG.  A clip set on a buffer whose values are missing or stale (a collection
 * since) is refused by both entry points before anything is launched: PPO_ERR_ARG, "value clipping needs
 * ppo_rollouts_compute_values or ppo_rollouts_compute_gae on these rollouts first".
 * Statistics: while the clip is set, ppo_value_train reduces every epoch's delta once, in fp64 and in a fixed order, to
 *     clip_fraction  = mean(|delta| > c)
 *     mean_sq_change = mean(delta^2)
 * each transition entering with the parameters its own minibatch saw.  ppo_value_forward_backward applies the clip and
 * stores no statistics.  Across data-parallel ranks: ppo_value_train_dp.  Not persisted in checkpoints (like target_kl). */
/* no reference op.  0 off; > 0 or +inf on; < 0 / NaN: PPO_ERR_ARG */
int32_t ppo_policy_set_value_clip(ppo_policy_t critic, double clip);
/* no reference op */
int32_t ppo_policy_get_value_clip(ppo_policy_t critic, double* clip);
/* no reference op.  Of the latest ppo_value_train on this handle: epochs_run and the first min(cap, epochs_run) entries
 * of each per-epoch array (NaN for a call that ran with the clip off); every output may be NULL */
int32_t ppo_policy_last_value_stats(ppo_policy_t critic, int32_t cap, int32_t* epochs_run, double* clip_fraction,
                                    double* mean_sq_change);

/* Native hook (the default of bench.py and DataParallel): the same all-reduce as ONE RCCL call made by the library
 * itself on the engine's stream -- no host-language callback per optimiser step.  RCCL is resolved with dlopen at first
 * use (a host that already carries an RCCL, e.g. torch, shares its copy).  The engine owns no rendezvous: the host
 * distributes the 128-byte unique id between its ranks (rank 0 calls ppo_rccl_unique_id, every rank ppo_rccl_init
 * after ppo_device_init), runs ppo_rccl_self_test collectively, and passes ppo_rccl_allreduce as the `allreduce`
 * argument of ppo_train.  Replaces, on the reference side, nothing: the reference is single-process. */
int32_t ppo_rccl_probe(void);                      /* local: can librccl be resolved?  agree on it before ppo_rccl_init */
int32_t ppo_rccl_unique_id(uint8_t* out128);
int32_t ppo_rccl_init(int32_t rank, int32_t world, const uint8_t* id128);
int32_t ppo_rccl_allreduce(void* ctx, void* grad_dev, int64_t n_floats);      /* a ppo_allreduce_fn */
int32_t ppo_rccl_comm_info(int32_t* rank, int32_t* world);                    /* as the communicator reports them */
int32_t ppo_rccl_self_test(int32_t* ok);                                      /* collective: known-answer all-reduce */
int32_t ppo_rccl_finalize(void);

/* ---------------------------------------------------------------- out-of-core rollout store
 * DiskRollouts / DiskDataset (src/rollouts_to_disk.jl:1-171, src/dataset.jl:1-82) for rollouts that should not
 * stay resident: while ppo_collect_rollouts runs, every finished step [N] is copied device -> pinned host with
 * hipMemcpyAsync on a copy stream (ordered by events, overlapping the next step's kernels) and a writer thread
 * appends it to <dir>/rollout.bin; the returns column is appended when the scan has run (the reference rewrites
 * trajectory.csv at the same point, :106-132).  One fixed-size binary shard instead of one BSON file per state;
 * the reference's CSV + per-state BSON layout is produced by the host-side exporter for small runs.
 * attach wipes and recreates <dir> like the DiskRollouts constructor (:7-13,23-45). */
int32_t ppo_rollouts_attach_disk(ppo_rollouts_t ro, const char* dir, int32_t pinned_slots);
int32_t ppo_rollouts_detach_disk(ppo_rollouts_t ro);
/* Deferred finish of a streamed collection.  ppo_set_disk_async(1) (PPO_DISK_ASYNC=1; default 0): the pinned ring is sized to
 * hold EVERY step of the collection (up to PPO_DISK_ASYNC_MAX_BYTES, default 1 GiB), ppo_collect_rollouts returns as soon as the
 * last step and the returns column are on the copy stream, and the writer thread finishes <dir>/rollout.bin on its own while
 * the caller trains on the columns that stayed in HBM.  The file is complete when ppo_rollouts_disk_sync returns (the next
 * collection into the same buffer, detach and destroy wait for it too).  With mode 0 the file is complete when
 * ppo_collect_rollouts returns, as before (the reference's rollouts_to_disk is synchronous: src/rollouts_to_disk.jl:73-132). */
int32_t ppo_set_disk_async(int32_t mode);
/* the mode in force (0 / 1), whether it came from ppo_set_disk_async or from PPO_DISK_ASYNC at load */
int32_t ppo_get_disk_async(int32_t* mode);
int32_t ppo_rollouts_disk_sync(ppo_rollouts_t ro);
/* Write failures (disk full, file size limit, I/O error) are host errors; each is reported exactly once, as PPO_ERR_ARG with
 * a ppo_last_error that names the write.
 *   mode 0: ppo_collect_rollouts itself fails -- for a record, for the returns column, and for the tail of the returns column
 *           that the stream only writes when the file is closed.
 *   mode 1: ppo_collect_rollouts may have returned PPO_OK already.  The failure is then reported by the FIRST wait point that
 *           follows: ppo_rollouts_disk_sync, ppo_rollouts_detach_disk (the sink is detached all the same), a second
 *           ppo_rollouts_attach_disk, or the next ppo_collect_rollouts into the same attached buffer, which reports the previous
 *           file's failure and starts nothing (no env step, no new file); the call after it runs normally.
 *           ppo_rollouts_destroy has no status for it: it waits, leaves ppo_last_error set, and never blocks on a failed writer.
 * What is left on disk: a reported failure unlinks <dir>/rollout.bin, so the directory never yields a dataset
 * (ppo_rollouts_load_disk: "trajectory file missing").  The buffer's columns in HBM are complete and usable, the pinned
 * records return to the pool, and the next collection -- into this sink or a fresh one -- is unaffected. */
/* DiskDataset: read <dir>/rollout.bin back into the (device) rollout buffer; shapes must match the env it was
 * created for.  All transitions are valid afterwards. */
int32_t ppo_rollouts_load_disk(ppo_rollouts_t ro, const char* dir);

/* average_returns(policy, env, num_trajectories) -> (mean, sample std [n-1]) of the UNdiscounted episode return
 *                                                          src/evaluate.jl:1-25
 * exactly num_trajectories whole episodes, trajectory e on resident env e mod N (reset! before each, stochastic policy);
 * `scratch` is a rollout buffer created for this env (its contents are overwritten). */
int32_t ppo_average_returns(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                            double* mean, double* std);

/* Evaluator variants (test/quad_game_utilities.jl:280-307,369-387), same trajectory-to-env assignment as
 * ppo_average_returns.  env.current_score of the synthetic env = sum of |vertex score| over the active quads,
 * env.opt_score = |sum of vertex scores| (the two numbers its termination test compares).
 *   average_best_returns:       mean / sample std of  initial_score - min(score seen on the trajectory)      :280-307
 *   average_normalized_returns: the same divided by maxreturn = initial_score - opt_score; a trajectory whose
 *                               maxreturn is 0 counts 1.0 and is NOT played (:369-378)                        :369-387
 * ppo_evaluate_trajectories returns the per-trajectory values themselves (kind 1 = single_trajectory_return
 * src/evaluate.jl:1-16, 2 = best_single_trajectory_return, 3 = single_trajectory_normalized_return), env-major:
 * env n's trajectories (e = n, n + N, ...) are consecutive. */
int32_t ppo_average_best_returns(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                                 double* mean, double* std);
int32_t ppo_average_normalized_returns(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch,
                                       int64_t num_trajectories, double* mean, double* std);
int32_t ppo_evaluate_trajectories(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                                  int32_t kind, double* values);

/* best_state_in_rollout(wrapper, policy)                     test/quad_game_utilities.jl:341-358
 * One stochastic trajectory per slot; the state (start included) at argmin(current_score - opt_score) comes back: the FIRST
 * minimum, like Julia's argmin.  Per trajectory: best_state [2V] = score[V] then degree[V], best_active, best_gap, best_step
 * (steps played when it was reached; 0 = the start), length, initial_gap; optional trace [max_actions] = initial_score -
 * current_score behind every step (single_trajectory_scores :309-323; INT32_MIN behind the trajectory's end) and
 * type_counts [4] = actions played by type a % 4 (count_non_flips, test/random_quad.jl:9-27, is types 2 and 3).
 *   reset_first = 1: the average_best_returns convention -- trajectory e on env e mod N, reset! before each, env-major output.
 *   reset_first = 0: num_trajectories <= N; env n < num_trajectories plays one trajectory from the state it holds, no reset!
 *                    runs and no episode counter is consumed; an env that is already terminal is PPO_ERR_ARG. */
int32_t ppo_best_states(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                        int32_t reset_first, int8_t* best_state, uint32_t* best_active, int32_t* best_gap,
                        int32_t* best_step, int32_t* length, int32_t* initial_gap, int32_t* trace_or_null,
                        int32_t* type_counts_or_null);
/* Best of K trajectories from each of num_starts caller-supplied states (score, degree [num_starts][V], active
 * [num_starts], checked like ppo_env_set_internal), 1 <= K <= N.  Sampling is keyed on (global env id, tick), so the K envs
 * loaded with one start play K different trajectories.  Rounds of N / K starts: env n of a round holds start n / K as clone
 * n % K, the envs behind them idle (their ticks do not move).  Per start: the winner's best_state [2V], best_active,
 * best_gap, best_clone, best_step, initial_gap; ties go to the lowest clone, then that clone's first minimum.  Optional
 * clone_gaps [num_starts][K]: every clone's best gap.  No reset! runs: episode counters are unchanged, ticks advance by the
 * steps each env played, the envs that played are left terminal. */
int32_t ppo_search_best_states(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                               const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                               uint32_t* best_active, int32_t* best_gap, int32_t* best_clone, int32_t* best_step,
                               int32_t* initial_gap, int32_t* clone_gaps_or_null);
/* Resampling search: ppo_search_best_states' schedule (rounds of N / K starts, clone n % K of start n / K on env n, no
 * reset!, ticks advance by the steps played) with a resample event behind every interval-th loop step t of a round (t %
 * interval == 0, t < max_actions), for every start of the round:
 *   fold  the clone with the lowest (record best_gap, clone) of all K: its record (best_state, best_active, best_gap,
 *         best_step, initial_gap) becomes the start's result on the start's first fold, later only on a strictly lower gap;
 *   rank  the live clones (not terminal) ascending by (current_score - opt_score of the state held now, clone); the first
 *         m = min(survivors, live) keep their state;
 *   copy  the clone of rank r >= m takes score, degree, active, steps, reward, its whole record and its step count from the
 *         clone of rank (r - m) % m; tick, episode and done stay its own, so the copies diverge at the next step.
 * One more fold runs behind the round's last step.  best_step counts loop steps along the lineage.  clone_gaps (optional):
 * every clone's record gap at that last fold.  donors (optional) [num_starts][E][K], E = (max_actions - 1) / interval: the
 * donor clone of a receiver, -1 for a live clone that kept its state, -2 for a terminal clone and for every clone of an
 * event that did not run because the round had finished.  interval >= max_actions runs no event: ppo_search_best_states.
 * interval < 1 or survivors outside 1 .. K: PPO_ERR_ARG; K > 4096: PPO_ERR_UNSUPPORTED. */
int32_t ppo_search_resample_states(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                                   const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                                   uint32_t* best_active, int32_t* best_gap, int32_t* best_clone, int32_t* best_step,
                                   int32_t* initial_gap, int32_t* clone_gaps_or_null, int64_t interval, int64_t survivors,
                                   int32_t* donors_or_null);

/* The action path to the best state.  A best state is a snapshot of the built-in env; what a caller who holds a real mesh
 * next to it needs is the SEQUENCE OF ACTIONS that leads there (the reference's step!(wrapper, quad, edge, type) and
 * plot_trajectory replay actions onto a mesh).  The three calls above, each with one more output of 0-based int16 action
 * indices (an index is below 16 Q <= 512); every other argument and result is the plain call's:
 *   ppo_best_states_actions           actions [num_trajectories][max_actions]: the whole trajectory, -1 behind `length`; its
 *                                     first best_step entries lead from the trajectory's start to best_state;
 *   ppo_search_best_states_path       path [num_starts][max_actions]: the winner's first best_step actions, -1 behind them;
 *   ppo_search_resample_states_path   path [num_starts][max_actions], likewise.  The action history belongs to the LINEAGE:
 *                                     a receiver takes the donor's played prefix together with its record and step count,
 *                                     and a fold that takes a winner's record takes the first best_step entries of that
 *                                     winner's history with it.  best_step counts steps along the lineage, so the path has
 *                                     best_step entries.
 * In every case ppo_env_apply_paths(start, path) gives best_state, best_active and best_gap, with applied == best_step. */
int32_t ppo_best_states_actions(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                                int32_t reset_first, int8_t* best_state, uint32_t* best_active, int32_t* best_gap,
                                int32_t* best_step, int32_t* length, int32_t* initial_gap, int32_t* trace_or_null,
                                int32_t* type_counts_or_null, int16_t* actions);
int32_t ppo_search_best_states_path(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                                    const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                                    uint32_t* best_active, int32_t* best_gap, int32_t* best_clone, int32_t* best_step,
                                    int32_t* initial_gap, int32_t* clone_gaps_or_null, int16_t* path);
int32_t ppo_search_resample_states_path(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                                        const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                                        uint32_t* best_active, int32_t* best_gap, int32_t* best_clone, int32_t* best_step,
                                        int32_t* initial_gap, int32_t* clone_gaps_or_null, int64_t interval, int64_t survivors,
                                        int32_t* donors_or_null, int16_t* path);
/* ppo_search_resample_states ranking by the critic's value.  `critic` is a ppo_policy_t read as a state value
 * (ppo_value_forward).  The env's reward is old_total - new_total, so a trained critic estimates the score reduction still to
 * come and cur_gap - V(s) where a clone will end.  In front of every event the envs are observed and the critic's forward
 * runs on the device; a live clone then ranks by the fp32 number
 *     s = fmaf(-(float)value_weight, v, (float)cur_gap),   v = V(state the clone holds behind the step), 0 if not finite,
 * ascending, -0.0 before +0.0, ties to the lower clone.  Everything else -- the fold (by the record's real best_gap), terminal
 * clones, m = min(survivors, live), the donor of rank r being rank (r - m) % m, the copy, the path -- is the plain call's;
 * value_weight = 0 is the plain call.  event_values (optional) [num_starts][E][K] float: the raw v a live clone was ranked
 * with, NaN for a terminal clone and for every clone of an event that did not run.  path may be null.  PPO_ERR_UNSUPPORTED:
 * a bf16-dtype critic, a critic whose input width is not the env's F; PPO_ERR_ARG: value_weight negative, not finite or
 * above FLT_MAX. */
int32_t ppo_search_resample_states_value(ppo_policy_t pol, ppo_policy_t critic, ppo_env_t env, ppo_rollouts_t scratch,
                                         int64_t num_starts, int64_t K, const int8_t* score, const int8_t* degree,
                                         const uint32_t* active, int8_t* best_state, uint32_t* best_active, int32_t* best_gap,
                                         int32_t* best_clone, int32_t* best_step, int32_t* initial_gap,
                                         int32_t* clone_gaps_or_null, int64_t interval, int64_t survivors, double value_weight,
                                         int32_t* donors_or_null, float* event_values_or_null, int16_t* path_or_null);
/* Beam search (no reference op): the K action sequences from each start to which the policy gives the highest
 * probability, deterministic and seed-free; K = 1 is the greedy trajectory.  Starts as for ppo_search_best_states, 1 <= K <= N,
 * rounds of S = N / K starts; start s of a round owns resident envs s*K .. s*K + K - 1, its slots.  A slot carries a live flag
 * and a weight (m, e), m an fp64 in [0.5, 1), e an int32, standing for the path probability m * 2^e.  Load: all K envs hold the
 * start's state, slot 0 is live with (0.5, 1), the others are dead.  Step t = 0 .. max_actions - 1 of an unfinished start:
 *   probabilities  p[slot][a], fp32: ppo_policy_forward's launcher on the states the envs hold (selection and truncation of
 *                  the handle are not read);
 *   candidates     every (k, a) with slot k live and p[k][a] > 0; x = m_k * (double)p[k][a], ONE IEEE fp64 multiply;
 *                  (m', d) = frexp(x), e' = e_k + d.  Nothing else rounds;
 *   select         candidates ordered by e' descending, then m' descending, then k*A + a ascending; the first
 *                  n = min(K, #candidates): rank j becomes slot j with parent k, action a, weight (m', e'); slots n .. K-1 die;
 *   expand         slot j takes score, degree, active and steps its parent held in front of the step, then plays its action
 *                  with the env's own step (a no-op action included);
 *   fold           the start's result (gap, state, step, slot) is the load state with step 0, slot 0, until some live slot's
 *                  gap = current_score - opt_score is STRICTLY below it: then the lowest (gap, slot) of the step, with
 *                  best_step = t + 1, best_beam = slot;
 *   finish         the result's gap is 0, or t + 1 == max_actions.  The start's slots then idle.
 * Per start: best_state [2V], best_active, best_gap, best_beam, best_step, initial_gap, and best_mant / best_exp, the weight
 * of the slot the result was taken from ((0.5, 1) for step 0).  Optional: path [num_starts][max_actions] int16, the best_step
 * 0-based actions to best_state and -1 behind them, walked on the host from the back-pointer log; log_parent, log_action
 * [num_starts][max_actions][K] int16, per step and slot, -1 for a dead slot and for a step that did not run; log_mant (fp64)
 * and log_exp (int32), the slots' weights, 0 where the others hold -1.  A log is kept on the device only where an output is
 * made of it: path, log_parent or log_action cost 4 * num_starts * max_actions * K bytes there (and as much on the host while
 * the path is walked), log_mant 8 and log_exp 4 bytes per entry; with all five null no log exists.  ppo_env_apply_paths(start, path) gives best_state,
 * best_active and best_gap with applied == best_step.  No reset! runs and no random number is drawn: tick and episode counters
 * of every env are unchanged; the slots' envs are left terminal; envs at and beyond S*K are untouched.
 * PPO_ERR_ARG: K < 1, K > N, a bad start.  PPO_ERR_UNSUPPORTED: a bf16-dtype policy, H other than 32 / 128, K > 256 (the
 * chosen keys and the weights are staged in LDS, one thread per slot). */
int32_t ppo_beam_search_states(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                               const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                               uint32_t* best_active, int32_t* best_gap, int32_t* best_beam, int32_t* best_step,
                               int32_t* initial_gap, double* best_mant, int32_t* best_exp, int16_t* path_or_null,
                               int16_t* log_parent_or_null, int16_t* log_action_or_null, double* log_mant_or_null,
                               int32_t* log_exp_or_null);
/* The distinct beam: ppo_beam_search_states with its select and expand replaced by a walk that keeps K
 * DIFFERENT states per step.  distinct_mode 0 is ppo_beam_search_states itself (rounds is not read, log_rank and examined must
 * be null); 1 "children", 2 "parents".  A state's identity is the bytes of score[V], degree[V] and the active word.  The seen
 * set of a step is empty in mode 1 and holds the states of the live slots in front of the step in mode 2.  The candidates
 * are taken in ppo_beam_search_states' order, at most B = 256 * rounds of them; examining (k, a) forms the child (slot k's
 * state in front of the step after the env's own step with a, a no-op included); a child whose state is in the seen set is
 * rejected, any other becomes slot j = the number accepted so far with parent k, action a and its own weight (m', e') -- the
 * probabilities of rejected paths are not added to it -- and joins the seen set.  The walk stops at K accepted, at the end of
 * the candidates or at B examined; slots n .. K-1 are dead.  Fold and finish as in ppo_beam_search_states, the finish also
 * when nothing was accepted (the result stands as it is).  Outputs as there; additionally log_rank [num_starts][max_actions][K]
 * int32, the 0-based position of the slot's candidate in the step's order (-1: a dead slot, a step that did not run), and
 * examined [num_starts][max_actions] int32, the candidates the walk looked at: the last accepted rank + 1 if it stopped at K,
 * otherwise min(#candidates, B); -1 for a step that did not run.
 * PPO_ERR_ARG: distinct_mode outside 0 .. 2, rounds outside 1 .. 16 in modes 1 and 2, a rank or examined output in mode 0;
 * everything else as ppo_beam_search_states. */
int32_t ppo_beam_search_states_distinct(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                                        const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                                        uint32_t* best_active, int32_t* best_gap, int32_t* best_beam, int32_t* best_step,
                                        int32_t* initial_gap, double* best_mant, int32_t* best_exp, int16_t* path_or_null,
                                        int16_t* log_parent_or_null, int16_t* log_action_or_null, double* log_mant_or_null,
                                        int32_t* log_exp_or_null, int32_t distinct_mode, int32_t rounds,
                                        int32_t* log_rank_or_null, int32_t* examined_or_null);
/* Teacher-forced replay without a policy: path m of paths [M][stride] (0-based actions; an entry < 0 ends a path) is
 * applied to start m (score, degree [M][V], active [M], checked like ppo_env_set_internal), which begins as reset! leaves an
 * env (steps = 0, not terminal).  A path ends at its first entry < 0, after stride entries, or once the state is terminal
 * (the optimum reached, or max_actions steps), whichever comes first.  Per path: out_state [2V] = score[V] then degree[V],
 * out_active, out_gap = current_score - opt_score of that state, applied = the actions stepped; optional trace [M][stride] =
 * initial_score - current_score behind every step, INT32_MIN behind `applied`.  The env handle supplies Q, max_actions and
 * no_action_reward only: the resident envs, their ticks, episode counters and error flags are unchanged.  PPO_ERR_ARG before
 * anything runs: a bad start, an entry >= 16 Q, stride < 1.  PPO_ERR_DEVICE_FLAG, the outputs filled: an action on an
 * inactive quad (the step counts and changes nothing, as step! does). */
int32_t ppo_env_apply_paths(ppo_env_t env, int64_t M, const int8_t* score, const int8_t* degree, const uint32_t* active,
                            const int16_t* paths, int64_t stride, int8_t* out_state, uint32_t* out_active, int32_t* out_gap,
                            int32_t* applied, int32_t* trace_or_null);

/* Teacher-forced collection: the collector that plays GIVEN actions instead of sampled ones and leaves an
 * ordinary rollout buffer behind, so that the paths of a search (or recorded action histories) can be trained on without a
 * host replay.  Starts and paths as for ppo_env_apply_paths: path m of paths [M][stride] (0-based; its declared length is
 * the index of its first entry < 0, at most stride) on start m, 1 <= M <= N.  Resident envs 0 .. M - 1 are loaded with the
 * starts as reset! leaves an env; the loop of ppo_collect_rollouts_episodes then runs T = max(1, longest declared length)
 * steps: observe, (snapshot,) the policy forward WITHOUT sampling -- p_sel = the probability the policy gives the path's
 * action in the state in front of the step --, step!.  Env n idles at step t (valid 0, reward 0, done 1, untouched) when
 * n >= M, t is at or behind its path's declared length, or it is terminal.  terminal = is_terminal OR "the path's last
 * entry": every path is a whole episode for the return scan and GAE, and a path cut short of the optimum is a truncation
 * for ppo_rollouts_compute_gae_critic_boot, which then bootstraps from the critic's value of the state it was cut in.
 * Storage form (compact / expanded), index (env-major, valid transitions only), length and returns as the episodes form
 * leaves them; record_probs as ppo_collect_rollouts.  The envs that played keep the states their paths ended in, their
 * ticks advanced by the steps played, their episode counters unchanged; the other envs and the env's flag word are
 * untouched.  PPO_ERR_ARG before anything runs: M < 1, M > N, stride < 1, a bad start, an entry >= 16 Q.
 * PPO_ERR_UNSUPPORTED: a bf16-dtype policy, a disk sink attached to ro, H other than 32 / 128.  PPO_ERR_DEVICE_FLAG, the
 * buffer filled: an action on an inactive quad -- played and penalised as step! does, recorded with valid = 0 and
 * p_sel = 0, so it is in no dataset (the forward reports it in bit 64 of the call's flag word, the step in bit 1). */
int32_t ppo_collect_paths(ppo_rollouts_t ro, ppo_env_t env, ppo_policy_t pol, int64_t M, const int8_t* score,
                          const int8_t* degree, const uint32_t* active, const int16_t* paths, int64_t stride,
                          double discount, int32_t discount_is_f32, int32_t record_probs);

/* Action selection of the calls that APPLY a policy (no reference op).  A policy handle carries a selection
 * (rule, temperature), default (PPO_SELECT_SAMPLE, 1.0), which is what every call did before the setter existed.  Per step, on
 * the logits l the forward holds in front of its softmax:
 *     inv = (float)(1.0 / temperature);  l' = l * inv (one fp32 multiply per logit);  p = the masked softmax of l';
 *     PPO_SELECT_SAMPLE: a = rand(Categorical(p)), the same inverse-CDF walk on the same Philox uniform of (global env id, tick);
 *     PPO_SELECT_GREEDY: a = argmax(p), the LOWEST action index among the largest p (Julia's argmax); no random number is drawn;
 *     p_sel = p[a], the tempered probability.
 * Greedy with temperature != 1 is allowed and is defined on the tempered p.  Ticks and episode counters move as they always do.
 * READ by: ppo_average_returns / _best_returns / _normalized_returns, ppo_evaluate_trajectories, ppo_best_states(_actions),
 * ppo_search_best_states(_path), ppo_search_resample_states(_path, _value).  (With a non-default selection ppo_average_returns
 * is the mean / std of ppo_evaluate_trajectories kind 1, the same statistic.)
 * NOT READ by: ppo_collect_rollouts, _episodes, _steps, ppo_collect_paths, ppo_policy_forward and every training call -- a
 * rollout buffer's p_old must be the probability under the distribution the training pass differentiates, which is the
 * untempered softmax.
 * PPO_ERR_ARG: an unknown rule; a temperature that is NaN, infinite or <= 0.  The setter makes no device call.  A bf16-dtype
 * policy keeps the default only: a reading call returns PPO_ERR_UNSUPPORTED while another selection is set. */
#define PPO_SELECT_SAMPLE 0
#define PPO_SELECT_GREEDY 1
int32_t ppo_policy_set_selection(ppo_policy_t pol, int32_t rule, double temperature);
int32_t ppo_policy_get_selection(ppo_policy_t pol, int32_t* rule, double* temperature);

/* Truncation of the distribution that PPO_SELECT_SAMPLE draws from: top-k and nucleus (no reference op).  A policy
 * handle carries a truncation (top_k, top_p), default (0, 1.0), separate from the selection and composing with it.  Per step, on
 * the tempered masked softmax p of the selection above (A entries):
 *     b precedes a  iff  p[b] > p[a] || (p[b] == p[a] && b < a)      -- equal probabilities rank by the lower index, like greedy;
 *     rank(a) = the number of b that precede a;  mass_before(a) = the fp32 sum of their p[b], added one by one in ascending b;
 *     keep(a) = (top_k == 0 || rank(a) < top_k) && (top_p == 1.0f || mass_before(a) < (float)top_p);
 *     q = keep ? p : 0;  S' = the sum of q in the softmax's own order;  p'' = q / S' (one fp32 division per entry);
 *     a = rand(Categorical(p'')) by the same walk on the same Philox uniform;  p_sel = p''[a].
 * The arg-max has rank 0 and mass 0 and is always kept; top_k = 1 plays greedy's action with p_sel = 1.  Any non-default
 * truncation renormalises, also one that keeps everything (top_k >= A).  top_p = 1 skips the mass test; it does not test
 * mass_before < 1.  PPO_SELECT_GREEDY ignores the truncation: every truncation keeps the arg-max.
 * READ by the calls that read the selection, NOT READ by the others: ppo_collect_rollouts, _episodes, _steps,
 * ppo_collect_paths, ppo_policy_forward and every training call never see it, for the selection's reason.
 * PPO_ERR_ARG: top_k < 0; top_p NaN, <= 0 or > 1 (judged before the handle).  The setter makes no device call.  A bf16-dtype
 * policy keeps the default only: a reading call returns PPO_ERR_UNSUPPORTED while another truncation is set. */
int32_t ppo_policy_set_truncation(ppo_policy_t pol, int32_t top_k, double top_p);
int32_t ppo_policy_get_truncation(ppo_policy_t pol, int32_t* top_k, double* top_p);

/* timing of the dominant kernels of the last ppo_train / ppo_collect_rollouts call, measured with
 * HIP events on the engine's stream (bench.py roofline leg) */
/* measurement helper: run the return scan `iters` times on device-resident synthetic [T,N] columns (no host
 * copies in the timed region) and report the average kernel time (HIP events).  K6 roofline leg of bench.py. */
int32_t ppo_profile_returns(int64_t T, int64_t N, double discount, int32_t iters, double* avg_ms);
int32_t ppo_profile_gae(int64_t T, int64_t N, double gamma, double lambda, int32_t iters, double* avg_ms);
int32_t ppo_profile_enable(int32_t on);
int32_t ppo_profile_get(const char* kernel_name, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif
