# ProximalPolicyOptimizationHIP.jl -- reference-side binding of libppo_hip.so (include/ppo_hip.h).
#
# UNTESTED AT RUN TIME: the build container has no `julia` binary (SURVEY.md 8(c)), so this file has never been
# executed.  What IS checked, on every test run, is its C boundary: tests/test_abi.py parses every `ccall` below and
# compares symbol, arity and argument types with include/ppo_hip.h.  It is the binding a maintainer of
# ProximalPolicyOptimization.jl would add: methods of the package's own generic functions
# (src/ProximalPolicyOptimization.jl:16-30) for GPU-resident types, each a thin `ccall`; the Python mirror
# (proximalpolicyoptimization.jl_amd/__init__.py) is the executed twin of this file.
module ProximalPolicyOptimizationHIP

using ProximalPolicyOptimization
import Flux
using Printf
const PPO = ProximalPolicyOptimization
const LIB = get(ENV, "PPO_HIP_LIB", "libppo_hip.so")

function check(status::Int32)
    status == 0 && return
    buf = Vector{UInt8}(undef, 1024)
    ccall((:ppo_last_error, LIB), Int32, (Ptr{UInt8}, Int64), buf, 1024)
    msg = unsafe_string(pointer(buf))
    startswith(msg, "AssertionError") ? throw(AssertionError(msg)) : error(msg)
end

# Seed of the device-side minibatch permutations (the stand-in for randperm, src/train.jl:93).  The reference never
# seeds its RNG; here runs are reproducible by default and `set_seed!` changes the stream.  The optimiser handle
# counts the epochs it has trained, so successive ppo_train! calls draw different permutations from one seed.
const SEED = Ref{UInt64}(0)
set_seed!(s::Integer) = (SEED[] = UInt64(s))

# ---------------------------------------------------------------- handles
mutable struct HipVecEnv
    h::Ptr{Cvoid}; N::Int; Q::Int; H::Int; F::Int; A::Int; max_actions::Int
    function HipVecEnv(num_envs; Q = 8, max_actions = 128, no_action_reward = -4f0, seed = 1234, global_offset = 0)
        r = Ref{Ptr{Cvoid}}()
        check(ccall((:ppo_env_create, LIB), Int32, (Int32, Int64, Int64, Int32, Int32, Float32, UInt64, Ref{Ptr{Cvoid}}),
                    0, num_envs, global_offset, Q, max_actions, no_action_reward, seed, r))
        n, hh, ff, aa = Ref{Int64}(), Ref{Int32}(), Ref{Int32}(), Ref{Int32}()          # shapes as the engine reports them
        check(ccall((:ppo_env_dims, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int32}, Ref{Int32}, Ref{Int32}), r[], n, hh, ff, aa))
        e = new(r[], n[], Q, hh[], ff[], aa[], max_actions)
        finalizer(x -> ccall((:ppo_env_destroy, LIB), Int32, (Ptr{Cvoid},), x.h), e)
    end
end

mutable struct HipPolicy
    h::Ptr{Cvoid}; nparams::Int
    function HipPolicy(in_channels, hidden_channels, num_hidden_layers, num_output)   # test/policy.jl:9
        r = Ref{Ptr{Cvoid}}()
        check(ccall((:ppo_policy_create, LIB), Int32, (Int32, Int32, Int32, Int32, Ref{Ptr{Cvoid}}),
                    in_channels, hidden_channels, num_hidden_layers, num_output, r))
        n = Ref{Int64}()
        check(ccall((:ppo_policy_num_params, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), r[], n))
        p = new(r[], n[])
        finalizer(x -> ccall((:ppo_policy_destroy, LIB), Int32, (Ptr{Cvoid},), x.h), p)
    end
end

# arithmetic of the MLP's Dense products: :f32 (Flux's Float32, default) or :bf16 (bf16 MFMA, fp32 accumulation)
set_dtype!(p::HipPolicy, dtype::Symbol) =
    check(ccall((:ppo_policy_set_dtype, LIB), Int32, (Ptr{Cvoid}, Int32), p.h, dtype === :bf16 ? 1 : 0))

# arithmetic of the fp32 TRAINING pass of Policy(72, h, 2, 4): true (default) = its Dense products as split-fp32 products on the
# bf16 matrix pipe (three exact bfloat16 pieces per operand, six piece products, fp32 accumulation: the distance to a Float64
# gradient is that of the fp32 kernels), false = fp32 MFMA.  Rollouts are not affected (their actions are pinned bit for bit).
set_training_split_bf16!(on::Bool) = check(ccall((:ppo_set_bwd_split_bf16, LIB), Int32, (Int32,), on ? 1 : 0))

# Flux.params(policy) round trip: flat vector in Flux order (W1,b1, the num_hidden_layers-1 hidden (W,b) pairs, W_out,b_out),
# W [out,in] column-major; any num_hidden_layers in 1..4 (test/policy.jl:9-19)
set_params!(p::HipPolicy, flat::Vector{Float32}) =
    check(ccall((:ppo_policy_set_params, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}), p.h, flat))
function get_params(p::HipPolicy)
    flat = Vector{Float32}(undef, p.nparams)
    check(ccall((:ppo_policy_get_params, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}), p.h, flat)); flat
end
load_flux_chain!(p::HipPolicy, chain) = set_params!(p, vcat([vec(Float32.(x)) for x in Flux.params(chain)]...))

struct StateData                      # test/quad_game_utilities.jl:17-20 (int8 rows + active-quad bits)
    vertex_score::Array{Int8}; action_mask
end

mutable struct HipRollouts
    h::Ptr{Cvoid}; env::Union{Nothing,HipVecEnv}
    HipRollouts() = new(C_NULL, nothing)              # PPO.BufferRollouts()
end
function ensure!(r::HipRollouts, env::HipVecEnv, T)
    if r.h == C_NULL
        ref = Ref{Ptr{Cvoid}}()
        check(ccall((:ppo_rollouts_create, LIB), Int32, (Ptr{Cvoid}, Int64, Ref{Ptr{Cvoid}}), env.h, T, ref))
        r.h = ref[]; r.env = env
        finalizer(x -> ccall((:ppo_rollouts_destroy, LIB), Int32, (Ptr{Cvoid},), x.h), r)
    end
    r.h
end

# BufferRollouts for a user env whose state(env) rows are not the built-in env's (host-supplied columns: N columns of
# [F, H] Int8 rows, any F the policy was created for -- e.g. the 216-feature level-4 template); filled with set_columns!
function HipRollouts(N::Integer, H::Integer, F::Integer, T::Integer)
    r = HipRollouts()
    ref = Ref{Ptr{Cvoid}}()
    check(ccall((:ppo_rollouts_create_shape, LIB), Int32, (Int64, Int32, Int32, Int64, Ref{Ptr{Cvoid}}), N, H, F, T, ref))
    r.h = ref[]
    finalizer(x -> ccall((:ppo_rollouts_destroy, LIB), Int32, (Ptr{Cvoid},), x.h), r)
    r
end
function set_columns!(r::HipRollouts, states::Array{Int8}, active::Array{UInt32}, actions1, p_sel::Array{Float32}, returns::Array{Float32})
    T = size(active, 2)                                # columns are [N, T] column-major == [T][N]
    check(ccall((:ppo_rollouts_set, LIB), Int32,
                (Ptr{Cvoid}, Int64, Ptr{Int8}, Ptr{UInt32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}),
                r.h, T, states, active, Int32.(actions1 .- 1), p_sel, returns, C_NULL))
end

struct HipAdam; h::Ptr{Cvoid}; eta::Float64; end      # member of a Flux.Optimiser-like iterable
function HipAdam(p::HipPolicy, eta = 1e-3, beta = (0.9, 0.999), eps = 1e-8)
    r = Ref{Ptr{Cvoid}}()
    check(ccall((:ppo_adam_create, LIB), Int32, (Ptr{Cvoid}, Float64, Float64, Float64, Float64, Ref{Ptr{Cvoid}}),
                p.h, eta, beta[1], beta[2], eps, r))
    HipAdam(r[], eta)
end

# Flux.Optimiser chain on the device (ppo_optimiser_create): 1 to 4 of Flux's legacy Adam, ExpDecay, Descent, Momentum,
# Nesterov, RMSProp, ClipValue, ClipNorm, WeightDecay, InvDecay, each kind once, e.g.
# HipChain(policy, Flux.Optimiser(Flux.Adam(1e-4), Flux.ExpDecay(1.0, 0.5, 1000, 1e-6))) or HipChain(policy, Flux.AdamW(3e-4)).
# Iterates the Flux members, so get_optimizer_learning_rate (src/train.jl:155-158) runs on it when every member has an eta;
# their etas (thresh / wd / gamma for the members without) are pushed to the device before each ppo_train! and the decayed
# ExpDecay eta is pulled back after it.
struct HipChain; h::Ptr{Cvoid}; os::Vector{Any}; end
Base.iterate(c::HipChain, s...) = iterate(c.os, s...)
member_row(o::Flux.Adam) = (Int32(1), [o.eta, o.beta[1], o.beta[2], o.epsilon, 0.0])
member_row(o::Flux.ExpDecay) = (Int32(2), [o.eta, o.decay, Float64(o.step), o.clip, Float64(o.start)])
member_row(o::Flux.Descent) = (Int32(3), [o.eta, 0.0, 0.0, 0.0, 0.0])
member_row(o::Flux.Momentum) = (Int32(4), [o.eta, o.rho, 0.0, 0.0, 0.0])
member_row(o::Flux.Nesterov) = (Int32(5), [o.eta, o.rho, 0.0, 0.0, 0.0])
member_row(o::Flux.RMSProp) = (Int32(6), [o.eta, o.rho, o.epsilon, 0.0, 0.0])
member_row(o::Flux.ClipValue) = (Int32(7), [Float64(o.thresh), 0.0, 0.0, 0.0, 0.0])
member_row(o::Flux.ClipNorm) = (Int32(8), [Float64(o.thresh), 0.0, 0.0, 0.0, 0.0])
member_row(o::Flux.WeightDecay) = (Int32(9), [Float64(o.wd), 0.0, 0.0, 0.0, 0.0])
member_row(o::Flux.InvDecay) = (Int32(10), [Float64(o.gamma), 0.0, 0.0, 0.0, 0.0])
member_row(o) = throw(ArgumentError("Optimiser member $(typeof(o)) is not supported on the device"))
function HipChain(p::HipPolicy, opt::Flux.Optimiser)
    1 <= length(opt.os) <= 4 || throw(ArgumentError("the device runs Optimiser chains of 1 to 4 members"))
    rows = map(member_row, opt.os)
    kinds, hyper = Int32[first(r) for r in rows], reduce(vcat, [last(r) for r in rows])
    allunique(kinds) || throw(ArgumentError("each Optimiser member kind at most once on the device"))
    r = Ref{Ptr{Cvoid}}()
    check(ccall((:ppo_optimiser_create, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                p.h, length(kinds), kinds, hyper, r))
    HipChain(r[], collect(opt.os))
end
function push_etas!(c::HipChain)
    for (j, o) in enumerate(c.os)
        if hasproperty(o, :eta)
            check(ccall((:ppo_optimiser_set_eta, LIB), Int32, (Ptr{Cvoid}, Int32, Float64), c.h, j - 1, o.eta))
        else                                          # ClipValue / ClipNorm / WeightDecay / InvDecay: the whole hyper row
            check(ccall((:ppo_optimiser_set_hyper, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}), c.h, j - 1, last(member_row(o))))
        end
    end
end
function pull_etas!(c::HipChain)
    e = Ref{Float64}()
    for (j, o) in enumerate(c.os)
        o isa Flux.ExpDecay || continue                # (members without eta have nothing the device changes)
        check(ccall((:ppo_optimiser_get_eta, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{Float64}), c.h, j - 1, e))
        o.eta = e[]
    end
end
# checkpoint / resume of member j (1-based): (s0, s1, scalars, count) -- Adam (m, v, beta powers), Momentum / Nesterov
# velocity, RMSProp acc, ExpDecay / InvDecay its update count; n = the policy's parameter count
function member_state(c::HipChain, j, n)
    s0, s1, sc, cnt = zeros(Float32, n), zeros(Float32, n), zeros(2), Ref{Int64}(0)
    check(ccall((:ppo_optimiser_get_state, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float64}, Ref{Int64}),
                c.h, j - 1, s0, s1, sc, cnt))
    s0, s1, sc, cnt[]
end
function member_state!(c::HipChain, j, s0::Vector{Float32}, s1::Vector{Float32}, sc::Vector{Float64}, cnt::Int64)
    check(ccall((:ppo_optimiser_set_state, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float64}, Ref{Int64}),
                c.h, j - 1, s0, s1, sc, Ref(cnt)))
end
opt_handle(o::HipChain) = (push_etas!(o); o.h)
opt_handle(o) = (first(o)::HipAdam).h                  # (HipAdam(policy, eta),): the Adam-only form
opt_done!(o::HipChain) = pull_etas!(o)
opt_done!(o) = nothing

# ---------------------------------------------------------------- env plugin methods  (:16-20)
function PPO.state(env::HipVecEnv)
    obs = Array{Int8}(undef, env.F, env.H, env.N); act = Vector{UInt32}(undef, env.N)   # column-major [F,H,N]
    check(ccall((:ppo_env_get_state, LIB), Int32, (Ptr{Cvoid}, Ptr{Int8}, Ptr{UInt32}), env.h, obs, act))
    StateData(obs, act)
end
function PPO.reward(env::HipVecEnv)
    r = Vector{Float32}(undef, env.N)
    check(ccall((:ppo_env_get_reward, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}), env.h, r)); r
end
function PPO.is_terminal(env::HipVecEnv)
    d = Vector{UInt8}(undef, env.N)
    check(ccall((:ppo_env_get_terminal, LIB), Int32, (Ptr{Cvoid}, Ptr{UInt8}), env.h, d)); d .!= 0
end
PPO.reset!(env::HipVecEnv) = check(ccall((:ppo_env_reset, LIB), Int32, (Ptr{Cvoid},), env.h))
PPO.step!(env::HipVecEnv, actions::AbstractVector{<:Integer}) =                      # 1-based -> 0-based
    check(ccall((:ppo_env_step, LIB), Int32, (Ptr{Cvoid}, Ptr{Int32}), env.h, Int32.(actions .- 1)))

# ---------------------------------------------------------------- policy / batching plugin methods  (:23-29)
function PPO.batch_action_probabilities(p::HipPolicy, s::StateData)      # -> [A,B]
    H, B = size(s.vertex_score, 2), size(s.vertex_score, 3)
    probs = Matrix{Float32}(undef, 4H, B)
    check(ccall((:ppo_policy_forward, LIB), Int32, (Ptr{Cvoid}, Ptr{Int8}, Ptr{UInt32}, Int64, Int32, Ptr{Float32}),
                p.h, s.vertex_score, UInt32.(s.action_mask), B, H, probs))
    probs
end
PPO.action_probabilities(p::HipPolicy, s::StateData) = vec(PPO.batch_action_probabilities(p, s))
PPO.number_of_actions_per_state(s::StateData) = 4 * size(s.vertex_score, 2)
PPO.batch_advantage(s::StateData, returns) = returns                    # raw returns (no method exists upstream)

# ---------------------------------------------------------------- path entry points
# compute_returns(rewards, terminal, discount) (src/collect_rollouts.jl:26-42) on the device.  Its own name on purpose:
# the reference's method is untyped, so a `PPO.compute_returns(::Vector{Float32}, ::Vector{Bool}, ::Any)` method here
# would silently re-route every caller's CPU buffers; a user who wants exactly that adds the one-line method
#     PPO.compute_returns(r::Vector{Float32}, t::Vector{Bool}, d) = ProximalPolicyOptimizationHIP.compute_returns_hip(r, t, d)
function compute_returns_hip(rewards::Vector{Float32}, terminal::AbstractVector{Bool}, discount)
    out = similar(rewards)
    check(ccall((:ppo_compute_returns, LIB), Int32, (Ptr{Float32}, Ptr{UInt8}, Int64, Float64, Int32, Ptr{Float32}),
                rewards, UInt8.(terminal), length(rewards), Float64(discount), discount isa Float32, out)); out
end

# collect_rollouts!(rollouts, env, policy, num_episodes, discount) (src/rollout_buffer.jl:66-79): exactly num_episodes
# whole episodes, played in parallel on the resident envs (episode e on env e mod N)
function PPO.collect_rollouts!(r::HipRollouts, env::HipVecEnv, p::HipPolicy, num_episodes, discount)
    h = ensure!(r, env, cld(num_episodes, env.N) * env.max_actions)
    check(ccall((:ppo_collect_rollouts_episodes, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Int32),
                h, env.h, p.h, num_episodes, Float64(discount), discount isa Float32))
end
function Base.length(r::HipRollouts)
    n = Ref{Int64}(); check(ccall((:ppo_rollouts_len, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), r.h, n)); n[]
end
PPO.construct_dataset(r::HipRollouts) = r              # dataset == non-owning view of the same handle

# average_returns(policy, env, num_trajectories) (src/evaluate.jl:18-25) -> (mean, std)
function PPO.average_returns(p::HipPolicy, env::HipVecEnv, num_trajectories)
    scratch = HipRollouts()
    h = ensure!(scratch, env, cld(num_trajectories, env.N) * env.max_actions)
    m, s = Ref{Float64}(), Ref{Float64}()
    check(ccall((:ppo_average_returns, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{Float64}, Ref{Float64}),
                p.h, env.h, h, num_trajectories, m, s))
    m[], s[]
end

# evaluator variants of test/quad_game_utilities.jl:280-307,369-387 (argument order as there: env first)
function average_best_returns(env::HipVecEnv, p::HipPolicy, num_trajectories)
    scratch = HipRollouts()
    h = ensure!(scratch, env, 1)
    m, s = Ref{Float64}(), Ref{Float64}()
    check(ccall((:ppo_average_best_returns, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{Float64}, Ref{Float64}),
                p.h, env.h, h, num_trajectories, m, s))
    m[], s[]
end
function average_normalized_returns(env::HipVecEnv, p::HipPolicy, num_trajectories)
    scratch = HipRollouts()
    h = ensure!(scratch, env, 1)
    m, s = Ref{Float64}(), Ref{Float64}()
    check(ccall((:ppo_average_normalized_returns, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{Float64}, Ref{Float64}),
                p.h, env.h, h, num_trajectories, m, s))
    m[], s[]
end
# per-trajectory values: kind 1 = single_trajectory_return, 2 = best_single_trajectory_return, 3 = single_trajectory_normalized_return
function evaluate_trajectories(env::HipVecEnv, p::HipPolicy, num_trajectories, kind)
    scratch = HipRollouts()
    h = ensure!(scratch, env, 1)
    v = zeros(Float64, num_trajectories)
    check(ccall((:ppo_evaluate_trajectories, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}),
                p.h, env.h, h, num_trajectories, Int32(kind), v))
    v
end

# caller-supplied env states: score, degree [V, N] column-major == [N][V] (V = 4Q), active [N]; every env is left as reset!
# would leave it, the episode and tick counters stay
function set_internal!(env::HipVecEnv, score::Matrix{Int8}, degree::Matrix{Int8}, active::Vector{UInt32})
    check(ccall((:ppo_env_set_internal, LIB), Int32, (Ptr{Cvoid}, Ptr{Int8}, Ptr{Int8}, Ptr{UInt32}), env.h, score, degree, active))
end
function active_quads(env::HipVecEnv)
    a = zeros(UInt32, env.N)
    check(ccall((:ppo_env_get_active, LIB), Int32, (Ptr{Cvoid}, Ptr{UInt32}), env.h, a))
    a
end

# best_state_in_rollout (test/quad_game_utilities.jl:341-358) for num_trajectories trajectories; reset_first = true: the
# average_best_returns convention (reset! before each, env-major), false: every env below num_trajectories plays one
# trajectory from the state it holds.  best_state[:, i] = score[V] then degree[V] of trajectory i's best state; trace[:, i] =
# single_trajectory_scores (:309-323; typemin(Int32) behind the end); type_counts[3:4, i] sum to count_non_flips
function best_states(env::HipVecEnv, p::HipPolicy, num_trajectories; reset_first = true)
    scratch = HipRollouts()
    h = ensure!(scratch, env, 1)
    nt, V = Int(num_trajectories), 4 * env.Q
    st, act = zeros(Int8, 2V, nt), zeros(UInt32, nt)
    gap, step, len, init = zeros(Int32, nt), zeros(Int32, nt), zeros(Int32, nt), zeros(Int32, nt)
    trace, types = zeros(Int32, env.max_actions, nt), zeros(Int32, 4, nt)
    check(ccall((:ppo_best_states, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Int8}, Ptr{UInt32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32},
                 Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                p.h, env.h, h, nt, Int32(reset_first), st, act, gap, step, len, init, trace, types))
    (best_state = st, best_active = act, best_gap = gap, best_step = step, length = len, initial_gap = init, trace = trace,
     type_counts = types)
end
best_state_in_rollout(env::HipVecEnv, p::HipPolicy) = best_states(env, p, env.N; reset_first = false)

# best of K trajectories from each start state: score, degree [V, M] column-major == [M][V], active [M]
function search_best_states(env::HipVecEnv, p::HipPolicy, score::Matrix{Int8}, degree::Matrix{Int8}, active::Vector{UInt32}, K)
    scratch = HipRollouts()
    h = ensure!(scratch, env, 1)
    M, V = length(active), 4 * env.Q
    st, act = zeros(Int8, 2V, M), zeros(UInt32, M)
    gap, clone, step, init = zeros(Int32, M), zeros(Int32, M), zeros(Int32, M), zeros(Int32, M)
    gaps = zeros(Int32, Int(K), M)
    check(ccall((:ppo_search_best_states, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{UInt32}, Ptr{Int8}, Ptr{UInt32},
                 Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                p.h, env.h, h, M, Int64(K), score, degree, active, st, act, gap, clone, step, init, gaps))
    (best_state = st, best_active = act, best_gap = gap, best_clone = clone, best_step = step, initial_gap = init,
     clone_gaps = gaps)
end

# search_best_states with a resample event behind every interval-th step: each start folds its clones' records into its
# result, then the live clones of rank >= min(survivors, live) by (current gap, clone) take the state and record of the
# best-ranked ones.  donors[:, e, i]: per clone of start i at event e the donor clone, -1 kept its state, -2 terminal / no event
function search_resample_states(env::HipVecEnv, p::HipPolicy, score::Matrix{Int8}, degree::Matrix{Int8}, active::Vector{UInt32},
                                K, interval, survivors)
    scratch = HipRollouts()
    h = ensure!(scratch, env, 1)
    M, V = length(active), 4 * env.Q
    st, act = zeros(Int8, 2V, M), zeros(UInt32, M)
    gap, clone, step, init = zeros(Int32, M), zeros(Int32, M), zeros(Int32, M), zeros(Int32, M)
    gaps = zeros(Int32, Int(K), M)
    donors = fill(Int32(-2), Int(K), div(env.max_actions - 1, Int(interval)), M)
    check(ccall((:ppo_search_resample_states, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{UInt32}, Ptr{Int8}, Ptr{UInt32},
                 Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64, Int64, Ptr{Int32}),
                p.h, env.h, h, M, Int64(K), score, degree, active, st, act, gap, clone, step, init, gaps, Int64(interval),
                Int64(survivors), donors))
    (best_state = st, best_active = act, best_gap = gap, best_clone = clone, best_step = step, initial_gap = init,
     clone_gaps = gaps, donors = donors)
end

# The action path to the best state: what step!(wrapper, quad, edge, type) replays onto a mesh.  The three calls above with one
# more output, Int16 [max_actions, n] of 1-based action indices (as the rollout buffer's selected_actions), 0 behind a path's
# end.  The library speaks 0-based indices with -1 as padding: the shim adds / subtracts the 1.  (Int16 arrays cross the ccall
# as Ptr{Cvoid}.)
function best_states_actions(env::HipVecEnv, p::HipPolicy, num_trajectories; reset_first = true)
    scratch = HipRollouts()
    h = ensure!(scratch, env, 1)
    nt, V = Int(num_trajectories), 4 * env.Q
    st, act = zeros(Int8, 2V, nt), zeros(UInt32, nt)
    gap, step, len, init = zeros(Int32, nt), zeros(Int32, nt), zeros(Int32, nt), zeros(Int32, nt)
    trace, types = zeros(Int32, env.max_actions, nt), zeros(Int32, 4, nt)
    actions = zeros(Int16, env.max_actions, nt)
    check(ccall((:ppo_best_states_actions, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Int8}, Ptr{UInt32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32},
                 Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Cvoid}),
                p.h, env.h, h, nt, Int32(reset_first), st, act, gap, step, len, init, trace, types, actions))
    (best_state = st, best_active = act, best_gap = gap, best_step = step, length = len, initial_gap = init, trace = trace,
     type_counts = types, actions = actions .+ Int16(1))
end
# path[1:best_step[i], i]: the winner's actions from start i to its best state
function search_best_states_path(env::HipVecEnv, p::HipPolicy, score::Matrix{Int8}, degree::Matrix{Int8}, active::Vector{UInt32}, K)
    scratch = HipRollouts()
    h = ensure!(scratch, env, 1)
    M, V = length(active), 4 * env.Q
    st, act = zeros(Int8, 2V, M), zeros(UInt32, M)
    gap, clone, step, init = zeros(Int32, M), zeros(Int32, M), zeros(Int32, M), zeros(Int32, M)
    gaps = zeros(Int32, Int(K), M)
    path = zeros(Int16, env.max_actions, M)
    check(ccall((:ppo_search_best_states_path, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{UInt32}, Ptr{Int8}, Ptr{UInt32},
                 Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Cvoid}),
                p.h, env.h, h, M, Int64(K), score, degree, active, st, act, gap, clone, step, init, gaps, path))
    (best_state = st, best_active = act, best_gap = gap, best_clone = clone, best_step = step, initial_gap = init,
     clone_gaps = gaps, path = path .+ Int16(1))
end
# ... along the lineage of the result: a copy carries the donor's actions with its record
function search_resample_states_path(env::HipVecEnv, p::HipPolicy, score::Matrix{Int8}, degree::Matrix{Int8},
                                     active::Vector{UInt32}, K, interval, survivors)
    scratch = HipRollouts()
    h = ensure!(scratch, env, 1)
    M, V = length(active), 4 * env.Q
    st, act = zeros(Int8, 2V, M), zeros(UInt32, M)
    gap, clone, step, init = zeros(Int32, M), zeros(Int32, M), zeros(Int32, M), zeros(Int32, M)
    gaps = zeros(Int32, Int(K), M)
    donors = fill(Int32(-2), Int(K), div(env.max_actions - 1, Int(interval)), M)
    path = zeros(Int16, env.max_actions, M)
    check(ccall((:ppo_search_resample_states_path, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{UInt32}, Ptr{Int8}, Ptr{UInt32},
                 Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64, Int64, Ptr{Int32}, Ptr{Cvoid}),
                p.h, env.h, h, M, Int64(K), score, degree, active, st, act, gap, clone, step, init, gaps, Int64(interval),
                Int64(survivors), donors, path))
    (best_state = st, best_active = act, best_gap = gap, best_clone = clone, best_step = step, initial_gap = init,
     clone_gaps = gaps, donors = donors, path = path .+ Int16(1))
end
# ... ranking the live clones by where the critic (a HipPolicy with 4 outputs read as a state value) expects them to end: by
# fma(-Float32(value_weight), V(s), Float32(current gap)) instead of the current gap; a V(s) that is not finite counts as 0.
# event_values[:, e, i]: the V(s) every live clone of start i was ranked with at event e, NaN for a terminal clone / no event
function search_resample_states_value(env::HipVecEnv, p::HipPolicy, critic::HipPolicy, score::Matrix{Int8}, degree::Matrix{Int8},
                                      active::Vector{UInt32}, K, interval, survivors; value_weight = 1.0)
    scratch = HipRollouts()
    h = ensure!(scratch, env, 1)
    M, V = length(active), 4 * env.Q
    st, act = zeros(Int8, 2V, M), zeros(UInt32, M)
    gap, clone, step, init = zeros(Int32, M), zeros(Int32, M), zeros(Int32, M), zeros(Int32, M)
    gaps = zeros(Int32, Int(K), M)
    donors = fill(Int32(-2), Int(K), div(env.max_actions - 1, Int(interval)), M)
    event_values = fill(NaN32, Int(K), div(env.max_actions - 1, Int(interval)), M)
    path = zeros(Int16, env.max_actions, M)
    check(ccall((:ppo_search_resample_states_value, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{UInt32}, Ptr{Int8},
                 Ptr{UInt32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64, Int64, Float64, Ptr{Int32},
                 Ptr{Float32}, Ptr{Cvoid}),
                p.h, critic.h, env.h, h, M, Int64(K), score, degree, active, st, act, gap, clone, step, init, gaps,
                Int64(interval), Int64(survivors), Float64(value_weight), donors, event_values, path))
    (best_state = st, best_active = act, best_gap = gap, best_clone = clone, best_step = step, initial_gap = init,
     clone_gaps = gaps, donors = donors, event_values = event_values, path = path .+ Int16(1))
end
# beam search: the K likeliest action sequences from every start, deterministic and seed-free (K = 1 is the greedy trajectory).
# A slot's weight (mant, exp) stands for the path probability mant * 2^exp; log_prob = log(best_mant) + best_exp * log(2).
# path = true adds path [max_actions, M]; log = true adds parents / actions / mant / exp [K, max_actions, M], the back-pointer
# log, 1-based with 0 for a dead slot or a step that did not run.  What is not asked for is neither allocated nor kept on the device
# distinct = :children or :parents keeps K DIFFERENT states per step (DESIGN.md 7p): the candidates are walked in the same order,
# at most 256 * rounds of them, and a child whose state equals one accepted before it (:parents: or a live slot's in front of the
# step) is rejected.  log = true then adds rank [K, max_actions, M] (0-based, -1 dead) and examined [max_actions, M]
function beam_search_states(env::HipVecEnv, p::HipPolicy, score::Matrix{Int8}, degree::Matrix{Int8}, active::Vector{UInt32}, K;
                            path::Bool = true, log::Bool = false, distinct::Union{Nothing, Symbol} = nothing, rounds::Integer = 4)
    mode = distinct === nothing ? Int32(0) : distinct === :children ? Int32(1) : distinct === :parents ? Int32(2) :
           throw(ArgumentError("beam_search_states: distinct must be nothing, :children or :parents"))
    scratch = HipRollouts()
    h = ensure!(scratch, env, 1)
    M, V, T = length(active), 4 * env.Q, env.max_actions
    st, act = zeros(Int8, 2V, M), zeros(UInt32, M)
    gap, beam, step, init = zeros(Int32, M), zeros(Int32, M), zeros(Int32, M), zeros(Int32, M)
    bmant, bexp = zeros(Float64, M), zeros(Int32, M)
    pa = path ? zeros(Int16, T, M) : nothing
    lp, la = log ? (zeros(Int16, Int(K), T, M), zeros(Int16, Int(K), T, M)) : (nothing, nothing)
    lm, le = log ? (zeros(Float64, Int(K), T, M), zeros(Int32, Int(K), T, M)) : (nothing, nothing)
    ornull(a) = a === nothing ? C_NULL : pointer(a)
    lr = log && mode != 0 ? zeros(Int32, Int(K), T, M) : nothing
    lx = log && mode != 0 ? zeros(Int32, T, M) : nothing
    GC.@preserve pa lp la lm le lr lx begin
        if mode == 0
            check(ccall((:ppo_beam_search_states, LIB), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{UInt32}, Ptr{Int8}, Ptr{UInt32},
                         Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
                         Ptr{Cvoid}, Ptr{Cvoid}),
                        p.h, env.h, h, M, Int64(K), score, degree, active, st, act, gap, beam, step, init, bmant, bexp, ornull(pa),
                        ornull(lp), ornull(la), ornull(lm), ornull(le)))
        else
            check(ccall((:ppo_beam_search_states_distinct, LIB), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{UInt32}, Ptr{Int8}, Ptr{UInt32},
                         Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
                         Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
                        p.h, env.h, h, M, Int64(K), score, degree, active, st, act, gap, beam, step, init, bmant, bexp, ornull(pa),
                        ornull(lp), ornull(la), ornull(lm), ornull(le), mode, Int32(rounds), ornull(lr), ornull(lx)))
        end
    end
    out = (best_state = st, best_active = act, best_gap = gap, best_beam = beam, best_step = step, initial_gap = init,
           log_prob = Base.log.(bmant) .+ bexp .* Base.log(2.0))
    path && (out = merge(out, (path = pa .+ Int16(1),)))
    log && (out = merge(out, (parents = lp .+ Int16(1), actions = la .+ Int16(1), mant = lm, exp = le)))
    log && mode != 0 && (out = merge(out, (rank = lr, examined = lx)))
    out
end
# teacher-forced replay without a policy: paths [stride, M] column-major == [M][stride], 1-based, anything <= 0 ends a path;
# start i (score, degree [V, M], active [M]) begins as reset! leaves an env.  env supplies Q, max_actions and no_action_reward
# only.  apply_paths(env, starts..., r.path) of a search result r gives r.best_state, r.best_active, r.best_gap, applied == r.best_step
function apply_paths(env::HipVecEnv, score::Matrix{Int8}, degree::Matrix{Int8}, active::Vector{UInt32}, paths::Matrix{Int16})
    M, V, stride = length(active), 4 * env.Q, size(paths, 1)
    raw = max.(paths, Int16(0)) .- Int16(1)
    st, act = zeros(Int8, 2V, M), zeros(UInt32, M)
    gap, applied = zeros(Int32, M), zeros(Int32, M)
    trace = zeros(Int32, stride, M)
    check(ccall((:ppo_env_apply_paths, LIB), Int32,
                (Ptr{Cvoid}, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{UInt32}, Ptr{Cvoid}, Int64, Ptr{Int8}, Ptr{UInt32}, Ptr{Int32},
                 Ptr{Int32}, Ptr{Int32}),
                env.h, M, score, degree, active, raw, Int64(stride), st, act, gap, applied, trace))
    (state = st, active = act, gap = gap, applied = applied, trace = trace)
end
# teacher-forced collection: env i (i <= M <= env.N) is loaded with start i and plays paths[:, i] instead of sampled actions;
# r becomes an ordinary rollout buffer -- the state in front of every step, the path's action, the probability the CURRENT
# policy gives it, reward, terminal (is_terminal or the path's last entry), returns -- that construct_dataset, train! and the
# critic calls take unchanged.  The data is off-policy: p_old is the policy's probability of another sampler's action
function collect_paths!(r::HipRollouts, env::HipVecEnv, p::HipPolicy, score::Matrix{Int8}, degree::Matrix{Int8},
                        active::Vector{UInt32}, paths::Matrix{Int16}, discount)
    M, stride = length(active), size(paths, 1)
    raw = max.(paths, Int16(0)) .- Int16(1)
    h = ensure!(r, env, max(stride, 1))
    check(ccall((:ppo_collect_paths, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{UInt32}, Ptr{Cvoid}, Int64, Float64, Int32, Int32),
                h, env.h, p.h, M, score, degree, active, raw, Int64(stride), Float64(discount), discount isa Float32, Int32(0)))
end

# batch_advantage plugin mode handed to the engine: 0 = returns (PPO.batch_advantage above), 1 = normalised returns,
# 2 / 3 = GAE(gamma, lambda) / normalised GAE over values supplied through compute_gae!
const ADV_MODE = Ref{Int32}(0)
function compute_gae!(r::HipRollouts, values::Matrix{Float32}, gamma, lambda)           # values: [N, T+1] column-major == [T+1][N]
    check(ccall((:ppo_rollouts_compute_gae, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Float64, Float64, Ptr{Float32}, Ptr{Float32}),
                r.h, values, Float64(gamma), Float64(lambda), C_NULL, C_NULL))
end
# ... with time-limit truncations bootstrapped (no reference op): final_values [N, T] column-major == [T][N], the caller's
# value of the state each truncated episode was cut in, 0 at real terminals and at transitions that end no episode
function compute_gae!(r::HipRollouts, values::Matrix{Float32}, final_values::Matrix{Float32}, gamma, lambda)
    check(ccall((:ppo_rollouts_compute_gae_boot, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Float64, Float64, Ptr{Float32}, Ptr{Float32}),
                r.h, values, final_values, Float64(gamma), Float64(lambda), C_NULL, C_NULL))
end
# standalone scan, rewards / done / boot [N, T] and values [N, T+1] column-major -> (advantages, lambda_returns)
function gae_boot_tn(rewards::Matrix{Float32}, done::Matrix{UInt8}, values::Matrix{Float32}, boot::Matrix{Float32}, gamma, lambda)
    adv, ret = similar(rewards), similar(rewards)
    check(ccall((:ppo_gae_boot_tn, LIB), Int32,
                (Ptr{Float32}, Ptr{UInt8}, Ptr{Float32}, Ptr{Float32}, Int64, Int64, Float64, Float64, Ptr{Float32}, Ptr{Float32}),
                rewards, done, values, boot, size(rewards, 2), size(rewards, 1), Float64(gamma), Float64(lambda), adv, ret))
    adv, ret
end
# which done transitions of a built-in-env buffer were time limits, and the states they cut the episodes in: the number K,
# and with fetch the observations [F, H, K], active words [K] (ascending transition id) for a host critic
function truncated_transitions(r::HipRollouts, H, F; fetch = true)
    k = Ref{Int64}()
    check(ccall((:ppo_rollouts_truncated, LIB), Int32, (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int8}, Ptr{UInt32}, Int64, Ref{Int64}),
                r.h, C_NULL, C_NULL, C_NULL, 0, k))
    fetch || return k[]
    states, active = zeros(Int8, F, H, k[]), zeros(UInt32, k[])
    check(ccall((:ppo_rollouts_truncated, LIB), Int32, (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int8}, Ptr{UInt32}, Int64, Ref{Int64}),
                r.h, C_NULL, states, active, k[], k))
    k[], states, active
end

# ppo_train!(policy, optimizer, dataset, epsilon, batch_size, num_epochs, entropy_weight) (src/train.jl:130-153).
# rank / world / hook: data-parallel runs (one process per GPU; INTEGRATION.md section 5); single process: 0 / 1 / C_NULL
function PPO.ppo_train!(p::HipPolicy, optimizer, r::HipRollouts, epsilon, batch_size, num_epochs, entropy_weight;
                        rank = 0, world = 1, hook = C_NULL)
    oh = opt_handle(optimizer)                         # a HipChain, or an iterable whose first member is a HipAdam
    ph, eh, lh = zeros(num_epochs), zeros(num_epochs), zeros(num_epochs)
    status = ccall((:ppo_train, LIB), Int32,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Int64, Int32, Float64, Int32, Ptr{Int64}, UInt64, Int32, Int32,
                    Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                   p.h, oh, r.h, epsilon, batch_size, num_epochs, entropy_weight, ADV_MODE[], C_NULL, SEED[], rank, world,
                   hook, C_NULL, ph, eh, lh)
    opt_done!(optimizer)                               # lr history == get_optimizer_learning_rate(optimizer) afterwards
    check(status)
    n = last_train_stats(p).epochs_run                 # fewer than num_epochs when set_target_kl! ended the call early
    for e in 1:n
        @printf "EPOCH : %d \t PPO LOSS : %1.4f\t ENTROPY LOSS : %1.4f \t LR : %1.1e\n" e ph[e] eh[e] lh[e]
    end
    ph[1:n], eh[1:n], lh[1:n]
end
# ---- behaviour cloning (include/ppo_hip.h "behaviour cloning"; no reference op): supervised learning on the buffer's stored
# actions (collect_paths! of a search's paths, or recorded action histories): -mean(w log pi(a|s)) plus the entropy term.
# weights = :uniform (w = 1) or :positive_advantage (w = max(adv, 0), self-imitation) with advantage = :returns or :gae
const IMITATE_WEIGHTS = Dict(:uniform => Int32(0), :positive_advantage => Int32(1))
const IMITATE_ADV = Dict(:returns => Int32(0), :gae => Int32(2))
function imitate_forward_backward(p::HipPolicy, r::HipRollouts, idx::Vector{Int64}; entropy_weight = 0.0, weights = :uniform,
                                  advantage = :returns, B_global = length(idx))
    check(ccall((:ppo_imitate_forward_backward, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Int64, Int64, Float64, Int32, Int32),
                p.h, r.h, idx .- 1, length(idx), B_global, Float64(entropy_weight), IMITATE_WEIGHTS[weights], IMITATE_ADV[advantage]))
    ce, el = Ref{Float64}(), Ref{Float64}()
    check(ccall((:ppo_last_losses, LIB), Int32, (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}), p.h, ce, el))
    ce[], el[]
end
# the epoch loop of ppo_train! on that loss -> (ce_history, entropy_history, lr_history); never stops early, leaves
# last_train_stats(p) what the latest ppo_train! left.  rank / world / hook as in ppo_train!
function imitate_train!(p::HipPolicy, optimizer, r::HipRollouts, batch_size, num_epochs; entropy_weight = 0.0, weights = :uniform,
                        advantage = :returns, rank = 0, world = 1, hook = C_NULL)
    oh = opt_handle(optimizer)
    ch, eh, lh = zeros(num_epochs), zeros(num_epochs), zeros(num_epochs)
    status = ccall((:ppo_imitate_train, LIB), Int32,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Float64, Int32, Int32, Ptr{Int64}, UInt64, Int32, Int32,
                    Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                   p.h, oh, r.h, batch_size, num_epochs, Float64(entropy_weight), IMITATE_WEIGHTS[weights], IMITATE_ADV[advantage],
                   C_NULL, SEED[], rank, world, hook, C_NULL, ch, eh, lh)
    opt_done!(optimizer)
    check(status)
    ch, eh, lh
end
# ---- policy distillation (include/ppo_hip.h "policy distillation"; no reference op): training towards a distribution over
# actions per stored state.  fill_targets!(r, teacher) leaves the teacher's action probabilities of every stored state in the
# buffer's target column, on the device; targets = :column reads that column, :recorded the distributions a collection with
# record_probs kept.  The loss is -mean(w sum_k q_k log pi(k|s)) plus the entropy term; weights / advantage as for imitation
const DISTILL_TARGETS = Dict(:column => Int32(0), :recorded => Int32(1))
function fill_targets!(r::HipRollouts, teacher::HipPolicy)
    check(ccall((:ppo_rollouts_fill_targets, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), teacher.h, r.h))
end
function distill_forward_backward(p::HipPolicy, r::HipRollouts, idx::Vector{Int64}; entropy_weight = 0.0, weights = :uniform,
                                  advantage = :returns, targets = :column, B_global = length(idx))
    check(ccall((:ppo_distill_forward_backward, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Int64, Int64, Float64, Int32, Int32, Int32),
                p.h, r.h, idx .- 1, length(idx), B_global, Float64(entropy_weight), IMITATE_WEIGHTS[weights], IMITATE_ADV[advantage],
                DISTILL_TARGETS[targets]))
    ce, el = Ref{Float64}(), Ref{Float64}()
    check(ccall((:ppo_last_losses, LIB), Int32, (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}), p.h, ce, el))
    ce[], el[]
end
# the epoch loop of imitate_train! on that loss -> (ce_history, entropy_history, lr_history); never stops early
function distill_train!(p::HipPolicy, optimizer, r::HipRollouts, batch_size, num_epochs; entropy_weight = 0.0, weights = :uniform,
                        advantage = :returns, targets = :column, rank = 0, world = 1, hook = C_NULL)
    oh = opt_handle(optimizer)
    ch, eh, lh = zeros(num_epochs), zeros(num_epochs), zeros(num_epochs)
    status = ccall((:ppo_distill_train, LIB), Int32,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Float64, Int32, Int32, Int32, Ptr{Int64}, UInt64, Int32, Int32,
                    Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                   p.h, oh, r.h, batch_size, num_epochs, Float64(entropy_weight), IMITATE_WEIGHTS[weights], IMITATE_ADV[advantage],
                   DISTILL_TARGETS[targets], C_NULL, SEED[], rank, world, hook, C_NULL, ch, eh, lh)
    opt_done!(optimizer)
    check(status)
    ch, eh, lh
end
# ---- update statistics (include/ppo_hip.h "update statistics"; no reference op): approx_kl = mean((r - 1) - log r),
# old_approx_kl = mean(-log r) and clip_fraction = mean(|r - 1| > epsilon) of every epoch of the latest ppo_train!, and the
# target-KL stop: ppo_train! ends after the first epoch whose approx_kl exceeds target_kl (nothing / 0 = off, Inf = record only)
function set_target_kl!(p::HipPolicy, target_kl)
    check(ccall((:ppo_policy_set_target_kl, LIB), Int32, (Ptr{Cvoid}, Float64), p.h, target_kl === nothing ? 0.0 : Float64(target_kl)))
end
function target_kl(p::HipPolicy)
    t = Ref{Float64}()
    check(ccall((:ppo_policy_get_target_kl, LIB), Int32, (Ptr{Cvoid}, Ref{Float64}), p.h, t))
    t[] == 0 ? nothing : t[]
end
function last_train_stats(p::HipPolicy)
    n, stopped = Ref{Int32}(), Ref{Int32}()
    check(ccall((:ppo_policy_last_train_stats, LIB), Int32,
                (Ptr{Cvoid}, Int32, Ref{Int32}, Ref{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                p.h, Int32(0), n, stopped, C_NULL, C_NULL, C_NULL))
    kl, okl, cf = zeros(n[]), zeros(n[]), zeros(n[])
    check(ccall((:ppo_policy_last_train_stats, LIB), Int32,
                (Ptr{Cvoid}, Int32, Ref{Int32}, Ref{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                p.h, n[], n, stopped, kl, okl, cf))
    (epochs_run = Int(n[]), stopped_early = stopped[] != 0, approx_kl = kl, old_approx_kl = okl, clip_fraction = cf)
end
# ---- KL-anchored PPO (include/ppo_hip.h "KL-anchored PPO"; no reference op): while an anchor is set, ppo_train! and step_batch!
# minimise the PPO loss plus coef * the cross-entropy against the rollouts' target rows (the gradient of coef * KL(q || pi)).
# source = :column (fill_targets!: a frozen cloned or teacher policy) or :recorded (record_probs: PPO's penalty form); target = 0
# keeps coef fixed, d > 0 doubles it behind an epoch whose mean anchor KL exceeds 1.5 d and halves it below d / 1.5
function set_kl_anchor!(p::HipPolicy, coef, source::Symbol = :column, target = 0.0)
    check(ccall((:ppo_policy_set_kl_anchor, LIB), Int32, (Ptr{Cvoid}, Float64, Int32, Float64),
                p.h, Float64(coef), DISTILL_TARGETS[source], Float64(target)))
end
function clear_kl_anchor!(p::HipPolicy)
    check(ccall((:ppo_policy_set_kl_anchor, LIB), Int32, (Ptr{Cvoid}, Float64, Int32, Float64), p.h, 0.0, Int32(-1), 0.0))
end
function kl_anchor(p::HipPolicy)
    c, s, t = Ref{Float64}(), Ref{Int32}(), Ref{Float64}()
    check(ccall((:ppo_policy_get_kl_anchor, LIB), Int32, (Ptr{Cvoid}, Ref{Float64}, Ref{Int32}, Ref{Float64}), p.h, c, s, t))
    s[] < 0 ? nothing : (coef = c[], source = s[] == 0 ? :column : :recorded, target = t[])
end
function last_anchor_stats(p::HipPolicy)
    n = Ref{Int32}()
    check(ccall((:ppo_policy_last_anchor_stats, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}, Ptr{Float64}, Ptr{Float64}),
                p.h, Int32(0), n, C_NULL, C_NULL))
    kl, co = zeros(n[]), zeros(n[])
    check(ccall((:ppo_policy_last_anchor_stats, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}, Ptr{Float64}, Ptr{Float64}),
                p.h, n[], n, kl, co))
    (anchor_kl = kl, anchor_coef = co)
end
# ---- action selection (include/ppo_hip.h "Action selection"; no reference op): how the evaluators, best_states! and the searches
# choose an action -- :sample draws rand(Categorical(p)), :greedy plays argmax(p), p = softmax(logits / temperature).  The
# default (:sample, 1.0) is the reference's rule.  collect_rollouts!, collect_paths!, action_probabilities and train! never read it
const SELECT_RULES = (:sample, :greedy)
function set_selection!(p::HipPolicy, rule::Symbol = :sample, temperature = 1.0)
    r = findfirst(==(rule), SELECT_RULES)
    r === nothing && error("set_selection!: rule must be :sample or :greedy")
    check(ccall((:ppo_policy_set_selection, LIB), Int32, (Ptr{Cvoid}, Int32, Float64), p.h, Int32(r - 1), Float64(temperature)))
end
function get_selection(p::HipPolicy)
    r, t = Ref{Int32}(), Ref{Float64}()
    check(ccall((:ppo_policy_get_selection, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Float64}), p.h, r, t))
    (SELECT_RULES[r[] + 1], t[])
end
# ---- truncation of the distribution :sample draws from (include/ppo_hip.h "Truncation"; no reference op): the top_k likeliest
# actions (0: all) and the likeliest set whose mass in front of an action is below top_p (1.0: all), renormalised; read where the
# selection is read.  :greedy ignores it
function set_truncation!(p::HipPolicy, top_k::Integer = 0, top_p = 1.0)
    check(ccall((:ppo_policy_set_truncation, LIB), Int32, (Ptr{Cvoid}, Int32, Float64), p.h, Int32(top_k), Float64(top_p)))
end
function get_truncation(p::HipPolicy)
    k, t = Ref{Int32}(), Ref{Float64}()
    check(ccall((:ppo_policy_get_truncation, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Float64}), p.h, k, t))
    (Int(k[]), t[])
end
# ---- device critic: a HipPolicy(F, hidden, L, 4) read as a state value (mean of the outputs of the active quads' rows),
# trained with Flux.mse; its state values feed GAE without leaving the device (include/ppo_hip.h "critic")
const VTARGET = Dict(:returns => Int32(0), :lambda_returns => Int32(1))
function batch_state_values(c::HipPolicy, s::StateData)
    vs = s.vertex_score; B = size(vs, 3)                               # [F, H, B] column-major == [B][H][F]
    v = Vector{Float32}(undef, B)
    check(ccall((:ppo_value_forward, LIB), Int32, (Ptr{Cvoid}, Ptr{Int8}, Ptr{UInt32}, Int64, Int32, Ptr{Float32}),
                c.h, vs, UInt32.(s.action_mask), B, size(vs, 2), v))
    v
end
function compute_values!(r::HipRollouts, env::Union{Nothing,HipVecEnv}, c::HipPolicy)
    check(ccall((:ppo_rollouts_compute_values, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}),
                r.h, env === nothing ? C_NULL : env.h, c.h, C_NULL))
end
function compute_gae_critic!(r::HipRollouts, env::Union{Nothing,HipVecEnv}, c::HipPolicy, gamma, lambda)
    check(ccall((:ppo_rollouts_compute_gae_critic, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Float32}, Ptr{Float32}),
                r.h, env === nothing ? C_NULL : env.h, c.h, Float64(gamma), Float64(lambda), C_NULL, C_NULL))
end
# ... with time-limit truncations bootstrapped from the critic's value of the replayed final states -> their number
function compute_gae_critic_boot!(r::HipRollouts, env::Union{Nothing,HipVecEnv}, c::HipPolicy, gamma, lambda)
    k = Ref{Int64}()
    check(ccall((:ppo_rollouts_compute_gae_critic_boot, LIB), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Float32}, Ptr{Float32}, Ref{Int64}),
                r.h, env === nothing ? C_NULL : env.h, c.h, Float64(gamma), Float64(lambda), C_NULL, C_NULL, k))
    k[]
end
function value_forward_backward(c::HipPolicy, r::HipRollouts, idx::Vector{Int64}; target = :returns, B_global = length(idx))
    loss = Ref{Float64}()
    check(ccall((:ppo_value_forward_backward, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Int64, Int64, Int32, Ref{Float64}),
                c.h, r.h, idx .- 1, length(idx), B_global, VTARGET[target], loss))
    loss[]
end
# rank / world / hook as in ppo_train!: every rank trains its replica of the critic on its own shard, the loss history and the
# value-clip statistics are the global ones
function value_train!(c::HipPolicy, optimizer, r::HipRollouts, batch_size, num_epochs; target = :returns,
                      rank = 0, world = 1, hook = C_NULL)
    oh = opt_handle(optimizer)
    mh, lh = zeros(num_epochs), zeros(num_epochs)
    status = if world == 1 && hook == C_NULL
        ccall((:ppo_value_train, LIB), Int32,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Int64}, UInt64, Ptr{Float64}, Ptr{Float64}),
              c.h, oh, r.h, batch_size, num_epochs, VTARGET[target], C_NULL, SEED[], mh, lh)
    else
        ccall((:ppo_value_train_dp, LIB), Int32,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Int64}, UInt64, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid},
               Ptr{Float64}, Ptr{Float64}),
              c.h, oh, r.h, batch_size, num_epochs, VTARGET[target], C_NULL, SEED[], rank, world, hook, C_NULL, mh, lh)
    end
    opt_done!(optimizer)
    check(status)
    mh, lh
end

# ---- PPO's clipped value loss (include/ppo_hip.h "critic: PPO-clipped value loss"; no reference op): with a clip c set on the
# critic, value_forward_backward / value_train! minimise max((V - t)^2, (Vold + clamp(V - Vold, -c, c) - t)^2), Vold = the values
# compute_values! / compute_gae_critic! left on the device (nothing / 0 = off, Inf = record the statistics only); value_train!
# then keeps per epoch clip_fraction = mean(|V - Vold| > c) and mean_sq_change = mean((V - Vold)^2)
function set_value_clip!(c::HipPolicy, clip)
    check(ccall((:ppo_policy_set_value_clip, LIB), Int32, (Ptr{Cvoid}, Float64), c.h, clip === nothing ? 0.0 : Float64(clip)))
end
function value_clip(c::HipPolicy)
    t = Ref{Float64}()
    check(ccall((:ppo_policy_get_value_clip, LIB), Int32, (Ptr{Cvoid}, Ref{Float64}), c.h, t))
    t[] == 0 ? nothing : t[]
end
function last_value_stats(c::HipPolicy)
    n = Ref{Int32}()
    check(ccall((:ppo_policy_last_value_stats, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}, Ptr{Float64}, Ptr{Float64}),
                c.h, Int32(0), n, C_NULL, C_NULL))
    cf, ms = zeros(n[]), zeros(n[])
    check(ccall((:ppo_policy_last_value_stats, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}, Ptr{Float64}, Ptr{Float64}),
                c.h, n[], n, cf, ms))
    (epochs_run = Int(n[]), clip_fraction = cf, mean_sq_change = ms)
end

# 1 - Var(t - V) / Var(t) over the valid transitions, V = the values compute_values! / compute_gae_critic! left on the device
function explained_variance(r::HipRollouts; target = :lambda_returns)
    s = zeros(5)
    check(ccall((:ppo_rollouts_value_moments, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}), r.h, VTARGET[target], s))
    var_t = s[3] / s[1] - (s[2] / s[1])^2
    var_d = s[5] / s[1] - (s[4] / s[1])^2
    var_t == 0 ? NaN : 1 - var_d / var_t
end
# one data-parallel rank's share of it: (n, mean t, M2 t, mean (t - V), M2 (t - V)), M2 = the sum of squared deviations.  The
# host gathers the ranks' rows and merges them in rank order (Chan's pairwise formula) before forming 1 - M2_d / M2_t
function value_moments_row(r::HipRollouts; target = :lambda_returns)
    s, sh = zeros(5), zeros(2)
    check(ccall((:ppo_rollouts_value_moments_shifts, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}),
                r.h, VTARGET[target], s, sh))
    n = s[1]
    (n, sh[1] + s[2] / n, s[3] - s[2]^2 / n, sh[2] + s[4] / n, s[5] - s[4]^2 / n)
end

# ppo_iterate!(policy, env, optimizer, ...) (src/train.jl:210-249) then works unchanged once
# `BufferRollouts()` on its line 230 is replaced by `HipRollouts()` (or dispatched on the env type).

end # module
