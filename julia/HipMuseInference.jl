# HipMuseInference.jl -- the reference-side binding a MuseInference.jl maintainer would add to put
# the MI355X engine (libmuse_hip.so, include/muse_hip.h) behind the package's own problem interface.
#
# NOT exercised in this repository's CI: the build image has no julia.  It is the `ccall` counterpart
# of museinference.jl_amd/problem.py + muse.py (which ARE exercised), kept next to them so that the
# two bindings of the C ABI can be reviewed side by side.  Citations are to the reference sources.
module HipMuseInference

using MuseInference
using MuseInference: AbstractMuseProblem, MuseResult, UnTransformedθ, Transformedθ
import MuseInference: sample_x_z, logLike_and_∇z_logLike, ∇θ_logLike, ẑ_at_θ, logPriorθ, standardizeθ,
                      muse!, get_J!, get_H!, finalize_result!
using Random, Statistics, LinearAlgebra
using Dates: Millisecond

const libmuse_hip = get(ENV, "LIBMUSE_HIP", "libmuse_hip.so")
# :user = the model of a library built from a user's header (include/muse_model.h: the closures of SimpleMuseProblem,
# src/simple.jl:79-89, as three C functions); point LIBMUSE_HIP at libmuse_hip_model_<name>.so
const MODELS = Dict(:funnel => 0, :noise => 1, :smooth => 2, :user => 3)
model_name(id) = (p = ccall((:muse_model_name, libmuse_hip), Cstring, (Cint,), id); p == C_NULL ? nothing : unsafe_string(p))
const MEM_HOST = Cint(0)

struct MuseInfo            # muse_info of include/muse_hip.h
    iterations::Int32
    f_calls::Int32
    status::Int32
    hist_words::Int32
    f_min::Float64
    gnorm::Float64
end

function check(rc::Cint)
    rc == 0 && return
    error("libmuse_hip error $rc: " * unsafe_string(ccall((:muse_last_error, libmuse_hip), Cstring, ())))
end

# A problem whose operators run on the GPU; plays the role of SimpleMuseProblem (src/simple.jl:4-12).
mutable struct HipMuseProblem <: AbstractMuseProblem
    ctx::Ptr{Cvoid}
    x::Vector{Float64}
    N::Int
    nθ::Int
    logPriorθ
    function HipMuseProblem(x::Vector{Float64}; model=:funnel, nθ=1, logPriorθ=(θ->0), device=0)
        ctx = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:muse_ctx_create, libmuse_hip), Cint, (Cint, Int64, Cint, Cint, Ref{Ptr{Cvoid}}),
                    MODELS[model], length(x), nθ, device, ctx))
        check(ccall((:muse_set_data, libmuse_hip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), ctx[], x, MEM_HOST))
        prob = new(ctx[], x, length(x), nθ, logPriorθ)
        finalizer(p -> ccall((:muse_ctx_destroy, libmuse_hip), Cint, (Ptr{Cvoid},), p.ctx), prob)
    end
end

standardizeθ(prob::HipMuseProblem, θ) = collect(Float64, θ isa Number ? [θ] : θ)
logPriorθ(prob::HipMuseProblem, θ) = prob.logPriorθ(θ)

# An rng for this engine is (master seed, sim index): split_rng's contract (src/util.jl:87-92).
struct SimRng <: AbstractRNG
    seed::UInt64
    sim::Int64
end

# ---- per-simulation interface (src/interface.jl:41-99,141-166)
function sample_x_z(prob::HipMuseProblem, rng::SimRng, θ)
    x = Vector{Float64}(undef, prob.N); z = similar(x)
    check(ccall((:muse_sample_x_z, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint),
                prob.ctx, rng.seed, rng.sim, standardizeθ(prob, θ), x, z, MEM_HOST))
    (;x, z)
end
function logLike_and_∇z_logLike(prob::HipMuseProblem, x, z, θ)
    g = similar(z); f = Ref{Float64}(0)
    check(ccall((:muse_logLike_and_grad_z, libmuse_hip), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Cint),
                prob.ctx, x, z, standardizeθ(prob, θ), f, g, MEM_HOST))
    (f[], g)
end
function ∇θ_logLike(prob::HipMuseProblem, x, z, θ)
    g = Vector{Float64}(undef, prob.nθ)
    check(ccall((:muse_grad_theta, libmuse_hip), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint),
                prob.ctx, x, z, standardizeθ(prob, θ), g, MEM_HOST))
    g
end
function ẑ_at_θ(prob::HipMuseProblem, x, z₀, θ; ∇z_logLike_atol)
    ẑ = similar(z₀); info = Ref{MuseInfo}()
    check(ccall((:muse_zhat_at_theta, libmuse_hip), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ref{MuseInfo}, Cint),
                prob.ctx, x, z₀, standardizeθ(prob, θ), ∇z_logLike_atol, ẑ, info, MEM_HOST))
    info[].status >= 3 && @warn("MAP solution did not converge within tolerance, result could be erroneous.")
    isfinite(info[].f_min) || @error("MAP solution failed with logjoint(MAP)=$(-info[].f_min).")
    ẑ, info[]
end

# ---- batched seams: one launch for all elements of the reference's pmap (src/muse.jl:169-176,508-525)
function map_and_score_batch(prob::HipMuseProblem, seed::Integer, sims::UnitRange, θ;
                             include_data=false, atol=1e-2, z0_mode=0)
    n = length(sims) + include_data
    g = Matrix{Float64}(undef, prob.nθ, n); info = Vector{MuseInfo}(undef, n)
    check(ccall((:muse_map_and_score_batch, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int64, Cint, Ptr{Float64}, Float64, Cint, Ptr{Float64}, Ptr{MuseInfo}),
                prob.ctx, seed, first(sims), last(sims) + 1, include_data, standardizeθ(prob, θ), atol, z0_mode, g, info))
    [g[:, i] for i in 1:n], info
end

# muse! for this problem type: the reference's own loop (src/muse.jl:159-236) with the pmap replaced by
# one batched launch; dispatch on the problem type as src/turing.jl:248-256 does for PPL models.
function muse!(result::MuseResult, prob::HipMuseProblem, θ₀=nothing; rng=nothing, maxsteps=50, θ_rtol=1e-1,
               ∇z_logLike_atol=1e-2, nsims=100, α=0.7, get_covariance=false, native_prior=nothing, kwargs...)
    seed = UInt64(something(rng, result.rng, rand(UInt32)))
    result.rng = seed
    θ = standardizeθ(prob, something(result.θ, θ₀))
    history = result.history
    if native_prior !== nothing && isempty(history) && isempty(kwargs) && prob.nθ <= 8
        # The plain option set (untransformed θ, "sims" Jacobian update, constant α, a prior the library evaluates itself:
        # native_prior = (kind, mean, sigma), kind 0 flat / 1 independent Gaussian): the whole loop runs in the library --
        # muse_run_device, ONE persistent launch for every iteration; it falls back to muse_run (one launch per iteration)
        # by itself where the loop kernel does not apply.  Same bits either way, and the same as the loop below.
        # (names that shadow nothing: an `if` block opens no scope in Julia, so `mean = ...` here would make Statistics.mean a
        #  function-wide local and break the loop below)
        pkind, pmean, psigma = native_prior
        θ, hist, gs = muse_run_device(prob, seed, θ; nsims, maxsteps, θ_rtol, ∇z_logLike_atol, α, prior_kind=pkind,
                                      prior_mean=pmean, prior_sigma=psigma)
        nθ = prob.nθ
        for i in 1:size(hist, 2)          # MUSE_RUN_HIST record -> the reference's history record (src/muse.jl:211-221)
            h = hist[:, i]
            θi, g_dat, g_like′, g_prior′, g_post′ = (h[(k-1)*nθ+1:k*nθ] for k in 1:5)
            H⁻¹_like′ = Diagonal(h[5nθ+1:6nθ]); H_prior′ = Diagonal(h[6nθ+1:7nθ])
            H⁻¹_post′ = reshape(h[7nθ+1:7nθ+nθ^2], nθ, nθ)'
            g_like_sims = [gs[:, s, i] for s in 1:nsims]
            push!(history, (;θ=θi, θunreg=θi, θ′=θi, θunreg′=θi, g_like_sims, g_like_dat′=g_dat, g_like_sims′=g_like_sims,
                            g_like′, g_prior′, g_post′, H⁻¹_post′, H_prior′, H⁻¹_like′, H⁻¹_like_sims′=H⁻¹_like′,
                            ẑ_history_dat=nothing, ẑ_history_sims=nothing, t=h[end], ẑ_dat=nothing, ẑ_sims=fill(nothing, nsims)))
        end
        result.θ = θ
        result.gs = history[end].g_like_sims
        result.time += Millisecond(round(Int, 1e3 * sum(hist[end, :])))   # src/muse.jl:232 (the record's t is in seconds)
        if get_covariance
            get_J!(result, prob; rng=seed, nsims, ∇z_logLike_atol)
            get_H!(result, prob; rng=seed, nsims=max(1, nsims ÷ 10), ∇z_logLike_atol)
        end
        return result
    end
    for i = (length(history)+1):maxsteps
        if i > 2
            Δθ = history[end].θ′ - history[end-1].θ′
            sqrt(-(Δθ' * history[end].H⁻¹_post′ * Δθ)) < θ_rtol && break
        end
        z0_mode = i == length(history) + 1 ? 0 : 2     # zero(z) first, then warm starts (src/muse.jl:151,181)
        t₀ = time()
        gs, infos = map_and_score_batch(prob, seed, 0:nsims-1, θ; include_data=true, atol=∇z_logLike_atol, z0_mode)
        g_like_dat, g_like_sims = gs[1], gs[2:end]
        g_like′ = g_like_dat .- Statistics.mean(g_like_sims)
        g_prior′ = MuseInference.AD.gradient(MuseInference.AD.ForwardDiffBackend(), θ -> logPriorθ(prob, θ), θ)[1]
        g_post′ = g_like′ .+ g_prior′
        H⁻¹_like′ = Diagonal(-1 ./ var(g_like_sims))
        H_prior′ = MuseInference.AD.hessian(MuseInference.AD.ForwardDiffBackend(), θ -> logPriorθ(prob, θ), θ)[1]
        H⁻¹_post′ = inv(inv(H⁻¹_like′) + H_prior′)
        # the reference's record, all 19 fields (src/muse.jl:211-221); this problem type has identity transforms,
        # no `regularize` and the "sims" Jacobian update, so several fields coincide
        push!(history, (;θ, θunreg=θ, θ′=θ, θunreg′=θ, g_like_sims, g_like_dat′=g_like_dat, g_like_sims′=g_like_sims,
                        g_like′, g_prior′, g_post′, H⁻¹_post′, H_prior′, H⁻¹_like′, H⁻¹_like_sims′=H⁻¹_like′,
                        ẑ_history_dat=infos[1], ẑ_history_sims=infos[2:end], t=time()-t₀, ẑ_dat=nothing,
                        ẑ_sims=fill(nothing, nsims)))
        θ = θ .- α .* (H⁻¹_post′ * g_post′)
        result.θ = θ
        result.gs = g_like_sims
        result.time += Millisecond(round(Int, 1e3 * history[end].t))      # src/muse.jl:232
    end
    if get_covariance
        get_J!(result, prob; rng=seed, nsims, ∇z_logLike_atol)
        get_H!(result, prob; rng=seed, nsims=max(1, nsims ÷ 10), ∇z_logLike_atol)
    end
    result
end

# The score boards of muse_run_sharded's persistent loop (include/muse_hip.h: muse_comm_board_status) -- COLLECTIVE over a
# shared-memory communicator the first time it is called: (board, device_handshake, host_handshake, device_seen, host_seen,
# last_loop, wait_us) with board / last_loop 0 none, 1 pinned host memory, 2 device memory (hipIpc).
function comm_board_status(prob::HipMuseProblem)
    st = Vector{Cint}(undef, 6); w = Vector{Float64}(undef, 2)
    check(ccall((:muse_comm_board_status, libmuse_hip), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Float64}), prob.ctx, st, w))
    (; board=st[1], device_handshake=st[2], host_handshake=st[3], device_seen=st[4], host_seen=st[5], last_loop=st[6], wait_us=w)
end

# Workgroups per map element (include/muse_hip.h: muse_set_element_split) -- for launches with fewer elements than
# the GPU has compute units, e.g. a rank's share of a strongly scaled map.
set_element_split(prob::HipMuseProblem, split::Integer) =
    check(ccall((:muse_set_element_split, libmuse_hip), Cint, (Ptr{Cvoid}, Cint), prob.ctx, split))

# Columns [col_begin, col_end) of the list (sim_begin, column 0), (sim_begin, column 1), ...: the unit a worker takes when
# get_H! maps over Jacobian columns instead of sims (src/muse.jl:327-333).  Returns an nθ x n matrix of columns.
function fd_jacobian_columns(prob::HipMuseProblem, seed::Integer, sim_begin, col_begin, col_end, θ₀, step; atol=1e-2)
    cols = Matrix{Float64}(undef, prob.nθ, col_end - col_begin)
    check(ccall((:muse_fd_jacobian_columns, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Cint, Int64, Ptr{Float64}, Ptr{Cvoid}),
                prob.ctx, seed, sim_begin, col_begin, col_end, standardizeθ(prob, θ₀), collect(Float64, step), atol, 0, (1 << 62) - 1,
                cols, C_NULL))
    cols
end

# The same loop run by the library's native host code (muse_run of include/muse_hip.h): for a flat or
# independent-Gaussian prior (prior_kind, mean, sigma), constant α and the default "sims" Jacobian update the
# host spends microseconds between two map launches.  Returns (θ, history matrix, per-iteration sim scores).
struct MuseRunOptions
    nsims::Int32; maxsteps::Int32
    θ_rtol::Float64; atol::Float64; α::Float64
    prior_kind::Int32; z0_warm::Int32
    prior_mean::NTuple{8,Float64}; prior_sigma::NTuple{8,Float64}
end
function muse_run(prob::HipMuseProblem, seed::Integer, θ₀; nsims=100, maxsteps=50, θ_rtol=1e-1, ∇z_logLike_atol=1e-2,
                  α=0.7, prior_kind=0, prior_mean=ntuple(_ -> 0.0, 8), prior_sigma=ntuple(_ -> 1.0, 8))
    nθ = prob.nθ; W = 7nθ + nθ^2 + 1                      # MUSE_RUN_HIST(ntheta)
    opt = Ref(MuseRunOptions(nsims, maxsteps, θ_rtol, ∇z_logLike_atol, α, prior_kind, 0, prior_mean, prior_sigma))
    n = Ref{Int32}(0); θ = Vector{Float64}(undef, nθ)
    hist = Matrix{Float64}(undef, W, maxsteps); gs = Array{Float64}(undef, nθ, nsims, maxsteps)
    check(ccall((:muse_run, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Ptr{Float64}, Ref{MuseRunOptions}, Ref{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                prob.ctx, seed, standardizeθ(prob, θ₀), opt, n, θ, hist, gs, C_NULL))
    θ, hist[:, 1:n[]], gs[:, :, 1:n[]]
end

# muse_run_device: the same signature -- ONE persistent launch runs every iteration (map, exchange of the scores between the
# workgroups, step on the GPU, next map); muse_run_sharded: this rank's share of the loop over the ranks of the context's
# communicator (comm_init first) -- a persistent launch per rank whose scores meet on the node's board in pinned host memory,
# or the host-driven loop where that does not apply.  Every rank gets the same (θ, history, scores).
function _native_loop(sym::Symbol, prob::HipMuseProblem, seed::Integer, θ₀; nsims=100, maxsteps=50, θ_rtol=1e-1, ∇z_logLike_atol=1e-2,
                      α=0.7, prior_kind=0, prior_mean=ntuple(_ -> 0.0, 8), prior_sigma=ntuple(_ -> 1.0, 8), z0_warm=false)
    nθ = prob.nθ; W = 7nθ + nθ^2 + 1
    opt = Ref(MuseRunOptions(nsims, maxsteps, θ_rtol, ∇z_logLike_atol, α, prior_kind, z0_warm, prior_mean, prior_sigma))
    n = Ref{Int32}(0); θ = Vector{Float64}(undef, nθ)
    hist = Matrix{Float64}(undef, W, maxsteps); gs = Array{Float64}(undef, nθ, nsims, maxsteps)
    args = (prob.ctx, UInt64(seed), standardizeθ(prob, θ₀), opt, n, θ, hist, gs, C_NULL)
    if sym === :muse_run_device
        check(ccall((:muse_run_device, libmuse_hip), Cint, (Ptr{Cvoid}, UInt64, Ptr{Float64}, Ref{MuseRunOptions}, Ref{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}), args...))
    else
        check(ccall((:muse_run_sharded, libmuse_hip), Cint, (Ptr{Cvoid}, UInt64, Ptr{Float64}, Ref{MuseRunOptions}, Ref{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}), args...))
    end
    θ, hist[:, 1:n[]], gs[:, :, 1:n[]]
end
muse_run_device(prob::HipMuseProblem, seed::Integer, θ₀; kw...) = _native_loop(:muse_run_device, prob, seed, θ₀; kw...)
muse_run_sharded(prob::HipMuseProblem, seed::Integer, θ₀; kw...) = _native_loop(:muse_run_sharded, prob, seed, θ₀; kw...)

# What a SimpleMuseProblem closure captures (src/simple.jl:79-89: a spectrum, a noise map, a mask) for a user-supplied model
# whose header declares run-time constants (include/muse_model.h, muse_const): vector k, one entry per element.
set_constants(prob::HipMuseProblem, k::Integer, values::Vector{Float64}) =
    check(ccall((:muse_set_constants, libmuse_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Cint), prob.ctx, k, values, length(values), MEM_HOST))
# The operator of the "smooth" model as state of the problem (include/muse_hip.h: muse_set_stencil): (A z)_i = w1 (z_{i-1} + z_{i+1})
# + w0 z_i, periodic, any finite pair -- used by every operator, map and get_H! branch from the next call on; `nothing`: back to the
# built-in (1/2, 1/4) stencil and its kernels.
set_stencil(prob::HipMuseProblem, w::Union{Nothing,NTuple{2,Real}}) =
    check(ccall((:muse_set_stencil, libmuse_hip), Cint, (Ptr{Cvoid}, Ptr{Float64}), prob.ctx,
                w === nothing ? C_NULL : Float64[w[1], w[2]]))
function get_stencil(prob::HipMuseProblem)
    w = Vector{Float64}(undef, 2); rt = Ref{Cint}(0)
    check(ccall((:muse_get_stencil, libmuse_hip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cint}), prob.ctx, w, rt))
    (; weights=(w[1], w[2]), runtime=rt[] != 0)
end
# The noise of the "smooth" model as state of the problem (include/muse_hip.h: muse_set_noise): a standard deviation per element
# (finite, > 0) and a mask (true / 1: observed, false / 0: masked; `nothing`: all observed) -- used by every operator, map and
# get_H! branch from the next call on; sd = `nothing`: back to unit noise and the kernels without noise vectors.
function set_noise(prob::HipMuseProblem, sd::Union{Nothing,Vector{Float64}}, mask::Union{Nothing,AbstractVector}=nothing)
    sd === nothing && return check(ccall((:muse_set_noise, libmuse_hip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint), prob.ctx, C_NULL, C_NULL, MEM_HOST))
    m = mask === nothing ? nothing : Float64.(mask)
    check(ccall((:muse_set_noise, libmuse_hip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint), prob.ctx, sd, m === nothing ? C_NULL : m, MEM_HOST))
end
function get_noise(prob::HipMuseProblem)
    sd = Vector{Float64}(undef, prob.N); mask = Vector{Float64}(undef, prob.N); rt = Ref{Cint}(0)
    check(ccall((:muse_get_noise, libmuse_hip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}), prob.ctx, sd, mask, rt))
    (; sd=sd, mask=mask .!= 0, runtime=rt[] != 0)
end
# A pointwise response behind the operator of the "smooth" model as state of the problem (include/muse_hip.h: muse_set_link):
# x_i = phi((A z)_i) + sd_i n_i, phi(u) = u + a2 u^2 + a3 u^3, any finite pair -- used by every operator, map and finite-difference
# get_H! from the next call on (the implicit-differentiation branch is refused while a link is set); `nothing`: no link and the
# kernels that ran before.
# (a library built from a response header -- include/muse_model.h, MUSE_MODEL_RESPONSE -- takes the same call: a = (p0, p1), the
#  header's two run-time numbers; `nothing` means (0, 0))
set_link(prob::HipMuseProblem, a::Union{Nothing,NTuple{2,Real}}) =
    check(ccall((:muse_set_link, libmuse_hip), Cint, (Ptr{Cvoid}, Ptr{Float64}), prob.ctx,
                a === nothing ? C_NULL : Float64[a[1], a[2]]))
function get_link(prob::HipMuseProblem)
    a = Vector{Float64}(undef, 2); rt = Ref{Cint}(0)
    check(ccall((:muse_get_link, libmuse_hip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cint}), prob.ctx, a, rt))
    (; link=(a[1], a[2]), runtime=rt[] != 0)
end
# plain maps over simulations the context has drawn before load their standard normals instead of generating them: off / on
set_normals_cache(prob::HipMuseProblem, enabled::Bool) =
    check(ccall((:muse_set_normals_cache, libmuse_hip), Cint, (Ptr{Cvoid}, Cint), prob.ctx, enabled))
# A user-supplied model's header evaluated for one element on the host -- (grad, objective term, score term, ozz, ozx, bz, bx, z, x,
# dx/dsd): what a consistency check differentiates numerically where the reference has AD (src/simple.jl:84-85)
model_has_second() = ccall((:muse_model_has_second, libmuse_hip), Cint, ()) != 0
function model_eval(prob::HipMuseProblem, iv, sd, x, z, n1, n2, i::Integer)
    out = Vector{Float64}(undef, 12)
    check(ccall((:muse_model_eval, libmuse_hip), Cint, (Ptr{Cvoid}, Float64, Float64, Float64, Float64, Float64, Float64, Int64, Ptr{Float64}),
                prob.ctx, iv, sd, x, z, n1, n2, i, out))
    out
end

# get_H! by implicit differentiation (src/muse.jl:335-405): H = H1 - dFdθᵀ A⁻¹ dFdθ1 with conjugate gradients on the device, for
# whole simulations (nθ × nθ per sim) or for a range of the flattened (sim, column) list (a worker's block, src/muse.jl:327-333)
function implicit_H_batch(prob::HipMuseProblem, seed::Integer, sims::UnitRange, θ₀; atol=1e-1, cg_maxiter=100)
    n = length(sims)
    Hs = Array{Float64}(undef, prob.nθ, prob.nθ, n); its = Matrix{Int32}(undef, prob.nθ, n)
    check(ccall((:muse_implicit_H_batch, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int64, Ptr{Float64}, Float64, Cint, Ptr{Float64}, Ptr{Int32}),
                prob.ctx, UInt64(seed), first(sims), last(sims) + 1, standardizeθ(prob, θ₀), atol, cg_maxiter, Hs, its))
    [permutedims(Hs[:, :, s]) for s in 1:n], its          # (the C ABI is row-major [sim][i][j])
end
function implicit_H_columns(prob::HipMuseProblem, seed::Integer, sim_begin, col_begin, col_end, θ₀; atol=1e-1, cg_maxiter=100)
    cols = Matrix{Float64}(undef, prob.nθ, col_end - col_begin); its = Vector{Int32}(undef, col_end - col_begin)
    check(ccall((:muse_implicit_H_columns, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int64, Int64, Ptr{Float64}, Float64, Cint, Ptr{Float64}, Ptr{Int32}),
                prob.ctx, UInt64(seed), sim_begin, col_begin, col_end, standardizeθ(prob, θ₀), atol, cg_maxiter, cols, its))
    cols, its
end
# The same two with the remaining keywords of the reference's branch (cg_reltol, cg_abstol: IterativeSolvers.cg's keywords; H1_is_zero: get_H!'s implicit_diff_H1_is_zero -- values other than the
#  defaults are honoured for a user's header with second derivatives and, together with Pl = :jacobi, for the built-in funnel and noise models; refused otherwise).  Pl = :jacobi is IterativeSolvers.cg's Pl as
#  Diagonal(diag(A)) of the Hessian the branch applies, formed in the kernel (flag bit MUSE_IMPLICIT_PL_JACOBI); nothing: the identity
const MUSE_IMPLICIT_H1_IS_ZERO = 1
const MUSE_IMPLICIT_PL_JACOBI = 2
function implicit_flags(H1_is_zero, Pl)
    Pl === nothing || Pl === :jacobi || Pl == "jacobi" || throw(ArgumentError("Pl must be nothing (the identity) or :jacobi"))
    (H1_is_zero ? MUSE_IMPLICIT_H1_IS_ZERO : 0) | (Pl === nothing ? 0 : MUSE_IMPLICIT_PL_JACOBI)
end
function implicit_H_batch_ex(prob::HipMuseProblem, seed::Integer, sims::UnitRange, θ₀; atol=1e-1, cg_maxiter=100, cg_reltol=sqrt(eps()),
                          cg_abstol=0.0, H1_is_zero=false, Pl=nothing)
    n = length(sims)
    Hs = Array{Float64}(undef, prob.nθ, prob.nθ, n); its = Matrix{Int32}(undef, prob.nθ, n)
    check(ccall((:muse_implicit_H_batch_ex, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int64, Ptr{Float64}, Float64, Cint, Float64, Float64, Cint, Ptr{Float64}, Ptr{Int32}),
                prob.ctx, UInt64(seed), first(sims), last(sims) + 1, standardizeθ(prob, θ₀), atol, cg_maxiter, cg_reltol, cg_abstol,
                implicit_flags(H1_is_zero, Pl), Hs, its))
    [permutedims(Hs[:, :, s]) for s in 1:n], its          # (the C ABI is row-major [sim][i][j])
end
function implicit_H_columns_ex(prob::HipMuseProblem, seed::Integer, sim_begin, col_begin, col_end, θ₀; atol=1e-1, cg_maxiter=100,
                            cg_reltol=sqrt(eps()), cg_abstol=0.0, H1_is_zero=false, Pl=nothing)
    cols = Matrix{Float64}(undef, prob.nθ, col_end - col_begin); its = Vector{Int32}(undef, col_end - col_begin)
    check(ccall((:muse_implicit_H_columns_ex, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int64, Int64, Ptr{Float64}, Float64, Cint, Float64, Float64, Cint, Ptr{Float64}, Ptr{Int32}),
                prob.ctx, UInt64(seed), sim_begin, col_begin, col_end, standardizeθ(prob, θ₀), atol, cg_maxiter, cg_reltol, cg_abstol,
                implicit_flags(H1_is_zero, Pl), cols, its))
    cols, its
end
# The second derivatives of a header of the two-parameter family (MUSE_MODEL_PAIR_SECOND) for one element on the host:
# (ozz, ozx, gza, gzb, sxa, sxb, xa, xb)
function model_eval_pair_second(prob::HipMuseProblem, a, b, x, z, n1, n2, i::Integer)
    out = Vector{Float64}(undef, 8)
    check(ccall((:muse_model_eval_pair_second, libmuse_hip), Cint,
                (Ptr{Cvoid}, Float64, Float64, Float64, Float64, Float64, Float64, Int64, Ptr{Float64}),
                prob.ctx, a, b, x, z, n1, n2, i, out))
    out
end

# One process per GPU (e.g. MPI.jl ranks or Distributed workers pinned to devices): after
#   id = rank == 0 ? comm_unique_id() : nothing;  id = bcast(id);  comm_init(prob, nranks, rank, id)
# every rank solves its own block of sims and receives everybody's scores: transport = :shm for the workers of one
# node (blocks exchanged host to host through a shared-memory segment, no collective kernel), :rccl for ONE RCCL
# all-gather on the device over xGMI.
function comm_unique_id(transport::Symbol=:rccl; block_doubles=0)
    id = Vector{UInt8}(undef, 128)
    check(ccall((:muse_comm_unique_id_ex, libmuse_hip), Cint, (Cint, Int64, Ptr{UInt8}),
                transport === :shm ? 1 : 0, block_doubles, id)); id
end
comm_init(prob::HipMuseProblem, nranks, rank, id) =
    check(ccall((:muse_comm_init, libmuse_hip), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}), prob.ctx, nranks, rank, id))
function map_and_score_batch_gathered(prob::HipMuseProblem, seed::Integer, mysims::UnitRange, θ, nranks, rows_per_rank;
                                      include_data=false, atol=1e-2, z0_mode=0, area=0)
    check(ccall((:muse_map_and_score_batch_gather_async, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int64, Cint, Ptr{Float64}, Float64, Cint, Int64, Cint),
                prob.ctx, seed, first(mysims), last(mysims) + 1, include_data, standardizeθ(prob, θ), atol, z0_mode, rows_per_rank, area))
    g = Array{Float64}(undef, prob.nθ, rows_per_rank, nranks)     # [nθ, row, rank] column-major = C's [rank][row][nθ]
    check(ccall((:muse_batch_wait_gathered, libmuse_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Cvoid}), prob.ctx, area, g, C_NULL))
    g
end

function get_J!(result::MuseResult, prob::HipMuseProblem, θ₀=nothing; rng=result.rng, nsims=100, ∇z_logLike_atol=1e-2, kwargs...)
    θ₀ = standardizeθ(prob, something(θ₀, result.θ))
    existing = length(result.gs)
    if nsims > existing                                   # src/muse.jl:499-506
        gs, _ = map_and_score_batch(prob, UInt64(rng), existing:nsims-1, θ₀; atol=∇z_logLike_atol, z0_mode=1)
        append!(result.gs, gs)
    end
    result.J = cov(reduce(hcat, result.gs)'; corrected=true)
    finalize_result!(result, prob)
end

# Several independent maps (one θ each) in ONE launch: muse_map_and_score_multi_async -- what keeps a GPU full when one
# map's share of the sims is smaller than the GPU (bench.py --gpus N).  thetas: nθ × nmaps.
function map_and_score_multi(prob::HipMuseProblem, seed::Integer, sims::UnitRange, thetas::AbstractMatrix;
                             include_data=false, atol=1e-2, z0_mode=0, area=0)
    nmaps = size(thetas, 2)
    n = length(sims) + (include_data ? 1 : 0)
    check(ccall((:muse_map_and_score_multi_async, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int64, Cint, Cint, Ptr{Float64}, Float64, Cint, Cint),
                prob.ctx, seed, first(sims), last(sims) + 1, include_data, nmaps, Matrix{Float64}(thetas), atol, z0_mode, area))
    g = Array{Float64}(undef, prob.nθ, n, nmaps)                  # column-major [nθ, element, map] = C's [map][element][nθ]
    check(ccall((:muse_batch_wait, libmuse_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Cvoid}), prob.ctx, area, g, C_NULL))
    g
end

# The values fdm(f, 0[, step]) asks for in pjacobian (src/util.jl:9-27), every grid point of every (sim, column) unit one
# problem of one launch: offsets is G × nθ (one column of offsets per θ component, shared by the sims).
function fd_values(prob::HipMuseProblem, seed::Integer, nsims::Integer, θ₀, offsets::AbstractMatrix; atol=1e-2)
    G = size(offsets, 1)
    F = Array{Float64}(undef, prob.nθ, G, prob.nθ, nsims)         # [i, grid point, column j, sim]
    check(ccall((:muse_fd_values_columns, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int64, Int64, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Float64, Cint, Int64, Ptr{Float64}, Ptr{Cvoid}),
                prob.ctx, seed, 0, 0, nsims * prob.nθ, θ₀, G, Matrix{Float64}(offsets), 0, atol, 0, (1 << 62) - 1, F, C_NULL))
    F
end

function get_H!(result::MuseResult, prob::HipMuseProblem, θ₀=nothing; rng=result.rng, nsims=10, step=nothing,
                fdm=central_fdm(3,1), ∇z_logLike_atol=1e-2, kwargs...)
    θ₀ = standardizeθ(prob, something(θ₀, result.θ))
    remaining = nsims - length(result.Hs)
    remaining <= 0 && return
    if !(step === nothing && isempty(result.gs)) && fdm.grid != [-1, 0, 1]
        # another central_fdm(p, 1) with an explicit step: its non-zero-coefficient grid points through fd_values
        step = collect(Float64, something(step, 0.1 ./ std(result.gs)))
        nz = findall(!iszero, fdm.coefs)
        F = fd_values(prob, UInt64(rng), remaining, θ₀, [fdm.grid[g] * step[j] for g in nz, j in 1:prob.nθ]; atol=∇z_logLike_atol)
        append!(result.Hs, [hcat((sum(fdm.coefs[nz[g]] .* F[:, g, j, s] for g in eachindex(nz)) ./ step[j] for j in 1:prob.nθ)...) for s in 1:remaining])
        result.H = mean(result.Hs)
        return finalize_result!(result, prob)
    end
    # (neither step nor result.gs: FiniteDifferences estimates the step per call; the Python host does that through the same
    #  entry point with offsets per (sim, column) unit -- museinference.jl_amd/fdm.py, muse.py:_fd_batched)
    step = something(step, 0.1 ./ std(result.gs))         # src/muse.jl:411-413
    Hs = Array{Float64}(undef, prob.nθ, prob.nθ, remaining)
    check(ccall((:muse_fd_jacobian_batch, libmuse_hip), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Cint, Int64, Ptr{Float64}, Ptr{Cvoid}),
                prob.ctx, UInt64(rng), 0, remaining, θ₀, collect(Float64, step), ∇z_logLike_atol, 0, (1 << 62) - 1, Hs, C_NULL))
    # the C ABI returns row-major [sim][i][j]; Julia reads it column-major as [j][i][sim]
    append!(result.Hs, [permutedims(Hs[:, :, s]) for s in 1:remaining])
    result.H = mean(result.Hs)
    finalize_result!(result, prob)
end

end # module
