# ACMEHip.jl -- Julia binding of libacme_hip.so (include/acme_hip.h) for ACME.jl.
#
# Drops the MI355X batch runner in behind ACME's own circuit-derivation front end WITHOUT any change
# to ACME: everything the C ABI needs is read from an ordinary `DiscreteModel` --
#   * the model matrices are its fields (src/ACME.jl:118-148),
#   * the element table (kind, parameters, q offset, residual offset per nonlinear element, in
#     `CircuitNLFunc` order, src/circuit.jl:68-86) is recovered by walking the closures the model
#     already holds: Julia closures expose their captured variables as fields, so
#     `model.nonlinear_eq_funcs[idx]` (src/ACME.jl:176-189) -> `circ_nl_func::CircuitNLFunc` ->
#     `.fs[k]` (src/circuit.jl:76-80: captures `q_indices`, `nleqfunc`) -> the element's own closure
#     (src/elements.jl), whose captured variables are the element parameters,
#   * each solver's initial extrapolation origin (p = 0, z = init_z; src/ACME.jl:253-259) comes from
#     `get_extrapolation_origin` of the innermost solver of `model.solvers[idx]`.
#
# Two levels, as SURVEY.md 8(b) describes:
#   * `BatchRunner` / `run!(::BatchRunner, y, u)` -- the performant seam: N instances of a model
#     advance together on the GPU (the batch analogue of `ModelRunner`, src/ACME.jl:570-664).
#   * `GPUBatchSolver <: ACME.NonlinearSolver` -- the solver plugin contract of src/solvers.jl:139-205
#     (constructor `S(nleq, initial_p, initial_z)`, `solve`, `hasconverged`, `needediterations`,
#     `set_resabstol!`, `get/set_extrapolation_origin`, `get_extrapolation_jacobian`) on top of
#     `acme_batch_solve`, so that `DiscreteModel(circ, t, ACMEHip.GPUBatchSolver)`, `steadystate`,
#     `linearize` and ACME's own solver tests run against the device code.  One `ccall` per solve:
#     this is for API parity and validation, not for throughput.
#
# NOTE: the build image of this repository has no Julia; this file is written against the ACME.jl
# sources cited above (and Julia >= 1.6 semantics) but has not been executed here.  The same ABI is
# exercised end to end by acme_jl_amd/runner.py (ctypes) and examples/abi_demo.c (plain C).
module ACMEHip

using ACME
using ACME: DiscreteModel, NonlinearSolver, ParametricNonLinEq
using LinearAlgebra: I
import ProgressMeter
import ACME: run!, solve, hasconverged, needediterations, set_resabstol!,
             get_extrapolation_origin, set_extrapolation_origin, get_extrapolation_jacobian

export BatchRunner, MultiBatchRunner, GPUBatchSolver, element_table, retain_host_buffers!, release_host_buffers!, set_isolation!, set_balance!,
       MeasureSpec, Measurement, set_measurement!, clear_measurement!, reset_measurement!, measurement, measurement_plan, measure!,
       set_source!, clear_source!, source_clock, source_clock!, run_sources!, render_sources,
       set_source_multisine!, set_source_noise!, set_source_pulse!, set_source_burst!, set_measurement_bins!, set_measurement_series!, measurement_series,
       set_measurement_fold!, measurement_fold, set_measurement_spectrum!, measurement_spectrum,
       set_measurement_cross!, measurement_cross, set_measurement_target!, measurement_target,
       set_measurement_weighting!, measurement_weighting, set_measurement_ensemble!, measurement_ensemble,
       set_measurement_histogram!, measurement_histogram, set_measurement_events!, measurement_events

const lib = get(ENV, "ACME_HIP_LIB", "libacme_hip.so")

# ---- include/acme_hip.h ------------------------------------------------------------------------
const ACME_KIND_DIODE, ACME_KIND_BJT, ACME_KIND_POT = Cint(1), Cint(2), Cint(3)
const ACME_KIND_MOSFET, ACME_KIND_MACAK, ACME_KIND_JA = Cint(4), Cint(5), Cint(6)
const ACME_MAX_ELEM_PAR = 16
const ACME_SOLVER_SIMPLE, ACME_SOLVER_HOMOTOPY, ACME_SOLVER_CACHING_HOMOTOPY = Cint(0), Cint(1), Cint(2)
const ACME_MEM_HOST, ACME_MEM_DEVICE = Cint(0), Cint(1)
const ACME_MAX_OVERSAMPLING = 16
const ACME_MAX_HARMONICS = 32
const ACME_MAX_SERIES_WINDOWS = 1048576
const ACME_MIN_SPECTRUM = 64
const ACME_MAX_SPECTRUM = 4096
const ACME_MAX_TARGETS = 64
const ACME_MAX_WEIGHTING_SECTIONS = 8
const ACME_MAX_ENSEMBLE = 16777216
const ACME_HIST_SIGNED, ACME_HIST_ABS = Cint(0), Cint(1)
const ACME_MAX_HIST_BINS = 4096
const ACME_MAX_HISTOGRAM = 268435456
const ACME_MAX_EVENT_LEVELS = 8
const ACME_MAX_EVENT_SLOTS = 16
const ACME_MAX_EVENTS = 16777216
const ACME_EVENT_RISE, ACME_EVENT_FALL, ACME_EVENT_HIGH, ACME_EVENT_LOW, ACME_EVENT_UNKNOWN = Cint(0), Cint(1), Cint(2), Cint(3), Cint(4)
const ACME_SOURCE_CONST, ACME_SOURCE_SINE, ACME_SOURCE_TABLE, ACME_SOURCE_MULTISINE = Cint(1), Cint(2), Cint(3), Cint(4)
const ACME_SOURCE_NOISE = Cint(5)
const ACME_SOURCE_PULSE, ACME_SOURCE_BURST = Cint(6), Cint(7)
const ACME_NOISE_UNIFORM, ACME_NOISE_GAUSSIAN = Cint(0), Cint(1)
const ACME_MAX_SOURCE_TABLE = 16777216
const ACME_MAX_SOURCE_TONES = 4
const KIND_NQ = Dict(1 => 2, 2 => 4, 3 => 5, 4 => 3, 5 => 2, 6 => 4)
const KIND_NN = Dict(1 => 1, 2 => 2, 3 => 2, 4 => 1, 5 => 1, 6 => 1)

struct AcmeOptions
    solver::Cint
    tol::Cdouble
    maxiter::Cint
    device::Cint
    per_instance_matrices::Cint
end

struct AcmeReport
    n_warn::Clonglong
    first_nonconverged::Clonglong
    first_nonfinite::Clonglong
    iters_total::Clonglong
    iters_max::Clonglong
end

lasterror() = unsafe_string(ccall((:acme_last_error, lib), Cstring, ()))
check(rc) = rc < 0 ? error("libacme_hip: " * lasterror()) : rc
"number of HIP devices the library sees"
device_count() = Int(ccall((:acme_device_count, lib), Cint, ()))

# ---- closures -> element table -----------------------------------------------------------------
"captured variable `name` of closure `f` (unwrapping the Box of a re-assigned capture)"
function captured(f, name::Symbol)
    v = getfield(f, name)
    return v isa Core.Box ? v.contents : v
end
hascaptured(f, name::Symbol) = name in fieldnames(typeof(f))
capturednames(f) = fieldnames(typeof(f))

"""
    describe_element(f) -> (kind, params)

`f` is the `nonlinear_eq` closure of one element (src/elements.jl); the kind is recognised by the
set of variables it captures, the parameter vector is laid out as include/acme_hip.h documents.
"""
function describe_element(f)
    names = capturednames(f)
    par = zeros(Float64, ACME_MAX_ELEM_PAR)
    if :βf in names                                   # bjt, src/elements.jl:323-401
        g = (n, default) -> hascaptured(f, n) ? Float64(captured(f, n)) : default
        ηe, ηc = g(:ηe, 1.0), g(:ηc, 1.0)
        par[1:14] = [g(:ise, 1e-12), g(:isc, 1e-12), ηe, ηc, g(:βf, 1000.0), g(:βr, 10.0),
                     g(:ile, 0.0), g(:ilc, 0.0), g(:ηel, ηe), g(:ηcl, ηc),
                     g(:vaf, Inf), g(:var, Inf), g(:ikf, Inf), g(:ikr, Inf)]
        return ACME_KIND_BJT, par
    elseif :is in names && :η in names                # diode, :238-244
        par[1:2] = [Float64(captured(f, :is)), Float64(captured(f, :η))]
        return ACME_KIND_DIODE, par
    elseif :polarity in names && :vt in names         # mosfet, :453-479
        vt, α = captured(f, :vt), captured(f, :α)
        (length(vt) <= 4 && length(α) <= 4) || error("mosfet: at most 4 polynomial coefficients are supported")
        par[1] = Float64(captured(f, :polarity)); par[2] = Float64(captured(f, :λ))
        par[3] = length(vt); par[4:3+length(vt)] .= Float64.(vt)
        par[8] = length(α); par[9:8+length(α)] .= Float64.(α)
        return ACME_KIND_MOSFET, par
    elseif :gain in names && :scale in names          # opamp(Val{:macak}, ...), :540-546
        par[1:2] = [Float64(captured(f, :gain)), Float64(captured(f, :scale))]
        return ACME_KIND_MACAK, par
    elseif :Ms in names                               # Jiles-Atherton core, :107-129
        par[1:5] = Float64[captured(f, :Ms), captured(f, :a), captured(f, :α), captured(f, :c), captured(f, :k)]
        return ACME_KIND_JA, par
    elseif names == (:r,)                             # potentiometer(r), :25-30
        par[1] = Float64(captured(f, :r))
        return ACME_KIND_POT, par
    end
    error("ACMEHip: nonlinear element of unknown kind (captures $(names)); the device code knows " *
          "diode, bjt, potentiometer, mosfet, opamp(Val{:macak}) and the Jiles-Atherton core")
end

"""
    element_table(circ_nl_func) -> (kinds, qoff, roff, par)

The element table of one nonlinear sub-problem, in `CircuitNLFunc` order (src/circuit.jl:68-86).
`circ_nl_func.fs[k]` captures `q_indices` (the element's columns of q) and `nleqfunc`.
"""
function element_table(cnl)
    kinds, qoff, roff = Cint[], Cint[], Cint[]
    par = zeros(Float64, ACME_MAX_ELEM_PAR, length(cnl.fs))   # column-major 16 x n == row-major n x 16
    r = 0
    for (k, f) in enumerate(cnl.fs)
        qi = captured(f, :q_indices)
        kind, p = describe_element(captured(f, :nleqfunc))
        length(qi) == KIND_NQ[Int(kind)] || error("ACMEHip: element $k has $(length(qi)) q rows, kind $kind expects $(KIND_NQ[Int(kind)])")
        push!(kinds, kind); push!(qoff, first(qi) - 1); push!(roff, r)
        par[:, k] = p
        r += KIND_NN[Int(kind)]
    end
    return kinds, qoff, roff, par
end

"`CircuitNLFunc` of sub-problem idx of a model: captured by the closure of src/ACME.jl:176-189"
circuit_nl_func(model::DiscreteModel, idx) = captured(model.nonlinear_eq_funcs[idx], :circ_nl_func)

# (p, z) the innermost solver extrapolates from; HomotopySolver has no get_extrapolation_origin of
# its own in the reference (src/solvers.jl:198,398), so unwrap `.basesolver`
base_origin(s::ACME.SimpleSolver) = get_extrapolation_origin(s)
base_origin(s::NonlinearSolver) = hasfield(typeof(s), :basesolver) ? base_origin(s.basesolver) : get_extrapolation_origin(s)

solver_id(::Type{<:ACME.SimpleSolver}) = ACME_SOLVER_SIMPLE
solver_id(::Type{<:ACME.HomotopySolver{<:ACME.SimpleSolver}}) = ACME_SOLVER_HOMOTOPY
solver_id(::Type{<:ACME.HomotopySolver{<:ACME.CachingSolver}}) = ACME_SOLVER_CACHING_HOMOTOPY   # bounded store, see acme_hip.h
solver_id(::Type{T}) where {T} = error("ACMEHip: no device counterpart of solver type $T")

# ---- acme_model ---------------------------------------------------------------------------------
mutable struct ModelHandle
    h::Ptr{Cvoid}
    function ModelHandle(h)
        m = new(h)
        finalizer(m -> ccall((:acme_model_destroy, lib), Cvoid, (Ptr{Cvoid},), m.h), m)
        return m
    end
end

function add_subproblem!(h::Ptr{Cvoid}, nn, nq, np, pexp, dq, eq, fqprev, fq, q0, init_z, cnl)
    kinds, qoff, roff, par = element_table(cnl)
    check(ccall((:acme_model_add_subproblem, lib), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
         Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
        h, nn, nq, np, Matrix{Float64}(pexp), Matrix{Float64}(dq), Matrix{Float64}(eq),
        Matrix{Float64}(fqprev), Matrix{Float64}(fq), Vector{Float64}(q0), Vector{Float64}(init_z),
        length(kinds), kinds, qoff, roff, par))
end

"acme_model of a whole DiscreteModel (all matrices are Matrix{Float64}, column-major: passed as they are)"
function ModelHandle(model::DiscreteModel)
    h = Ref{Ptr{Cvoid}}()
    check(ccall((:acme_model_create, lib), Cint,
        (Cint, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
         Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
        ACME.nx(model), ACME.nu(model), ACME.ny(model), ACME.nn(model),
        model.a, model.b, model.c, model.x0, model.dy, model.ey, model.fy, model.y0, h))
    mh = ModelHandle(h[])
    for idx in 1:length(model.solvers)
        _, init_z = base_origin(model.solvers[idx])                  # (0, init_z) on a fresh model
        add_subproblem!(mh.h, ACME.nn(model, idx), ACME.nq(model, idx), ACME.np(model, idx),
                        model.pexps[idx], model.dqs[idx], model.eqs[idx], model.fqprevs[idx],
                        model.fqs[idx], model.q0s[idx], init_z, circuit_nl_func(model, idx))
    end
    return mh
end

# ---- BatchRunner: N instances of a model on one GPU ------------------------------------------------
"""
    BatchRunner(model::DiscreteModel, n; device=-1, solver=<the model's own solver type>)

N parallel copies of `model` on one MI355X: the batch analogue of `ACME.ModelRunner`
(src/ACME.jl:570-604).  Every instance starts like a fresh model (x = 0, origin (0, init_z)).
"""
mutable struct BatchRunner
    model::DiscreteModel
    n::Int
    h::Ptr{Cvoid}
    mh::ModelHandle
    warned::Int
    progress::Base.RefValue{Any}      # the ProgressMeter.Progress of the run in flight (showprogress = true)
    showprogress::Bool
    meas::Any                         # the armed MeasureSpec (nothing: none)
    sources::Set{Int}                 # the input rows (1-based) that have a source
    spectrum::Int                     # nfft of the spectrum set on the armed measurement (0: none)
    cross::Int                        # nfft of the cross-spectrum set on the armed measurement (0: none)
    ensemble::Tuple{Int,Int}          # (G, stride) of the ensemble set on the armed measurement ((0, 0): none)
    histogram::Int                    # the bins B of the histogram set on the armed measurement (0: none)
    events::Tuple{Int,Int}            # (C, E) of the events set on the armed measurement ((0, 0): none)
end

# @showprogress of run!(runner, y, u) (src/ACME.jl:587-604,653): the library reports after every time slice of a
# host-buffer run through a C callback; `user` points at the runner's `progress` cell (kept alive by the runner)
function progress_trampoline(user::Ptr{Cvoid}, done::Clonglong, total::Clonglong)::Cvoid
    p = unsafe_pointer_to_objref(user)::Base.RefValue{Any}
    p[] === nothing || ProgressMeter.update!(p[], Int(done))
    return nothing
end

function BatchRunner(model::DiscreteModel, n::Integer; device::Integer=-1,
                     solver=isempty(model.solvers) ? ACME_SOLVER_HOMOTOPY : solver_id(typeof(model.solvers[1])),
                     per_instance_matrices::Bool=false, showprogress::Bool=false)
    mh = ModelHandle(model)
    opts = Ref(AcmeOptions(solver, 1e-10, 500, device, per_instance_matrices ? 1 : 0))
    b = Ref{Ptr{Cvoid}}()
    check(ccall((:acme_batch_create, lib), Cint, (Ptr{Cvoid}, Clonglong, Ref{AcmeOptions}, Ref{Ptr{Cvoid}}),
                mh.h, n, opts, b))
    r = BatchRunner(model, n, b[], mh, 0, Ref{Any}(nothing), showprogress, nothing, Set{Int}(), 0, 0, (0, 0), 0, (0, 0))
    finalizer(r -> ccall((:acme_batch_destroy, lib), Cvoid, (Ptr{Cvoid},), r.h), r)
    if showprogress
        cb = @cfunction(progress_trampoline, Cvoid, (Ptr{Cvoid}, Clonglong, Clonglong))
        check(ccall((:acme_batch_set_progress_callback, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                    r.h, cb, pointer_from_objref(r.progress)))
    end
    return r
end

"""
    retain_host_buffers!(runner, keep=true)

By default `run!` leaves nothing of `u` / `y` registered with the GPU runtime once it returns (they are ordinary,
garbage-collected arrays: a registration must never outlive them).  `retain_host_buffers!(runner)` is the caller's
promise to keep the arrays it passes alive -- reuse them across `run!(runner, y, u)` calls, hold references -- until it
passes others, calls `release_host_buffers!` or drops the runner: they are then page-locked once and runs are streamed
at the device-resident rate (`acme_batch_set_host_retention`, `include/acme_hip.h`).
"""
retain_host_buffers!(r::BatchRunner, keep::Bool=true) =
    (check(ccall((:acme_batch_set_host_retention, lib), Cint, (Ptr{Cvoid}, Cint), r.h, keep ? 1 : 0)); r)

"""
    release_host_buffers!(runner)

Un-page-lock what a retaining runner (`retain_host_buffers!`) holds: before freeing or resizing the arrays while the
runner lives on.
"""
release_host_buffers!(r::BatchRunner) =
    (check(ccall((:acme_batch_release_host_buffers, lib), Cint, (Ptr{Cvoid},), r.h)); r)

"""
    set_isolation!(runner, iters_per_sample)

Launch the instances that needed more than `iters_per_sample` Newton iterations per sample over the previous run on
their own (a pathological cell of a sweep otherwise holds every other instance's results back by its own, hundreds of
times longer, run; `include/acme_hip.h`).  `0` switches it off.
"""
set_isolation!(r::BatchRunner, iters_per_sample::Real) =
    (check(ccall((:acme_batch_set_isolation, lib), Cint, (Ptr{Cvoid}, Cdouble), r.h, iters_per_sample)); r)

"""
    set_balance!(runner, mode)

Placement of a launch's waves by their measured cost (`acme_batch_set_balance`): `-1` lets the library decide (the
default: on when the launch has more blocks than the device has compute units), `0` switches it off, `1` on.
What an instance computes does not depend on it.
"""
set_balance!(r::BatchRunner, mode::Integer) =
    (check(ccall((:acme_batch_set_balance, lib), Cint, (Ptr{Cvoid}, Cint), r.h, mode)); r)

"""
    oversampling_design(factor) -> Vector{Float64}

The library's default lowpass for oversampling by `factor` (`acme_oversampling_design`): linear-phase Kaiser-windowed
sinc at the high rate, unit DC gain, passband to 0.40 fs, at least 80 dB from 0.50 fs, length L odd with L = 1 (mod
factor) -- the pair delays the signal by (L - 1) / factor base-rate samples.  Python and Julia get the same taps.
"""
function oversampling_design(factor::Integer)
    n = check(ccall((:acme_oversampling_design, lib), Cint, (Cint, Ptr{Cdouble}, Cint), factor, C_NULL, 0))
    taps = zeros(Float64, n)
    check(ccall((:acme_oversampling_design, lib), Cint, (Cint, Ptr{Cdouble}, Cint), factor, taps, n))
    return taps
end

"""
    set_oversampling!(runner, factor; up=nothing, down=nothing, held_rows=())

Oversampled runs (`acme_batch_set_oversampling`): the runner's model is derived at `factor` x the signal rate; `run!`
then takes `u` and returns `y` at the BASE rate while the model advances `factor` samples per column.  Input rows are
interpolated with `factor * up`, the rows in `held_rows` (1-based: pot positions, supplies, mix controls) held, the
outputs decimated with `down`; `nothing` = the library's default lowpass (`oversampling_design`).  Resets the filters'
histories: each signal's first column extends into the past at the next `run!`, later calls continue where the last
ended.  Reports count model-rate samples.  `factor = 1` switches it off.
"""
function set_oversampling!(r::BatchRunner, factor::Integer; up=nothing, down=nothing, held_rows=())
    nu = ACME.nu(r.model)
    mask = UInt64(0)
    for k in held_rows
        1 <= k <= min(nu, 64) || throw(DimensionMismatch("held row $k of a model with $nu inputs"))
        mask |= UInt64(1) << (k - 1)
    end
    hu = up === nothing ? Float64[] : collect(Float64, up)
    hd = down === nothing ? Float64[] : collect(Float64, down)
    GC.@preserve hu hd check(ccall((:acme_batch_set_oversampling, lib), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Culonglong),
                r.h, factor, up === nothing ? Ptr{Cdouble}(C_NULL) : pointer(hu), length(hu),
                down === nothing ? Ptr{Cdouble}(C_NULL) : pointer(hd), length(hd), mask))
    return r
end

"""
    set_models!(runner, first, models)

Monte-Carlo component tolerances: instances `first`, `first+1`, ... (0-based) take the matrices of
`models[k]` (same circuit topology; the runner must have been created with
`per_instance_matrices=true`) and the freshly constructed state of that model.
"""
function set_models!(r::BatchRunner, first::Integer, models::AbstractVector{<:DiscreteModel})
    hs = [ModelHandle(m) for m in models]
    ptrs = Ptr{Cvoid}[m.h for m in hs]
    GC.@preserve hs check(ccall((:acme_batch_set_matrices, lib), Cint,
        (Ptr{Cvoid}, Clonglong, Clonglong, Ptr{Ptr{Cvoid}}), r.h, first, length(ptrs), ptrs))
    return r
end

function reports(r::BatchRunner)
    reps = Vector{AcmeReport}(undef, r.n)
    check(ccall((:acme_batch_get_report, lib), Cint, (Ptr{Cvoid}, Ptr{AcmeReport}), r.h, reps))
    return reps
end

"""
    run!(runner::BatchRunner, y::Array{Float64,3}, u::Array{Float64,3})
    run!(runner::BatchRunner, u::Array{Float64,3}) -> y

`u` is `nu × T × N`, `y` is `ny × T × N` (Julia's column-major layout of these IS the ABI's
[N][T][nu] layout): slice `[:, :, i]` is exactly the matrix `ACME.run!` takes for instance `i`.
Errors and warnings follow `step!` (src/ACME.jl:688-694) and `checkiosizes` (:625-635).
"""
function checkiosizes(m::DiscreteModel, n::Integer, y::Array{Float64,3}, u::Array{Float64,3})      # src/ACME.jl:625-635
    size(u, 1) == ACME.nu(m) || throw(DimensionMismatch("input matrix has $(size(u,1)) rows, but model has $(ACME.nu(m)) inputs"))
    size(y, 1) == ACME.ny(m) || throw(DimensionMismatch("output matrix has $(size(y,1)) rows, but model has $(ACME.ny(m)) outputs"))
    size(u, 2) == size(y, 2) || throw(DimensionMismatch("input matrix has $(size(u,2)) columns, output matrix has $(size(y,2)) columns"))
    (size(u, 3) == n && size(y, 3) == n) || throw(DimensionMismatch("u and y need one nu × T (ny × T) slice per instance ($n)"))
end

"the policy of `step!` (src/ACME.jl:688-694) on the reports a run left behind; `offset`: instances before this batch"
function checkreports!(r::BatchRunner, offset::Integer=0)
    reps = reports(r)
    bad = findfirst(rep -> rep.first_nonfinite >= 0, reps)
    bad === nothing || error("Failed to converge while solving non-linear equation, got non-finite result. " *
                             "(instance $(offset + bad), sample $(reps[bad].first_nonfinite + 1))")
    nwarn = sum(rep -> rep.n_warn, reps)
    if nwarn > r.warned
        @warn "Failed to converge while solving non-linear equation."
        r.warned = nwarn
    end
    return nothing
end

function run!(r::BatchRunner, y::Array{Float64,3}, u::Array{Float64,3})
    checkiosizes(r.model, r.n, y, u)
    r.showprogress && (r.progress[] = ProgressMeter.Progress(size(u, 2)))     # (as @showprogress for n = 1:size(u, 2))
    GC.@preserve r check(ccall((:acme_batch_run, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Clonglong, Cint, Ptr{Cvoid}),
                r.h, u, y, size(u, 2), ACME_MEM_HOST, C_NULL))
    r.showprogress && (ProgressMeter.finish!(r.progress[]); r.progress[] = nothing)
    return checkreports!(r)
end

function run!(r::BatchRunner, u::Array{Float64,3})
    y = Array{Float64,3}(undef, ACME.ny(r.model), size(u, 2), r.n)
    run!(r, y, u)
    return y
end

"""
    run!(r::BatchRunner, y, u_var, u_const, const_rows)

`run!` with CONSTANT input rows: the rows named in `const_rows` (1-based) keep the value `u_const[k, i]` (`u_const`:
nu x N) for the whole call in instance `i` -- a potentiometer position, a supply voltage -- and `u_var`
(nu_var x T x N) holds the other rows in row order.  Where the reference copies column `n` of a full `u` into `ucur`
sample by sample (src/ACME.jl:672-674), the library puts the full rows together on the device: a sweep over three pot
positions of a four-input model moves a quarter of the bytes over the bus.  Results: those of `run!(r, y, u)` on the
materialised `u`, bit for bit.
"""
function run!(r::BatchRunner, y::Array{Float64,3}, u_var::Array{Float64,3}, u_const::Matrix{Float64}, const_rows)
    nu = ACME.nu(r.model)
    mask = UInt64(0)
    for k in const_rows
        1 <= k <= nu || throw(DimensionMismatch("constant row $k of a model with $nu inputs"))
        mask |= UInt64(1) << (k - 1)
    end
    nuv = nu - count_ones(mask)
    size(u_var, 1) == nuv || throw(DimensionMismatch("u_var has $(size(u_var, 1)) rows, $nuv inputs vary"))
    size(u_const) == (nu, r.n) || throw(DimensionMismatch("u_const must be $nu x $(r.n)"))
    size(u_var, 3) == r.n && size(y, 3) == r.n || throw(DimensionMismatch("u_var and y must hold $(r.n) instances"))
    size(y, 1) == ACME.ny(r.model) && size(y, 2) == size(u_var, 2) ||
        throw(DimensionMismatch("output matrix must be $(ACME.ny(r.model)) x $(size(u_var, 2)) x $(r.n)"))
    GC.@preserve r check(ccall((:acme_batch_run_const, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Culonglong, Ptr{Cdouble}, Clonglong, Cint, Ptr{Cvoid}),
                r.h, u_var, u_const, mask, y, size(u_var, 2), ACME_MEM_HOST, C_NULL))
    return checkreports!(r)
end

# ---- output measurements ---------------------------------------------------------------------------------------
"""
    MeasureSpec(; start=0, length=0, f0=0//1, harmonics=0, rows=())

The window and quantities of an output measurement -- the arguments of `acme_batch_set_measurement`: samples
`start <= n < start + length` counted from arming (`length = 0`: all from `start` on), the fundamental `f0` as a
`Rational` of the sample rate, `harmonics` (0 ... 32) of it, the output `rows` measured (1-based; empty: all).
"""
struct MeasureSpec
    start::Int64
    length::Int64
    f_num::Int64
    f_den::Int64
    harmonics::Int32
    rows::UInt64
end
function MeasureSpec(; start::Integer=0, length::Integer=0, f0::Rational=0//1, harmonics::Integer=0, rows=())
    mask = UInt64(0)
    for k in rows
        1 <= k <= 64 || throw(DimensionMismatch("output row $k: rows 1 ... 64 can be measured"))
        mask |= UInt64(1) << (k - 1)
    end
    return MeasureSpec(start, length, numerator(f0), denominator(f0), harmonics, mask)
end

"""
What `measurement(runner)` returns, per instance and measured row (`rows`, 1-based, ascending): `mean`, `rms`, `min`,
`max` (nrows x N) and `harmonics` (H x nrows x N), the complex amplitudes A_h = (2 / count) sum_m y[m] exp(-j h w m);
`count` samples were measured.  `peak(m)`, `thd(m)`.
"""
struct Measurement
    count::Int
    rows::Vector{Int}
    mean::Matrix{Float64}
    rms::Matrix{Float64}
    min::Matrix{Float64}
    max::Matrix{Float64}
    harmonics::Array{ComplexF64,3}
end
peak(m::Measurement) = max.(abs.(m.min), abs.(m.max))
"total harmonic distortion sqrt(sum_{h >= 2} |A_h|^2) / |A_1| (nrows x N)"
thd(m::Measurement) = dropdims(sqrt.(sum(abs2, m.harmonics[2:end, :, :]; dims=1)) ./ abs.(m.harmonics[1:1, :, :]); dims=1)

"""
    set_measurement!(runner, spec::MeasureSpec)
    set_measurement!(runner; start=0, length=0, f0=0//1, harmonics=0, rows=())

Arm an output measurement (`acme_batch_set_measurement`): from now on every `run!` / `measure!` feeds per instance and
measured output row the mean, RMS, min, max and the complex amplitudes of the fundamental's harmonics over the window
-- on the GPU, in place of the outputs a sweep would otherwise have to keep.  `measure!` then runs without `y`.
"""
function set_measurement!(r::BatchRunner, spec::MeasureSpec)
    check(ccall((:acme_batch_set_measurement, lib), Cint,
                (Ptr{Cvoid}, Clonglong, Clonglong, Clonglong, Clonglong, Cint, Culonglong),
                r.h, spec.start, spec.length, spec.f_num, spec.f_den, spec.harmonics, spec.rows))
    r.meas = spec
    r.spectrum = 0
    r.cross = 0
    r.ensemble = (0, 0)
    r.histogram = 0
    r.events = (0, 0)
    return r
end
function set_measurement!(r::BatchRunner; f_den=nothing, f_num=nothing, kwargs...)
    f_num === nothing && f_den === nothing && return set_measurement!(r, MeasureSpec(; kwargs...))
    (f_num === nothing || f_den === nothing) && error("per-instance fundamentals need both f_den and f_num")
    haskey(kwargs, :f0) && error("f0 and f_den / f_num exclude each other")
    return set_measurement!(r, MeasureSpec(; f0=0 // Int64(f_den), kwargs...), Int64(f_den), convert(Vector{Int64}, f_num))
end

"""
    set_measurement!(runner; start=0, length=0, harmonics=0, rows=(), f_den, f_num::Vector{Int64})

Arm a measurement with a fundamental PER INSTANCE (`acme_batch_set_measurement_per_instance`): instance `i` correlates with
`f_num[i] / f_den` of the sample rate -- the batch a per-instance sine source drives as a frequency sweep is measured as
one.  A window of `length = f_den` samples holds whole periods of every instance's fundamental.
"""
function set_measurement!(r::BatchRunner, spec::MeasureSpec, f_den::Int64, f_num::Vector{Int64})
    length(f_num) == r.n || throw(DimensionMismatch("f_num needs one entry per instance ($(r.n))"))
    GC.@preserve f_num check(ccall((:acme_batch_set_measurement_per_instance, lib), Cint,
                (Ptr{Cvoid}, Clonglong, Clonglong, Clonglong, Ptr{Clonglong}, Cint, Culonglong),
                r.h, spec.start, spec.length, f_den, f_num, spec.harmonics, spec.rows))
    r.meas = spec
    r.spectrum = 0
    r.cross = 0
    r.ensemble = (0, 0)
    r.histogram = 0
    r.events = (0, 0)
    return r
end

"""
    set_measurement_bins!(runner, coef::Matrix{<:Integer}, f_den, f_num::Matrix{Int64}; start=0, length=0, rows=())

Arm a measurement whose bins are integer combinations of per-instance tones (`acme_batch_set_measurement_bins`): `f_num` is
N x tones (column j: tone j of every instance), `coef` is tones x bins (column b: the coefficients of bin b), and bin `b` of
instance `i` correlates with `(sum_j coef[j, b] f_num[i, j]) mod f_den` of `f_den` -- the sum and difference products of a
two-tone intermodulation test.  `measurement(runner).harmonics[b, row, i]` is then the complex amplitude of bin `b`.  A
combination below zero reads the mirrored line (the conjugate amplitude): choose signs that give a positive frequency.
"""
function set_measurement_bins!(r::BatchRunner, coef::Matrix{<:Integer}, f_den::Integer, f_num::Matrix{Int64};
                               start::Integer=0, length::Integer=0, rows=())
    tones, bins = size(coef)
    size(f_num) == (r.n, tones) || throw(DimensionMismatch("f_num must be N x tones ($(r.n) x $tones)"))
    1 <= tones <= ACME_MAX_SOURCE_TONES || error("1 ... $ACME_MAX_SOURCE_TONES tones")
    spec = MeasureSpec(; start=start, length=length, f0=0 // Int(f_den), harmonics=bins, rows=rows)
    c = convert(Matrix{Cint}, coef)         # (column-major tones x bins = the ABI's [bins][tones])
    GC.@preserve f_num c check(ccall((:acme_batch_set_measurement_bins, lib), Cint,
                (Ptr{Cvoid}, Clonglong, Clonglong, Clonglong, Cint, Ptr{Clonglong}, Cint, Ptr{Cint}, Culonglong),
                r.h, spec.start, spec.length, f_den, tones, f_num, bins, c, spec.rows))
    r.meas = spec
    r.spectrum = 0
    r.cross = 0
    r.ensemble = (0, 0)
    r.histogram = 0
    r.events = (0, 0)
    return r
end

"""
    measurement_plan(runner) -> (groups, chunk, perm, wave_group)

The plan of the armed per-instance measurement (`acme_batch_get_measurement_plan`): distinct frequencies, samples per
step, lane slot -> pair (0-based), and per wave of 64 slots its one group or -1 (a mixed wave).
"""
function measurement_plan(r::BatchRunner)
    spec = r.meas
    spec === nothing && error("no measurement is armed")
    ny = ACME.ny(r.model)
    P = r.n * (spec.rows == 0 ? min(ny, 64) : count_ones(spec.rows))
    perm, wg = Vector{Int64}(undef, P), Vector{Cint}(undef, cld(P, 64))
    groups, chunk = Ref{Clonglong}(0), Ref{Clonglong}(0)
    check(ccall((:acme_batch_get_measurement_plan, lib), Cint,
                (Ptr{Cvoid}, Ref{Clonglong}, Ref{Clonglong}, Ptr{Clonglong}, Ptr{Cint}), r.h, groups, chunk, perm, wg))
    return (groups=groups[], chunk=chunk[], perm=perm, wave_group=wg)
end

"switch the measurement off (`acme_batch_clear_measurement`)"
function clear_measurement!(r::BatchRunner)
    check(ccall((:acme_batch_clear_measurement, lib), Cint, (Ptr{Cvoid},), r.h))
    r.meas = nothing
    r.spectrum = 0
    r.cross = 0
    r.ensemble = (0, 0)
    r.histogram = 0
    r.events = (0, 0)
    return r
end

"zero the accumulators and restart the window's clock (`acme_batch_reset_measurement`)"
reset_measurement!(r::BatchRunner) = (check(ccall((:acme_batch_reset_measurement, lib), Cint, (Ptr{Cvoid},), r.h)); r)

"the armed measurement's results so far (`acme_batch_get_measurement`)"
function measurement(r::BatchRunner)
    spec = r.meas
    spec === nothing && error("no measurement is armed")
    ny = ACME.ny(r.model)
    rows = spec.rows == 0 ? collect(1:min(ny, 64)) : [k for k in 1:64 if (spec.rows >> (k - 1)) & 1 == 1]
    H = Int(spec.harmonics)
    out = Array{Float64,3}(undef, 4 + 2H, length(rows), r.n)        # the ABI's [N][nrows][4 + 2H]
    count = Ref{Clonglong}(0)
    check(ccall((:acme_batch_get_measurement, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Clonglong}), r.h, out, count))
    return Measurement(count[], rows, out[1, :, :], out[2, :, :], out[3, :, :], out[4, :, :],
                       complex.(out[5:2:end, :, :], out[6:2:end, :, :]))
end

"""
    set_measurement_series!(runner, win; hop=win, windows=1)

Turn the armed measurement's one window into a series (`acme_batch_set_measurement_series`): `windows` windows of `win`
samples, one every `hop` samples, window `w` (0-based) over `start + w hop <= n < start + w hop + win` -- all accumulated in
the same pass, each bit for bit the single window armed there.  Needs a measurement armed with `length = 0` that has not
been fed yet.
"""
function set_measurement_series!(r::BatchRunner, win::Integer; hop::Integer=win, windows::Integer=1)
    r.meas === nothing && error("no measurement is armed")
    check(ccall((:acme_batch_set_measurement_series, lib), Cint, (Ptr{Cvoid}, Clonglong, Clonglong, Clonglong),
                r.h, win, hop, windows))
    return r
end

"""
    measurement_series(runner, first, n) -> Vector{Measurement}

The windows `first ... first + n - 1` (0-based) of the series so far (`acme_batch_get_measurement_series`), each a
`Measurement` with its own `count`; a window never reached has count 0.
"""
function measurement_series(r::BatchRunner, first::Integer, n::Integer)
    spec = r.meas
    spec === nothing && error("no measurement is armed")
    ny = ACME.ny(r.model)
    rows = spec.rows == 0 ? collect(1:min(ny, 64)) : [k for k in 1:64 if (spec.rows >> (k - 1)) & 1 == 1]
    H = Int(spec.harmonics)
    out = Array{Float64,4}(undef, 4 + 2H, length(rows), r.n, n)     # the ABI's [n][N][nrows][4 + 2H]
    counts = Vector{Clonglong}(undef, n)
    check(ccall((:acme_batch_get_measurement_series, lib), Cint,
                (Ptr{Cvoid}, Clonglong, Clonglong, Ptr{Cdouble}, Ptr{Clonglong}), r.h, first, n, out, counts))
    return [Measurement(counts[w], rows, out[1, :, :, w], out[2, :, :, w], out[3, :, :, w], out[4, :, :, w],
                        complex.(out[5:2:end, :, :, w], out[6:2:end, :, :, w])) for w in 1:n]
end

"""
    set_measurement_fold!(runner; period=0, period_i=nothing)

Fold the armed measurement's window onto one period (`acme_batch_set_measurement_fold`, synchronous averaging): slot
`m mod period` of the window-relative sample `m` accumulates y, per instance and measured row.  `period` samples for every
instance, or `period_i::Vector{Int64}`, one period per instance (1 ... 65536).  Needs an armed measurement that has not been
fed yet; not together with a series.
"""
function set_measurement_fold!(r::BatchRunner; period::Integer=0, period_i=nothing)
    r.meas === nothing && error("no measurement is armed")
    per = period_i === nothing ? Int64[] : convert(Vector{Int64}, period_i)
    period_i === nothing || length(per) == r.n || throw(DimensionMismatch("period_i needs one entry per instance ($(r.n))"))
    GC.@preserve per check(ccall((:acme_batch_set_measurement_fold, lib), Cint, (Ptr{Cvoid}, Clonglong, Ptr{Clonglong}),
                r.h, period, ptr_or_null(per)))
    return r
end

"""
    measurement_fold(runner; sums=false) -> (mean, period, count)

The fold so far (`acme_batch_get_measurement_fold`): `mean` is Pmax x nrows x N, slot `s` (1-based) of instance `i` the mean of
the window's samples `m` with `m mod period[i] == s - 1`; slots no sample has reached, and those beyond `period[i]`, are NaN.
`sums=true`: `mean` holds the slots' sums, undivided (`acme_batch_get_measurement_fold_sums`).
"""
function measurement_fold(r::BatchRunner; sums::Bool=false)
    spec = r.meas
    spec === nothing && error("no measurement is armed")
    ny = ACME.ny(r.model)
    nrows = spec.rows == 0 ? min(ny, 64) : count_ones(spec.rows)
    period = Vector{Clonglong}(undef, r.n)
    count = Ref{Clonglong}(0)
    check(ccall((:acme_batch_get_measurement_fold, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Clonglong}, Ptr{Clonglong}),
                r.h, C_NULL, period, count))
    mean = Array{Float64,3}(undef, maximum(period; init=0), nrows, r.n)     # the ABI's [N][nrows][Pmax]
    if sums
        check(ccall((:acme_batch_get_measurement_fold_sums, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), r.h, mean))
    else
        check(ccall((:acme_batch_get_measurement_fold, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Clonglong}, Ptr{Clonglong}),
                    r.h, mean, C_NULL, C_NULL))
    end
    return (mean=mean, period=period, count=count[])
end

"""
    set_measurement_spectrum!(runner, nfft; hop=nfft ÷ 2, window=nothing)

Welch-averaged periodograms of the armed measurement's window (`acme_batch_set_measurement_spectrum`): segments of `nfft`
samples (a power of two, 64 ... 4096), one every `hop`, each multiplied by `window::Vector{Float64}` (`nothing`: the
periodic Hann window; `:rect`: all ones), transformed on the device and |X_k|^2 accumulated per instance, measured row and
bin.  Needs an armed measurement that has not been fed yet; not together with a series.
"""
function set_measurement_spectrum!(r::BatchRunner, nfft::Integer; hop::Integer=nfft ÷ 2, window=nothing)
    r.meas === nothing && error("no measurement is armed")
    w = window === :rect ? Float64[] :
        window === nothing ? [0.5 - 0.5 * cos(2pi * j / nfft) for j in 0:nfft-1] : convert(Vector{Float64}, window)
    window === :rect || length(w) == nfft || throw(DimensionMismatch("the window needs $nfft values"))
    GC.@preserve w check(ccall((:acme_batch_set_measurement_spectrum, lib), Cint,
                (Ptr{Cvoid}, Clonglong, Clonglong, Ptr{Cdouble}), r.h, nfft, hop, ptr_or_null(w)))
    r.spectrum = Int(nfft)
    return r
end

"""
    measurement_spectrum(runner; sums=false) -> (power, segments, count, window, table)

The spectrum so far (`acme_batch_get_measurement_spectrum`): `power` is (nfft ÷ 2 + 1) x nrows x N, the mean over `segments`
segments of |FFT(w x)|^2, unscaled (NaN while `segments == 0`); `sums=true`: the bins' sums, undivided
(`acme_batch_get_measurement_spectrum_sums`).  `window` (nfft) and `table` (2 x nfft ÷ 2: cos, -sin of 2 pi k / nfft) are
what the kernel uses (`acme_batch_get_measurement_spectrum_table`).
"""
function measurement_spectrum(r::BatchRunner; sums::Bool=false)
    spec = r.meas
    (spec === nothing || r.spectrum == 0) && error("no measurement spectrum is set")
    ny = ACME.ny(r.model)
    nrows = spec.rows == 0 ? min(ny, 64) : count_ones(spec.rows)
    nfft = r.spectrum
    segments, count = Ref{Clonglong}(0), Ref{Clonglong}(0)
    power = Array{Float64,3}(undef, nfft ÷ 2 + 1, nrows, r.n)       # the ABI's [N][nrows][nfft / 2 + 1]
    check(ccall((:acme_batch_get_measurement_spectrum, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Clonglong}, Ptr{Clonglong}),
                r.h, power, segments, count))
    if sums
        check(ccall((:acme_batch_get_measurement_spectrum_sums, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), r.h, power))
    end
    window, table = Vector{Float64}(undef, nfft), Matrix{Float64}(undef, 2, nfft ÷ 2)
    check(ccall((:acme_batch_get_measurement_spectrum_table, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), r.h, window, table))
    return (power=power, segments=segments[], count=count[], window=window, table=table)
end

"""
    set_measurement_cross!(runner, in_row, nfft; hop=nfft ÷ 2, window=nothing)

The cross-spectrum of input row `in_row` (1-based) and the measured output rows over the armed measurement's window
(`acme_batch_set_measurement_cross`): segments of `nfft` samples (a power of two, 64 ... 4096), one every `hop`, each multiplied
by `window::Vector{Float64}` (`nothing`: the periodic Hann window; `:rect`: all ones); the input row as the run sees it at the
base rate and a measured row go through one complex transform on the device, and |X|^2, |Y|^2 and conj(X) Y are accumulated
per instance, measured row and bin.  Needs an armed measurement that has not been fed yet; not together with a series.
"""
function set_measurement_cross!(r::BatchRunner, in_row::Integer, nfft::Integer; hop::Integer=nfft ÷ 2, window=nothing)
    r.meas === nothing && error("no measurement is armed")
    w = window === :rect ? Float64[] :
        window === nothing ? [0.5 - 0.5 * cos(2pi * j / nfft) for j in 0:nfft-1] : convert(Vector{Float64}, window)
    window === :rect || length(w) == nfft || throw(DimensionMismatch("the window needs $nfft values"))
    GC.@preserve w check(ccall((:acme_batch_set_measurement_cross, lib), Cint,
                (Ptr{Cvoid}, Cint, Clonglong, Clonglong, Ptr{Cdouble}), r.h, in_row - 1, nfft, hop, ptr_or_null(w)))
    r.cross = Int(nfft)
    return r
end

"""
    measurement_cross(runner; sums=false) -> (sxx, syy, sxy, segments, count, window, table)

The cross-spectrum so far (`acme_batch_get_measurement_cross`): `sxx`, `syy` (real) and `sxy` (complex) are
(nfft ÷ 2 + 1) x nrows x N, the means over `segments` segments of |X|^2, |Y|^2 and conj(X) Y, unscaled (NaN while
`segments == 0`); `sums=true`: the bins' sums, undivided (`acme_batch_get_measurement_cross_sums`).  The H1 estimate of the
frequency response is `sxy ./ sxx`, the coherence `abs2.(sxy) ./ (sxx .* syy)`.  `window` (nfft) and `table` (2 x nfft ÷ 2) are
what the kernel uses (`acme_batch_get_measurement_cross_table`).
"""
function measurement_cross(r::BatchRunner; sums::Bool=false)
    spec = r.meas
    (spec === nothing || r.cross == 0) && error("no measurement cross-spectrum is set")
    ny = ACME.ny(r.model)
    nrows = spec.rows == 0 ? min(ny, 64) : count_ones(spec.rows)
    nfft = r.cross
    segments, count = Ref{Clonglong}(0), Ref{Clonglong}(0)
    out = Array{Float64,4}(undef, nfft ÷ 2 + 1, 4, nrows, r.n)       # the ABI's [N][nrows][4][nfft / 2 + 1]
    check(ccall((:acme_batch_get_measurement_cross, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Clonglong}, Ptr{Clonglong}),
                r.h, out, segments, count))
    if sums
        check(ccall((:acme_batch_get_measurement_cross_sums, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), r.h, out))
    end
    window, table = Vector{Float64}(undef, nfft), Matrix{Float64}(undef, 2, nfft ÷ 2)
    check(ccall((:acme_batch_get_measurement_cross_table, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), r.h, window, table))
    return (sxx=out[:, 1, :, :], syy=out[:, 2, :, :], sxy=complex.(out[:, 3, :, :], out[:, 4, :, :]),
            segments=segments[], count=count[], window=window, table=table)
end

"""
    set_measurement_target!(runner, target; which=nothing, lag=nothing, preemphasis=0.0)

Compare the armed measurement's window with a waveform of the caller's (`acme_batch_set_measurement_target`): per instance
and measured row the sums of (y - t)^2, t^2, y t and t, the peak |y - t| and, behind the pre-emphasis filter
1 - `preemphasis` z^-1, the sums of the filtered error's and target's squares.  `target` is `P`, `P x nrows` or
`P x nrows x K` (K <= 64 looped recordings, one waveform per measured row); `which::Vector` (0-based, one per
instance, `nothing`: 0) selects the recording instance `i` is compared with, `lag::Vector` (0 ... P - 1, `nothing`: 0) the
number of samples it reads the target ahead.  Needs an armed measurement that has not been fed yet; not together with a series.
"""
function set_measurement_target!(r::BatchRunner, target::AbstractArray{<:Real}; which=nothing, lag=nothing,
                                 preemphasis::Real=0.0)
    spec = r.meas
    spec === nothing && error("no measurement is armed")
    ny = ACME.ny(r.model)
    nrows = spec.rows == 0 ? min(ny, 64) : count_ones(spec.rows)
    t = convert(Array{Float64}, target)
    ndims(t) == 1 && (t = repeat(t, 1, nrows))
    ndims(t) == 2 && (t = reshape(t, size(t, 1), size(t, 2), 1))
    (ndims(t) == 3 && size(t, 2) == nrows) || throw(DimensionMismatch("the target must be P, P x $nrows or P x $nrows x K"))
    1 <= size(t, 3) <= ACME_MAX_TARGETS || throw(DimensionMismatch("1 ... $ACME_MAX_TARGETS targets"))
    wh = perinstance(Cint, which, r.n)
    lg = perinstance(Int64, lag, r.n)
    GC.@preserve t wh lg check(ccall((:acme_batch_set_measurement_target, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Clonglong, Clonglong, Ptr{Cint}, Ptr{Clonglong}, Cdouble),
                r.h, t, size(t, 3), size(t, 1), ptr_or_null(wh), ptr_or_null(lg), preemphasis))
    return r
end

"""
    measurement_target(runner) -> (see, stt, syt, st, emax, pee, ptt, count)

The residual against the target so far (`acme_batch_get_measurement_target`): the seven chains, undivided, `nrows x N` each --
the error-to-signal ratio is `see ./ stt`, behind the pre-emphasis `pee ./ ptt`, the least-squares gain `syt ./ stt` -- and
the number of samples measured.
"""
function measurement_target(r::BatchRunner)
    spec = r.meas
    spec === nothing && error("no measurement is armed")
    ny = ACME.ny(r.model)
    nrows = spec.rows == 0 ? min(ny, 64) : count_ones(spec.rows)
    count = Ref{Clonglong}(0)
    out = Array{Float64,3}(undef, 7, nrows, r.n)                     # the ABI's [N][nrows][7]
    check(ccall((:acme_batch_get_measurement_target, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Clonglong}), r.h, out, count))
    return (see=out[1, :, :], stt=out[2, :, :], syt=out[3, :, :], st=out[4, :, :], emax=out[5, :, :], pee=out[6, :, :],
            ptt=out[7, :, :], count=count[])
end

"""
    set_measurement_weighting!(runner, sos)

Put a cascade of second-order sections ahead of the armed measurement (`acme_batch_set_measurement_weighting`): every form
then reads the weighted output, filtered from the first sample after arming on (transposed direct form II, no fused
multiply-add).  `sos` is `S x 5` with the rows `b0 b1 b2 a1 a2`, or `S x 6` in the layout `b0 b1 b2 a0 a1 a2` with
`a0 == 1`; `S <= 8`.  Needs an armed measurement that has not been fed yet.
"""
function set_measurement_weighting!(r::BatchRunner, sos::AbstractMatrix{<:Real})
    r.meas === nothing && error("no measurement is armed")
    a = convert(Matrix{Float64}, sos)
    if size(a, 2) == 6
        all(a[:, 4] .== 1.0) || throw(ArgumentError("second-order sections with six columns must have a0 == 1"))
        a = a[:, [1, 2, 3, 5, 6]]
    end
    (size(a, 2) == 5 && 1 <= size(a, 1) <= ACME_MAX_WEIGHTING_SECTIONS) ||
        throw(DimensionMismatch("second-order sections must be S x 5 or S x 6, S = 1 ... $ACME_MAX_WEIGHTING_SECTIONS"))
    t = Matrix{Float64}(transpose(a))                                # the ABI's [S][5]
    GC.@preserve t check(ccall((:acme_batch_set_measurement_weighting, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint),
                               r.h, t, size(a, 1)))
    return r
end

"""
    measurement_weighting(runner) -> Matrix{Float64}

The cascade of the armed measurement as set (`acme_batch_get_measurement_weighting`): `S x 5`, the rows `b0 b1 b2 a1 a2`.
"""
function measurement_weighting(r::BatchRunner)
    S = Ref{Cint}(0)
    out = zeros(Float64, 5, ACME_MAX_WEIGHTING_SECTIONS)             # the ABI's [8][5]
    check(ccall((:acme_batch_get_measurement_weighting, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Cint}), r.h, out, S))
    return Matrix{Float64}(transpose(out[:, 1:S[]]))
end

"""
    set_measurement_ensemble!(runner; groups=nothing, n_groups=nothing, stride=1)

Reduce the armed measurement's window ACROSS the instances (`acme_batch_set_measurement_ensemble`): per group, measured row
and recorded sample the sum, the sum of squares, the minimum and the maximum over the group's members, in ascending instance
order, and the instances that set the extremes.  `groups::Vector` (0-based, one per instance, `-1`: in no group; `nothing`:
every instance in group 0), `n_groups` the number of groups (`nothing`: the largest index + 1), every `stride`-th window
sample recorded.  Needs an armed measurement with a bounded window (`length > 0`) that has not been fed yet; not together
with a series.
"""
function set_measurement_ensemble!(r::BatchRunner; groups=nothing, n_groups=nothing, stride::Integer=1)
    r.meas === nothing && error("no measurement is armed")
    g = perinstance(Cint, groups, r.n)
    G = n_groups === nothing ? max(isempty(g) ? 1 : Int(maximum(g)) + 1, 1) : Int(n_groups)
    GC.@preserve g check(ccall((:acme_batch_set_measurement_ensemble, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}, Cint, Clonglong),
                               r.h, ptr_or_null(g), G, stride))
    r.ensemble = (G, Int(stride))
    return r
end

"""
    measurement_ensemble(runner) -> (sum, sumsq, min, max, argmin, argmax, members, filled)

The statistics across the groups' instances so far (`acme_batch_get_measurement_ensemble`), for the groups and the stride
that `set_measurement_ensemble!` set (the runner keeps both and sizes the arrays from them): the four chains, undivided,
and the 0-based instances that set the extremes (`-1`: no member), `E x nrows x G` each with `E = cld(length, stride)`;
`members` the groups' sizes; `filled` the number of slots recorded so far.
"""
function measurement_ensemble(r::BatchRunner)
    spec = r.meas
    n_groups, stride = r.ensemble
    (spec === nothing || n_groups == 0) && error("no measurement ensemble is set")
    ny = ACME.ny(r.model)
    nrows = spec.rows == 0 ? min(ny, 64) : count_ones(spec.rows)
    E = cld(spec.length, stride)
    out = Array{Float64,4}(undef, 4, E, nrows, n_groups)             # the ABI's [G][nrows][E][4]
    arg = Array{Int64,4}(undef, 2, E, nrows, n_groups)               # ... and [G][nrows][E][2]
    members = zeros(Int64, n_groups)
    filled = Ref{Clonglong}(0)
    check(ccall((:acme_batch_get_measurement_ensemble, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Clonglong}, Ptr{Clonglong}, Ref{Clonglong}), r.h, out, arg, members, filled))
    return (sum=out[1, :, :, :], sumsq=out[2, :, :, :], min=out[3, :, :, :], max=out[4, :, :, :],
            argmin=arg[1, :, :, :], argmax=arg[2, :, :, :], members=members, filled=filled[])
end

"""
    set_measurement_histogram!(runner, bins, lo, hi; mode=:signed)

Count how the amplitude of every measured row is distributed (`acme_batch_set_measurement_histogram`): `bins` equal bins over
`[lo, hi)` per instance plus the samples below, at or above the range and not a number.  `lo`, `hi`: two numbers, or two
vectors with one entry per instance; `mode` `:signed` or `:abs` (the magnitude is binned).  Needs an armed measurement that has
not been fed yet; not together with a series.
"""
function set_measurement_histogram!(r::BatchRunner, bins::Integer, lo, hi; mode::Symbol=:signed)
    r.meas === nothing && error("no measurement is armed")
    mode in (:signed, :abs) || throw(ArgumentError("mode must be :signed or :abs"))
    (lo isa Number) == (hi isa Number) || throw(ArgumentError("lo and hi are both numbers or both vectors"))
    m = mode === :abs ? ACME_HIST_ABS : ACME_HIST_SIGNED
    if lo isa Number
        check(ccall((:acme_batch_set_measurement_histogram, lib), Cint,
                    (Ptr{Cvoid}, Cint, Cint, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}), r.h, bins, m, lo, hi, C_NULL, C_NULL))
    else
        l, h = perinstance(Float64, lo, r.n), perinstance(Float64, hi, r.n)
        GC.@preserve l h check(ccall((:acme_batch_set_measurement_histogram, lib), Cint,
                    (Ptr{Cvoid}, Cint, Cint, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}), r.h, bins, m, 0.0, 0.0, pointer(l), pointer(h)))
    end
    r.histogram = Int(bins)
    return r
end

"""
    measurement_histogram(runner) -> (counts, under, over, nan, lo, hi, scale, count)

The counters so far (`acme_batch_get_measurement_histogram`), for the bins that `set_measurement_histogram!` set (the runner
keeps them and sizes the arrays): `counts` `B x nrows x N`, `under`, `over`, `nan` `nrows x N`, the instances' ranges and
scales `B / (hi - lo)` as stored, and `count`, the samples measured -- every pair's counters sum to it.
"""
function measurement_histogram(r::BatchRunner)
    spec = r.meas
    B = r.histogram
    (spec === nothing || B == 0) && error("no measurement histogram is set")
    ny = ACME.ny(r.model)
    nrows = spec.rows == 0 ? min(ny, 64) : count_ones(spec.rows)
    raw = Array{Int64,3}(undef, B + 3, nrows, r.n)                   # the ABI's [N][nrows][B + 3]
    range = Matrix{Float64}(undef, 3, r.n)                           # ... and [N][3]
    count = Ref{Clonglong}(0)
    check(ccall((:acme_batch_get_measurement_histogram, lib), Cint,
                (Ptr{Cvoid}, Ptr{Clonglong}, Ptr{Cdouble}, Ref{Clonglong}), r.h, raw, range, count))
    return (counts=raw[2:B + 1, :, :], under=raw[1, :, :], over=raw[B + 2, :, :], nan=raw[B + 3, :, :],
            lo=range[1, :], hi=range[2, :], scale=range[3, :], count=count[])
end

"""
    set_measurement_events!(runner, lo, hi; slots=8)

Record when every measured row crosses levels (`acme_batch_set_measurement_events`): `lo` and `hi` are `N x C` matrices (or
vectors of `C` levels that serve every instance), level `c` of instance `i` the band `[lo[i, c], hi[i, c]]` -- `lo == hi` a plain
comparator, `lo < hi` a Schmitt trigger; `slots` the first events recorded per direction.  Needs an armed measurement that has
not been fed yet; not together with a series.
"""
function set_measurement_events!(r::BatchRunner, lo, hi; slots::Integer=8)
    r.meas === nothing && error("no measurement is armed")
    full(a) = a isa AbstractVector ? repeat(reshape(Float64.(a), 1, :), r.n, 1) : Matrix{Float64}(a)
    l, h = full(lo), full(hi)                                        # N x C column-major: the ABI's [C][N]
    size(l) == size(h) && size(l, 1) == r.n || throw(DimensionMismatch("lo and hi are N x C matrices, or vectors of C levels"))
    nc = size(l, 2)
    GC.@preserve l h check(ccall((:acme_batch_set_measurement_events, lib), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint), r.h, nc, pointer(l), pointer(h), slots))
    r.events = (nc, Int(slots))
    return r
end

"""
    measurement_events(runner) -> (counts, idx, ab, count)

The events so far (`acme_batch_get_measurement_events`), for the levels and slots that `set_measurement_events!` set (the runner
keeps them and sizes the arrays): `counts` `5 x C x nrows x N` (RISE, FALL, HIGH, LOW, UNKNOWN), `idx` `(E + 1) x 2 x C x nrows x N`
the window samples `m` of the first `E` and the last event of either direction (rises, then falls; -1: empty), `ab`
`2 x (E + 1) x 2 x C x nrows x N` their `v[m - 1]` and `v[m]`, and `count`, the samples measured.  The time of an event to a
fraction of a sample is `(m - 1) + (thr - a) / (b - a)` with `thr` the level's `hi` for a rise and `lo` for a fall.
"""
function measurement_events(r::BatchRunner)
    spec = r.meas
    nc, E = r.events
    (spec === nothing || nc == 0) && error("no measurement events are set")
    ny = ACME.ny(r.model)
    nrows = spec.rows == 0 ? min(ny, 64) : count_ones(spec.rows)
    counts = Array{Int64,4}(undef, 5, nc, nrows, r.n)                 # the ABI's [N][nrows][C][5]
    idx = Array{Int64,5}(undef, E + 1, 2, nc, nrows, r.n)             # ... [N][nrows][C][2][E + 1]
    ab = Array{Float64,6}(undef, 2, E + 1, 2, nc, nrows, r.n)         # ... and [N][nrows][C][2][E + 1][2]
    count = Ref{Clonglong}(0)
    check(ccall((:acme_batch_get_measurement_events, lib), Cint,
                (Ptr{Cvoid}, Ptr{Clonglong}, Ptr{Clonglong}, Ptr{Cdouble}, Ref{Clonglong}), r.h, counts, idx, ab, count))
    return (counts=counts, idx=idx, ab=ab, count=count[])
end

"""
    measure!(runner, u::Array{Float64,3})

`run!` without outputs: advance the instances over `u` (`nu × T × N`) and only feed the armed measurement -- y = NULL,
nothing of the outputs is written, staged or copied back.
"""
function measure!(r::BatchRunner, u::Array{Float64,3})
    r.meas === nothing && error("measure! needs an armed measurement (set_measurement!)")
    size(u, 1) == ACME.nu(r.model) || throw(DimensionMismatch("input matrix has $(size(u,1)) rows, but model has $(ACME.nu(r.model)) inputs"))
    size(u, 3) == r.n || throw(DimensionMismatch("u needs one nu × T slice per instance ($(r.n))"))
    GC.@preserve r check(ccall((:acme_batch_run, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Clonglong, Cint, Ptr{Cvoid}),
                r.h, u, C_NULL, size(u, 2), ACME_MEM_HOST, C_NULL))
    checkreports!(r)
    return r
end

# ---- sources: input rows generated on the device -----------------------------------------------------------------
# a per-instance parameter as the ABI takes it: nothing -> NULL (the default for every instance), a number -> N copies
perinstance(::Type{T}, ::Nothing, n) where {T} = T[]
perinstance(::Type{T}, v::Number, n) where {T} = fill(T(v), n)
function perinstance(::Type{T}, v::AbstractVector, n) where {T}
    length(v) == n || throw(DimensionMismatch("per-instance source parameters need $n values"))
    return convert(Vector{T}, v)
end
ptr_or_null(v::Vector{T}) where {T} = isempty(v) ? Ptr{T}(C_NULL) : pointer(v)

"""
    set_source!(runner, row, :const; offset=nothing)
    set_source!(runner, row, :sine; f_den, f_num=nothing, phase=nothing, amp=nothing, offset=nothing)
    set_source!(runner, row, :table; table, amp=nothing, offset=nothing)

Give input row `row` (1-based) a source (`acme_batch_set_source_*`): the library generates the row on the device -- at
source clock n (base-rate samples since the first source was armed) instance i gets `offset[i]`,
`fma(amp[i], sin(2π κ / f_den), offset[i])` with κ = (f_num[i] n + phase[i]) mod f_den reduced exactly in integers, or
`fma(amp[i], table[n mod P + 1], offset[i])`.  Parameters: `nothing` (amp 1, the others 0), a number, or N values.
`run_sources!` then runs without these rows; its results are those of `run!` on `render_sources`' array, bit for bit.
"""
function set_source!(r::BatchRunner, row::Integer, kind::Symbol; f_den::Integer=0, f_num=nothing, phase=nothing,
                     table=nothing, amp=nothing, offset=nothing)
    a, o = perinstance(Cdouble, amp, r.n), perinstance(Cdouble, offset, r.n)
    if kind === :const
        GC.@preserve o check(ccall((:acme_batch_set_source_const, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}), r.h, row - 1, ptr_or_null(o)))
    elseif kind === :sine
        f, p = perinstance(Clonglong, f_num, r.n), perinstance(Clonglong, phase, r.n)
        GC.@preserve f p a o check(ccall((:acme_batch_set_source_sine, lib), Cint,
                    (Ptr{Cvoid}, Cint, Clonglong, Ptr{Clonglong}, Ptr{Clonglong}, Ptr{Cdouble}, Ptr{Cdouble}),
                    r.h, row - 1, f_den, ptr_or_null(f), ptr_or_null(p), ptr_or_null(a), ptr_or_null(o)))
    elseif kind === :table
        table === nothing && error("a table source needs a table")
        w = convert(Vector{Cdouble}, table)
        GC.@preserve w a o check(ccall((:acme_batch_set_source_table, lib), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Clonglong, Ptr{Cdouble}, Ptr{Cdouble}),
                    r.h, row - 1, w, length(w), ptr_or_null(a), ptr_or_null(o)))
    else
        error("unknown source kind $kind: :const, :sine or :table")
    end
    push!(r.sources, Int(row))
    return r
end

"""
    set_source_multisine!(runner, row, f_den, f_num::Matrix{Int64}; phase=nothing, amp=nothing, offset=nothing)

Give input row `row` (1-based) a sum of 1 ... 4 sines (`acme_batch_set_source_multisine`): `f_num`, `phase` (`Matrix{Int64}`)
and `amp` (`Matrix{Float64}`) are N x tones (column k: tone k of every instance), `offset` as for `set_source!`.  The row's
value is one fma chain in tone order from `offset[i]`; one tone is the `:sine` row bit for bit.
"""
function set_source_multisine!(r::BatchRunner, row::Integer, f_den::Integer, f_num::Matrix{Int64};
                               phase::Union{Nothing,Matrix{Int64}}=nothing, amp::Union{Nothing,Matrix{Float64}}=nothing, offset=nothing)
    tones = size(f_num, 2)
    size(f_num, 1) == r.n || throw(DimensionMismatch("f_num must be N x tones"))
    (phase === nothing || size(phase) == size(f_num)) && (amp === nothing || size(amp) == size(f_num)) ||
        throw(DimensionMismatch("phase and amp must have the size of f_num"))
    p = phase === nothing ? Clonglong[] : vec(phase)
    a = amp === nothing ? Cdouble[] : vec(amp)
    o = perinstance(Cdouble, offset, r.n)
    GC.@preserve f_num p a o check(ccall((:acme_batch_set_source_multisine, lib), Cint,
                (Ptr{Cvoid}, Cint, Clonglong, Cint, Ptr{Clonglong}, Ptr{Clonglong}, Ptr{Cdouble}, Ptr{Cdouble}),
                r.h, row - 1, f_den, tones, f_num, ptr_or_null(p), ptr_or_null(a), ptr_or_null(o)))
    push!(r.sources, Int(row))
    return r
end

"""
    set_source_noise!(runner, row; dist=:gaussian, hold=1, stream=nothing, amp=nothing, offset=nothing)

Give input row `row` (1-based) a noise source (`acme_batch_set_source_noise`): `fma(amp[i], d, offset[i])` with d an
independent, reproducible random draw per (stream[i], row, n div hold) -- counter based (Philox4x32-10), so the value at source
clock n depends on nothing generated before, on no call boundary and on no device.  `dist = :uniform`: d in (-1, 1), never 0,
variance 1/3; `dist = :gaussian`: d standard normal (Box-Muller, one draw per sample).  `hold` (1 ... 2^31 - 1): the draw is
held over blocks of `hold` samples aligned to the clock.  `stream`: N `Int64` (read as unsigned 64-bit values), or `nothing`:
instance i (0-based) takes stream i.  `amp`, `offset` as for `set_source!`.
"""
function set_source_noise!(r::BatchRunner, row::Integer; dist::Symbol=:gaussian, hold::Integer=1, stream=nothing, amp=nothing, offset=nothing)
    d = dist === :gaussian ? ACME_NOISE_GAUSSIAN : dist === :uniform ? ACME_NOISE_UNIFORM : error("unknown noise distribution $dist: :gaussian or :uniform")
    s, a, o = perinstance(Clonglong, stream, r.n), perinstance(Cdouble, amp, r.n), perinstance(Cdouble, offset, r.n)
    GC.@preserve s a o check(ccall((:acme_batch_set_source_noise, lib), Cint,
                (Ptr{Cvoid}, Cint, Cint, Clonglong, Ptr{Clonglong}, Ptr{Cdouble}, Ptr{Cdouble}),
                r.h, row - 1, d, hold, ptr_or_null(s), ptr_or_null(a), ptr_or_null(o)))
    push!(r.sources, Int(row))
    return r
end

# the [5][N] integer block of a pulse or burst row: period, delay, rise, on, fall (each a number or N values)
pulse_shape(r::BatchRunner, period, delay, rise, on, fall) =
    vcat(perinstance(Clonglong, period, r.n), perinstance(Clonglong, delay, r.n), perinstance(Clonglong, rise, r.n),
         perinstance(Clonglong, on, r.n), perinstance(Clonglong, fall, r.n))

"""
    set_source_pulse!(runner, row; period, on, delay=0, rise=0, fall=0, amp=nothing, offset=nothing)

Give input row `row` (1-based) a pulse source (`acme_batch_set_source_pulse`): `fma(amp[i], e, offset[i])` with e a per-instance
trapezoid over j = (n - delay[i]) mod period[i] -- j / rise on the rising ramp, 1 for `on` samples, (rise + on + fall - j) / fall
on the falling ramp, 0 otherwise; one correctly rounded division per ramp sample, so the row is pinned bit for bit.  `period`
(1 ... 2^31 - 1), `delay` (0 ... period - 1), `rise`, `on`, `fall` (>= 0, rise + on + fall <= period): a number or N integers.
A step is a pulse of period 2^31 - 1; a PWM or duty sweep, an edge-time sweep, a delay scan are each one batch.  On an
oversampled batch an ideal edge wants the row in `held_rows`.
"""
function set_source_pulse!(r::BatchRunner, row::Integer; period, on, delay=0, rise=0, fall=0, amp=nothing, offset=nothing)
    s, a, o = pulse_shape(r, period, delay, rise, on, fall), perinstance(Cdouble, amp, r.n), perinstance(Cdouble, offset, r.n)
    GC.@preserve s a o check(ccall((:acme_batch_set_source_pulse, lib), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Clonglong}, Ptr{Cdouble}, Ptr{Cdouble}),
                r.h, row - 1, pointer(s), ptr_or_null(a), ptr_or_null(o)))
    push!(r.sources, Int(row))
    return r
end

"""
    set_source_burst!(runner, row; period, on, f_den, f_num=nothing, phase=nothing, delay=0, rise=0, fall=0, amp=nothing, offset=nothing)

Give input row `row` (1-based) a tone burst (`acme_batch_set_source_burst`): g = amp[i] e, then `fma(g, sin(th), offset[i])` with
e the envelope of `set_source_pulse!` and th the `:sine` row's angle from `f_den`, `f_num`, `phase` (the tone's).  Where e = 1
the row is the sine row bit for bit, where e = 0 it is `offset[i]`.  The tone runs with the clock, it does not restart per
burst: a burst starts at a zero crossing when `delay` and `period` are multiples of the tone's period.
"""
function set_source_burst!(r::BatchRunner, row::Integer; period, on, f_den::Integer, f_num=nothing, phase=nothing, delay=0, rise=0, fall=0,
                           amp=nothing, offset=nothing)
    s, a, o = pulse_shape(r, period, delay, rise, on, fall), perinstance(Cdouble, amp, r.n), perinstance(Cdouble, offset, r.n)
    f, p = perinstance(Clonglong, f_num, r.n), perinstance(Clonglong, phase, r.n)
    GC.@preserve s f p a o check(ccall((:acme_batch_set_source_burst, lib), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Clonglong}, Clonglong, Ptr{Clonglong}, Ptr{Clonglong}, Ptr{Cdouble}, Ptr{Cdouble}),
                r.h, row - 1, pointer(s), f_den, ptr_or_null(f), ptr_or_null(p), ptr_or_null(a), ptr_or_null(o)))
    push!(r.sources, Int(row))
    return r
end

"the row (1-based) is the caller's again (`acme_batch_clear_source`); `row = 0`: every row"
function clear_source!(r::BatchRunner, row::Integer=0)
    check(ccall((:acme_batch_clear_source, lib), Cint, (Ptr{Cvoid}, Cint), r.h, row - 1))
    row == 0 ? empty!(r.sources) : delete!(r.sources, Int(row))
    return r
end

"the source clock: base-rate samples the source runs have advanced since the first source was armed"
function source_clock(r::BatchRunner)
    n = Ref{Clonglong}(0)
    check(ccall((:acme_batch_get_source_clock, lib), Cint, (Ptr{Cvoid}, Ref{Clonglong}), r.h, n))
    return Int(n[])
end
source_clock!(r::BatchRunner, n::Integer) = (check(ccall((:acme_batch_set_source_clock, lib), Cint, (Ptr{Cvoid}, Clonglong), r.h, n)); r)

# the rows without a source: nu_var × T × N, or nothing when every row has one
function checkuvar(r::BatchRunner, u_var, T::Integer)
    nuv = ACME.nu(r.model) - length(r.sources)
    isempty(r.sources) && error("no input row has a source (set_source!)")
    if u_var === nothing
        nuv == 0 || throw(DimensionMismatch("u_var must be $nuv × T × $(r.n)"))
        return Ptr{Cdouble}(C_NULL), Int(T)
    end
    size(u_var, 1) == nuv && size(u_var, 3) == r.n || throw(DimensionMismatch("u_var must be $nuv × T × $(r.n)"))
    return pointer(u_var), size(u_var, 2)
end

"""
    run_sources!(runner, y, T; u_var=nothing)
    run_sources!(runner, T; u_var=nothing)        # measured run: no outputs

`run!` with the sourced rows generated on the device (`acme_batch_run_sources`): `u_var` (nu_var × T × N) holds only the
rows without a source, in row order; `nothing` when every row has one.  Without `y` (a measurement armed) nothing of the
outputs is stored: a level sweep owns no N × T array anywhere.
"""
function run_sources!(r::BatchRunner, y::Union{Array{Float64,3},Nothing}, T::Integer; u_var::Union{Array{Float64,3},Nothing}=nothing)
    up, T = checkuvar(r, u_var, T)
    y === nothing || size(y) == (ACME.ny(r.model), T, r.n) || throw(DimensionMismatch("output must be $(ACME.ny(r.model)) × $T × $(r.n)"))
    y === nothing && r.meas === nothing && error("run_sources! without y needs an armed measurement (set_measurement!)")
    GC.@preserve r u_var y check(ccall((:acme_batch_run_sources, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Clonglong, Cint, Ptr{Cvoid}),
                r.h, up, y === nothing ? Ptr{Cdouble}(C_NULL) : pointer(y), T, ACME_MEM_HOST, C_NULL))
    checkreports!(r)
    return y === nothing ? r : y
end
run_sources!(r::BatchRunner, T::Integer; kwargs...) = run_sources!(r, nothing, T; kwargs...)

"""
    render_sources(runner, T; u_var=nothing) -> nu × T × N

The input a source run of `T` samples would feed from the current clock (`acme_batch_render_sources`): sourced rows
generated, the others from `u_var` (zeros if `nothing`).  Advances neither the clock nor the model.
"""
function render_sources(r::BatchRunner, T::Integer; u_var::Union{Array{Float64,3},Nothing}=nothing)
    up = u_var === nothing ? Ptr{Cdouble}(C_NULL) : checkuvar(r, u_var, T)[1]
    u = Array{Float64,3}(undef, ACME.nu(r.model), T, r.n)
    GC.@preserve u_var check(ccall((:acme_batch_render_sources, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Clonglong, Cint, Ptr{Cvoid}),
                r.h, up, u, T, ACME_MEM_HOST, C_NULL))
    return u
end

# ---- MultiBatchRunner: N instances over the GPUs of one node, one Julia process -----------------------
"contiguous instance range (1-based) of part `k` of `parts`; sizes differ by at most one (acme_jl_amd/dist.py)"
function shard_range(n::Integer, k::Integer, parts::Integer)
    base, rem = divrem(n, parts)
    lo = (k - 1) * base + min(k - 1, rem)
    return lo+1:lo+base+(k <= rem ? 1 : 0)
end

"""
    MultiBatchRunner(model, n; devices=0:device_count()-1, solver=..., per_instance_matrices=false)

`n` instances of `model` spread over several GPUs by ONE process: contiguous instance ranges, one
`BatchRunner` per device.  `run!` starts every device's run asynchronously (`acme_batch_run_async`: the
library drives each from a worker thread of its own) and then joins them (`acme_batch_wait`); every
batch reads and writes its own `[:, :, range]` slice of `u` / `y` in place.  The sweep shards perfectly
(instances never interact), so there is no collective and no MPI/RCCL dependency on the Julia side.
"""
struct MultiBatchRunner
    model::DiscreteModel
    n::Int
    runners::Vector{BatchRunner}
    ranges::Vector{UnitRange{Int}}
end

function MultiBatchRunner(model::DiscreteModel, n::Integer; devices=0:device_count()-1, kwargs...)
    isempty(devices) && error("libacme_hip: no HIP device available")
    ranges = [shard_range(n, k, length(devices)) for k in 1:length(devices)]
    keep = [k for k in 1:length(devices) if !isempty(ranges[k])]
    runners = [BatchRunner(model, length(ranges[k]); device=devices[k], kwargs...) for k in keep]
    return MultiBatchRunner(model, n, runners, ranges[keep])
end

function run!(mr::MultiBatchRunner, y::Array{Float64,3}, u::Array{Float64,3})
    checkiosizes(mr.model, mr.n, y, u)
    T = size(u, 2)
    su, sy = size(u, 1) * T, size(y, 1) * T                   # doubles per instance
    GC.@preserve u y begin
        started = 0
        rcs, msg = Cint[], ""                                 # (assigned in the finally clause below)
        try
            for (r, rg) in zip(mr.runners, mr.ranges)
                check(ccall((:acme_batch_run_async, lib), Cint,
                            (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Clonglong, Cint, Ptr{Cvoid}),
                            r.h, pointer(u) + 8 * su * (first(rg) - 1), pointer(y) + 8 * sy * (first(rg) - 1),
                            T, ACME_MEM_HOST, C_NULL))
                started += 1
            end
        finally                                               # never leave a run in flight behind
            rcs = [ccall((:acme_batch_wait, lib), Cint, (Ptr{Cvoid},), r.h) for r in mr.runners[1:started]]
            msg = lasterror()
        end
        all(rc -> rc >= 0, rcs) || error("libacme_hip: " * msg)
    end
    for (r, rg) in zip(mr.runners, mr.ranges)
        checkreports!(r, first(rg) - 1)
    end
    return nothing
end

function run!(mr::MultiBatchRunner, u::Array{Float64,3})
    y = Array{Float64,3}(undef, ACME.ny(mr.model), size(u, 2), mr.n)
    run!(mr, y, u)
    return y
end

# sources on every device's batch, each with its instances' parameters
slicepar(v, rg) = v isa AbstractVector ? v[rg] : v
function set_source!(mr::MultiBatchRunner, row::Integer, kind::Symbol; f_den::Integer=0, f_num=nothing, phase=nothing,
                     table=nothing, amp=nothing, offset=nothing)
    for (r, rg) in zip(mr.runners, mr.ranges)
        set_source!(r, row, kind; f_den=f_den, f_num=slicepar(f_num, rg), phase=slicepar(phase, rg), table=table,
                    amp=slicepar(amp, rg), offset=slicepar(offset, rg))
    end
    return mr
end
clear_source!(mr::MultiBatchRunner, row::Integer=0) = (foreach(r -> clear_source!(r, row), mr.runners); mr)

"`run_sources!` on every device at once (`acme_batch_run_sources_async`, then joined); every row has a source"
function run_sources!(mr::MultiBatchRunner, y::Union{Array{Float64,3},Nothing}, T::Integer)
    sy = ACME.ny(mr.model) * T
    y === nothing || size(y) == (ACME.ny(mr.model), T, mr.n) || throw(DimensionMismatch("output must be $(ACME.ny(mr.model)) × $T × $(mr.n)"))
    GC.@preserve y begin
        started = 0
        rcs, msg = Cint[], ""
        try
            for (r, rg) in zip(mr.runners, mr.ranges)
                check(ccall((:acme_batch_run_sources_async, lib), Cint,
                            (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Clonglong, Cint, Ptr{Cvoid}),
                            r.h, Ptr{Cdouble}(C_NULL), y === nothing ? Ptr{Cdouble}(C_NULL) : pointer(y) + 8 * sy * (first(rg) - 1),
                            T, ACME_MEM_HOST, C_NULL))
                started += 1
            end
        finally
            rcs = [ccall((:acme_batch_wait, lib), Cint, (Ptr{Cvoid},), r.h) for r in mr.runners[1:started]]
            msg = lasterror()
        end
        all(rc -> rc >= 0, rcs) || error("libacme_hip: " * msg)
    end
    for (r, rg) in zip(mr.runners, mr.ranges)
        checkreports!(r, first(rg) - 1)
    end
    return y === nothing ? mr : y
end

reports(mr::MultiBatchRunner) = reduce(vcat, [reports(r) for r in mr.runners])
set_resabstol!(mr::MultiBatchRunner, tol) = (foreach(r -> set_resabstol!(r, tol), mr.runners); tol)

set_resabstol!(r::BatchRunner, tol) =
    (check(ccall((:acme_batch_set_resabstol, lib), Cint, (Ptr{Cvoid}, Cdouble), r.h, tol)); tol)

"(x, last_p, last_z) of all instances: nx × N, Σnp × N, Σnn × N"
function get_state(r::BatchRunner)
    m = r.model
    x = zeros(ACME.nx(m), r.n)
    p = zeros(sum(ACME.np(m, k) for k in 1:length(m.solvers); init=0), r.n)
    z = zeros(ACME.nn(m), r.n)
    check(ccall((:acme_batch_get_state, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), r.h, x, p, z))
    return x, p, z
end

# ---- GPUBatchSolver: the solver plugin contract (src/solvers.jl:139-205) ---------------------------
"""
    GPUBatchSolver(nleq::ParametricNonLinEq, initial_p, initial_z)

A `NonlinearSolver` whose `solve` runs on the GPU (HomotopySolver{SimpleSolver} semantics: Newton
from the first-order extrapolated start, bisection homotopy on failure).  Built, like the
reference's solvers, from the equation object alone (src/ACME.jl:253-259): the data of the closures
in `nleq` -- `fq` and the `CircuitNLFunc` inside `nleq.func` (src/ACME.jl:176-194), `pexp`/`q0`
inside `nleq.set_p` (:236-244), or the identity parametrisation p == q of the three-argument
`ParametricNonLinEq` constructor (src/solvers.jl:23-28) -- is packed as a one-sub-problem model
without states.  Usable wherever ACME takes a solver type:

    model = DiscreteModel(circ, 1//44100, ACMEHip.GPUBatchSolver)
"""
mutable struct GPUBatchSolver <: NonlinearSolver
    mh::ModelHandle
    h::Ptr{Cvoid}
    nn::Int
    np::Int
    z::Vector{Float64}
    converged::Bool
    iters::Int
    function GPUBatchSolver(nleq::ParametricNonLinEq, initial_p::Vector{Float64}, initial_z::Vector{Float64})
        nn_, np_ = ACME.nn(nleq), ACME.np(nleq)
        f = nleq.func                              # (res, J, scratch, z) -> nleq´(res, J, scratch[1], scratch[2], fq, z)
        fq = Matrix{Float64}(captured(f, :fq))
        cnl = captured(captured(f, :nleq), :circ_nl_func)
        nq_ = size(fq, 1)
        if hascaptured(nleq.set_p, :pexp)          # src/ACME.jl:236-244
            pexp = Matrix{Float64}(captured(nleq.set_p, :pexp))
            q0 = Vector{Float64}(captured(nleq.set_p, :q0))
        else                                       # default_set_p: p == q
            np_ == nq_ || error("ACMEHip: identity parametrisation needs np == nq")
            pexp = Matrix{Float64}(I, nq_, nq_)
            q0 = zeros(nq_)
        end
        h = Ref{Ptr{Cvoid}}()
        e = Float64[]
        check(ccall((:acme_model_create, lib), Cint,
            (Cint, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
             Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}),
            0, 0, 0, nn_, e, e, e, e, e, e, e, e, h))
        mh = ModelHandle(h[])
        add_subproblem!(mh.h, nn_, nq_, np_, pexp, zeros(np_, 0), zeros(np_, 0), zeros(np_, nn_), fq, q0,
                        initial_z, cnl)
        opts = Ref(AcmeOptions(ACME_SOLVER_HOMOTOPY, 1e-10, 500, -1, 0))
        b = Ref{Ptr{Cvoid}}()
        check(ccall((:acme_batch_create, lib), Cint, (Ptr{Cvoid}, Clonglong, Ref{AcmeOptions}, Ref{Ptr{Cvoid}}),
                    mh.h, 1, opts, b))
        s = new(mh, b[], nn_, np_, copy(initial_z), true, 0)
        finalizer(s -> ccall((:acme_batch_destroy, lib), Cvoid, (Ptr{Cvoid},), s.h), s)
        set_extrapolation_origin(s, initial_p, initial_z)
        return s
    end
end

"z = solve(solver, p): returns the solver's internal buffer, like the reference (the caller copies, src/ACME.jl:695)"
function solve(s::GPUBatchSolver, p::AbstractVector{Float64})
    conv, iters = Ref{Cint}(0), Ref{Cint}(0)
    check(ccall((:acme_batch_solve, lib), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cint}, Ref{Cint}, Cint, Ptr{Cvoid}),
                s.h, 0, Vector{Float64}(p), s.z, conv, iters, ACME_MEM_HOST, C_NULL))
    s.converged = conv[] != 0
    s.iters = iters[]
    return s.z
end

hasconverged(s::GPUBatchSolver) = s.converged
needediterations(s::GPUBatchSolver) = s.iters
set_resabstol!(s::GPUBatchSolver, tol) =
    (check(ccall((:acme_batch_set_resabstol, lib), Cint, (Ptr{Cvoid}, Cdouble), s.h, tol)); tol)

function get_extrapolation_origin(s::GPUBatchSolver)
    p, z = zeros(s.np), zeros(s.nn)
    check(ccall((:acme_batch_get_state, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                s.h, C_NULL, p, z))
    return p, z
end

function set_extrapolation_origin(s::GPUBatchSolver, p, z)
    check(ccall((:acme_batch_set_state, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                s.h, C_NULL, Vector{Float64}(p), Vector{Float64}(z)))
    return nothing
end

"-(J \\ Jp) at the extrapolation origin (src/solvers.jl:198-201), nn × np"
function get_extrapolation_jacobian(s::GPUBatchSolver)
    jac = zeros(s.nn, s.np)
    check(ccall((:acme_batch_get_extrapolation_jacobian, lib), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cvoid}), s.h, 0, jac, ACME_MEM_HOST, C_NULL))
    return jac
end

end # module
