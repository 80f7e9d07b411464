# OSQPAMD.jl -- thin Julia layer over the extension entry points of libosqp_amd.so.
#
# The 30 `osqp_*` symbols that osqp/OSQP.jl binds need no new Julia code: point `OSQP.osqp` at
# libosqp_amd.so (INTEGRATION.md, section 2) and the reference's `setup!/solve!/update!/warm_start!`
# and its MathOptInterface wrapper run on the MI355X unchanged.  This module only adds what the
# reference has no call for: problems generated directly in HBM, the batched small-QP path, device
# selection, statistics.  Style follows [REF src/interface.jl]: one `ccall` per entry point, a
# non-zero exit flag becomes `error(...)`.
#
# NOTE: Julia is not installed in the build image, so this file is not executed by the test suite;
# the same entry points are exercised through the Python mirror (osqp.jl_amd/interface.py, batch.py).
module OSQPAMD

using OSQP
using SparseArrays

const lib = get(ENV, "OSQP_AMD_LIB", joinpath(@__DIR__, "..", "csrc", "libosqp_amd.so"))
const Cc_int = OSQP.Cc_int

@enum ProblemKind RANDOM_QP = 0 LASSO = 1 MPC = 2

"""
    set_device(local_rank)

Select the HIP device for workspaces created afterwards (one process per GPU).
"""
function set_device(device::Integer)
    flag = ccall((:osqp_amd_set_device, lib), Cc_int, (Cc_int,), device)
    flag == 0 || error("Error selecting device $(device): $(last_error())")
    return nothing
end

last_error() = unsafe_string(ccall((:osqp_amd_last_error, lib), Cstring, ()))

"""
    setup_generated!(model, kind, n; per_row = 0, seed = 1, settings...)

Build one of the synthetic problem families of SURVEY.md 8d directly in HBM and run setup on it.
Mirrors `OSQP.setup!` [REF src/interface.jl:35-162] after the point where the data are handed to C.
"""
function setup_generated!(model::OSQP.Model, kind::ProblemKind, n::Integer; per_row::Integer = 0, seed::Integer = 1, settings...)
    settings_dict = Dict{Symbol,Any}(settings)
    stgs = OSQP.Settings(settings_dict)
    workspace = Ref{Ptr{OSQP.Workspace}}()
    flag = ccall(
        (:osqp_amd_setup_generated, lib),
        Cc_int,
        (Ptr{Ptr{OSQP.Workspace}}, Cc_int, Cc_int, Cc_int, Culonglong, Ptr{OSQP.Settings}),
        workspace, Int(kind), n, per_row, seed, Ref(stgs),
    )
    flag == 0 || error("Error in OSQP setup: $(last_error())")
    model.workspace = workspace[]
    (nn, m) = OSQP.dimensions(model)
    resize!(model.lcache, m)
    resize!(model.ucache, m)
    model.isempty = false
    return model
end

"""
    stats(model) -> Vector{Float64}

Back-end in use, non-zero counts, nnz(L), CG / ADMM iteration totals, device bytes, algorithmic bytes
of the dominant kernels (see include/osqp_amd.h, `osqp_amd_get_stats`).
"""
function stats(model::OSQP.Model)
    out = zeros(Float64, 26)  # OSQP_AMD_STATS_COUNT (include/osqp_amd.h)
    k = ccall((:osqp_amd_get_stats, lib), Cc_int, (Ptr{OSQP.Workspace}, Ptr{Cdouble}, Cc_int), model.workspace, out, length(out))
    return out[1:k]
end

"""
    iterate!(model, iters)

Run exactly `iters` ADMM iterations from the current iterate (benchmark hook).
"""
function iterate!(model::OSQP.Model, iters::Integer)
    flag = ccall((:osqp_amd_iterate, lib), Cc_int, (Ptr{OSQP.Workspace}, Cc_int), model.workspace, iters)
    flag == 0 || error("Error iterating: $(last_error())")
    return nothing
end

"""
    adjoint(model; dx = nothing, dy = nothing, want = (:q, :l, :u, :Px, :Ax)) -> NamedTuple

Gradients of a scalar loss through the solution of the last `OSQP.solve!` (osqp_amd_adjoint in include/osqp_amd.h): from
`dx` = dloss/dx and `dy` = dloss/dy (either may be `nothing` = 0) the gradients named in `want` -- `q`, `l`, `u`, `Px` (upper
triangle of P), `Ax`, both in the nnz order `OSQP.update!` takes -- plus `act` (-1 lower, 0 inactive, 1 upper).  Vectors give
vectors; matrices with one column per cotangent (`n x ncot`, `m x ncot`: column-major here is cotangent-major on the C side)
give matrices with one column per cotangent.  The first call after a solve factorises and keeps the factor
(`adjoint_release!`); every update, warm start and solve drops it.
"""
function adjoint(model::OSQP.Model; dx::Union{Nothing,VecOrMat{Float64}} = nothing, dy::Union{Nothing,VecOrMat{Float64}} = nothing,
                 want = (:q, :l, :u, :Px, :Ax))
    (n, m) = OSQP.dimensions(model)
    all(k -> k in (:q, :l, :u, :Px, :Ax), want) || error("want: unknown gradient")
    isempty(want) || dx !== nothing || dy !== nothing || error("a gradient is wanted but dx and dy are both nothing")
    dx === nothing || size(dx, 1) == n || error("dx must have n = $n rows")
    dy === nothing || size(dy, 1) == m || error("dy must have m = $m rows")
    ncot = dx !== nothing ? size(dx, 2) : (dy !== nothing ? size(dy, 2) : 1)
    dx === nothing || dy === nothing || (size(dy, 2) == ncot && ndims(dx) == ndims(dy)) || error("dx and dy differ in the number of cotangents")
    many = (dx !== nothing && dx isa Matrix) || (dy !== nothing && dy isa Matrix)
    st = stats(model)
    rows = (q = n, l = m, u = m, Px = Int(st[4]), Ax = Int(st[2]))
    out = Dict(k => fill(NaN, rows[k], ncot) for k in want)
    act = zeros(Float64, m)
    ptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(a)
    GC.@preserve dx dy out act begin
        flag = ccall((:osqp_amd_adjoint, lib), Cc_int,
                     (Ptr{OSQP.Workspace}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                      Ptr{Cdouble}, Ptr{Cdouble}),
                     model.workspace, ncot, ptr(dx), ptr(dy), ptr(get(out, :q, nothing)), ptr(get(out, :l, nothing)),
                     ptr(get(out, :u, nothing)), ptr(get(out, :Px, nothing)), ptr(get(out, :Ax, nothing)), act)
    end
    flag == 0 || error("Error in adjoint: $(last_error())")
    grads = [k => (many ? out[k] : vec(out[k])) for k in want]
    return (; grads..., act = Int.(act))
end

"""
    jvp(model; q = nothing, l = nothing, u = nothing, Px = nothing, Ax = nothing) -> (x, y, act)

Forward sensitivities of the solution of the last `OSQP.solve!` along a direction of the data (osqp_amd_jvp in
include/osqp_amd.h): tangents `q` [n], `l`, `u` [m], `Px` (upper triangle of P), `Ax`, both in the nnz order `OSQP.update!` takes
(`nothing` = 0; not all).  Vectors give vectors; matrices with one column per direction (column-major here is direction-major
on the C side) give matrices with one column per direction.  On a row with `l == u` only `l` is read.  The factor is
`adjoint`'s: whichever is called first after a solve builds it, the other reuses it.  Not executed by the test suite; the
Python mirror (`interface.jvp`) is.
"""
function jvp(model::OSQP.Model; q::Union{Nothing,VecOrMat{Float64}} = nothing, l::Union{Nothing,VecOrMat{Float64}} = nothing,
             u::Union{Nothing,VecOrMat{Float64}} = nothing, Px::Union{Nothing,VecOrMat{Float64}} = nothing,
             Ax::Union{Nothing,VecOrMat{Float64}} = nothing)
    (n, m) = OSQP.dimensions(model)
    st = stats(model)
    rows = (q = n, l = m, u = m, Px = Int(st[4]), Ax = Int(st[2]))
    given = [(k, v) for (k, v) in pairs((q = q, l = l, u = u, Px = Px, Ax = Ax)) if v !== nothing]
    isempty(given) && error("jvp: q, l, u, Px and Ax are all nothing: at least one tangent is needed")
    for (k, v) in given
        size(v, 1) == rows[k] || error("$k must have $(rows[k]) rows")
    end
    length(unique(ndims(v) for (_, v) in given)) == 1 || error("the tangents must all be vectors or all be matrices")
    ndir = size(given[1][2], 2)
    all(size(v, 2) == ndir for (_, v) in given) || error("the tangents differ in the number of directions")
    ndir >= 1 || error("jvp: ndir must be at least 1")
    many = given[1][2] isa Matrix
    tx, ty, act = fill(NaN, n, ndir), fill(NaN, m, ndir), zeros(Float64, m)
    ptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(a)
    GC.@preserve q l u Px Ax tx ty act begin
        flag = ccall((:osqp_amd_jvp, lib), Cc_int,
                     (Ptr{OSQP.Workspace}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                      Ptr{Cdouble}, Ptr{Cdouble}),
                     model.workspace, ndir, ptr(q), ptr(l), ptr(u), ptr(Px), ptr(Ax), tx, ty, act)
    end
    flag == 0 || error("Error in jvp: $(last_error())")
    return (x = many ? tx : vec(tx), y = many ? ty : vec(ty), act = Int.(act))
end

"Drop the factor `adjoint` keeps (osqp_amd_adjoint_release); it is as large as a polish's."
function adjoint_release!(model::OSQP.Model)
    flag = ccall((:osqp_amd_adjoint_release, lib), Cc_int, (Ptr{OSQP.Workspace},), model.workspace)
    flag == 0 || error("Error in adjoint_release!: $(last_error())")
    return nothing
end

"(builds, solves, n_low, n_upp, kept, bytes) of the adjoint's kept factor (osqp_amd_adjoint_stats)."
function adjoint_stats(model::OSQP.Model)
    out = zeros(Float64, 6)  # OSQP_AMD_ADJOINT_STATS_COUNT (include/osqp_amd.h)
    k = ccall((:osqp_amd_adjoint_stats, lib), Cc_int, (Ptr{OSQP.Workspace}, Ptr{Cdouble}, Cc_int), model.workspace, out, length(out))
    k == length(out) || error("osqp_amd_adjoint_stats: bad argument")
    return (builds = Int(out[1]), solves = Int(out[2]), n_low = Int(out[3]), n_upp = Int(out[4]), kept = out[5] == 1.0, bytes = Int(out[6]))
end

"""
    derivative_method!(model, method = :direct; max_outer = 0, rel_drop = 0.0)

Which KKT solve `adjoint` and `jvp` use (osqp_amd_derivative_method, DESIGN.md section 17): `:direct` the kept factor,
`:auto` the factor where it can be built and the iterative solve on the operator of the indirect back-end on a compact
workspace or where the factor does not fit, `:iterative` always the iterative solve.  0 keeps the defaults (40 outer steps,
a drop of 1e-10).  Drops the derivative state the current solution keeps.
"""
function derivative_method!(model::OSQP.Model, method::Symbol = :direct; max_outer::Integer = 0, rel_drop::Real = 0.0)
    code = findfirst(==(method), (:direct, :auto, :iterative))
    code === nothing && error("derivative_method!: expected :direct, :auto or :iterative, got $(method)")
    flag = ccall((:osqp_amd_derivative_method, lib), Cc_int, (Ptr{OSQP.Workspace}, Cc_int, Cc_int, Cdouble), model.workspace, code - 1, max_outer, rel_drop)
    flag == 0 || error("Error in derivative_method!: $(last_error())")
    return nothing
end

"(builds, outer_steps, cg_iters, last_outer_steps, last_drop, kept, bytes) of the iterative derivatives (osqp_amd_derivative_iter_stats)."
function derivative_iter_stats(model::OSQP.Model)
    out = zeros(Float64, 7)  # OSQP_AMD_DERIVATIVE_ITER_STATS_COUNT (include/osqp_amd.h)
    k = ccall((:osqp_amd_derivative_iter_stats, lib), Cc_int, (Ptr{OSQP.Workspace}, Ptr{Cdouble}, Cc_int), model.workspace, out, length(out))
    k == length(out) || error("osqp_amd_derivative_iter_stats: bad argument")
    return (builds = Int(out[1]), outer_steps = Int(out[2]), cg_iters = Int(out[3]), last_outer_steps = Int(out[4]), last_drop = out[5],
            kept = out[6] == 1.0, bytes = Int(out[7]))
end

"""
    adjoint_retain!(model, on = true)

Let the factor `adjoint` and `jvp` keep outlive its solution (osqp_amd_adjoint_retain, DESIGN.md section 18): updates, warm
starts and solves mark it stale instead of dropping it, and the first derivative call on the next solution checks on the
device whether a row changed its side.  None did: the factor is reused (after a numeric refactorisation where P or A
changed); otherwise it is rebuilt as by default.  `on = false` drops a stale factor at once.
"""
function adjoint_retain!(model::OSQP.Model, on::Bool = true)
    flag = ccall((:osqp_amd_adjoint_retain, lib), Cc_int, (Ptr{OSQP.Workspace}, Cc_int), model.workspace, on ? 1 : 0)
    flag == 0 || error("Error in adjoint_retain!: $(last_error())")
    return nothing
end

"(mode, checks, reused, refactorised, rebuilt_active_set, rebuilt_failed, last_rows_changed, stale) of the retained factor (osqp_amd_adjoint_retain_stats)."
function adjoint_retain_stats(model::OSQP.Model)
    out = zeros(Float64, 8)  # OSQP_AMD_ADJOINT_RETAIN_STATS_COUNT (include/osqp_amd.h)
    k = ccall((:osqp_amd_adjoint_retain_stats, lib), Cc_int, (Ptr{OSQP.Workspace}, Ptr{Cdouble}, Cc_int), model.workspace, out, length(out))
    k == length(out) || error("osqp_amd_adjoint_retain_stats: bad argument")
    return (mode = Int(out[1]), checks = Int(out[2]), reused = Int(out[3]), refactorised = Int(out[4]), rebuilt_active_set = Int(out[5]),
            rebuilt_failed = Int(out[6]), last_rows_changed = Int(out[7]), stale = out[8] == 1.0)
end

"""
    duality_gap_check!(model, on = true)

Add the duality gap |x'Px + q'x + SC(y)| < eps_abs + eps_rel max(|x'Px|, |q'x|, |SC|) to the termination test of every later
`OSQP.solve!` (osqp_amd_duality_gap_check, DESIGN.md section 19; OSQP 1.0's check_dualgap).  Off by default.  The call does
not move the iterate, rho, the factor or a kept derivative factor.
"""
function duality_gap_check!(model::OSQP.Model, on::Bool = true)
    flag = ccall((:osqp_amd_duality_gap_check, lib), Cc_int, (Ptr{OSQP.Workspace}, Cc_int), model.workspace, on ? 1 : 0)
    flag == 0 || error("Error in duality_gap_check!: $(last_error())")
    return nothing
end

"(prim_obj, dual_obj, gap, eps_gap, rule, gap_refusals) of the pair (x, y) the model holds (osqp_amd_duality); changes nothing."
function duality(model::OSQP.Model)
    out = zeros(Float64, 6)  # OSQP_AMD_DUALITY_COUNT (include/osqp_amd.h)
    flag = ccall((:osqp_amd_duality, lib), Cc_int, (Ptr{OSQP.Workspace}, Ptr{Cdouble}, Cc_int), model.workspace, out, length(out))
    flag == 0 || error("Error in duality: $(last_error())")
    return (prim_obj = out[1], dual_obj = out[2], gap = out[3], eps_gap = out[4], rule = out[5] == 1.0, gap_refusals = Int(out[6]))
end

# ---- device-pointer forms of a single model's life cycle (include/osqp_amd.h, DESIGN.md section 16) ----
# Every array is a DEVICE address on the model's device, as a `Ptr{Cdouble}` (`C_NULL`: not given / not wanted) -- for an
# AMDGPU.jl array `Ptr{Cdouble}(UInt(pointer(a)))`; the package itself does not depend on a GPU array type.  The library runs
# on its own stream and blocks: the caller has finished producing the inputs before the call.  Each call leaves the model in
# the state its host twin leaves it in, bit for bit.  Not executed by the test suite; the Python mirror (`interface.update`,
# `warm_start`, `solution`, `adjoint`, `jvp` with device arrays) is.
const DevicePtr = Ptr{Cdouble}
const DEV_NULL = Ptr{Cdouble}(C_NULL)

"`OSQP.update!(model; q, l, u)` from device arrays (osqp_amd_update_vectors_dev); a crossed pair of bounds changes nothing."
function update_vectors_dev!(model::OSQP.Model; q::DevicePtr = DEV_NULL, l::DevicePtr = DEV_NULL, u::DevicePtr = DEV_NULL)
    flag = ccall((:osqp_amd_update_vectors_dev, lib), Cc_int, (Ptr{OSQP.Workspace}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                 model.workspace, q, l, u)
    flag == 0 || error("Error updating q, l, u from device arrays: $(last_error())")
    return nothing
end

"`OSQP.update!(model; Px, Ax)` with full value arrays on the device, in the caller's nnz order (osqp_amd_update_values_dev)."
function update_values_dev!(model::OSQP.Model; Px::DevicePtr = DEV_NULL, Ax::DevicePtr = DEV_NULL)
    flag = ccall((:osqp_amd_update_values_dev, lib), Cc_int, (Ptr{OSQP.Workspace}, Ptr{Cdouble}, Ptr{Cdouble}), model.workspace, Px, Ax)
    flag == 0 || error("Error updating P and A from device arrays: $(last_error())")
    return nothing
end

"`OSQP.warm_start!(model; x, y)` from device arrays (osqp_amd_warm_start_dev); one of them alone zeroes the other block."
function warm_start_dev!(model::OSQP.Model; x::DevicePtr = DEV_NULL, y::DevicePtr = DEV_NULL)
    flag = ccall((:osqp_amd_warm_start_dev, lib), Cc_int, (Ptr{OSQP.Workspace}, Ptr{Cdouble}, Ptr{Cdouble}), model.workspace, x, y)
    flag == 0 || error("Error in warm starting from device arrays: $(last_error())")
    return nothing
end

"The solution of the last `OSQP.solve!` into the device arrays `x` [n] and `y` [m] (osqp_amd_solution_dev)."
function solution_dev!(model::OSQP.Model; x::DevicePtr = DEV_NULL, y::DevicePtr = DEV_NULL)
    flag = ccall((:osqp_amd_solution_dev, lib), Cc_int, (Ptr{OSQP.Workspace}, Ptr{Cdouble}, Ptr{Cdouble}), model.workspace, x, y)
    flag == 0 || error("Error in solution_dev!: $(last_error())")
    return nothing
end

"""
    adjoint_dev!(model, ncot; dx, dy, dq, dl, du, dPx, dAx, act)

`adjoint` from device arrays into device arrays (osqp_amd_adjoint_dev): cotangents `[ncot x n]` / `[ncot x m]` cotangent-major,
the outputs that are given are written, `act` is `[m]` doubles.  The kept factor is `adjoint`'s.
"""
function adjoint_dev!(model::OSQP.Model, ncot::Integer = 1; dx::DevicePtr = DEV_NULL, dy::DevicePtr = DEV_NULL, dq::DevicePtr = DEV_NULL,
                      dl::DevicePtr = DEV_NULL, du::DevicePtr = DEV_NULL, dPx::DevicePtr = DEV_NULL, dAx::DevicePtr = DEV_NULL,
                      act::DevicePtr = DEV_NULL)
    flag = ccall((:osqp_amd_adjoint_dev, lib), Cc_int,
                 (Ptr{OSQP.Workspace}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                  Ptr{Cdouble}, Ptr{Cdouble}),
                 model.workspace, ncot, dx, dy, dq, dl, du, dPx, dAx, act)
    flag == 0 || error("Error in adjoint_dev!: $(last_error())")
    return nothing
end

"""
    jvp_dev!(model, ndir; q, l, u, Px, Ax, tx, ty, act)

`jvp` from device arrays into device arrays (osqp_amd_jvp_dev): tangents `[ndir x cols]` direction-major, `tx` / `ty` written
where given.
"""
function jvp_dev!(model::OSQP.Model, ndir::Integer = 1; q::DevicePtr = DEV_NULL, l::DevicePtr = DEV_NULL, u::DevicePtr = DEV_NULL,
                  Px::DevicePtr = DEV_NULL, Ax::DevicePtr = DEV_NULL, tx::DevicePtr = DEV_NULL, ty::DevicePtr = DEV_NULL,
                  act::DevicePtr = DEV_NULL)
    flag = ccall((:osqp_amd_jvp_dev, lib), Cc_int,
                 (Ptr{OSQP.Workspace}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                  Ptr{Cdouble}, Ptr{Cdouble}),
                 model.workspace, ndir, q, l, u, Px, Ax, tx, ty, act)
    flag == 0 || error("Error in jvp_dev!: $(last_error())")
    return nothing
end

"The device-form calls this model has served (osqp_amd_device_form_calls)."
function device_form_calls(model::OSQP.Model)
    out = zeros(Float64, 6)  # OSQP_AMD_DEVICE_FORM_COUNT (include/osqp_amd.h)
    k = ccall((:osqp_amd_device_form_calls, lib), Cc_int, (Ptr{OSQP.Workspace}, Ptr{Cdouble}, Cc_int), model.workspace, out, length(out))
    k == length(out) || error("osqp_amd_device_form_calls: bad argument")
    return (update_vectors = Int(out[1]), update_values = Int(out[2]), warm_start = Int(out[3]), solution = Int(out[4]),
            adjoint = Int(out[5]), jvp = Int(out[6]))
end

"""
    batch_solve(P, A, Px, Ax, q, l, u; device = 0, settings...) -> (x, y, infos)

`count` independent QPs that share the sparsity pattern of `P` (upper triangle) and `A`; the value arrays
are `count x nnz` / `count x n|m` matrices stored row-major on the C side, hence the transposes.
One workgroup per QP with the reduced KKT system factorised in LDS (csrc/batch.hip).
"""
function batch_solve(P::SparseMatrixCSC, A::SparseMatrixCSC, Px::Matrix{Float64}, Ax::Matrix{Float64},
                     q::Matrix{Float64}, l::Matrix{Float64}, u::Matrix{Float64}; device::Integer = 0, settings...)
    Pu = istriu(P) ? P : triu(P)
    n = size(A, 2); m = size(A, 1); count = size(q, 1)
    stgs = OSQP.Settings(Dict{Symbol,Any}(settings))
    Pp = convert(Vector{Cc_int}, Pu.colptr .- 1); Pi = convert(Vector{Cc_int}, Pu.rowval .- 1)
    Ap = convert(Vector{Cc_int}, A.colptr .- 1);  Ai = convert(Vector{Cc_int}, A.rowval .- 1)
    # row-major [count x .] on the C side = column-major [. x count] here
    Pxt = permutedims(Px); Axt = permutedims(Ax); qt = permutedims(q)
    lt = permutedims(max.(l, -OSQP.OSQP_INFTY)); ut = permutedims(min.(u, OSQP.OSQP_INFTY))
    x = Matrix{Float64}(undef, n, count); y = Matrix{Float64}(undef, m, count)
    infos = Vector{OSQP.CInfo}(undef, count)
    flag = ccall(
        (:osqp_amd_batch_solve, lib),
        Cc_int,
        (Cc_int, Cc_int, Cc_int, Ptr{Cc_int}, Ptr{Cc_int}, Ptr{Cdouble}, Ptr{Cc_int}, Ptr{Cc_int}, Ptr{Cdouble},
         Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{OSQP.Settings}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{OSQP.CInfo}, Cc_int),
        count, n, m, Pp, Pi, Pxt, Ap, Ai, Axt, qt, lt, ut, Ref(stgs), x, y, infos, device,
    )
    flag == 0 || error("Error in batched solve: $(last_error())")
    results = map(infos) do ci
        info = OSQP.Info()
        OSQP.copyto!(info, ci)
        info
    end
    return permutedims(x), permutedims(y), results
end

# ---------------------------------------------------------------------------------------------
# Row-sharded solve of one large QP over several GPUs (include/osqp_amd.h, "Row-sharded workspaces")
# ---------------------------------------------------------------------------------------------

"""
Opaque handle of the library's communicator (one in-place all-gather of doubles).  Must outlive the models
set up with it.
"""
mutable struct Comm
    handle::Ptr{Cvoid}
    rank::Int
    world::Int
    keep::Any   # the @cfunction / closure of the host transport, kept alive
end

function close!(comm::Comm)
    comm.handle == C_NULL || ccall((:osqp_amd_comm_destroy, lib), Cc_int, (Ptr{Cvoid},), comm.handle)
    comm.handle = C_NULL
    return nothing
end

"""
    unique_id() -> Vector{UInt8}

The 128 bytes of an ncclUniqueId; call on one rank and distribute (e.g. `MPI.Bcast!`).
"""
function unique_id(; librccl::Union{Nothing,String} = nothing)
    id = Vector{UInt8}(undef, 128)
    flag = ccall((:osqp_amd_comm_unique_id, lib), Cc_int, (Ptr{UInt8}, Cstring), id, librccl === nothing ? C_NULL : librccl)
    flag == 0 || error("Error creating the RCCL id: $(last_error())")
    return id
end

"""
    rccl_comm(rank, world, id) -> Comm

ncclAllGather on the engine's stream (RCCL over xGMI); `id` from `unique_id()` of rank 0.
"""
function rccl_comm(rank::Integer, world::Integer, id::Vector{UInt8}; librccl::Union{Nothing,String} = nothing)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    flag = ccall((:osqp_amd_comm_create_rccl, lib), Cc_int, (Ptr{Ptr{Cvoid}}, Cc_int, Cc_int, Ptr{UInt8}, Cstring),
                 h, rank, world, id, librccl === nothing ? C_NULL : librccl)
    flag == 0 || error("Error creating the RCCL communicator: $(last_error())")
    return Comm(h[], rank, world, nothing)
end

"""
    host_comm(rank, world, allgather!) -> Comm

Host-staged transport: `allgather!(buf::Vector{Float64}, count)` receives world*count doubles with chunk `rank`
filled in and fills in the others (e.g. `MPI.Allgather!(MPI.IN_PLACE, UBuffer(buf, count), comm)`).
"""
function host_comm(rank::Integer, world::Integer, allgather!)
    function trampoline(ctx::Ptr{Cvoid}, buf::Ptr{Cdouble}, count::Clonglong)::Cint
        try
            allgather!(unsafe_wrap(Array, buf, world * count), Int(count))
            return 0
        catch
            return 1
        end
    end
    cb = @cfunction($trampoline, Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Clonglong))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    flag = ccall((:osqp_amd_comm_create_host, lib), Cc_int, (Ptr{Ptr{Cvoid}}, Cc_int, Cc_int, Ptr{Cvoid}, Ptr{Cvoid}),
                 h, rank, world, cb, C_NULL)
    flag == 0 || error("Error creating the host communicator: $(last_error())")
    return Comm(h[], rank, world, cb)
end

"""
    setup_sharded!(model, comm; P, q, A, l, u, settings...)

As `OSQP.setup!` [REF src/interface.jl:35-162] with the same (full) problem on every rank; the library keeps
this rank's row block.  `OSQP.solve!`, `update_q!`, `update_bounds!`, `warm_start!` then work unchanged (every
rank calls them in the same order and receives the full solution).
"""
function setup_sharded!(model::OSQP.Model, comm::Comm; P::SparseMatrixCSC, q::Vector{Float64}, A::SparseMatrixCSC,
                        l::Vector{Float64}, u::Vector{Float64}, settings...)
    n = size(P, 1); m = size(A, 1)
    Pu = istriu(P) ? P : triu(P)
    u = min.(u, OSQP.OSQP_INFTY); l = max.(l, -OSQP.OSQP_INFTY)
    managedP = OSQP.ManagedCcsc(Pu); managedA = OSQP.ManagedCcsc(A)
    Pdata = Ref(OSQP.Ccsc(managedP)); Adata = Ref(OSQP.Ccsc(managedA))
    stgs = OSQP.Settings(Dict{Symbol,Any}(settings))
    workspace = Ref{Ptr{OSQP.Workspace}}()
    flag = GC.@preserve managedP Pdata managedA Adata q l u begin   # as [REF src/interface.jl:132-155]
        data = OSQP.Data(n, m, Base.unsafe_convert(Ptr{OSQP.Ccsc}, Pdata), Base.unsafe_convert(Ptr{OSQP.Ccsc}, Adata),
                         pointer(q), pointer(l), pointer(u))
        ccall((:osqp_amd_setup_sharded, lib), Cc_int,
              (Ptr{Ptr{OSQP.Workspace}}, Ptr{OSQP.Data}, Ptr{OSQP.Settings}, Ptr{Cvoid}),
              workspace, Ref(data), Ref(stgs), comm.handle)
    end
    flag == 0 || error("Error in OSQP setup: $(last_error())")
    model.workspace = workspace[]
    resize!(model.lcache, m); resize!(model.ucache, m)
    model.isempty = false
    return model
end

# ---------------------------------------------------------------------------------------------------------
# The batched path over several GPUs (include/osqp_amd.h: osqp_amd_batch_mpc_*): `total` MPC instances cut into
# contiguous blocks over the ranks of a communicator, resident in HBM; `batch_mpc_solve!` = every rank its block
# (one workgroup per instance) + ONE in-place all-gather of the packed rows [x (100) | y (200) | iter, status, pri, dua]
# on the library's own RCCL communicator.  `packed` is a DEVICE pointer to total * 304 doubles (e.g. from AMDGPU.jl's
# allocator or hipMalloc through ccall); nothing else crosses ranks.
# ---------------------------------------------------------------------------------------------------------
mutable struct MpcBatch
    handle::Ptr{Cvoid}
    total::Int
end

function batch_mpc_create(total::Integer; seed::Integer = 1, comm::Ptr{Cvoid} = C_NULL, device::Integer = 0, settings...)
    stgs = OSQP.Settings(Dict{Symbol,Any}(settings))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    flag = ccall((:osqp_amd_batch_mpc_create, lib), Cc_int,
                 (Ptr{Ptr{Cvoid}}, Cc_int, Culonglong, Ptr{OSQP.Settings}, Ptr{Cvoid}, Cc_int),
                 h, total, seed, Ref(stgs), comm, device)
    flag == 0 || error("Error in batched setup: $(last_error())")
    b = MpcBatch(h[], total)
    finalizer(x -> ccall((:osqp_amd_batch_destroy, lib), Cc_int, (Ptr{Cvoid},), x.handle), b)
    return b
end

function batch_mpc_solve!(b::MpcBatch, packed::Ptr{Cdouble})
    flag = ccall((:osqp_amd_batch_mpc_solve, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}), b.handle, packed)
    flag == 0 || error("Error in batched solve: $(last_error())")
    return nothing
end

# ---------------------------------------------------------------------------------------------------------
# The resident batch of the caller's own QPs (include/osqp_amd.h: osqp_amd_batch_setup ... _resolve): `count` QPs sharing
# one sparsity pattern, set up once, then `batch_update!` / `batch_warm_start!` / `batch_solve!` as often as wanted -- the
# life cycle of `OSQP.setup!` / `update!` / `warm_start!` / `solve!`, instance by instance, without leaving HBM.  P (upper
# triangle) and A give the pattern; the value arrays are `count` columns of a Julia matrix (column i = instance i: the
# row-major [count x .] layout of the C side).  Array arguments are host `Matrix{Float64}` (where = 0) or device
# pointers `Ptr{Cdouble}` (where = 1, e.g. from AMDGPU.jl).  (Not executed by the test suite, like the rest of this file;
# the Python mirror `batch.ResidentBatch` is what the tests drive.)
# ---------------------------------------------------------------------------------------------------------
mutable struct ResidentBatch
    handle::Ptr{Cvoid}
    count::Int
    n::Int
    m::Int
end

function batch_setup(P::SparseMatrixCSC, A::SparseMatrixCSC, Px::Matrix{Float64}, Ax::Matrix{Float64}, q::Matrix{Float64},
                     l::Matrix{Float64}, u::Matrix{Float64}; device::Integer = 0, settings...)
    Pu = triu(P)
    n, m, count = size(A, 2), size(A, 1), size(q, 2)
    size(Px) == (nnz(Pu), count) || error("Px: expected $(nnz(Pu)) x $(count)")
    size(Ax) == (nnz(A), count) || error("Ax: expected $(nnz(A)) x $(count)")
    size(q, 1) == n || error("q: expected $(n) x $(count)")
    size(l) == (m, count) && size(u) == (m, count) || error("l, u: expected $(m) x $(count)")
    stgs = OSQP.Settings(Dict{Symbol,Any}(settings))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    Pp, Pi = Vector{Cc_int}(Pu.colptr .- 1), Vector{Cc_int}(Pu.rowval .- 1)
    Ap, Ai = Vector{Cc_int}(A.colptr .- 1), Vector{Cc_int}(A.rowval .- 1)
    flag = ccall((:osqp_amd_batch_setup, lib), Cc_int,
                 (Ptr{Ptr{Cvoid}}, Cc_int, Cc_int, Cc_int, Ptr{Cc_int}, Ptr{Cc_int}, Ptr{Cdouble}, Ptr{Cc_int}, Ptr{Cc_int}, Ptr{Cdouble},
                  Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{OSQP.Settings}, Cc_int),
                 h, count, n, m, Pp, Pi, Px, Ap, Ai, Ax, q, l, u, Ref(stgs), device)
    flag == 0 || error("Error in batched setup: $(last_error())")
    b = ResidentBatch(h[], count, n, m)
    finalizer(x -> ccall((:osqp_amd_batch_destroy, lib), Cc_int, (Ptr{Cvoid},), x.handle), b)
    return b
end

const BatchArg = Union{Nothing,Matrix{Float64},Ptr{Cdouble}}
_batch_ptr(a::Nothing) = Ptr{Cdouble}(C_NULL)
_batch_ptr(a::Matrix{Float64}) = pointer(a)
_batch_ptr(a::Ptr{Cdouble}) = a
_batch_where(args...) = any(a -> a isa Ptr{Cdouble}, args) ? 1 : 0

"New q / l / u / values of P / values of A for every instance, in the order of `OSQP.update!`; `nothing` keeps what is there."
function batch_update!(b::ResidentBatch; q::BatchArg = nothing, l::BatchArg = nothing, u::BatchArg = nothing,
                       Px::BatchArg = nothing, Ax::BatchArg = nothing)
    GC.@preserve q l u Px Ax begin
        if q !== nothing
            flag = ccall((:osqp_amd_batch_update_lin_cost, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Cc_int), b.handle, _batch_ptr(q), _batch_where(q))
            flag == 0 || error("Error in batched update: $(last_error())")
        end
        if l !== nothing || u !== nothing
            flag = ccall((:osqp_amd_batch_update_bounds, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                         b.handle, _batch_ptr(l), _batch_ptr(u), _batch_where(l, u))
            flag == 0 || error("Error in batched update: $(last_error())")
        end
        if Px !== nothing || Ax !== nothing
            flag = ccall((:osqp_amd_batch_update_matrices, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                         b.handle, _batch_ptr(Px), _batch_ptr(Ax), _batch_where(Px, Ax))
            flag == 0 || error("Error in batched update: $(last_error())")
        end
    end
    return nothing
end

function batch_warm_start!(b::ResidentBatch; x::BatchArg = nothing, y::BatchArg = nothing)
    GC.@preserve x y begin
        flag = ccall((:osqp_amd_batch_warm_start, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                     b.handle, _batch_ptr(x), _batch_ptr(y), _batch_where(x, y))
    end
    flag == 0 || error("Error in batched warm start: $(last_error())")
    return nothing
end

"Solve every instance -> (x [n x count], y [m x count], info [6 x count]: iter, status_val, pri_res, dua_res, obj_val, rho_updates)."
function batch_solve!(b::ResidentBatch)
    x, y, info = Matrix{Float64}(undef, b.n, b.count), Matrix{Float64}(undef, b.m, b.count), Matrix{Float64}(undef, 6, b.count)
    flag = ccall((:osqp_amd_batch_resolve, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int), b.handle, x, y, info, 0)
    flag == 0 || error("Error in batched solve: $(last_error())")
    return x, y, info
end

"The same into device arrays (pointers to n * count, m * count, 6 * count doubles on the handle's device)."
function batch_solve!(b::ResidentBatch, x::Ptr{Cdouble}, y::Ptr{Cdouble}, info::Ptr{Cdouble})
    flag = ccall((:osqp_amd_batch_resolve, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int), b.handle, x, y, info, 1)
    flag == 0 || error("Error in batched solve: $(last_error())")
    return nothing
end

# ---- the same calls for a selection of the instances (osqp_amd_batch_*_rows) ----------------------------------------------
# `rows`: distinct 1-based instance numbers, in any order; the arrays then have one COLUMN per selected instance, column j for
# instance rows[j].  A selected instance gets the bits of the whole-batch call; every other instance -- data, record,
# certificates, polish status -- stays as it was.  The library checks the selection (range, repeats, 1 <= k <= count).
_batch_rows(rows::AbstractVector{<:Integer}) = Vector{Cc_int}(rows .- 1)

"`batch_update!` for the instances `rows` only; only they are re-equilibrated when Px / Ax are given."
function batch_update!(b::ResidentBatch, rows::AbstractVector{<:Integer}; q::BatchArg = nothing, l::BatchArg = nothing,
                       u::BatchArg = nothing, Px::BatchArg = nothing, Ax::BatchArg = nothing)
    r = _batch_rows(rows)
    k = length(r)
    GC.@preserve q l u Px Ax begin
        if q !== nothing
            flag = ccall((:osqp_amd_batch_update_lin_cost_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Cc_int),
                         b.handle, r, k, _batch_ptr(q), _batch_where(q))
            flag == 0 || error("Error in batched update: $(last_error())")
        end
        if l !== nothing || u !== nothing
            flag = ccall((:osqp_amd_batch_update_bounds_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                         b.handle, r, k, _batch_ptr(l), _batch_ptr(u), _batch_where(l, u))
            flag == 0 || error("Error in batched update: $(last_error())")
        end
        if Px !== nothing || Ax !== nothing
            flag = ccall((:osqp_amd_batch_update_matrices_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                         b.handle, r, k, _batch_ptr(Px), _batch_ptr(Ax), _batch_where(Px, Ax))
            flag == 0 || error("Error in batched update: $(last_error())")
        end
    end
    return nothing
end

function batch_warm_start!(b::ResidentBatch, rows::AbstractVector{<:Integer}; x::BatchArg = nothing, y::BatchArg = nothing)
    r = _batch_rows(rows)
    GC.@preserve x y begin
        flag = ccall((:osqp_amd_batch_warm_start_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                     b.handle, r, length(r), _batch_ptr(x), _batch_ptr(y), _batch_where(x, y))
    end
    flag == 0 || error("Error in batched warm start: $(last_error())")
    return nothing
end

"Solve the instances `rows` only -> (x [n x k], y [m x k], info [6 x k]); k workgroups per launch."
function batch_solve!(b::ResidentBatch, rows::AbstractVector{<:Integer})
    r = _batch_rows(rows)
    k = length(r)
    x, y, info = Matrix{Float64}(undef, b.n, k), Matrix{Float64}(undef, b.m, k), Matrix{Float64}(undef, 6, k)
    flag = ccall((:osqp_amd_batch_resolve_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                 b.handle, r, k, x, y, info, 0)
    flag == 0 || error("Error in batched solve: $(last_error())")
    return x, y, info
end

"The same into device arrays (pointers to n * k, m * k, 6 * k doubles on the handle's device)."
function batch_solve!(b::ResidentBatch, rows::AbstractVector{<:Integer}, x::Ptr{Cdouble}, y::Ptr{Cdouble}, info::Ptr{Cdouble})
    r = _batch_rows(rows)
    flag = ccall((:osqp_amd_batch_resolve_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                 b.handle, r, length(r), x, y, info, 1)
    flag == 0 || error("Error in batched solve: $(last_error())")
    return nothing
end

"status_polish of every instance from the last `batch_solve!`: 1 accepted, -1 refused, 0 not polished (not Solved, or polish off)."
function batch_polish_status(b::ResidentBatch)
    st = Vector{Float64}(undef, b.count)
    flag = ccall((:osqp_amd_batch_polish_status, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Cc_int), b.handle, st, 0)
    flag == 0 || error("Error in batched polish status: $(last_error())")
    return Int.(st)
end

"The same into a device array (a pointer to `count` doubles on the handle's device)."
function batch_polish_status(b::ResidentBatch, st::Ptr{Cdouble})
    flag = ccall((:osqp_amd_batch_polish_status, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Cc_int), b.handle, st, 1)
    flag == 0 || error("Error in batched polish status: $(last_error())")
    return nothing
end

"status_polish of the instances `rows` only (osqp_amd_batch_polish_status_rows): entry j is of instance rows[j]."
function batch_polish_status(b::ResidentBatch, rows::AbstractVector{<:Integer})
    r = _batch_rows(rows)
    st = Vector{Float64}(undef, length(r))
    flag = ccall((:osqp_amd_batch_polish_status_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Cc_int),
                 b.handle, r, length(r), st, 0)
    flag == 0 || error("Error in batched polish status: $(last_error())")
    return Int.(st)
end

"The same into a device array (a pointer to k doubles on the handle's device)."
function batch_polish_status(b::ResidentBatch, rows::AbstractVector{<:Integer}, st::Ptr{Cdouble})
    r = _batch_rows(rows)
    flag = ccall((:osqp_amd_batch_polish_status_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Cc_int),
                 b.handle, r, length(r), st, 1)
    flag == 0 || error("Error in batched polish status: $(last_error())")
    return nothing
end

"Polishing of the following solves on / off and its number of refinement steps: `OSQP.update_settings!(polish = ..., polish_refine_iter = ...)` for the batch."
function batch_update_polish!(b::ResidentBatch, polish::Bool; polish_refine_iter::Integer = 3)
    flag = ccall((:osqp_amd_batch_update_polish, lib), Cc_int, (Ptr{Cvoid}, Cc_int, Cc_int), b.handle, polish ? 1 : 0, polish_refine_iter)
    flag == 0 || error("Error in batched update: $(last_error())")
    return nothing
end

const BATCH_UPDATABLE_SETTINGS = (OSQP.UPDATABLE_SETTINGS..., :scaled_termination)

"""
    batch_update_settings!(b; settings...)

`OSQP.update_settings!` for the batch (osqp_amd_batch_update_setting): the names of `OSQP.UPDATABLE_SETTINGS` and
`scaled_termination`, each checked by the rule of the single-model update; any other name is an error before the library is
called, `nothing` values are skipped.  `rho` also replaces the rho of every instance; the iterate stays.
"""
function batch_update_settings!(b::ResidentBatch; settings...)
    for (key, _) in settings
        key in BATCH_UPDATABLE_SETTINGS || error("$(key) cannot be updated or is not recognized")
    end
    given = Dict{Symbol,Any}(settings)
    for key in BATCH_UPDATABLE_SETTINGS
        value = get(given, key, nothing)
        value === nothing && continue
        flag = ccall((:osqp_amd_batch_update_setting, lib), Cc_int, (Ptr{Cvoid}, Cstring, Cdouble), b.handle, String(key), Float64(value))
        flag == 0 || error("Error in batched settings update: $(last_error())")
    end
    return nothing
end

"""
    batch_certificates(b) -> (prim_inf_cert [m x count], dual_inf_cert [n x count])

The infeasibility certificates of the last `batch_solve!` (osqp_amd_batch_certificates): column i of the first is the
direction that proves instance i primal infeasible, of the second dual infeasible, each with largest entry +-1; every other
column is NaN, and all columns before the first solve.  With m = 0 the first is `nothing`.
"""
function batch_certificates(b::ResidentBatch)
    p = b.m > 0 ? Matrix{Float64}(undef, b.m, b.count) : nothing
    d = Matrix{Float64}(undef, b.n, b.count)
    GC.@preserve p d begin
        flag = ccall((:osqp_amd_batch_certificates, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int), b.handle, _batch_ptr(p), _batch_ptr(d), 0)
    end
    flag == 0 || error("Error in batched certificates: $(last_error())")
    return p, d
end

"The same into device arrays (pointers to m * count and n * count doubles on the handle's device; `C_NULL`: not wanted)."
function batch_certificates(b::ResidentBatch, p::Ptr{Cdouble}, d::Ptr{Cdouble})
    flag = ccall((:osqp_amd_batch_certificates, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int), b.handle, p, d, 1)
    flag == 0 || error("Error in batched certificates: $(last_error())")
    return nothing
end

"The certificates of the instances `rows` only (osqp_amd_batch_certificates_rows) -> ([m x k], [n x k]); column j is of instance rows[j]."
function batch_certificates(b::ResidentBatch, rows::AbstractVector{<:Integer})
    r = _batch_rows(rows)
    k = length(r)
    p = b.m > 0 ? Matrix{Float64}(undef, b.m, k) : nothing
    d = Matrix{Float64}(undef, b.n, k)
    GC.@preserve p d begin
        flag = ccall((:osqp_amd_batch_certificates_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                     b.handle, r, k, _batch_ptr(p), _batch_ptr(d), 0)
    end
    flag == 0 || error("Error in batched certificates: $(last_error())")
    return p, d
end

"The same into device arrays (pointers to m * k and n * k doubles on the handle's device; `C_NULL`: not wanted)."
function batch_certificates(b::ResidentBatch, rows::AbstractVector{<:Integer}, p::Ptr{Cdouble}, d::Ptr{Cdouble})
    r = _batch_rows(rows)
    flag = ccall((:osqp_amd_batch_certificates_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                 b.handle, r, length(r), p, d, 1)
    flag == 0 || error("Error in batched certificates: $(last_error())")
    return nothing
end

"""
    batch_duality(b) -> [3 x count]

prim_obj, dual_obj and gap = prim_obj - dual_obj of the pair every instance's last `batch_solve!` returned (osqp_amd_batch_duality,
DESIGN.md section 19): column i is of instance i, NaN where its solve left no solution.  Every instance must be current.
"""
function batch_duality(b::ResidentBatch)
    out = Matrix{Float64}(undef, 3, b.count)
    GC.@preserve out begin
        flag = ccall((:osqp_amd_batch_duality, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Cc_int), b.handle, pointer(out), 0)
    end
    flag == 0 || error("Error in batched duality: $(last_error())")
    return out
end

"The same into a device array (a pointer to 3 * count doubles on the handle's device)."
function batch_duality(b::ResidentBatch, out::Ptr{Cdouble})
    flag = ccall((:osqp_amd_batch_duality, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Cc_int), b.handle, out, 1)
    flag == 0 || error("Error in batched duality: $(last_error())")
    return nothing
end

"The instances `rows` only (osqp_amd_batch_duality_rows) -> [3 x k]; column j is of instance rows[j]; only they must be current."
function batch_duality(b::ResidentBatch, rows::AbstractVector{<:Integer})
    r = _batch_rows(rows)
    out = Matrix{Float64}(undef, 3, length(r))
    GC.@preserve out begin
        flag = ccall((:osqp_amd_batch_duality_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Cc_int), b.handle, r, length(r), pointer(out), 0)
    end
    flag == 0 || error("Error in batched duality: $(last_error())")
    return out
end

"""
    batch_duality_gap_check!(b, on = true)

The duality gap as a third termination test of every later `batch_solve!`, whole or `rows`, inside the batched solve kernels
(osqp_amd_batch_duality_gap_check, DESIGN.md section 19): evaluated where both residual tests hold; an instance it refuses
iterates on, the others stop where they stopped before.  Off by default.  Drops nothing of the handle; the refusal counts
start from zero.
"""
function batch_duality_gap_check!(b::ResidentBatch, on::Bool = true)
    flag = ccall((:osqp_amd_batch_duality_gap_check, lib), Cc_int, (Ptr{Cvoid}, Cc_int), b.handle, on ? 1 : 0)
    flag == 0 || error("Error in batch_duality_gap_check!: $(last_error())")
    return nothing
end

"""
    batch_large!(on = true) -> Bool

The opt-in path for instances with 128 < n <= 256 (osqp_amd_batch_large, DESIGN.md section 13.1): a process-wide switch, off
at start; returns the previous value.  While it is on, the batched solve and the setup of a resident batch accept such
patterns and serve them with a kernel that reads the inverse of the reduced KKT matrix from global memory every iteration
(slower per iteration than the register kernels); every pattern with n <= 128 runs as before.  A resident batch remembers
the path it was set up on.
"""
function batch_large!(on::Bool = true)
    return ccall((:osqp_amd_batch_large, lib), Cc_int, (Cc_int,), on ? 1 : 0) != 0
end

"""
    batch_large_plan(n, m, nnzA, nnzF) -> (lds_bytes, scratch_bytes, tiles_per_wave)

What that kernel needs for a shape (osqp_amd_batch_large_plan; host only, no device is touched): nnzF counts the stored
entries of the full symmetric P.  A shape it does not take raises with the library's reason.
"""
function batch_large_plan(n::Integer, m::Integer, nnzA::Integer, nnzF::Integer)
    out = zeros(Cc_int, 3)
    GC.@preserve out begin
        flag = ccall((:osqp_amd_batch_large_plan, lib), Cc_int, (Cc_int, Cc_int, Cc_int, Cc_int, Ptr{Cc_int}), n, m, nnzA, nnzF, pointer(out))
    end
    flag == 0 || error("Error in batched plan: $(last_error())")
    return (lds_bytes = Int(out[1]), scratch_bytes = Int(out[2]), tiles_per_wave = Int(out[3]))
end

# ---------------------------------------------------------------------------------------------------------
# The shared batch (include/osqp_amd.h: osqp_amd_shared_batch_*, DESIGN.md section 13.3): ONE model (P, A, q0, l0, u0, settings)
# and `count` instances that differ in q, l and u only, on one shared inverse of the reduced KKT matrix.  Instance i is
# `setup!` on the base data, `update!(q = q[:, i], l = l[:, i], u = u[:, i])`, `solve!`.  `adaptive_rho` is set to false unless
# given; every row of every instance must keep the kind (loose / equality / inequality) it has under (l0, u0).  Arrays are one
# COLUMN per instance, host `Matrix{Float64}` or device pointers, as for the resident batch.
# ---------------------------------------------------------------------------------------------------------
mutable struct SharedBatch
    handle::Ptr{Cvoid}
    count::Int
    n::Int
    m::Int
    nnzP::Int
    nnzA::Int
end

"(T, lds_bytes, model_bytes, instance_bytes) for a shape (osqp_amd_shared_batch_plan; host only): T, the instances per workgroup, depends on the shape alone."
function shared_batch_plan(n::Integer, m::Integer, nnzA::Integer, nnzF::Integer)
    out = zeros(Cc_int, 4)
    GC.@preserve out begin
        flag = ccall((:osqp_amd_shared_batch_plan, lib), Cc_int, (Cc_int, Cc_int, Cc_int, Cc_int, Ptr{Cc_int}), n, m, nnzA, nnzF, pointer(out))
    end
    flag == 0 || error("Error in batched plan: $(last_error())")
    return (T = Int(out[1]), lds_bytes = Int(out[2]), model_bytes = Int(out[3]), instance_bytes = Int(out[4]))
end

function shared_batch_setup(P::SparseMatrixCSC, A::SparseMatrixCSC, q0::Vector{Float64}, l0::Vector{Float64}, u0::Vector{Float64},
                            count::Integer; device::Integer = 0, settings...)
    Pu = triu(P)
    n, m = size(A, 2), size(A, 1)
    length(q0) == n && length(l0) == m && length(u0) == m || error("q0, l0, u0: expected lengths $(n), $(m), $(m)")
    d = Dict{Symbol,Any}(settings)
    haskey(d, :adaptive_rho) || (d[:adaptive_rho] = false)
    stgs = OSQP.Settings(d)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    Pp, Pi = Vector{Cc_int}(Pu.colptr .- 1), Vector{Cc_int}(Pu.rowval .- 1)
    Ap, Ai = Vector{Cc_int}(A.colptr .- 1), Vector{Cc_int}(A.rowval .- 1)
    flag = ccall((:osqp_amd_shared_batch_setup, lib), Cc_int,
                 (Ptr{Ptr{Cvoid}}, Cc_int, Cc_int, Cc_int, Ptr{Cc_int}, Ptr{Cc_int}, Ptr{Cdouble}, Ptr{Cc_int}, Ptr{Cc_int}, Ptr{Cdouble},
                  Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{OSQP.Settings}, Cc_int),
                 h, count, n, m, Pp, Pi, Vector{Float64}(Pu.nzval), Ap, Ai, Vector{Float64}(A.nzval), q0, l0, u0, Ref(stgs), device)
    flag == 0 || error("Error in shared batch setup: $(last_error())")
    b = SharedBatch(h[], count, n, m, length(Pu.nzval), length(A.nzval))
    finalizer(x -> ccall((:osqp_amd_shared_batch_destroy, lib), Cc_int, (Ptr{Cvoid},), x.handle), b)
    return b
end

"New q [n x count] and / or bounds l, u [m x count] (both).  Bounds that cross or change the kind of a row are refused."
function shared_batch_update!(b::SharedBatch; q::BatchArg = nothing, l::BatchArg = nothing, u::BatchArg = nothing)
    (l === nothing) == (u === nothing) || error("l and u: a shared batch updates both bounds in one call")
    GC.@preserve q l u begin
        if q !== nothing
            flag = ccall((:osqp_amd_shared_batch_update_lin_cost, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Cc_int), b.handle, _batch_ptr(q), _batch_where(q))
            flag == 0 || error("Error in shared batch update: $(last_error())")
        end
        if l !== nothing
            flag = ccall((:osqp_amd_shared_batch_update_bounds, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                         b.handle, _batch_ptr(l), _batch_ptr(u), _batch_where(l, u))
            flag == 0 || error("Error in shared batch update: $(last_error())")
        end
    end
    return nothing
end

function shared_batch_warm_start!(b::SharedBatch; x::BatchArg = nothing, y::BatchArg = nothing)
    GC.@preserve x y begin
        flag = ccall((:osqp_amd_shared_batch_warm_start, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                     b.handle, _batch_ptr(x), _batch_ptr(y), _batch_where(x, y))
    end
    flag == 0 || error("Error in shared batch warm start: $(last_error())")
    return nothing
end

"Solve every instance in one launch -> (x [n x count], y [m x count], info [6 x count]: iter, status_val, pri_res, dua_res, obj_val, 0)."
function shared_batch_solve!(b::SharedBatch)
    x, y, info = Matrix{Float64}(undef, b.n, b.count), Matrix{Float64}(undef, b.m, b.count), Matrix{Float64}(undef, 6, b.count)
    flag = ccall((:osqp_amd_shared_batch_resolve, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int), b.handle, x, y, info, 0)
    flag == 0 || error("Error in shared batch solve: $(last_error())")
    return x, y, info
end

"The same into device arrays."
function shared_batch_solve!(b::SharedBatch, x::Ptr{Cdouble}, y::Ptr{Cdouble}, info::Ptr{Cdouble})
    flag = ccall((:osqp_amd_shared_batch_resolve, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int), b.handle, x, y, info, 1)
    flag == 0 || error("Error in shared batch solve: $(last_error())")
    return nothing
end

"max_iter, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, alpha, check_termination, scaled_termination, rho (one re-factorisation)."
function shared_batch_update_settings!(b::SharedBatch; kwargs...)
    for (key, value) in kwargs
        flag = ccall((:osqp_amd_shared_batch_update_setting, lib), Cc_int, (Ptr{Cvoid}, Cstring, Cdouble), b.handle, String(key), Float64(value))
        flag == 0 || error("Error in shared batch settings update: $(last_error())")
    end
    return nothing
end

shared_batch_device_bytes(b::SharedBatch) = Int(ccall((:osqp_amd_shared_batch_device_bytes, lib), Cc_int, (Ptr{Cvoid},), b.handle))
shared_batch_launches() = Int(ccall((:osqp_amd_shared_batch_launches, lib), Cc_int, ()))

"""
    shared_batch_adjoint(b; dx = nothing, dy = nothing, want = (:q, :l, :u, :Px, :Ax), sums = ()) -> NamedTuple

Gradients of a scalar loss through the solutions of the last `shared_batch_solve!` (osqp_amd_shared_batch_adjoint, DESIGN.md
section 13.4).  dx [n x count] / dy [m x count] (or [n x count x ncot] / [m x count x ncot] for several cotangents; `nothing` =
zeros, not both).  Returns the entries of `want` per instance ([cols x count] or [cols x count x ncot]), the entries of `sums`
(a subset of (:Px, :Ax)) as `Px_sum` / `Ax_sum` ([nnz] or [nnz x ncot]: the gradients of the SHARED values, summed over the
instances on the device in blocks of 16 -- the order is in include/osqp_amd.h), plus `act` [m x count] and `status` [count].
Refused before the first solve and after any update, warm start or rho update that followed the last one.
"""
function shared_batch_adjoint(b::SharedBatch; dx::Union{Nothing,Array{Float64}} = nothing, dy::Union{Nothing,Array{Float64}} = nothing,
                              want = (:q, :l, :u, :Px, :Ax), sums = ())
    all(w -> w in (:q, :l, :u, :Px, :Ax), want) || error("want: expected a subset of (:q, :l, :u, :Px, :Ax)")
    all(w -> w in (:Px, :Ax), sums) || error("sums: expected a subset of (:Px, :Ax)")
    dx === nothing && dy === nothing && error("dx and dy: at least one incoming gradient is needed")
    ref = dx === nothing ? dy : dx
    many = ndims(ref) == 3
    ncot = many ? size(ref, 3) : 1
    for (name, v, k) in (("dx", dx, b.n), ("dy", dy, b.m))
        v === nothing || size(v) == (many ? (k, b.count, ncot) : (k, b.count)) || error("$(name): expected [$(k) x $(b.count)] or [$(k) x $(b.count) x ncot]")
    end
    cols = (q = b.n, l = b.m, u = b.m, Px = b.nnzP, Ax = b.nnzA)
    per = Dict(k => (k in want && cols[k] > 0 ? (many ? zeros(cols[k], b.count, ncot) : zeros(cols[k], b.count)) : nothing) for k in keys(cols))
    tot = Dict(k => (k in sums && cols[k] > 0 ? (many ? zeros(cols[k], ncot) : zeros(cols[k])) : nothing) for k in (:Px, :Ax))
    act, status = zeros(b.m, b.count), zeros(b.count)
    p(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(a)
    GC.@preserve dx dy per tot act status begin
        flag = ccall((:osqp_amd_shared_batch_adjoint, lib), Cc_int,
                     (Ptr{Cvoid}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                      Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                     b.handle, ncot, p(dx), p(dy), p(per[:q]), p(per[:l]), p(per[:u]), p(per[:Px]), p(per[:Ax]), p(tot[:Px]), p(tot[:Ax]),
                     b.m > 0 ? pointer(act) : Ptr{Cdouble}(C_NULL), pointer(status), 0)
    end
    flag == 0 || error("Error in shared batch adjoint: $(last_error())")
    return (q = per[:q], l = per[:l], u = per[:u], Px = per[:Px], Ax = per[:Ax], Px_sum = tot[:Px], Ax_sum = tot[:Ax],
            act = Matrix{Int}(act), status = Vector{Int}(status))
end

"Accepted `shared_batch_adjoint` calls of this process: one per call whatever ncot; a refused call does not count."
shared_batch_adjoint_launches() = Int(ccall((:osqp_amd_shared_batch_adjoint_launches, lib), Cc_int, ()))

"""
    shared_batch_jvp(b; tq = nothing, tl = nothing, tu = nothing, tPx = nothing, tAx = nothing) -> NamedTuple

Forward sensitivities of the solutions of the last `shared_batch_solve!` along directions of the data
(osqp_amd_shared_batch_jvp, DESIGN.md section 13.5).  tq [n x count], tl, tu [m x count] are PER INSTANCE; tPx [nnzP] and tAx [nnzA]
are ONE tangent of the SHARED values for the whole batch, in the index spaces of `Px_sum` / `Ax_sum` (`nothing` = zeros, not
all).  Or all with a trailing axis, [. x count x ndir] and [nnz x ndir], for several directions in one call.  Returns `x`
[n x count (x ndir)], `y` [m x count (x ndir)], `act` [m x count] and `status` [count], as `shared_batch_adjoint` returns them.  On a
row with l == u only `tl` is read.  Refused before the first solve and after any update, warm start or rho update that followed
the last one.
"""
function shared_batch_jvp(b::SharedBatch; tq::Union{Nothing,Array{Float64}} = nothing, tl::Union{Nothing,Array{Float64}} = nothing,
                          tu::Union{Nothing,Array{Float64}} = nothing, tPx::Union{Nothing,Array{Float64}} = nothing,
                          tAx::Union{Nothing,Array{Float64}} = nothing)
    per = (("tq", tq, b.n), ("tl", tl, b.m), ("tu", tu, b.m))
    shared = (("tPx", tPx, b.nnzP), ("tAx", tAx, b.nnzA))
    extra = vcat([ndims(v) - 2 for (_, v, _) in per if v !== nothing], [ndims(v) - 1 for (_, v, _) in shared if v !== nothing])
    isempty(extra) && error("tq, tl, tu, tPx, tAx: at least one tangent is needed")
    (all(==(extra[1]), extra) && extra[1] in (0, 1)) ||
        error("tangents: expected tq, tl, tu [cols x count] with tPx, tAx [nnz], or all with a trailing axis [... x ndir]")
    many = extra[1] == 1
    given = [v for (_, v, _) in (per..., shared...) if v !== nothing]
    ndir = many ? size(given[1], ndims(given[1])) : 1
    ndir >= 1 || error("tangents: ndir must be at least 1")
    for (name, v, k) in per
        v === nothing || size(v) == (many ? (k, b.count, ndir) : (k, b.count)) || error("$(name): expected [$(k) x $(b.count)] or [$(k) x $(b.count) x ndir]")
    end
    for (name, v, k) in shared
        v === nothing || size(v) == (many ? (k, ndir) : (k,)) || error("$(name): expected [$(k)] or [$(k) x ndir]")
    end
    tx = many ? zeros(b.n, b.count, ndir) : zeros(b.n, b.count)
    ty = many ? zeros(b.m, b.count, ndir) : zeros(b.m, b.count)
    act, status = zeros(b.m, b.count), zeros(b.count)
    p(a) = (a === nothing || isempty(a)) ? Ptr{Cdouble}(C_NULL) : pointer(a)
    GC.@preserve tq tl tu tPx tAx tx ty act status begin
        flag = ccall((:osqp_amd_shared_batch_jvp, lib), Cc_int,
                     (Ptr{Cvoid}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                      Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                     b.handle, ndir, p(tq), p(tl), p(tu), p(tPx), p(tAx), pointer(tx), p(ty), p(act), pointer(status), 0)
    end
    flag == 0 || error("Error in shared batch jvp: $(last_error())")
    return (x = tx, y = ty, act = Matrix{Int}(act), status = Vector{Int}(status))
end

"Accepted `shared_batch_jvp` calls of this process: one per call whatever ndir; a refused call does not count."
shared_batch_jvp_launches() = Int(ccall((:osqp_amd_shared_batch_jvp_launches, lib), Cc_int, ()))

"""
    batch_large_factor!(b, on = true) -> Bool

Polish, adjoint and JVP on a resident batch with 128 < n <= 256 (osqp_amd_batch_large_factor, DESIGN.md section 13.2): a switch
per handle, off after setup; returns the previous value.  While it is on the three kernels keep the factor of M in the
instance's block of global scratch.  A batch with n <= 128 raises.
"""
function batch_large_factor!(b::ResidentBatch, on::Bool = true)
    before = ccall((:osqp_amd_batch_large_factor, lib), Cc_int, (Ptr{Cvoid}, Cc_int), b.handle, on ? 1 : 0)
    before >= 0 || error("Error in batch_large_factor!: $(last_error())")
    return before != 0
end

"""
    batch_large_factor_plan(n, m, nnzA, nnzF) -> (lds_bytes, scratch_bytes, nb)

What those kernels need for a shape (osqp_amd_batch_large_factor_plan; host only): nnzF counts the stored entries of the full
symmetric P.  A shape they do not take raises with the library's reason.
"""
function batch_large_factor_plan(n::Integer, m::Integer, nnzA::Integer, nnzF::Integer)
    out = zeros(Cc_int, 3)
    GC.@preserve out begin
        flag = ccall((:osqp_amd_batch_large_factor_plan, lib), Cc_int, (Cc_int, Cc_int, Cc_int, Cc_int, Ptr{Cc_int}), n, m, nnzA, nnzF, pointer(out))
    end
    flag == 0 || error("Error in batched plan: $(last_error())")
    return (lds_bytes = Int(out[1]), scratch_bytes = Int(out[2]), nb = Int(out[3]))
end

"[count]: the checks of every instance's own last `batch_solve!` that the gap test alone refused (osqp_amd_batch_gap_refusals); zeros while the rule is off."
function batch_gap_refusals(b::ResidentBatch)
    out = Vector{Float64}(undef, b.count)
    GC.@preserve out begin
        flag = ccall((:osqp_amd_batch_gap_refusals, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Cc_int), b.handle, pointer(out), 0)
    end
    flag == 0 || error("Error in batched gap refusals: $(last_error())")
    return out
end

"The instances `rows` only (osqp_amd_batch_gap_refusals_rows) -> [k]; entry j is of instance rows[j]."
function batch_gap_refusals(b::ResidentBatch, rows::AbstractVector{<:Integer})
    r = _batch_rows(rows)
    out = Vector{Float64}(undef, length(r))
    GC.@preserve out begin
        flag = ccall((:osqp_amd_batch_gap_refusals_rows, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Cc_int), b.handle, r, length(r), pointer(out), 0)
    end
    flag == 0 || error("Error in batched gap refusals: $(last_error())")
    return out
end

const AdjointArg = Union{Nothing,Matrix{Float64},Array{Float64,3},Ptr{Cdouble}}
_batch_ptr(a::Array{Float64,3}) = pointer(a)

"""
    batch_adjoint!(b; dx = nothing, dy = nothing, dq = nothing, dl = nothing, du = nothing, dPx = nothing, dAx = nothing,
                   act = nothing, status = nothing, rows = nothing, ncot = nothing)

Gradients of a scalar loss through the solutions of the last `batch_solve!` (osqp_amd_batch_adjoint in include/osqp_amd.h):
`dx` [n x count] and `dy` [m x count] are the loss's gradients with respect to x and y (`nothing` = zero, not both); every
output that is given is filled in place -- `dq` [n x count], `dl`, `du`, `act` [m x count], `dPx` [nnz(triu(P)) x count],
`dAx` [nnz(A) x count], `status` [1 x count] -- and `nothing` means not wanted.  All arrays are host matrices or all are
device pointers, as for `batch_update!`.  The handle must have been solved since its last update or warm start.
`rows` (distinct 1-based instance numbers, any order): the instances `rows` only, in a launch of k workgroups
(osqp_amd_batch_adjoint_rows); every array then has one column per selected instance, column j for instance rows[j], and
only the selected instances must have been solved since their last update or warm start.
`ncot` (>= 1): that many pairs (`dx`, `dy`) per instance in ONE launch (osqp_amd_batch_adjoint_multi, _multi_rows) -- one
factorisation per instance, one solve per cotangent.  `dx`, `dy` and the five gradients then have a third axis,
[. x count x ncot] ([. x k x ncot] with `rows`; host arrays `Array{Float64,3}`, whose third axis must be `ncot`), while `act` and
`status` stay per instance.  `nothing`: the one-cotangent entries, as before.  Like the rest of this file the keyword is not
executed by the test suite; the Python mirror (`ResidentBatch.adjoint` with a leading axis) is.
"""
function batch_adjoint!(b::ResidentBatch; dx::AdjointArg = nothing, dy::AdjointArg = nothing, dq::AdjointArg = nothing,
                        dl::AdjointArg = nothing, du::AdjointArg = nothing, dPx::AdjointArg = nothing, dAx::AdjointArg = nothing,
                        act::BatchArg = nothing, status::BatchArg = nothing,
                        rows::Union{Nothing,AbstractVector{<:Integer}} = nothing, ncot::Union{Nothing,Integer} = nothing)
    all_args = (dx, dy, dq, dl, du, dPx, dAx, act, status)
    given = filter(a -> a !== nothing, collect(all_args))
    if ncot !== nothing
        ncot >= 1 || error("batch_adjoint!: ncot must be at least 1")
        all(a -> a isa Ptr{Cdouble}, given) || all(a -> a isa Array{Float64}, given) ||
            error("batch_adjoint!: the arrays must all be host arrays or all device pointers")
        all(a -> !(a isa Array{Float64}) || (ndims(a) == 3 && size(a, 3) == ncot), all_args[1:7]) ||
            error("batch_adjoint!: with ncot, dx, dy and the gradients are [. x count x ncot]")
        GC.@preserve dx dy dq dl du dPx dAx act status begin
            if rows !== nothing
                r = _batch_rows(rows)
                flag = ccall((:osqp_amd_batch_adjoint_multi_rows, lib), Cc_int,
                             (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                              Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                             b.handle, r, length(r), ncot, map(_batch_ptr, all_args)..., _batch_where(all_args...))
            else
                flag = ccall((:osqp_amd_batch_adjoint_multi, lib), Cc_int,
                             (Ptr{Cvoid}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                              Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                             b.handle, ncot, map(_batch_ptr, all_args)..., _batch_where(all_args...))
            end
        end
        flag == 0 || error("Error in batched adjoint: $(last_error())")
        return nothing
    end
    all(a -> a isa Ptr{Cdouble}, given) || all(a -> a isa Matrix{Float64}, given) ||
        error("batch_adjoint!: the arrays must all be host matrices or all device pointers")
    if rows !== nothing
        r = _batch_rows(rows)
        GC.@preserve dx dy dq dl du dPx dAx act status begin
            flag = ccall((:osqp_amd_batch_adjoint_rows, lib), Cc_int,
                         (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                          Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                         b.handle, r, length(r), map(_batch_ptr, all_args)..., _batch_where(all_args...))
        end
        flag == 0 || error("Error in batched adjoint: $(last_error())")
        return nothing
    end
    GC.@preserve dx dy dq dl du dPx dAx act status begin
        flag = ccall((:osqp_amd_batch_adjoint, lib), Cc_int,
                     (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                      Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                     b.handle, map(_batch_ptr, all_args)..., _batch_where(all_args...))
    end
    flag == 0 || error("Error in batched adjoint: $(last_error())")
    return nothing
end

const JvpArg = AdjointArg

"""
    batch_jvp!(b; tq = nothing, tl = nothing, tu = nothing, tPx = nothing, tAx = nothing, tx = nothing, ty = nothing,
               act = nothing, status = nothing, ndir = nothing, rows = nothing)

Forward sensitivities of the solutions of the last `batch_solve!` along directions of the data (osqp_amd_batch_jvp in
include/osqp_amd.h): the tangents `tq` [n x count], `tl`, `tu` [m x count], `tPx` [nnz(triu(P)) x count], `tAx`
[nnz(A) x count] (`nothing` = zero, not all five), or each with a third axis [. x count x ndir] for several directions in one
launch (one factorisation per instance, one solve per direction).  `tx` [n x count (x ndir)] and `ty` [m x count (x ndir)]
are filled in place (`nothing` = not wanted, not both), as are `act` [m x count] and `status` [1 x count], once per call.  All
arrays are host arrays or all are device pointers, as for `batch_adjoint!`; with device pointers `ndir` gives the number of
directions (default 1), with host arrays it is read from the third axis and all arrays must agree.  The handle must have
been solved since its last update or warm start.  `rows` (distinct 1-based instance numbers, any order): the instances
`rows` only, in a launch of k workgroups (osqp_amd_batch_jvp_rows); every array then has k columns, [. x k (x ndir)], column
j for instance rows[j], and only the selected instances must be current.  Julia is not installed in the build image: like the rest of this file
this function is not executed by the test suite; the Python mirror (`ResidentBatch.jvp`) is.
"""
function batch_jvp!(b::ResidentBatch; tq::JvpArg = nothing, tl::JvpArg = nothing, tu::JvpArg = nothing, tPx::JvpArg = nothing,
                    tAx::JvpArg = nothing, tx::JvpArg = nothing, ty::JvpArg = nothing, act::BatchArg = nothing,
                    status::BatchArg = nothing, ndir::Union{Nothing,Integer} = nothing,
                    rows::Union{Nothing,AbstractVector{<:Integer}} = nothing)
    dirs = (tq, tl, tu, tPx, tAx, tx, ty)
    all_args = (dirs..., act, status)
    given = filter(a -> a !== nothing, collect(all_args))
    all(a -> a isa Ptr{Cdouble}, given) || all(a -> a isa Array{Float64}, given) ||
        error("batch_jvp!: the arrays must all be host arrays or all device pointers")
    host = filter(a -> a isa Array{Float64}, collect(dirs))
    if !isempty(host)
        counts = unique(map(a -> size(a, 3), host))
        length(counts) == 1 && length(unique(map(ndims, host))) == 1 ||
            error("batch_jvp!: the tangents and tx, ty must all have the same number of directions")
        ndir === nothing || ndir == counts[1] || error("batch_jvp!: ndir does not match the arrays")
        ndir = counts[1]
    end
    nd = ndir === nothing ? 1 : Int(ndir)
    if rows !== nothing
        r = _batch_rows(rows)
        GC.@preserve tq tl tu tPx tAx tx ty act status begin
            flag = ccall((:osqp_amd_batch_jvp_rows, lib), Cc_int,
                         (Ptr{Cvoid}, Ptr{Cc_int}, Cc_int, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                          Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                         b.handle, r, length(r), nd, map(_batch_ptr, all_args)..., _batch_where(all_args...))
        end
        flag == 0 || error("Error in batched sensitivities: $(last_error())")
        return nothing
    end
    GC.@preserve tq tl tu tPx tAx tx ty act status begin
        flag = ccall((:osqp_amd_batch_jvp, lib), Cc_int,
                     (Ptr{Cvoid}, Cc_int, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                      Ptr{Cdouble}, Ptr{Cdouble}, Cc_int),
                     b.handle, nd, map(_batch_ptr, all_args)..., _batch_where(all_args...))
    end
    flag == 0 || error("Error in batched sensitivities: $(last_error())")
    return nothing
end

"In-place all-gather of `count` doubles per rank on a device buffer, on the library's communicator."
function comm_all_gather!(comm::Ptr{Cvoid}, buf::Ptr{Cdouble}, count::Integer)
    flag = ccall((:osqp_amd_comm_all_gather, lib), Cc_int, (Ptr{Cvoid}, Ptr{Cdouble}, Cc_int), comm, buf, count)
    flag == 0 || error("Error in all-gather: $(last_error())")
    return nothing
end


end # module
