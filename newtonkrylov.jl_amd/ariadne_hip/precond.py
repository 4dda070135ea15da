"""Preconditioners for the device GMRES / FGMRES / CG: Krylov.jl's right `N` and left `M` (ldiv =
false: z = P v approximates J^{-1} v; for CG, M is the SPD preconditioner).  SURVEY.md §8f rank 3:
device Jacobi and ILU(0) preconditioners built from the Jacobian, an inner GMRES, a geometric multigrid
V-cycle for the stencil Jacobians (MultigridPreconditioner / `multigrid`), and any other
preconditioner supplied as device code (UserPreconditioner).

`newton_krylov_(…, N=factory, M=factory)`: a factory is called as `factory(J)` once per Newton step
(the JacobianOperator of that step) and returns one of these (e.g. `N=jacobi`, `M=ilu0`, `N=multigrid`).
"""
from __future__ import annotations

import sys

from . import _lib
from ._lib import load
from .device import DeviceArray


class Preconditioner:
    """Base: `as_c()` returns the nk_precond descriptor (kept alive by the object)."""

    def as_c(self) -> _lib.nk_precond:
        raise NotImplementedError

    def apply(self, J, v: DeviceArray, z: DeviceArray | None = None) -> DeviceArray:
        """z = N v (Krylov.jl's mulorldiv!(z, N, v, ldiv)); J = the JacobianOperator a GMRES
        preconditioner solves with (its u / F0 / Jv mode)."""
        import ctypes as C

        z = v.zero() if z is None else z
        prob = J.problem()
        F0 = J.res.ptr if J.jv_mode == _lib.NK_JV_FD else None
        v.ctx.check(load().nk_precond_apply(v.ctx.handle, C.byref(prob), C.byref(self.as_c()), J.u.ptr, F0,
                                            J.jv_mode, z.ptr, v.ptr), "mul!(z, N, v)")
        return z


class DiagonalPreconditioner(Preconditioner):
    """z = d .* v with a device grid function d (NK_PRECOND_DIAG)."""

    def __init__(self, d: DeviceArray):
        self.d = d
        self._c = _lib.nk_precond(_lib.NK_PRECOND_DIAG, d.ptr, _lib.NK_USER_PRECOND(), None)

    def as_c(self):
        return self._c


class UserPreconditioner(Preconditioner):
    """z = N v computed by `apply(z, v)` on DeviceArray views, on the library's stream (runs inside
    ctx.torch_stream() when torch is loaded, like a UserResidual)."""

    def __init__(self, apply, grid, ctx):
        self.apply, self.grid, self.ctx = apply, grid, ctx

        def run(_d, _c, out, inp):
            try:
                o, i = DeviceArray(grid, ctx, _ptr=out), DeviceArray(grid, ctx, _ptr=inp)
                if "torch" in sys.modules:
                    with ctx.torch_stream():
                        apply(o, i)
                else:
                    apply(o, i)
                return 0
            except BaseException as e:
                _lib.set_user_error(e)
                return 1

        self._cb = _lib.NK_USER_PRECOND(run)
        self._c = _lib.nk_precond(_lib.NK_PRECOND_USER, None, self._cb, None)

    def as_c(self):
        return self._c


def jacobian_diag(J, reciprocal: bool = False) -> DeviceArray:
    """diag(J(u)) of a built-in residual on the device (bit-identical to the diagonal of collect(J))."""
    import ctypes as C

    out = J.u.zero()
    prob = J.problem()
    J.u.ctx.check(load().nk_jacobian_diag(J.u.ctx.handle, C.byref(prob), out.ptr, J.u.ptr, int(bool(reciprocal))),
                  "nk_jacobian_diag")
    return out


def jacobi(J) -> DiagonalPreconditioner:
    """Jacobi preconditioner N = diag(J(u))^{-1} (the reference's examples build theirs from
    collect(J), bratu.jl:121-137); use as `N=jacobi` in newton_krylov_ (called per Newton step)."""
    return DiagonalPreconditioner(jacobian_diag(J, reciprocal=True))


class GmresPreconditioner(Preconditioner):
    """`GmresPreconditioner(J, itmax)` of examples/bratu.jl:139-157: mul!(y, P, x) runs
    `gmres(P.J, x; P.itmax)` (Krylov.jl defaults: memory 20, no restart, atol = rtol = √eps) and copies
    the solution into y.  Here the inner solve is the device GMRES on J's operator (NK_PRECOND_GMRES),
    in a workspace of its own; use it with algo="fgmres" (N changes from step to step)."""

    def __init__(self, J, itmax: int, workspace=None):
        from .krylov import KrylovConstructor, krylov_workspace

        self.J, self.itmax = J, int(itmax)
        self.ws = workspace or krylov_workspace("gmres", KrylovConstructor(J.u, memory=20))
        self._c = _lib.nk_precond(_lib.NK_PRECOND_GMRES, None, _lib.NK_USER_PRECOND(), None, self.ws.handle, self.itmax)

    def as_c(self):
        return self._c


def gmres_preconditioner(itmax: int):
    """N factory `(J) -> GmresPreconditioner(J, itmax)` for newton_krylov_ (bratu.jl:150-155); the
    inner workspace is allocated once and reused by every Newton step."""
    cache = {}

    def factory(J):
        key = (id(J.u.ctx), J.u.grid)
        if key not in cache:
            cache.clear()
            cache[key] = GmresPreconditioner(J, itmax).ws
        return GmresPreconditioner(J, itmax, workspace=cache[key])

    return factory


class Ilu0Preconditioner(Preconditioner):
    """`ilu(collect(J))` (examples/bratu.jl:119-137, used with krylov_kwargs = (; ldiv = true)) on the
    device: ILU(0) of J(u) in natural order on J's own sparsity pattern -- for the 1D Bratu Jacobian
    (tridiagonal) this is its exact LU, as IncompleteLU.jl's threshold ILU is there.  Factored once
    (nk_ilu0_factor), applied as z = (L U)^-1 v by two wavefront sweeps (NK_PRECOND_ILU0).  A
    factorisation: it is applied by division, so ldiv=True is accepted (and implied)."""

    ldiv = True

    def __init__(self, J):
        import ctypes as C

        self.J = J
        self.d = J.u.zero()
        prob = J.problem()
        J.u.ctx.check(load().nk_ilu0_factor(J.u.ctx.handle, C.byref(prob), J.u.ptr, self.d.ptr), "nk_ilu0_factor")
        self._c = _lib.nk_precond(_lib.NK_PRECOND_ILU0, self.d.ptr, _lib.NK_USER_PRECOND(), None, None, 0)

    def as_c(self):
        return self._c


def ilu0(J) -> Ilu0Preconditioner:
    """N factory: `N = ilu0` is the device counterpart of `N = (J) -> ilu(collect(J))`."""
    return Ilu0Preconditioner(J)


class MultigridPreconditioner(Preconditioner):
    """One geometric multigrid V-cycle on the stencil Jacobian J(u) = Σ_a k_a δ²_a + diag(s) (NK_PRECOND_MG,
    DESIGN.md §10): weighted Jacobi smoothing (`nu` pre / post sweeps, `coarse_sweeps` on the coarsest
    level, weight `omega`, default 2d / (2d + 1)), per axis n -> n // 2 while n > 3 (`max_levels` = 0: until
    every axis is <= 3), rediscretised coarse operators, linear prolongation, restriction D^-1 P^T.  A fixed
    linear map: valid as N or M of gmres as well as fgmres.  Built-in stencil residuals, bc_zero_, one
    rank (`distributed=True`: slabs; `periodic=True`: bc_periodic_); everything else raises NotImplementedError.
    `update(J)` refreshes s = λ exp(u) for a new u.

    `spd=True` (or `.spd = True` at any time) is the SPD form for CG's M: z = σ V(v) with σ the sign of the level-0
    diagonal (-1 for the built-in Jacobians, which are negative definite: M = -V, as the Jacobi M is
    -1 ./ diag(J)), exactly the default result times σ, on the leading levels whose diagonal has that sign.

    `coarsening="semi"`: on every level only the axes whose coupling c_a = |k_a| / h_a² is at least `threshold` (in
    (0, 1], default 0.5) times the strongest one are halved, until the level is isotropic; then every axis is, as
    with "full" (nk_mg_plan_semi / nk_mg_create_levels; the same smoother and transfers, and the SPD form carries
    over).  Switch to it when the spacings of the grid differ between the axes (a non-square grid on the unit
    square: 16384 x 2048 has c_x = 64 c_y) or, with from_coefficients, when k does: point Jacobi with full
    coarsening does not damp the error that is smooth along the strong axis only, and the Krylov step count grows
    with the ratio.  Where the couplings are within a factor 1 / threshold of each other both give
    the same levels.  The default stays "full".

    `distributed=True`: the hierarchy on a slab-distributed grid (`ah.slab` on a context of several ranks, equal
    slabs: the global extent of the slowest axis is nranks x the local one).  Each level's rows are split over the
    ranks; level l + 1 exists only while the local slab extent is even (`multigrid_plan(local, nranks=R)`), so the
    cycle is the one-rank cycle of the global grid with `max_levels` = that count, bit for bit, and its coarsest
    level runs `coarse_sweeps` sweeps -- raise them on many ranks.  Construction, `update` and
    `set_coefficients` are collective, and every rank must apply the cycle; `levels` reports local extents.  2D and
    3D built-in kinds, bc_zero_, full coarsening, no 3D blocks.  Without the flag a distributed context or a slab
    keeps raising NotImplementedError.

    `periodic=True`: the hierarchy of a periodic grid, for the heat residuals with bc_periodic_ on one rank.  The levels
    are nested (coarse point j is fine point 2 j): an axis is halved while it is even and has at least 6 points
    (`multigrid_plan(shape, periodic=True)`), so extents (3, 4 or 5) * 2^k are the intended ones -- an odd axis is never
    coarsened, which is valid but weak.  Neighbours and transfers wrap, the coarse operators keep the period
    (h_l = h_0 n_0 / n_l); smoother, cycle, sign check, `spd`, `update` and `set_coefficients` work as above.  The
    nearly constant mode (eigenvalue s = -1 against a large diagonal) is left to the Krylov method.
    Full coarsening, not distributed.  Without the flag a periodic problem keeps raising NotImplementedError."""

    def __init__(self, J, nu: int = 2, coarse_sweeps: int = 8, omega: float | None = None, max_levels: int = 0,
                 spd: bool = False, coarsening: str = "full", threshold: float = 0.5, distributed: bool = False,
                 periodic: bool = False):
        self.distributed, self.periodic = bool(distributed), bool(periodic)
        prob = _mg_problem(J, distributed, coarsening, periodic)
        # the built-in Jacobians have the same k on every axis: the plan depends on the spacings alone
        self._create(J.u.ctx, J.u.grid, prob, nu, coarse_sweeps, omega, max_levels, coarsening, threshold, None)
        self.spd = spd
        self.update(J)

    def _create(self, ctx, grid, prob, nu, coarse_sweeps, omega, max_levels, coarsening="full", threshold=0.5, k=None):
        import ctypes as C

        coarsening, threshold = _mg_coarsening(coarsening, threshold)
        self.ctx, self.grid, self.handle = ctx, grid, None
        self.caller_operator = False  # True: k and s came from from_coefficients, and update(J) is not applied
        self.coarsening, self.threshold = coarsening, threshold
        self.opts = _lib.nk_mg_opts(int(nu), int(coarse_sweeps), float(omega or 0.0), int(max_levels))
        h = C.c_void_p()
        if coarsening == "full":
            ctx.check(load().nk_mg_create(ctx.handle, C.byref(prob), C.byref(self.opts), C.byref(h)), "nk_mg_create")
        else:
            lv = multigrid_plan(grid.shape_xyz, max_levels, coarsening="semi", h=[prob.hx, prob.hy, prob.hz][: grid.dim], k=k,
                                threshold=threshold)
            ext = (C.c_int64 * (3 * len(lv)))(*[n for e in lv for n in (list(e) + [1, 1])[:3]])
            ctx.check(load().nk_mg_create_levels(ctx.handle, C.byref(prob), C.byref(self.opts), ext, len(lv), C.byref(h)),
                      "nk_mg_create_levels")
        self.handle = h
        self._c = _lib.nk_precond(_lib.NK_PRECOND_MG, None, _lib.NK_USER_PRECOND(), h, None, 0)

    @classmethod
    def from_coefficients(cls, grid, k, s, *, h=None, ctx=None, nu: int = 2, coarse_sweeps: int = 8,
                          omega: float | None = None, max_levels: int = 0, spd: bool = False, coarsening: str = "full",
                          threshold: float = 0.5, distributed: bool = False, periodic: bool = False):
        """The V-cycle for A = Σ_a k[a] δ²_a(h[a]) + diag(s) on `grid` with caller-supplied coefficients: k per
        axis, s a DeviceArray on the grid or a constant; h = the spacings (default 1 / (n + 1) per axis).  Such an
        object keeps the caller's operator: the Newton drivers do not refresh it from the Jacobian (so it also
        serves a UserResidual); call update(J) yourself to switch it to a built-in J's coefficients.
        coarsening="semi": the plan is made from this k and h (a later set_coefficients keeps it).
        distributed=True: `grid` is this rank's slab (ah.slab, equal slabs) and s its slab of the coefficient; the
        default spacings are those of the global grid.
        periodic=True: the operator on the periodic grid (2D / 3D; neighbours wrap), default spacings 1 / n per axis."""
        from .device import default_context

        _mg_coarsening(coarsening, threshold)
        if periodic:
            _mg_periodic_check(distributed, coarsening)
            if grid.dim == 1:
                raise NotImplementedError("multigrid: periodic=True covers 2D and 3D grids (there is no periodic 1D kind)")
        self = cls.__new__(cls)
        self.distributed, self.periodic = bool(distributed), bool(periodic)
        ctx = ctx or (s.ctx if isinstance(s, DeviceArray) else default_context())
        if distributed:
            _mg_slab_check(ctx, grid, coarsening)
        elif getattr(ctx, "nranks", 1) != 1 or tuple(grid.shape_xyz) != tuple(grid.global_xyz):
            raise NotImplementedError("multigrid: one rank only (a distributed grid needs distributed=True)")
        k = [float(x) for x in (k if hasattr(k, "__len__") else [k] * grid.dim)]
        if len(k) != grid.dim:
            raise ValueError("k: one coefficient per axis")
        h = [float(x) for x in (h if h is not None else [1.0 / (n if periodic else n + 1) for n in grid.global_xyz])]
        if len(h) != grid.dim:
            raise ValueError("h: one spacing per axis")
        if isinstance(s, DeviceArray) and s.grid != grid:
            raise ValueError("s must be a DeviceArray on `grid` (or a constant)")
        prob = grid.geometry_problem()
        prob.hx, prob.hy, prob.hz = (h + [1.0, 1.0])[:3]
        if periodic:  # the carrier kind: a heat kind of the grid's dimension, which bc_periodic_ is defined for
            prob.kind, prob.bc = (_lib.NK_HEAT2D_EULER if grid.dim == 2 else _lib.NK_HEAT3D_EULER), _lib.NK_BC_PERIODIC
        self._create(ctx, grid, prob, nu, coarse_sweeps, omega, max_levels, coarsening, threshold, k)
        self.spd = spd
        return self.set_coefficients(k, s)

    def set_coefficients(self, k, s) -> "MultigridPreconditioner":
        """Other caller-supplied coefficients on the live hierarchy (nk_mg_set_operator): k per axis, s a
        DeviceArray on the grid or a constant, as in from_coefficients; the spacings stay.  The sign check runs
        again, so `levels` may change."""
        import ctypes as C

        k = [float(x) for x in (k if hasattr(k, "__len__") else [k] * self.grid.dim)]
        if len(k) != self.grid.dim:
            raise ValueError("k: one coefficient per axis")
        if isinstance(s, DeviceArray) and s.grid != self.grid:
            raise ValueError("s must be a DeviceArray on `grid` (or a constant)")
        kk = (C.c_double * 3)(*(k + [0.0, 0.0])[:3])
        sd, sc = (s.ptr, 0.0) if isinstance(s, DeviceArray) else (None, float(s))
        self.ctx.check(load().nk_mg_set_operator(self.handle, kk, sd, sc), "nk_mg_set_operator")
        self.caller_operator = True
        return self

    def update(self, J) -> "MultigridPreconditioner":
        """k and s of J(u) at J's current u (nk_mg_set_jacobian): call after u changed."""
        import ctypes as C

        prob = _mg_problem(J, getattr(self, "distributed", False), periodic=getattr(self, "periodic", False))
        self.caller_operator = False
        if J.u.grid != self.grid or J.u.ctx is not self.ctx:
            raise ValueError("multigrid: J lives on another grid / context than the hierarchy")
        self.ctx.check(load().nk_mg_set_jacobian(self.handle, C.byref(prob), J.u.ptr), "nk_mg_set_jacobian")
        return self

    def vcycle(self, v: DeviceArray, z: DeviceArray | None = None) -> DeviceArray:
        """z = V-cycle(v) (nk_mg_apply, then a sync): the preconditioner by itself, without an operator J.
        z may alias v (`vcycle(v, z=v)`: in place)."""
        z = v.zero() if z is None else z
        self.ctx.check(load().nk_mg_apply(self.handle, z.ptr, v.ptr), "nk_mg_apply")
        self.ctx.sync()
        return z

    def vcycle_dot(self, v: DeviceArray, z: DeviceArray | None = None):
        """(z, <v, z>) with z = vcycle(v): the inner product is accumulated by the launch that writes z
        (nk_mg_apply_dot; fixed order, so two calls give the same bits).  What CG does with M = this object."""
        import ctypes as C

        z = v.zero() if z is None else z
        vz = C.c_double(0.0)
        self.ctx.check(load().nk_mg_apply_dot(self.handle, z.ptr, v.ptr, C.byref(vz)), "nk_mg_apply_dot")
        return z, vz.value

    @property
    def spd(self) -> bool:
        """The SPD form (nk_mg_set_spd): settable at any time, no set-up is redone."""
        import ctypes as C

        on = C.c_int32(0)
        self.ctx.check(load().nk_mg_get_spd(self.handle, C.byref(on)), "nk_mg_get_spd")
        return bool(on.value)

    @spd.setter
    def spd(self, on: bool):
        self.ctx.check(load().nk_mg_set_spd(self.handle, int(bool(on))), "nk_mg_set_spd")

    @property
    def levels(self) -> list:
        """Extents (x fastest) of the levels in use, finest first."""
        import ctypes as C

        ext, n = (C.c_int64 * (3 * 64))(), C.c_int32(0)
        self.ctx.check(load().nk_mg_level_extents(self.handle, ext, 64, C.byref(n)), "nk_mg_level_extents")
        return [tuple(int(ext[3 * l + a]) for a in range(self.grid.dim)) for l in range(min(n.value, 64))]

    def as_c(self):
        return self._c

    def free(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            load().nk_mg_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _mg_slab_check(ctx, grid, coarsening="full"):
    """distributed=True: what the slab-distributed hierarchy needs of the context and the grid (values every rank
    holds alike); NotImplementedError naming the reason otherwise"""
    nranks = getattr(ctx, "nranks", 1)
    if nranks <= 1:
        raise NotImplementedError("multigrid: distributed=True needs a context of several ranks (nranks == 1: leave it out)")
    pgrid = getattr(ctx, "pgrid", None)
    if grid.origin is not None or (pgrid is not None and pgrid[0] * pgrid[1] > 1):
        raise NotImplementedError("multigrid: distributed=True covers slabs (3D blocks are not implemented)")
    if grid.dim == 1:
        raise NotImplementedError("multigrid: distributed=True covers 2D and 3D grids (1D kinds are not distributed)")
    if coarsening != "full":
        raise NotImplementedError('multigrid: coarsening="semi" is not implemented with distributed=True')
    loc, glob = tuple(grid.shape_xyz), tuple(grid.global_xyz)
    if loc[:-1] != glob[:-1] or glob[-1] != nranks * loc[-1]:
        raise NotImplementedError("multigrid: distributed=True needs equal slabs of the slowest axis over the context's "
                                  f"{nranks} ranks (uneven slabs are not implemented): local {loc}, global {glob}")
    if loc[-1] % 2:
        raise NotImplementedError("multigrid: slabs of an odd number of planes cannot be coarsened")


def _mg_periodic_check(distributed, coarsening):
    """periodic=True: what it does not combine with (NotImplementedError, on the host)"""
    if distributed:
        raise NotImplementedError("multigrid: periodic=True is not implemented with distributed=True")
    if coarsening != "full":
        raise NotImplementedError('multigrid: coarsening="semi" is not implemented with periodic=True')


def _mg_problem(J, distributed=False, coarsening="full", periodic=False):
    """J's nk_problem if the multigrid preconditioner covers it; NotImplementedError naming the reason if not
    (checked on the host, before anything touches the device)."""
    from .problems import UserResidual

    if isinstance(J.f, UserResidual):
        raise NotImplementedError("multigrid: a user residual has no known stencil coefficients -- build the V-cycle "
                                  "with MultigridPreconditioner.from_coefficients(grid, k, s)")
    ctx, grid = J.u.ctx, J.u.grid
    if periodic:
        _mg_periodic_check(distributed, coarsening)
    if distributed:
        _mg_slab_check(ctx, grid, coarsening)
    elif getattr(ctx, "nranks", 1) != 1 or tuple(grid.shape_xyz) != tuple(grid.global_xyz):
        raise NotImplementedError("multigrid: one rank only (a distributed context / slab needs distributed=True)")
    prob = J.problem()
    if periodic:
        if prob.bc != _lib.NK_BC_PERIODIC:
            raise ValueError("multigrid: periodic=True on a bc_zero_ problem (leave the keyword out)")
    elif prob.bc != _lib.NK_BC_ZERO:
        raise NotImplementedError("multigrid: a periodic problem (bc_periodic_) needs the keyword periodic=True; "
                                  "the default hierarchy is bc_zero_ only")
    if distributed and prob.kind == _lib.NK_BRATU3D:
        raise NotImplementedError("multigrid: 3D Bratu runs on one rank (distributed=True is not implemented for it)")
    return prob


def _mg_coarsening(coarsening, threshold):
    """(coarsening, threshold) checked on the host: ValueError for an unknown name or a threshold outside (0, 1]"""
    if coarsening not in ("full", "semi"):
        raise ValueError(f'multigrid: coarsening must be "full" or "semi", not {coarsening!r}')
    threshold = float(threshold)
    if not 0.0 < threshold <= 1.0:
        raise ValueError(f"multigrid: threshold must lie in (0, 1], not {threshold!r}")
    return coarsening, threshold


def multigrid_plan(shape_xyz, max_levels: int = 0, *, coarsening: str = "full", h=None, k=None, threshold: float = 0.5,
                   nranks: int = 1, periodic: bool = False) -> list:
    """The level extents of a grid (host only, no GPU): [(nx[, ny[, nz]]), ...].  coarsening="full": nk_mg_plan.
    "semi": nk_mg_plan_semi with the spacings h (default 1 / (n + 1) per axis), the coefficients k per axis
    (default all ones) and the threshold (MultigridPreconditioner).  nranks > 1: the plan of the slab-distributed
    hierarchy (distributed=True; nk_mg_plan_slabs) -- shape_xyz is one rank's LOCAL extents (equal slabs), and so
    are the levels; NotImplementedError where no such hierarchy exists (an odd local slab extent, a 1D grid).
    periodic=True: the plan of a periodic grid (nk_mg_plan_periodic): an axis is halved while it is even and has at
    least 6 points; ValueError where a used axis has fewer than 3 points."""
    import ctypes as C

    coarsening, threshold = _mg_coarsening(coarsening, threshold)
    dim = len(shape_xyz)
    n = (C.c_int64 * 3)(*(list(shape_xyz) + [1, 1])[:3])
    ext = (C.c_int64 * (3 * 64))()
    nl = C.c_int32(0)
    if periodic:
        _mg_periodic_check(int(nranks) != 1, coarsening)
        if load().nk_mg_plan_periodic(n, int(max_levels), ext, 64, C.byref(nl)) != 0:
            raise ValueError(f"multigrid: no periodic plan for {tuple(shape_xyz)} (every used axis needs at least 3 points, "
                             "max_levels >= 0)")
        return [tuple(int(ext[3 * l + a]) for a in range(dim)) for l in range(min(nl.value, 64))]
    if int(nranks) != 1:
        if coarsening != "full":
            raise NotImplementedError('multigrid: coarsening="semi" is not implemented on slabs (nranks > 1)')
        if load().nk_mg_plan_slabs(n, int(nranks), int(max_levels), ext, 64, C.byref(nl)) != 0:
            raise NotImplementedError(f"multigrid: no slab plan for local extents {tuple(shape_xyz)} on {nranks} ranks (slabs "
                                      "of an odd number of planes cannot be coarsened; 2D and 3D grids, nranks >= 2)")
        return [tuple(int(ext[3 * l + a]) for a in range(dim)) for l in range(min(nl.value, 64))]
    if coarsening == "semi":
        hh = [float(x) for x in (h if h is not None else [1.0 / (m + 1) for m in shape_xyz])]
        kk = [float(x) for x in (k if k is not None else [1.0] * dim)]
        if len(hh) != dim or len(kk) != dim:
            raise ValueError("h, k: one value per axis")
        _lib.check(load().nk_mg_plan_semi(n, (C.c_double * 3)(*(hh + [1.0, 1.0])[:3]), (C.c_double * 3)(*(kk + [1.0, 1.0])[:3]),
                                          threshold, int(max_levels), ext, 64, C.byref(nl)), None, "nk_mg_plan_semi")
        return [tuple(int(ext[3 * l + a]) for a in range(dim)) for l in range(min(nl.value, 64))]
    _lib.check(load().nk_mg_plan(n, int(max_levels), ext, 64, C.byref(nl)), None, "nk_mg_plan")
    return [tuple(int(ext[3 * l + a]) for a in range(dim)) for l in range(min(nl.value, 64))]


class _MultigridFactory:
    """(J) -> MultigridPreconditioner with one hierarchy kept across calls: allocated for the first J, then
    only refreshed (s = λ exp(u) and the level diagonals) while the context, grid, spacings and residual kind
    stay; anything else builds a new hierarchy (and frees the old one)."""

    def __init__(self, opts):
        self.opts, self.key, self.mg = dict(opts), None, None

    def __call__(self, J):
        prob = _mg_problem(J, self.opts.get("distributed", False), self.opts.get("coarsening", "full"),
                           self.opts.get("periodic", False))
        key = (id(J.u.ctx), J.u.grid, prob.kind, prob.hx, prob.hy, prob.hz, prob.bc)  # (the options are the factory's own)
        if self.mg is None or self.key != key or self.mg.handle is None or self.mg.ctx is not J.u.ctx:
            self.free()
            self.key, self.mg = key, MultigridPreconditioner(J, **self.opts)
            return self.mg
        return self.mg.update(J)

    def free(self):
        if self.mg is not None:
            self.mg.free()
        self.key, self.mg = None, None


def multigrid(J=None, **opts):
    """N / M factory for newton_krylov_: `N=multigrid` (the defaults) or `N=multigrid(nu=3, ...)`.  The
    hierarchy is allocated once per Newton solve and reused by every step (as gmres_preconditioner reuses its
    workspace); each step refreshes s = λ exp(u) and the level diagonals from that step's u.  A factory made by
    `multigrid(...)` keeps its hierarchy for as long as it lives (`.free()` releases it); `N=multigrid` itself
    keeps nothing beyond the solve.  Called with an operator, `multigrid(J)` is MultigridPreconditioner(J).
    `M=multigrid(spd=True)` is the SPD form, CG's and MINRES's preconditioner (algo="cg" / "minres"); `N=multigrid(coarsening="semi")` the
    semicoarsened hierarchy for grids whose spacings differ between the axes (MultigridPreconditioner);
    `N=multigrid(distributed=True)` the hierarchy on equal slabs of a distributed context (every rank builds one);
    `N=multigrid(periodic=True)` the hierarchy of a periodic grid (heat residuals with bc_periodic_)."""
    if J is None:
        _mg_coarsening(opts.get("coarsening", "full"), opts.get("threshold", 0.5))
        return _MultigridFactory(opts)
    if opts:
        raise TypeError("multigrid(J, ...) with options: use MultigridPreconditioner(J, ...) or N=multigrid(...)")
    return MultigridPreconditioner(J)
