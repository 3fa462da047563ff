"""A batch of QPs as a differentiable torch operation: solve_qp(solver, Q=..., c=..., ...) -> x.

Forward: load_tensors, solve, the solutions.  Backward: the loss's gradient with respect to x as one cotangent row
per QP, the adjoint Newton solve at the converged iterate (J^T w = -g, ipmz_*_newton_adjoint_multi) and its
contraction with d r / d data (ipmz_batch_data_vjp): the implicit-function theorem on the Newton system, all on the
device.  Forward mode (solution_jvp, and solve_qp under torch.autograd.forward_ad): tangents of the data to the
residual rows (ipmz_batch_data_jvp), then the Newton solve of all rows from one factor (ipmz_*_newton_solve_multi).
Reverse mode for a block of cotangents per QP (solution_vjp, solution_jacobian): one adjoint solve of all rows from
one factor, then their contraction with d r / d data in one call (ipmz_batch_data_vjp_multi).
"""
import torch

from . import _BLOCKS, Batch, IpmzError, lib

_NAMES = tuple(b[0] for b in _BLOCKS)


def _even(k):
    return k + (k & 1)


class _SolveQP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, max_iter, strict, symmetrize, *blocks):
        # (after the data blocks: the warm start, an iterate per QP and its floor, then solve_all's skip_converged
        # and check_every, then -- only when asked for -- the barrier parameter of the centering with its tolerance
        # and iteration limit; no inputs of the derivative)
        blocks, warm = blocks[:len(_NAMES)], blocks[len(_NAMES):]
        skip_converged, check_every = warm[2:4] if len(warm) >= 4 else (False, 1)
        barrier, barrier_tol, barrier_max_iter = warm[4:7] if len(warm) >= 7 else (None, 1e-10, 30)
        ctx.extra = len(warm)
        given = {k: t.detach() for k, t in zip(_NAMES, blocks) if t is not None}
        solver.load_tensors(**given)
        if warm and warm[0] is not None:
            solver.set_state_tensor(warm[0].detach(), floor=warm[1], check=True)
        batch = lib.ipmz_batch_size(solver.h)
        if skip_converged and not solver.can_skip_converged():
            raise IpmzError("solve_qp: skip_converged=True, but this solver cannot skip converged QPs "
                            "(can_skip_converged() is False: a batch of more than one QP with N <= 1024 and inner "
                            "block 64 is needed)")
        if isinstance(solver, Batch):
            its, converged = solver.solve_all(max_iter, skip_converged=skip_converged, check_every=check_every)
        else:
            its, trace = solver.solve(max_iter)
            converged = int(solver.scalars()["converged"] == 1.0)
        if strict and converged != batch:
            raise IpmzError(f"solve_qp: {batch - converged} of {batch} QPs did not converge in {max_iter} iterations "
                            "(strict=True: the gradient is that of the solution map only at a converged solution)")
        if barrier is not None:
            its, centered = solver.center(barrier, barrier_tol, barrier_max_iter)
            if strict and centered != batch:
                raise IpmzError(f"solve_qp: {batch - centered} of {batch} QPs were not centered on the central path "
                                f"at barrier={barrier} to barrier_tol={barrier_tol} in {barrier_max_iter} iterations "
                                "(strict=True: the gradient is exact only at a centered iterate)")
        x = solver.solution_tensor().clone()
        ctx.solver, ctx.symmetrize = solver, symmetrize
        ctx.generation = solver._generation
        # an input given once for every QP (a 2-D matrix, a 1-D vector) receives the gradient summed over the batch
        ctx.shared = tuple(k for k, t in given.items() if t.dim() == (2 if k in ("Q", "A_ineq", "A_eq") else 1))
        ctx.shapes = {k: tuple(t.shape) for k, t in given.items()}
        return x

    @staticmethod
    def backward(ctx, grad_x):
        s = ctx.solver
        if s._generation != ctx.generation:
            raise IpmzError("solve_qp: the solver's iterate or data changed between forward and backward (a load, "
                            "step, solve or set_vars since); one forward / backward pair is in flight per solver")
        batch, L, n = lib.ipmz_batch_size(s.h), s.state_len, s.n
        ld = _even(L)
        # one cotangent row per QP in the layout of IPMZ_STATE_DAFF: grad_output in the x slot (x leads the Newton
        # order in every formulation), zeros elsewhere; the adjoint's Out in place
        G = torch.zeros((batch, ld), dtype=torch.float64, device=grad_x.device)
        G[:, :n] = grad_x
        s._order_torch_stream(torch)
        if isinstance(s, Batch) and batch > 1:
            s.newton_adjoint_all(G.data_ptr(), G.data_ptr(), 1, ld, ld, ld, ld)
        else:
            s.newton_adjoint(G.data_ptr(), G.data_ptr(), 1, ld, ld)
        wanted = [k for i, k in enumerate(_NAMES) if ctx.needs_input_grad[4 + i] and k in ctx.shapes]
        grads = s.data_grad_tensors(G, shared=[k for k in ctx.shared if k in wanted], symmetrize=ctx.symmetrize,
                                    only=wanted) if wanted else {}
        out = []
        for k in _NAMES:
            g = grads.get(k)
            if g is None and k in wanted:  # a block of dimension 0
                g = torch.zeros(ctx.shapes[k], dtype=torch.float64, device=grad_x.device)
            out.append(None if g is None else g.reshape(ctx.shapes[k]))
        return (None, None, None, None, *out, *([None] * ctx.extra))

    @staticmethod
    def jvp(ctx, _solver, _max_iter, _strict, _symmetrize, *tangents):
        # torch.autograd.forward_ad: one tangent per dual input (ntan = 1); the tangent of an input given once for
        # every QP is a shared tangent.  The generation check and strict are forward's and backward's
        s = ctx.solver
        if s._generation != ctx.generation:
            raise IpmzError("solve_qp: the solver's iterate or data changed between forward and jvp (a load, step, "
                            "solve or set_vars since); one forward / jvp pair is in flight per solver")
        batch = lib.ipmz_batch_size(s.h)
        given = {}
        for k, t in zip(_NAMES, tangents):
            if t is None or k not in ctx.shapes:
                continue
            t = t.detach().reshape(ctx.shapes[k])
            given[k] = t.unsqueeze(0 if k in ctx.shared else 1)
        if not given:
            return torch.zeros((batch, s.n), dtype=torch.float64, device=f"cuda:{s.ctx.device}")
        return solution_jvp(s, **given)[0][:, 0].clone()


def solution_jvp(solver, **tangents):
    """(dx, dz): the tangents of the solution and of the whole Newton state of every QP of `solver` (an Optimizer
    or a Batch) along tangents of its data, at the solver's current iterate.

    tangents: float64 CUDA tensors under load_tensors' names with a tangent dimension after the batch's, as
    Optimizer.data_jvp_tensors takes them: matrices (batch, ntan, rows, n) or (ntan, rows, n) for data given once
    for every QP, vectors (batch, ntan, len) or (ntan, len); missing names are zero tangents.  The chain is
    data tangents -> R = (d r / d data) D (ipmz_batch_data_jvp) -> the Newton solve of all ntan rows from one
    factor, in place (ipmz_*_newton_solve_multi): dz = -J^{-1} R.  Returns dx, the (batch, ntan, n) view of dz's
    leading entries (x leads the Newton order in every formulation), and dz, (batch, ntan, state_len).  The
    solver's iterate and generation counter do not move.

    What it is the derivative of depends on the iterate.  At an iterate centered on the central path
    (Optimizer.center(kappa), or solve_qp(barrier=kappa)) it is the exact derivative of data -> z(data; kappa), the
    point with r(z; mu = kappa) = 0, duals included, at any active set: kappa is a constant, J is nonsingular there
    and the map is smooth.  At the final iterate of a solve without centering the old caveat stands: it is the
    derivative of the solution map only at a converged, strictly complementary solution -- the implicit-function
    theorem on the Newton system at the current iterate with mu held constant -- and at an iterate that has not
    converged, or where a constraint is active with a zero multiplier, it is the derivative of nothing in
    particular."""
    s = solver
    batch, L = lib.ipmz_batch_size(s.h), s.state_len
    R = s.data_jvp_tensors(tangents)
    ntan, ld = R.shape[1], R.stride(1) if R.shape[1] > 1 else R.shape[2]
    if isinstance(s, Batch) and batch > 1:
        s.newton_solve_all(R.data_ptr(), R.data_ptr(), ntan, ld, ntan * ld, ld, ntan * ld)
    else:
        s.newton_solve(R.data_ptr(), R.data_ptr(), ntan, ld, ld)
    dz = R[:, :, :L]
    return dz[:, :, :s.n], dz


def solution_vjp(solver, G, *, shared=(), only=None, symmetrize=False):
    """(grads, W): cotangents of the solution of every QP of `solver` (an Optimizer or a Batch) pulled back to its
    data, ncot rows per QP from one factor, at the solver's current iterate: the reverse counterpart of
    solution_jvp.

    G: a float64 CUDA tensor, (batch, ncot, n) -- cotangents of x* -- or (batch, ncot, state_len) -- cotangents of
    the whole Newton state, duals included (the adjoint takes any g).  The chain is: G into an even-stride buffer
    -> the adjoint Newton solve of all ncot rows in place, J^T w = -g (ipmz_*_newton_adjoint_multi, nrhs = ncot)
    -> its contraction with d r / d data (ipmz_batch_data_vjp_multi).  Returns grads, Optimizer.
    data_grad_tensors_multi's dict -- (batch, ncot, ...) per QP, (ncot, ...) summed over the batch for the names in
    `shared`; only, symmetrize as there -- and W, the (batch, ncot, state_len) view of the residual cotangents.
    The solver's iterate and generation counter do not move.

    What it is the derivative of depends on the iterate.  At an iterate centered on the central path
    (Optimizer.center(kappa), or solve_qp(barrier=kappa)) it is the exact derivative of data -> z(data; kappa), the
    point with r(z; mu = kappa) = 0, duals included, at any active set: kappa is a constant, J is nonsingular there
    and the map is smooth.  At the final iterate of a solve without centering the old caveat stands: it is the
    derivative of the solution map only at a converged, strictly complementary solution -- the implicit-function
    theorem on the Newton system at the current iterate with mu held constant -- and at an iterate that has not
    converged, or where a constraint is active with a zero multiplier, it is the derivative of nothing in
    particular."""
    s = solver
    batch, L, n = lib.ipmz_batch_size(s.h), s.state_len, s.n
    if not isinstance(G, torch.Tensor) or G.dtype != torch.float64 or G.dim() != 3 or G.shape[0] != batch or \
            G.shape[2] not in (n, L):
        raise ValueError(f"G: a float64 ({batch}, ncot, {n}) or ({batch}, ncot, {L}) tensor is needed, got "
                         f"{getattr(G, 'dtype', type(G))} {tuple(getattr(G, 'shape', ()))}")
    s._on_device(G, "G")
    ncot, ld = G.shape[1], _even(L)
    buf = torch.zeros((batch, ncot, ld), dtype=torch.float64, device=G.device)
    buf[:, :, :G.shape[2]] = G
    if ncot:
        s._order_torch_stream(torch)
        if isinstance(s, Batch) and batch > 1:
            s.newton_adjoint_all(buf.data_ptr(), buf.data_ptr(), ncot, ld, ncot * ld, ld, ncot * ld)
        else:
            s.newton_adjoint(buf.data_ptr(), buf.data_ptr(), ncot, ld, ld)
    grads = s.data_grad_tensors_multi(buf, shared=shared, symmetrize=symmetrize, only=only)
    return grads, buf[:, :, :L]


def solution_jacobian(solver, *, shared=(), only=None):
    """(grads, W) of solution_vjp with G the n unit rows for every QP: grads[name][q, i] is d x_i* / d name of QP q
    (for the names in `shared`, grads[name][i] is the sum over the QPs), the whole reverse-mode Jacobian of the
    solution from one factor.  solution_vjp's note on the iterate holds: exact for data -> z(data; kappa) at an
    iterate centered on the central path (Optimizer.center), at any active set; otherwise only at a converged,
    strictly complementary iterate, mu held constant."""
    s = solver
    batch, n = lib.ipmz_batch_size(s.h), s.n
    G = torch.eye(n, dtype=torch.float64, device=f"cuda:{s.ctx.device}").expand(batch, n, n)
    return solution_vjp(s, G, shared=shared, only=only)


def solve_qp(solver, *, Q=None, c=None, l_x=None, u_x=None, A_ineq=None, l_A_ineq=None, u_A_ineq=None, A_eq=None,
             b_eq=None, max_iter=100, strict=True, symmetrize=False, warm_start=None, warm_floor=0.0,
             skip_converged=False, check_every=1, barrier=None, barrier_tol=1e-10, barrier_max_iter=30):
    """x* of every QP of `solver` (an Optimizer or a Batch), (batch, n), differentiable with respect to the data.

    The data are float64 CUDA tensors under load_tensors' names and rules: matrices (batch, rows, n) or (rows, n)
    given once for every QP, vectors (batch, len) or (len,); None keeps the block the solver holds (and has no
    gradient).  Forward: load_tensors, solve_all / solve (at most max_iter steps), the solutions.  Backward:
    the adjoint Newton solve at the final iterate, then ipmz_batch_data_vjp; an input given once for every QP
    receives the gradient summed over the batch, inputs that do not require grad are skipped.

    barrier=None (default): the gradient is that of the solution map only at a converged, strictly complementary
    solution: it is the implicit-function theorem on the Newton system at the final iterate with mu held constant,
    so at an iterate that has not converged, or where a constraint is active with a zero multiplier, it is the
    derivative of nothing in particular (a coordinate that sits on a bound gets gradient 0, a weakly active one
    whatever the ill-conditioned Newton system returns).  strict=True (default) raises IpmzError when any QP did
    not converge in max_iter steps.

    barrier=kappa > 0: after the same solve (and the same strict check) every QP is moved onto the central path at
    the fixed barrier parameter kappa, solver.center(kappa, barrier_tol, barrier_max_iter): x is then x(data; kappa)
    with r(z; mu = kappa) = 0, within O(kappa) of x*, and backward, jvp, solution_jvp, solution_vjp and
    solution_jacobian return the exact derivative of data -> z(data; kappa), duals included, at any active set --
    kappa is a constant of the problem, J is nonsingular there and the map is smooth, so a coordinate on a bound
    gets a gradient strictly between 0 and the unconstrained one.  strict=True also raises when a QP was not
    centered.  barrier_tol (|r(z; kappa)|inf <= barrier_tol) and barrier_max_iter are parameters; their defaults
    1e-10 and 30 come from a CPU prototype of the loop in numpy (2-6 iterations from a converged iterate on
    generated QPs at kappa 1e-2 .. 1e-6, 9-12 on a diagonal box QP with coordinates on a bound; include/ipmz.h at
    ipmz_batch_center); on the device 1024 QPs of n = 256 and one of n = 8192 needed at most 11, an iteration costing
    about one Newton step (DESIGN.md "Centering on the central path").  Not served: EQ_PENALTY, INEQ_SLACKS and what the adjoint
    solve refuses.  barrier=None is the path without the call, bit for bit.

    Q's entries are independent inputs: dL/dQ = w_x x^T, not symmetric.  symmetrize=True returns (gQ + gQ^T) / 2,
    the gradient for a caller who builds Q symmetric.  Formulations: those the adjoint solve serves (not
    EQ_SLACKED_SLACKS / EQ_NAIVE_SLACKS); INEQ_SLACKS does not converge (the reference's corrector defect).

    warm_start: None (the solve starts from build_environment's iterate), or a float64 CUDA tensor (batch,
    state_len), an iterate per QP in the order of state_tensor() -- typically the previous solve's: after
    load_tensors it is set with set_state_tensor(warm_start, floor=warm_floor, check=True) and the solve starts
    there.  It takes no gradient and is no differentiable input; backward and jvp read the final iterate as before.
    A converged iterate lies on the boundary -- of every complementary pair one side is near 0, and a Newton step
    from there is short -- so a warm start normally wants warm_floor > 0, which raises every slack and inequality
    multiplier below it.  How many iterations a warm start saves, and with which floor, is a measurement
    (the warm start's table), not a promise; the default warm_floor stays 0.0 until it is settled.

    skip_converged, check_every: handed to Batch.solve_all -- a converged QP then takes no part in the later steps
    and the host looks at the device every check_every steps; x* and every gradient keep their bits (backward and
    jvp read the final iterate, and their factor covers every QP).  skip_converged=True on a solver that cannot
    skip (can_skip_converged() is False) raises IpmzError.

    The solver keeps the iterate the backward pass reads: one forward / backward pair is in flight per solver, and
    backward raises IpmzError when a load, step, solve, set_vars or set_state_tensor has moved the solver since its
    forward."""
    given = dict(Q=Q, c=c, l_x=l_x, u_x=u_x, A_ineq=A_ineq, l_A_ineq=l_A_ineq, u_A_ineq=u_A_ineq, A_eq=A_eq, b_eq=b_eq)
    if warm_start is not None:
        warm_start = warm_start.detach()
    extra = () if barrier is None else (float(barrier), float(barrier_tol), int(barrier_max_iter))
    return _SolveQP.apply(solver, max_iter, strict, symmetrize, *[given[k] for k in _NAMES], warm_start, warm_floor,
                          skip_converged, check_every, *extra)
