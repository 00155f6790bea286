"""Float64 references of the Sinkhorn term differentiated THROUGH its L iterations (OptTrans(no_bp_P_L=False),
fi_ot_sinkhorn_backprop): the reverse recurrence restated in the kernel's order (forward with its iterates kept, the
sweep, the rank-2L sum M, then dC) and the autograd of the non-detached formula it must equal.  The formula itself is
tests/fp64_ref.py's (_ot_cost, _ot_plan); tests/test_ot_backprop_cpu.py holds the two to each other on the CPU,
tests/test_gpu_ot_backprop.py checks the kernel against them on the device."""
import torch

from fp64_ref import OT_EPS, _ot_cost, _ot_plan

# (S, D, L, mode): off and on the 8 x 8 register tile, D around the 16-column staging chunk, L = 1 (b_0 is a constant),
# the first chained step, the workload's 50
CPU_SHAPES = [(9, 3, 1, 0), (33, 17, 2, 1), (33, 17, 5, 0), (256, 1, 50, 0), (256, 1, 50, 1), (256, 16, 50, 1)]


def inputs(S, D, P=1, seed=0):
    """x, y [P,S,D] float64 on the CPU; D = 1 inputs ReLU'd as the workload's 1-D form (about half the samples 0)."""
    g = torch.Generator().manual_seed(1000 * S + 10 * D + seed)
    x = torch.randn(P, S, D, generator=g, dtype=torch.float64)
    y = torch.randn(P, S, D, generator=g, dtype=torch.float64)
    if D == 1:
        x, y = torch.relu(x), torch.relu(y)
    return x, y


def recurrence_dcost(C, eps_inv, L):
    """(loss, dC, P) of loss = sum (a_L K b_L^T) o C, K = exp(-eps_inv C), by the reverse recurrence:
         abar = G b_L, bbar = G^T a_L, G = K o C
         for l = L..1:  ubar = -bbar o b_l^2 / u;  abar += K ubar;  vbar = -abar o a_l^2 / u;  bbar = K^T vbar;  abar = 0
         M = sum_l a_l ubar_l^T + vbar_l b_{l-1}^T   (after the sweep, from the saved vectors)
         dC = P o (1 - eps_inv C) - eps_inv K o M."""
    C = C.detach()
    S = C.shape[0]
    K = torch.exp(-eps_inv * C)
    u = torch.full((S,), 1.0 / S, dtype=C.dtype, device=C.device)
    a_s, b_s = [], [u]
    b = u
    for _ in range(L):
        a = u / (K @ b + OT_EPS)
        b = u / (K.t() @ a + OT_EPS)
        a_s.append(a)
        b_s.append(b)
    P = a_s[-1][:, None] * K * b_s[-1][None, :]
    loss = (P * C).sum()
    G = K * C
    abar, bbar = G @ b_s[L], G.t() @ a_s[L - 1]
    ubars, vbars = [None] * L, [None] * L
    for l in range(L, 0, -1):
        ubar = -bbar * b_s[l] ** 2 / u
        abar = abar + K @ ubar
        vbar = -abar * a_s[l - 1] ** 2 / u
        bbar = K.t() @ vbar
        abar = torch.zeros_like(abar)
        ubars[l - 1], vbars[l - 1] = ubar, vbar
    M = torch.zeros_like(C)
    for l in range(1, L + 1):
        M += torch.outer(a_s[l - 1], ubars[l - 1]) + torch.outer(vbars[l - 1], b_s[l - 1])
    return loss, P * (1.0 - eps_inv * C) - eps_inv * K * M, P


def autograd_dcost(C, eps_inv, L):
    """d / dC of (_ot_plan(C) o C).sum() with the plan NOT detached."""
    Cg = C.detach().clone().requires_grad_(True)
    (_ot_plan(Cg, float(eps_inv), int(L)) * Cg).sum().backward()
    return Cg.grad


def cost(x, y, mode):
    return _ot_cost(x, y, mode)


def backprop_loss(x, y, eps_inv, L, form, detach=False):
    """The differentiable loss of OT_module.sinkhorn_loss(..., detach_plan=detach) on float64 x, y [P,S,D]."""
    mode = {"cosine": 0, "l2": 1}[form]
    out = []
    for p in range(x.shape[0]):
        C = _ot_cost(x[p], y[p], mode)
        plan = _ot_plan(C, float(eps_inv), int(L))
        out.append(((plan.detach() if detach else plan) * C).sum())
    return torch.stack(out)
