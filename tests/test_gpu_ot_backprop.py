"""GPU: the Sinkhorn term differentiated through its iterations -- fi_ot_sinkhorn_backprop (csrc/sinkhorn_bp.hip,
include/fi_ot.h), OT_module.sinkhorn_loss(detach_plan=False), OptTrans(no_bp_P_L=False) and DEV.OT_NO_BP_P_L -- against
float64 torch.autograd of the non-detached formula of tests/fp64_ref.py (tests/ot_backprop_ref.py; the reference's own
backward raises under modern torch, so there is no reference-run golden).  The bar is the project's for every
Sinkhorn term, 1e-4 of the largest element (REL of tests/test_gpu_loss_kernels.py): two orders above what a float32
evaluation of the recurrence reaches (<= 7.2e-7), three below the distance to the detached form (>= 0.15 on every case
here with more than one sample).  Write-only outputs and the workspace sit between NaN guard bands."""
import copy
import ctypes
import types

import pytest
import torch
import torch.nn as nn

import fp64_ref as R
import ot_backprop_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
REL = 1e-4
ZERO_GRAD = 1e-12          # of the largest parameter gradient (float64): below it a gradient is zero by construction
GUARD = 64
P = 3
SINKHORN_SHAPES = [(1, 1), (7, 15), (9, 16), (9, 17), (33, 15), (33, 33), (200, 1), (255, 16), (255, 17), (256, 1), (256, 16),
                   (256, 17)]                            # tests/test_gpu_loss_kernels.py's list


def _libs():
    from feature_intertwiner_amd import OT_module, _lib as M
    return M, M.load(), OT_module.load_ot()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(S, D, mode, seed=0):
    x, y = B.inputs(S, D, P=P, seed=seed)
    x, y = x.float().to(DEV), y.float().to(DEV)
    if mode == 2:
        x = x / (torch.norm(x, dim=2, keepdim=True) + 1e-20)
        y = y / (torch.norm(y, dim=2, keepdim=True) + 1e-20)
    return x.contiguous(), y.contiguous()


class _Run:
    """One call of the entry with loss, dcost and the workspace between NaN guard bands."""

    def __init__(self, x, y, L, mode, ws_floats=None, S=None, null_dcost=False):
        M, _, Lo = _libs()
        n, s, D = x.shape
        S = s if S is None else S
        self.n, self.S = n, s
        need = Lo.fi_ot_sinkhorn_backprop_workspace_bytes(n, s, max(L, 1)) // 4
        self.ws_floats = need if ws_floats is None else ws_floats
        self.loss_buf = torch.full((2 * GUARD + n,), NAN, device=DEV)
        self.dc_buf = torch.full((2 * GUARD + n * s * s,), NAN, device=DEV)
        self.ws_buf = torch.full((2 * GUARD + need,), NAN, device=DEV)
        self.loss = self.loss_buf[GUARD:GUARD + n]
        self.dcost = self.dc_buf[GUARD:GUARD + n * s * s]
        ws = self.ws_buf[GUARD:]
        self.status = Lo.fi_ot_sinkhorn_backprop(M.ptr(x), M.ptr(y), n, S, D, 1.0, L, mode, M.ptr(self.loss),
                                                 None if null_dcost else M.ptr(self.dcost), M.ptr(ws),
                                                 ctypes.c_size_t(self.ws_floats * 4), M.current_stream())
        torch.cuda.synchronize()

    def guards_intact(self):
        ok = True
        for buf, n in ((self.loss_buf, self.n), (self.dc_buf, self.n * self.S * self.S), (self.ws_buf, self.ws_floats)):
            ok = ok and bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())
        return ok

    def untouched(self):
        return all(bool(torch.isnan(b).all()) for b in (self.loss_buf, self.dc_buf, self.ws_buf))


def _forward_loss(x, y, L, mode, S=None):
    M, Lf, _ = _libs()
    n, s, D = x.shape
    loss = torch.full((n,), NAN, device=DEV)
    st = Lf.fi_sinkhorn_forward(M.ptr(x), M.ptr(y), n, s if S is None else S, D, 1.0, L, mode, M.ptr(loss), None, None,
                                None, M.current_stream())
    torch.cuda.synchronize()
    return st, loss


@pytest.mark.parametrize("S,Dm", SINKHORN_SHAPES)
def test_raw_entry_matches_fp64_autograd(S, Dm):
    """dcost of fi_ot_sinkhorn_backprop per problem within 1e-4 of max|dC_ref| for L in {1, 2, 50} and the three cost
    modes; loss bit-equal to fi_sinkhorn_forward's; guard bands intact.  In the float64 reference alone the
    differentiable gradient is at least 0.1 max|dC_ref| away from the plan (measured on the CPU: 0.15 .. 0.70, at L = 1
    too), so the detached form cannot pass.  S = 1 is the exception BY MATHEMATICS: one sample's plan is the constant 1
    whatever C is, so dC = P = 1 exactly, and that is what is asserted there."""
    for mode in (0, 1, 2):
        x, y = _inputs(S, Dm, mode)
        for iters in (1, 2, 50):
            run = _Run(x, y, iters, mode)
            assert run.status == 0
            assert run.guards_intact()
            assert bool(torch.isfinite(run.dcost).all()) and bool(torch.isfinite(run.loss).all())
            st, fl = _forward_loss(x, y, iters, mode)
            assert st == 0 and torch.equal(_bits(run.loss), _bits(fl)), (mode, iters)
            for p in range(P):
                C = R._ot_cost(x[p].double(), y[p].double(), mode)
                ref = B.autograd_dcost(C, 1.0, iters)
                plan = R._ot_plan(C, 1.0, iters)
                scale = float(ref.abs().max())
                got = run.dcost[p * S * S:(p + 1) * S * S].view(S, S).double()
                err = float((got - ref).abs().max()) / scale
                dist = float((ref - plan).abs().max()) / scale
                print("S=%d D=%d mode=%d L=%d p=%d: err %.3g of max|dC|, |dC - P| %.3g" % (S, Dm, mode, iters, p, err, dist))
                assert err <= REL, (mode, iters, p, err)
                if S == 1:
                    assert dist <= 1e-12 and abs(float(ref) - 1.0) <= 1e-12
                else:
                    assert dist >= 0.1, (mode, iters, p, dist)


@pytest.mark.parametrize("S,Dm,iters,mode", [(256, 1, 50, 0), (255, 17, 50, 1), (33, 33, 2, 2)])
def test_deterministic_and_independent_of_the_batch(S, Dm, iters, mode):
    x, y = _inputs(S, Dm, mode, seed=1)
    a, b = _Run(x, y, iters, mode), _Run(x, y, iters, mode)
    assert a.status == 0 and b.status == 0
    assert torch.equal(_bits(a.dcost), _bits(b.dcost)) and torch.equal(_bits(a.loss), _bits(b.loss))
    for p in range(P):
        one = _Run(x[p:p + 1].contiguous(), y[p:p + 1].contiguous(), iters, mode)
        assert one.status == 0 and one.guards_intact()
        assert torch.equal(_bits(one.dcost), _bits(a.dcost[p * S * S:(p + 1) * S * S])), p
        assert torch.equal(_bits(one.loss), _bits(a.loss[p:p + 1]))


def test_argument_checks():
    """The mistakes fi_sinkhorn_forward refuses get its status here; a short workspace is an invalid argument; nothing
    is launched (the NaN-filled outputs and workspace stay NaN)."""
    M, Lf, Lo = _libs()
    x, y = _inputs(9, 3, 1)
    for kw, fwd in ((dict(S=257), dict(S=257)), (dict(L=0), dict(L=0)), (dict(mode=3), dict(mode=3))):
        run = _Run(x, y, kw.get("L", 5), kw.get("mode", 1), S=kw.get("S"))
        st, _ = _forward_loss(x, y, fwd.get("L", 5), fwd.get("mode", 1), S=fwd.get("S"))
        assert run.status == st and st < 0, (kw, run.status, st)
        assert run.untouched(), kw
    assert _Run(x, y, 5, 1, S=257).status == -3 and _Run(x, y, 0, 1).status == -1          # FI_ERR_UNSUPPORTED / _INVALID_ARG
    # a null output: fi_sinkhorn_forward's status for a null loss
    st = Lf.fi_sinkhorn_forward(M.ptr(x), M.ptr(y), P, 9, 3, 1.0, 5, 1, None, None, None, None, M.current_stream())
    run = _Run(x, y, 5, 1, null_dcost=True)
    assert run.status == st == -1 and run.untouched()
    need = Lo.fi_ot_sinkhorn_backprop_workspace_bytes(P, 9, 5) // 4
    assert need == P * (21 * 256 + 256 * 256)
    run = _Run(x, y, 5, 1, ws_floats=need - 1)
    assert run.status == -1 and run.untouched()
    assert b"workspace" in Lf.fi_last_error()
    assert Lo.fi_ot_sinkhorn_backprop_workspace_bytes(P, 257, 5) == 0 and Lo.fi_ot_sinkhorn_backprop_workspace_bytes(P, 9, 0) == 0
    assert _Run(x, y, 5, 1).status == 0                                                        # and the good call runs


@pytest.mark.parametrize("form", ["cosine", "l2"])
@pytest.mark.parametrize("S,Dm,iters", [(256, 1, 50), (33, 17, 5), (9, 16, 1), (255, 17, 50)])
def test_input_gradients_match_fp64_autograd(S, Dm, iters, form):
    """sinkhorn_loss(detach_plan=False), weighted per problem, against float64 autograd of the non-detached formula:
    elementwise |got - ref| <= 1e-4 max|ref| over the kept rows.  Left out are exactly the rows whose float64 gradient
    is non-finite or >= 1e10 (the rule of test_sinkhorn_backward_matches_fp64_autograd): every one of them must be an
    exact-zero input row, and for l2 or D > 1 there must be none.  Cosine at D = 1: the kept rows' gradient is
    mathematically zero (x / |x| = sign x); finite everywhere and <= 1e-6 on the kept rows, as the existing test asserts.
    The loss has the bits of the detached form's."""
    from feature_intertwiner_amd.OT_module import sinkhorn_loss
    g = torch.Generator().manual_seed(S + Dm)
    x, y = torch.randn(P, S, Dm, generator=g), torch.randn(P, S, Dm, generator=g)
    if Dm == 1:
        x, y = torch.relu(x), torch.relu(y)
    w = torch.randn(P, generator=g)
    xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    loss = sinkhorn_loss(xg, yg, 1.0, iters, form, detach_plan=False)
    (loss * w.to(DEV)).sum().backward()
    detached = sinkhorn_loss(x.to(DEV).requires_grad_(True), y.to(DEV), 1.0, iters, form)
    assert torch.equal(_bits(loss.detach()), _bits(detached.detach()))
    with torch.no_grad():
        assert torch.equal(_bits(sinkhorn_loss(x.to(DEV), y.to(DEV), 1.0, iters, form, detach_plan=False)), _bits(loss.detach()))
    xd, yd = x.double().to(DEV).requires_grad_(True), y.double().to(DEV).requires_grad_(True)
    (B.backprop_loss(xd, yd, 1.0, iters, form) * w.double().to(DEV)).sum().backward()
    for name, got, ref, inp in (("x", xg.grad, xd.grad, x), ("y", yg.grad, yd.grad, y)):
        assert bool(torch.isfinite(got).all()), name
        out = (~torch.isfinite(ref) | (ref.abs() >= 1e10)).any(2)                   # [P,S] rows
        zero_rows = (inp == 0).all(2).to(DEV)
        assert not bool((out & ~zero_rows).any())
        if form == "l2" or Dm > 1:
            assert int(out.sum()) == 0
        keep = ~out
        gk, rk = got.double()[keep], ref[keep]
        scale = float(rk.abs().max())
        err = float((gk - rk).abs().max())
        print("%s S=%d D=%d L=%d %s: max|got - ref| %.3g, max|ref| %.3g, rows left out %d" % (
            form, S, Dm, iters, name, err, scale, int(out.sum())))
        if form == "cosine" and Dm == 1:
            assert int(out.sum()) > 0 and float(gk.abs().max()) <= 1e-6
        else:
            assert scale > 1e-4 and err <= REL * scale, (name, err, scale)


def test_second_derivative_raises():
    from feature_intertwiner_amd.OT_module import sinkhorn_loss
    x, y = _inputs(9, 3, 1)
    xg = x.clone().requires_grad_(True)
    loss = sinkhorn_loss(xg, y, 1.0, 2, "l2", detach_plan=False).sum()
    (gx,) = torch.autograd.grad(loss, xg, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


# ---- the module against itself in float64 torch ------------------------------------------------------------------------
def _cfg():
    return types.SimpleNamespace(DEV=types.SimpleNamespace(OT_ONE_DIM_FORM="conv"))


def _double_twin(m):
    """G_net and critic of an OptTrans as float64 torch.nn modules with the same weights."""
    def conv(layer):
        w = layer.weight
        if isinstance(layer, nn.ConvTranspose2d):
            t = nn.ConvTranspose2d(w.shape[0], w.shape[1], 3, padding=1, stride=layer.stride, output_padding=layer.output_padding)
        elif w.dim() == 3:
            t = nn.Conv1d(w.shape[1], w.shape[0], 3, padding=1, stride=1)
        else:
            t = nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1, stride=2)
        t.load_state_dict({"weight": w.detach().clone(), "bias": layer.bias.detach().clone()})
        return t

    def twin(seq):
        out = []
        for layer in seq:
            if isinstance(layer, nn.ReLU):
                out.append(nn.ReLU())
            elif isinstance(layer, nn.BatchNorm2d):
                out.append(copy.deepcopy(layer))
            else:
                out.append(conv(layer))
        return nn.Sequential(*out).double().to(DEV).train()
    return twin(m.G_net), twin(m.critic)


def _twin_loss(G, critic, x, y, eps_inv, L, form, detach):
    samples = lambda c: c.reshape(c.size(0), c.size(1), -1)          # bs, channels (samples), spatial (features)
    bs = x.size(0)
    cx, cy = samples(critic(G(x))), samples(critic(y))
    t = B.backprop_loss(torch.cat((cx, cx, cy), 0), torch.cat((cy, cx, cy), 0), eps_inv, L, form, detach=detach)
    return 2 * t[:bs] - t[bs:2 * bs] - t[2 * bs:]


@pytest.mark.parametrize("case", ["1d_64", "1d_1024", "2d_32", "1d_64_l2", "1d_1024_l2"])
def test_module_matches_its_float64_twin(case):
    """OptTrans(no_bp_P_L=False) against the same module in float64 torch (nn.Conv1d / Conv2d / ConvTranspose2d in
    double, same weights): loss to 1e-4 relative, every parameter's gradient to a relative L2 error of 1e-4; and, in
    float64 alone, the detached module's gradient is at least 1e-2 (relative L2) away for every parameter with a
    non-zero gradient.

    Conditions on the inputs, not on the code.  (1) The loss is the debiased 2 T(x, y) - T(x, x) - T(y, y): with x and y
    alike it is the residue of a cancellation (terms 0.7, loss 4e-3: the float32 terms, right to 1e-6, then leave it off
    by 1.1e-4 .. 1.4e-4, measured), so the 1-D cases feed a large x and a small y into a critic whose bias is shifted by
    0.05 -- the two sample sets then differ in their share of dead samples and the loss is 5 .. 50 % of a term.
    (2) In the 1-D COSINE form every sample has one feature, x / (|x| + 1e-20) = sign x does not move with x, and every
    parameter gradient is mathematically zero in either form (float64 leaves 1e-14; nothing is "1e-2 away" from
    nothing).  There the check is the one tests/test_gpu_loss_kernels.py makes for the input gradients of that form --
    finite, and no larger than what its 1e-6 per sample can add up to in the parameter -- and the 1-D module is held
    to the full bars with the l2 cost (1d_*_l2), where its gradient is not zero.  (3) A bias in front of a BatchNorm has
    a zero gradient by construction (1e-16 of the others in float64): the bar there is 1e-4 of the largest gradient."""
    from feature_intertwiner_amd.OT_module import OptTrans
    torch.manual_seed(11)
    g = torch.Generator().manual_seed(5)
    n = 2
    if case == "2d_32":
        m = OptTrans(_cfg(), ch_x=32, spatial_x=8, spatial_y=16, L=5, no_bp_P_L=False)
        x, y = torch.randn(n, 32, 8, 8, generator=g), torch.randn(n, 32, 16, 16, generator=g)
    else:
        ch = 64 if "_64" in case else 1024
        m = OptTrans(_cfg(), ch_x=ch, L=5 if ch == 64 else 50, C_form="l2" if case.endswith("l2") else "cosine",
                     no_bp_P_L=False)
        with torch.no_grad():
            m.critic[0].bias.add_(0.05)
        x, y = 3.0 * torch.relu(torch.randn(n, ch, 1, generator=g)), 0.01 * torch.relu(torch.randn(n, ch, 1, generator=g))
    zero_by_form = case in ("1d_64", "1d_1024")
    m = m.to(DEV).train()
    w = torch.rand(n, generator=g) + 0.5
    G, critic = _double_twin(m)
    x, y = x.to(DEV), y.to(DEV)
    loss = m(x, y)
    (loss * w.to(DEV)).sum().backward()
    got = {k: p.grad.double() for k, p in m.named_parameters()}
    names = [k for k, _ in m.named_parameters()]
    twin_params = [p for mod in (G, critic) for p in mod.parameters()]
    assert len(twin_params) == len(names)
    grads = {}
    for detach in (False, True):
        for p in twin_params:
            p.grad = None
        ref_loss = _twin_loss(G, critic, x.double(), y.double(), m.epsilon, m.L, m.C_form, detach)
        (ref_loss * w.double().to(DEV)).sum().backward()
        grads[detach] = [p.grad.clone() for p in twin_params]
        if not detach:
            rel = float(((loss.double() - ref_loss).abs() / ref_loss.abs()).max())
            print("%s: loss %s, float64 %s, relative error %.3g" % (case, loss.tolist(), ref_loss.detach().tolist(), rel))
            loss_rel = rel
    top = max(float(r.norm()) for r in grads[False])
    bad = []
    if zero_by_form:
        # |d loss / d critic output| <= 1e-6 * |w| per sample; a parameter's gradient element sums it over n samples
        # (critic) or over the 3 * ch / 4 critic weights of an input channel first (G_net), times the layer's input
        per_sample = 1e-6 * float(w.max())
        act = float(G(x.double()).abs().max())
        through = 3 * (x.size(1) // 4) * float(m.critic[0].weight.abs().max()) * per_sample
        bound = {"critic.0.weight": n * per_sample * act, "critic.0.bias": n * per_sample,
                 "G_net.0.weight": n * through * float(x.abs().max()), "G_net.0.bias": n * through}
        for k, ref in zip(names, grads[False]):
            big = float(got[k].abs().max())
            print("%s %s: float64 |gradient| %.3g (zero by the form), largest element computed %.3g, bound %.3g" % (
                case, k, float(ref.norm()), big, bound[k]))
            if not (float(ref.norm()) <= 1e-9 and bool(torch.isfinite(got[k]).all()) and big <= bound[k]):
                bad.append((k, big, bound[k]))
    for k, ref, det in zip(names, grads[False], grads[True]):
        if zero_by_form:
            break
        ref, det = ref.reshape(got[k].shape), det.reshape(got[k].shape)
        nrm = float(ref.norm())
        err = float((got[k] - ref).norm()) / max(nrm, 1e-300)
        away = float((det - ref).norm()) / max(nrm, 1e-300)
        print("%s %s: relative L2 error %.3g, |ref| %.3g (largest %.3g), |got| %.3g, detached form %.3g away" % (
            case, k, err, nrm, top, float(got[k].norm()), away))
        if nrm <= ZERO_GRAD * top:
            if float(got[k].norm()) > 1e-4 * top:
                bad.append((k, "zero gradient", float(got[k].norm())))
            continue
        if err > 1e-4:
            bad.append((k, "error", err))
        if away < 1e-2:
            bad.append((k, "detached form too close", away))
    assert not bad, bad
    assert loss_rel <= 1e-4, loss_rel


def test_config_switch_trains_with_the_differentiable_form():
    """DEV.OT_NO_BP_P_L = False on the smallest OT-on configuration: two train steps (the first fills the history
    buffer) run, the ot_loss.* gradients of the second are finite and differ from the default form's on the same
    weights, inputs and draws."""
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.synthetic import SyntheticProposals, synthetic_batch
    from feature_intertwiner_amd.workflow import set_optimizer, train_step
    grads = {}
    for flag in (True, False):
        torch.manual_seed(2000)
        cfg = make_config("resnet50", 256, 2, 64, dev_switch=True, loss_choice="ot", ot_L=5)
        if not flag:
            cfg.DEV.OT_NO_BP_P_L = False
        model = MaskRCNN(cfg).to(DEV)
        assert model.ot_loss.no_bp_P_L is flag
        opt = set_optimizer(model, cfg.TRAIN)
        batch = synthetic_batch(2, 256, device=DEV)
        model.external_proposals = SyntheticProposals(batch[2], 256)
        model.generator = torch.Generator(device=DEV).manual_seed(3)
        for _ in range(2):
            terms = train_step(model, opt, list(batch))
        torch.cuda.synchronize()
        assert all(torch.isfinite(v) for v in terms.values()), terms
        grads[flag] = {k: p.grad.detach().clone() for k, p in model.named_parameters()
                       if k.startswith("ot_loss.") and p.grad is not None}
        del model, opt
    assert sorted(grads[True]) == sorted(grads[False]) and len(grads[False]) == 4
    away = {}
    for k in grads[False]:
        assert bool(torch.isfinite(grads[False][k]).all()), k
        away[k] = float((grads[False][k] - grads[True][k]).norm() / grads[True][k].norm().clamp_min(1e-30))
    print("ot_loss gradients, differentiable vs detached form (relative L2):", away)
    assert max(away.values()) >= 1e-2, away
