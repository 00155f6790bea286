"""What the Sinkhorn term costs when it is differentiated through its iterations (OptTrans(no_bp_P_L=False)).

Workload: the headline's 240 problems, S = 256, D = 1, L = 50 (cosine on normalised, ReLU'd rows).  In ONE process,
interleaved round by round, each timed with a HIP event pair around the call and reported as the median over the rounds:
  backprop   fi_ot_sinkhorn_backprop (loss + d loss / d C, one launch)
  forward    fi_sinkhorn_forward with a plan: what the detached form costs
  tensor     the batched tensor formulation of the same gradient: torch.bmm over the 240 problems with autograd, fp32,
             forward + backward to d loss / d C -- the only other way to get it
and the agreement of `backprop` with `tensor` on the timed inputs.  It has no profiling id: the events are the timer.

    python scripts/sinkhorn_backprop_probe.py [--rounds 30] [--out profiles/sinkhorn_backprop_probe.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, S, D, L = 240, 256, 1, 50
OT_EPS = 1e-20


def tensor_dcost(C, iters):
    """d / dC of sum (a_L K b_L^T) o C, all problems at once, fp32 autograd through the 2 L batched mat-vecs."""
    Cg = C.detach().clone().requires_grad_(True)
    K = torch.exp(-Cg)
    u = torch.full((C.shape[0], C.shape[1], 1), 1.0 / C.shape[1], device=C.device)
    b = u
    for _ in range(iters):
        a = u / (torch.bmm(K, b) + OT_EPS)
        b = u / (torch.bmm(K.transpose(1, 2), a) + OT_EPS)
    ((a * K * b.transpose(1, 2)) * Cg).sum().backward()
    return Cg.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sinkhorn_backprop_probe.txt"))
    args = ap.parse_args()
    from feature_intertwiner_amd import OT_module, _lib as M
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    Lf, Lo = M.load(), OT_module.load_ot()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(2000)
    x = torch.relu(torch.randn(P, S, D, generator=g)).to(dev)
    y = torch.relu(torch.randn(P, S, D, generator=g)).to(dev)
    xn = (x / (torch.norm(x, dim=2, keepdim=True) + OT_EPS)).contiguous()
    yn = (y / (torch.norm(y, dim=2, keepdim=True) + OT_EPS)).contiguous()
    C = (1.0 - torch.bmm(xn, yn.transpose(1, 2))).contiguous()
    loss_b, loss_f = torch.empty(P, device=dev), torch.empty(P, device=dev)
    dcost, plan = torch.empty(P, S, S, device=dev), torch.empty(P, S, S, device=dev)
    nbytes = Lo.fi_ot_sinkhorn_backprop_workspace_bytes(P, S, L)
    ws = torch.empty(nbytes // 4, device=dev)
    st = M.current_stream()

    def backprop():
        M.check(Lo.fi_ot_sinkhorn_backprop(M.ptr(xn), M.ptr(yn), P, S, D, 1.0, L, 2, M.ptr(loss_b), M.ptr(dcost), M.ptr(ws),
                                           ctypes.c_size_t(nbytes), st), "fi_ot_sinkhorn_backprop")

    def forward():
        M.check(Lf.fi_sinkhorn_forward(M.ptr(xn), M.ptr(yn), P, S, D, 1.0, L, 2, M.ptr(loss_f), M.ptr(plan), None, None, st),
                "fi_sinkhorn_forward")

    ref = {}

    def tensor():
        ref["dC"] = tensor_dcost(C, L)

    runs = (("backprop", backprop), ("forward", forward), ("tensor", tensor))
    for _ in range(3):                                    # warm-up: code objects, the allocator, rocBLAS's choice
        for _, fn in runs:
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in runs}
    for _ in range(args.rounds):
        for k, fn in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    scale = ref["dC"].abs().amax((1, 2))
    err = float(((dcost - ref["dC"]).abs().amax((1, 2)) / scale).max())
    lines = ["sinkhorn backprop probe: %d problems, S = %d, D = %d, L = %d, %d interleaved rounds, HIP events, median (min .. max) us"
             % (P, S, D, L, args.rounds)]
    for k, _ in runs:
        lines.append("%-9s %9.1f  (%.1f .. %.1f)" % (k, med[k], min(times[k]), max(times[k])))
    lines.append("backprop / forward = %.2f    tensor / backprop = %.2f" % (med["backprop"] / med["forward"],
                                                                           med["tensor"] / med["backprop"]))
    lines.append("workspace %.1f MiB; loss bit-equal to the forward's: %s; max |dC - tensor dC| / max|dC| per problem = %.3g"
                 % (nbytes / 2 ** 20, bool(torch.equal(loss_b.view(torch.int32), loss_f.view(torch.int32))), err))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
