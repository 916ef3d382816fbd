"""Shared pieces of the FusedSGD tests (no test in here): the float64 restatement of the update that
csrc/optim.hip's header states, and the tolerance of an fp32 run against it.

    g   = g * min(max_norm / (norm + 1e-6), 1)        (clip_grad_norm_; the clipped g stays in .grad)
    d   = g + wd * p                                  (wd != 0; added after the clip, before momentum)
    buf = momentum * buf + d                          (momentum != 0; buf starts at zero: first-step buf = d)
    p   = p - lr * (buf if momentum != 0 else d)

test_optim_surface.py pins ``_SgdRef`` to torch.optim.SGD + clip_grad_norm_ in float64 on the CPU;
test_gpu_sgd.py compares the kernels with it.
"""
import torch


def F32(v):
    """The value a float argument of the C ABI holds."""
    return float(torch.tensor(v, dtype=torch.float32).item())


class _SgdRef:
    """The four lines above in float64 on one flat vector.  Hyper-parameters are used as given (pass F32
    values to mirror the C ABI) and ``lr`` may be changed between steps.  ``P`` and ``B`` follow the
    trajectory: max |p| (the start included) and max |buf| (max |d| when momentum is 0)."""

    def __init__(self, p, lr, momentum=0.0, wd=0.0, max_norm=None):
        self.p = p.detach().double().cpu().reshape(-1).clone()
        self.buf = torch.zeros_like(self.p) if momentum else None
        self.lr, self.momentum, self.wd, self.max_norm = lr, momentum, wd, max_norm
        self.P = self.p.abs().max().item()
        self.B = 0.0
        self.steps = 0

    def step(self, g):
        """g: the gradient.  Returns (the pre-clip norm, the clipped gradient) as clip_grad_norm_ leaves them."""
        g = g.detach().double().cpu().reshape(-1)
        norm = g.norm().item()
        if self.max_norm:
            g = g * min(self.max_norm / (norm + 1e-6), 1.0)
        d = g + self.wd * self.p if self.wd else g
        if self.momentum:
            self.buf = self.momentum * self.buf + d
            d = self.buf
        self.p = self.p - self.lr * d
        self.P = max(self.P, self.p.abs().max().item())
        self.B = max(self.B, d.abs().max().item())
        self.steps += 1
        return norm, g

    def tol(self, lr=None):
        """Bound on |p_fp32 - p| after the steps taken so far (``lr``: the largest rate used, default the
        current one):

            steps * [2^-23 P + lr B (2^-23 / (1 - momentum) + 2e-5 * clipped)]

        two fp32 roundings per step in p (half an ulp of P each), two per step in buf, which the
        recurrence accumulates geometrically (1 / (1 - momentum)), and, when clipping, the clip
        coefficient's error: twice the 1e-5 relative bound the project holds the fp32 norm to
        (test_gpu_optim.py)."""
        lr = self.lr if lr is None else lr
        return self.steps * 2.0 ** -23 * self.P + lr * self.buf_tol()

    def buf_tol(self):
        """Bound on |buf_fp32 - buf|: the second term of ``tol`` without the learning rate."""
        return self.steps * self.B * (2.0 ** -23 / (1.0 - self.momentum) + (2e-5 if self.max_norm else 0.0))
