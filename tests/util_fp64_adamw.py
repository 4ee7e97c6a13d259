"""AdamW (decoupled weight decay, optional AMSGrad) restated in float64, one function per stage, as plain torch code without a
project import: what ``test_adamw_ref_cpu.py`` ties to ``torch.optim.AdamW`` on double parameters and what
``test_gpu_adamw_fp64.py`` holds every route of ``dp.FlatAdamW`` to, stage by stage.

    m' = beta1 m + (1 - beta1) g          v' = beta2 v + (1 - beta2) g^2          vmax' = max(vmax, v')
    p' = p (1 - lr wd)  -  lr / (1 - beta1^step) * m' / (sqrt(d) / sqrt(1 - beta2^step) + eps),   d = vmax' (AMSGrad) or v'

``step`` is the count of the TENSOR the element belongs to (``Bookkeeper``): ``torch.optim.AdamW`` keeps one per parameter
tensor, advanced only on the steps where the tensor has a gradient."""
import torch as th

U32 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)

# gradient magnitudes of the GPU cases: every class at both signs, exact zeros among them.  1e-6 stands beside the five classes
# of the case list so that BOTH values of eps the cases use (1e-8, 1e-6) have a class whose sqrt(v') / sqrt(bc2) is comparable
# to eps (``near_eps``); nothing goes below 1e-12, so g^2 and v stay normal fp32 numbers
MAGNITUDES = (0.0, 1e-12, 1e-8, 1e-6, 1e-4, 1.0, 1e3)


def moments(m, v, vmax, g, beta1, beta2):
    """(m', v', vmax') of one step; ``vmax`` None: no AMSGrad, vmax' is None."""
    m, v, g = m.double(), v.double(), g.double()
    m2 = beta1 * m + (1.0 - beta1) * g
    v2 = beta2 * v + (1.0 - beta2) * g * g
    return m2, v2, None if vmax is None else th.maximum(vmax.double(), v2)


def update(p, m, d, lr, beta1, beta2, eps, weight_decay, step):
    """p' from the moments AFTER the step (``d``: vmax' with AMSGrad, else v').  ``step``: a number, or a tensor of one count
    per element (>= 1)."""
    step = th.as_tensor(step, dtype=th.float64)
    bc1 = 1.0 - th.pow(th.tensor(beta1, dtype=th.float64), step)
    bc2 = 1.0 - th.pow(th.tensor(beta2, dtype=th.float64), step)
    denom = d.double().sqrt() / bc2.sqrt() + eps
    return p.double() * (1.0 - lr * weight_decay) - (lr / bc1) * (m.double() / denom)


class Bookkeeper:
    """Host-side step counts of P parameter tensors, kept as ``torch.optim.AdamW`` keeps them: a tensor's count advances only
    on a step where it has a gradient, a vetoed step advances nothing.  ``shared=True``: the documented behaviour of a flat
    buffer WITHOUT per-tensor counts (more than 1024 tensors, or hand-set live runs): one count for the buffer, advanced by
    every step that is not vetoed; a live tensor is updated at that count.  Never reads a device.

    Beside the counts it keeps what the guarded routes keep in their veto word: [flags since the last step (0 after a step),
    every flag ever raised, was the last step dropped, steps dropped so far]."""

    def __init__(self, P, shared=False, start=0):
        self.P, self.shared = int(P), bool(shared)
        self.steps = [int(start)] * self.P
        self.taken = int(start)               # optimizer steps that were not vetoed
        self.word = [0, 0, 0, 0]

    def advance(self, live=None, flags=None, mask=0):
        """One optimizer step.  ``live``: indices of the tensors with a gradient (None: all); ``flags``: the veto word's
        flags before the step (None: no veto word).  Returns a list of P counts: the step count each tensor is updated at,
        0 for a tensor that is left alone."""
        if flags is not None:
            drop = (int(flags) & int(mask)) != 0
            self.word = [0, self.word[1] | int(flags), int(drop), self.word[3] + int(drop)]
            if drop:
                return [0] * self.P
        self.taken += 1
        live = set(range(self.P) if live is None else live)
        out = []
        for s in range(self.P):
            if s not in live:
                out.append(0)
            elif self.shared:
                out.append(self.taken)
            else:
                self.steps[s] += 1
                out.append(self.steps[s])
        return out


def grad_classes(n, seed):
    """Class (index into ``MAGNITUDES``) of each of n elements: cyclic from a seed-dependent start, so that a tensor of a few
    elements still mixes several classes and every class occurs once n >= 7.  Fixed over the steps of a case."""
    return (th.arange(n, dtype=th.int64) + int(seed)) % len(MAGNITUDES)


def gradient(n, seed, it, spike=False):
    """fp32 gradient [n] of step ``it``: class magnitude x a factor in [0.5, 1.5) x a random sign (x 10 at a spike)."""
    gen = th.Generator().manual_seed(1000003 * int(seed) + 7919 * int(it) + 11)
    mag = th.tensor(MAGNITUDES, dtype=th.float64)[grad_classes(n, seed)]
    fac = 0.5 + th.rand(n, generator=gen, dtype=th.float64)
    sign = th.randint(0, 2, (n,), generator=gen).double() * 2.0 - 1.0
    return (mag * fac * sign * (10.0 if spike else 1.0)).float()


def parameter(n, seed):
    """fp32 start values [n]: standard normal, every third scaled by 1e-3 and every third an exact zero -- beside a parameter
    of magnitude 1 the update (about lr) is under a thousandth of the value and its error hides below the parameter's own
    rounding; at zero the update is all there is."""
    gen = th.Generator().manual_seed(2000003 * int(seed) + 5)
    scale = th.tensor([1.0, 1e-3, 0.0], dtype=th.float64)[(th.arange(n) + int(seed)) % 3]
    return (th.randn(n, generator=gen, dtype=th.float64) * scale).float()


def near_eps(g, classes, magnitude, eps, beta2):
    """Of a step-1 gradient ``g`` with the element classes ``classes``: min and max, over the elements of the class of
    ``magnitude``, of  (sqrt(v') / sqrt(bc2)) / eps.  Where that is of order 1, moving eps inside the bias correction changes
    the element's update by a factor of order 1 / sqrt(bc2)."""
    _, v2, _ = moments(th.zeros_like(g), th.zeros_like(g), None, g, 0.0, beta2)
    r = (v2.sqrt() / (1.0 - beta2) ** 0.5)[classes == MAGNITUDES.index(magnitude)] / eps
    return float(r.min()), float(r.max())
